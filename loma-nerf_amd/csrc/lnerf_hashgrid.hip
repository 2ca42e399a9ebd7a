// lnerf_hashgrid.hip -- the multiresolution hash-grid encoding (include/lnerf.h "Multiresolution hash
// grid"): a learned scene representation between the sample points and the MLP. An extension: the
// reference's only encoder is pos_encoding.py.
//
//  hg_encode_kernel       points (R, 3), table -> encoded (R, levels * F): trilinear gather per level
//  hg_grad_table_kernel   d_encoded -> d_table: the scatter-add of the same eight corners per level
//  hg_grad_points_kernel  d_encoded, table -> d_points (R, 3)
//
// Cell arithmetic is float64 (the project's rule for input producers); encoded and d_points are
// fixed-order float64 sums rounded once, so repeated calls give the same bits. d_table is summed with
// float32 atomic adds here: the one output of the library whose last bits depend on arrival order
// (its ordered float64 form, LNERF_HASHGRID_REPRODUCIBLE, is lnerf_hashgrid_sorted.hip). The cell
// arithmetic is lnerf_hashgrid_cell.h, shared with that file. Built with -ffp-contract=off like
// lnerf_sampling.hip. No context, no workspace: free functions on a stream.
//
// Every table index is below the level's entry count by construction: the coordinate is clamped to
// the box first (a NaN becomes 0), the cell i_c is at most res - 2, a dense index is then below
// res^3 and a hashed one is masked to T - 1; lnerf_api.cpp has checked that the level owns that many
// entries.
#include "lnerf_hashgrid.h"
#include "lnerf_hashgrid_cell.h"

namespace lnerf {

namespace {

constexpr int kThreads = 256;

// One table row of F floats, as one 4 F-byte load up to 16 bytes (the callers checked the alignment)
template <int F>
__device__ __forceinline__ void hg_load_row(const float* __restrict__ row, float (&t)[F]) {
    if constexpr (F == 1) {
        t[0] = row[0];
    } else if constexpr (F == 2) {
        const float2 v = *reinterpret_cast<const float2*>(row);
        t[0] = v.x;
        t[1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(row + 4 * q);
            t[4 * q] = v.x;
            t[4 * q + 1] = v.y;
            t[4 * q + 2] = v.z;
            t[4 * q + 3] = v.w;
        }
    }
}

// ---- 1. forward ---------------------------------------------------------------------------------
// One thread per (row, level); the grid is level-major (blockIdx.y = level), so the workgroups in
// flight together gather from one level's table.
template <int F>
__global__ void __launch_bounds__(kThreads) hg_encode_kernel(HgParams g, const float* __restrict__ table,
                                                             const float* __restrict__ points, long long R,
                                                             float* __restrict__ encoded) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const int l = blockIdx.y;
    const HgLevel lv = g.lv[l];
    const HgCell c = hg_cell(g, lv.res, points + (size_t)r * 3);
    const float* __restrict__ base = table + (size_t)lv.offset * F;
    double acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float t[F];
        hg_load_row<F>(base + (size_t)hg_index(c, k, lv.res, lv.dense, g.mask) * F, t);
        const double w = hg_weight(c, k);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] += w * (double)t[f];
    }
    float* __restrict__ out = encoded + ((size_t)r * g.levels + l) * F;
#pragma unroll
    for (int f = 0; f < F; ++f) out[f] = (float)acc[f];
}

// ---- 2. d_table ---------------------------------------------------------------------------------
// d_table[entry][f] += (float)(scale w_k dE[r][l F + f]) over every row and corner that maps to the
// entry. One thread per (row, level), blockIdx.y = level; lanes are consecutive rows, i.e. consecutive
// samples of a ray, which share cells at the coarse levels. Two paths, chosen per level on the host:
//
//  LDS path (lv.lds_blocks > 0: a dense level of at most kHgLdsFloats values that receives at least
//  as many rows as it has entries): lds_blocks workgroups each sum a strided share of the rows into a
//  copy of the level in LDS (ds_add_f32) and flush it once, 256 contiguous bytes per wave-instruction
//  -- the shape global float atomics run at full rate in -- skipping the zeros.
//
//  merge path (every other level): per corner, a run of adjacent lanes with the same entry index is
//  summed into its first lane by a segmented suffix sum over lane shuffles, and only run heads issue
//  the atomic. At the fine, hashed levels every lane is a head and the wave skips the shuffles: what
//  is left there is the plain per-corner atomicAdd (global_atomic_add_f32, no compare-and-swap loop).
template <int F>
__global__ void __launch_bounds__(kThreads) hg_grad_table_kernel(HgParams g, const float* __restrict__ points,
                                                                 long long R, const float* __restrict__ d_encoded,
                                                                 const float* __restrict__ scale,
                                                                 float* __restrict__ d_table) {
    __shared__ float acc_lds[kHgLdsFloats];
    const int l = blockIdx.y;
    const HgLevel lv = g.lv[l];
    const double sc = scale ? (double)*scale : 1.0;
    float* __restrict__ base = d_table + (size_t)lv.offset * F;

    if (lv.lds_blocks > 0) {
        if ((int)blockIdx.x >= lv.lds_blocks) return;
        const int n = lv.res * lv.res * lv.res * F;   // <= kHgLdsFloats (host)
        for (int i = threadIdx.x; i < n; i += kThreads) acc_lds[i] = 0.0f;
        __syncthreads();
        const long long stride = (long long)lv.lds_blocks * kThreads;
        for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < R; r += stride) {
            const HgCell c = hg_cell(g, lv.res, points + (size_t)r * 3);
            const float* __restrict__ de = d_encoded + ((size_t)r * g.levels + l) * F;
            double d[F];
#pragma unroll
            for (int f = 0; f < F; ++f) d[f] = (double)de[f];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned idx = hg_index(c, k, lv.res, 1, g.mask);   // < res^3
                const double w = sc * hg_weight(c, k);
#pragma unroll
                for (int f = 0; f < F; ++f) atomicAdd(&acc_lds[idx * F + f], (float)(w * d[f]));
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const float v = acc_lds[i];
            if (v != 0.0f) atomicAdd(base + i, v);   // (a NaN compares unequal: it is flushed)
        }
        return;
    }

    const int lane = threadIdx.x & 63;
    const long long r_raw = (long long)blockIdx.x * kThreads + threadIdx.x;
    const bool valid = r_raw < R;
    const size_t r = (size_t)(valid ? r_raw : R - 1);   // a lane past the end recomputes the last row, adds nothing
    const HgCell c = hg_cell(g, lv.res, points + r * 3);
    const float* __restrict__ de = d_encoded + (r * g.levels + l) * F;
    double d[F];
#pragma unroll
    for (int f = 0; f < F; ++f) d[f] = (double)de[f];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // lanes past the end carry an index no entry has, so they end the last row's run
        const unsigned idx = valid ? hg_index(c, k, lv.res, lv.dense, g.mask) : 0xffffffffu;
        const double w = sc * hg_weight(c, k);
        float v[F];
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = (float)(w * d[f]);
        const unsigned prev = __shfl_up(idx, 1, 64);
        const bool head = lane == 0 || prev != idx;
        const unsigned long long heads = __ballot(head);
        if (heads != ~0ull) {   // wave-uniform: some run is longer than one lane
            // my run ends before the next head above me
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int run_end = above ? lane + __ffsll(above) : 64;
            for (int s = 1; s < 64; s <<= 1) {
                const bool take = lane + s < run_end;
                if (!__any(take)) break;   // wave-uniform: no run reaches this far
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const float o = __shfl_down(v[f], s, 64);
                    if (take) v[f] += o;
                }
            }
        }
        if (valid && head) {
#pragma unroll
            for (int f = 0; f < F; ++f) atomicAdd(base + (size_t)idx * F + f, v[f]);
        }
    }
}

// ---- 3. d_points --------------------------------------------------------------------------------
// d_points[r][a] = (float)(scale sum_l ((sum_f dE[l F + f] (sum_k dw_k/dpos_a table_k[f])) (res_l - 1) / ext_a)),
// dw_k/dpos_x = +- wy_k wz_k (+ where corner k has its x bit set), likewise y and z; exactly 0 for a
// coordinate the clamp moved or a NaN. One thread per row, levels, features and corners in order.
template <int F>
__global__ void __launch_bounds__(kThreads) hg_grad_points_kernel(HgParams g, const float* __restrict__ table,
                                                                  const float* __restrict__ points, long long R,
                                                                  const float* __restrict__ d_encoded,
                                                                  const float* __restrict__ scale,
                                                                  float* __restrict__ d_points) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const float* __restrict__ p3 = points + (size_t)r * 3;
    double acc[3] = {0.0, 0.0, 0.0};
    bool live[3] = {false, false, false};
    for (int l = 0; l < g.levels; ++l) {
        const HgLevel lv = g.lv[l];
        const HgCell c = hg_cell(g, lv.res, p3);
        const float* __restrict__ base = table + (size_t)lv.offset * F;
        const float* __restrict__ de = d_encoded + ((size_t)r * g.levels + l) * F;
        double dw[3][F];   // sum_k dw_k/dpos_a table_k[f]
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int f = 0; f < F; ++f) dw[a][f] = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t[F];
            hg_load_row<F>(base + (size_t)hg_index(c, k, lv.res, lv.dense, g.mask) * F, t);
            const double wx = (k & 1) ? c.w[0] : 1.0 - c.w[0];
            const double wy = (k & 2) ? c.w[1] : 1.0 - c.w[1];
            const double wz = (k & 4) ? c.w[2] : 1.0 - c.w[2];
            const double gx = (k & 1) ? wy * wz : -(wy * wz);
            const double gy = (k & 2) ? wx * wz : -(wx * wz);
            const double gz = (k & 4) ? wx * wy : -(wx * wy);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const double tf = (double)t[f];
                dw[0][f] += gx * tf;
                dw[1][f] += gy * tf;
                dw[2][f] += gz * tf;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double s = 0.0;
#pragma unroll
            for (int f = 0; f < F; ++f) s += (double)de[f] * dw[a][f];
            acc[a] += s * (double)(lv.res - 1) / g.ext[a];
            live[a] = c.live[a];   // the same at every level
        }
    }
    const double sc = scale ? (double)*scale : 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) d_points[(size_t)r * 3 + a] = live[a] ? (float)(sc * acc[a]) : 0.0f;
}

unsigned row_blocks(long long R) { return (unsigned)((R + kThreads - 1) / kThreads); }

}  // namespace

#define HG_DISPATCH_F(F_, CALL)          \
    switch (F_) {                        \
        case 1: { constexpr int F = 1; CALL; } break; \
        case 2: { constexpr int F = 2; CALL; } break; \
        case 4: { constexpr int F = 4; CALL; } break; \
        default: { constexpr int F = 8; CALL; } break; \
    }

void k_hashgrid_encode(const HgParams& g, const float* table, const float* points, long long R, float* encoded,
                       hipStream_t s) {
    const dim3 grid(row_blocks(R), (unsigned)g.levels);
    HG_DISPATCH_F(g.features, (hg_encode_kernel<F><<<grid, kThreads, 0, s>>>(g, table, points, R, encoded)));
}

void k_hashgrid_grad_table(HgParams g, const float* points, long long R, const float* d_encoded, const float* scale,
                           float* d_table, hipStream_t s) {
    for (int l = 0; l < g.levels; ++l) {
        HgLevel& lv = g.lv[l];
        lv.lds_blocks = 0;
        if (!lv.dense) continue;
        const long long entries = (long long)lv.res * lv.res * lv.res;
        if (entries * g.features > kHgLdsFloats || R < entries) continue;
        // each workgroup flushes the whole level once: give it at least as many rows as the level
        // has entries (and 2048), so that the flush stays a fraction of the adds it replaces
        const long long per_block = entries > 2048 ? entries : 2048;
        const long long blocks = (R + per_block - 1) / per_block;
        lv.lds_blocks = (int)(blocks < 1 ? 1 : blocks > row_blocks(R) ? row_blocks(R) : blocks);
    }
    const dim3 grid(row_blocks(R), (unsigned)g.levels);
    HG_DISPATCH_F(g.features,
                  (hg_grad_table_kernel<F><<<grid, kThreads, 0, s>>>(g, points, R, d_encoded, scale, d_table)));
}

void k_hashgrid_grad_points(const HgParams& g, const float* table, const float* points, long long R,
                            const float* d_encoded, const float* scale, float* d_points, hipStream_t s) {
    HG_DISPATCH_F(g.features, (hg_grad_points_kernel<F><<<row_blocks(R), kThreads, 0, s>>>(g, table, points, R,
                                                                                           d_encoded, scale, d_points)));
}

}  // namespace lnerf
