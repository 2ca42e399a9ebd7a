// lnerf_hashgrid_sorted.hip -- d_table of lnerf_hashgrid_grad under LNERF_HASHGRID_REPRODUCIBLE
// (include/lnerf.h "Multiresolution hash grid"): every entry's terms are brought together by a stable
// sort and summed in float64 in an order that is a function of the inputs alone. No float atomics, no
// dependence on launch geometry, arrival order or timing. One level at a time, so the scratch is
// proportional to R and not to R * levels:
//
//  hg_keys_kernel   one thread per row: the level's eight entry indices (the keys), the contribution
//                   ids c = 8 r + k in ascending order (the values) and the float64 factors
//                   (double)scale * weight_k(r), all indexed by c
//  rocprim::radix_sort_pairs on ceil(log2 E_l) bits: stable, so each entry's ids stay ascending
//  hg_sum_kernel    one thread per sorted position. A segment (the run of one key) belongs to the wave
//                   that holds its head. Every lane forms the term of its own position and parks it in
//                   LDS; the head lane of a segment of fewer than kLongMin terms then sums the segment
//                   alone, from LDS while it is inside the wave's 64 positions and by gathering past
//                   them. A longer segment is summed by the whole wave: each lane takes one run of
//                   kRun positions, the partials are added in lane order.
//
// The order, whichever path a segment takes (include/lnerf.h states it): with the entry's terms
// t_0 .. t_{n-1} in ascending c, partial_q = ((+0 + t_{8q}) + t_{8q+1}) + ... over at most kRun = 8
// terms, sum = ((+0 + partial_0) + partial_1) + ...; a term is (scale weight_k) * d_encoded, two
// float64 products, never rounded to float32. Built with -ffp-contract=off.
//
// Every index is in bounds by construction: keys are below E_l (lnerf_hashgrid_cell.h: clamp first,
// hash after), ids are below 8 R, sorted positions are compared with N = 8 R before every access.
#include <cstring>   // (before rocprim: its texture_cache_iterator.hpp uses memset)

#include <rocprim/rocprim.hpp>

#include "lnerf_hashgrid.h"
#include "lnerf_hashgrid_cell.h"

namespace lnerf {

namespace {

constexpr int kThreads = 256;
constexpr unsigned kRun = 8;          // positions per partial sum: part of the contract
constexpr unsigned kLongMin = 128;    // terms from which the whole wave sums a segment (speed only)
constexpr unsigned kNoKey = 0xffffffffu;   // no entry has it: keys are below 2^24

// ---- 1. keys ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) hg_keys_kernel(HgParams g, int l, const float* __restrict__ points,
                                                           long long R, const float* __restrict__ scale,
                                                           unsigned* __restrict__ keys, unsigned* __restrict__ ids,
                                                           double* __restrict__ factor) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const HgLevel lv = g.lv[l];
    const HgCell c = hg_cell(g, lv.res, points + (size_t)r * 3);
    const double sc = scale ? (double)*scale : 1.0;
    unsigned key[8];
    double w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        key[k] = hg_index(c, k, lv.res, lv.dense, g.mask);
        w[k] = sc * hg_weight(c, k);
    }
    const unsigned c0 = (unsigned)r * 8u;   // R <= 2^28 (lnerf_api.cpp)
    uint4* __restrict__ ko = reinterpret_cast<uint4*>(keys + c0);
    uint4* __restrict__ io = reinterpret_cast<uint4*>(ids + c0);
    double2* __restrict__ wo = reinterpret_cast<double2*>(factor + c0);
    ko[0] = make_uint4(key[0], key[1], key[2], key[3]);
    ko[1] = make_uint4(key[4], key[5], key[6], key[7]);
    io[0] = make_uint4(c0, c0 + 1, c0 + 2, c0 + 3);
    io[1] = make_uint4(c0 + 4, c0 + 5, c0 + 6, c0 + 7);
#pragma unroll
    for (int q = 0; q < 4; ++q) wo[q] = make_double2(w[2 * q], w[2 * q + 1]);
}

// ---- 3. segmented sum -----------------------------------------------------------------------------
// The term of contribution c at level l: (scale weight_k) * d_encoded[r][l F + f]
template <int F>
__device__ __forceinline__ void hg_term(unsigned c, const double* __restrict__ factor,
                                        const float* __restrict__ d_encoded, int levels, int l, double (&t)[F]) {
    const double w = factor[c];
    const float* __restrict__ de = d_encoded + ((size_t)(c >> 3) * levels + l) * F;
#pragma unroll
    for (int f = 0; f < F; ++f) t[f] = w * (double)de[f];
}

// One d_table row: (float)sum, or what the row holds plus that (one float32 add), as one access of
// 4 F bytes up to 16 (lnerf_api.cpp checked the alignment)
template <int F, bool ACC>
__device__ __forceinline__ void hg_store_row(float* __restrict__ row, const double (&sum)[F]) {
    float v[F];
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = (float)sum[f];
    if constexpr (F == 1) {
        row[0] = ACC ? row[0] + v[0] : v[0];
    } else if constexpr (F == 2) {
        float2* p = reinterpret_cast<float2*>(row);
        if constexpr (ACC) {
            const float2 h = *p;
            *p = make_float2(h.x + v[0], h.y + v[1]);
        } else {
            *p = make_float2(v[0], v[1]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            float4* p = reinterpret_cast<float4*>(row + 4 * q);
            if constexpr (ACC) {
                const float4 h = *p;
                *p = make_float4(h.x + v[4 * q], h.y + v[4 * q + 1], h.z + v[4 * q + 2], h.w + v[4 * q + 3]);
            } else {
                *p = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            }
        }
    }
}

template <int F, bool ACC>
__global__ void __launch_bounds__(kThreads) hg_sum_kernel(const unsigned* __restrict__ ks,
                                                          const unsigned* __restrict__ cs,
                                                          const double* __restrict__ factor, unsigned N,
                                                          const float* __restrict__ d_encoded, int levels, int l,
                                                          float* __restrict__ base) {
    __shared__ double term_lds[kThreads * F];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned j = blockIdx.x * (unsigned)kThreads + threadIdx.x;   // < 2^31 + 256
    const unsigned tile0 = j - lane, tile_end = tile0 + 64u;
    double* __restrict__ wave_lds = term_lds + (size_t)(threadIdx.x - lane) * F;

    const bool valid = j < N;
    const unsigned key = valid ? ks[j] : kNoKey;
    const unsigned prev = (valid && j > 0) ? ks[j - 1] : kNoKey;
    const bool head = valid && prev != key;
    const unsigned long long heads = __ballot(head);

    // where the segment that leaves the wave's positions ends (wave-uniform): the keys are sorted, so
    // the next 64 positions decide it unless the segment covers them all; then a binary search does
    unsigned tail_end = N;
    if (tile_end < N) {
        const unsigned last_key = __shfl(key, 63, 64);
        const unsigned pj = tile_end + lane;
        const unsigned kn = pj < N ? ks[pj] : kNoKey;
        const unsigned long long diff = __ballot(kn != last_key);
        if (diff) {
            tail_end = tile_end + (unsigned)(__ffsll((long long)diff) - 1);
        } else {   // every one of pj < N held last_key, so tile_end + 64 <= N
            unsigned lo = tile_end + 64u, hi = N;
            while (lo < hi) {
                const unsigned mid = lo + (hi - lo) / 2u;
                if (ks[mid] == last_key) lo = mid + 1u; else hi = mid;
            }
            tail_end = lo;
        }
    }
    const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const unsigned end = above ? j + (unsigned)__ffsll((long long)above) : tail_end;
    const unsigned n = head ? end - j : 0u;
    const bool is_long = head && n >= kLongMin;
    const bool is_short = head && !is_long;

    // every lane's own term, parked in LDS for the head lanes
    if (__ballot(is_short) != 0ull && valid) {
        double t[F];
        hg_term<F>(cs[j], factor, d_encoded, levels, l, t);
#pragma unroll
        for (int f = 0; f < F; ++f) wave_lds[lane * F + f] = t[f];
    }
    __syncthreads();

    if (is_short) {
        double sum[F], part[F];
#pragma unroll
        for (int f = 0; f < F; ++f) sum[f] = part[f] = 0.0;
        for (unsigned p = 0; p < n; ++p) {
            const unsigned pos = j + p;
            double t[F];
            if (pos < tile_end) {
#pragma unroll
                for (int f = 0; f < F; ++f) t[f] = wave_lds[(pos - tile0) * F + f];
            } else {
                hg_term<F>(cs[pos], factor, d_encoded, levels, l, t);
            }
#pragma unroll
            for (int f = 0; f < F; ++f) part[f] += t[f];
            if ((p & (kRun - 1u)) == kRun - 1u) {
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    sum[f] += part[f];
                    part[f] = 0.0;
                }
            }
        }
        if (n & (kRun - 1u)) {
#pragma unroll
            for (int f = 0; f < F; ++f) sum[f] += part[f];
        }
        hg_store_row<F, ACC>(base + (size_t)key * F, sum);
    }

    // the long segments whose heads this wave holds, one after the other, all lanes on each
    unsigned long long longs = __ballot(is_long);
    while (longs) {
        const int h = __ffsll((long long)longs) - 1;
        longs &= longs - 1ull;
        const unsigned s = tile0 + (unsigned)h;
        const unsigned nn = __shfl(n, h, 64);
        const unsigned kk = __shfl(key, h, 64);
        double sum[F];
#pragma unroll
        for (int f = 0; f < F; ++f) sum[f] = 0.0;
        for (unsigned b = 0; b < nn; b += 64u * kRun) {
            const unsigned p0 = b + kRun * lane;
            double part[F];
#pragma unroll
            for (int f = 0; f < F; ++f) part[f] = 0.0;
            if (p0 < nn) {
                const unsigned cnt = nn - p0 < kRun ? nn - p0 : kRun;
                for (unsigned q = 0; q < cnt; ++q) {
                    double t[F];
                    hg_term<F>(cs[s + p0 + q], factor, d_encoded, levels, l, t);
#pragma unroll
                    for (int f = 0; f < F; ++f) part[f] += t[f];
                }
            }
            const unsigned left = (nn - b + kRun - 1u) / kRun;
            const int runs = (int)(left < 64u ? left : 64u);
            for (int i = 0; i < runs; ++i) {
#pragma unroll
                for (int f = 0; f < F; ++f) sum[f] += __shfl(part[f], i, 64);
            }
        }
        if (lane == 0u) hg_store_row<F, ACC>(base + (size_t)kk * F, sum);
    }
}

unsigned row_blocks(long long R) { return (unsigned)((R + kThreads - 1) / kThreads); }

int level_bits(const HgParams& g, int l) {
    const long long entries = g.lv[l].dense ? (long long)g.lv[l].res * g.lv[l].res * g.lv[l].res : (long long)g.mask + 1;
    int bits = 1;
    while ((1ll << bits) < entries) ++bits;
    return bits;
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// the carve of the scratch: keys and ids twice (the sort's double buffers), the factors, the sort's own
struct Carve {
    size_t keys[2], ids[2], factor, sort, sort_bytes, total;
};

hipError_t carve(const HgParams& g, long long R, hipStream_t s, Carve& c) {
    const size_t N = (size_t)R * 8;
    size_t sort_bytes = 0;
    for (int l = 0; l < g.levels; ++l) {
        rocprim::double_buffer<unsigned> k(nullptr, nullptr), v(nullptr, nullptr);
        size_t need = 0;
        const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, k, v, N, 0u, (unsigned)level_bits(g, l), s);
        if (e != hipSuccess) return e;
        sort_bytes = need > sort_bytes ? need : sort_bytes;
    }
    size_t at = 0;
    for (int i = 0; i < 2; ++i) {
        c.keys[i] = at;
        at += align256(N * sizeof(unsigned));
        c.ids[i] = at;
        at += align256(N * sizeof(unsigned));
    }
    c.factor = at;
    at += align256(N * sizeof(double));
    c.sort = at;
    c.sort_bytes = sort_bytes;
    c.total = at + align256(sort_bytes);
    return hipSuccess;
}

}  // namespace

#define HG_SUM_DISPATCH(F_, ACC_, CALL)                                   \
    switch (F_) {                                                         \
        case 1: if (ACC_) { constexpr int F = 1; constexpr bool A = true; CALL; } else { constexpr int F = 1; constexpr bool A = false; CALL; } break; \
        case 2: if (ACC_) { constexpr int F = 2; constexpr bool A = true; CALL; } else { constexpr int F = 2; constexpr bool A = false; CALL; } break; \
        case 4: if (ACC_) { constexpr int F = 4; constexpr bool A = true; CALL; } else { constexpr int F = 4; constexpr bool A = false; CALL; } break; \
        default: if (ACC_) { constexpr int F = 8; constexpr bool A = true; CALL; } else { constexpr int F = 8; constexpr bool A = false; CALL; } break; \
    }

hipError_t k_hashgrid_sorted_scratch_bytes(const HgParams& g, long long R, hipStream_t s, size_t* bytes) {
    Carve c;
    const hipError_t e = carve(g, R, s, c);
    if (e == hipSuccess) *bytes = c.total;
    return e;
}

hipError_t k_hashgrid_grad_table_sorted(const HgParams& g, const float* points, long long R, const float* d_encoded,
                                        const float* scale, bool accumulate, float* d_table, void* scratch,
                                        hipStream_t s) {
    Carve c;
    hipError_t e = carve(g, R, s, c);
    if (e != hipSuccess) return e;
    char* p = static_cast<char*>(scratch);
    const unsigned N = (unsigned)(R * 8);   // R <= 2^28
    double* factor = reinterpret_cast<double*>(p + c.factor);
    for (int l = 0; l < g.levels; ++l) {
        rocprim::double_buffer<unsigned> keys(reinterpret_cast<unsigned*>(p + c.keys[0]),
                                              reinterpret_cast<unsigned*>(p + c.keys[1]));
        rocprim::double_buffer<unsigned> ids(reinterpret_cast<unsigned*>(p + c.ids[0]),
                                             reinterpret_cast<unsigned*>(p + c.ids[1]));
        hg_keys_kernel<<<row_blocks(R), kThreads, 0, s>>>(g, l, points, R, scale, keys.current(), ids.current(), factor);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t sort_bytes = c.sort_bytes;
        e = rocprim::radix_sort_pairs(p + c.sort, sort_bytes, keys, ids, (size_t)N, 0u, (unsigned)level_bits(g, l), s);
        if (e != hipSuccess) return e;
        float* base = d_table + (size_t)g.lv[l].offset * g.features;
        const unsigned blocks = (unsigned)(((size_t)N + kThreads - 1) / kThreads);
        HG_SUM_DISPATCH(g.features, accumulate,
                        (hg_sum_kernel<F, A><<<blocks, kThreads, 0, s>>>(keys.current(), ids.current(), factor, N,
                                                                         d_encoded, g.levels, l, base)));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace lnerf
