// lnerf_occgrid.hip -- the occupancy grid: a coarse grid of res^3 cells over a box that keeps a
// decayed running maximum of sigma per cell, its threshold packed into a bitfield, and the sampler
// that marches rays over the bitfield and spreads the S samples over the occupied steps alone.
// Extensions: the reference samples linspace(near, far, S) only (train_nerf.py:289-306).
//
//  occ_cell_points_kernel  cells (n), u (n, 3) -> points (n, 3) inside the cells
//  occ_decay_kernel        density *= decay
//  occ_max_kernel          density[cell_i] = max(density[cell_i], sigma_i), an integer atomic maximum
//  occ_sum_kernel          stage 1 of the mean: float64 partial sums of density, fixed order
//  occ_mean_kernel         stage 2: the mean, the threshold thr, the zeroed population count
//  occ_pack_kernel         bit c = density[c] > thr: 64 cells per wave by ballot, two 32-bit stores;
//                          the population count, one integer atomic add per workgroup
//  occ_sample_kernel       rays, bits -> sample_t (n, S), dists (n, S), n_occ (n): one wave per ray
//
// The project's rule for input producers: float64 or integer arithmetic, one rounding to float32 at
// the store, every sum in a fixed order, so repeated calls give the same bits (the two atomics here
// are integer ones: a maximum and a count, exact in any order). Built with -ffp-contract=off like
// lnerf_sampling.hip. No context, no workspace: free functions on a stream.
#include <cfloat>

#include "lnerf_internal.h"
#include "lnerf_occgrid.h"

namespace lnerf {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPasses = 16;      // 1024 steps / 64 lanes
constexpr int kMaxParts = 1024;     // stage-1 partial sums of the mean
constexpr int kPackSpan = 8;        // 256-cell groups a workgroup of the pack kernel takes

// u clamped to [0, 1], NaN taken as 0 (a NaN fails the first comparison)
__device__ __forceinline__ double unit_clamp(float u) { return u > 0.0f ? (u < 1.0f ? (double)u : 1.0) : 0.0; }

// ---- 1. points inside cells -------------------------------------------------------------------
// p_c = (float)(lo_c + (g_c + u_c) / res * (hi_c - lo_c)); an index outside the grid gives the box
// centre (float)(lo_c + 0.5 (hi_c - lo_c)). One thread per cell of the list.
__global__ void __launch_bounds__(kThreads) occ_cell_points_kernel(OccParams g, const int* __restrict__ cells,
                                                                   long long n, const float* __restrict__ u,
                                                                   float* __restrict__ points) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long c = cells ? (long long)cells[i] : i;
    const bool inside = c >= 0 && c < g.cells;
    const int ci = inside ? (int)c : 0;
    const int gi[3] = {ci & (g.res - 1), (ci >> g.shift) & (g.res - 1), ci >> (2 * g.shift)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double uc = u ? unit_clamp(u[(size_t)i * 3 + a]) : 0.5;
        const double w = inside ? ((double)gi[a] + uc) / (double)g.res : 0.5;
        points[(size_t)i * 3 + a] = (float)(g.lo[a] + w * g.ext[a]);
    }
}

// ---- 2. the decayed running maximum -----------------------------------------------------------
__global__ void __launch_bounds__(kThreads) occ_decay_kernel(long long cells, float decay, float* __restrict__ density) {
    const long long c = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (c < cells) density[c] = density[c] * decay;
}

// A non-negative float's bits order as the float does, so the maximum is an integer atomicMax: exact
// in any order. A NaN or a value <= 0 is ignored (both fail s > 0), +inf counts as FLT_MAX.
__global__ void __launch_bounds__(kThreads) occ_max_kernel(long long cells, const int* __restrict__ idx, long long n,
                                                           const float* __restrict__ sigma, int stride,
                                                           float* __restrict__ density) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long c = idx ? (long long)idx[i] : i;
    if (c < 0 || c >= cells) return;
    const float s = sigma[(size_t)i * (size_t)stride];
    if (!(s > 0.0f)) return;
    atomicMax(reinterpret_cast<int*>(density) + c, __float_as_int(s < FLT_MAX ? s : FLT_MAX));
}

// ---- 3. the threshold -------------------------------------------------------------------------
// Stage 1: workgroup b sums cells [b per, (b + 1) per): thread t adds t, t + 256, ... in order, then
// a fixed tree over the 256 partials in LDS.
__global__ void __launch_bounds__(kThreads) occ_sum_kernel(long long cells, long long per,
                                                           const float* __restrict__ density,
                                                           double* __restrict__ part) {
    __shared__ double red[kThreads];
    const long long c0 = (long long)blockIdx.x * per;
    const long long c1 = c0 + per < cells ? c0 + per : cells;
    double acc = 0.0;
    for (long long c = c0 + threadIdx.x; c < c1; c += kThreads) acc += (double)density[c];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int d = kThreads >> 1; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// Stage 2, one wave: lane l adds parts l, l + 64, ... in order, then a fixed tree of lane shuffles.
// Writes the mean, thr (to the scratch slot the pack kernel reads) and zeroes the population count.
__global__ void __launch_bounds__(64) occ_mean_kernel(const double* __restrict__ part, int parts, long long cells,
                                                      float threshold, int use_mean, double* __restrict__ thr,
                                                      double* __restrict__ mean, long long* __restrict__ occupied) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (int i = lane; i < parts; i += 64) acc += part[i];
    for (int d = 32; d > 0; d >>= 1) acc = acc + __shfl_down(acc, d, 64);
    if (lane == 0) {
        const double m = acc / (double)cells;
        if (mean) *mean = m;
        *thr = use_mean && m < (double)threshold ? m : (double)threshold;
        if (occupied) *occupied = 0;
    }
}

// One thread per cell, kPackSpan cells of a workgroup's own in turn; res^3 is a multiple of 64, so a
// wave is wholly inside the grid or wholly past it. The population count is summed per workgroup (the
// waves' counts through LDS) and leaves as ONE integer atomic add: 32 768 per-wave atomics on the one
// address took 0.4 ms at res 128.
__global__ void __launch_bounds__(kThreads) occ_pack_kernel(long long cells, const float* __restrict__ density,
                                                            const double* __restrict__ thr,
                                                            unsigned* __restrict__ bits,
                                                            long long* __restrict__ occupied) {
    __shared__ int wave_count[kThreads >> 6];
    const double t = *thr;
    int count = 0;
#pragma unroll
    for (int it = 0; it < kPackSpan; ++it) {
        const long long c = ((long long)blockIdx.x * kPackSpan + it) * kThreads + threadIdx.x;
        if (c < cells) {
            const unsigned long long m = __ballot((double)density[c] > t);
            count += __popcll(m);
            if (bits && (threadIdx.x & 63) == 0) {
                bits[2 * (c >> 6)] = (unsigned)m;
                bits[2 * (c >> 6) + 1] = (unsigned)(m >> 32);
            }
        }
    }
    if (!occupied) return;
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < (kThreads >> 6); ++w) total += wave_count[w];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(occupied), (unsigned long long)total);
    }
}

// ---- 4. the sampler ---------------------------------------------------------------------------
struct OccSampleArgs {
    OccParams g;
    const unsigned* bits;
    const float* rays;       // (n, 6)
    int n, S, steps;
    float near_t, far_t;
    const float* u;          // (n, S) or NULL: 0.5
    int last_opaque;
    float* sample_t;         // (n, S) or NULL
    float* dists;            // (n, S) or NULL
    int* n_occ;              // (n) or NULL
};

// One wave per ray, four rays per workgroup. Pass p: lane l tests step 64 p + l at its midpoint and
// the ballot is the pass's mask; the 16 masks and their running population counts are wave-uniform
// (every loop over them is unrolled, so they stay in registers; passes past M / 64 hold 0). Lane l
// then takes samples l, l + 64, ...: sample j wants the k-th occupied step, k from integer counts
// and u alone; its pass is the last whose running count is <= k, and inside the pass the k-th set
// bit of the mask is found by six popcount halvings. Trip counts depend on M and S only; a wave
// past the last ray recomputes the last ray and stores nothing. No LDS, no barrier.
__global__ void __launch_bounds__(kThreads) occ_sample_kernel(OccSampleArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long ray_raw = (long long)blockIdx.x * (kThreads >> 6) + wv;
    const bool live = ray_raw < a.n;
    const size_t ray = (size_t)(live ? ray_raw : a.n - 1);
    const int M = a.steps, S = a.S, passes = M >> 6;
    const double near_d = (double)a.near_t;
    const double h = ((double)a.far_t - near_d) / (double)M;
    double o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = (double)a.rays[ray * 6 + c];
        d[c] = (double)a.rays[ray * 6 + 3 + c];
    }

    unsigned long long mask[kMaxPasses];
    int before[kMaxPasses + 1];       // before[p]: occupied steps in passes 0..p-1
    before[0] = 0;
#pragma unroll
    for (int p = 0; p < kMaxPasses; ++p) {
        unsigned long long m = 0;
        if (p < passes) {
            const int i = 64 * p + lane;
            const double t = near_d + ((double)i + 0.5) * h;
            bool inside = true;
            int cell = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double w = ((o[c] + d[c] * t) - a.g.lo[c]) / a.g.ext[c];
                const bool ok = w >= 0.0 && w < 1.0;     // a NaN fails
                inside = inside && ok;
                const int gc = min((int)(ok ? w * (double)a.g.res : 0.0), a.g.res - 1);
                cell |= gc << (c * a.g.shift);
            }
            // cell is inside the grid whatever the ray holds (each g_c is 0..res-1)
            const unsigned word = a.bits[cell >> 5];
            m = __ballot(inside && ((word >> (cell & 31)) & 1u));
        }
        mask[p] = m;
        before[p + 1] = before[p] + __popcll(m);
    }
    const int N = before[kMaxPasses];
    if (N == 0) {
        // no occupied step: sample as if every step were (n_occ still reports 0)
#pragma unroll
        for (int p = 0; p < kMaxPasses; ++p) {
            mask[p] = p < passes ? ~0ull : 0ull;
            before[p + 1] = min(64 * (p + 1), M);
        }
    }
    const int Np = N == 0 ? M : N;
    if (live && a.n_occ && lane == 0) a.n_occ[ray] = N;

    const float share = (float)((double)Np * h / (double)S);
    for (int j = lane; j < S; j += 64) {
        const double uj = a.u ? unit_clamp(a.u[ray * S + j]) : 0.5;
        const double q = ((double)j + uj) * (double)Np / (double)S;
        const long long kq = (long long)q;               // 0 <= q <= N'
        const int k = (int)(kq < (long long)(Np - 1) ? kq : (long long)(Np - 1));
        const double f = q - (double)k;
        unsigned long long m = mask[0];
        int pass = 0, base = 0;
#pragma unroll
        for (int p = 1; p < kMaxPasses; ++p)
            if (before[p] <= k) {
                m = mask[p];
                base = before[p];
                pass = p;
            }
        // the kr-th set bit of m (kr < popcount(m)): halve the window six times
        int kr = k - base, pos = 0;
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            const int low = __popcll(m & ((1ull << w) - 1ull));
            const bool up = kr >= low;
            kr -= up ? low : 0;
            m = up ? m >> w : m;
            pos += up ? w : 0;
        }
        const int i = 64 * pass + pos;
        if (live && a.sample_t) a.sample_t[ray * S + j] = (float)(near_d + ((double)i + f) * h);
        if (live && a.dists) a.dists[ray * S + j] = (a.last_opaque && j == S - 1) ? 1e8f : share;
    }
}

unsigned blocks_for(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

int sum_parts(const OccParams& g) {
    const long long p = (g.cells + kThreads - 1) / kThreads;
    return (int)(p > kMaxParts ? kMaxParts : p);
}

}  // namespace

void k_occgrid_cell_points(const OccParams& g, const int* cells, long long n, const float* u, float* points,
                           hipStream_t s) {
    occ_cell_points_kernel<<<blocks_for(n), kThreads, 0, s>>>(g, cells, n, u, points);
}

void k_occgrid_update(const OccParams& g, float* density, const int* cells, long long n, const float* sigma,
                      int sigma_stride, float decay, hipStream_t s) {
    if (decay != 1.0f)
        occ_decay_kernel<<<blocks_for(g.cells), kThreads, 0, s>>>(g.cells, decay == 0.0f ? 0.0f : decay, density);
    occ_max_kernel<<<blocks_for(n), kThreads, 0, s>>>(g.cells, cells, n, sigma, sigma_stride, density);
}

int occgrid_threshold_scratch(const OccParams& g) { return sum_parts(g) + 1; }

void k_occgrid_threshold(const OccParams& g, const float* density, float threshold, int flags, unsigned* bits,
                         double* mean, long long* occupied, double* scratch, hipStream_t s) {
    const int parts = sum_parts(g);
    const long long per = (g.cells + parts - 1) / parts;
    double* thr = scratch + parts;
    occ_sum_kernel<<<parts, kThreads, 0, s>>>(g.cells, per, density, scratch);
    occ_mean_kernel<<<1, 64, 0, s>>>(scratch, parts, g.cells, threshold, (flags & LNERF_OCC_MEAN) ? 1 : 0, thr, mean,
                                     occupied);
    if (bits || occupied)
        occ_pack_kernel<<<blocks_for((g.cells + kPackSpan - 1) / kPackSpan), kThreads, 0, s>>>(g.cells, density, thr, bits,
                                                                                              occupied);
}

void k_sample_occupancy(const OccParams& g, const unsigned* bits, const float* rays, int n, int S, int steps,
                        float near_t, float far_t, const float* u, int flags, float* sample_t, float* dists,
                        int* n_occ, hipStream_t s) {
    OccSampleArgs a{};
    a.g = g;
    a.bits = bits;
    a.rays = rays;
    a.n = n;
    a.S = S;
    a.steps = steps;
    a.near_t = near_t;
    a.far_t = far_t;
    a.u = u;
    a.last_opaque = (flags & LNERF_OCC_LAST_OPAQUE) ? 1 : 0;
    a.sample_t = sample_t;
    a.dists = dists;
    a.n_occ = n_occ;
    const int per = kThreads >> 6;
    occ_sample_kernel<<<(unsigned)(((long long)n + per - 1) / per), kThreads, 0, s>>>(a);
}

}  // namespace lnerf
