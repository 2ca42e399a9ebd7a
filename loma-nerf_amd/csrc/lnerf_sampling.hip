// lnerf_sampling.hip -- per-ray sample depths on the device: the producers that turn rays plus
// per-ray depths into what LNERF_INPUT_POINTS and lnerf_render_maps(..., sample_t, ...) accept, and
// the reverse of the point producer. Extensions: the reference samples linspace(near, far, S) only
// (its jitter is a TODO, train_nerf.py:289-294) and has no hierarchical sampling.
//
//  stratified_kernel     u (rays, S) -> sample_t (rays, S), one jittered depth per linspace cell
//  importance_kernel     weights (rays, S) -> t_fine (rays, n_fine) by inverting the piecewise-linear
//                        cdf of the interior weights, and t_all = sort(concat(t_coarse, t_fine))
//  ray_points_kernel     rays, sample_t -> points o + d t (rays*S, 3), dists (rays, S)
//  ray_points_grad_kernel  d_points -> d_rays (n, 6) = [sum_j d_p[j], sum_j t_j d_p[j]]
//
// The project's rule for input producers: float64 arithmetic, one rounding to float32 at the store,
// every sum in a fixed order (no atomics), so repeated calls give the same bits. Built with
// -ffp-contract=off like lnerf_input_grad.hip. No context, no workspace: free functions on a stream.
#include <cfloat>

#include "lnerf_internal.h"

namespace lnerf {

namespace {

constexpr int kThreads = 256;

// u clamped to [0, 1], NaN taken as 0 (a NaN fails the first comparison)
__device__ __forceinline__ double unit_clamp(float u) { return u > 0.0f ? (u < 1.0f ? (double)u : 1.0) : 0.0; }

// ---- 1. stratified jitter ---------------------------------------------------------------------
// Cell j of the linspace g: [lower_j, upper_j] with lower_j = j ? (g_{j-1} + g_j) / 2 : g_0 and
// upper_j = j < S - 1 ? (g_j + g_{j+1}) / 2 : g_{S-1}; t_j = lower_j + (upper_j - lower_j) u_j.
// upper_j is lower_{j+1}, so the depths are non-decreasing along a ray. One thread per sample.
__global__ void __launch_bounds__(kThreads) stratified_kernel(long long rows, int S, float near_t, float far_t,
                                                              const float* __restrict__ u,
                                                              float* __restrict__ sample_t) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= rows) return;
    const int j = (int)(r % S);
    const double g = ray_depth(j, S, near_t, far_t);
    const double lower = j ? 0.5 * (ray_depth(j - 1, S, near_t, far_t) + g) : g;
    const double upper = j < S - 1 ? 0.5 * (g + ray_depth(j + 1, S, near_t, far_t)) : g;
    sample_t[r] = (float)(lower + (upper - lower) * unit_clamp(u[r]));
}

// ---- 2. importance sampling -------------------------------------------------------------------
struct ImpArgs {
    int rays, S, n_fine;
    float near_t, far_t;
    const float* t_coarse;   // (rays, S) or NULL: (float)linspace(near_t, far_t, S)
    const float* weights;    // (rays, S)
    const float* u;          // (rays, n_fine) or NULL: (k + 0.5) / n_fine
    float* t_fine;           // (rays, n_fine) or NULL
    float* t_all;            // (rays, S + n_fine) or NULL
    int fine_pow2;           // P: the power of two from 64 up that holds n_fine
    int wave_doubles;        // LDS doubles per wave: 2 (S - 1) + (S + n_fine + P + 1) / 2
    int chunk;               // interior weights per lane in the scan: ceil((S - 2) / 64)
    int bin_steps;           // ceil(log2(S - 2)): halvings that bring S - 2 bins down to one
    int rank_steps;          // ceil(log2(S + 1)): the same for the S + 1 ranks among the coarse depths
    int fine_steps;          // ceil(log2(n_fine + 1)): and for the n_fine + 1 ranks among the fine ones
};

// One wave per ray, blockDim / 64 rays per workgroup; each wave works in an LDS region of its own:
//   m[S-1]    the bin edges, midpoints of the coarse depths (float64; exact for float32 depths)
//   cdf[S-1]  cdf_0 = 0, cdf_{i+1} = (sum_{k<=i} p_k) / sum p, the last exactly 1, p_i = w_{i+1} + 1e-5
//   tc[S]     the coarse depths, tf[n_fine] the rounded fine ones in u's order, ts[P] the fine ones
//             sorted (float32, for the merge)
// The cdf: each lane sums a contiguous chunk of p in index order, the chunk totals go through an
// inclusive wave scan by lane shuffles, and a prefix is its lane's exclusive offset plus its partial
// sum -- one fixed order. Every index below is bounded by S and n_fine alone: the weights and u only
// ever reach comparisons, so a NaN u or a garbage weight cannot move one. The barriers are workgroup
// barriers (every wave runs the same trip counts; a wave past the last ray recomputes the last ray
// and stores nothing).
__global__ void __launch_bounds__(kThreads) importance_kernel(ImpArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = a.S, nf = a.n_fine, nb = S - 1, np = S - 2;
    const long long ray_raw = (long long)blockIdx.x * (blockDim.x >> 6) + wv;
    const bool live = ray_raw < a.rays;
    const size_t ray = (size_t)(live ? ray_raw : a.rays - 1);
    double* m = lds + (size_t)wv * a.wave_doubles;
    double* cdf = m + nb;
    float* tc = reinterpret_cast<float*>(cdf + nb);
    float* tf = tc + S;
    float* ts = tf + nf;

    for (int j = lane; j < S; j += 64)
        tc[j] = a.t_coarse ? a.t_coarse[ray * S + j] : (float)ray_depth(j, S, a.near_t, a.far_t);
    // p into cdf[1..np] (coalesced loads); a NaN, infinite or negative weight counts as 0
    for (int i = lane; i < np; i += 64) {
        const float w = a.weights[ray * S + i + 1];
        cdf[i + 1] = (double)((w > 0.0f && w <= FLT_MAX) ? w : 0.0f) + 1e-5;
    }
    if (lane == 0) cdf[0] = 0.0;
    __syncthreads();
    for (int j = lane; j < nb; j += 64) m[j] = 0.5 * ((double)tc[j] + (double)tc[j + 1]);
    const int c0 = min(lane * a.chunk, np), c1 = min(c0 + a.chunk, np);
    double part = 0.0;
    for (int i = c0; i < c1; ++i) {
        part += cdf[i + 1];
        cdf[i + 1] = part;
    }
    double incl = part;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(incl, d, 64);
        if (lane >= d) incl = o + incl;
    }
    const double total = __shfl(incl, 63, 64);
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0;
    for (int i = c0; i < c1; ++i) cdf[i + 1] = i == np - 1 ? 1.0 : (excl + cdf[i + 1]) / total;
    __syncthreads();

    const double m_first = m[0], m_last = m[nb - 1];
    for (int k = lane; k < nf; k += 64) {
        const double u = a.u ? unit_clamp(a.u[ray * nf + k]) : ((double)k + 0.5) / (double)nf;
        // the largest bin i in [0, S - 3] with cdf_i <= u (cdf_0 = 0 <= u always)
        int lo = 0, hi = np - 1;
        for (int it = 0; it < a.bin_steps; ++it) {
            const int mid = min(max((lo + hi + 1) >> 1, 0), np - 1);
            if (cdf[mid] <= u) lo = mid;
            else hi = mid - 1;
        }
        const double ca = cdf[lo], cb = cdf[lo + 1], ma = m[lo], mb = m[lo + 1];
        // cb - ca > 0 wherever the 1e-5 floor is not swallowed (weights up to ~1e10); past that the
        // comparison keeps the quotient finite
        const double den = cb - ca;
        double frac = den > 0.0 ? (u - ca) / den : 0.0;
        frac = frac > 0.0 ? (frac < 1.0 ? frac : 1.0) : 0.0;
        float z = (float)(ma + frac * (mb - ma));
        // the one rounding may leave [m_0, m_{S-2}] (an edge need not be a float32): step back inside
        if ((double)z > m_last) z = nextafterf(z, -INFINITY);
        if ((double)z < m_first) z = nextafterf(z, INFINITY);
        tf[k] = z;
        if (live && a.t_fine) a.t_fine[ray * nf + k] = z;
    }
    if (!a.t_all) return;
    __syncthreads();

    // t_all = sort(concat(coarse, fine)) on the float32 values. Equal values have equal bits, so any
    // order among ties gives the same array. First the fine depths sorted into ts[0..P), P the power
    // of two from 64 up that holds n_fine, padded with +inf: a bitonic network, in registers by lane
    // shuffles when P = 64 (a lane per element), through LDS with a barrier per stage above that.
    const int P = a.fine_pow2;
    if (P == 64) {
        float v = lane < nf ? tf[lane] : INFINITY;
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const float o = __shfl_xor(v, j, 64);
                const bool keep_min = ((lane & k) == 0) == ((lane & j) == 0);
                v = keep_min ? fminf(v, o) : fmaxf(v, o);
            }
        ts[lane] = v;
    } else {
        for (int i = lane; i < P; i += 64) ts[i] = i < nf ? tf[i] : INFINITY;
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;   // i < p < P
                    const float x = ts[i], y = ts[p];
                    if ((x > y) == ((i & k) == 0)) {
                        ts[i] = y;
                        ts[p] = x;
                    }
                }
            }
    }
    __syncthreads();
    // Then the merge by rank: coarse j goes to j + #{fine < c_j} (ties: coarse first), the k-th
    // smallest fine depth to k + #{coarse <= it}; both counts are binary searches of fixed length.
    const int all = S + nf;
    for (int j = lane; j < S; j += 64) {
        const float v = tc[j];
        int lo = 0, hi = nf;
        for (int it = 0; it < a.fine_steps; ++it) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ts[mid] < v) lo = mid + 1;
                else hi = mid;
            }
        }
        const int pos = min(j + lo, all - 1);
        if (live) a.t_all[ray * all + pos] = v;
    }
    for (int k = lane; k < nf; k += 64) {
        const float v = ts[k];
        int lo = 0, hi = S;                  // the coarse depths are non-decreasing
        for (int it = 0; it < a.rank_steps; ++it) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tc[mid] <= v) lo = mid + 1;
                else hi = mid;
            }
        }
        const int pos = min(k + lo, all - 1);
        if (live) a.t_all[ray * all + pos] = v;
    }
}

// ---- 3. points and dists ----------------------------------------------------------------------
// points[i S + j] = o_i + d_i t_ij, dists[i][j] = t_{i,j+1} - t_ij, the last 1e8
// (train_nerf.py:306-311). One thread per sample.
__global__ void __launch_bounds__(kThreads) ray_points_kernel(const float* __restrict__ rays, long long rows, int S,
                                                              const float* __restrict__ sample_t,
                                                              float* __restrict__ points, float* __restrict__ dists) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= rows) return;
    const long long i = r / S;
    const int j = (int)(r - i * S);
    const double t = (double)sample_t[r];
    if (points) {
        const float* ray6 = rays + (size_t)i * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) points[(size_t)r * 3 + c] = (float)((double)ray6[c] + (double)ray6[3 + c] * t);
    }
    if (dists) dists[r] = j < S - 1 ? (float)((double)sample_t[r + 1] - t) : 1e8f;
}

// ---- 4. the reverse of (3) --------------------------------------------------------------------
// d_rays[i] = [sum_j d_p[j], sum_j t_j d_p[j]]. A group of G lanes (a power of two, 4..64, the
// smallest holding S or 64) owns a ray: lane g sums samples g, g + G, ... in order, then a fixed
// tree of lane shuffles inside the group (a NaN stays in its ray). 256 / G rays per workgroup.
__global__ void __launch_bounds__(kThreads) ray_points_grad_kernel(int n, int S, int G,
                                                                   const float* __restrict__ sample_t,
                                                                   const float* __restrict__ d_points,
                                                                   const float* __restrict__ scale,
                                                                   float* __restrict__ d_rays) {
    const int g = threadIdx.x & (G - 1);
    const long long ray_raw = (long long)blockIdx.x * (kThreads / G) + threadIdx.x / G;
    const bool live = ray_raw < n;
    const size_t ray = (size_t)(live ? ray_raw : n - 1);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = g; j < S; j += G) {
        const size_t r = ray * S + j;
        const double t = (double)sample_t[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double dp = (double)d_points[r * 3 + c];
            acc[c] += dp;
            acc[3 + c] += t * dp;
        }
    }
    for (int d = G >> 1; d > 0; d >>= 1)
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] = acc[q] + __shfl_down(acc[q], d, G);
    if (live && g == 0) {
        const double sc = scale ? (double)*scale : 1.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) d_rays[ray * 6 + q] = (float)(acc[q] * sc);
    }
}

int ceil_log2(int n) {
    int s = 0;
    while ((1 << s) < n) ++s;
    return s;
}

}  // namespace

void k_sample_stratified(int rays, int S, float near_t, float far_t, const float* u, float* sample_t,
                         hipStream_t s) {
    const long long rows = (long long)rays * S;
    stratified_kernel<<<(unsigned)((rows + kThreads - 1) / kThreads), kThreads, 0, s>>>(rows, S, near_t, far_t, u,
                                                                                          sample_t);
}

void k_sample_importance(int rays, int S, const float* t_coarse, float near_t, float far_t, const float* weights,
                         int n_fine, const float* u, float* t_fine, float* t_all, hipStream_t s) {
    ImpArgs a{};
    a.rays = rays;
    a.S = S;
    a.n_fine = n_fine;
    a.near_t = near_t;
    a.far_t = far_t;
    a.t_coarse = t_coarse;
    a.weights = weights;
    a.u = u;
    a.t_fine = t_fine;
    a.t_all = t_all;
    a.fine_pow2 = 64;
    while (a.fine_pow2 < n_fine) a.fine_pow2 <<= 1;
    a.wave_doubles = 2 * (S - 1) + (S + n_fine + a.fine_pow2 + 1) / 2;
    a.chunk = (S - 2 + 63) / 64;
    a.bin_steps = ceil_log2(S - 2);
    a.rank_steps = ceil_log2(S + 1);
    a.fine_steps = ceil_log2(n_fine + 1);
    // as many waves (rays) per workgroup as fit 64 KB of LDS: 4 at frame sizes, 2 at the largest
    // shape (28.7 KB a wave)
    const size_t wave_bytes = (size_t)a.wave_doubles * sizeof(double);
    int waves = (int)((size_t)(64 * 1024) / wave_bytes);
    waves = waves < 1 ? 1 : waves > kThreads / 64 ? kThreads / 64 : waves;
    const unsigned grid = (unsigned)(((long long)rays + waves - 1) / waves);
    importance_kernel<<<grid, waves * 64, wave_bytes * waves, s>>>(a);
}

void k_ray_points(const float* rays, int n, int S, const float* sample_t, float* points, float* dists,
                  hipStream_t s) {
    const long long rows = (long long)n * S;
    ray_points_kernel<<<(unsigned)((rows + kThreads - 1) / kThreads), kThreads, 0, s>>>(rays, rows, S, sample_t,
                                                                                          points, dists);
}

void k_ray_points_grad(int n, int S, const float* sample_t, const float* d_points, const float* scale,
                       float* d_rays, hipStream_t s) {
    int G = 4;
    while (G < 64 && G < S) G <<= 1;
    const int per = kThreads / G;
    ray_points_grad_kernel<<<(unsigned)(((long long)n + per - 1) / per), kThreads, 0, s>>>(n, S, G, sample_t,
                                                                                            d_points, scale, d_rays);
}

}  // namespace lnerf
