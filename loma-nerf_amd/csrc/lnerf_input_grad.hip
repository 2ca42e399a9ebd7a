// lnerf_input_grad.hip -- gradients with respect to what the caller passed in: the reverse of the
// positional encoding (pos_encoding.py:38-69), of the ray sampling o + d t (train_nerf.py:289-299)
// and of get_rays (train_nerf.py:23-62). Extensions: loma differentiates none of the three (they
// are numpy code in the reference), so there is no loma counterpart.
//
//  input_grad_kernel   dE (rays*S, 3 + 6F) -> d_points (rays*S, 3) or d_rays (rays, 6) = [d_o, d_d]
//  pose_part_kernel    d_rays (n, 6) -> per-workgroup partials of the 12 sums of d_c2w
//  pose_sum_kernel     the partials, summed in index order
//
// Everything is float64 with one rounding to float32 at the store (the pose gradient stays
// float64), every sum has a fixed order (no atomics): repeated calls give the same bits. Built
// with -ffp-contract=off like lnerf_generic.hip.
#include "lnerf_composite.h"
#include "lnerf_internal.h"

namespace lnerf {

namespace {

constexpr size_t kStageBytes = 60 * 1024;   // LDS budget of the staged dE rows

// The fields comp::sample_coord reads (input_mode, x, S, near_t, far_t) and the kernel's own.
struct IgArgs {
    int input_mode;
    const float* x;
    int S;
    float near_t, far_t;
    int rays;          // RAYS: rays; POINTS: sample rows
    int F, k0;
    int rpw;           // RAYS: whole rays per workgroup (1 when a ray is longer than the workgroup)
    const float* dE;
    const float* scale;
    float* out;
};

// d_p[c] = dE[c] + sum_q 2^q (cos(2^q p_c) dE[3 + 6q + c] - sin(2^q p_c) dE[6 + 6q + c]) for the
// sample at row gs, whose dE row sits at e (LDS). p_c comes from the forward's own float64 path
// (comp::sample_coord: the given point, or ray_point's o + d t), and so do sin / cos: one sincos
// and the double-angle recurrence of comp::encode_coord, kept in float64 here (encode_coord itself
// rounds each value to float32 as it stores it, which is the forward's job, not the derivative's);
// LNERF_PE_DOUBLING = 0 takes one sincos per frequency, as the forward then does.
__device__ __forceinline__ void row_grad(const IgArgs& a, int gs, const float* e, double (&dp)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double g = (double)e[c];
        if (a.F > 0) {
            const double xc = comp::sample_coord(a, gs, c);
            double sn, cs, w = 1.0;
            if (LNERF_PE_DOUBLING) sincos(xc, &sn, &cs);
            for (int q = 0; q < a.F; ++q) {
                if (!LNERF_PE_DOUBLING) sincos(ldexp(xc, q), &sn, &cs);
                g += w * (cs * (double)e[3 + 6 * q + c] - sn * (double)e[6 + 6 * q + c]);
                if (LNERF_PE_DOUBLING) {
                    const double s2 = 2.0 * sn * cs;
                    cs = (cs - sn) * (cs + sn);
                    sn = s2;
                }
                w += w;
            }
        }
        dp[c] = g;
    }
}

// One workgroup of RB threads stages RB consecutive dE rows (contiguous in memory, so the loads
// coalesce) in LDS and gives each thread one row: a row is 3 + 6F floats, an odd stride, so the
// one-row-per-lane reads hit distinct banks.
//  POINTS: thread t writes row blockIdx RB + t.
//  RAYS:   a workgroup owns rpw = RB / S whole rays (S <= RB), or one ray that it walks RB samples
//          at a time (S > RB; no upper limit on S). Each thread keeps [sum d_p, sum t_j d_p] of its
//          own samples; the per-ray sums are then an inclusive segmented scan by lane shuffles (a
//          lane adds only lanes of its own ray: a NaN stays in its ray) and, for a ray spanning
//          waves, the earlier waves' lane-63 partials through LDS, added by the ray's last thread.
template <int RB>
__global__ void __launch_bounds__(RB) input_grad_kernel(IgArgs a) {
    extern __shared__ float stage[];
    __shared__ double pub[RB / 64][6];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k0 = a.k0;
    const double sc = a.scale ? (double)*a.scale : 1.0;
    if (a.input_mode != LNERF_INPUT_RAYS) {
        const long long row0 = (long long)blockIdx.x * RB;
        const int nrows = (int)min((long long)RB, (long long)a.rays - row0);
        const float* src = a.dE + (size_t)row0 * k0;
        for (int i = tid; i < nrows * k0; i += RB) stage[i] = src[i];
        __syncthreads();
        if (tid < nrows) {
            double dp[3];
            row_grad(a, (int)(row0 + tid), stage + tid * k0, dp);
#pragma unroll
            for (int c = 0; c < 3; ++c) a.out[(size_t)(row0 + tid) * 3 + c] = (float)(dp[c] * sc);
        }
        return;
    }
    const int S = a.S;
    const int seg = S < RB ? S : RB;             // threads per ray
    const int rl = tid / seg, jj = tid - rl * seg;
    const int ray0 = blockIdx.x * a.rpw, ray = ray0 + rl;
    const bool mine = rl < a.rpw && ray < a.rays;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < S; j0 += RB) {         // one pass when S <= RB
        const long long row0 = (long long)ray0 * S + j0;
        const int nrows = S <= RB ? min(a.rpw, a.rays - ray0) * S : min(RB, S - j0);
        if (j0) __syncthreads();                 // the previous pass's reads of stage
        const float* src = a.dE + (size_t)row0 * k0;
        for (int i = tid; i < nrows * k0; i += RB) stage[i] = src[i];
        __syncthreads();
        if (mine && tid < nrows) {
            double dp[3];
            row_grad(a, (int)(row0 + tid), stage + tid * k0, dp);
            const double t = ray_depth(j0 + jj, S, a.near_t, a.far_t);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] += dp[c];
                acc[3 + c] += t * dp[c];
            }
        }
    }
    const int jw = jj < lane ? jj : lane;        // this ray's threads before this one in this wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double o = __shfl_up(acc[q], d, 64);
            if (jw >= d) acc[q] = o + acc[q];
        }
    }
    if (lane == 63)
#pragma unroll
        for (int q = 0; q < 6; ++q) pub[wv][q] = acc[q];
    __syncthreads();
    if (mine && jj == seg - 1) {
        const int ws = (tid - jj) >> 6;          // the wave holding the ray's first thread
        for (int w = wv - 1; w >= ws; --w)
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] = pub[w][q] + acc[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) a.out[(size_t)ray * 6 + q] = (float)(acc[q] * sc);
    }
}

template <int RB>
void launch_input_grad(const IgArgs& a0, hipStream_t s) {
    IgArgs a = a0;
    unsigned grid;
    if (a.input_mode == LNERF_INPUT_RAYS) {
        a.rpw = a.S <= RB ? RB / a.S : 1;
        grid = (unsigned)((a.rays + a.rpw - 1) / a.rpw);
    } else {
        a.rpw = 0;
        grid = (unsigned)(((long long)a.rays + RB - 1) / RB);
    }
    input_grad_kernel<RB><<<grid, RB, (size_t)RB * a.k0 * sizeof(float), s>>>(a);
}

// ---- the reverse of get_rays ------------------------------------------------------------------
// rays[p] = [c2w[:, 3], c2w[:, :3] dir(p)], so d_c2w[a][3] = sum_p d_o[p][a] and d_c2w[a][b] =
// sum_p d_d[p][a] dir_b(p), dir(p) from cam_pixel_dir (get_rays_kernel's own). Stage 1: workgroup b
// sums the contiguous range [b per, (b + 1) per) of the rays, each thread its strided share in
// order, then a fixed tree in LDS. A pixel index outside the grid contributes nothing.
constexpr int kPoseThreads = 256;
constexpr int kPoseMaxParts = 256;
struct PoseCam {
    double K[9];
};
__global__ void __launch_bounds__(kPoseThreads) pose_part_kernel(int width, PoseCam cam,
                                                                 const int* __restrict__ pixels, int n, int per,
                                                                 const float* __restrict__ d_rays,
                                                                 double* __restrict__ part) {
    __shared__ double red[12][kPoseThreads];
    const int t = threadIdx.x, b0 = blockIdx.x * per, b1 = min(n, b0 + per);
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    for (int i = b0 + t; i < b1; i += kPoseThreads) {
        const int p = pixels ? pixels[i] : i;
        if (p < 0 || p >= width * width) continue;
        double dir[3];
        cam_pixel_dir(width, cam.K, p, dir);
        const float* r = d_rays + (size_t)i * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double dd = (double)r[3 + a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[a * 4 + b] += dd * dir[b];
            acc[a * 4 + 3] += (double)r[a];
        }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) red[q][t] = acc[q];
    __syncthreads();
    for (int w = kPoseThreads / 2; w > 0; w >>= 1) {
        if (t < w)
#pragma unroll
            for (int q = 0; q < 12; ++q) red[q][t] = red[q][t] + red[q][t + w];
        __syncthreads();
    }
    if (t < 12) part[(size_t)blockIdx.x * 12 + t] = red[t][0];
}

__global__ void __launch_bounds__(64) pose_sum_kernel(const double* __restrict__ part, int parts,
                                                      double* __restrict__ d_c2w) {
    const int q = threadIdx.x;
    if (q >= 12) return;
    double s = 0.0;
    for (int b = 0; b < parts; ++b) s += part[(size_t)b * 12 + q];
    d_c2w[q] = s;
}

}  // namespace

void k_input_grad(const lnerf_batch& b, const float* dE, const float* scale, float* d_input, hipStream_t s) {
    IgArgs a{};
    a.input_mode = b.input_mode;
    a.x = b.x;
    a.S = b.samples;
    a.near_t = b.near_t;
    a.far_t = b.far_t;
    a.rays = b.input_mode == LNERF_INPUT_RAYS ? b.rays : b.rays * b.samples;
    a.F = b.num_freqs;
    a.k0 = 3 + 6 * b.num_freqs;
    a.dE = dE;
    a.scale = scale;
    a.out = d_input;
    if (a.F < 0 || a.F > kMaxInputGradFreqs) marshal::fail("input gradient: num_freqs %d outside 0..%d", a.F, kMaxInputGradFreqs);
    const size_t row = (size_t)a.k0 * sizeof(float);
    if (256 * row <= kStageBytes) launch_input_grad<256>(a, s);
    else if (128 * row <= kStageBytes) launch_input_grad<128>(a, s);
    else launch_input_grad<64>(a, s);
}

int pose_grad_parts(int n) {
    const int g = (n + kPoseThreads - 1) / kPoseThreads;
    return g < 1 ? 1 : g > kPoseMaxParts ? kPoseMaxParts : g;
}

void k_pose_grad(int width, const double* K, const int* pixels, int n, const float* d_rays, double* part,
                 double* d_c2w, hipStream_t s) {
    PoseCam cam;
    for (int i = 0; i < 9; ++i) cam.K[i] = K[i];
    const int parts = pose_grad_parts(n);
    const int per = (n + parts - 1) / parts;
    pose_part_kernel<<<parts, kPoseThreads, 0, s>>>(width, cam, pixels, n, per, d_rays, part);
    pose_sum_kernel<<<1, 64, 0, s>>>(part, parts, d_c2w);
}

}  // namespace lnerf
