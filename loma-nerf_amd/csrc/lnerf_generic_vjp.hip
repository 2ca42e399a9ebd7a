// lnerf_generic_vjp.hip -- the loma-order compositing reverse seeded from the caller's adjoints
// (lnerf_render_maps_vjp on the generic path; an extension, no loma counterpart).
//
// lg_composite_bwd_kernel (lnerf_generic.hip) with its loss reverse replaced: the stages, the loop
// order and every adjoint expression from the colour reverse down are the same, so with
// d_acc_color = 2 (C - target) and no other adjoint the results are lnerf_train_step's generic
// path's at seed 1, bit for bit. One thread per ray, any number of samples.
//
// Compiled with -ffp-contract=off like lnerf_generic.hip.
#include "lnerf_internal.h"

#include <math.h>

namespace lnerf {
namespace {

__device__ __forceinline__ float& io_at(const LgDims& d, float* IO, int l, int i, int j) {
    return IO[((size_t)l * d.io_rows + i) * d.io_cols + j];
}

// The adjoint buffers arrive zeroed (generic_step), as for lg_composite_bwd_kernel.
__global__ void lg_composite_vjp_kernel(LgDims d, const float* __restrict__ rgba,
                                        const float* __restrict__ dists,
                                        const float* __restrict__ alpha,
                                        const float* __restrict__ cpT,   // final cp (T values)
                                        const float* __restrict__ cpC,
                                        const float* __restrict__ cpP,
                                        const float* __restrict__ wsamp, LgAdjoints a, LgVjp vjp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.th) return;
    const int S = d.S, L = d.L;
    const size_t o = (size_t)i * S;
    const comp::VjpArgs& v = vjp.v;
    float* dacc = a.dacc + (size_t)i * d.acc_cols;
    // the seeds (in place of the loss reverse, :297-302): dacc = dC, dwsamp_j = t_j dD + dO + dWt_j,
    // drgba_j = dRGBA_j. A NULL adjoint contributes no term at all.
    if (v.d_acc_color)
        for (int j = 2; j >= 0; --j) dacc[j] += v.d_acc_color[(size_t)i * 3 + j];
    for (int j = S - 1; j >= 0; --j) {
        if (v.d_depth) {
            const float t = vjp.rays_mode ? (float)ray_depth(j, S, vjp.near_t, vjp.far_t) : v.sample_t[o + j];
            a.dwsamp[o + j] += t * v.d_depth[i];
        }
        if (v.d_opacity) a.dwsamp[o + j] += v.d_opacity[i];
        if (v.d_weights) a.dwsamp[o + j] += v.d_weights[o + j];
        if (v.d_rgba)
            for (int k = 3; k >= 0; --k) a.drgba[(o + j) * 4 + k] += v.d_rgba[(o + j) * 4 + k];
    }
    // colour reverse (:281-288), statements c = 2, 1, 0
    if (v.d_acc_color)
        for (int j = S - 1; j >= 0; --j)
            for (int c = 2; c >= 0; --c) {
                const float adj = dacc[c];
                const float a_w = rgba[(o + j) * 4 + c] * adj;
                const float a_rgb = wsamp[o + j] * adj;
                dacc[c] = 0.0f;
                dacc[c] += adj;
                a.dwsamp[o + j] += a_w;
                a.drgba[(o + j) * 4 + c] += a_rgb;
            }
    // weights reverse (:267-272)
    for (int j = S - 1; j >= 0; --j) {
        const float adj = a.dwsamp[o + j];
        const float a_al = cpT[o + j] * adj;
        const float a_cp = alpha[o + j] * adj;
        a.dwsamp[o + j] = 0.0f;
        a.dalpha[o + j] += a_al;
        a.dcp[o + j] += a_cp;
    }
    // T_0 = 1 reverse (:252-258)
    if (S > 0) a.dcp[o] = 0.0f;
    // shift reverse (:238-246)
    for (int j = S - 1; j >= 0; --j) {
        const float adj = a.dwsamp[o + j];
        a.dwsamp[o + j] = 0.0f;
        if (j == 0) a.dalpha[o] += adj;
        else a.dcp[o + j - 1] += adj;
    }
    // cumprod reverse (:226-232)
    for (int j = S - 1; j >= 1; --j) {
        const float adj = a.dcp[o + j];
        const float a_left = cpC[o + j] * adj;
        const float a_right = cpP[o + j - 1] * adj;
        a.dcp[o + j] = 0.0f;
        a.dcp[o + j - 1] += a_left;
        a.dcp[o + j] += a_right;
    }
    // cumprod init reverse (:215-220)
    for (int j = S - 1; j >= 0; --j) {
        const float adj = a.dcp[o + j];
        a.dcp[o + j] = 0.0f;
        a.dalpha[o + j] += 0.0f - adj;
    }
    // alpha reverse (:200-205): alpha = 1 - exp((0 - sigma) * delta). drgba[..][3] already holds
    // dRGBA_j[3]; the ReLU gate on the post value comes after, in lg_act_bwd_kernel.
    for (int j = S - 1; j >= 0; --j) {
        const float sigma = rgba[(o + j) * 4 + 3], delta = dists[o + j];
        const float adj = a.dalpha[o + j];
        const float adj1 = 0.0f - adj;
        const float adj2 = adj1 * expf((0.0f - sigma) * delta);
        const float a_sigma = 0.0f - (delta * adj2);
        const float a_delta = (0.0f - sigma) * adj2;
        a.dalpha[o + j] = 0.0f;
        a.drgba[(o + j) * 4 + 3] += a_sigma;
        a.ddists[o + j] += a_delta;
    }
    // copy reverse (:182-191)
    for (int j = S - 1; j >= 0; --j)
        for (int k = 3; k >= 0; --k) {
            const float adj = a.drgba[(o + j) * 4 + k];
            a.drgba[(o + j) * 4 + k] = 0.0f;
            io_at(d, a.dIO, L - 1, i * S + j, k) += adj;
        }
}

}  // namespace

void lg_composite_vjp_launch(const LgDims& d, const LgBuffers& b, const LgAdjoints& a, const LgVjp& vjp,
                             hipStream_t s) {
    if (d.th > 0)
        lg_composite_vjp_kernel<<<(d.th + 127) / 128, 128, 0, s>>>(d, b.rgba, b.dists, b.alpha, b.cp, b.cpC, b.cpP,
                                                                   b.wsamp, a, vjp);
}

}  // namespace lnerf
