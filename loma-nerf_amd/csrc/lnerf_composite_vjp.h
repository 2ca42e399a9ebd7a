// lnerf_composite_vjp.h -- composite_tile_wave (lnerf_composite.h) with the reverse seeded from the
// caller's adjoints of the render maps instead of the loss (lnerf_render_maps_vjp; an extension, no
// loma counterpart). Included by the VJP object alone (lnerf_k16_vjp.hip).
#pragma once
#include "lnerf_composite.h"

namespace lnerf {
namespace comp {

// t_j of sample row gs for the depth term (read only when d_depth is given)
template <class A>
__device__ __forceinline__ float vjp_sample_t(const A& a, const VjpArgs& v, size_t gs, int j) {
    if (a.input_mode == LNERF_INPUT_RAYS) return (float)ray_depth(j, a.S, a.near_t, a.far_t);
    return v.sample_t[gs];
}

// The forward half is composite_tile_wave's, statement for statement (acc_color comes out with the
// training step's bits); no loss is formed (rayloss 0) and no d_target written. The ray's last
// sample loads the per-ray adjoints into LDS -- dC into c_ray [rays][4] at 11 TS as the training
// variant leaves its dacc there, dD and dO into [rays][2] at 15 TS (free in this variant, inside
// kCompFloats = 21 per sample) -- and after the barrier every sample forms its seeds
//   dw   = rgb . dC + t dD + dO + dWt      drgb = w dC + dRGBA[0..2]      dsigma += dRGBA[3]
// (dsigma before the ReLU gate: rgba's sigma is the post-ReLU value). A NULL adjoint's term is never
// formed, so with dC alone the expressions are the training variant's. From dal = T dw on, the suffix
// scan, dc, the alpha reverse and the head reverse are composite_tile_wave's.
template <int TS, class A>
__device__ __forceinline__ void composite_tile_wave_vjp(const A& a, int wg, float* comp, float* rayloss,
                                                        const VjpArgs& v) {
    static_assert(TS % 64 == 0, "whole waves of samples");
    static_assert((TS / 64) * 8 <= TS, "the wave partials [TS / 64][8] fit their TS-float region at 8 TS");
    static_assert(17 <= kCompFloats, "dD / dO [rays][2] at 15 TS fit the compositing scratch");
    const int tid = threadIdx.x, S = a.S, lane = tid & 63, wv = tid >> 6;
    float* c_z = comp;
    float* c_gz = comp + 4 * TS;
    float* pub = comp + 8 * TS;
    float* c_cc = comp + 9 * TS;
    float* c_P = comp + 10 * TS;
    float* c_ray = comp + 11 * TS;
    float* c_ray2 = comp + 15 * TS;
    const bool act = tid < TS;
    const int ls = act ? tid : 0;
    const int rl = ls / S, j = ls - rl * S;   // ray within the tile, sample within the ray
    const int ray = wg * a.rpw + rl;
    const int ntile = a.rpw * S;
    const bool valid = act && ls < ntile && ray < a.rays;
    const size_t gs = (size_t)ray * S + j;
    float z[4] = {0, 0, 0, 0}, rgb[3] = {0, 0, 0}, sigma = 0, delta = 0, al = 0, cc = 1;
    if (valid) {
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = c_z[ls * 4 + k];
        // head activation (nerf.py:153-167): channel 3 ReLU, 0..2 sigmoid
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = 1.0f / (1.0f + expf(0.0f - z[k]));
        sigma = (z[3] > 0.0f) ? z[3] : 0.0f;
        delta = a.dists ? a.dists[gs] : ray_delta(j, S, a.near_t, a.far_t);
        al = 1.0f - expf((0.0f - sigma) * delta);
        cc = (1.0f - al) + (float)(1e-10);
    }
    // the per-sample adjoints, in flight over the scans: one coalesced float and one 16-byte load
    typedef float f4 __attribute__((ext_vector_type(4)));
    float dwt = 0.0f, tj = 0.0f;
    f4 drg = f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        if (v.d_weights) dwt = v.d_weights[gs];
        if (v.d_rgba) drg = *(const f4*)(v.d_rgba + gs * 4);
        if (v.d_depth) tj = vjp_sample_t(a, v, gs, j);
    }
    const int jw = j < lane ? j : lane;        // this ray's samples before this one in this wave
    const int ws = (ls - j) >> 6;              // the wave holding the ray's first sample
    // P_j, the inclusive product (nerf.py:226-272)
    float P = cc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(P, d, 64);
        if (jw >= d) P = o * P;
    }
    if (act) {
        if (lane == 63) pub[wv * 8] = P;
        c_cc[ls] = cc;
    }
    __syncthreads();
    if (act) {
        for (int w = wv - 1; w >= ws; --w) P = pub[w * 8] * P;
        c_P[ls] = P;
    }
    const float T = (j == 0) ? 1.0f : P;
    const float wgt = al * T;
    // colour: the segmented sum of w rgb, read at the ray's last sample
    float cv[3] = {wgt * rgb[0], wgt * rgb[1], wgt * rgb[2]};
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float o = __shfl_up(cv[k], d, 64);
            if (jw >= d) cv[k] = o + cv[k];
        }
    }
    if (act && lane == 63)
#pragma unroll
        for (int k = 0; k < 3; ++k) pub[wv * 8 + 1 + k] = cv[k];
    __syncthreads();
    if (act && j == S - 1 && ls < ntile) {
        for (int w = wv - 1; w >= ws; --w)
#pragma unroll
            for (int k = 0; k < 3; ++k) cv[k] = pub[w * 8 + 1 + k] + cv[k];
        if (valid) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (a.acc_color) a.acc_color[(size_t)ray * 3 + k] = cv[k];
            // the ray's adjoints, for every sample of the ray
            if (v.d_acc_color)
                for (int k = 2; k >= 0; --k) c_ray[rl * 4 + k] = v.d_acc_color[(size_t)ray * 3 + k];
            if (v.d_depth) c_ray2[rl * 2] = v.d_depth[ray];
            if (v.d_opacity) c_ray2[rl * 2 + 1] = v.d_opacity[ray];
        }
        rayloss[rl] = 0.0f;
    }
    __syncthreads();

    // ---- reverse, per sample ----
    float dacc[3] = {0, 0, 0}, dw = 0.0f, drgb[4] = {0, 0, 0, 0};
    if (valid) {
        if (v.d_acc_color) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dacc[k] = c_ray[rl * 4 + k];
            for (int k = 2; k >= 0; --k) {
                dw += rgb[k] * dacc[k];
                drgb[k] += wgt * dacc[k];
            }
        }
        if (v.d_depth) dw += tj * c_ray2[rl * 2];
        if (v.d_opacity) dw += c_ray2[rl * 2 + 1];
        if (v.d_weights) dw += dwt;
        if (v.d_rgba) {
#pragma unroll
            for (int k = 0; k < 3; ++k) drgb[k] += drg[k];
        }
    }
    float dal = T * dw;
    // G_j = a_j + c_{j+1} G_{j+1}: the suffix composition of (a, b) pairs, in-wave, then the later
    // waves' partials (their lane 0's composition; the ray's last sample has b = 0)
    float ga = (j >= 1) ? al * dw : 0.0f;
    float gb = (valid && j + 1 < S) ? c_cc[ls + 1] : 0.0f;
    const int rest = S - 1 - j, lrest = 63 - lane;
    const int je = rest < lrest ? rest : lrest;   // this ray's samples after this one in this wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float oa = __shfl_down(ga, d, 64), ob = __shfl_down(gb, d, 64);
        if (je >= d) {
            ga = ga + gb * oa;
            gb = gb * ob;
        }
    }
    if (act && lane == 0) {
        pub[wv * 8 + 4] = ga;
        pub[wv * 8 + 5] = gb;
    }
    __syncthreads();
    // the wave holding the ray's last sample; a pseudo-ray past the tile's last whole ray (ls >=
    // ntile, never valid) may end past the last wave: clamped, so the carry never reads past pub's
    // [TS / 64][8] partials
    const int we = min((ls - j + S - 1) >> 6, TS / 64 - 1);
    if (act && we > wv) {
        float gn = 0.0f;
        for (int w = we; w > wv; --w) gn = pub[w * 8 + 4] + pub[w * 8 + 5] * gn;
        ga = ga + gb * gn;
    }
    if (valid) {
        const float dc = (j >= 1) ? c_P[ls - 1] * ga : ga;
        dal += 0.0f - dc;                                       // cC = (1 - al) + 1e-10
        const float adj2 = (0.0f - dal) * expf((0.0f - sigma) * delta);   // alpha reverse
        drgb[3] += 0.0f - (delta * adj2);
        if (v.d_rgba) drgb[3] += drg[3];                        // before the gate: sigma's own adjoint
        if (a.d_dists) a.d_dists[gs] = 0.0f + (0.0f - sigma) * adj2;
        // head activation reverse (reverse_diff.py Div/exp/Sub rules; ReLU on the post value)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dz = drgb[k];
            float g;
            if (k == 3) {
                g = (sigma > 0.0f) ? dz : 0.0f;
            } else {
                const float x = z[k];
                const float u = 1.0f + expf(0.0f - x);
                const float adj_div = ((0.0f - dz) * 1.0f) / (u * u);
                g = 0.0f + (0.0f - adj_div * expf(0.0f - x));
            }
            c_gz[ls * 4 + k] = g;
        }
    } else if (act) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c_gz[ls * 4 + k] = 0.0f;
    }
}

}  // namespace comp
}  // namespace lnerf
