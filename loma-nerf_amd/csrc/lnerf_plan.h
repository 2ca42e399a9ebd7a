// lnerf_plan.h -- host-only sizes of one fused step (no HIP): the layout of its slabs, planes and
// partials, and the one carve of the fused workspace into regions.
//
// lnerf_fused.hip turns the carve into device pointers (fused_plan_tile) and sizes the allocation
// from it (fused_workspace_bytes); tests/native/plan_check.cpp checks it on its own under
// AddressSanitizer / UBSan. The LNERF_HD helpers are the ones the kernels call too.
#pragma once

#include "lnerf.h"
#include "lnerf_marshal.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LNERF_HD __host__ __device__ constexpr
#else
#define LNERF_HD constexpr
#endif

namespace lnerf {

constexpr int kTileSamples = 128;   // samples per k16 workgroup (8 waves x 16); 64 with K16_W4
constexpr int kLossStage1 = 256;    // blocks of the render loss's first reduction stage (loss_stage1_kernel)
constexpr int kWmaxParts = 32;   // blocks per layer of the max|W| pass before the fp16x3 packing
constexpr int kHeadCols = 16;    // head columns with their own fp16x3 weight shift (k16 head outputs)
constexpr int kDefaultDwGrid = 512;   // dW workgroups per step unless LNERF_OPT_DW_GRID says otherwise
// The default budget for a batch of `samples` sample rows: 512 at the bench size and above, down to
// 256 for smaller batches, where k2 is latency-bound and its time flat from 256 to 512 workgroups
// while the in-order reduce over the splits grows with them (config 2, 32 768 samples, round 5:
// 256 -> 0.073 ms per step, 512 -> 0.082; cfg3 keeps 512: 384 -> 0.88 ms of k2, 512 -> 0.73)
LNERF_HD int default_dw_grid(long long samples) {
    return samples / 128 >= kDefaultDwGrid ? kDefaultDwGrid : samples / 128 <= 256 ? 256 : (int)(samples / 128);
}

// ---- int24 activation slabs (fp16x3 training) --------------------------------------------------
// k1 stores each A_l value (X for l = 0) that k2 reads as q = rint(x 2^(xa + 8)), xa = the
// sample's row shift (fp16x3_shift of its max|x|, so |q| < 2^22), as the low 24 bits of the float
// 1.5 2^23 + q (whose mantissa field is 2^22 + q); 4 values in 12 B. 2^-22 of the row's max|x|,
// the precision fp16x3 keeps of it anyway; 25 % fewer bytes through HBM for the A half of the
// slabs. G_l slabs stay fp32 (their rows span more range: tests/test_gpu_edge.py). A tile-block
// (32 samples x 32 features) is then 3 KiB = 768 float slots instead of 1024.
#ifndef LNERF_A24
#define LNERF_A24 1
#endif
LNERF_HD bool a24_slabs(int PL) { return PL == 2 && LNERF_A24 != 0; }
LNERF_HD int a_tile_floats(int PL) { return a24_slabs(PL) ? 768 : 1024; }

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int pow2_16(int t) { return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : 16; }

// Sizes and offsets of one step's workspace (floats unless noted).
struct Layout {
    int ht16, ks16_f[kMaxLayers], ks16_b[kMaxLayers], to16_f[kMaxLayers], to16_b[kMaxLayers];
    size_t w16f_off[kMaxLayers], w16b_off[kMaxLayers], w16_total;   // u16
    size_t b16_total;
    size_t mask_total;                                               // u64
    size_t act_off[kMaxLayers], x_off, act_total;
    size_t grad_off[kMaxLayers], grad_total;
    int splits[kMaxLayers], wg_off[kMaxLayers], dw_grid;
    size_t dwp_off[kMaxLayers], dwp_total, dbp_off[kMaxLayers], dbp_total;
    int num_wg, blocks, rpw;
};

// train = false (render): no slabs, masks or dW partials (the forward-only kernel writes none).
// a_tile: float slots per 32 x 32 tile-block of an activation slab (a_tile_floats: 768 for int24 A
// slabs, 1024 for fp32; the workspace is sized with 1024)
inline void make_layout(Layout& y, const lnerf_mlp& m, int rays, int S, bool train, int dw_grid, int tile,
                        int a_tile = 1024) {
    const int L = m.num_layers;
    int kt[kMaxLayers], nt[kMaxLayers];
    for (int l = 0; l < L; ++l) {
        kt[l] = (m.k[l] + 31) / 32;
        nt[l] = (m.n[l] + 31) / 32;
    }
    // k16 packing: every hidden layer's forward and every l >= 1 backward with ht16 16-wide output
    // tiles, the head forward with 1 and the dX pass with pow2(k0 / 16); per layer and pass, 3
    // planes of [k-step][output tile][1 KiB] (sized for bf16x6; fp16x3 / bf16 use 2 / 1)
    int mx16 = 1;
    for (int l = 0; l + 1 < L; ++l) mx16 = (m.n[l] + 15) / 16 > mx16 ? (m.n[l] + 15) / 16 : mx16;
    y.ht16 = pow2_16(mx16);
    size_t off = 0;
    for (int l = 0; l < L; ++l) {
        y.ks16_f[l] = kt[l];
        y.ks16_b[l] = nt[l];
        y.to16_f[l] = (l < L - 1) ? y.ht16 : 1;
        y.to16_b[l] = (l >= 1) ? y.ht16 : pow2_16((m.k[0] + 15) / 16);
        y.w16f_off[l] = off; off += align_up((size_t)y.ks16_f[l] * y.to16_f[l] * 3 * 512, 512);
        y.w16b_off[l] = off; off += align_up((size_t)y.ks16_b[l] * y.to16_b[l] * 3 * 512, 512);
    }
    y.w16_total = off;
    y.b16_total = (size_t)L * 256;
    y.rpw = S >= tile ? 1 : tile / S;
    y.num_wg = (rays + y.rpw - 1) / y.rpw;
    y.mask_total = train ? (size_t)y.num_wg * (L > 1 ? L - 1 : 0) * (tile / 16) * 64 : 0;
    y.blocks = y.num_wg * (tile / 32);
    off = 0;
    y.x_off = off; off += (size_t)y.blocks * kt[0] * a_tile;
    for (int l = 0; l < L - 1; ++l) { y.act_off[l] = off; off += (size_t)y.blocks * nt[l] * a_tile; }
    y.act_total = train ? off : 0;
    off = 0;
    for (int l = 0; l < L; ++l) { y.grad_off[l] = off; off += (size_t)y.blocks * nt[l] * 1024; }
    y.grad_total = train ? off : 0;
    // dW: one launch over every layer, ~dw_grid workgroups (lnerf_ctx_set_option
    // LNERF_OPT_DW_GRID; 512 by default) split between the layers in proportion to the slab bytes
    // each one streams (kt + nt tiles per 32-sample block): the kernel is bandwidth-bound, so
    // equal bytes per workgroup balance it. One partial per split.
    const int grid = dw_grid > 0 ? (dw_grid < 16 ? 16 : dw_grid > 4096 ? 4096 : dw_grid)
                                 : default_dw_grid((long long)rays * S);
    auto weight = [&](int l) { return kt[l] + nt[l]; };
    int tiles_sum = 0;
    for (int l = 0; l < L; ++l) tiles_sum += weight(l);
    size_t dwp = 0, dbp = 0;
    int wg = 0;
    for (int l = 0; l < L; ++l) {
        int sp = (int)((long long)grid * weight(l) / tiles_sum);
        sp = sp < 1 ? 1 : sp;
        sp = sp > y.blocks ? y.blocks : sp;
        y.splits[l] = sp;
        y.wg_off[l] = wg;
        wg += sp;
        y.dwp_off[l] = dwp;
        dwp += (size_t)sp * kt[l] * 32 * nt[l] * 32;
        y.dbp_off[l] = dbp;
        dbp += (size_t)sp * nt[l] * 32;
    }
    y.dw_grid = wg;
    y.dwp_total = train ? dwp : 0;
    y.dbp_total = train ? dbp : 0;
}

// The fused workspace's regions as float offsets from its base, in carve order, each on a 64-float
// boundary; total is where the carve ends. The one statement of the carve: fused_plan_tile adds the
// offsets to the base, fused_workspace_floats sizes the allocation from total.
struct FusedCarve {
    size_t guard, grad, loss_part, dw_part, db_part, loss_total, loss_stage;   // FusedPlan's pointers of these names
    size_t w16, w16x, b16, mask_g;
    size_t wexp16;                // then, kMaxLayers ints on, dw_shift
    size_t wmax_part, hexp16;
    size_t sexp, epart, xcount;   // training only: a render carve advances nothing for them
    size_t act;                   // last: see fused_carve
    size_t total;
};

inline FusedCarve fused_carve(const Layout& y, int L, int tile, bool train) {
    FusedCarve c{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t o = off;
        off += align_up(floats, 64);
        return o;
    };
    // every region but the activation slabs (whose size follows the split: a_tile_floats) first, so
    // that the fp16x3 plan and its bf16x6 re-run (the floor guard) share all other offsets
    c.guard = take(64);
    c.grad = take(y.grad_total);
    c.loss_part = take((size_t)y.num_wg);
    c.dw_part = take(y.dwp_total);
    c.db_part = take(y.dbp_total);
    c.loss_total = take(1);
    c.loss_stage = take(kLossStage1);
    c.w16 = take((y.w16_total + 1) / 2);
    c.w16x = take((y.w16_total + 1) / 2);
    c.b16 = take(y.b16_total);
    c.mask_g = take(y.mask_total * 2);
    c.wexp16 = take(2 * kMaxLayers);
    c.wmax_part = take((size_t)kMaxLayers * kWmaxParts + kWmaxParts * kHeadCols);
    c.hexp16 = take((size_t)kHeadCols);
    c.sexp = take(train ? (size_t)L * y.num_wg * tile : 0);
    c.epart = take(train ? (size_t)L * y.num_wg * 8 : 0);
    c.xcount = take(train ? (size_t)2 * y.dw_grid : 0);
    c.act = take(y.act_total);
    c.total = off;
    return c;
}

// The floats to allocate for any plan of this batch: the larger carve over the tile sizes a plan may
// take (64 under LNERF_K16_W4, which needs S <= 64; 128 otherwise), with fp32 slabs (a_tile = 1024).
inline size_t fused_workspace_floats(const lnerf_mlp& m, int rays, int S, bool train, int dw_grid) {
    size_t f = 0;
    for (int tile = kTileSamples; tile >= (S <= 64 ? 64 : kTileSamples); tile /= 2) {
        Layout y;
        make_layout(y, m, rays, S, train, dw_grid, tile);
        const size_t t = fused_carve(y, m.num_layers, tile, train).total;
        f = t > f ? t : f;
    }
    return f;
}

}  // namespace lnerf
