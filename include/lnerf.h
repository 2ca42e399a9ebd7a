/*
 * lnerf.h -- C ABI of libloma_nerf.so, the MI355X-native NeRF ray-marching engine.
 *
 * Two levels, both exported by the same library (see INTEGRATION.md for the bindings):
 *
 *  (1) loma-compat entry points with the exact signatures loma's C target generates for
 *      scripts/nerf.py and scripts/mlp_fit.py (codegen_c.py:8-30,47-57; reverse_diff.py:504-517).
 *      Arrays are nested host pointer tables (mlp_utils.py:33-118), exactly what ctypes passes.
 *      They gather into pinned memory, run the HIP kernels on the calling thread's stream and
 *      scatter the results back, with loma's semantics.
 *
 *  (2) the native batched API on device-resident, contiguous buffers (the throughput path).
 *
 * No torch or HIP types appear here: streams are passed as `void*` (a hipStream_t; NULL = the
 * device's default (null) stream, which is torch's default stream). Every entry point returns 0
 * on success / a negative error code, or (loma-compat float returns) NaN on failure; lnerf_last_error() describes it.
 */
#ifndef LNERF_H
#define LNERF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNERF_MAX_LAYERS 16

/* ------------------------------------------------------------------------------------------ */
/* (1) loma-compat ABI                                                                          */
/* ------------------------------------------------------------------------------------------ */

/* Replaces the loma-generated `nerf_evaluate_and_march` (scripts/nerf.py:1-304, bound at
 * train_nerf.py:212 and called at :325 and :616). Returns the sum-of-squares loss. */
float nerf_evaluate_and_march(float** layer_input, int layer_input_h, int layer_input_w,
                              float*** ws, float** bs, float** target_image, int target_image_h,
                              int target_image_w, int num_weights, int** weight_shapes,
                              int** bias_shapes, int** intermediate_output_shapes,
                              float*** intermediate_outputs, float*** img_sample_rgba_arr,
                              int num_samples, float** dists, float** alpha,
                              float** cumprod_alpha, float** weights_samples,
                              float** accumulated_color);

/* Replaces `grad_nerf_evaluate_and_march = rev_diff(nerf_evaluate_and_march)`
 * (scripts/nerf.py:306, bound at train_nerf.py:213, called at :395-478). Every In array is
 * followed by its adjoint buffer, every In int by an int* adjoint (never written), and the last
 * argument is the seed `_dreturn` (reverse_diff.py:504-517). Adjoint buffers are accumulated
 * into; primal buffers are left unchanged. */
void grad_nerf_evaluate_and_march(
    float** layer_input, float** d_layer_input, int layer_input_h, int* d_layer_input_h,
    int layer_input_w, int* d_layer_input_w, float*** ws, float*** d_ws, float** bs,
    float** d_bs, float** target_image, float** d_target_image, int target_image_h,
    int* d_target_image_h, int target_image_w, int* d_target_image_w, int num_weights,
    int* d_num_weights, int** weight_shapes, int** d_weight_shapes, int** bias_shapes,
    int** d_bias_shapes, int** intermediate_output_shapes, int** d_intermediate_output_shapes,
    float*** intermediate_outputs, float*** d_intermediate_outputs,
    float*** img_sample_rgba_arr, float*** d_img_sample_rgba_arr, int num_samples,
    int* d_num_samples, float** dists, float** d_dists, float** alpha, float** d_alpha,
    float** cumprod_alpha, float** d_cumprod_alpha, float** weights_samples,
    float** d_weights_samples, float** accumulated_color, float** d_accumulated_color,
    float _dreturn);

/* Replaces loma's `mlp_fit` (scripts/mlp_fit.py:1-147; fit_img.py:359,515-530). `layer_output`
 * is unused, as in the reference. */
float mlp_fit(float** layer_input, int layer_input_h, int layer_input_w, float** layer_output,
              float*** ws, float** bs, float** target_image, int target_image_h,
              int target_image_w, int num_weights, int** weight_shapes, int** bias_shapes,
              int** intermediate_output_shapes, float*** intermediate_outputs);

/* Replaces `grad_mlp_fit = rev_diff(mlp_fit)` (scripts/mlp_fit.py:174; fit_img.py:361,468-498). */
void grad_mlp_fit(float** layer_input, float** d_layer_input, int layer_input_h,
                  int* d_layer_input_h, int layer_input_w, int* d_layer_input_w,
                  float** layer_output, float** d_layer_output, float*** ws, float*** d_ws,
                  float** bs, float** d_bs, float** target_image, float** d_target_image,
                  int target_image_h, int* d_target_image_h, int target_image_w,
                  int* d_target_image_w, int num_weights, int* d_num_weights,
                  int** weight_shapes, int** d_weight_shapes, int** bias_shapes,
                  int** d_bias_shapes, int** intermediate_output_shapes,
                  int** d_intermediate_output_shapes, float*** intermediate_outputs,
                  float*** d_intermediate_outputs, float _dreturn);

/* Replaces loma's `mult_a_b` (scripts/mlp_fit.py:150-172; fit_img.py:360,370). */
void mult_a_b(float** a, int a_h, int a_w, float** b, int b_h, int b_w, float** c);

/* ------------------------------------------------------------------------------------------ */
/* (2) native batched API (device pointers)                                                    */
/* ------------------------------------------------------------------------------------------ */

typedef struct lnerf_ctx lnerf_ctx;

/* MLP shape. Weights use the reference's padded layout (mlp_utils.py:272-313): ws[l][k][j] at
 * ws[(l*w_k + k)*w_n + j], bs[l][j] at bs[l*w_n + j]; layer l maps k[l] -> n[l] features,
 * ReLU on hidden layers, head = sigmoid(rgb) + ReLU(sigma) (scripts/nerf.py:134-167). */
typedef struct {
    int num_layers;
    int k[LNERF_MAX_LAYERS];
    int n[LNERF_MAX_LAYERS];
    int w_k, w_n;
} lnerf_mlp;

enum {
    LNERF_INPUT_ENCODED = 0, /* x = layer_input, (rays*S, k[0]) float32 row-major          */
    LNERF_INPUT_POINTS = 1,  /* x = sample positions, (rays*S, 3) float32; the engine      */
                             /*     applies positional_encoding_3d (pos_encoding.py:38-69)  */
    LNERF_INPUT_RAYS = 2     /* x = rays, (rays, 6) float32 [origin xyz, direction xyz]; the */
                             /*     engine samples t = linspace(near, far, S), the points   */
                             /*     o + d t and dists = [diff(t), 1e8] in float64           */
                             /*     (train_nerf.py:289-306), then applies the encoding      */
};

/* One batch of rays; all pointers are device pointers. Sample r of ray i is row i*S + r
 * (train_nerf.py:327). */
typedef struct {
    int rays;
    int samples;         /* S */
    int input_mode;      /* LNERF_INPUT_* */
    int num_freqs;       /* F (POINTS mode; k[0] must equal 3 + 6F) */
    const float* x;
    const float* dists;  /* (rays, S) delta t, last = 1e8 in the reference (train_nerf.py:306); */
                         /* ignored (may be NULL) in RAYS mode                               */
    const float* target; /* (rays, 3) */
    float near_t, far_t; /* RAYS mode: sampling range (train_nerf.py: near 2, far 6)          */
} lnerf_batch;

enum {
    LNERF_SEED_CONST = 0,     /* gradients seeded with `seed`                                 */
    LNERF_SEED_LOSS = 1,      /* seeded with the batch loss itself (train_nerf.py:477)        */
    LNERF_ACCUMULATE = 2,     /* add into d_ws/d_bs (loma semantics) instead of overwriting:
                                 one fp32 add per element of the padded layout, so padded
                                 entries keep their bits (without the flag they are written
                                 +0). The other outputs are overwritten as always. Fused path
                                 only: on the generic path (LNERF_GENERIC, or a shape the fused
                                 path does not take) lnerf_train_step fails and writes nothing */
    LNERF_WANT_DX = 4,        /* also produce d_x (d_layer_input), ENCODED mode only          */
    LNERF_GENERIC = 8,        /* force the stage-by-stage loma-order kernels (no MFMA fusion) */
    LNERF_FAST = 16,          /* require the fused MFMA path (error if the shape is unsupported) */
    LNERF_TIMING = 32,        /* record per-kernel HIP events (read with lnerf_ctx_timings)   */
    LNERF_MFMA_F32 = 64,      /* removed in round 4 (the one-wave exact-f32 MFMA kernel): an
                                 error; exact fp32 arithmetic is LNERF_GENERIC                 */
    LNERF_MFMA_BF16 = 128,    /* fused path: plain bf16 operands, fp32 accumulate (one MFMA per
                                 product; reduced precision -- inference / config 5 render)   */
    LNERF_MFMA_F16X3 = 256,   /* fused path: the fp16x3 split, the fused path's default:
                                 x 2^e = hi + lo in fp16 with per-sample (k1) or per-sample
                                 balanced (k2) and per-layer weight exponent shifts, three fp16
                                 MFMAs per product, fp32 accumulate. Each product drops
                                 <= ~3 2^-22 of its operands' shifted magnitudes, i.e. relative to
                                 max|w| max|x| of the shift group (one sample's row of one layer),
                                 not to |w x| itself: an operand x scaled by 2^e keeps
                                 |x 2^e - hi - lo| <= 2^-22 |x 2^e| + 2^-25, so a value more than
                                 ~2^17 below its row's maximum loses bits to fp16's subnormals
                                 (e.g. a dW column whose G values sit 1e-9 below the row's other
                                 columns keeps ~2 % -- tests/test_gpu_edge.py fp16x3_dw_bound;
                                 LNERF_MFMA_BF16X6 has fp32's exponent range and no such limit).
                                 The head's weights carry a shift per output column and, in
                                 training, its dW runs on the bf16x6 split, so rgb and sigma
                                 adjoints far apart (delta = 1e8 rays) keep their own ranges.
                                 Training in fp16x3 keeps the activations it hands from the
                                 forward to the dW pass as int24 (x rounded to a multiple of
                                 2^-23 of its row's max|x|), inside the same row-relative bound;
                                 a row holding NaN/inf is marked and reaches dW as NaN.        */
    LNERF_MFMA_BF16X6 = 512,  /* fused path: the bf16x6 split (x = hi+mid+lo in bf16, six bf16
                                 MFMAs per product, dropped terms <= 2^-24 |w x|)              */
    LNERF_K32 = 2048,         /* removed in round 4 (it lost to k16): an error                 */
    LNERF_HEAD_FIT = 8192,    /* the mlp_fit head instead of the NeRF one (scripts/mlp_fit.py:
                                 120-145, fit_img.py:423-532): sigmoid on every output channel,
                                 loss = sum over rows x outputs of (sigmoid(z) - target)^2, no
                                 compositing. samples must be 1 (a "ray" is one row of the
                                 image), input ENCODED (rows, k[0]), target (rows, n_out) with
                                 1 <= n_out <= 4, dists unused; acc_color receives the sigmoid
                                 outputs (rows, n_out) and d_target (rows, n_out). Runs on k16
                                 in fp16x3 or bf16 only (LNERF_GENERIC / LNERF_MFMA_BF16X6 are
                                 errors).                                                      */
    LNERF_K16_W4 = 4096,      /* fused path: k16 on 4-wave, 64-sample workgroups (two per CU)
                                 instead of 8-wave, 128-sample ones (samples <= 64, fp16x3 or
                                 plain bf16, else an error; A/B -- measured slower at cfg3)     */
    LNERF_RENDER_K16 = 16384, /* lnerf_render in plain bf16: k16's forward (one 16-sample group
                                 per wave) instead of kr (lnerf_render.hip: two groups per wave,
                                 each weight fragment read from LDS feeds both; A/B)           */
    LNERF_WANT_DINPUT = 32768, /* also produce d_x as the gradient with respect to the batch's own x,
                                 in x's layout: ENCODED (rays*S, k[0]), the same code path as
                                 LNERF_WANT_DX and bit-identical to it; POINTS (rays*S, 3), the
                                 reverse of positional_encoding_3d (pos_encoding.py:38-69); RAYS
                                 (rays, 6) = [d_o, d_d], also the reverse of o + d t
                                 (train_nerf.py:289-299; the depths and dists depend only on
                                 near_t, far_t and S, so there is no dists term). On the fused
                                 path (every precision, LNERF_K16_W4) and the generic one. d_x is
                                 overwritten (also under LNERF_ACCUMULATE) and carries the seed
                                 like the other per-ray adjoints (the loss under
                                 LNERF_SEED_LOSS); a NULL d_x computes nothing. Together with
                                 LNERF_WANT_DX on non-ENCODED input: an error. lnerf_render
                                 ignores it. The encoded gradient goes through a scratch buffer
                                 the context owns (not part of lnerf_workspace_bytes); its
                                 reverse (lnerf_input_grad's kernel) runs last in the step, so
                                 lnerf_ctx_timings counts it in [4] and [5]. At most 39
                                 frequencies. An extension (no loma counterpart: the reference
                                 encodes in numpy and never differentiates it).                */
    LNERF_HASHGRID_REPRODUCIBLE = 65536, /* lnerf_hashgrid_grad only: d_table as float64 sums in a
                                 fixed order, the same bits on every call (see there)           */
    LNERF_ONE_WAVE = 1024     /* removed in round 4 (the one-wave-per-SIMD kernel pair): an error.
                                 At most one LNERF_MFMA_* precision flag may be set; any fused-
                                 path flag (LNERF_MFMA_*, LNERF_K16_W4) on a shape the fused path
                                 cannot run (a head over 16 outputs, samples over 128) is an
                                 error, as is LNERF_GENERIC together with one.                  */
};

/* Engine options (lnerf_ctx_set_option). */
enum {
    LNERF_OPT_DW_GRID = 1     /* dW kernel workgroups per step (16..4096; 0 = the default: 512 from
                                 65 536 sample rows up, samples / 128 below, at least 256)       */
};

/* Optional outputs (device pointers; any may be NULL, and so may the struct's own pointer: a NULL
 * output is never written). */
typedef struct {
    float* loss;         /* 1 float                                     */
    float* acc_color;    /* (rays, 3)                                   */
    float* d_ws;         /* (L, w_k, w_n) padded                        */
    float* d_bs;         /* (L, w_n)                                    */
    float* d_x;          /* (rays*S, k[0]) with LNERF_WANT_DX; in x's   */
                         /* own layout with LNERF_WANT_DINPUT           */
    float* d_dists;      /* (rays, S)                                   */
    float* d_target;     /* (rays, 3)                                   */
} lnerf_outputs;

const char* lnerf_last_error(void);
const char* lnerf_version(void);
/* Build fingerprint: a bitmask of the kernel objects' compile-time knobs (k1 / k2 scheduling, the
   int24 slab format, the phase-profiling build) that differ from the product build. 0 for the
   shipped library; A/B variants (Makefile defvariant / dwdefvariant) report what they moved.
   No reference counterpart (engine-only). */
unsigned lnerf_build_knobs(void);

/* A context owns the device workspace of its steps and renders (grow-only; activation slabs,
 * partials, packed weights). Every call on a context uses that one workspace, on the stream the
 * call names, so calls on one context must be ordered on the device: issue them on one stream, or
 * order the streams yourself (events) so that no two of them overlap, a reallocation for a larger
 * batch included (it frees the old block). The context's mutex orders only the host side of
 * concurrent calls. Work on different contexts is independent and may overlap on different
 * streams. The context creates no stream of its own. */
int lnerf_ctx_create(lnerf_ctx** out, int device);
void lnerf_ctx_destroy(lnerf_ctx* ctx);
/* Bytes of device workspace a train step needs (activation slabs, partials) at the default
 * LNERF_OPT_DW_GRID. */
size_t lnerf_workspace_bytes(const lnerf_mlp* mlp, int rays, int samples);
/* Bytes of its workspace the last fused lnerf_train_step / lnerf_render on `ctx` laid out (the
 * floor guard's re-run included); 0 after a generic-path call. A step whose layout
 * would pass the bytes allocated for it fails before any launch. For tests. */
size_t lnerf_ctx_workspace_used(lnerf_ctx* ctx);

/* Forward (PE + MLP + compositing + loss) and reverse pass over the MLP weights: the work of one
 * nerf_evaluate_and_march + grad_nerf_evaluate_and_march pair on the whole batch. */
int lnerf_train_step(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                     const lnerf_batch* batch, float seed, int flags, const lnerf_outputs* out,
                     void* stream);

/* get_rays (train_nerf.py:23-62) on the device: the width x width pixel grid of
 * linspace(0, 1, width) (the reference uses `width` for both axes), directions
 * [(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -1] rotated by c2w[:3,:3], origins
 * c2w[:3,3], computed in float64 and stored as float32 rays (width*width, 6) = [o, d], ready for
 * LNERF_INPUT_RAYS. K (3x3) and c2w (3x4 or the top of a 4x4, row-major) are host arrays. */
int lnerf_get_rays(int width, const double* K, const double* c2w, float* rays, void* stream);

/* The reverse of the engine's input producers applied to a caller-supplied d_encoded
 * (rays*S, 3 + 6F): the kernel LNERF_WANT_DINPUT runs. POINTS: d_input (rays*S, 3), per coordinate c
 * d_p[c] = dE[c] + sum_f 2^f (cos(2^f p_c) dE[3+6f+c] - sin(2^f p_c) dE[6+6f+c]), the reverse of
 * positional_encoding_3d (pos_encoding.py:38-69). RAYS: d_input (rays, 6) = [sum_j d_p[j],
 * sum_j t_j d_p[j]] with t = linspace(near_t, far_t, S), also the reverse of o + d t
 * (train_nerf.py:289-299). float64 arithmetic on the forward's own points and sin / cos values,
 * one rounding to float32; fixed-order sums (repeated calls give the same bits). `batch` supplies
 * x, rays, samples (no upper limit), input_mode (POINTS or RAYS only), num_freqs (0..39) and
 * near_t / far_t; target and dists are ignored and may be NULL. `scale` (nullable) is a device
 * scalar multiplied in. An extension (no loma counterpart). */
int lnerf_input_grad(const lnerf_batch* batch, const float* d_encoded, const float* scale,
                     float* d_input, void* stream);

/* The reverse of lnerf_get_rays (train_nerf.py:23-62) with respect to c2w: d_c2w (12 device
 * doubles, 3x4 row-major) from d_rays (n, 6) device floats = [d_o, d_d]:
 * d_c2w[a][3] = sum_p d_o[p][a], d_c2w[a][b] = sum_p d_d[p][a] dir_b(p) for b < 3, dir(p) the
 * float64 camera-frame direction lnerf_get_rays forms for the pixel of ray p. `pixels` is a device
 * array of n int32 indices into the width x width grid (repeats allowed); NULL means
 * n == width*width and ray p belongs to pixel p. An index outside the grid is skipped by the kernel
 * (it contributes nothing; nothing is read out of bounds and no error is reported). K (3x3) is a
 * host array. Two fixed-order float64 stages (deterministic). An extension (no loma counterpart). */
int lnerf_pose_grad(int width, const double* K, const int* pixels, int n, const float* d_rays,
                    double* d_c2w, void* stream);

/* ---- Per-ray sample depths -------------------------------------------------------------------
 * Four free functions on a stream (no context, no workspace) that turn rays plus per-ray depths
 * into what LNERF_INPUT_POINTS and lnerf_render_maps(..., sample_t, ...) accept, and back. The
 * reference samples linspace(near, far, S) only (its jitter is a TODO, train_nerf.py:289-294).
 * All arithmetic is float64 with one rounding to float32 at the store, every sum has a fixed order:
 * repeated calls give the same bits. All pointers are device pointers. An error returns a negative
 * code, sets lnerf_last_error and launches and writes nothing; rays == 0 (n == 0) succeeds and
 * launches nothing. At most 2^31 - 1 values per array. */

/* Stratified jitter of the engine's linspace: sample_t (rays, S) from u (rays, S), e.g. uniform
 * random numbers of the caller's (the library owns no generator, so results are reproducible).
 * With g = linspace(near_t, far_t, S) in float64 (the depths LNERF_INPUT_RAYS samples) and the
 * cell edges lower_j = j ? (g_{j-1} + g_j) / 2 : g_0, upper_j = j < S-1 ? (g_j + g_{j+1}) / 2 : g_{S-1}:
 * t_j = (float)(lower_j + (upper_j - lower_j) u_j), u clamped to [0, 1], a NaN taken as 0. S == 1
 * gives near_t. Non-decreasing along each ray. u == NULL is an error.
 * An extension (no loma counterpart). */
int lnerf_sample_stratified(int rays, int S, float near_t, float far_t, const float* u,
                            float* sample_t, void* stream);

/* Hierarchical (importance) sampling: n_fine depths per ray drawn from the coarse pass's weights
 * (rays, S), as lnerf_render_maps writes them, by inverting their piecewise-linear cdf.
 *   t_coarse (rays, S), non-decreasing per ray; NULL: (float)linspace(near_t, far_t, S), the depths
 * lnerf_render_maps reports for RAYS input (near_t / far_t are read only then).
 *   u (rays, n_fine), clamped as above; NULL: the deterministic u_k = (k + 0.5) / n_fine.
 *   Per ray, in float64: bin edges m_i = (t_i + t_{i+1}) / 2, i = 0..S-2; p_i = w_{i+1} + 1e-5,
 * i = 0..S-3 (the interior weights; a NaN, infinite or negative weight counts as 0); cdf_0 = 0,
 * cdf_{i+1} = (sum_{k<=i} p_k) / sum p, the last exactly 1. For each u: bin i = the largest index
 * with cdf_i <= u, at most S-3, and z = m_i + (u - cdf_i) / (cdf_{i+1} - cdf_i) (m_{i+1} - m_i),
 * rounded once to float32 (and moved one float32 inward should that rounding leave [m_0, m_{S-2}]).
 * Every output is finite and inside [m_0, m_{S-2}] whatever the weights hold.
 *   t_fine (rays, n_fine), in u's order. t_all (rays, S + n_fine): the ray's coarse and fine depths
 * merged in non-decreasing order of their float32 values (ties coarse first, then fine; equal
 * values have equal bits, so the order among them cannot be seen), i.e.
 * sort(concat(t_coarse, t_fine)) bit for bit. Either may be NULL, not both.
 *   3 <= S <= 1024 and 1 <= n_fine <= 1024. An extension (no loma counterpart). */
int lnerf_sample_importance(int rays, int S, const float* t_coarse, float near_t, float far_t,
                            const float* weights, int n_fine, const float* u, float* t_fine,
                            float* t_all, void* stream);

/* The sample points and dists of rays (n, 6) = [o, d] at per-ray depths sample_t (n, S):
 * points[i S + j][c] = (float)((double)o_c + (double)d_c (double)t_ij), (n*S, 3), and
 * dists[i][j] = (float)((double)t_{i,j+1} - (double)t_ij), the last 1e8f (train_nerf.py:306-311),
 * (n, S): ready for LNERF_INPUT_POINTS, with sample_t for lnerf_render_maps. Either output may be
 * NULL. An extension (no loma counterpart). */
int lnerf_ray_points(const float* rays, int n, int S, const float* sample_t, float* points,
                     float* dists, void* stream);

/* The reverse of lnerf_ray_points with respect to the rays: d_rays (n, 6) = [sum_j d_p[j],
 * sum_j t_ij d_p[j]] from d_points (n*S, 3) -- what LNERF_WANT_DINPUT returns for POINTS input --
 * summed in float64 in a fixed order, rounded once; feeds lnerf_pose_grad unchanged. `scale`
 * (nullable) is a device scalar multiplied in, as in lnerf_input_grad. (The depths are inputs of
 * their own: there is no gradient with respect to sample_t.) An extension (no loma counterpart). */
int lnerf_ray_points_grad(int n, int S, const float* sample_t, const float* d_points,
                          const float* scale, float* d_rays, void* stream);

/* ---- Multiresolution hash grid ----------------------------------------------------------------
 * A trainable scene representation between the sample points and the MLP: `levels` grids of
 * increasing resolution over a box, F features per grid point, each level either stored densely or
 * hashed into T = 2^log2_table entries; a point's encoding is the trilinear interpolation of its
 * cell's eight corners at every level, (R, levels * F), ready for LNERF_INPUT_ENCODED with
 * k[0] = levels * F. LNERF_WANT_DX returns d_encoded, lnerf_hashgrid_grad turns it into the
 * gradients of the table and of the points, and lnerf_ray_points_grad / lnerf_pose_grad carry the
 * latter to the camera. Free functions on a stream (no context, no workspace). An error returns a
 * negative code, sets lnerf_last_error and launches and writes nothing; R == 0 succeeds and launches
 * nothing (it does not zero d_table either). All pointers but the grid are device pointers. An
 * extension: the reference's only encoder is pos_encoding.py.
 *
 * The table is (offset[levels], F) float32 row-major: level l owns entries offset[l] ..
 * offset[l+1] - 1, of which it uses the first E_l = res[l]^3 if res[l]^3 <= T (a dense level),
 * else T (a hashed one). The struct may be filled by lnerf_hashgrid_init or by hand; the entry
 * points validate it on every call: 1 <= levels <= 32, F in {1, 2, 4, 8}, 4 <= log2_table <= 24,
 * res[l] >= 2, offset[0] >= 0, offset[l+1] - offset[l] >= E_l, hi > lo (finite) on every axis.
 * `table` must be aligned to min(16, 4 F) bytes (a row is one load up to 16 bytes).
 *
 * Per level l and coordinate c, in float64:
 *   u_c = clamp(((double)p_c - lo_c) / ((double)hi_c - lo_c), 0, 1), a NaN taken as 0;
 *   pos_c = u_c (res - 1);  i_c = min((int)floor(pos_c), res - 2);  w_c = pos_c - i_c.
 * Corner k = 0..7 has bit c of k as its offset along c: grid point g_c = i_c + bit, factor w_c if
 * the bit is set, else 1 - w_c; the corner's weight is (fx fy) fz. Its entry is
 *   dense:  g_x + res (g_y + res g_z)
 *   hashed: (g_x ^ g_y 2654435761u ^ g_z 805459861u) & (T - 1)   in uint32
 * so every index is below E_l whatever the point holds (clamp first, hash after). */
#define LNERF_HASHGRID_MAX_LEVELS 32
typedef struct {
    int levels;                                      /* 1..32 */
    int features;                                    /* F in {1, 2, 4, 8} */
    int log2_table;                                  /* T = 2^log2_table, 4..24 */
    int res[LNERF_HASHGRID_MAX_LEVELS];              /* grid points per axis, >= 2 */
    long long offset[LNERF_HASHGRID_MAX_LEVELS + 1]; /* level l's first entry; [levels] = total */
    float lo[3], hi[3];                              /* the box; hi > lo */
} lnerf_hashgrid;

/* Host only (needs no device): fills *grid and returns the total number of entries, offset[levels],
 * or a negative code (*grid is then untouched). res[l] = floor(base_res b^l + 0.5) in double with
 * b = exp(ln(max_res / base_res) / (levels - 1)) (levels == 1: res[0] = base_res); 2 <= base_res <=
 * max_res. offset[0] = 0 and each level's E_l is rounded up to a multiple of 4, so that every
 * level's rows stay 16-byte aligned at F = 1. lo, hi: 3 host floats each. */
long long lnerf_hashgrid_init(lnerf_hashgrid* grid, int levels, int features, int log2_table,
                              int base_res, int max_res, const float* lo, const float* hi);

/* encoded[r][l F + f] = (float) sum_{k=0..7} weight_k (double)table[offset_l + entry_k][f] for
 * points (R, 3): float64 products (no FMA contraction) summed in the order of k from 0, rounded to
 * float32 once; repeated calls give the same bits. A point outside the box encodes as the nearest
 * point of the box, a NaN coordinate as lo_c. R <= 2^39. */
int lnerf_hashgrid_encode(const lnerf_hashgrid* grid, const float* table, const float* points,
                          long long R, float* encoded, void* stream);

/* The reverse of lnerf_hashgrid_encode from d_encoded (R, levels * F). `scale` (nullable) is a
 * device scalar multiplied in; `flags` is 0, LNERF_ACCUMULATE, LNERF_HASHGRID_REPRODUCIBLE or both.
 * Either output may be NULL, both NULL is an error; `table` may be NULL when d_points is.
 *   d_table (offset[levels], F): d_table[offset_l + entry_k][f] += (float)(scale weight_k
 * d_encoded[r][l F + f]) over every row, level and corner; cells that collide in a hashed level sum.
 * Without LNERF_ACCUMULATE the call first zeroes all offset[levels] * F values on the stream (entries
 * no sample touches are +0); with it the call adds into what is there and untouched entries keep
 * their bits. In the default mode d_table is summed with float32 atomic adds (within a wave, adjacent
 * rows that share an entry are added together first; small dense levels are summed per workgroup in
 * LDS): its last bits depend on arrival order, so the default mode of d_table is not bit-reproducible
 * from call to call -- the one output of this library that is not, unlike d_points and encoded --
 * and under LNERF_HASHGRID_REPRODUCIBLE (below) it is. In the default mode an entry that receives n
 * terms is within
 *     2^-23 |exact| + (n + 2) 2^-24 sum |term|
 * of the exact sum (one float32 rounding per term and at most n float32 adds, in any order).
 *   LNERF_HASHGRID_REPRODUCIBLE changes how d_table is formed and nothing else (d_points has the
 * same bits with and without it; with d_table == NULL it is accepted and takes no scratch). For
 * entry e of level l and feature f, a term is
 *     t(r, k, f) = ((double)scale weight_k(r)) (double)d_encoded[r][l F + f]
 * with the encoder's float64 weight (fx fy) fz: two float64 products in that order, no contraction,
 * not rounded to float32. The terms of the contributions (r, k) whose corner maps to e, taken in
 * ascending contribution id c = 8 r + k as t_0 .. t_{n-1}, are summed in float64 in this order:
 *     partial_q = ((+0 + t_{8q}) + t_{8q+1}) + ... + t_{min(8q+7, n-1)}     q = 0 .. ceil(n / 8) - 1
 *     sum       = ((+0 + partial_0) + partial_1) + ...
 * i.e. runs of eight consecutive positions of the entry's ascending-c list, then the partial sums in
 * ascending order (n <= 8: the plain sequential sum). The order depends on that list alone, never on
 * launch geometry, the number of compute units, arrival order or timing. Then d_table[e][f] =
 * (float)sum, or under LNERF_ACCUMULATE d_table[e][f] + (float)sum (one float32 add). An entry that
 * receives no term is +0 without LNERF_ACCUMULATE; with it the entry is skipped and keeps its bits
 * (a held -0 stays -0). A NaN or infinity in a row's d_encoded reaches exactly that row's entries,
 * as in the default mode. The same inputs give the same bits on every call, stream and device of
 * this kind; the result is within
 *     2^-24 |exact| + 2^-149 + (n + 1) 2^-52 sum |term|
 * of the exact sum (one float32 rounding; n float64 products and adds). No float atomics: per level
 * a stable radix sort brings each entry's ids together (keys: the entry indices, ceil(log2 E_l)
 * bits) and a segmented float64 sum writes one row per touched entry. R <= 2^28 under the flag (a
 * contribution id must fit 32 bits; more is an error and nothing is launched or written) and d_table
 * must be aligned like `table`, to min(16, 4 F) bytes (rows are stored whole). Scratch comes from
 * the stream's memory pool for the duration of the call (hipMallocAsync / hipFreeAsync on `stream`):
 * 192 bytes per row -- per contribution two 4-byte keys, two 4-byte ids and one float64 factor,
 * one level at a time, so independent of `levels` -- plus the sort's own temporary storage;
 * lnerf_hashgrid_grad_scratch returns the exact count.
 *   d_points (R, 3): d_points[r][c] = (float)(scale sum_l ((sum_f d_encoded[r][l F + f]
 * (sum_k (d weight_k / d pos_c) table_k[f])) (res_l - 1) / (hi_c - lo_c))), d weight_k / d pos_x =
 * +- fy fz (+ where bit x of k is set), likewise y and z; float64 in that fixed order, rounded once:
 * repeated calls give the same bits. It is exactly 0 for a coordinate the clamp moved (outside the
 * box; a coordinate on lo_c or hi_c itself counts as inside) and for a NaN. */
int lnerf_hashgrid_grad(const lnerf_hashgrid* grid, const float* table, const float* points,
                        long long R, const float* d_encoded, const float* scale, int flags,
                        float* d_table, float* d_points, void* stream);

/* The bytes an lnerf_hashgrid_grad call with LNERF_HASHGRID_REPRODUCIBLE, a d_table and R rows takes
 * from the stream's memory pool while it runs (0 for R == 0), or a negative code. Needs a device
 * (the sort sizes its temporary storage for it); launches and writes nothing. R <= 2^28. */
long long lnerf_hashgrid_grad_scratch(const lnerf_hashgrid* grid, long long R, void* stream);

/* ---- Occupancy grid ---------------------------------------------------------------------------
 * Where the scene is empty, known without a network evaluation: a coarse grid of res^3 cells over
 * a box that keeps a decayed running maximum of sigma per cell (`density`), its threshold packed
 * into a bitfield (`bits`), and a sampler that marches each ray over the bitfield in M fixed steps
 * and spreads the S samples over the occupied steps alone. The caller evaluates sigma at points
 * inside cells (lnerf_occgrid_cell_points, then e.g. lnerf_render_maps' rgba), folds it in
 * (lnerf_occgrid_update), thresholds (lnerf_occgrid_threshold) and samples (lnerf_sample_occupancy);
 * lnerf_ray_points (points only) and LNERF_INPUT_POINTS / ENCODED with the sampler's dists and
 * sample_t take it from there. Free functions on a stream (no context, no workspace). The struct is
 * validated on every call. An error returns a negative code, sets lnerf_last_error and launches and
 * writes nothing; n == 0 succeeds and launches nothing (lnerf_occgrid_update then skips the decay
 * too). All pointers but the grid are device pointers. All arithmetic is float64 or integer, with one
 * rounding to float32 at a store, and the only atomics are integer ones (a maximum, a count): every
 * output has the same bits on every call. An extension: the reference samples linspace only
 * (train_nerf.py:289-306).
 *
 * Cell (gx, gy, gz) has index c = gx + res (gy + res gz). `density` is res^3 float32, non-negative
 * and finite (start from zeros); every call keeps that. `bits` is res^3 / 32 uint32: cell c is bit
 * c & 31 of word c >> 5. */
typedef struct {
    int res;            /* cells per axis: a power of two, 4..256 (res^3 is a multiple of 64) */
    float lo[3], hi[3]; /* the box; hi > lo, finite */
} lnerf_occgrid;
enum { LNERF_OCC_MEAN = 1, LNERF_OCC_LAST_OPAQUE = 2 };

/* points (n, 3) inside the cells `cells` (n): p_c = (float)(lo_c + (g_c + u_c) / res (hi_c - lo_c))
 * in float64 in that order, rounded once, with u (n, 3) clamped to [0, 1] and a NaN taken as 0 (the
 * caller's random numbers); u == NULL means 0.5, the cell centre. cells == NULL means cell i is i
 * and needs n == res^3. An index outside 0..res^3-1 gives the box centre (float)(lo_c + 0.5 (hi_c -
 * lo_c)); lnerf_occgrid_update skips it. n <= 2^39. */
int lnerf_occgrid_cell_points(const lnerf_occgrid* grid, const int* cells, long long n, const float* u,
                              float* points, void* stream);

/* The decayed running maximum. First every cell of `density` is multiplied by `decay` (float32, once
 * per call; 0 <= decay <= 1, decay == 1 skips the pass). Then for i < n: density[cell_i] =
 * max(density[cell_i], s_i) with s_i = sigma[i sigma_stride] (sigma_stride >= 1; 4 with sigma = rgba
 * + 3 reads lnerf_render_maps' rgba in place). A NaN or a value <= 0 is ignored, +inf counts as
 * FLT_MAX. cells as above (NULL: n == res^3); an index outside the grid is skipped; duplicate cells
 * take the maximum (an integer atomic maximum on the float's bits: exact in any order). */
int lnerf_occgrid_update(const lnerf_occgrid* grid, float* density, const int* cells, long long n,
                         const float* sigma, int sigma_stride, float decay, void* stream);

/* bits: bit c = (double)density[c] > thr with thr = threshold, or min(threshold, mean(density)) under
 * LNERF_OCC_MEAN (the only flag). The mean is a float64 sum in two fixed-order stages divided by
 * res^3, so it has the same bits on every call; a cell within res^3 2^-52 mean of the mean may fall
 * on either side of what another summation order decides. *mean (that mean, whatever the flag) and
 * *occupied (the number of set bits, exact) are nullable device scalars; bits is nullable too
 * (statistics only); all three NULL is an error, and so is a NaN threshold. */
int lnerf_occgrid_threshold(const lnerf_occgrid* grid, const float* density, float threshold, int flags,
                            unsigned* bits, double* mean, long long* occupied, void* stream);

/* Empty-space-skipping sample depths for rays (n, 6) = [o, d]: sample_t (n, S), dists (n, S) and
 * n_occ (n), each nullable, not all three. steps = M, a multiple of 64 in 64..1024; 1 <= S <= 1024;
 * far_t > near_t, both finite; u (n, S) clamped as above, NULL means 0.5; flags is 0 or
 * LNERF_OCC_LAST_OPAQUE. n S <= 2^31 - 1. Per ray, in float64 with no FMA contraction:
 *   h = ((double)far_t - (double)near_t) / M; step i has the midpoint c_i = near_t + (i + 0.5) h and
 * the point p = (double)o + (double)d c_i; w_c = (p_c - lo_c) / ((double)hi_c - lo_c). Step i is
 * occupied if 0 <= w_c < 1 on all three axes (a NaN fails) and the bit of the cell g_c =
 * min((int)(w_c res), res - 1) is set. N = the number of occupied steps, written to n_occ. If
 * N == 0 the ray is sampled as if every step were occupied (N' = M, else N' = N); n_occ still
 * reports 0, so the caller can mask the ray.
 *   Sample j: q = ((double)j + u_j) N' / S, k = min((long long)q, N' - 1), f = q - k, i = the index of
 * the k-th occupied step counting from 0, t_j = (float)(near_t + (i + f) h). The depths are
 * non-decreasing along a ray and each lies in an occupied step (to the one rounding).
 *   dists_j = (float)(N' h / S) for every j -- each sample stands for an equal share of the occupied
 * length; it is NOT the difference to the next sample, which would span the gaps -- and under
 * LNERF_OCC_LAST_OPAQUE the last one is 1e8f, the reference's convention (train_nerf.py:306).
 *   Every index depends on integer counts alone; the only floating-point values that reach a
 * comparison are u and the cell test. */
int lnerf_sample_occupancy(const lnerf_occgrid* grid, const unsigned* bits, const float* rays, int n,
                           int S, int steps, float near_t, float far_t, const float* u, int flags,
                           float* sample_t, float* dists, int* n_occ, void* stream);

/* Forward only (eval render, train_nerf.py:616-661, which always has a target image): acc_color
 * and the loss against batch->target. batch->target is required (NULL: an error, nothing is
 * launched or written); the loss is always computed and written to out->loss unless that is NULL.
 * The gradient outputs are ignored. */
int lnerf_render(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                 const lnerf_batch* batch, int flags, const lnerf_outputs* out, void* stream);

/* Render maps: lnerf_render's forward with the standard outputs of a volume renderer beside the
 * colour, and no need for a target. An extension: the reference computes the per-sample arrays
 * (img_sample_rgba_arr, weights_samples) but never a depth or an opacity.
 *   w_j are the reference's own compositing weights, alpha_j T_j with its INCLUSIVE transmittance
 * (nerf.py:226-272: T_0 = 1, T_j = P_j = prod_{i<=j} (1 - alpha_i + 1e-10) for j >= 1), the
 * weights acc_color is summed with. So opacity = sum_j w_j stays below 1 even on an opaque ray
 * (sample j >= 1 is attenuated by its own alpha too), and a ray's last sample (delta = 1e8 in the
 * reference, alpha = 1 wherever sigma > 0) contributes about 1e-10: the maps are consistent with
 * the colour the engine returns, not with the textbook exclusive transmittance. depth is not
 * divided by the opacity. depth, opacity and acc_color are fp32 segmented sums in one order (the
 * fused kernels' scans; the generic path sums sequentially in j).
 *   t_j: in RAYS mode (float)linspace(near_t, far_t, S)[j], the depths the engine samples at;
 * sample_t must be NULL there. In POINTS / ENCODED mode sample_t is a device (rays, S) float array;
 * asking for depth without it is an error, and nothing else reads it.
 *   batch->target may be NULL: no loss is computed then, and a non-NULL out->loss is an error.
 * With a target the loss is lnerf_render's, and acc_color is lnerf_render's bit for bit under the
 * same flags. Any output pointer may be NULL, and so may `out`: a NULL output is never written. An
 * error launches nothing and writes nothing. Flags as lnerf_render (the LNERF_MFMA_* precisions,
 * LNERF_RENDER_K16, LNERF_K16_W4, LNERF_GENERIC, LNERF_FAST, LNERF_TIMING); LNERF_HEAD_FIT is an
 * error. Shapes the fused path does not take (samples > 128, a head over 16 outputs) run the
 * generic path, which has no limit on samples. lnerf_ctx_last_path reports the kernels' bits plus
 * LNERF_PATH_MAPS; the other lnerf_ctx_* queries behave as after lnerf_render. The maps go straight
 * to the caller's buffers: no workspace beyond lnerf_render's. */
typedef struct {
    float* acc_color;  /* (rays, 3)                                                 */
    float* depth;      /* (rays)      sum_j w_j t_j  (not divided by opacity)       */
    float* opacity;    /* (rays)      sum_j w_j                                     */
    float* weights;    /* (rays, S)   w_j = alpha_j T_j, the weights the colour uses */
    float* rgba;       /* (rays*S, 4) sigmoid(rgb), ReLU(sigma): the reference's
                          img_sample_rgba_arr; 16-byte aligned                      */
    float* loss;       /* 1 float; only with batch->target                          */
} lnerf_render_outputs;

int lnerf_render_maps(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                      const lnerf_batch* batch, const float* sample_t, int flags,
                      const lnerf_render_outputs* out, void* stream);

/* The reverse of lnerf_render_maps: the vector-Jacobian product of the render with the caller's
 * adjoints of its maps, for any loss on colour, depth, opacity, sample weights and rgba (depth
 * supervision, a mask loss, a white background C + (1 - O) bg, a regulariser on the weights, a robust
 * colour loss, ...). An extension (the reference reverses its sum-of-squares colour loss only).
 *   One call recomputes the forward exactly as lnerf_train_step does and reverses it from the
 * adjoints. With t_j as in lnerf_render_maps, each sample's reverse is seeded with
 *     dw_j     = rgb_j . d_acc_color + t_j d_depth + d_opacity + d_weights_j
 *     drgb_j   = w_j d_acc_color + d_rgba_j[0..2]
 *     dsigma_j += d_rgba_j[3]     (before the ReLU gate sigma > 0: rgba's sigma is the post-ReLU value)
 * and everything after that -- the transmittance reverse, the alpha reverse, the head and the MLP's
 * reverse chain, dW / db, the fp16x3 floor guard and its re-run, the exceptional rows -- is
 * lnerf_train_step's. With d_acc_color = 2 (acc_color - target) and no other adjoint every output has
 * lnerf_train_step's bits at LNERF_SEED_CONST, seed 1. A NULL adjoint's term is never formed (no
 * 0 * x): a NaN or an infinity in t or rgb cannot leak through an adjoint that was not given, and the
 * other terms keep their bits. All five NULL is an error. The seed is 1: the adjoints carry any scale.
 *   Writes out->d_ws, d_bs, d_dists and, under LNERF_WANT_DX / LNERF_WANT_DINPUT, d_x (layouts and
 * rules of lnerf_train_step), and out->acc_color, the recomputed colour (lnerf_train_step's bit for
 * bit). batch->target is ignored and may be NULL; a non-NULL out->loss or out->d_target is an error.
 * `out` and every output pointer may be NULL.
 *   sample_t: NULL in RAYS mode (t_j = (float)linspace(near_t, far_t, S)[j]); in POINTS / ENCODED
 * mode required with d_depth and not read otherwise. There is no gradient with respect to sample_t
 * here: it is w_j d_depth per sample, which the caller forms from lnerf_render_maps' weights.
 *   Flags: the default precision (fp16x3 with the floor guard), LNERF_MFMA_F16X3, LNERF_MFMA_BF16X6,
 * LNERF_MFMA_BF16, LNERF_GENERIC, LNERF_FAST, LNERF_TIMING, LNERF_ACCUMULATE (fused path only),
 * LNERF_WANT_DX, LNERF_WANT_DINPUT. LNERF_SEED_LOSS, LNERF_HEAD_FIT, LNERF_K16_W4 and
 * LNERF_RENDER_K16 are errors. Shapes the fused path does not take (samples > 128, a head over 16
 * outputs) run the generic path, which has no limit on samples. An error launches nothing and writes
 * nothing. Afterwards lnerf_ctx_relu_masks, _exceptional_rows, _guard_fired, _timings and
 * _workspace_used behave as after a training step, and lnerf_ctx_last_path reports the training
 * step's bits plus LNERF_PATH_VJP. */
typedef struct {               /* device pointers, each nullable; all NULL is an error */
    const float* d_acc_color;  /* (rays, 3)    */
    const float* d_depth;      /* (rays)       */
    const float* d_opacity;    /* (rays)       */
    const float* d_weights;    /* (rays, S)    */
    const float* d_rgba;       /* (rays*S, 4), 16-byte aligned */
} lnerf_render_adjoints;

int lnerf_render_maps_vjp(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                          const lnerf_batch* batch, const float* sample_t,
                          const lnerf_render_adjoints* adj, int flags, const lnerf_outputs* out,
                          void* stream);

/* Per-kernel times (ms) of the last LNERF_TIMING step or render on `ctx`, measured with HIP events
 * on its stream: [0] weight pack, [1] fused fwd+reverse-chain kernel (a render: the forward
 * kernel), [2] loss reduce, [3] dW kernel, [4] dW/db reduce (with LNERF_WANT_DINPUT also the
 * input-gradient kernel), [5] whole step (0 for the kernels a
 * render does not run). Synchronises on the step. Returns the number
 * of values written (0 if no timed step ran on the fused path). */
int lnerf_ctx_timings(lnerf_ctx* ctx, float* ms_out, int n);

/* Which kernels the last lnerf_train_step / lnerf_render on `ctx` ran (for tests and benches):
 * a mask of LNERF_PATH_* bits, the operand planes of the fused MFMAs in bits 8-9 (3 = bf16x6
 * split, 2 = fp16x3 split, 1 = plain bf16, 0 = the generic path), or a negative
 * error code. 0 if no step has run. */
enum {
    LNERF_PATH_GENERIC = 1,   /* the loma-order stage-by-stage kernels                        */
    LNERF_PATH_FUSED = 2,     /* the fused MFMA step (k16, + dw16 when training)              */
    LNERF_PATH_K16 = 4,       /* fused kernel on wave pairs (k16_fwd_bwd_kernel)              */
    LNERF_PATH_DW16 = 8,      /* dW kernel on wave pairs (dw16_kernel)                        */
    LNERF_PATH_K32 = 16,      /* reserved (k32, removed in round 4)                           */
    LNERF_PATH_K16_W4 = 32,   /* k16 on 4-wave, 64-sample workgroups (two per CU)             */
    LNERF_PATH_KR = 64,       /* the render ran kr (lnerf_render.hip), not k16's forward      */
    LNERF_PATH_A24 = 128,     /* training kept the activation slabs as int24 (fp16x3)         */
    LNERF_PATH_MAPS = 1024,   /* lnerf_render_maps: the MAPS instantiations (bits 8-9: planes)  */
    LNERF_PATH_VJP = 2048     /* lnerf_render_maps_vjp: the training step's bits plus this one  */
};
int lnerf_ctx_last_path(lnerf_ctx* ctx);

/* The hidden-layer ReLU decisions of the last training step on `ctx` (k16 path only, for parity
 * tests: scripts/nerf.py:141-144 takes z > 0): `out` (device) receives (L-1) x R x 32 bytes, bit
 * f % 8 of byte [(l R + r) 32 + f / 8] set when feature f of hidden layer l at sample row r was
 * positive. Valid until the next call on `ctx`; an error after any other kind of call. A head-only
 * MLP (L = 1) has no hidden layer: the call succeeds and writes nothing (`out` may be NULL). */
int lnerf_ctx_relu_masks(lnerf_ctx* ctx, unsigned char* out, size_t out_bytes, void* stream);

/* The exceptional rows of the last training step on `ctx` (k16 + dw16 with the fp16x3 split): the
 * sample rows, summed over the layers, that dw16 multiplied on the bf16x6 split instead of the
 * fp16x3 one because fp16's range at their balanced shift could not keep every nonzero element to
 * 2^-17 (every ray's last sample always is one; lnerf_internal.h kXrowT); *last_samples (nullable)
 * receives how many of them were rays' last samples. 0 for the other precisions. Synchronises the
 * device. An extension (no loma counterpart). */
int lnerf_ctx_exceptional_rows(lnerf_ctx* ctx, long long* rows, long long* last_samples);

/* The fp16x3 floor guard of the last training step on `ctx`: *fired = 1 if k1 met a hidden-layer
 * gradient element below what the fp16x3 split can carry (more than ~2^37 below its row's maximum,
 * lnerf_internal.h kGuardExp) and the step was therefore re-run on the device on the bf16x6 split
 * (every output of the step comes from that re-run), 0 if not, -1 if the last call on `ctx` had no
 * guard (a training step with an explicit precision flag, the generic path, LNERF_HEAD_FIT or
 * LNERF_K16_W4; a render). Synchronises the device. An extension (no loma counterpart). */
int lnerf_ctx_guard_fired(lnerf_ctx* ctx, int* fired);

/* Sets an engine option (LNERF_OPT_*) for later steps on `ctx`. Returns 0, or a negative code for
 * an unknown option or an out-of-range value. */
int lnerf_ctx_set_option(lnerf_ctx* ctx, int option, int value);

/* buf[i] *= *scale for i < n (device pointers): applies a loss seed after an all-reduce of
 * unit-seeded gradients (the data-parallel path). */
int lnerf_scale_by_device_scalar(float* buf, size_t n, const float* scale, void* stream);

/* The reference's Adam (train_nerf.py:133-161) on device: params -= lr_t m_hat/(sqrt(v_hat)+eps).
 * `t` is the 1-based step count after the increment. */
int lnerf_adam_update(float* params, const float* grads, float* m, float* v, size_t n, int t,
                      float lr, float beta1, float beta2, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LNERF_H */
