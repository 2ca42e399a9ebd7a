// lnerf_api.cpp -- the C ABI of libloma_nerf.so (declared in include/lnerf.h).
//
// loma-compat entry points: the reference passes nested host pointer tables built by
// mlp_utils.convert_ndim_array_to_ndim_ctypes (mlp_utils.py:33-118). We read exactly the elements
// the reference's loops touch (extents derived from the same loop bounds), gather them into one
// pinned staging block, run the loma-order HIP kernels (lnerf_generic.hip) on the calling
// thread's stream, and scatter the mutated buffers back. No CPU compute path exists: if the HIP
// runtime or device is unavailable the call fails loudly (NaN / error string).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <sys/syscall.h>
#include <unistd.h>

#include "lnerf_hashgrid.h"
#include "lnerf_occgrid.h"
#include "lnerf_internal.h"

using namespace lnerf;

namespace {

thread_local std::string g_last_error;

using marshal::fail;
using namespace marshal;

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) fail("%s failed: %s", #expr, hipGetErrorString(_e));          \
    } while (0)

void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) fail("%s: kernel launch failed: %s", what, hipGetErrorString(e));
}

// Grow-only device / pinned buffers.
struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    void* get(size_t bytes) {
        if (bytes > n) {
            if (p) HIP_OK(hipFree(p));
            p = nullptr;
            n = 0;
            HIP_OK(hipMalloc(&p, bytes));
            n = bytes;
        }
        return p;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
struct HostBuf {
    void* p = nullptr;
    size_t n = 0;
    void* get(size_t bytes) {
        if (bytes > n) {
            if (p) HIP_OK(hipHostFree(p));
            p = nullptr;
            n = 0;
            HIP_OK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
            n = bytes;
        }
        return p;
    }
    ~HostBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// Per-thread engine state for the loma-compat ABI (ctypes drops the GIL, so calls may come from
// several threads at once; each gets its own stream and staging).
struct CompatCtx {
    hipStream_t stream = nullptr;
    DevBuf dev;
    HostBuf host;
    CompatCtx() {
        int n = 0;
        HIP_OK(hipGetDeviceCount(&n));
        if (n < 1) fail("no HIP device visible");
        HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    ~CompatCtx() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};
// One CompatCtx per calling thread, freed when that thread exits (its stream and staging go with
// it). The main thread's context is left to process teardown: at exit() its thread_local
// destructor may run after the HIP runtime has begun shutting down, where hipStreamDestroy is
// not safe. The main thread is the one whose kernel thread id is the process id (whichever
// thread happened to load the library).
bool on_main_thread() { return (pid_t)syscall(SYS_gettid) == getpid(); }
struct CompatHolder {
    CompatCtx* ctx = nullptr;
    ~CompatHolder() {
        if (ctx && !on_main_thread()) delete ctx;
    }
};
thread_local CompatHolder tl_compat;
CompatCtx& compat() {
    if (!tl_compat.ctx) tl_compat.ctx = new CompatCtx();
    return *tl_compat.ctx;
}

// Carves one contiguous region into float arrays (same offsets on host and device).
struct Carve {
    size_t off = 0;
    size_t take(size_t nfloats) {
        size_t o = off;
        off += (nfloats + 63) / 64 * 64;
        return o;
    }
};

struct Offsets {
    size_t X, W, B, T, IO, rgba, dists, alpha, cp, wsamp, acc, loss, seed;
    size_t zpre, cpC, cpP;
    size_t dX, dW, dB, dT, dIO, drgba, ddists, dalpha, dcp, dwsamp, dacc;
    size_t total;
};

Offsets carve(const CallShape& c, bool grad) {
    const LgDims& d = c.d;
    Carve k;
    Offsets o{};
    const size_t nS = (size_t)d.th * d.S;
    o.X = k.take((size_t)d.in_h * d.x_cols);
    o.W = k.take((size_t)d.L * d.w_k * d.w_n);
    o.B = k.take((size_t)d.L * d.b_n);
    o.T = k.take((size_t)d.th * d.t_cols);
    o.IO = k.take((size_t)d.L * d.io_rows * d.io_cols);
    o.rgba = k.take(nS * 4);
    o.dists = k.take(nS);
    o.alpha = k.take(nS);
    o.cp = k.take(nS);
    o.wsamp = k.take(nS);
    o.acc = k.take((size_t)d.th * d.acc_cols);
    o.loss = k.take(1);
    o.seed = k.take(1);
    if (grad) {
        o.zpre = k.take((size_t)d.L * d.io_rows * d.io_cols);
        o.cpC = k.take(nS);
        o.cpP = k.take(nS);
        o.dX = k.take((size_t)d.in_h * d.x_cols);
        o.dW = k.take((size_t)d.L * d.w_k * d.w_n);
        o.dB = k.take((size_t)d.L * d.b_n);
        o.dT = k.take((size_t)d.th * d.t_cols);
        o.dIO = k.take((size_t)d.L * d.io_rows * d.io_cols);
        o.drgba = k.take(nS * 4);
        o.ddists = k.take(nS);
        o.dalpha = k.take(nS);
        o.dcp = k.take(nS);
        o.dwsamp = k.take(nS);
        o.dacc = k.take((size_t)d.th * d.acc_cols);
    }
    o.total = k.off;
    return o;
}

LgBuffers dev_buffers(float* base, const Offsets& o, bool grad) {
    LgBuffers b{};
    b.X = base + o.X;
    b.W = base + o.W;
    b.B = base + o.B;
    b.T = base + o.T;
    b.IO = base + o.IO;
    b.rgba = base + o.rgba;
    b.dists = base + o.dists;
    b.alpha = base + o.alpha;
    b.cp = base + o.cp;
    b.wsamp = base + o.wsamp;
    b.acc = base + o.acc;
    if (grad) {
        b.zpre = base + o.zpre;
        b.cpC = base + o.cpC;
        b.cpP = base + o.cpP;
    }
    return b;
}
LgAdjoints dev_adjoints(float* base, const Offsets& o, bool want_dx) {
    LgAdjoints a{};
    a.dX = want_dx ? base + o.dX : nullptr;
    a.dW = base + o.dW;
    a.dB = base + o.dB;
    a.dT = base + o.dT;
    a.dIO = base + o.dIO;
    a.drgba = base + o.drgba;
    a.ddists = base + o.ddists;
    a.dalpha = base + o.dalpha;
    a.dcp = base + o.dcp;
    a.dwsamp = base + o.dwsamp;
    a.dacc = base + o.dacc;
    return a;
}

// The nested pointer tables of one side of a loma call: the primal arguments, or their adjoints (the
// d_ arguments). The NeRF tables are null in an mlp_fit call.
struct LomaTables {
    float **x, ***ws, **bs, **target, ***io;
    float ***rgba, **dists, **alpha, **cp, **wsamp, **acc;
};

// The adjoint tables into the staging block (the device accumulates into them) or back out of it.
template <bool Out>
void move_adjoints(float* h, const Offsets& o, const CallShape& c, const LomaTables& t, bool nerf, bool want_dx) {
    const LgDims& d = c.d;
    auto rect = [&](float** tab, size_t off, int rows, int cols, int ld) {
        if (Out) scatter2(tab, h + off, rows, cols, ld);
        else gather2(h + off, tab, rows, cols, ld);
    };
    if (want_dx) rect(t.x, o.dX, d.in_h, d.in_w, d.x_cols);
    if (Out) scatter_w(t.ws, h + o.dW, c);
    else gather_w(h + o.dW, t.ws, c);
    if (Out) scatter_b(t.bs, h + o.dB, c);
    else gather_b(h + o.dB, t.bs, c);
    rect(t.target, o.dT, d.th, d.tw, d.t_cols);
    if (Out) scatter_io(t.io, h + o.dIO, c);
    else gather_io(h + o.dIO, t.io, c);
    if (!nerf) return;
    if (d.th > 0 && d.S > 0) {
        if (Out) scatter3(t.rgba, h + o.drgba, d.th, d.S, 4);
        else gather3(h + o.drgba, t.rgba, d.th, d.S, 4);
        rect(t.dists, o.ddists, d.th, d.S, d.S);
        rect(t.alpha, o.dalpha, d.th, d.S, d.S);
        rect(t.cp, o.dcp, d.th, d.S, d.S);
        rect(t.wsamp, o.dwsamp, d.th, d.S, d.S);
    }
    rect(t.acc, o.dacc, d.th, d.acc_cols, d.acc_cols);
}

// One compat call, nerf_evaluate_and_march (nerf) or mlp_fit, or with adj its grad_ form: the primal
// tables (and the seed and the adjoint tables) gathered into the pinned block, uploaded, the loma-order
// kernels run on the device block, what the call mutates downloaded and scattered back. A forward
// call returns the loss.
float stage_call(const char* what, bool nerf, const CallShape& c, const LomaTables& in, const LomaTables* adj,
                 float seed) {
    const LgDims& d = c.d;
    const bool grad = adj != nullptr, S_ok = d.th > 0 && d.S > 0;
    const Offsets o = carve(c, grad);
    CompatCtx& cx = compat();
    float* h = (float*)cx.host.get(o.total * sizeof(float));
    float* g = (float*)cx.dev.get(o.total * sizeof(float));
    std::memset(h, 0, o.total * sizeof(float));
    // primal inputs (a grad call re-executes the forward on them; the rest is overwritten before use)
    gather2(h + o.X, in.x, d.in_h, d.in_w, d.x_cols);
    gather_w(h + o.W, in.ws, c);
    gather_b(h + o.B, in.bs, c);
    gather2(h + o.T, in.target, d.th, d.tw, d.t_cols);
    gather_io(h + o.IO, in.io, c);
    if (nerf) {
        if (!grad || S_ok) gather2(h + o.dists, in.dists, d.th, d.S, d.S);
        gather2(h + o.acc, in.acc, d.th, d.acc_cols, d.acc_cols);
    }
    const bool want_dx = grad && adj->x != nullptr;
    if (grad) {
        h[o.seed] = seed;
        move_adjoints<false>(h, o, c, *adj, nerf, want_dx);
    }
    HIP_OK(hipMemcpyAsync(g, h, o.total * sizeof(float), hipMemcpyHostToDevice, cx.stream));
    if (!grad) (nerf ? lg_nerf_forward : lg_mlp_fit_forward)(d, dev_buffers(g, o, false), g + o.loss, cx.stream);
    else if (nerf) lg_nerf_grad(d, dev_buffers(g, o, true), dev_adjoints(g, o, want_dx), g + o.seed, cx.stream);
    else lg_mlp_fit_grad(d, dev_buffers(g, o, true), dev_adjoints(g, o, want_dx), g + o.seed, cx.stream);
    check_launch(what);
    // forward: everything from IO to the loss is contiguous in the carve; grad: the adjoints end it
    const size_t lo = grad ? o.dX : o.IO, hi = grad ? o.total : o.seed;
    HIP_OK(hipMemcpyAsync(h + lo, g + lo, (hi - lo) * sizeof(float), hipMemcpyDeviceToHost, cx.stream));
    HIP_OK(hipStreamSynchronize(cx.stream));
    if (grad) {
        move_adjoints<true>(h, o, c, *adj, nerf, want_dx);
        return 0.0f;
    }
    scatter_io(in.io, h + o.IO, c);
    if (nerf) {
        if (S_ok) {
            scatter3(in.rgba, h + o.rgba, d.th, d.S, 4);
            scatter2(in.alpha, h + o.alpha, d.th, d.S, d.S);
            scatter2(in.cp, h + o.cp, d.th, d.S, d.S);
            scatter2(in.wsamp, h + o.wsamp, d.th, d.S, d.S);
        }
        scatter2(in.acc, h + o.acc, d.th, 3, d.acc_cols);
    }
    return h[o.loss];
}

template <class F>
float guard_float(F&& f) {
    try {
        g_last_error.clear();
        return f();
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return std::numeric_limits<float>::quiet_NaN();
    }
}
template <class F>
int guard_int(F&& f) {
    try {
        g_last_error.clear();
        f();
        return 0;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return -1;
    }
}

}  // namespace

// =============================================================================================
// loma-compat ABI
// =============================================================================================
extern "C" float nerf_evaluate_and_march(float** layer_input, int layer_input_h, int layer_input_w,
                                         float*** ws, float** bs, float** target_image,
                                         int target_image_h, int target_image_w, int num_weights,
                                         int** weight_shapes, int** bias_shapes,
                                         int** intermediate_output_shapes,
                                         float*** intermediate_outputs,
                                         float*** img_sample_rgba_arr, int num_samples,
                                         float** dists, float** alpha, float** cumprod_alpha,
                                         float** weights_samples, float** accumulated_color) {
    (void)bias_shapes;  // never read by nerf.py
    return guard_float([&]() -> float {
        const CallShape c = make_shape(true, layer_input_h, layer_input_w, target_image_h, target_image_w,
                                       num_weights, weight_shapes, intermediate_output_shapes, num_samples);
        const LomaTables in{layer_input, ws, bs, target_image, intermediate_outputs, img_sample_rgba_arr,
                            dists, alpha, cumprod_alpha, weights_samples, accumulated_color};
        return stage_call("nerf_evaluate_and_march", true, c, in, nullptr, 0.0f);
    });
}

extern "C" void grad_nerf_evaluate_and_march(
    float** layer_input, float** d_layer_input, int layer_input_h, int* d_layer_input_h,
    int layer_input_w, int* d_layer_input_w, float*** ws, float*** d_ws, float** bs, float** d_bs,
    float** target_image, float** d_target_image, int target_image_h, int* d_target_image_h,
    int target_image_w, int* d_target_image_w, int num_weights, int* d_num_weights,
    int** weight_shapes, int** d_weight_shapes, int** bias_shapes, int** d_bias_shapes,
    int** intermediate_output_shapes, int** d_intermediate_output_shapes,
    float*** intermediate_outputs, float*** d_intermediate_outputs, float*** img_sample_rgba_arr,
    float*** d_img_sample_rgba_arr, int num_samples, int* d_num_samples, float** dists,
    float** d_dists, float** alpha, float** d_alpha, float** cumprod_alpha,
    float** d_cumprod_alpha, float** weights_samples, float** d_weights_samples,
    float** accumulated_color, float** d_accumulated_color, float _dreturn) {
    // int adjoints are never written by loma (reverse_diff.py:146-147)
    (void)d_layer_input_h; (void)d_layer_input_w; (void)d_target_image_h; (void)d_target_image_w;
    (void)d_num_weights; (void)d_weight_shapes; (void)d_bias_shapes;
    (void)d_intermediate_output_shapes; (void)d_num_samples; (void)bias_shapes;
    guard_int([&]() {
        const CallShape c = make_shape(true, layer_input_h, layer_input_w, target_image_h, target_image_w,
                                       num_weights, weight_shapes, intermediate_output_shapes, num_samples);
        // (of the primal tables the re-executed forward reads the inputs alone)
        const LomaTables in{layer_input, ws, bs, target_image, intermediate_outputs, img_sample_rgba_arr,
                            dists, alpha, cumprod_alpha, weights_samples, accumulated_color};
        const LomaTables adj{d_layer_input, d_ws, d_bs, d_target_image, d_intermediate_outputs, d_img_sample_rgba_arr,
                             d_dists, d_alpha, d_cumprod_alpha, d_weights_samples, d_accumulated_color};
        stage_call("grad_nerf_evaluate_and_march", true, c, in, &adj, _dreturn);
    });
}

extern "C" float mlp_fit(float** layer_input, int layer_input_h, int layer_input_w,
                         float** layer_output, float*** ws, float** bs, float** target_image,
                         int target_image_h, int target_image_w, int num_weights,
                         int** weight_shapes, int** bias_shapes, int** intermediate_output_shapes,
                         float*** intermediate_outputs) {
    (void)layer_output;  // unused by mlp_fit.py
    (void)bias_shapes;
    return guard_float([&]() -> float {
        const CallShape c = make_shape(false, layer_input_h, layer_input_w, target_image_h, target_image_w,
                                       num_weights, weight_shapes, intermediate_output_shapes, 0);
        const LomaTables in{layer_input, ws, bs, target_image, intermediate_outputs};
        return stage_call("mlp_fit", false, c, in, nullptr, 0.0f);
    });
}

extern "C" void grad_mlp_fit(float** layer_input, float** d_layer_input, int layer_input_h,
                             int* d_layer_input_h, int layer_input_w, int* d_layer_input_w,
                             float** layer_output, float** d_layer_output, float*** ws,
                             float*** d_ws, float** bs, float** d_bs, float** target_image,
                             float** d_target_image, int target_image_h, int* d_target_image_h,
                             int target_image_w, int* d_target_image_w, int num_weights,
                             int* d_num_weights, int** weight_shapes, int** d_weight_shapes,
                             int** bias_shapes, int** d_bias_shapes,
                             int** intermediate_output_shapes,
                             int** d_intermediate_output_shapes, float*** intermediate_outputs,
                             float*** d_intermediate_outputs, float _dreturn) {
    (void)d_layer_input_h; (void)d_layer_input_w; (void)layer_output; (void)d_layer_output;
    (void)d_target_image_h; (void)d_target_image_w; (void)d_num_weights; (void)d_weight_shapes;
    (void)bias_shapes; (void)d_bias_shapes; (void)d_intermediate_output_shapes;
    guard_int([&]() {
        const CallShape c = make_shape(false, layer_input_h, layer_input_w, target_image_h, target_image_w,
                                       num_weights, weight_shapes, intermediate_output_shapes, 0);
        const LomaTables in{layer_input, ws, bs, target_image, intermediate_outputs};
        const LomaTables adj{d_layer_input, d_ws, d_bs, d_target_image, d_intermediate_outputs};
        stage_call("grad_mlp_fit", false, c, in, &adj, _dreturn);
    });
}

extern "C" void mult_a_b(float** a, int a_h, int a_w, float** b, int b_h, int b_w, float** c) {
    (void)b_h;
    guard_int([&]() {
        if (a_h < 0 || a_w < 0 || b_w < 0) fail("negative dimension");
        CompatCtx& cx = compat();
        Carve k;
        const size_t oa = k.take((size_t)a_h * a_w), ob = k.take((size_t)a_w * b_w),
                     oc = k.take((size_t)a_h * b_w);
        float* h = (float*)cx.host.get(k.off * sizeof(float));
        float* g = (float*)cx.dev.get(k.off * sizeof(float));
        gather2(h + oa, a, a_h, a_w, a_w);
        gather2(h + ob, b, a_w, b_w, b_w);  // mult_a_b reads b[k][j] for k < a_w
        gather2(h + oc, c, a_h, b_w, b_w);
        HIP_OK(hipMemcpyAsync(g, h, k.off * sizeof(float), hipMemcpyHostToDevice, cx.stream));
        lg_mult_a_b(g + oa, a_h, a_w, g + ob, b_w, g + oc, cx.stream);
        check_launch("mult_a_b");
        HIP_OK(hipMemcpyAsync(h + oc, g + oc, (size_t)a_h * b_w * sizeof(float),
                              hipMemcpyDeviceToHost, cx.stream));
        HIP_OK(hipStreamSynchronize(cx.stream));
        scatter2(c, h + oc, a_h, b_w, b_w);
    });
}

// =============================================================================================
// native batched API
// =============================================================================================
struct lnerf_ctx {
    int device = 0;
    DevBuf fused_ws;
    DevBuf generic_ws;
    DevBuf dinput_ws;    // LNERF_WANT_DINPUT: the encoded gradient (R, k[0]) the input-gradient kernel reads
    std::mutex mu;
    hipEvent_t ev[7] = {};
    bool timed = false;
    int last_path = 0;   // lnerf_ctx_last_path
    int dw_grid = 0;     // LNERF_OPT_DW_GRID (0: default_dw_grid)
    FusedPlan last_plan{};   // the last fused training step's plan (lnerf_ctx_relu_masks)
    bool last_k16_train = false;
    size_t ws_used = 0;  // lnerf_ctx_workspace_used
};

// The plan's carve against the bytes allocated for it: one carve (lnerf_plan.h) but two calls of it, the
// plan's at its own tile and slab format, the allocation's at the larger of each.
static size_t check_workspace(const FusedPlan& p, size_t bytes) {
    const size_t used = p.ws_floats * sizeof(float);
    if (used > bytes) fail("internal: the fused plan needs %zu workspace bytes, %zu were allocated", used, bytes);
    return used;
}

static int path_bits(const FusedPlan& p, bool train, bool kr = false) {
    return LNERF_PATH_FUSED | LNERF_PATH_K16 | (p.tile == 64 ? LNERF_PATH_K16_W4 : 0) | (kr ? LNERF_PATH_KR : 0) |
           (train ? LNERF_PATH_DW16 : 0) | (train && a24_slabs(p.x6) ? LNERF_PATH_A24 : 0) | (p.x6 << 8);
}

// Flags that ask for a fused-path kernel or precision: an explicit request that cannot be served
// is an error, never a silent substitute.
constexpr int kFusedRequests = LNERF_MFMA_BF16 | LNERF_MFMA_F16X3 | LNERF_MFMA_BF16X6 | LNERF_K16_W4 |
                               LNERF_RENDER_K16;

// At most one MFMA precision flag; the round-1..3 kernel selectors are gone (lnerf.h).
static void check_precision_flags(int flags) {
    if (flags & (LNERF_MFMA_F32 | LNERF_ONE_WAVE | LNERF_K32))
        fail("flags 0x%x select a removed kernel (LNERF_MFMA_F32 / LNERF_ONE_WAVE / LNERF_K32): the fused "
             "path is k16 + dw16; exact fp32 arithmetic is LNERF_GENERIC",
             flags & (LNERF_MFMA_F32 | LNERF_ONE_WAVE | LNERF_K32));
    const int prec = flags & (LNERF_MFMA_BF16 | LNERF_MFMA_F16X3 | LNERF_MFMA_BF16X6);
    if (prec & (prec - 1)) fail("conflicting MFMA precision flags 0x%x (set at most one)", prec);
    if ((flags & LNERF_GENERIC) && (flags & kFusedRequests))
        fail("LNERF_GENERIC conflicts with the fused-path flags 0x%x", flags & kFusedRequests);
}

extern "C" const char* lnerf_last_error(void) { return g_last_error.c_str(); }
extern "C" const char* lnerf_version(void) { return "loma-nerf-amd 0.5 (gfx950)"; }

extern "C" unsigned lnerf_build_knobs(void) {
    return lnerf::k16_build_knobs() | lnerf::dw16_build_knobs() | lnerf::kr_build_knobs();
}

extern "C" int lnerf_ctx_create(lnerf_ctx** out, int device) {
    return guard_int([&]() {
        if (!out) fail("null out");
        int n = 0;
        HIP_OK(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) fail("device %d not visible (%d devices)", device, n);
        HIP_OK(hipSetDevice(device));
        lnerf_ctx* c = new lnerf_ctx();
        c->device = device;
        for (auto& e : c->ev) HIP_OK(hipEventCreate(&e));
        *out = c;
    });
}

extern "C" void lnerf_ctx_destroy(lnerf_ctx* ctx) {
    if (!ctx) return;
    for (auto& e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    delete ctx;
}

static void validate(const lnerf_mlp* m, const lnerf_batch* b, bool need_target = true) {
    if (!m || !b) fail("null mlp/batch");
    if (m->num_layers < 1 || m->num_layers > kMaxLayers) fail("num_layers out of range");
    for (int l = 0; l < m->num_layers; ++l) {
        if (m->k[l] < 1 || m->n[l] < 1) fail("layer %d has an empty shape", l);
        if (m->k[l] > m->w_k || m->n[l] > m->w_n) fail("layer %d exceeds padded layout", l);
        if (l > 0 && m->k[l] != m->n[l - 1]) fail("k[%d] != n[%d]", l, l - 1);
    }
    if (b->rays < 1 || b->samples < 1) fail("empty batch");
    if (!b->x) fail("null batch pointer: batch->x is required");
    if (need_target && !b->target)
        fail("null batch pointer: batch->target is required (lnerf_render computes the loss too)");
    if (b->input_mode == LNERF_INPUT_POINTS || b->input_mode == LNERF_INPUT_RAYS) {
        if (b->num_freqs < 0 || m->k[0] != 3 + 6 * b->num_freqs)
            fail("POINTS/RAYS mode needs k[0] == 3 + 6F");
    } else if (b->input_mode != LNERF_INPUT_ENCODED) {
        fail("unknown input_mode");
    }
}

// NeRF head (rgb + sigma) needs dists (unless RAYS) and >= 4 outputs; the mlp_fit head
// (LNERF_HEAD_FIT) runs only on the fused k16 path, one row per "ray", without dists.
static void validate_head(const lnerf_mlp* m, const lnerf_batch* b, int flags) {
    if (!(flags & LNERF_HEAD_FIT)) {
        if (m->n[m->num_layers - 1] < 4) fail("head needs >= 4 outputs");
        if (b->input_mode != LNERF_INPUT_RAYS && !b->dists) fail("null dists");
        return;
    }
    if (flags & (LNERF_GENERIC | LNERF_MFMA_BF16X6))
        fail("LNERF_HEAD_FIT runs on the k16 kernel in fp16x3 or bf16 only");
    if (b->samples != 1 || b->input_mode != LNERF_INPUT_ENCODED || m->n[m->num_layers - 1] > 4)
        fail("LNERF_HEAD_FIT needs samples == 1, ENCODED input and 1..4 outputs");
}

extern "C" size_t lnerf_workspace_bytes(const lnerf_mlp* mlp, int rays, int samples) {
    if (!mlp) return 0;
    return fused_workspace_bytes(*mlp, rays, samples);
}

// Standard-semantics generic call: io rows = R, zero-initialised buffers (train_nerf.py builds
// fresh zero arrays for every call, :313-317, :370-392).
static void generic_step(lnerf_ctx* ctx, const lnerf_mlp& m, const float* ws, const float* bs,
                         const lnerf_batch& bt, float seed, int flags, const lnerf_outputs& out,
                         bool want_grad, hipStream_t s, const comp::MapsArgs* maps = nullptr,
                         const comp::VjpArgs* vjp = nullptr) {
    const int L = m.num_layers, R = bt.rays * bt.samples, S = bt.samples, th = bt.rays;
    if (want_grad && (flags & LNERF_ACCUMULATE))
        fail("LNERF_ACCUMULATE is only supported on the fused path");
    LgDims d{};
    d.L = L;
    d.in_h = R;
    d.in_w = m.k[0];
    d.th = th;
    d.tw = 3;
    d.S = S;
    d.nerf_head = 1;
    int maxn = 4;
    for (int l = 0; l < L; ++l) {
        d.wsh1[l] = m.n[l];
        d.ios0[l] = R;
        d.ios1[l] = m.n[l];
        maxn = std::max(maxn, m.n[l]);
    }
    d.x_cols = m.k[0];
    d.w_k = m.w_k;
    d.w_n = m.w_n;
    d.b_n = m.w_n;
    d.io_rows = R;
    d.io_cols = maxn;
    d.t_cols = 3;
    d.acc_cols = 3;
    Carve k;
    const size_t nio = (size_t)L * R * maxn, nS = (size_t)R;
    const size_t oX = k.take((size_t)R * m.k[0]), oIO = k.take(nio), oZ = k.take(nio),
                 odIO = k.take(nio), org = k.take(nS * 4), oal = k.take(nS), ocp = k.take(nS),
                 ows = k.take(nS), ocC = k.take(nS), ocP = k.take(nS), oacc = k.take((size_t)th * 3),
                 odrg = k.take(nS * 4), odal = k.take(nS), odcp = k.take(nS), odws = k.take(nS),
                 odd = k.take(nS), odacc = k.take((size_t)th * 3), odT = k.take((size_t)th * 3),
                 odW = k.take((size_t)L * m.w_k * m.w_n), odB = k.take((size_t)L * m.w_n),
                 oloss = k.take(1), oseed = k.take(1), odX = k.take((size_t)R * m.k[0]),
                 odist = k.take(nS);
    float* g = (float*)ctx->generic_ws.get(k.off * sizeof(float));
    const float* X = bt.x;
    const float* dists = bt.dists;
    if (bt.input_mode == LNERF_INPUT_POINTS) {
        k_positional_encoding(bt.x, R, bt.num_freqs, g + oX, m.k[0], s);
        X = g + oX;
    } else if (bt.input_mode == LNERF_INPUT_RAYS) {
        k_positional_encoding_rays(bt.x, bt.rays, S, bt.near_t, bt.far_t, bt.num_freqs, g + oX,
                                   m.k[0], s);
        k_ray_dists(bt.rays, S, bt.near_t, bt.far_t, g + odist, s);
        X = g + oX;
        dists = g + odist;
    }
    // forward call (nerf_evaluate_and_march)
    HIP_OK(hipMemsetAsync(g + oIO, 0, nio * sizeof(float), s));
    HIP_OK(hipMemsetAsync(g + oacc, 0, (size_t)th * 3 * sizeof(float), s));
    LgBuffers b{};
    b.X = X;
    b.W = ws;
    b.B = bs;
    b.T = vjp ? nullptr : bt.target;   // lnerf_render_maps_vjp ignores the target: no loss stage
    b.IO = g + oIO;
    b.rgba = g + org;
    b.dists = dists;
    b.alpha = g + oal;
    b.cp = g + ocp;
    b.wsamp = g + ows;
    b.acc = g + oacc;
    lg_nerf_forward(d, b, g + oloss, s);
    if (out.loss) HIP_OK(hipMemcpyAsync(out.loss, g + oloss, 4, hipMemcpyDeviceToDevice, s));
    if (out.acc_color)
        HIP_OK(hipMemcpyAsync(out.acc_color, g + oacc, (size_t)th * 3 * 4, hipMemcpyDeviceToDevice, s));
    if (maps) {
        // lnerf_render_maps: the forward's own img_sample_rgba_arr and weights_samples, and the per-ray
        // sums of the latter
        if (maps->rgba) HIP_OK(hipMemcpyAsync(maps->rgba, g + org, nS * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (maps->weights) HIP_OK(hipMemcpyAsync(maps->weights, g + ows, nS * sizeof(float), hipMemcpyDeviceToDevice, s));
        k_ray_maps(g + ows, maps->sample_t, th, S, bt.near_t, bt.far_t, maps->depth, maps->opacity, s);
    }
    if (!want_grad) return;
    // grad call on fresh zero buffers, seeded with the loss or the constant
    HIP_OK(hipMemsetAsync(g + oIO, 0, (oloss - oIO) * sizeof(float), s));  // primal + adjoints
    HIP_OK(hipMemsetAsync(g + odX, 0, (size_t)R * m.k[0] * sizeof(float), s));
    const float* seed_dev = g + oloss;
    if (!(flags & LNERF_SEED_LOSS)) {
        k_fill(g + oseed, seed, 1, s);
        seed_dev = g + oseed;
    }
    b.zpre = g + oZ;
    b.cpC = g + ocC;
    b.cpP = g + ocP;
    LgAdjoints a{};
    a.dX = out.d_x ? g + odX : nullptr;
    a.dW = g + odW;
    a.dB = g + odB;
    a.dT = g + odT;
    a.dIO = g + odIO;
    a.drgba = g + odrg;
    a.ddists = g + odd;
    a.dalpha = g + odal;
    a.dcp = g + odcp;
    a.dwsamp = g + odws;
    a.dacc = g + odacc;
    // lnerf_render_maps_vjp: the compositing reverse seeded from the caller's adjoints
    const LgVjp lv{vjp ? *vjp : comp::VjpArgs{}, bt.input_mode == LNERF_INPUT_RAYS, bt.near_t, bt.far_t};
    lg_nerf_grad(d, b, a, seed_dev, s, vjp ? &lv : nullptr);
    const size_t nW = (size_t)L * m.w_k * m.w_n, nB = (size_t)L * m.w_n;
    auto emit = [&](float* dst, const float* src, size_t n) {
        if (dst) HIP_OK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    };
    emit(out.d_ws, g + odW, nW);
    emit(out.d_bs, g + odB, nB);
    emit(out.d_dists, g + odd, nS);
    emit(out.d_target, g + odT, (size_t)th * 3);
    emit(out.d_x, g + odX, (size_t)R * m.k[0]);
}

static bool use_fused(const lnerf_mlp& m, const lnerf_batch& b, int flags) {
    if (flags & LNERF_GENERIC) return false;
    const char* why = nullptr;
    const bool fit = (flags & LNERF_HEAD_FIT) != 0;
    const bool ok = fused_supported(m, b.rays, b.samples, b.input_mode, &why, fit);
    if (fit && !ok) fail("mlp_fit head: %s", why);
    if (!ok && (flags & LNERF_FAST)) fail("fused path unavailable: %s", why);
    if (!ok && (flags & kFusedRequests))
        fail("flags 0x%x ask for the fused path, which is unavailable: %s", flags & kFusedRequests, why);
    if (ok && (flags & LNERF_WANT_DX) && b.input_mode != LNERF_INPUT_ENCODED)
        fail("LNERF_WANT_DX needs ENCODED input");
    return ok;
}

// ---- the context entry points' shared steps (train step, render, render maps, their VJP) ----------
static void validate_call(const lnerf_mlp* m, const lnerf_batch* b, int flags, const float* ws, const float* bs,
                          bool need_target = true) {
    validate(m, b, need_target);
    validate_head(m, b, flags);
    if (!ws || !bs) fail("null weights");
}

// LNERF_WANT_DINPUT: d_x in x's own layout. ENCODED input: that is LNERF_WANT_DX, on its code path.
// POINTS / RAYS: the step writes the encoded gradient to the context's scratch and the input-gradient
// kernel reverses it into the caller's d_x, which is returned (else NULL).
static float* resolve_dinput(int& flags, const lnerf_batch& b, lnerf_outputs& o) {
    if (flags & LNERF_WANT_DINPUT) {
        if (b.input_mode == LNERF_INPUT_ENCODED) flags |= LNERF_WANT_DX;
        else if (flags & LNERF_WANT_DX)
            fail("LNERF_WANT_DX | LNERF_WANT_DINPUT needs ENCODED input (d_x cannot hold both layouts)");
        else if (b.num_freqs > kMaxInputGradFreqs)
            fail("LNERF_WANT_DINPUT runs at most %d frequencies", kMaxInputGradFreqs);
    }
    if (!(flags & (LNERF_WANT_DX | LNERF_WANT_DINPUT))) o.d_x = nullptr;
    return (flags & LNERF_WANT_DX) ? nullptr : o.d_x;   // non-null: reverse the encoding
}

// A call's hold on its context, once its arguments have passed: the lock, the device, the stream. Any
// failure from here on leaves the masks unreadable: the workspace they live in may be reallocated
// before the call fails, and a render reuses it.
struct CtxCall {
    std::lock_guard<std::mutex> lock;
    hipStream_t s;   // NULL: the device's default (null) stream
    CtxCall(lnerf_ctx* ctx, void* stream) : lock(ctx->mu), s((hipStream_t)stream) {
        ctx->last_k16_train = false;
        ctx->ws_used = 0;
        HIP_OK(hipSetDevice(ctx->device));
    }
};

// What a call that ran leaves on the context. ev: the timing events it recorded, or NULL. train
// (nullable): the fused training plan the masks, the guard word and the exceptional rows are read through.
static hipEvent_t* timing_events(lnerf_ctx* ctx, int flags) { return (flags & LNERF_TIMING) ? ctx->ev : nullptr; }
static void finish_call(lnerf_ctx* ctx, const hipEvent_t* ev, int path, const FusedPlan* train = nullptr) {
    ctx->timed = ev != nullptr;
    ctx->last_path = path;
    if (train) {
        ctx->last_plan = *train;
        ctx->last_k16_train = true;
    }
}

// A training call once its arguments have passed: lnerf_train_step, or with vjp lnerf_render_maps_vjp
// (the same sequence seeded from the caller's adjoints; seed is 1 and the flags hold no LNERF_SEED_LOSS,
// LNERF_K16_W4 or LNERF_HEAD_FIT then). d_input: resolve_dinput's.
static void training_call(lnerf_ctx* ctx, const char* what, const lnerf_mlp& m, const float* ws, const float* bs,
                          const lnerf_batch& b, float seed, int flags, lnerf_outputs o, float* d_input,
                          const comp::VjpArgs* vjp, void* stream) {
    const CtxCall call(ctx, stream);
    const int vjp_bit = vjp ? LNERF_PATH_VJP : 0;
    const bool fused = use_fused(m, b, flags);
    if (d_input) o.d_x = (float*)ctx->dinput_ws.get((size_t)b.rays * b.samples * m.k[0] * sizeof(float));
    if (!fused) {
        generic_step(ctx, m, ws, bs, b, seed, flags, o, true, call.s, nullptr, vjp);
        // (the generic reverse pass has seeded the encoded gradient already)
        if (d_input) k_input_grad(b, o.d_x, nullptr, d_input, call.s);
        finish_call(ctx, nullptr, LNERF_PATH_GENERIC | vjp_bit);
        check_launch(what);
        return;
    }
    const size_t bytes = fused_workspace_bytes(m, b.rays, b.samples, true, ctx->dw_grid);
    void* wsb = ctx->fused_ws.get(bytes);
    FusedPlan p{}, px{};
    fused_plan(p, m, b, wsb, flags, true, ctx->dw_grid);
    // the fp16x3 floor guard (lnerf_internal.h kGuardExp) under the default precision: the bf16x6 plan
    // of the same step, run on the device only if k1 finds a hidden G element below fp16x3's floor (an
    // explicit LNERF_MFMA_F16X3 asks for fp16x3 exactly; the mlp_fit head and the 64-sample workgroups
    // have no bf16x6 k1)
    const bool guarded = LNERF_GUARD && p.x6 == 2 && !(flags & (LNERF_MFMA_F16X3 | LNERF_K16_W4 | LNERF_HEAD_FIT));
    if (guarded) {
        fused_plan(px, m, b, wsb, flags | LNERF_MFMA_BF16X6, true, ctx->dw_grid);
        px.guard = nullptr;
        px.gate = p.guard;
        px.w16 = p.w16x;   // packed by p's own pack launch, beside its fp16x3 planes
        px.w16x = nullptr;
        // (its fp32 activation slabs end the carve later than p's int24 ones)
        ctx->ws_used = check_workspace(px, bytes);
    } else {
        ctx->ws_used = check_workspace(p, bytes);
        p.guard = nullptr;
        p.w16x = nullptr;
    }
    hipEvent_t* ev = timing_events(ctx, flags);
    if (vjp) fused_render_vjp(p, ws, bs, b, flags, o, *vjp, call.s, ev, guarded ? &px : nullptr, d_input);
    else fused_train_step(p, ws, bs, b, seed, flags, o, call.s, ev, guarded ? &px : nullptr, d_input);
    check_launch(what);
    finish_call(ctx, ev, path_bits(p, true) | vjp_bit, &p);
}

// A render once its arguments have passed: lnerf_render, or with maps lnerf_render_maps.
static void render_call(lnerf_ctx* ctx, const char* what, const lnerf_mlp& m, const float* ws, const float* bs,
                        const lnerf_batch& b, int flags, const lnerf_outputs& o, const comp::MapsArgs* maps,
                        void* stream) {
    const CtxCall call(ctx, stream);
    const int maps_bit = maps ? LNERF_PATH_MAPS : 0;
    flags &= ~(LNERF_WANT_DX | LNERF_WANT_DINPUT | LNERF_ACCUMULATE | LNERF_SEED_LOSS);   // a training call's
    if (use_fused(m, b, flags)) {
        const size_t bytes = fused_workspace_bytes(m, b.rays, b.samples, false, ctx->dw_grid);
        FusedPlan p{};
        fused_plan(p, m, b, ctx->fused_ws.get(bytes), flags, false, ctx->dw_grid);
        ctx->ws_used = check_workspace(p, bytes);
        p.guard = nullptr;   // (the floor guard is a training-step feature)
        p.w16x = nullptr;
        hipEvent_t* ev = timing_events(ctx, flags);
        if (maps) fused_render_maps(p, ws, bs, b, o, *maps, call.s, flags, ev);
        else fused_render(p, ws, bs, b, o, call.s, flags, ev);
        finish_call(ctx, ev, path_bits(p, false, fused_render_uses_kr(p, flags)) | maps_bit);
    } else {
        generic_step(ctx, m, ws, bs, b, 1.0f, 0, o, false, call.s, maps);
        finish_call(ctx, nullptr, LNERF_PATH_GENERIC | maps_bit);
    }
    check_launch(what);
}

extern "C" int lnerf_train_step(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws,
                                const float* bs, const lnerf_batch* batch, float seed, int flags,
                                const lnerf_outputs* out, void* stream) {
    return guard_int([&]() {
        if (!ctx) fail("null ctx");
        validate_call(mlp, batch, flags, ws, bs);
        lnerf_outputs o = out ? *out : lnerf_outputs{};
        float* d_input = resolve_dinput(flags, *batch, o);
        if (flags & LNERF_HEAD_FIT) o.d_dists = nullptr;
        check_precision_flags(flags);
        training_call(ctx, "lnerf_train_step", *mlp, ws, bs, *batch, seed, flags, o, d_input, nullptr, stream);
    });
}

extern "C" int lnerf_get_rays(int width, const double* K, const double* c2w, float* rays,
                              void* stream) {
    return guard_int([&]() {
        if (width < 1 || !K || !c2w || !rays) fail("lnerf_get_rays: bad arguments");
        k_get_rays(width, K, c2w, rays, (hipStream_t)stream);
        check_launch("lnerf_get_rays");
    });
}

// The entry points below take no context: they need a device all the same (no CPU path).
static void need_device() {
    int n = 0;
    HIP_OK(hipGetDeviceCount(&n));
    if (n < 1) fail("no HIP device visible");
}

extern "C" int lnerf_input_grad(const lnerf_batch* batch, const float* d_encoded, const float* scale,
                                float* d_input, void* stream) {
    return guard_int([&]() {
        // (validate() serves the steps and insists on a target; this call has none)
        if (!batch || !batch->x || !d_encoded || !d_input) fail("lnerf_input_grad: null argument");
        if (batch->input_mode != LNERF_INPUT_POINTS && batch->input_mode != LNERF_INPUT_RAYS)
            fail("lnerf_input_grad: input_mode must be LNERF_INPUT_POINTS or LNERF_INPUT_RAYS");
        if (batch->num_freqs < 0 || batch->num_freqs > kMaxInputGradFreqs)
            fail("lnerf_input_grad: num_freqs %d outside 0..%d", batch->num_freqs, kMaxInputGradFreqs);
        if (batch->rays < 1 || batch->samples < 1) fail("lnerf_input_grad: empty batch");
        if ((long long)batch->rays * batch->samples > (long long)std::numeric_limits<int>::max())
            fail("lnerf_input_grad: more than 2^31 - 1 sample rows");
        need_device();
        k_input_grad(*batch, d_encoded, scale, d_input, (hipStream_t)stream);
        check_launch("lnerf_input_grad");
    });
}

extern "C" int lnerf_pose_grad(int width, const double* K, const int* pixels, int n, const float* d_rays,
                               double* d_c2w, void* stream) {
    return guard_int([&]() {
        if (width < 1 || width > 46340 || !K || !d_rays || !d_c2w) fail("lnerf_pose_grad: bad arguments");
        if (n < 1) fail("lnerf_pose_grad: no rays");
        if (!pixels && n != width * width) fail("lnerf_pose_grad: n must be width * width without pixel indices");
        need_device();
        // the stage-1 partials: stream-ordered scratch, so calls on several streams never share it
        hipStream_t s = (hipStream_t)stream;
        double* part = nullptr;
        HIP_OK(hipMallocAsync((void**)&part, (size_t)pose_grad_parts(n) * 12 * sizeof(double), s));
        k_pose_grad(width, K, pixels, n, d_rays, part, d_c2w, s);
        const hipError_t launched = hipGetLastError();
        HIP_OK(hipFreeAsync(part, s));
        if (launched != hipSuccess) fail("lnerf_pose_grad: kernel launch failed: %s", hipGetErrorString(launched));
    });
}

// ---- per-ray sample depths (lnerf_sampling.hip): free functions on a stream, no context ----------
static void check_rows(const char* what, int rays, int per_ray) {
    if (rays < 0) fail("%s: negative ray count %d", what, rays);
    if ((long long)rays * per_ray > (long long)std::numeric_limits<int>::max())
        fail("%s: more than 2^31 - 1 values", what);
}

extern "C" int lnerf_sample_stratified(int rays, int S, float near_t, float far_t, const float* u,
                                       float* sample_t, void* stream) {
    return guard_int([&]() {
        if (!u) fail("lnerf_sample_stratified: u is NULL (the library owns no random numbers)");
        if (!sample_t) fail("lnerf_sample_stratified: sample_t is NULL");
        if (S < 1) fail("lnerf_sample_stratified: S = %d, need at least 1", S);
        check_rows("lnerf_sample_stratified", rays, S);
        if (rays == 0) return;
        need_device();
        k_sample_stratified(rays, S, near_t, far_t, u, sample_t, (hipStream_t)stream);
        check_launch("lnerf_sample_stratified");
    });
}

extern "C" int lnerf_sample_importance(int rays, int S, const float* t_coarse, float near_t, float far_t,
                                       const float* weights, int n_fine, const float* u, float* t_fine,
                                       float* t_all, void* stream) {
    return guard_int([&]() {
        if (S < 3 || S > 1024) fail("lnerf_sample_importance: S = %d outside 3..1024", S);
        if (n_fine < 1 || n_fine > 1024) fail("lnerf_sample_importance: n_fine = %d outside 1..1024", n_fine);
        if (!weights) fail("lnerf_sample_importance: weights is NULL");
        if (!t_fine && !t_all) fail("lnerf_sample_importance: t_fine and t_all are both NULL");
        check_rows("lnerf_sample_importance", rays, S + n_fine);
        if (rays == 0) return;
        need_device();
        k_sample_importance(rays, S, t_coarse, near_t, far_t, weights, n_fine, u, t_fine, t_all,
                            (hipStream_t)stream);
        check_launch("lnerf_sample_importance");
    });
}

extern "C" int lnerf_ray_points(const float* rays, int n, int S, const float* sample_t, float* points,
                                float* dists, void* stream) {
    return guard_int([&]() {
        if (!rays || !sample_t) fail("lnerf_ray_points: null argument");
        if (S < 1) fail("lnerf_ray_points: S = %d, need at least 1", S);
        check_rows("lnerf_ray_points", n, S);
        if (n == 0 || (!points && !dists)) return;
        need_device();
        k_ray_points(rays, n, S, sample_t, points, dists, (hipStream_t)stream);
        check_launch("lnerf_ray_points");
    });
}

extern "C" int lnerf_ray_points_grad(int n, int S, const float* sample_t, const float* d_points,
                                     const float* scale, float* d_rays, void* stream) {
    return guard_int([&]() {
        if (!sample_t || !d_points || !d_rays) fail("lnerf_ray_points_grad: null argument");
        if (S < 1) fail("lnerf_ray_points_grad: S = %d, need at least 1", S);
        check_rows("lnerf_ray_points_grad", n, S);
        if (n == 0) return;
        need_device();
        k_ray_points_grad(n, S, sample_t, d_points, scale, d_rays, (hipStream_t)stream);
        check_launch("lnerf_ray_points_grad");
    });
}

// ---- multiresolution hash grid (lnerf_hashgrid.hip): free functions on a stream, no context -------
// A level's entry count before the rounding lnerf_hashgrid_init applies: res^3 if that fits the
// table (dense), else T (hashed). T <= 2^24, so a dense level has res <= 256.
static long long hashgrid_level_entries(int res, int log2_table, bool* dense) {
    const long long T = 1ll << log2_table;
    const bool d = res <= 256 && (long long)res * res * res <= T;
    if (dense) *dense = d;
    return d ? (long long)res * res * res : T;
}

static void hashgrid_check_shape(const char* what, int levels, int features, int log2_table) {
    if (levels < 1 || levels > LNERF_HASHGRID_MAX_LEVELS)
        fail("%s: levels = %d outside 1..%d", what, levels, LNERF_HASHGRID_MAX_LEVELS);
    if (features != 1 && features != 2 && features != 4 && features != 8)
        fail("%s: features = %d, need 1, 2, 4 or 8", what, features);
    if (log2_table < 4 || log2_table > 24) fail("%s: log2_table = %d outside 4..24", what, log2_table);
}

// The validated, kernel-side form of `grid`; every index the kernels form is inside the level it
// belongs to once this has passed.
static HgParams hashgrid_params(const char* what, const lnerf_hashgrid* grid) {
    if (!grid) fail("%s: grid is NULL", what);
    hashgrid_check_shape(what, grid->levels, grid->features, grid->log2_table);
    HgParams g{};
    g.levels = grid->levels;
    g.features = grid->features;
    g.mask = (1u << grid->log2_table) - 1u;
    if (grid->offset[0] < 0) fail("%s: offset[0] = %lld is negative", what, grid->offset[0]);
    for (int l = 0; l < grid->levels; ++l) {
        if (grid->res[l] < 2) fail("%s: res[%d] = %d, need at least 2", what, l, grid->res[l]);
        bool dense = false;
        const long long entries = hashgrid_level_entries(grid->res[l], grid->log2_table, &dense);
        // (written as a comparison of offsets, so a huge offset cannot overflow the difference)
        if (grid->offset[l + 1] < grid->offset[l] || grid->offset[l + 1] - grid->offset[l] < entries)
            fail("%s: level %d (res %d) needs %lld entries, offset gives it %lld", what, l, grid->res[l], entries,
                 grid->offset[l + 1] - grid->offset[l]);
        g.lv[l].offset = grid->offset[l];
        g.lv[l].res = grid->res[l];
        g.lv[l].dense = dense ? 1 : 0;
    }
    if (grid->offset[grid->levels] > (1ll << 40)) fail("%s: more than 2^40 entries", what);
    for (int c = 0; c < 3; ++c) {
        if (!(grid->hi[c] > grid->lo[c]) || !std::isfinite(grid->hi[c]) || !std::isfinite(grid->lo[c]))
            fail("%s: the box needs finite hi > lo on axis %d", what, c);
        g.lo[c] = (double)grid->lo[c];
        g.ext[c] = (double)grid->hi[c] - (double)grid->lo[c];
    }
    return g;
}

static void hashgrid_check_rows(const char* what, long long R) {
    if (R < 0) fail("%s: negative row count %lld", what, R);
    if (R > (long long)std::numeric_limits<int>::max() * 256) fail("%s: more than 2^39 rows", what);
}

// table rows are read as one 4 F-byte access up to 16 bytes
static void hashgrid_check_aligned(const char* what, const char* name, const void* p, int features) {
    const size_t a = features >= 4 ? 16 : 4 * (size_t)features;
    if ((size_t)p % a) fail("%s: %s must be %zu-byte aligned at F = %d", what, name, a, features);
}

extern "C" long long lnerf_hashgrid_init(lnerf_hashgrid* grid, int levels, int features, int log2_table,
                                         int base_res, int max_res, const float* lo, const float* hi) {
    long long total = 0;
    const int rc = guard_int([&]() {
        const char* what = "lnerf_hashgrid_init";
        if (!grid || !lo || !hi) fail("%s: null argument", what);
        hashgrid_check_shape(what, levels, features, log2_table);
        if (base_res < 2 || max_res < base_res) fail("%s: need 2 <= base_res <= max_res", what);
        for (int c = 0; c < 3; ++c)
            if (!(hi[c] > lo[c]) || !std::isfinite(hi[c]) || !std::isfinite(lo[c]))
                fail("%s: the box needs finite hi > lo on axis %d", what, c);
        lnerf_hashgrid g{};
        g.levels = levels;
        g.features = features;
        g.log2_table = log2_table;
        const double b = levels > 1 ? std::exp(std::log((double)max_res / (double)base_res) / (double)(levels - 1)) : 1.0;
        for (int l = 0; l < levels; ++l) {
            g.res[l] = (int)std::floor((double)base_res * std::pow(b, (double)l) + 0.5);
            const long long entries = hashgrid_level_entries(g.res[l], log2_table, nullptr);
            g.offset[l + 1] = g.offset[l] + (entries + 3) / 4 * 4;
        }
        for (int c = 0; c < 3; ++c) {
            g.lo[c] = lo[c];
            g.hi[c] = hi[c];
        }
        *grid = g;
        total = g.offset[levels];
    });
    return rc ? rc : total;
}

extern "C" int lnerf_hashgrid_encode(const lnerf_hashgrid* grid, const float* table, const float* points,
                                     long long R, float* encoded, void* stream) {
    return guard_int([&]() {
        const char* what = "lnerf_hashgrid_encode";
        const HgParams g = hashgrid_params(what, grid);
        if (!table || !points || !encoded) fail("%s: null argument", what);
        hashgrid_check_aligned(what, "table", table, g.features);
        hashgrid_check_rows(what, R);
        if (R == 0) return;
        need_device();
        k_hashgrid_encode(g, table, points, R, encoded, (hipStream_t)stream);
        check_launch(what);
    });
}

extern "C" int lnerf_hashgrid_grad(const lnerf_hashgrid* grid, const float* table, const float* points,
                                   long long R, const float* d_encoded, const float* scale, int flags,
                                   float* d_table, float* d_points, void* stream) {
    return guard_int([&]() {
        const char* what = "lnerf_hashgrid_grad";
        const HgParams g = hashgrid_params(what, grid);
        if (flags & ~(LNERF_ACCUMULATE | LNERF_HASHGRID_REPRODUCIBLE))
            fail("%s: flags 0x%x: only LNERF_ACCUMULATE and LNERF_HASHGRID_REPRODUCIBLE apply", what, flags);
        const bool ordered = (flags & LNERF_HASHGRID_REPRODUCIBLE) != 0;
        if (!d_table && !d_points) fail("%s: d_table and d_points are both NULL", what);
        if (!points || !d_encoded) fail("%s: null argument", what);
        if (d_points && !table) fail("%s: d_points needs the table", what);
        if (d_points) hashgrid_check_aligned(what, "table", table, g.features);
        hashgrid_check_rows(what, R);
        // a contribution id 8 r + k must fit 32 bits
        if (ordered && R > (1ll << 28)) fail("%s: more than 2^28 rows under LNERF_HASHGRID_REPRODUCIBLE", what);
        if (ordered && d_table) hashgrid_check_aligned(what, "d_table", d_table, g.features);   // rows are stored whole
        if (R == 0) return;
        need_device();
        hipStream_t s = (hipStream_t)stream;
        if (d_table && ordered) {
            // stream-ordered scratch, as lnerf_pose_grad: calls on several streams never share it
            size_t bytes = 0;
            HIP_OK(k_hashgrid_sorted_scratch_bytes(g, R, s, &bytes));
            void* scratch = nullptr;
            HIP_OK(hipMallocAsync(&scratch, bytes, s));
            hipError_t done = hipSuccess;
            if (!(flags & LNERF_ACCUMULATE))
                done = hipMemsetAsync(d_table, 0, (size_t)grid->offset[g.levels] * g.features * sizeof(float), s);
            if (done == hipSuccess)
                done = k_hashgrid_grad_table_sorted(g, points, R, d_encoded, scale, (flags & LNERF_ACCUMULATE) != 0,
                                                    d_table, scratch, s);
            HIP_OK(hipFreeAsync(scratch, s));
            if (done != hipSuccess) fail("%s: the sorted d_table failed: %s", what, hipGetErrorString(done));
        } else if (d_table) {
            if (!(flags & LNERF_ACCUMULATE))
                HIP_OK(hipMemsetAsync(d_table, 0, (size_t)grid->offset[g.levels] * g.features * sizeof(float), s));
            k_hashgrid_grad_table(g, points, R, d_encoded, scale, d_table, s);
            check_launch(what);
        }
        if (d_points) {
            k_hashgrid_grad_points(g, table, points, R, d_encoded, scale, d_points, s);
            check_launch(what);
        }
    });
}

extern "C" long long lnerf_hashgrid_grad_scratch(const lnerf_hashgrid* grid, long long R, void* stream) {
    long long total = 0;
    const int rc = guard_int([&]() {
        const char* what = "lnerf_hashgrid_grad_scratch";
        const HgParams g = hashgrid_params(what, grid);
        hashgrid_check_rows(what, R);
        if (R > (1ll << 28)) fail("%s: more than 2^28 rows under LNERF_HASHGRID_REPRODUCIBLE", what);
        if (R == 0) return;
        need_device();
        size_t bytes = 0;
        HIP_OK(k_hashgrid_sorted_scratch_bytes(g, R, (hipStream_t)stream, &bytes));
        total = (long long)bytes;
    });
    return rc ? rc : total;
}

// ---- occupancy grid (lnerf_occgrid.hip): free functions on a stream, no context -------------------
// The validated, kernel-side form of `grid`; every cell index the kernels form from a point or
// accept from a list is inside 0..res^3-1 once this has passed.
static OccParams occgrid_params(const char* what, const lnerf_occgrid* grid) {
    if (!grid) fail("%s: grid is NULL", what);
    const int res = grid->res;
    if (res < 4 || res > 256 || (res & (res - 1))) fail("%s: res = %d, need a power of two in 4..256", what, res);
    OccParams g{};
    g.res = res;
    while ((1 << g.shift) < res) ++g.shift;
    g.cells = (long long)res * res * res;
    for (int c = 0; c < 3; ++c) {
        if (!(grid->hi[c] > grid->lo[c]) || !std::isfinite(grid->hi[c]) || !std::isfinite(grid->lo[c]))
            fail("%s: the box needs finite hi > lo on axis %d", what, c);
        g.lo[c] = (double)grid->lo[c];
        g.ext[c] = (double)grid->hi[c] - (double)grid->lo[c];
    }
    return g;
}

// n cells of a list, or all res^3 of them in order when there is no list
static void occgrid_check_cells(const char* what, const OccParams& g, const int* cells, long long n) {
    if (n < 0) fail("%s: negative count %lld", what, n);
    if (n > (long long)std::numeric_limits<int>::max() * 256) fail("%s: more than 2^39 cells", what);
    if (!cells && n != 0 && n != g.cells)
        fail("%s: n = %lld without a cell list, need res^3 = %lld", what, n, g.cells);
}

extern "C" int lnerf_occgrid_cell_points(const lnerf_occgrid* grid, const int* cells, long long n, const float* u,
                                         float* points, void* stream) {
    return guard_int([&]() {
        const char* what = "lnerf_occgrid_cell_points";
        const OccParams g = occgrid_params(what, grid);
        if (!points) fail("%s: points is NULL", what);
        occgrid_check_cells(what, g, cells, n);
        if (n == 0) return;
        need_device();
        k_occgrid_cell_points(g, cells, n, u, points, (hipStream_t)stream);
        check_launch(what);
    });
}

extern "C" int lnerf_occgrid_update(const lnerf_occgrid* grid, float* density, const int* cells, long long n,
                                    const float* sigma, int sigma_stride, float decay, void* stream) {
    return guard_int([&]() {
        const char* what = "lnerf_occgrid_update";
        const OccParams g = occgrid_params(what, grid);
        if (!density || !sigma) fail("%s: null argument", what);
        if (sigma_stride < 1) fail("%s: sigma_stride = %d, need at least 1", what, sigma_stride);
        if (!(decay >= 0.0f && decay <= 1.0f)) fail("%s: decay = %g outside 0..1", what, (double)decay);
        occgrid_check_cells(what, g, cells, n);
        if (n == 0) return;
        need_device();
        k_occgrid_update(g, density, cells, n, sigma, sigma_stride, decay, (hipStream_t)stream);
        check_launch(what);
    });
}

extern "C" int lnerf_occgrid_threshold(const lnerf_occgrid* grid, const float* density, float threshold, int flags,
                                       unsigned* bits, double* mean, long long* occupied, void* stream) {
    return guard_int([&]() {
        const char* what = "lnerf_occgrid_threshold";
        const OccParams g = occgrid_params(what, grid);
        if (!density) fail("%s: density is NULL", what);
        if (flags & ~LNERF_OCC_MEAN) fail("%s: flags 0x%x: only LNERF_OCC_MEAN applies", what, flags);
        if (std::isnan(threshold)) fail("%s: threshold is NaN", what);
        if (!bits && !mean && !occupied) fail("%s: bits, mean and occupied are all NULL", what);
        need_device();
        // the stage-1 partial sums and thr: stream-ordered scratch, so calls on several streams never share it
        hipStream_t s = (hipStream_t)stream;
        double* scratch = nullptr;
        HIP_OK(hipMallocAsync((void**)&scratch, (size_t)occgrid_threshold_scratch(g) * sizeof(double), s));
        k_occgrid_threshold(g, density, threshold, flags, bits, mean, occupied, scratch, s);
        const hipError_t launched = hipGetLastError();
        HIP_OK(hipFreeAsync(scratch, s));
        if (launched != hipSuccess) fail("%s: kernel launch failed: %s", what, hipGetErrorString(launched));
    });
}

extern "C" int lnerf_sample_occupancy(const lnerf_occgrid* grid, const unsigned* bits, const float* rays, int n,
                                      int S, int steps, float near_t, float far_t, const float* u, int flags,
                                      float* sample_t, float* dists, int* n_occ, void* stream) {
    return guard_int([&]() {
        const char* what = "lnerf_sample_occupancy";
        const OccParams g = occgrid_params(what, grid);
        if (!bits || !rays) fail("%s: null argument", what);
        if (steps < 64 || steps > 1024 || steps % 64)
            fail("%s: steps = %d, need a multiple of 64 in 64..1024", what, steps);
        if (S < 1 || S > 1024) fail("%s: S = %d outside 1..1024", what, S);
        if (!(far_t > near_t) || !std::isfinite(far_t) || !std::isfinite(near_t))
            fail("%s: need finite far_t > near_t", what);
        if (flags & ~LNERF_OCC_LAST_OPAQUE) fail("%s: flags 0x%x: only LNERF_OCC_LAST_OPAQUE applies", what, flags);
        if (!sample_t && !dists && !n_occ) fail("%s: sample_t, dists and n_occ are all NULL", what);
        check_rows(what, n, S);
        if (n == 0) return;
        need_device();
        k_sample_occupancy(g, bits, rays, n, S, steps, near_t, far_t, u, flags, sample_t, dists, n_occ,
                           (hipStream_t)stream);
        check_launch(what);
    });
}

extern "C" int lnerf_render(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                            const lnerf_batch* batch, int flags, const lnerf_outputs* out,
                            void* stream) {
    return guard_int([&]() {
        if (!ctx) fail("null ctx");
        validate_call(mlp, batch, flags, ws, bs);
        const lnerf_outputs o = out ? *out : lnerf_outputs{};
        check_precision_flags(flags);
        render_call(ctx, "lnerf_render", *mlp, ws, bs, *batch, flags, o, nullptr, stream);
    });
}

extern "C" int lnerf_render_maps(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                                 const lnerf_batch* batch, const float* sample_t, int flags,
                                 const lnerf_render_outputs* out, void* stream) {
    return guard_int([&]() {
        if (!ctx) fail("null ctx");
        if (flags & LNERF_HEAD_FIT) fail("lnerf_render_maps: LNERF_HEAD_FIT has no compositing to map");
        validate_call(mlp, batch, flags, ws, bs, false);
        const lnerf_render_outputs ro = out ? *out : lnerf_render_outputs{};
        if (!batch->target && ro.loss) fail("lnerf_render_maps: out->loss needs batch->target");
        if ((uintptr_t)ro.rgba % 16) fail("lnerf_render_maps: out->rgba must be 16-byte aligned (one store per sample)");
        if (batch->input_mode == LNERF_INPUT_RAYS) {
            if (sample_t) fail("lnerf_render_maps: sample_t must be NULL in RAYS mode (the engine samples the depths)");
        } else if (ro.depth && !sample_t) {
            fail("lnerf_render_maps: depth needs sample_t (rays, S) in POINTS / ENCODED mode");
        }
        lnerf_outputs o{};
        o.loss = ro.loss;
        o.acc_color = ro.acc_color;
        comp::MapsArgs maps{ro.depth, ro.opacity, ro.weights, ro.rgba, sample_t};
        check_precision_flags(flags);
        render_call(ctx, "lnerf_render_maps", *mlp, ws, bs, *batch, flags, o, &maps, stream);
    });
}

extern "C" int lnerf_render_maps_vjp(lnerf_ctx* ctx, const lnerf_mlp* mlp, const float* ws, const float* bs,
                                     const lnerf_batch* batch, const float* sample_t,
                                     const lnerf_render_adjoints* adj, int flags, const lnerf_outputs* out,
                                     void* stream) {
    return guard_int([&]() {
        if (!ctx) fail("null ctx");
        constexpr int kRefused = LNERF_SEED_LOSS | LNERF_HEAD_FIT | LNERF_K16_W4 | LNERF_RENDER_K16;
        if (flags & kRefused)
            fail("lnerf_render_maps_vjp: flags 0x%x (LNERF_SEED_LOSS / LNERF_HEAD_FIT / LNERF_K16_W4 / "
                 "LNERF_RENDER_K16) have no meaning here", flags & kRefused);
        validate_call(mlp, batch, flags, ws, bs, false);
        if (!adj) fail("lnerf_render_maps_vjp: null adjoints");
        const comp::VjpArgs vjp{adj->d_acc_color, adj->d_depth, adj->d_opacity, adj->d_weights, adj->d_rgba, sample_t};
        if (!vjp.d_acc_color && !vjp.d_depth && !vjp.d_opacity && !vjp.d_weights && !vjp.d_rgba)
            fail("lnerf_render_maps_vjp: every adjoint is NULL (nothing to reverse)");
        if ((uintptr_t)vjp.d_rgba % 16) fail("lnerf_render_maps_vjp: adj->d_rgba must be 16-byte aligned (one load per sample)");
        if (batch->input_mode == LNERF_INPUT_RAYS) {
            if (sample_t) fail("lnerf_render_maps_vjp: sample_t must be NULL in RAYS mode (the engine samples the depths)");
        } else if (vjp.d_depth && !sample_t) {
            fail("lnerf_render_maps_vjp: d_depth needs sample_t (rays, S) in POINTS / ENCODED mode");
        }
        lnerf_outputs o = out ? *out : lnerf_outputs{};
        if (o.loss || o.d_target)
            fail("lnerf_render_maps_vjp: out->loss and out->d_target must be NULL (there is no loss and no target)");
        float* d_input = resolve_dinput(flags, *batch, o);   // d_x as lnerf_train_step forms it
        check_precision_flags(flags);
        training_call(ctx, "lnerf_render_maps_vjp", *mlp, ws, bs, *batch, 1.0f, flags, o, d_input, &vjp, stream);
    });
}

extern "C" int lnerf_ctx_timings(lnerf_ctx* ctx, float* ms_out, int n) {
    int written = 0;
    const int rc = guard_int([&]() {
        if (!ctx || !ms_out) fail("null argument");
        if (!ctx->timed) return;
        HIP_OK(hipEventSynchronize(ctx->ev[5]));
        float v[6];
        for (int i = 0; i < 5; ++i) HIP_OK(hipEventElapsedTime(&v[i], ctx->ev[i], ctx->ev[i + 1]));
        HIP_OK(hipEventElapsedTime(&v[5], ctx->ev[0], ctx->ev[5]));
        for (int i = 0; i < 6 && i < n; ++i) ms_out[written++] = v[i];
    });
    return rc != 0 ? rc : written;
}

extern "C" int lnerf_ctx_last_path(lnerf_ctx* ctx) {
    int path = 0;
    const int rc = guard_int([&]() {
        if (!ctx) fail("null ctx");
        std::lock_guard<std::mutex> lock(ctx->mu);
        path = ctx->last_path;
    });
    return rc != 0 ? rc : path;
}

extern "C" size_t lnerf_ctx_workspace_used(lnerf_ctx* ctx) {
    if (!ctx) return 0;
    std::lock_guard<std::mutex> lock(ctx->mu);
    return ctx->ws_used;
}

extern "C" int lnerf_ctx_relu_masks(lnerf_ctx* ctx, unsigned char* out, size_t out_bytes, void* stream) {
    return guard_int([&]() {
        if (!ctx) fail("null argument");
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!ctx->last_k16_train) fail("no k16 training step has run on this context since the last other call");
        const FusedPlan& p = ctx->last_plan;
        const size_t need = (size_t)(p.L - 1) * p.R * 32;
        if (need == 0) return;   // a head-only MLP has no hidden layer: nothing to write (out may be NULL)
        if (!out) fail("null argument");
        if (out_bytes < need) fail("relu mask buffer holds %zu bytes, needs %zu", out_bytes, need);
        HIP_OK(hipSetDevice(ctx->device));
        k16_masks_launch(p, out, (hipStream_t)stream);
        check_launch("lnerf_ctx_relu_masks");
    });
}

extern "C" int lnerf_ctx_exceptional_rows(lnerf_ctx* ctx, long long* rows, long long* last_samples) {
    return guard_int([&]() {
        if (!ctx || !rows) fail("null argument");
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (!ctx->last_k16_train) fail("no k16 training step has run on this context since the last other call");
        const FusedPlan& p = ctx->last_plan;
        *rows = 0;
        if (last_samples) *last_samples = 0;
        if (p.x6 != 2) return;   // only the fp16x3 split has exceptional rows
        HIP_OK(hipSetDevice(ctx->device));
        std::vector<int> c((size_t)2 * p.dw_grid);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(c.data(), p.xcount, c.size() * sizeof(int), hipMemcpyDeviceToHost));
        long long t = 0, l = 0;
        for (int i = 0; i < p.dw_grid; ++i) {
            t += c[2 * i];
            l += c[2 * i + 1];
        }
        *rows = t;
        if (last_samples) *last_samples = l;
    });
}

extern "C" int lnerf_ctx_guard_fired(lnerf_ctx* ctx, int* fired) {
    return guard_int([&]() {
        if (!ctx || !fired) fail("null argument");
        std::lock_guard<std::mutex> lock(ctx->mu);
        *fired = -1;   // no guard on the last call (the generic path, a render, an explicit precision)
        if (!ctx->last_k16_train) return;
        const FusedPlan& p = ctx->last_plan;
        if (!p.guard) return;
        HIP_OK(hipSetDevice(ctx->device));
        HIP_OK(hipDeviceSynchronize());
        int w = 0;
        HIP_OK(hipMemcpy(&w, p.guard, sizeof(int), hipMemcpyDeviceToHost));
        *fired = w != 0 ? 1 : 0;
    });
}

extern "C" int lnerf_ctx_set_option(lnerf_ctx* ctx, int option, int value) {
    return guard_int([&]() {
        if (!ctx) fail("null ctx");
        std::lock_guard<std::mutex> lock(ctx->mu);
        switch (option) {
            case LNERF_OPT_DW_GRID:
                if (value != 0 && (value < 16 || value > 4096)) fail("LNERF_OPT_DW_GRID %d outside 16..4096", value);
                ctx->dw_grid = value;
                break;
            default:
                fail("unknown option %d", option);
        }
    });
}

extern "C" int lnerf_scale_by_device_scalar(float* buf, size_t n, const float* scale, void* stream) {
    return guard_int([&]() {
        k_scale_by_scalar(buf, n, scale, (hipStream_t)stream);
        check_launch("lnerf_scale_by_device_scalar");
    });
}

extern "C" int lnerf_adam_update(float* params, const float* grads, float* m, float* v, size_t n,
                                 int t, float lr, float beta1, float beta2, float eps,
                                 void* stream) {
    return guard_int([&]() {
        if (t < 1) fail("adam step t must be >= 1");
        k_adam(params, grads, m, v, n, t, lr, beta1, beta2, eps, (hipStream_t)stream);
        check_launch("lnerf_adam_update");
    });
}
