"""Python binding of libloma_nerf.so (include/lnerf.h) -- the host side of the MI355X engine.

Two surfaces:
  * `load_library()` returns the ctypes CDLL with argtypes for every exported symbol (the
    loma-compat ones are what `compiler.compile` hands to train_nerf.py / fit_img.py).
  * `Engine` drives the native batched API on torch device tensors (torch is used only for
    device memory and streams). There is no CPU fallback: without the library or a GPU the
    calls raise.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

HERE = os.path.dirname(os.path.abspath(__file__))
# LNERF_LIB: an alternative in-tree build (e.g. the LNERF_PROF phase-counter variant)
LIB_PATH = os.environ.get("LNERF_LIB") or os.path.join(HERE, "lib", "libloma_nerf.so")
MAX_LAYERS = 16

INPUT_ENCODED = 0
INPUT_POINTS = 1
INPUT_RAYS = 2
SEED_CONST = 0
SEED_LOSS = 1
ACCUMULATE = 2
WANT_DX = 4
GENERIC = 8
FAST = 16
TIMING = 32
MFMA_F32 = 64     # removed in round 4 (one-wave exact-f32 kernel): an error; exact fp32 is GENERIC
MFMA_BF16 = 128   # fused path: plain bf16 operands (reduced precision; inference)
MFMA_F16X3 = 256  # fused path: fp16x3 split (22-bit products, fp32 accumulate; the k16 default)
MFMA_BF16X6 = 512  # fused path: bf16x6 split (fp32-accurate products)
ONE_WAVE = 1024    # removed in round 4 (the one-wave-per-SIMD kernel pair): an error
K32 = 2048         # removed in round 4 (k32 lost to k16): an error
K16_W4 = 4096      # fused path: k16 on 4-wave 64-sample workgroups, two per CU (A/B)
HEAD_FIT = 8192    # the mlp_fit head (sigmoid on every output, no compositing; samples = 1)
RENDER_K16 = 16384  # render (plain bf16) on k16's forward instead of kr (A/B)
WANT_DINPUT = 32768  # d_x = the gradient with respect to the batch's own x, in x's layout
HASHGRID_REPRODUCIBLE = 65536  # lnerf_hashgrid_grad: d_table as ordered float64 sums, the same bits every call

OPT_DW_GRID = 1    # lnerf_ctx_set_option: dW workgroups per step (0 = default 512)

# every symbol include/lnerf.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "nerf_evaluate_and_march", "grad_nerf_evaluate_and_march", "mlp_fit", "grad_mlp_fit",
    "mult_a_b", "lnerf_last_error", "lnerf_version", "lnerf_ctx_create", "lnerf_ctx_destroy",
    "lnerf_workspace_bytes", "lnerf_train_step", "lnerf_render", "lnerf_scale_by_device_scalar",
    "lnerf_adam_update", "lnerf_ctx_timings", "lnerf_get_rays", "lnerf_ctx_last_path",
    "lnerf_ctx_set_option", "lnerf_ctx_relu_masks", "lnerf_build_knobs", "lnerf_ctx_exceptional_rows",
    "lnerf_ctx_guard_fired", "lnerf_input_grad", "lnerf_pose_grad", "lnerf_ctx_workspace_used",
    "lnerf_render_maps", "lnerf_sample_stratified", "lnerf_sample_importance", "lnerf_ray_points",
    "lnerf_ray_points_grad", "lnerf_render_maps_vjp", "lnerf_hashgrid_init", "lnerf_hashgrid_encode",
    "lnerf_hashgrid_grad", "lnerf_hashgrid_grad_scratch", "lnerf_occgrid_cell_points", "lnerf_occgrid_update", "lnerf_occgrid_threshold",
    "lnerf_sample_occupancy",
]

# lnerf_ctx_last_path bits
PATH_GENERIC = 1
PATH_FUSED = 2
PATH_K16 = 4
PATH_DW16 = 8
PATH_K32 = 16      # reserved (k32, removed in round 4)
PATH_K16_W4 = 32
PATH_KR = 64       # the render ran kr (lnerf_render.hip)
PATH_A24 = 128      # training kept the activation slabs as int24 (fp16x3)
PATH_MAPS = 1024    # lnerf_render_maps: the MAPS instantiations (bits 8-9 hold the plane count)
PATH_VJP = 2048     # lnerf_render_maps_vjp: the training step's bits plus this one


class LnerfMLP(ctypes.Structure):
    _fields_ = [("num_layers", ctypes.c_int), ("k", ctypes.c_int * MAX_LAYERS),
                ("n", ctypes.c_int * MAX_LAYERS), ("w_k", ctypes.c_int), ("w_n", ctypes.c_int)]


class LnerfBatch(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_int), ("samples", ctypes.c_int), ("input_mode", ctypes.c_int),
                ("num_freqs", ctypes.c_int), ("x", ctypes.c_void_p), ("dists", ctypes.c_void_p),
                ("target", ctypes.c_void_p), ("near_t", ctypes.c_float), ("far_t", ctypes.c_float)]


class LnerfOutputs(ctypes.Structure):
    _fields_ = [("loss", ctypes.c_void_p), ("acc_color", ctypes.c_void_p),
                ("d_ws", ctypes.c_void_p), ("d_bs", ctypes.c_void_p), ("d_x", ctypes.c_void_p),
                ("d_dists", ctypes.c_void_p), ("d_target", ctypes.c_void_p)]


class LnerfRenderOutputs(ctypes.Structure):
    _fields_ = [("acc_color", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("opacity", ctypes.c_void_p),
                ("weights", ctypes.c_void_p), ("rgba", ctypes.c_void_p), ("loss", ctypes.c_void_p)]


class LnerfRenderAdjoints(ctypes.Structure):
    _fields_ = [("d_acc_color", ctypes.c_void_p), ("d_depth", ctypes.c_void_p), ("d_opacity", ctypes.c_void_p),
                ("d_weights", ctypes.c_void_p), ("d_rgba", ctypes.c_void_p)]


HASHGRID_MAX_LEVELS = 32


class LnerfHashGrid(ctypes.Structure):
    _fields_ = [("levels", ctypes.c_int), ("features", ctypes.c_int), ("log2_table", ctypes.c_int),
                ("res", ctypes.c_int * HASHGRID_MAX_LEVELS),
                ("offset", ctypes.c_longlong * (HASHGRID_MAX_LEVELS + 1)),
                ("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3)]


OCC_MEAN = 1          # lnerf_occgrid_threshold: thr = min(threshold, mean(density))
OCC_LAST_OPAQUE = 2   # lnerf_sample_occupancy: the last dist of every ray is 1e8


class LnerfOccGrid(ctypes.Structure):
    _fields_ = [("res", ctypes.c_int), ("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3)]


_LIB = None

_F = ctypes.POINTER(ctypes.c_float)
_FF = ctypes.POINTER(_F)
_FFF = ctypes.POINTER(_FF)
_I = ctypes.POINTER(ctypes.c_int)
_II = ctypes.POINTER(_I)

# loma argtypes (compiler.py:25-51 mapping of the scripts/*.py signatures)
NERF_ARGTYPES = [_FF, ctypes.c_int, ctypes.c_int, _FFF, _FF, _FF, ctypes.c_int, ctypes.c_int,
                 ctypes.c_int, _II, _II, _II, _FFF, _FFF, ctypes.c_int, _FF, _FF, _FF, _FF, _FF]
MLP_FIT_ARGTYPES = [_FF, ctypes.c_int, ctypes.c_int, _FF, _FFF, _FF, _FF, ctypes.c_int,
                    ctypes.c_int, ctypes.c_int, _II, _II, _II, _FFF]
MULT_A_B_ARGTYPES = [_FF, ctypes.c_int, ctypes.c_int, _FF, ctypes.c_int, ctypes.c_int, _FF]


def rev_argtypes(fwd, ret_is_float=True):
    """reverse_diff.py:504-517: every In arg x is followed by an Out adjoint of x's type (arrays
    keep their pointer type, scalars become pointers); the float return adds a `_dreturn`."""
    out = []
    for t in fwd:
        out.append(t)
        out.append(t if issubclass(t, ctypes._Pointer) else ctypes.POINTER(t))
    if ret_is_float:
        out.append(ctypes.c_float)
    return out


def _preload_torch():
    # One HIP runtime per process: when torch is importable, let it load its libamdhip64 first so
    # ours resolves to the same SONAME instead of mapping a second copy.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch absent
        pass


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load libloma_nerf.so and set argtypes. Raises if the library is missing (no fallback)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"libloma_nerf.so not built at {p} (run __graft_entry__.build())")
    _preload_torch()
    lib = ctypes.CDLL(p)
    configure(lib)
    if path is None:
        _LIB = lib
    return lib


def configure(lib: ctypes.CDLL) -> None:
    lib.nerf_evaluate_and_march.argtypes = NERF_ARGTYPES
    lib.nerf_evaluate_and_march.restype = ctypes.c_float
    lib.grad_nerf_evaluate_and_march.argtypes = rev_argtypes(NERF_ARGTYPES)
    lib.grad_nerf_evaluate_and_march.restype = None
    lib.mlp_fit.argtypes = MLP_FIT_ARGTYPES
    lib.mlp_fit.restype = ctypes.c_float
    lib.grad_mlp_fit.argtypes = rev_argtypes(MLP_FIT_ARGTYPES)
    lib.grad_mlp_fit.restype = None
    lib.mult_a_b.argtypes = MULT_A_B_ARGTYPES
    lib.mult_a_b.restype = None
    lib.lnerf_last_error.restype = ctypes.c_char_p
    lib.lnerf_version.restype = ctypes.c_char_p
    lib.lnerf_build_knobs.argtypes = []
    lib.lnerf_build_knobs.restype = ctypes.c_uint
    lib.lnerf_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    lib.lnerf_ctx_destroy.argtypes = [ctypes.c_void_p]
    lib.lnerf_ctx_destroy.restype = None
    lib.lnerf_workspace_bytes.argtypes = [ctypes.POINTER(LnerfMLP), ctypes.c_int, ctypes.c_int]
    lib.lnerf_workspace_bytes.restype = ctypes.c_size_t
    lib.lnerf_train_step.argtypes = [ctypes.c_void_p, ctypes.POINTER(LnerfMLP), ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.POINTER(LnerfBatch), ctypes.c_float,
                                     ctypes.c_int, ctypes.POINTER(LnerfOutputs), ctypes.c_void_p]
    lib.lnerf_render.argtypes = [ctypes.c_void_p, ctypes.POINTER(LnerfMLP), ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.POINTER(LnerfBatch), ctypes.c_int,
                                 ctypes.POINTER(LnerfOutputs), ctypes.c_void_p]
    lib.lnerf_scale_by_device_scalar.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                 ctypes.c_void_p]
    lib.lnerf_adam_update.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    lib.lnerf_ctx_timings.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    lib.lnerf_ctx_last_path.argtypes = [ctypes.c_void_p]
    lib.lnerf_ctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.lnerf_ctx_relu_masks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    if hasattr(lib, "lnerf_ctx_exceptional_rows"):   # (older in-tree A/B builds lack it)
        lib.lnerf_ctx_exceptional_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                                   ctypes.POINTER(ctypes.c_longlong)]
    if hasattr(lib, "lnerf_ctx_guard_fired"):   # (round 6; older A/B builds lack it)
        lib.lnerf_ctx_guard_fired.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    if hasattr(lib, "lnerf_ctx_workspace_used"):   # (older in-tree A/B builds lack it)
        lib.lnerf_ctx_workspace_used.argtypes = [ctypes.c_void_p]
        lib.lnerf_ctx_workspace_used.restype = ctypes.c_size_t
    lib.lnerf_get_rays.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "lnerf_input_grad"):   # (older in-tree A/B builds lack the input gradients)
        lib.lnerf_input_grad.argtypes = [ctypes.POINTER(LnerfBatch), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]
        lib.lnerf_input_grad.restype = ctypes.c_int
        lib.lnerf_pose_grad.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.lnerf_pose_grad.restype = ctypes.c_int
    if hasattr(lib, "lnerf_render_maps"):   # (older in-tree A/B builds lack the render maps)
        lib.lnerf_render_maps.argtypes = [ctypes.c_void_p, ctypes.POINTER(LnerfMLP), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.POINTER(LnerfBatch), ctypes.c_void_p,
                                          ctypes.c_int, ctypes.POINTER(LnerfRenderOutputs), ctypes.c_void_p]
        lib.lnerf_render_maps.restype = ctypes.c_int
    if hasattr(lib, "lnerf_render_maps_vjp"):   # (older in-tree A/B builds lack the render's reverse)
        lib.lnerf_render_maps_vjp.argtypes = [ctypes.c_void_p, ctypes.POINTER(LnerfMLP), ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.POINTER(LnerfBatch), ctypes.c_void_p,
                                              ctypes.POINTER(LnerfRenderAdjoints), ctypes.c_int,
                                              ctypes.POINTER(LnerfOutputs), ctypes.c_void_p]
        lib.lnerf_render_maps_vjp.restype = ctypes.c_int
    if hasattr(lib, "lnerf_sample_importance"):   # (older in-tree A/B builds lack the sampling kernels)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.lnerf_sample_stratified.argtypes = [ci, ci, cf, cf, vp, vp, vp]
        lib.lnerf_sample_importance.argtypes = [ci, ci, vp, cf, cf, vp, ci, vp, vp, vp, vp]
        lib.lnerf_ray_points.argtypes = [vp, ci, ci, vp, vp, vp, vp]
        lib.lnerf_ray_points_grad.argtypes = [ci, ci, vp, vp, vp, vp, vp]
        for name in ("lnerf_sample_stratified", "lnerf_sample_importance", "lnerf_ray_points",
                     "lnerf_ray_points_grad"):
            getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "lnerf_hashgrid_encode"):   # (older in-tree A/B builds lack the hash grid)
        vp, ci, ll, hg = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(LnerfHashGrid)
        lib.lnerf_hashgrid_init.argtypes = [hg, ci, ci, ci, ci, ci, _F, _F]
        lib.lnerf_hashgrid_init.restype = ll
        lib.lnerf_hashgrid_encode.argtypes = [hg, vp, vp, ll, vp, vp]
        lib.lnerf_hashgrid_encode.restype = ci
        lib.lnerf_hashgrid_grad.argtypes = [hg, vp, vp, ll, vp, vp, ci, vp, vp, vp]
        lib.lnerf_hashgrid_grad.restype = ci
        if hasattr(lib, "lnerf_hashgrid_grad_scratch"):
            lib.lnerf_hashgrid_grad_scratch.argtypes = [hg, ll, vp]
            lib.lnerf_hashgrid_grad_scratch.restype = ll
    if hasattr(lib, "lnerf_sample_occupancy"):   # (older in-tree A/B builds lack the occupancy grid)
        vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
        og = ctypes.POINTER(LnerfOccGrid)
        lib.lnerf_occgrid_cell_points.argtypes = [og, vp, ll, vp, vp, vp]
        lib.lnerf_occgrid_update.argtypes = [og, vp, vp, ll, vp, ci, cf, vp]
        lib.lnerf_occgrid_threshold.argtypes = [og, vp, cf, ci, vp, vp, vp, vp]
        lib.lnerf_sample_occupancy.argtypes = [og, vp, vp, ci, ci, ci, cf, cf, vp, ci, vp, vp, vp, vp]
        for name in ("lnerf_occgrid_cell_points", "lnerf_occgrid_update", "lnerf_occgrid_threshold",
                     "lnerf_sample_occupancy"):
            getattr(lib, name).restype = ci
    for name in ("lnerf_ctx_timings", "lnerf_ctx_last_path", "lnerf_ctx_set_option", "lnerf_ctx_relu_masks",
                 "lnerf_ctx_exceptional_rows", "lnerf_ctx_guard_fired",
                 "lnerf_ctx_create", "lnerf_train_step", "lnerf_render",
                 "lnerf_scale_by_device_scalar", "lnerf_adam_update", "lnerf_get_rays"):
        if hasattr(lib, name):
            getattr(lib, name).restype = ctypes.c_int


def build_knobs() -> int:
    """lnerf_build_knobs(): non-default compile-time knobs of the loaded library (0 = product)."""
    return int(load_library().lnerf_build_knobs())


def last_error() -> str:
    return load_library().lnerf_last_error().decode()


def make_mlp(shapes, w_k: int, w_n: int) -> LnerfMLP:
    m = LnerfMLP()
    m.num_layers = len(shapes)
    for l, (k, n) in enumerate(shapes):
        m.k[l], m.n[l] = int(k), int(n)
    m.w_k, m.w_n = int(w_k), int(w_n)
    return m


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class HashGrid:
    """A multiresolution hash grid (lnerf.h "Multiresolution hash grid"): `levels` grids from base_res
    to max_res points per axis over the box [lo, hi], `features` values per grid point, each level
    dense or hashed into 2^log2_table entries. Wraps the lnerf_hashgrid struct that
    lnerf_hashgrid_init fills (host only: no GPU is needed to build one). `struct` is what the entry
    points take; its fields may also be set by hand (from_levels)."""

    def __init__(self, levels: int = 16, features: int = 2, log2_table: int = 19, base_res: int = 16,
                 max_res: int = 2048, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
        self.struct = LnerfHashGrid()
        lo3, hi3 = (ctypes.c_float * 3)(*map(float, lo)), (ctypes.c_float * 3)(*map(float, hi))
        total = load_library().lnerf_hashgrid_init(ctypes.byref(self.struct), int(levels), int(features),
                                                   int(log2_table), int(base_res), int(max_res), lo3, hi3)
        if total < 0:
            raise ValueError(f"lnerf_hashgrid_init: {last_error()}")

    @classmethod
    def from_levels(cls, res, features: int, log2_table: int, lo, hi, align: int = 4):
        """A grid with the given per-level resolutions, filled by hand: level l gets res^3 entries
        if that is at most 2^log2_table, else 2^log2_table, rounded up to a multiple of `align`. The
        library validates it when it is used."""
        self = cls.__new__(cls)
        g = self.struct = LnerfHashGrid()
        g.levels, g.features, g.log2_table = len(res), int(features), int(log2_table)
        off = 0
        for l, r in enumerate(res):
            g.res[l] = int(r)
            g.offset[l] = off
            off += -(-min(int(r) ** 3, 1 << int(log2_table)) // align) * align
        g.offset[len(res)] = off
        for c in range(3):
            g.lo[c], g.hi[c] = float(lo[c]), float(hi[c])
        return self

    levels = property(lambda self: int(self.struct.levels))
    features = property(lambda self: int(self.struct.features))
    log2_table = property(lambda self: int(self.struct.log2_table))
    res = property(lambda self: [int(self.struct.res[l]) for l in range(self.levels)])
    offsets = property(lambda self: [int(self.struct.offset[l]) for l in range(self.levels + 1)])
    lo = property(lambda self: [float(v) for v in self.struct.lo])
    hi = property(lambda self: [float(v) for v in self.struct.hi])

    @property
    def total_entries(self) -> int:
        return int(self.struct.offset[self.levels])

    @property
    def width(self) -> int:
        """The encoding's width levels * F: the MLP's k[0]."""
        return self.levels * self.features

    def new_table(self, std: float = 1e-4, seed: int = 0, device="cuda:0"):
        """A (total_entries, F) float32 table of normal(0, std) values from a seeded generator."""
        import torch
        gen = torch.Generator().manual_seed(int(seed))
        t = torch.randn(self.total_entries, self.features, generator=gen, dtype=torch.float32) * float(std)
        return t.to(device)


class OccGrid:
    """An occupancy grid (lnerf.h "Occupancy grid"): res^3 cells over the box [lo, hi], res a power
    of two in 4..256. It owns no device memory: `density` (num_cells float32, a decayed running
    maximum of sigma) and `bits` (num_cells / 32 int32 words, cell c = bit c & 31 of word c >> 5) are
    the caller's tensors, made by new_density / new_bits. `struct` is what the entry points take; the
    library validates it on every call."""

    def __init__(self, res: int = 128, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
        g = self.struct = LnerfOccGrid()
        g.res = int(res)
        for c in range(3):
            g.lo[c], g.hi[c] = float(lo[c]), float(hi[c])

    res = property(lambda self: int(self.struct.res))
    lo = property(lambda self: [float(v) for v in self.struct.lo])
    hi = property(lambda self: [float(v) for v in self.struct.hi])

    @property
    def num_cells(self) -> int:
        return self.res ** 3

    def new_density(self, device="cuda:0"):
        """(num_cells,) float32 zeros."""
        import torch
        return torch.zeros(self.num_cells, dtype=torch.float32, device=device)

    def new_bits(self, device="cuda:0"):
        """(num_cells / 32,) int32 zeros: the bitfield's uint32 words (torch has no uint32 arithmetic;
        the bit patterns are the library's)."""
        import torch
        return torch.zeros(self.num_cells // 32, dtype=torch.int32, device=device)


@dataclass
class StepResult:
    loss: object        # torch scalar tensor (device)
    acc_color: object   # (rays, 3)
    grads: object       # packed [d_ws (L*w_k*w_n), d_bs (L*w_n), loss] (device)
    d_ws: object
    d_bs: object
    d_dists: object = None
    d_target: object = None
    d_x: object = None
    d_input: object = None   # want_dinput: the gradient with respect to x, in x's shape


@dataclass
class RenderMaps:
    """Engine.render_maps' result: device tensors, None where not asked for."""
    color: object = None     # (rays, 3)
    depth: object = None     # (rays)      sum_j w_j t_j, not divided by the opacity
    opacity: object = None   # (rays)      sum_j w_j
    weights: object = None   # (rays, S)   w_j = alpha_j T_j (the reference's inclusive transmittance)
    rgba: object = None      # (rays*S, 4) sigmoid(rgb), ReLU(sigma)
    loss: object = None      # scalar; only with a target


MAP_NAMES = ("color", "depth", "opacity", "weights", "rgba", "loss")
ADJOINT_NAMES = ("color", "depth", "opacity", "weights", "rgba")   # the maps render_maps_vjp reverses


@dataclass
class VjpResult:
    """Engine.render_maps_vjp's result: device tensors, None where not asked for."""
    acc_color: object        # (rays, 3), the recomputed colour (train_step's bits)
    grads: object            # packed [d_ws (L*w_k*w_n), d_bs (L*w_n), unused] (device)
    d_ws: object
    d_bs: object
    d_dists: object = None   # (rays, S)
    d_x: object = None       # want_dx: (rays*S, k[0])
    d_input: object = None   # want_dinput: the gradient with respect to x, in x's shape


class Engine:
    """Native-API driver on one GPU. Inputs are torch tensors already resident on the device."""

    def __init__(self, device: int = 0):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.device = device
        h = ctypes.c_void_p()
        if self.lib.lnerf_ctx_create(ctypes.byref(h), device) != 0:
            raise RuntimeError(f"lnerf_ctx_create: {last_error()}")
        self.ctx = h

    def close(self):
        if self.ctx:
            self.lib.lnerf_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def alloc_grads(self, L: int, w_k: int, w_n: int):
        nW, nB = L * w_k * w_n, L * w_n
        g = self.torch.zeros(nW + nB + 1, dtype=self.torch.float32, device=f"cuda:{self.device}")
        return g, g[:nW].view(L, w_k, w_n), g[nW:nW + nB].view(L, w_n), g[nW + nB:]

    @staticmethod
    def _batch(rays, samples, input_mode, num_freqs, x, dists, target, near, far):
        return LnerfBatch(rays, samples, input_mode, num_freqs, x.data_ptr(),
                          None if dists is None else dists.data_ptr(), target.data_ptr(),
                          float(near), float(far))

    def train_step(self, mlp: LnerfMLP, ws, bs, x, dists, target, *, samples: int,
                   input_mode: int = INPUT_POINTS, num_freqs: int = 5, seed=None, flags: int = 0,
                   grads=None, want_per_ray: bool = False, want_dx: bool = False,
                   acc_color=None, near: float = 2.0, far: float = 6.0,
                   want_dinput: bool = False) -> StepResult:
        """One fwd+bwd over the batch. seed=None seeds with the batch loss (train_nerf.py:477);
        a float seeds with that constant. `grads` (from alloc_grads) is reused if given.
        INPUT_RAYS: x = (rays, 6) [o, d], dists=None, samples at linspace(near, far, S).
        want_dinput: StepResult.d_input = the gradient with respect to x, in x's shape (WANT_DINPUT)."""
        torch = self.torch
        rays = target.shape[0]
        b = self._batch(rays, samples, input_mode, num_freqs, x, dists, target, near, far)
        if grads is None:
            grads = self.alloc_grads(mlp.num_layers, mlp.w_k, mlp.w_n)
        g, dws, dbs, loss = grads
        if acc_color is None:
            acc_color = torch.empty(rays, 3, dtype=torch.float32, device=target.device)
        d_dists = d_target = d_x = None
        if want_per_ray:
            d_dists = torch.empty(rays, samples, dtype=torch.float32, device=target.device)
            d_target = torch.empty(rays, 3, dtype=torch.float32, device=target.device)
        if want_dx:
            d_x = torch.zeros(rays * samples, mlp.k[0], dtype=torch.float32, device=target.device)
            flags |= WANT_DX
        d_input = None
        if want_dinput:
            # (both flags at once: the library decides -- an error unless x is ENCODED)
            d_input = d_x if d_x is not None else torch.zeros_like(x, dtype=torch.float32)
            d_x = d_input
            flags |= WANT_DINPUT
        o = LnerfOutputs(loss.data_ptr(), acc_color.data_ptr(), dws.data_ptr(), dbs.data_ptr(),
                         None if d_x is None else d_x.data_ptr(),
                         None if d_dists is None else d_dists.data_ptr(),
                         None if d_target is None else d_target.data_ptr())
        if seed is None:
            flags |= SEED_LOSS
            seed = 1.0
        rc = self.lib.lnerf_train_step(self.ctx, ctypes.byref(mlp), ws.data_ptr(), bs.data_ptr(),
                                       ctypes.byref(b), float(seed), flags, ctypes.byref(o),
                                       self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_train_step: {last_error()}")
        return StepResult(loss[0], acc_color, g, dws, dbs, d_dists, d_target,
                          d_x if want_dx else None, d_input)

    def mlp_fit_step(self, mlp: LnerfMLP, ws, bs, x, target, *, seed=None, flags: int = 0, grads=None,
                     outputs=None, want_grad: bool = True):
        """fit_img.py's chunk step on the device (scripts/mlp_fit.py): the MLP on `x` (rows, k[0])
        ENCODED rows, sigmoid on every output, loss = sum (sigmoid(z) - target)^2 over
        (rows, n_out); with want_grad the reverse pass (grad_mlp_fit) into `grads`, seeded with
        `seed` (fit_img.py:515 passes the previous chunk loss) or, seed=None, with this loss.
        Returns (loss, outputs (rows, n_out), grads)."""
        torch = self.torch
        rows, nout = target.shape[0], mlp.n[mlp.num_layers - 1]
        if outputs is None:
            outputs = torch.empty(rows, nout, dtype=torch.float32, device=target.device)
        if not want_grad:
            loss, out = self.render(mlp, ws, bs, x, None, target, samples=1, input_mode=INPUT_ENCODED,
                                    flags=flags | HEAD_FIT, acc=outputs)
            return loss, out, None
        r = self.train_step(mlp, ws, bs, x, None, target, samples=1, input_mode=INPUT_ENCODED, seed=seed,
                            flags=flags | HEAD_FIT, grads=grads, acc_color=outputs)
        return r.loss, outputs, r.grads

    def render(self, mlp: LnerfMLP, ws, bs, x, dists, target, *, samples: int,
               input_mode: int = INPUT_POINTS, num_freqs: int = 5, near: float = 2.0,
               far: float = 6.0, flags: int = 0, acc=None, loss=None):
        """Forward only (train_nerf.py:616-661 eval render): (loss, acc_color). flags may select
        MFMA_BF16 (the config-5 inference precision), MFMA_BF16X6 or GENERIC."""
        torch = self.torch
        rays = target.shape[0]
        b = self._batch(rays, samples, input_mode, num_freqs, x, dists, target, near, far)
        if acc is None:
            acc = torch.empty(rays, 3, dtype=torch.float32, device=target.device)
        if loss is None:
            loss = torch.empty(1, dtype=torch.float32, device=target.device)
        o = LnerfOutputs(loss.data_ptr(), acc.data_ptr(), None, None, None, None, None)
        rc = self.lib.lnerf_render(self.ctx, ctypes.byref(mlp), ws.data_ptr(), bs.data_ptr(),
                                   ctypes.byref(b), flags, ctypes.byref(o), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_render: {last_error()}")
        return loss[0], acc

    def render_maps(self, mlp: LnerfMLP, ws, bs, x, dists, target=None, *, samples: int,
                    input_mode: int = INPUT_POINTS, num_freqs: int = 5, near: float = 2.0,
                    far: float = 6.0, sample_t=None, flags: int = 0,
                    want=("color", "depth", "opacity"), buffers=None) -> RenderMaps:
        """lnerf_render_maps: the forward render with the colour, the expected depth sum_j w_j t_j, the
        opacity sum_j w_j, the per-sample weights and rgba, and (with a target) the loss; `want` names
        the maps to produce (MAP_NAMES), every other field of the result is None. No target is needed.
        INPUT_RAYS: the depths are the engine's own linspace(near, far, S) and sample_t must be None;
        INPUT_POINTS / INPUT_ENCODED: sample_t (rays, S) is required for "depth". `buffers` may map a
        name to a preallocated float32 device tensor to write into. An extension (lnerf.h)."""
        torch = self.torch
        unknown = set(want) - set(MAP_NAMES)
        if unknown:
            raise ValueError(f"unknown maps {sorted(unknown)} (known: {MAP_NAMES})")
        rays = x.shape[0] if input_mode == INPUT_RAYS else x.shape[0] // samples
        b = LnerfBatch(rays, samples, input_mode, num_freqs, x.data_ptr(),
                       None if dists is None else dists.data_ptr(),
                       None if target is None else target.data_ptr(), float(near), float(far))
        shapes = dict(color=(rays, 3), depth=(rays,), opacity=(rays,), weights=(rays, samples),
                      rgba=(rays * samples, 4), loss=(1,))
        bufs = {}
        for name in want:
            t = (buffers or {}).get(name)
            bufs[name] = t if t is not None else torch.empty(shapes[name], dtype=torch.float32, device=x.device)
        o = LnerfRenderOutputs(_ptr(bufs.get("color")), _ptr(bufs.get("depth")), _ptr(bufs.get("opacity")),
                               _ptr(bufs.get("weights")), _ptr(bufs.get("rgba")), _ptr(bufs.get("loss")))
        rc = self.lib.lnerf_render_maps(self.ctx, ctypes.byref(mlp), ws.data_ptr(), bs.data_ptr(),
                                        ctypes.byref(b), _ptr(sample_t), flags, ctypes.byref(o), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_render_maps: {last_error()}")
        if "loss" in bufs:
            bufs["loss"] = bufs["loss"][0]
        return RenderMaps(**bufs)

    def render_maps_vjp(self, mlp: LnerfMLP, ws, bs, x, dists, adjoints: dict, *, samples: int,
                        input_mode: int = INPUT_POINTS, num_freqs: int = 5, near: float = 2.0,
                        far: float = 6.0, sample_t=None, flags: int = 0, grads=None,
                        want_dists: bool = True, want_dx: bool = False, want_dinput: bool = False,
                        acc_color=None) -> VjpResult:
        """lnerf_render_maps_vjp: the reverse of render_maps. `adjoints` maps names of ADJOINT_NAMES to
        the float32 device tensors dL/d(map) -- color (rays, 3), depth (rays), opacity (rays), weights
        (rays, S), rgba (rays*S, 4); a missing or None entry contributes nothing, at least one is
        needed. One call recomputes the forward and returns the gradients with respect to ws, bs,
        dists and (want_dx / want_dinput, as train_step) x; the adjoints carry any loss scale.
        INPUT_POINTS / INPUT_ENCODED: sample_t (rays, S) is required with a depth adjoint. The
        gradient with respect to sample_t is weights * d_depth[:, None], a torch op on render_maps'
        weights. `grads` (from alloc_grads) is reused if given, and added into under ACCUMULATE."""
        torch = self.torch
        unknown = set(adjoints) - set(ADJOINT_NAMES)
        if unknown:
            raise ValueError(f"unknown adjoints {sorted(unknown)} (known: {ADJOINT_NAMES})")
        rays = x.shape[0] if input_mode == INPUT_RAYS else x.shape[0] // samples
        shapes = dict(color=(rays, 3), depth=(rays,), opacity=(rays,), weights=(rays, samples),
                      rgba=(rays * samples, 4))
        adj = {k: self._f32(f"adjoints[{k!r}]", v, shapes[k]) for k, v in adjoints.items() if v is not None}
        b = LnerfBatch(rays, samples, input_mode, num_freqs, x.data_ptr(),
                       None if dists is None else dists.data_ptr(), None, float(near), float(far))
        if grads is None:
            grads = self.alloc_grads(mlp.num_layers, mlp.w_k, mlp.w_n)
        g, dws, dbs, _ = grads
        if acc_color is None:
            acc_color = torch.empty(rays, 3, dtype=torch.float32, device=x.device)
        d_dists = torch.empty(rays, samples, dtype=torch.float32, device=x.device) if want_dists else None
        d_x = None
        if want_dx:
            d_x = torch.zeros(rays * samples, mlp.k[0], dtype=torch.float32, device=x.device)
            flags |= WANT_DX
        d_input = None
        if want_dinput:
            d_input = d_x if d_x is not None else torch.zeros_like(x, dtype=torch.float32)
            d_x = d_input
            flags |= WANT_DINPUT
        a = LnerfRenderAdjoints(_ptr(adj.get("color")), _ptr(adj.get("depth")), _ptr(adj.get("opacity")),
                                _ptr(adj.get("weights")), _ptr(adj.get("rgba")))
        o = LnerfOutputs(None, acc_color.data_ptr(), dws.data_ptr(), dbs.data_ptr(), _ptr(d_x), _ptr(d_dists), None)
        rc = self.lib.lnerf_render_maps_vjp(self.ctx, ctypes.byref(mlp), ws.data_ptr(), bs.data_ptr(),
                                            ctypes.byref(b), _ptr(sample_t), ctypes.byref(a), flags,
                                            ctypes.byref(o), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_render_maps_vjp: {last_error()}")
        return VjpResult(acc_color, g, dws, dbs, d_dists, d_x if want_dx else None, d_input)

    def get_rays(self, width: int, K, c2w):
        """train_nerf.py:23-62 on the device: (width*width, 6) float32 rays [o, d]."""
        import numpy as np
        torch = self.torch
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        cd = np.ascontiguousarray(np.asarray(c2w, np.float64)[:3, :4])
        out = torch.empty(width * width, 6, dtype=torch.float32, device=f"cuda:{self.device}")
        dp = ctypes.POINTER(ctypes.c_double)
        rc = self.lib.lnerf_get_rays(width, Kd.ctypes.data_as(dp), cd.ctypes.data_as(dp),
                                     ctypes.c_void_p(out.data_ptr()), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_get_rays: {last_error()}")
        return out

    def input_grad(self, x, d_encoded, *, samples: int, input_mode: int, num_freqs: int,
                   near: float = 2.0, far: float = 6.0, scale=None):
        """lnerf_input_grad: the reverse of the positional encoding (INPUT_POINTS: x (rows, 3) ->
        (rows, 3)) and of the ray sampling o + d t (INPUT_RAYS: x (rays, 6) -> (rays, 6) = [d_o, d_d])
        applied to d_encoded (rows, 3 + 6 num_freqs); `scale` is an optional device scalar."""
        torch = self.torch
        rays = x.shape[0] if input_mode == INPUT_RAYS else x.shape[0] // samples
        rows = rays * samples
        if input_mode == INPUT_POINTS and x.shape[0] != rows:
            raise ValueError(f"{x.shape[0]} points are not whole rays of {samples} samples")
        if tuple(d_encoded.shape) != (rows, 3 + 6 * num_freqs):
            raise ValueError(f"d_encoded is {tuple(d_encoded.shape)}, expected {(rows, 3 + 6 * num_freqs)}")
        b = LnerfBatch(rays, samples, input_mode, num_freqs, x.data_ptr(), None, None, float(near), float(far))
        out = torch.empty_like(x, dtype=torch.float32)
        rc = self.lib.lnerf_input_grad(ctypes.byref(b), _ptr(d_encoded), _ptr(scale), _ptr(out), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_input_grad: {last_error()}")
        return out

    def pose_grad(self, width: int, K, d_rays, pixels=None):
        """lnerf_pose_grad, the reverse of get_rays: d_c2w as a float64 (3, 4) device tensor from
        d_rays (n, 6); `pixels` (optional int32 device tensor, n indices into the width x width grid,
        repeats allowed) names each ray's pixel, None means ray p is pixel p."""
        import numpy as np
        torch = self.torch
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        if pixels is not None and (pixels.dtype != torch.int32 or pixels.numel() != d_rays.shape[0]):
            raise ValueError("pixels must be int32, one index per ray")
        out = torch.empty(3, 4, dtype=torch.float64, device=d_rays.device)
        rc = self.lib.lnerf_pose_grad(width, Kd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _ptr(pixels),
                                      d_rays.shape[0], _ptr(d_rays), _ptr(out), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_pose_grad: {last_error()}")
        return out

    def _f32(self, name, t, shape=None):
        """`t` must be a contiguous float32 tensor on this engine's device (of `shape`, if given)."""
        torch = self.torch
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor")
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{name} must live on cuda:{self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} is {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def sample_stratified(self, rays: int, samples: int, u, near: float = 2.0, far: float = 6.0):
        """lnerf_sample_stratified: (rays, samples) float32 depths, one per cell of
        linspace(near, far, samples), placed inside its cell by u (rays, samples) in [0, 1] -- the
        caller's random numbers (e.g. torch.rand); non-decreasing along each ray."""
        self._f32("u", u, (rays, samples))
        out = self.torch.empty(rays, samples, dtype=self.torch.float32, device=u.device)
        rc = self.lib.lnerf_sample_stratified(rays, samples, float(near), float(far), _ptr(u), _ptr(out),
                                              self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_sample_stratified: {last_error()}")
        return out

    def sample_importance(self, weights, n_fine: int, t_coarse=None, u=None, near: float = 2.0,
                          far: float = 6.0, want=("fine", "all")):
        """lnerf_sample_importance: n_fine depths per ray drawn from the coarse pass's `weights`
        (rays, S), as render_maps(want=("weights",)) returns them. t_coarse (rays, S) are the coarse
        depths (None: the engine's linspace(near, far, S)), u (rays, n_fine) the caller's random
        numbers (None: the deterministic (k + 0.5) / n_fine). Returns (t_fine (rays, n_fine) in u's
        order, t_all (rays, S + n_fine) = the coarse and fine depths merged in order); an entry `want`
        does not name is None."""
        unknown = set(want) - {"fine", "all"}
        if unknown or not want:
            raise ValueError(f"want must name 'fine' and / or 'all', got {tuple(want)}")
        if weights.dim() != 2:
            raise ValueError(f"weights is {tuple(weights.shape)}, expected (rays, S)")
        rays, S = weights.shape
        self._f32("weights", weights)
        if t_coarse is not None:
            self._f32("t_coarse", t_coarse, (rays, S))
        if u is not None:
            self._f32("u", u, (rays, n_fine))
        torch = self.torch
        fine = torch.empty(rays, n_fine, dtype=torch.float32, device=weights.device) if "fine" in want else None
        both = torch.empty(rays, S + n_fine, dtype=torch.float32, device=weights.device) if "all" in want else None
        rc = self.lib.lnerf_sample_importance(rays, S, _ptr(t_coarse), float(near), float(far), _ptr(weights),
                                              int(n_fine), _ptr(u), _ptr(fine), _ptr(both), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_sample_importance: {last_error()}")
        return fine, both

    def ray_points(self, rays, sample_t):
        """lnerf_ray_points: (points (n*S, 3), dists (n, S)) of rays (n, 6) = [o, d] at the per-ray
        depths sample_t (n, S): points o + d t and dists = [diff(t), 1e8], ready for INPUT_POINTS
        (and sample_t for render_maps)."""
        if sample_t.dim() != 2:
            raise ValueError(f"sample_t is {tuple(sample_t.shape)}, expected (rays, S)")
        n, S = sample_t.shape
        self._f32("sample_t", sample_t)
        self._f32("rays", rays, (n, 6))
        torch = self.torch
        points = torch.empty(n * S, 3, dtype=torch.float32, device=rays.device)
        dists = torch.empty(n, S, dtype=torch.float32, device=rays.device)
        rc = self.lib.lnerf_ray_points(_ptr(rays), n, S, _ptr(sample_t), _ptr(points), _ptr(dists), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_ray_points: {last_error()}")
        return points, dists

    def ray_points_grad(self, sample_t, d_points, scale=None):
        """lnerf_ray_points_grad, the reverse of ray_points: d_rays (n, 6) = [sum_j d_p, sum_j t_j d_p]
        from d_points (n*S, 3) (StepResult.d_input of an INPUT_POINTS step); feeds pose_grad. `scale`
        is an optional float32 device scalar multiplied in."""
        if sample_t.dim() != 2:
            raise ValueError(f"sample_t is {tuple(sample_t.shape)}, expected (rays, S)")
        n, S = sample_t.shape
        self._f32("sample_t", sample_t)
        self._f32("d_points", d_points, (n * S, 3))
        if scale is not None:
            self._f32("scale", scale)
            if scale.numel() != 1:
                raise ValueError("scale must hold one value")
        out = self.torch.empty(n, 6, dtype=self.torch.float32, device=d_points.device)
        rc = self.lib.lnerf_ray_points_grad(n, S, _ptr(sample_t), _ptr(d_points), _ptr(scale), _ptr(out),
                                            self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_ray_points_grad: {last_error()}")
        return out

    def hashgrid_encode(self, grid: HashGrid, table, points, out=None):
        """lnerf_hashgrid_encode: the (R, grid.width) float32 encoding of points (R, 3) by `table`
        (grid.total_entries, F): per level the trilinear interpolation of the cell's eight corners."""
        self._f32("table", table, (grid.total_entries, grid.features))
        if points.dim() != 2:
            raise ValueError(f"points is {tuple(points.shape)}, expected (R, 3)")
        R = points.shape[0]
        self._f32("points", points, (R, 3))
        if out is None:
            out = self.torch.empty(R, grid.width, dtype=self.torch.float32, device=points.device)
        else:
            self._f32("out", out, (R, grid.width))
        rc = self.lib.lnerf_hashgrid_encode(ctypes.byref(grid.struct), _ptr(table), _ptr(points), R, _ptr(out),
                                            self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_hashgrid_encode: {last_error()}")
        return out

    def hashgrid_grad(self, grid: HashGrid, table, points, d_encoded, scale=None, accumulate: bool = False,
                      d_table=None, want_d_points: bool = False, want_d_table: bool = True,
                      reproducible: bool = False):
        """lnerf_hashgrid_grad, the reverse of hashgrid_encode: (d_table (total_entries, F), d_points
        (R, 3)) from d_encoded (R, grid.width) -- StepResult.d_x of an INPUT_ENCODED step with want_dx.
        `d_table` may be a buffer to write (accumulate=True: to add into; it is then required); an
        output that is not asked for is None. `table` may be None unless want_d_points. `scale` is an
        optional float32 device scalar multiplied in. By default d_table is summed with float32 atomics
        (its last bits vary from call to call); with reproducible=True (HASHGRID_REPRODUCIBLE) it is a
        float64 sum per entry in a fixed order, rounded once: the same bits on every call, from scratch
        the call takes from the stream's memory pool (hashgrid_grad_scratch bytes). d_points is
        bit-reproducible either way and has the same bits in both modes."""
        torch = self.torch
        if points.dim() != 2:
            raise ValueError(f"points is {tuple(points.shape)}, expected (R, 3)")
        R = points.shape[0]
        self._f32("points", points, (R, 3))
        self._f32("d_encoded", d_encoded, (R, grid.width))
        if table is not None:
            self._f32("table", table, (grid.total_entries, grid.features))
        if scale is not None:
            self._f32("scale", scale)
            if scale.numel() != 1:
                raise ValueError("scale must hold one value")
        if want_d_table:
            if d_table is None:
                if accumulate:
                    raise ValueError("accumulate=True needs the d_table to add into")
                d_table = torch.empty(grid.total_entries, grid.features, dtype=torch.float32, device=points.device)
            else:
                self._f32("d_table", d_table, (grid.total_entries, grid.features))
        else:
            d_table = None
        d_points = torch.empty(R, 3, dtype=torch.float32, device=points.device) if want_d_points else None
        flags = (ACCUMULATE if accumulate else 0) | (HASHGRID_REPRODUCIBLE if reproducible else 0)
        rc = self.lib.lnerf_hashgrid_grad(ctypes.byref(grid.struct), _ptr(table), _ptr(points), R, _ptr(d_encoded),
                                          _ptr(scale), flags, _ptr(d_table), _ptr(d_points), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_hashgrid_grad: {last_error()}")
        return d_table, d_points

    def hashgrid_grad_scratch(self, grid: HashGrid, rows: int) -> int:
        """lnerf_hashgrid_grad_scratch: the bytes a hashgrid_grad(..., reproducible=True) call on `rows`
        rows takes from the stream's memory pool while it runs."""
        n = self.lib.lnerf_hashgrid_grad_scratch(ctypes.byref(grid.struct), int(rows), self._stream())
        if n < 0:
            raise RuntimeError(f"lnerf_hashgrid_grad_scratch: {last_error()}")
        return int(n)

    def _dev(self, name, t, dtype, shape=None):
        """`t` must be a contiguous tensor of `dtype` on this engine's device (of `shape`, if given)."""
        torch = self.torch
        if not torch.is_tensor(t) or t.dtype != dtype:
            raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor")
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{name} must live on cuda:{self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} is {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def _occ_cells(self, occ, cells):
        """The length of the optional int32 cell list (None: every cell in order)."""
        if cells is None:
            return occ.num_cells
        self._dev("cells", cells, self.torch.int32)
        if cells.dim() != 1:
            raise ValueError(f"cells is {tuple(cells.shape)}, expected (n,)")
        return cells.shape[0]

    def occgrid_cell_points(self, occ: OccGrid, cells=None, u=None):
        """lnerf_occgrid_cell_points: (n, 3) float32 points inside the cells `cells` (n,) int32 (None:
        all num_cells cells in order), placed by u (n, 3) in [0, 1] (None: the cell centres). An index
        outside the grid gives the box centre."""
        n = self._occ_cells(occ, cells)
        if u is not None:
            self._f32("u", u, (n, 3))
        out = self.torch.empty(n, 3, dtype=self.torch.float32, device=f"cuda:{self.device}")
        rc = self.lib.lnerf_occgrid_cell_points(ctypes.byref(occ.struct), _ptr(cells), n, _ptr(u), _ptr(out),
                                                self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_occgrid_cell_points: {last_error()}")
        return out

    def occgrid_update(self, occ: OccGrid, density, sigma, cells=None, decay: float = 0.95, sigma_stride: int = 1):
        """lnerf_occgrid_update, in place on density (num_cells,): density *= decay, then
        density[cells[i]] = max(density[cells[i]], sigma.flatten()[i * sigma_stride]). `sigma` is any
        contiguous float32 tensor holding at least (n - 1) * sigma_stride + 1 values, e.g. an (n,)
        vector, or rgba.flatten()[3:] with sigma_stride=4. Returns density."""
        self._f32("density", density, (occ.num_cells,))
        n = self._occ_cells(occ, cells)
        self._f32("sigma", sigma)
        if sigma_stride < 1:
            raise ValueError("sigma_stride must be at least 1")
        if n and sigma.numel() < (n - 1) * int(sigma_stride) + 1:
            raise ValueError(f"sigma holds {sigma.numel()} values, {n} cells at stride {sigma_stride} "
                             f"need {(n - 1) * int(sigma_stride) + 1}")
        rc = self.lib.lnerf_occgrid_update(ctypes.byref(occ.struct), _ptr(density), _ptr(cells), n, _ptr(sigma),
                                           int(sigma_stride), float(decay), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_occgrid_update: {last_error()}")
        return density

    def occgrid_threshold(self, occ: OccGrid, density, threshold: float = 0.01, use_mean: bool = True, bits=None,
                          want=("bits", "mean", "occupied")):
        """lnerf_occgrid_threshold: (bits, mean, occupied). bits (num_cells / 32,) int32 words with bit
        c = density[c] > thr, thr = threshold or, with use_mean, min(threshold, mean(density)); mean a
        float64 and occupied an int64 device scalar (the mean of density, the number of set bits).
        `bits` may be a buffer to write; an entry `want` does not name is None."""
        torch = self.torch
        unknown = set(want) - {"bits", "mean", "occupied"}
        if unknown or not want:
            raise ValueError(f"want must name 'bits', 'mean' and / or 'occupied', got {tuple(want)}")
        self._f32("density", density, (occ.num_cells,))
        if "bits" not in want:
            bits = None
        elif bits is None:
            bits = torch.empty(occ.num_cells // 32, dtype=torch.int32, device=density.device)
        else:
            self._dev("bits", bits, torch.int32, (occ.num_cells // 32,))
        mean = torch.empty((), dtype=torch.float64, device=density.device) if "mean" in want else None
        occupied = torch.empty((), dtype=torch.int64, device=density.device) if "occupied" in want else None
        rc = self.lib.lnerf_occgrid_threshold(ctypes.byref(occ.struct), _ptr(density), float(threshold),
                                              OCC_MEAN if use_mean else 0, _ptr(bits), _ptr(mean), _ptr(occupied),
                                              self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_occgrid_threshold: {last_error()}")
        return bits, mean, occupied

    def sample_occupancy(self, occ: OccGrid, bits, rays, samples: int, steps: int = 1024, near: float = 2.0,
                         far: float = 6.0, u=None, last_opaque: bool = False, want=("t", "dists", "n_occ")):
        """lnerf_sample_occupancy: (sample_t (n, samples), dists (n, samples), n_occ (n,) int32) for rays
        (n, 6). Each ray is marched in `steps` steps over the bitfield and its samples are spread over
        the occupied steps alone, placed by u (n, samples) in [0, 1] (None: 0.5). dists is the equal
        share of the occupied length each sample stands for (last_opaque: the last one is 1e8); n_occ
        the number of occupied steps -- 0 marks a ray that met nothing, sampled over [near, far] as a
        whole. An entry `want` does not name is None."""
        torch = self.torch
        unknown = set(want) - {"t", "dists", "n_occ"}
        if unknown or not want:
            raise ValueError(f"want must name 't', 'dists' and / or 'n_occ', got {tuple(want)}")
        self._dev("bits", bits, torch.int32, (occ.num_cells // 32,))
        if rays.dim() != 2:
            raise ValueError(f"rays is {tuple(rays.shape)}, expected (n, 6)")
        n, S = rays.shape[0], int(samples)
        self._f32("rays", rays, (n, 6))
        if u is not None:
            self._f32("u", u, (n, S))
        t = torch.empty(n, max(S, 0), dtype=torch.float32, device=rays.device) if "t" in want else None
        dists = torch.empty(n, max(S, 0), dtype=torch.float32, device=rays.device) if "dists" in want else None
        n_occ = torch.empty(n, dtype=torch.int32, device=rays.device) if "n_occ" in want else None
        rc = self.lib.lnerf_sample_occupancy(ctypes.byref(occ.struct), _ptr(bits), _ptr(rays), n, S, int(steps),
                                             float(near), float(far), _ptr(u), OCC_LAST_OPAQUE if last_opaque else 0,
                                             _ptr(t), _ptr(dists), _ptr(n_occ), self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_sample_occupancy: {last_error()}")
        return t, dists, n_occ

    def timings(self):
        """Per-kernel ms of the last TIMING step: pack, fused, loss, dw, reduce, total."""
        out = (ctypes.c_float * 6)()
        n = self.lib.lnerf_ctx_timings(self.ctx, out, 6)
        if n < 0:
            raise RuntimeError(f"lnerf_ctx_timings: {last_error()}")
        keys = ("pack", "fused", "loss", "dw", "reduce", "total")
        return {keys[i]: out[i] for i in range(n)}

    def exceptional_rows(self, split=False):
        """Rows (summed over layers) the last fp16x3 training step multiplied on the bf16x6 split
        (lnerf_ctx_exceptional_rows; synchronises); split=True: (rows, of them rays' last samples)."""
        n, t = ctypes.c_longlong(0), ctypes.c_longlong(0)
        if self.lib.lnerf_ctx_exceptional_rows(self.ctx, ctypes.byref(n), ctypes.byref(t)) != 0:
            raise RuntimeError(f"lnerf_ctx_exceptional_rows: {last_error()}")
        return (int(n.value), int(t.value)) if split else int(n.value)

    def guard_fired(self):
        """The last training step's fp16x3 floor guard (lnerf_ctx_guard_fired; synchronises): 1 if k1
        found a hidden G element below fp16x3's floor and the step re-ran on the bf16x6 split, 0 if
        not, -1 if the step had no guard (an explicit precision flag, the generic path, ...)."""
        f = ctypes.c_int(0)
        if self.lib.lnerf_ctx_guard_fired(self.ctx, ctypes.byref(f)) != 0:
            raise RuntimeError(f"lnerf_ctx_guard_fired: {last_error()}")
        return int(f.value)

    def workspace_used(self) -> int:
        """Bytes of the workspace the last fused step / render laid out (lnerf_ctx_workspace_used)."""
        return int(self.lib.lnerf_ctx_workspace_used(self.ctx))

    def workspace_bytes(self, mlp: LnerfMLP, rays: int, samples: int) -> int:
        """lnerf_workspace_bytes: what a default-grid training step of this shape needs."""
        return int(self.lib.lnerf_workspace_bytes(ctypes.byref(mlp), rays, samples))

    def last_path(self) -> dict:
        """The kernels the last train_step/render ran (lnerf_ctx_last_path)."""
        v = self.lib.lnerf_ctx_last_path(self.ctx)
        if v < 0:
            raise RuntimeError(f"lnerf_ctx_last_path: {last_error()}")
        d = dict(generic=bool(v & PATH_GENERIC), fused=bool(v & PATH_FUSED),
                 k16=bool(v & PATH_K16), dw16=bool(v & PATH_DW16), k16_w4=bool(v & PATH_K16_W4),
                 kr=bool(v & PATH_KR), a24=bool(v & PATH_A24),
                 planes=(v >> 8) & 3)
        if v & PATH_MAPS:   # only after render_maps: the kernels' bits as after render, plus this key
            d["maps"] = True
        if v & PATH_VJP:    # only after render_maps_vjp: the training step's bits, plus this key
            d["vjp"] = True
        return d

    def relu_masks(self, L: int, R: int):
        """The last training step's hidden ReLU decisions (k16 path): numpy bool (L-1, R, 256),
        [l, r, f] = feature f of hidden layer l at sample row r was positive."""
        import numpy as np
        torch = self.torch
        out = torch.empty((L - 1) * R * 32, dtype=torch.uint8, device=f"cuda:{self.device}")
        rc = self.lib.lnerf_ctx_relu_masks(self.ctx, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                           self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_ctx_relu_masks: {last_error()}")
        bits = out.cpu().numpy().reshape(L - 1, R, 32)
        return np.unpackbits(bits, axis=2, bitorder="little").astype(bool)

    def set_option(self, option: int, value: int):
        """lnerf_ctx_set_option (OPT_DW_GRID: the dW kernel's workgroup budget, 0 = default)."""
        if self.lib.lnerf_ctx_set_option(self.ctx, option, value) != 0:
            raise RuntimeError(f"lnerf_ctx_set_option: {last_error()}")

    def scale_by_device_scalar(self, buf, scale):
        rc = self.lib.lnerf_scale_by_device_scalar(ctypes.c_void_p(buf.data_ptr()), buf.numel(),
                                                   ctypes.c_void_p(scale.data_ptr()),
                                                   self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_scale_by_device_scalar: {last_error()}")

    def adam_update(self, params, grads, m, v, t: int, lr: float, beta1=0.9, beta2=0.999,
                    eps=1e-8):
        rc = self.lib.lnerf_adam_update(params.data_ptr(), grads.data_ptr(), m.data_ptr(),
                                        v.data_ptr(), params.numel(), t, lr, beta1, beta2, eps,
                                        self._stream())
        if rc != 0:
            raise RuntimeError(f"lnerf_adam_update: {last_error()}")


_AUTOGRAD_FN = None


def _autograd_fn():
    """The torch.autograd.Function behind render_maps_autograd (built on first use: torch is optional
    for the ctypes surface)."""
    global _AUTOGRAD_FN
    if _AUTOGRAD_FN is not None:
        return _AUTOGRAD_FN
    import torch

    class RenderMapsFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, engine, mlp, cfg, ws, bs, x, dists, sample_t):
            want = cfg["want"]
            maps = engine.render_maps(mlp, ws, bs, x, dists, None, samples=cfg["samples"],
                                      input_mode=cfg["input_mode"], num_freqs=cfg["num_freqs"],
                                      near=cfg["near"], far=cfg["far"], sample_t=sample_t, flags=cfg["flags"],
                                      want=tuple(want) + (("weights",) if cfg["t_grad"] and "weights" not in want
                                                          else ()))
            ctx.engine, ctx.mlp, ctx.cfg = engine, mlp, cfg
            ctx.set_materialize_grads(False)   # a map the loss never used arrives as None: a NULL adjoint
            ctx.save_for_backward(ws, bs, x, dists, sample_t, maps.weights if cfg["t_grad"] else None)
            outs = tuple(getattr(maps, name) for name in want)
            ctx.mark_non_differentiable(*[o for o, name in zip(outs, want) if name not in ADJOINT_NAMES])
            return outs

        @staticmethod
        def backward(ctx, *gouts):
            ws, bs, x, dists, sample_t, weights = ctx.saved_tensors
            cfg, want = ctx.cfg, ctx.cfg["want"]
            adj = {name: g.contiguous().float() for name, g in zip(want, gouts)
                   if g is not None and name in ADJOINT_NAMES}
            need_x = ctx.needs_input_grad[5]
            need_dists = dists is not None and ctx.needs_input_grad[6]
            r = ctx.engine.render_maps_vjp(ctx.mlp, ws, bs, x, dists, adj, samples=cfg["samples"],
                                           input_mode=cfg["input_mode"], num_freqs=cfg["num_freqs"],
                                           near=cfg["near"], far=cfg["far"], sample_t=sample_t,
                                           flags=cfg["flags"], want_dists=need_dists, want_dinput=need_x)
            d_t = None
            if sample_t is not None and ctx.needs_input_grad[7] and "depth" in adj:
                d_t = weights * adj["depth"][:, None]
            return (None, None, None, r.d_ws.view_as(ws) if ctx.needs_input_grad[3] else None,
                    r.d_bs.view_as(bs) if ctx.needs_input_grad[4] else None,
                    r.d_input.view_as(x) if need_x else None, r.d_dists.view_as(dists) if need_dists else None, d_t)

    _AUTOGRAD_FN = RenderMapsFn
    return RenderMapsFn


def render_maps_autograd(engine: Engine, mlp: LnerfMLP, ws, bs, x, dists, *, samples: int,
                         input_mode: int = INPUT_POINTS, num_freqs: int = 5, sample_t=None,
                         near: float = 2.0, far: float = 6.0, flags: int = 0,
                         want=("color", "depth", "opacity", "weights")):
    """The render maps as differentiable torch tensors: a torch.autograd.Function whose forward is
    Engine.render_maps and whose backward is ONE Engine.render_maps_vjp call fed the gradients autograd
    hands back for the maps. Returns the maps `want` names (ADJOINT_NAMES), in that order. Gradients
    reach ws, bs, dists, x (through WANT_DINPUT, only if x requires grad) and sample_t
    (weights * d_depth[:, None]); a map that is not asked for, or receives no gradient, contributes
    nothing. Any torch loss on the maps can be trained this way, e.g.

        color, depth, opacity = render_maps_autograd(eng, mlp, ws, bs, rays, None, samples=64,
                                                     input_mode=INPUT_RAYS, want=("color", "depth", "opacity"))
        loss = ((color + (1 - opacity)[:, None] * 1.0 - target) ** 2).sum() + 0.1 * (depth - d_gt).abs().sum()
        loss.backward()      # ws.grad, bs.grad
    """
    unknown = set(want) - set(ADJOINT_NAMES)
    if unknown or not want:
        raise ValueError(f"want must name maps of {ADJOINT_NAMES}, got {tuple(want)}")
    t_grad = sample_t is not None and bool(getattr(sample_t, "requires_grad", False)) and "depth" in want
    cfg = dict(samples=samples, input_mode=input_mode, num_freqs=num_freqs, near=near, far=far, flags=flags,
               want=tuple(want), t_grad=t_grad)
    outs = _autograd_fn().apply(engine, mlp, cfg, ws, bs, x, dists, sample_t)
    return outs


_HASHGRID_FN = None


def _hashgrid_fn():
    """The torch.autograd.Function behind hashgrid_autograd (built on first use, as _autograd_fn)."""
    global _HASHGRID_FN
    if _HASHGRID_FN is not None:
        return _HASHGRID_FN
    import torch

    class HashGridFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, engine, grid, table, points, reproducible):
            ctx.engine, ctx.grid, ctx.reproducible = engine, grid, bool(reproducible)
            ctx.save_for_backward(table, points)
            return engine.hashgrid_encode(grid, table, points)

        @staticmethod
        def backward(ctx, g):
            table, points = ctx.saved_tensors
            need_t, need_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
            if not (need_t or need_p):
                return None, None, None, None, None
            d_table, d_points = ctx.engine.hashgrid_grad(ctx.grid, table, points, g.contiguous().float(),
                                                         want_d_table=need_t, want_d_points=need_p,
                                                         reproducible=ctx.reproducible)
            return None, None, d_table, d_points, None

    _HASHGRID_FN = HashGridFn
    return HashGridFn


def hashgrid_autograd(engine: Engine, grid: HashGrid, table, points, reproducible: bool = False):
    """The hash-grid encoding as a differentiable torch tensor: a torch.autograd.Function whose forward
    is Engine.hashgrid_encode and whose backward is ONE Engine.hashgrid_grad call. Gradients reach
    `table` and, if it requires grad, `points`; reproducible=True makes the table gradient the ordered
    float64 sum of HASHGRID_REPRODUCIBLE (the same bits on every backward). Feed the result to a torch MLP, or to
    render_maps_autograd(..., input_mode=INPUT_ENCODED) to train the grid under any loss on the maps:

        x = hashgrid_autograd(eng, grid, table, points)
        color, = render_maps_autograd(eng, mlp, ws, bs, x, dists, samples=S, input_mode=INPUT_ENCODED,
                                      want=("color",))
        ((color - target) ** 2).sum().backward()      # table.grad, ws.grad, bs.grad
    """
    return _hashgrid_fn().apply(engine, grid, table, points, reproducible)
