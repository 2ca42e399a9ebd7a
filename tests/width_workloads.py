"""Workloads that move the quantities the fused kernels branch on: the first layer's width k[0]
(k16's two POINTS / RAYS encoders split at 64, kr takes k[0] <= 64 only, the d_x store and the
layer-0 slabs follow k[0]), the number of encoding frequencies F (k[0] = 3 + 6 F) and the head width
(4..16 outputs in one 16-wide tile, of which only columns 0..3 are seeded by the reverse pass).

All of them are 24 rays x 32 samples (768 rows: six 128-sample tiles, several workgroups) under a
k[0] -> 30 -> 30 -> n MLP. Only oracle/ and numpy are used; tests/test_width_workloads.py holds the
conditions these inputs must meet before a GPU parity test on them means anything (live gradients,
semi-transparent rays, every probed feature visible in the outputs, the two references agreeing).

  * freq_workload(F)     nerf_np.make_workload("cfg2", rays=24, samples=32, num_functions=F) and the
                         float32 rays behind its points (make_workload's own selection, as
                         test_gpu_render_maps._cfg2 rebuilds them), so RAYS and POINTS see one scene;
  * encoded_workload(k0) ENCODED input of width k0, the recipe of test_gpu_contract._sweep_workload:
                         He-scaled weights, hidden biases uniform in [0.1, 0.6], a small positive
                         sigma column, X uniform in [-1, 1], dists 4 / (S - 1) with 1e8 last.
                         (N(0, 0.5) biases left whole batches dead at k0 = 64 and 256: sigma 0
                         everywhere, every gradient exactly 0, a parity test passing vacuously.)
  * head_workload(n)     33 -> 30 -> 30 -> n by the same recipe, head columns 4..n-1 (weights and
                         biases) multiplied by 8 so that a leak from them would be loud; it carries
                         the cfg2 points too, so both ENCODED (its X) and POINTS (its points) run.
"""
from __future__ import annotations

import functools

import numpy as np

import nerf_np
from fused_parity import rays_reference

RAYS, SAMPLES = 24, 32
FREQS = (0, 1, 10, 11, 20)                  # k0 = 3, 9, 63, 69, 123
ENCODED_K0 = (1, 15, 16, 17, 64, 65, 256)
HEADS = (5, 16)
HEAD_GAIN = 8.0
# features whose loss must show: both sides of every 16-wide tile edge up to 64, and the last one
PROBED = (0, 2, 15, 16, 31, 32, 47, 48, 62, 63, 64, 65)

# weight / input seeds of the synthetic workloads, chosen on the CPU so that the float64 reference
# alone meets the conditions of tests/test_width_workloads.py
ENCODED_SEEDS = {1: 1, 15: 1, 16: 1, 17: 1, 64: 1, 65: 1, 256: 4}
HEAD_SEEDS = {5: 1, 16: 1}


def probed_features(k0):
    return sorted({f for f in PROBED + (k0 - 1,) if 0 <= f < k0})


def select_rays32(N, side=100):
    """The float32 rays [o, d] behind make_workload("cfg2", rays=N)'s points."""
    focal = 0.5 / np.tan(0.5 * 0.6911112)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]]).astype(np.float32)
    o, d = nerf_np.get_rays(side, side, K, nerf_np.look_at_pose())
    sel = np.random.RandomState(0).choice(o.shape[0], size=N, replace=N > o.shape[0])
    return np.concatenate([o[sel], d[sel]], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def freq_workload(F, rays=RAYS, samples=SAMPLES):
    w = nerf_np.make_workload("cfg2", rays=rays, samples=samples, num_functions=F)
    return w, select_rays32(rays)


def _recipe(dims, N, S, seed):
    rng = np.random.RandomState(seed)
    ws = [(rng.randn(k, n) * np.sqrt(2.0 / k)).astype(np.float32) for k, n in zip(dims, dims[1:])]
    bs = [rng.uniform(0.1, 0.6, n).astype(np.float32) for n in dims[1:]]
    ws[-1][:, 3] = np.abs(ws[-1][:, 3]) * 0.05   # sigma > 0 and moderate: every sample contributes
    ws[-1][:, 4:] *= np.float32(HEAD_GAIN)
    bs[-1][4:] *= np.float32(HEAD_GAIN)
    X = rng.uniform(-1, 1, (N * S, dims[0])).astype(np.float32)
    dists = np.full((N, S), 4.0 / max(S - 1, 1), np.float32)
    dists[:, -1] = 1e8
    target = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    return ws, bs, X, dists, target


@functools.lru_cache(maxsize=None)
def encoded_workload(k0, seed=None, rays=RAYS, samples=SAMPLES):
    seed = ENCODED_SEEDS[k0] if seed is None else seed
    ws, bs, X, dists, target = _recipe([k0, 30, 30, 4], rays, samples, seed)
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(None, None, X, dists, target, ws, bs, wp, bp, 0, samples, rays)


@functools.lru_cache(maxsize=None)
def head_workload(n, seed=None, rays=RAYS, samples=SAMPLES):
    seed = HEAD_SEEDS[n] if seed is None else seed
    ws, bs, X, dists, target = _recipe([33, 30, 30, n], rays, samples, seed)
    wp, bp = nerf_np.pad_weights(ws, bs)
    c = nerf_np.make_workload("cfg2", rays=rays, samples=samples)
    return nerf_np.Workload(c.pts, c.pts32, X, dists, target, ws, bs, wp, bp, c.F, samples, rays)


def narrow_head(w):
    """The workload with its head cut to columns 0..3 (what a wide head must compute)."""
    ws = list(w.ws[:-1]) + [np.ascontiguousarray(w.ws[-1][:, :4])]
    bs = list(w.bs[:-1]) + [np.ascontiguousarray(w.bs[-1][:4])]
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)


def scale_wide_head(w, gain):
    """The workload with head columns 4.. (weights and biases) multiplied by gain."""
    ws = [x.copy() for x in w.ws]
    bs = [x.copy() for x in w.bs]
    ws[-1][:, 4:] *= np.float32(gain)
    bs[-1][4:] *= np.float32(gain)
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)


def points_input(w):
    """The float32-rounded encoding POINTS input computes from w's float32 points (the C oracle's
    float64 positional_encoding_3d, as fused_parity.encoded_input)."""
    import oracle
    return oracle.positional_encoding_3d(w.pts32.astype(np.float64), w.F)


CASES = [("freq", F, mode) for F in FREQS for mode in ("points", "rays")] + \
        [("encoded", k0, "encoded") for k0 in ENCODED_K0] + \
        [("head", n, mode) for n in HEADS for mode in ("encoded", "points")]


def case_id(case):
    kind, v, mode = case
    return f"{dict(freq='F', encoded='k0_', head='head')[kind]}{v}-{mode}"


def case_workload(case):
    """(workload, rays32 or None, X, dists) of a case: X (rows, k0) float32 and dists are what the
    device computes or is handed in that input mode, the float64 reference's input."""
    kind, v, mode = case
    if kind == "freq":
        w, rays32 = freq_workload(v)
    else:
        w, rays32 = (encoded_workload(v) if kind == "encoded" else head_workload(v)), None
    if mode == "rays":
        X, dists = rays_reference(rays32, w.S, w.F)
        return w, rays32, X, dists
    X = points_input(w) if mode == "points" else w.X
    return w, None, X, w.dists


def violation(got, want, rtol, atol_scale):
    """max |got - want| / (rtol |want| + atol_scale max|want|): loma_calls.assert_close's form; above 1
    it raises."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(np.abs(want).max(initial=0.0), 1e-30)
    return float((np.abs(got - want) / (rtol * np.abs(want) + atol_scale * scale)).max())
