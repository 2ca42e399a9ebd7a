"""Workloads that move the magnitude the fused kernels' shift machinery responds to (the per-layer
weight shift, the head's per-column shift, k1's per-sample row shifts and their signed bytes in the
slab word, the int24 activation slabs, dw16's per-layer product shift, the floor guard and the shift
clamp), by the one transformation a ReLU MLP is exactly equivariant under.

For powers of two g_l, one per hidden layer (g_{-1} = g_{L-1} = 1),

    W_l <- W_l g_l / g_{l-1}        b_l <- b_l g_l

scales the hidden activations A_{l+1} by g_l and their gradients G_l by 1 / g_l, leaves the head
output, the loss, the colours, d_dists, d_target, dX and every ReLU decision unchanged, and scales
dW_l by fW[l] = g_{l-1} / g_l and db_l by fB[l] = 1 / g_l. A power of two commutes with fp32 rounding
while nothing leaves the normal range, so an implementation whose every scale is a power of two
built from the operands' own exponents computes the same floats in both runs.

Only oracle/ and numpy are used; tests/test_scale_workloads.py holds the conditions these inputs
must meet (exact rescale, equivariant references, every intermediate inside fp32's normal range,
live gradients, layers at different scales) before the GPU tests of tests/test_gpu_scale.py mean
anything.
"""
from __future__ import annotations

import functools

import numpy as np

import nerf_np
import width_workloads as ww

# log2 g_l per hidden layer l = 0 .. H - 1
PATTERNS = {
    "up24": lambda H: [24] * H,
    "down24": lambda H: [-24] * H,
    "alt40": lambda H: [40 if l % 2 == 0 else -40 for l in range(H)],
    "ramp8": lambda H: [min(8 * (l + 1), 40) for l in range(H)],
    "one_up40": lambda H: [40 if l == H // 2 else 0 for l in range(H)],
    "one_down40": lambda H: [-40 if l == H // 2 else 0 for l in range(H)],
}
SPREAD_PATTERNS = ("up24", "down24", "alt40")   # the rescaled layers' max|dW| span >= 2^40
WORKLOADS = ("a", "b", "c", "d", "e")
# cfg3 under alt40 leaves the range every float32 intermediate must stay in (|G| down to 2^-139)
EXCLUDED = {("e", "alt40")}
PAIRS = [(n, p) for n in WORKLOADS for p in PATTERNS if (n, p) not in EXCLUDED]
RAYS_WORKLOADS = ("b", "d")          # these also run INPUT_RAYS on the rays behind their points
RANGE_LOG2 = 100                     # every nonzero |A|, |G|, |dW|, |db| lies in [2^-100, 2^100]
# weight / input seed of (b), chosen on the CPU so that the float64 reference alone meets the range
# condition in every pattern and input mode: on the cfg2 points seeds 1, 3 and 4 reach 2^-126,
# 2^-121 and 2^-121 under alt40 (2^-97 on their own ENCODED X); seed 2 stays within [2^-96.1, 2^83.1]
WIDE_SEED = 2


@functools.lru_cache(maxsize=None)
def wide_workload(seed=WIDE_SEED, rays=ww.RAYS, samples=ww.SAMPLES):
    """33 -> 64 -> 64 -> 64 -> 64 -> 4 by width_workloads' recipe, with the cfg2 points as
    head_workload carries them: ENCODED runs on its X, POINTS and RAYS on the points."""
    ws, bs, X, dists, target = ww._recipe([33, 64, 64, 64, 64, 4], rays, samples, seed)
    wp, bp = nerf_np.pad_weights(ws, bs)
    c = nerf_np.make_workload("cfg2", rays=rays, samples=samples)
    return nerf_np.Workload(c.pts, c.pts32, X, dists, target, ws, bs, wp, bp, c.F, samples, rays)


@functools.lru_cache(maxsize=None)
def base(name):
    """(workload, input mode of its plain run): (a) ENCODED, so dX is checked; the others POINTS."""
    if name == "a":
        return ww.encoded_workload(64), "encoded"
    if name == "b":
        return wide_workload(), "points"
    if name == "c":
        return ww.head_workload(16), "points"
    if name == "d":
        return nerf_np.make_workload("cfg2", rays=24, samples=32), "points"
    if name == "e":
        return nerf_np.make_workload("cfg3", rays=6, samples=32), "points"
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def head20_workload():
    """(d) under a 20-output head (test_gpu_native.test_wide_head_runs_generic_or_fails' recipe): a
    shape only the generic path takes."""
    w = base("d")[0]
    rng = np.random.RandomState(11)
    ws = list(w.ws[:-1]) + [(rng.randn(w.ws[-1].shape[0], 20) * 0.1).astype(np.float32)]
    bs = list(w.bs[:-1]) + [(rng.randn(20) * 0.1).astype(np.float32)]
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)


def rays32(w):
    """The float32 rays [o, d] behind the cfg2 points of w."""
    return ww.select_rays32(w.N)


def log2_gains(pattern, L):
    return [int(v) for v in PATTERNS[pattern](L - 1)]


def factors(log2_g, L):
    """(log2 fW, log2 fB) per layer of an L-layer MLP under hidden gains 2^log2_g."""
    assert len(log2_g) == L - 1
    g = list(log2_g) + [0]
    prev = [0] + g[:-1]
    return [p - q for p, q in zip(prev, g)], [-q for q in g]


def rescale(w, log2_g):
    """(workload with W_l g_l / g_{l-1} and b_l g_l, fW, fB): the products are formed in float64 and
    cast to float32 (exact while nothing leaves the normal range); fW[l] = g_{l-1} / g_l and
    fB[l] = 1 / g_l, float64 powers of two, are what dW_l and db_l are multiplied by."""
    L = len(w.ws)
    lw, lb = factors(log2_g, L)
    ws = [(x.astype(np.float64) * 2.0 ** -e).astype(np.float32) for x, e in zip(w.ws, lw)]
    bs = [(x.astype(np.float64) * 2.0 ** -e).astype(np.float32) for x, e in zip(w.bs, lb)]
    wp, bp = nerf_np.pad_weights(ws, bs)
    if wp.shape != w.wp.shape:          # a caller's wider padding is kept
        wp2, bp2 = np.zeros_like(w.wp), np.zeros_like(w.bp)
        wp2[:, :wp.shape[1], :wp.shape[2]] = wp
        bp2[:, :bp.shape[1]] = bp
        wp, bp = wp2, bp2
    out = nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)
    return out, [2.0 ** e for e in lw], [2.0 ** e for e in lb]


def rescale_padded(wp, bp, shapes, log2_g):
    """rescale for padded (L, K, N) / (L, N) float32 weights alone (the mlp_fit workloads):
    (wp, bp, log2 fW, log2 fB)."""
    lw, lb = factors(log2_g, len(shapes))
    wq = np.stack([np.ldexp(wp[l], -lw[l]) for l in range(len(shapes))]).astype(np.float32)
    bq = np.stack([np.ldexp(bp[l], -lb[l]) for l in range(len(shapes))]).astype(np.float32)
    return wq, bq, lw, lb


@functools.lru_cache(maxsize=None)
def scaled(name, pattern):
    """(rescaled workload, log2 fW, log2 fB) of a (workload, pattern) pair; pattern None: unscaled."""
    w = base(name)[0]
    L = len(w.ws)
    if pattern is None:
        return w, [0] * L, [0] * L
    g = log2_gains(pattern, L)
    return (rescale(w, g)[0],) + factors(g, L)


def unscale(a, log2_f):
    """a[l] / f[l] per layer of a padded float32 array, exactly (np.ldexp on float32)."""
    a = np.asarray(a)
    assert a.dtype == np.float32
    return np.stack([np.ldexp(a[l], -int(e)) for l, e in enumerate(log2_f)])


def inputs(w, mode):
    """(X, dists, rays32 or None): the float32 encoding and dists the device computes or is handed."""
    from fused_parity import rays_reference
    if mode == "rays":
        r = rays32(w)
        X, dists = rays_reference(r, w.S, w.F)
        return X, dists, r
    return (ww.points_input(w) if mode == "points" else w.X), w.dists, None


# ---- the per-layer bars -------------------------------------------------------------------------

def dw_col_over_bar(got, want, shapes):
    """Per layer, the worst |got - want| / (1e-5 |want| + 1e-4 x the column's own max |want|) over
    the layer's (k, n) block: the project's plain per-column dW bar (README "Precision")."""
    out = []
    for l, (k, n) in enumerate(shapes):
        w = np.asarray(want[l], np.float64)[:k, :n]
        err = np.abs(np.asarray(got[l], np.float64)[:k, :n] - w)
        lim = 1e-5 * np.abs(w) + 1e-4 * np.abs(w).max(axis=0, keepdims=True)
        out.append(float(np.where(err > 0, err / np.maximum(lim, 1e-300), 0.0).max()))
    return out


def db_layer_over_bar(got, want, shapes):
    """Per layer, the worst |got - want| / (1e-5 |want| + 1e-4 x the layer's own max |want|)."""
    out = []
    for l, (_, n) in enumerate(shapes):
        w = np.asarray(want[l], np.float64)[:n]
        err = np.abs(np.asarray(got[l], np.float64)[:n] - w)
        lim = 1e-5 * np.abs(w) + 1e-4 * np.abs(w).max()
        out.append(float(np.where(err > 0, err / np.maximum(lim, 1e-300), 0.0).max()))
    return out


def assert_per_layer(got_dW, got_dB, want_dW, want_dB, shapes):
    """dW per layer and per column, dB per layer, against per-layer lists or padded arrays; returns
    the worst (dW, dB) ratios."""
    rw = dw_col_over_bar(got_dW, want_dW, shapes)
    rb = db_layer_over_bar(got_dB, want_dB, shapes)
    assert max(rw) <= 1.0, f"dW error over the per-column bar, per layer: {np.round(rw, 3).tolist()}"
    assert max(rb) <= 1.0, f"dB error over the per-layer bar, per layer: {np.round(rb, 3).tolist()}"
    return max(rw), max(rb)
