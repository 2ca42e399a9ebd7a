"""Float64 compositing for the render maps (lnerf_render_maps): from per-sample (rgb, sigma, dists, t)
to (weights, colour, depth, opacity), and the error bars the GPU tests hold the fp32 maps to.

The weights are the reference's own (scripts/nerf.py:200-272): alpha_j = 1 - exp(-sigma_j delta_j),
c_j = (1 - alpha_j) + 1e-10, P_j = prod_{i<=j} c_i, T_0 = 1 and T_j = P_j for j >= 1 (the INCLUSIVE
transmittance), w_j = alpha_j T_j. colour = sum_j w_j rgb_j (nerf.py:281-288); depth = sum_j w_j t_j
and opacity = sum_j w_j are the engine's extension (the reference never forms them).
tests/test_render_maps_ref.py checks this file against oracle/nerf_np.py before it judges the GPU.
"""
import numpy as np

U = 2.0 ** -23   # fp32 unit roundoff (one ulp of 1)


def composite64(rgb, sigma, dists, t=None):
    """rgb (N, S, 3), sigma (N, S), dists (N, S), t (N, S) or None -> dict of float64 arrays:
    weights (N, S), color (N, 3), depth (N) (None without t), opacity (N)."""
    rgb = np.asarray(rgb, np.float64)
    sigma = np.asarray(sigma, np.float64)
    dists = np.asarray(dists, np.float64)
    alpha = 1.0 - np.exp(-sigma * dists)
    c = (1.0 - alpha) + 1e-10
    T = np.cumprod(c, axis=1)
    T[:, 0] = 1.0
    w = alpha * T
    out = dict(weights=w, color=(w[:, :, None] * rgb).sum(1), opacity=w.sum(1), depth=None)
    if t is not None:
        out["depth"] = (w * np.asarray(t, np.float64)).sum(1)
    return out


def weights_bar(w64, S):
    """|w - w64| <= 2^-22 (1 + (S + 1) w64): P_j is a product of at most S factors, each carrying at
    most 4 fp32 roundings (expf, the subtraction, + 1e-10, the multiply); alpha's own absolute error
    is <= 2^-23."""
    return 2.0 ** -22 * (1.0 + (S + 1) * np.asarray(w64, np.float64))


def sums_from_weights(weights, rgb, t=None):
    """Float64 sums of the RETURNED fp32 weights times 1 / t / rgb, with each sum's fp32 summation bar
    S 2^-23 sum_j |term_j| + 2^-23 |sum| (any summation order of S fp32 terms, plus the rounding of the
    terms themselves). Returns {name: (sum, bar)} for opacity, color (N, 3) and, with t, depth."""
    w = np.asarray(weights, np.float64)
    S = w.shape[1]

    def one(terms):
        s = terms.sum(1)
        return s, S * U * np.abs(terms).sum(1) + U * np.abs(s)

    out = dict(opacity=one(w), color=one(w[:, :, None] * np.asarray(rgb, np.float64)))
    if t is not None:
        out["depth"] = one(w * np.asarray(t, np.float64))
    return out


def ray_t(S, near=2.0, far=6.0):
    """The depths RAYS mode samples at, as the engine rounds them: (float)linspace(near, far, S)."""
    return np.linspace(np.float32(near).astype(np.float64), np.float32(far).astype(np.float64), S).astype(np.float32)


def map_ratios(out, dists, t, S):
    """Per ray, the error of the maps in `out` (weights (N, S), opacity, depth (N), color (N, 3), rgba (N S, 4))
    over the bars above, against float64 from the RETURNED rgba: what test_gpu_render_maps.compositing_ratios
    asserts on the worst ray, kept per ray so that a sweep can report which rays fail. A sum of exact zeros
    (a sigma = 0 ray) has a zero bar and must be exactly zero (inf otherwise)."""
    N = np.asarray(dists).shape[0]
    rgba = np.asarray(out["rgba"]).reshape(N, S, 4).astype(np.float64)
    w64 = composite64(rgba[:, :, :3], rgba[:, :, 3], dists, t)
    werr = np.abs(np.asarray(out["weights"], np.float64) - w64["weights"])
    ratios = dict(weights=(werr / weights_bar(w64["weights"], S)).max(axis=1))
    sums = sums_from_weights(out["weights"], rgba[:, :, :3], t)
    for k in ("opacity", "depth", "color"):
        s, bar = sums[k]
        err = np.abs(np.asarray(out[k], np.float64) - s)
        r = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
        ratios[k] = r.reshape(N, -1).max(axis=1)
    return ratios
