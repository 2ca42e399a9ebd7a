"""TEST INFRASTRUCTURE ONLY -- float64 numpy restatement of the per-ray sampling entry points of
include/lnerf.h (lnerf_sample_stratified, lnerf_sample_importance, lnerf_ray_points,
lnerf_ray_points_grad), written from their definitions and independent of the HIP code.
tests/test_sampling_ref.py checks this file against itself and against scene.make_batch before
tests/test_gpu_sampling.py judges the GPU with it.
"""
from __future__ import annotations

import numpy as np


def _f32_as_64(v):
    """A float argument as the C ABI receives it: rounded to float32, then widened."""
    return np.float64(np.float32(v))


def linspace64(S: int, near=2.0, far=6.0) -> np.ndarray:
    """The engine's linspace in float64 (lnerf_internal.h ray_depth): j ((far - near) / (S - 1)) + near,
    the last one exactly far; S == 1 gives near."""
    near, far = _f32_as_64(near), _f32_as_64(far)
    if S <= 1:
        return np.array([near])
    g = np.arange(S, dtype=np.float64) * ((far - near) / np.float64(S - 1)) + near
    g[-1] = far
    return g


def clamp_unit(u) -> np.ndarray:
    """u clamped to [0, 1], a NaN taken as 0; float64."""
    u = np.asarray(u, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(u > 0, np.where(u < 1, u, 1.0), 0.0)


def stratified_cells(S: int, near=2.0, far=6.0):
    """(lower, upper), the float64 cell edges of the linspace: midpoints between neighbours, the ends
    the first and last depth themselves."""
    g = linspace64(S, near, far)
    mid = 0.5 * (g[:-1] + g[1:])
    return np.concatenate([g[:1], mid]), np.concatenate([mid, g[-1:]])


def stratified(u, near=2.0, far=6.0) -> np.ndarray:
    """u (rays, S) -> float32 (rays, S): t_j = lower_j + (upper_j - lower_j) clamp(u_j)."""
    u = np.asarray(u)
    lower, upper = stratified_cells(u.shape[1], near, far)
    return (lower[None, :] + (upper - lower)[None, :] * clamp_unit(u)).astype(np.float32)


def linspace32(rays: int, S: int, near=2.0, far=6.0) -> np.ndarray:
    """What a NULL t_coarse stands for: (float)linspace, one row per ray."""
    return np.tile(linspace64(S, near, far).astype(np.float32), (rays, 1))


def importance(weights, n_fine: int, t_coarse=None, u=None, near=2.0, far=6.0) -> dict:
    """weights (rays, S), t_coarse (rays, S) float32 or None, u (rays, n_fine) or None -> dict of
    float64 arrays:
      z       (rays, n_fine)  the fine depths, NOT rounded to float32
      bin     (rays, n_fine)  the bin each u fell in (int)
      slope   (rays, n_fine)  (m_{i+1} - m_i) / (cdf_{i+1} - cdf_i) of that bin
      slopes  (rays, S - 2)   the same for every bin
      m       (rays, S - 1)   the bin edges, cdf (rays, S - 1) the cdf at them, u (rays, n_fine) clamped
    """
    w = np.asarray(weights, np.float32)
    rays, S = w.shape
    assert S >= 3 and n_fine >= 1
    tc = linspace32(rays, S, near, far) if t_coarse is None else np.asarray(t_coarse, np.float32)
    tc = tc.astype(np.float64)
    m = 0.5 * (tc[:, :-1] + tc[:, 1:])
    wi = w[:, 1:-1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        wi = np.where(np.isfinite(wi) & (wi > 0), wi, 0.0)
    csum = np.cumsum(wi + 1e-5, axis=1)
    cdf = np.concatenate([np.zeros((rays, 1)), csum / csum[:, -1:]], axis=1)
    cdf[:, -1] = 1.0
    if u is None:
        uh = np.tile((np.arange(n_fine, dtype=np.float64) + 0.5) / np.float64(n_fine), (rays, 1))
    else:
        uh = clamp_unit(np.asarray(u, np.float32))
    b = np.empty((rays, n_fine), np.int64)
    for r in range(rays):
        b[r] = np.searchsorted(cdf[r], uh[r], side="right") - 1     # the largest i with cdf_i <= u
    b = np.clip(b, 0, S - 3)
    take = lambda a, i: np.take_along_axis(a, i, axis=1)
    c0, c1, m0, m1 = take(cdf, b), take(cdf, b + 1), take(m, b), take(m, b + 1)
    z = m0 + (uh - c0) / (c1 - c0) * (m1 - m0)
    slopes = (m[:, 1:] - m[:, :-1]) / (cdf[:, 1:] - cdf[:, :-1])
    return dict(z=z, bin=b, slope=take(slopes, b), slopes=slopes, m=m, cdf=cdf, u=uh)


def neighbour_slope(r: dict) -> np.ndarray:
    """Per fine sample, the largest slope of its bin and the bins on either side (a u within the
    cdf's rounding of a bin edge may land in the neighbouring bin)."""
    s, b = r["slopes"], r["bin"]
    n = s.shape[1]
    take = lambda i: np.take_along_axis(s, np.clip(i, 0, n - 1), axis=1)
    return np.maximum(take(b), np.maximum(take(b - 1), take(b + 1)))


def cdf_at(r: dict, z) -> np.ndarray:
    """The piecewise-linear cdf of `r` (importance's result) evaluated at depths z (rays, k), each in
    the bin r['bin'] names."""
    b = r["bin"]
    take = lambda a, i: np.take_along_axis(a, i, axis=1)
    c0, c1, m0, m1 = take(r["cdf"], b), take(r["cdf"], b + 1), take(r["m"], b), take(r["m"], b + 1)
    return c0 + (np.asarray(z, np.float64) - m0) / (m1 - m0) * (c1 - c0)


WEIGHT_KINDS = ("uniform", "zero", "onehot", "composited", "nonfinite")


def make_weights(kind: str, rays: int, S: int, rng) -> np.ndarray:
    """The weight arrays the tests sample from, (rays, S) float32:
      uniform     U(0, 1)
      zero        all zero (the floor alone: a uniform cdf)
      onehot      one sample per ray at 1: the first, the last (both outside the interior, so the
                  interior is all zero), then interior positions
      composited  the reference's alpha_j T_j of random densities with the 1e8 last delta, whose last
                  weight is ~1e-10 (render_maps_ref.composite64)
      nonfinite   uniform with NaN, +inf, -inf and negative entries on every ray
    """
    if kind == "uniform":
        return rng.uniform(0, 1, (rays, S)).astype(np.float32)
    if kind == "zero":
        return np.zeros((rays, S), np.float32)
    if kind == "onehot":
        w = np.zeros((rays, S), np.float32)
        hot = [0, S - 1, 1, S - 2, S // 2]
        for r in range(rays):
            w[r, hot[r % len(hot)] if r < len(hot) else rng.randint(S)] = 1.0
        return w
    if kind == "composited":
        import render_maps_ref
        sigma = rng.uniform(0, 3, (rays, S)) * (rng.uniform(0, 1, (rays, S)) < 0.5)
        dists = np.concatenate([rng.uniform(0.02, 0.2, (rays, S - 1)), np.full((rays, 1), 1e8)], axis=1)
        sigma[:, -1] = 1.0
        return render_maps_ref.composite64(np.zeros((rays, S, 3)), sigma, dists)["weights"].astype(np.float32)
    if kind == "nonfinite":
        w = rng.uniform(0, 1, (rays, S)).astype(np.float32)
        for r in range(rays):
            for q, bad in enumerate((np.nan, np.inf, -np.inf, -0.5)):
                w[r, (1 + r + 3 * q) % S] = bad
        return w
    raise ValueError(kind)


def merge(t_coarse, t_fine) -> np.ndarray:
    """t_all: the float32 values of both, sorted per ray."""
    return np.sort(np.concatenate([np.asarray(t_coarse, np.float32), np.asarray(t_fine, np.float32)], axis=1), axis=1)


def ray_points(rays, sample_t):
    """rays (n, 6) = [o, d], sample_t (n, S) -> (points (n*S, 3) float32, dists (n, S) float32):
    o + d t and [diff(t), 1e8] in float64, rounded once (train_nerf.py:299-311)."""
    rays = np.asarray(rays, np.float64)
    t = np.asarray(sample_t, np.float64)
    pts = rays[:, None, :3] + rays[:, None, 3:] * t[:, :, None]
    dists = np.concatenate([t[:, 1:] - t[:, :-1], np.full((t.shape[0], 1), 1e8)], axis=1)
    return pts.reshape(-1, 3).astype(np.float32), dists.astype(np.float32)


def rays_bwd(dp, t) -> np.ndarray:
    """input_grad_ref.rays_bwd with per-ray depths: dp (N, S, 3), t (N, S) -> (N, 6) =
    [sum_j d_p[j], sum_j t_j d_p[j]] in float64."""
    dp = np.asarray(dp, np.float64)
    t = np.asarray(t, np.float64)
    return np.concatenate([dp.sum(1), np.einsum("ns,nsc->nc", t, dp)], axis=1)


def rays_bwd_l1(e, t) -> np.ndarray:
    """rays_bwd's L1 companion: per-element bounds e >= 0 on dp to bounds on d_rays; with e = |dp|,
    sum_j |d_p[j]| and sum_j |t_j d_p[j]|."""
    return rays_bwd(np.abs(np.asarray(e, np.float64)), np.abs(np.asarray(t, np.float64)))
