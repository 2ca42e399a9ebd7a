"""Numpy float64 / int64 checker of the occupancy grid (include/lnerf.h "Occupancy grid"): the four
formulas exactly as the header states them, operation for operation, so that the GPU's outputs can be
compared bit for bit. Nothing here imitates the kernels: the k-th occupied step comes from a cumsum
over the whole march, the bitfield is expanded to one boolean per cell, the maximum is a Python-level
np.maximum.at. tests/test_occgrid_ref.py checks this file against properties it must have (and a
separate brute-force march) before it judges the GPU.
"""
import numpy as np

OCC_MEAN = 1
OCC_LAST_OPAQUE = 2
FLT_MAX = np.float32(np.finfo(np.float32).max)


def unit_clamp(u):
    """u clamped to [0, 1] as float64, a NaN taken as 0."""
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(u > 0, np.where(u < 1, u.astype(np.float64), 1.0), 0.0)


def _box(lo, hi):
    lo = np.asarray(lo, np.float32).astype(np.float64)
    hi = np.asarray(hi, np.float32).astype(np.float64)
    return lo, hi - lo


def unpack_bits(bits, res):
    """(res^3,) booleans from the uint32 words: cell c is bit c & 31 of word c >> 5."""
    words = np.ascontiguousarray(bits).view(np.uint32).astype(np.uint64)
    c = np.arange(res ** 3, dtype=np.int64)
    return ((words[c >> 5] >> (c & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)


def pack_bits(flags):
    """The uint32 words of a (res^3,) boolean array."""
    f = np.asarray(flags, bool).reshape(-1, 32).astype(np.uint64)
    return (f << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def cell_points(res, lo, hi, cells=None, u=None):
    """p_c = (float)(lo_c + (g_c + u_c) / res * (hi_c - lo_c)); an index outside the grid gives the box
    centre (float)(lo_c + 0.5 (hi_c - lo_c))."""
    lo, ext = _box(lo, hi)
    c = np.arange(res ** 3, dtype=np.int64) if cells is None else np.asarray(cells, np.int64)
    inside = (c >= 0) & (c < res ** 3)
    ci = np.where(inside, c, 0)
    g = np.stack([ci % res, (ci // res) % res, ci // (res * res)], axis=1).astype(np.float64)
    uu = np.full((c.size, 3), 0.5) if u is None else unit_clamp(u)
    w = np.where(inside[:, None], (g + uu) / float(res), 0.5)
    return (lo[None, :] + w * ext[None, :]).astype(np.float32)


def update(res, density, cells, sigma, decay):
    """density * decay in float32 (skipped at decay == 1), then the maximum with every valid sigma: a NaN
    or a value <= 0 ignored, +inf as FLT_MAX, indices outside the grid skipped. `sigma` is (n,), already
    gathered at the caller's stride."""
    d = np.asarray(density, np.float32).copy()
    if np.float32(decay) != np.float32(1):
        d = d * np.float32(decay)
    c = np.arange(res ** 3, dtype=np.int64) if cells is None else np.asarray(cells, np.int64)
    s = np.asarray(sigma, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (c >= 0) & (c < res ** 3) & (s > 0)
    np.maximum.at(d, c[ok], np.minimum(s[ok], FLT_MAX))
    return d


def threshold(res, density, thr, flags=0):
    """(bits (res^3 / 32,) uint32, mean float64, occupied int): bit c = density[c] > thr', thr' = thr or,
    under OCC_MEAN, min(thr, mean)."""
    d = np.asarray(density, np.float32).astype(np.float64)
    mean = d.sum() / float(res ** 3)
    t = float(np.float32(thr))
    if flags & OCC_MEAN:
        t = min(t, mean)
    on = d > t
    return pack_bits(on), mean, int(on.sum())


def mean_margin(res, density):
    """The smallest |density[c] - mean| over the cells, over the tolerance res^3 2^-52 mean of the mean:
    above 1, no summation order can move a cell across the mean."""
    d = np.asarray(density, np.float32).astype(np.float64)
    mean = d.sum() / float(res ** 3)
    tol = res ** 3 * 2.0 ** -52 * mean
    return float(np.abs(d - mean).min() / tol) if tol > 0 else np.inf


def march(res, lo, hi, bits, rays, steps, near, far):
    """(n, M) booleans: step i of each ray is occupied. c_i = near + (i + 0.5) h, p = o + d c_i,
    w = (p - lo) / (hi - lo), inside if 0 <= w < 1 on every axis (a NaN fails), cell g = min((int)(w res),
    res - 1)."""
    lo, ext = _box(lo, hi)
    on = unpack_bits(bits, res)
    rays = np.asarray(rays, np.float32).astype(np.float64)
    near, far = float(np.float32(near)), float(np.float32(far))
    h = (far - near) / float(steps)
    c = near + (np.arange(steps, dtype=np.float64) + 0.5) * h
    with np.errstate(invalid="ignore", over="ignore"):
        p = rays[:, None, :3] + rays[:, None, 3:] * c[None, :, None]          # (n, M, 3)
        w = (p - lo) / ext
        ok = (w >= 0) & (w < 1)
        g = np.minimum(np.where(ok, w * float(res), 0.0).astype(np.int64), res - 1)
    cell = g[..., 0] + res * (g[..., 1] + res * g[..., 2])
    return ok.all(axis=2) & on[cell]


def sample(res, lo, hi, bits, rays, S, steps, near, far, u=None, flags=0):
    """(sample_t (n, S) float32, dists (n, S) float32, n_occ (n,) int32) as lnerf_sample_occupancy states
    them. The k-th occupied step is found by a cumsum over the ray's whole march."""
    occ = march(res, lo, hi, bits, rays, steps, near, far)
    n, M = occ.shape
    N = occ.sum(axis=1).astype(np.int64)
    eff = np.where((N == 0)[:, None], True, occ)
    Np = eff.sum(axis=1).astype(np.int64)
    near, far = float(np.float32(near)), float(np.float32(far))
    h = (far - near) / float(M)
    uu = np.full((n, S), 0.5) if u is None else unit_clamp(u)
    q = (np.arange(S, dtype=np.float64)[None, :] + uu) * Np[:, None].astype(np.float64) / float(S)
    k = np.minimum(q.astype(np.int64), Np[:, None] - 1)
    f = q - k.astype(np.float64)
    rank = np.cumsum(eff, axis=1) - 1                    # rank[r, i] = occupied steps before step i, at an occupied i
    idx = np.empty((n, S), np.int64)
    for r in range(n):
        steps_on = np.flatnonzero(eff[r])                # brute force: the list of occupied steps
        assert (rank[r, steps_on] == np.arange(steps_on.size)).all()
        idx[r] = steps_on[k[r]]
    t = (near + (idx.astype(np.float64) + f) * h).astype(np.float32)
    dists = np.repeat((Np.astype(np.float64) * h / float(S)).astype(np.float32)[:, None], S, axis=1)
    if flags & OCC_LAST_OPAQUE:
        dists[:, -1] = np.float32(1e8)
    return t, dists, N.astype(np.int32)
