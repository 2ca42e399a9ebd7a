"""The cases the occupancy-grid tests run (tests/test_occgrid_ref.py on the CPU, tests/test_gpu_occgrid.py
on the GPU): bitfields, rays with every planted kind, random numbers with the special values planted,
densities and update lists. Only numpy is used; tests/test_occgrid_ref.py holds the conditions these
inputs must meet before a GPU comparison on them means anything.

Sampler cases are (res, M, S, rays, bitfield kind, depth range). The box is [-1, 1]^3 throughout. Every
value of res in {4, 8, 32}, M in {64, 128, 1024}, S in {1, 3, 64, 65, 200} and rays in {1, 5, 130}
appears; 5 and 130 are no multiples of the four rays a workgroup takes.

Planted rays (kind -> what its march must look like, asserted on the CPU):
  miss      never inside the box: N = 0 whatever the bitfield
  inside    starts inside the box and stays there: N = M when every bit is set
  nan       a NaN direction component: every comparison fails, N = 0
  only0, only63, only64, onlylast
            clips the box's (-1, -1) edge so that exactly one step (0, 63, min(64, M - 1), M - 1) is
            inside it; the cell there, (0, 0, res / 2), is set in the "all" and "checker" bitfields
  alt       along +x through cell centres, one cell per step for the first res steps: under the
            "checker" bitfield its mask alternates
A case with fewer than 130 rays takes a window of the planted kinds that moves with the case's index,
so that the cases together hold them all.
"""
from __future__ import annotations

import functools

import numpy as np

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
RANGES = [(2.0, 6.0), (0.5, 3.25)]
KINDS = ("all", "none", "sphere", "checker", "random")
PLANTED = ("miss", "inside", "nan", "only0", "only63", "only64", "onlylast", "alt")

SAMPLER_CASES = [
    (4, 64, 1, 1, "all", 0),
    (4, 128, 3, 5, "checker", 1),
    (8, 1024, 64, 130, "sphere", 0),
    (8, 64, 65, 5, "random", 1),
    (32, 64, 200, 130, "checker", 0),
    (32, 128, 64, 5, "sphere", 0),
    (32, 1024, 65, 130, "random", 1),
    (8, 128, 200, 1, "none", 0),
    (4, 1024, 3, 130, "all", 1),
    (32, 1024, 1, 5, "checker", 0),
    (8, 128, 64, 5, "all", 0),
]


def case_id(case):
    res, M, S, rays, kind, rg = case
    return f"res{res}-M{M}-S{S}-rays{rays}-{kind}-range{rg}"


def cell_coords(res):
    c = np.arange(res ** 3, dtype=np.int64)
    return c % res, (c // res) % res, c // (res * res)


def bitfield(res, kind, seed=0):
    """(res^3 / 32,) uint32 words of a bitfield kind."""
    import occgrid_ref as oref
    gx, gy, gz = cell_coords(res)
    if kind == "all":
        on = np.ones(res ** 3, bool)
    elif kind == "none":
        on = np.zeros(res ** 3, bool)
    elif kind == "sphere":
        ctr = [(g + 0.5) * 2.0 / res - 1.0 for g in (gx, gy, gz)]
        on = ctr[0] ** 2 + ctr[1] ** 2 + ctr[2] ** 2 < 0.7 ** 2
    elif kind == "checker":
        on = ((gx + gy + gz) & 1) == 0
    elif kind == "random":
        on = np.random.RandomState(seed + res).uniform(0, 1, res ** 3) < 0.3
    else:
        raise ValueError(kind)
    return oref.pack_bits(on)


def planted_ray(kind, res, M, near, far):
    """The ray [o, d] (float64, before the float32 rounding) of a planted kind."""
    h = (far - near) / M
    if kind == "miss":
        return [5.0, 5.0, 5.0, 0.0, 0.0, 1.0]
    if kind == "inside":
        return [0.1, 0.2, -0.3, 0.1, 0.05, 0.02]
    if kind == "nan":
        return [0.1, 0.2, -0.3, np.nan, 0.0, 0.1]
    if kind == "alt":
        dx = 2.0 / (res * h)
        y = -1.0 + 1.0 / res          # the centre of cell row 0
        return [-1.0 - dx * near, y, y, dx, 0.0, 0.0]
    i = dict(only0=0, only63=63, only64=min(64, M - 1), onlylast=M - 1)[kind]
    c = near + (i + 0.5) * h
    # x = ox + t >= -1 from t = c - h / 4 on, y = oy - t >= -1 up to t = c + h / 4; z in cell res / 2
    return [-1.0 - c + h / 4, c + h / 4 - 1.0, 0.5 / res, 1.0, -1.0, 0.0]


def planted_step(kind, M):
    return dict(only0=0, only63=63, only64=min(64, M - 1), onlylast=M - 1)[kind]


def camera_rays(rng, n):
    """Rays from a sphere of radius 4 towards a jittered point near the origin, unit directions."""
    o = rng.normal(size=(n, 3))
    o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.6, 0.6, (n, 3)) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1)


def planted_u(rng, rays, n):
    """Uniform numbers with 0, the float32 just under 1, 1.5, -1 and NaN planted every few entries (the
    planting of tests/test_gpu_sampling.py::_u)."""
    u = rng.uniform(0, 1, (rays, n)).astype(np.float32)
    special = np.array([0.0, np.float32(1) - np.float32(2.0 ** -24), 1.5, -1.0, np.nan], np.float32)
    flat = u.reshape(-1)
    idx = np.arange(0, flat.size, 3)
    flat[idx] = special[np.arange(idx.size) % 5]
    return u


@functools.lru_cache(maxsize=None)
def sampler_case(index):
    """dict(res, M, S, n, near, far, bits (uint32 words), rays (n, 6) float32, kinds (n,) names, u (n, S)
    float32) of SAMPLER_CASES[index]. Cached: the arrays are shared and must not be written."""
    res, M, S, n, kind, rg = SAMPLER_CASES[index]
    near, far = RANGES[rg]
    rng = np.random.RandomState(1000 + index)
    pool = [planted_ray(k, res, M, near, far) for k in PLANTED]
    names = list(PLANTED)
    if n >= len(PLANTED):
        rows = np.concatenate([np.array(pool), camera_rays(rng, n - len(PLANTED))], axis=0)
        names += ["camera"] * (n - len(PLANTED))
    else:
        pick = (3 * index + np.arange(n)) % len(PLANTED)
        rows = np.array([pool[p] for p in pick])
        names = [PLANTED[p] for p in pick]
    out = dict(res=res, M=M, S=S, n=n, near=near, far=far, kind=kind, bits=bitfield(res, kind, index),
               rays=rows.astype(np.float32), kinds=tuple(names), u=planted_u(rng, n, S))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- densities, update lists ----------------------------------------------------------------------

LEVELS = np.array([0.0, 0.001, 0.5, 3.0, 40.0], np.float32)


def density(res, seed=0):
    """(res^3,) float32 from five well-separated levels, so that the mean (about 8.7) is far from every
    cell: no float64 summation order can move a cell across it (asserted in test_occgrid_ref.py)."""
    rng = np.random.RandomState(seed + 7 * res)
    return LEVELS[rng.randint(0, LEVELS.size, res ** 3)].copy()


UPDATE_CASES = [(res, decay, stride) for res in (4, 8) for decay in (1.0, 0.95, 0.0) for stride in (1, 4)]
SPECIAL_SIGMA = np.array([np.nan, -1.0, 0.0, -0.0, np.inf, -np.inf, 3.0e38, 1e-30], np.float32)


def update_list(res, stride, seed=0):
    """(cells (n,) int32, sigma buffer ((n - 1) stride + 1,) float32, sigma (n,) float32): random cells
    with duplicates (n = 3 res^3 / 2 draws from half the grid), indices outside the grid, and the special
    values, each of them also as the ONLY value its cell receives and on a cell that others raise."""
    cells_total = res ** 3
    rng = np.random.RandomState(seed + res + stride)
    n = 3 * cells_total // 2
    cells = rng.randint(0, cells_total // 2, n).astype(np.int32)
    sigma = rng.uniform(0.0, 50.0, n).astype(np.float32)
    cells[::17] = np.array([-1, cells_total, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int32)[
        np.arange(cells[::17].size) % 4]
    k = SPECIAL_SIGMA.size
    # alone on cells of the upper half (nobody else writes there) ...
    cells[1:1 + k] = cells_total // 2 + np.arange(k)
    sigma[1:1 + k] = SPECIAL_SIGMA
    # ... and on busy cells
    sigma[40:40 + k] = SPECIAL_SIGMA
    buf = rng.uniform(100.0, 200.0, (n - 1) * stride + 1).astype(np.float32)   # the other columns: loud
    buf[::stride] = sigma
    return cells, buf, sigma


def cell_list(res, seed=0):
    """(cells (n,) int32, u (n, 3) float32): a subset with repeats, indices outside the grid, and u with
    the special values planted."""
    rng = np.random.RandomState(seed + res)
    n = 77
    cells = rng.randint(0, res ** 3, n).astype(np.int32)
    cells[5] = cells[6] = cells[50]
    cells[10], cells[11], cells[12] = -1, res ** 3, np.iinfo(np.int32).max
    cells[0], cells[1] = 0, res ** 3 - 1
    return cells, planted_u(rng, n, 3)
