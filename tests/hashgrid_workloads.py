"""The cases tests/test_gpu_hashgrid.py runs and tests/test_hashgrid_ref.py qualifies on the CPU: small
hash grids over a non-cubic box and points laid out as rays x samples (row i S + j), so that
neighbouring rows share cells at the coarse levels the way a training batch does, with the special
points a kernel can get wrong planted among them. Built once per case and never modified.

The shapes are the smallest at which the kernels can go wrong: R = 1, 63, 64, 65 (one wave, a lane
short of one, a lane over) and 24 x 32 (three workgroups); F = 1, 2, 4, 8 (each load width);
resolutions 2 (one cell), 3 and 17 (odd), 4..64 with 33 (odd, hashed at T = 2^12); T = 2^4, where
nearly every cell of a hashed level collides, and 2^12. With these, a level is summed in LDS when it
is dense, holds at most 8192 values and R >= res^3 (res 2, 3 from R = 63; res 4 from R = 64 exactly;
res 8 at R = 768), by the merged atomics otherwise: both d_table paths, and the switch between them,
are covered.
"""
from __future__ import annotations

import functools

import numpy as np

import hashgrid_ref as hr

LO = (-1.0, -0.5, 0.25)
HI = (1.5, 0.75, 2.0)
S = 32                                   # samples per ray
RES_1, RES_3, RES_5 = [2], [2, 3, 17], [4, 8, 16, 33, 64]

# (R, F, res, log2_table)
CASES = [
    (1, 1, RES_1, 4), (63, 2, RES_1, 4), (65, 8, RES_1, 12),
    (64, 1, RES_3, 4), (768, 4, RES_3, 4), (63, 2, RES_3, 12), (65, 8, RES_3, 12),
    (1, 2, RES_5, 12), (63, 4, RES_5, 12), (64, 1, RES_5, 12), (65, 8, RES_5, 12),
    (768, 1, RES_5, 12), (768, 2, RES_5, 12), (768, 4, RES_5, 12), (768, 8, RES_5, 12),
]
# the end-to-end grid: 8 levels x 4 features = the 32-wide input of the 32 -> 30 -> 30 -> 4 MLP
E2E = (768, 4, [2, 3, 4, 8, 16, 17, 33, 64], 12)

# Seeds are a formula of the case; these two are moved on until two distinct cells of the hashed
# res-17 level share an entry (with some sixty points in 4913 cells and 4096 entries not every seed
# gives one; tests/test_hashgrid_ref.py asserts it)
SEED_SHIFT = {(63, 2, (2, 3, 17), 12): 1, (65, 8, (2, 3, 17), 12): 2}

# rows of the planted points (cases with R >= 63)
ROW_LO, ROW_HI, ROW_PLANE, ROW_OUT0, ROW_NAN = 3, 5, 7, 9, 16   # ROW_OUT0 .. ROW_OUT0 + 5: outside;
# ROW_LO/HI/PLANE + 1 and ROW_NAN + 1 .. + 6 hold second copies


def case_id(c):
    R, F, res, lt = c
    return f"R{R}-F{F}-L{len(res)}-T{lt}"


def make_points(R, seed):
    """(points (R, 3) float32, sample_t (rays, S), rays (rays, 6)): short ray segments inside and
    around the box -- a segment spans about a twentieth of the box, so adjacent samples share cells up
    to res 64 -- with the planted points written over rows of the first ray."""
    rs = np.random.RandomState(seed)
    n = -(-R // S)
    lo, hi = np.asarray(LO), np.asarray(HI)
    ext = hi - lo
    o = lo + ext * rs.uniform(-0.05, 0.8, size=(n, 3))
    d = ext * rs.uniform(0.02, 0.08, size=(n, 3)) * rs.choice([-1.0, 1.0], size=(n, 3))
    rays = np.concatenate([o, d], 1).astype(np.float32)
    t = np.sort(rs.uniform(0.0, 1.0, size=(n, S)), 1).astype(np.float32)
    pts = (rays[:, None, :3].astype(np.float64) + rays[:, None, 3:].astype(np.float64) * t[:, :, None].astype(np.float64))
    pts = pts.reshape(-1, 3).astype(np.float32)[:R].copy()
    if R >= 63:
        lo32, hi32 = np.asarray(LO, np.float32), np.asarray(HI, np.float32)
        # (each planted point twice, so that its entries are no lone terms: adjacent rows for the
        # first three -- one run of equal indices in a wave --, a second copy further out for the rest)
        pts[ROW_LO] = pts[ROW_LO + 1] = lo32
        pts[ROW_HI] = pts[ROW_HI + 1] = hi32
        pts[ROW_PLANE] = pts[ROW_PLANE + 1] = (lo32 + hi32) / 2    # u = 1/2 exactly: a grid plane of res 3, 17, 33
        inside = lo32 + (hi32 - lo32) * np.asarray([0.3, 0.6, 0.45], np.float32)
        for q in range(6):                          # outside the box, one side each
            a, up = q // 2, q % 2
            pts[ROW_OUT0 + q] = inside
            pts[ROW_OUT0 + q, a] = hi32[a] + 0.5 if up else lo32[a] - 0.5
            pts[ROW_NAN + 1 + q] = inside
            pts[ROW_NAN + 1 + q, a] = hi32[a] + 0.25 if up else lo32[a] - 0.25
        pts[ROW_NAN] = inside
        pts[ROW_NAN, 1] = np.nan
    return pts, t, rays


@functools.lru_cache(maxsize=None)
def build(case):
    """The case's grid, inputs and float64 references (computed once; treat as read-only)."""
    R, F, res, lt = case
    res = list(res)
    seed = 1000 * R + 10 * F + lt + len(res) + 100000 * SEED_SHIFT.get(case, 0)
    grid = hr.Grid(res, F, lt, LO, HI)
    pts, t, rays = make_points(R, seed)
    rs = np.random.RandomState(seed + 1)
    table = rs.normal(size=(grid.total, F)).astype(np.float32)
    d_enc = rs.normal(size=(R, grid.width)).astype(np.float32)
    scale = np.float32(0.37)
    enc, enc_mag = hr.encode(grid, table, pts)
    want, mag, n = hr.grad_table(grid, pts, d_enc, scale)
    dp, dp_mag, live = hr.grad_points(grid, table, pts, d_enc, scale)
    for a in (pts, table, d_enc, enc, enc_mag, want, mag, n, dp, dp_mag, live):
        a.setflags(write=False)
    return dict(case=case, grid=grid, points=pts, sample_t=t, rays=rays, table=table, d_encoded=d_enc,
                scale=scale, enc=enc, enc_mag=enc_mag, d_table=want, d_table_mag=mag, d_table_n=n,
                d_points=dp, d_points_mag=dp_mag, live=live)


def hashable(c):
    R, F, res, lt = c
    return (R, F, tuple(res), lt)


ALL = [hashable(c) for c in CASES]
