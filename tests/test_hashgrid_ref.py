"""CPU tests of the hash-grid checker (tests/hashgrid_ref.py) and of the cases the GPU tests run
(tests/hashgrid_workloads.py): the checker's gradients against central differences in float64, and the
conditions that keep tests/test_gpu_hashgrid.py from passing vacuously, asserted on those very cases.
Also the host-only parts of the binding: lnerf_hashgrid_init and the struct's layout. No GPU.
"""
import ctypes

import numpy as np
import pytest

import hashgrid_ref as hr
import hashgrid_workloads as hw
import lnerf


def _objective(grid, table, pts, d_enc):
    enc, _ = hr.encode(grid, table, pts)
    return float((enc * d_enc.astype(np.float64)).sum())


@pytest.mark.parametrize("F,lt", [(1, 4), (2, 12), (4, 12)])
def test_checker_gradients_match_central_differences(F, lt):
    """L = sum(encode * dE) is linear in the table and piecewise linear in each coordinate, so central
    differences are exact up to float64 rounding wherever the step stays inside one cell."""
    grid = hr.Grid([2, 3, 17, 33], F, lt, hw.LO, hw.HI)
    rs = np.random.RandomState(7 + F)
    lo, hi = np.asarray(hw.LO), np.asarray(hw.HI)
    pts = (lo + (hi - lo) * rs.uniform(0.02, 0.98, size=(40, 3))).astype(np.float32)
    table = rs.normal(size=(grid.total, F)).astype(np.float32)
    d_enc = rs.normal(size=(40, grid.width)).astype(np.float32)
    want, _, n = hr.grad_table(grid, pts, d_enc)
    dp, _, live = hr.grad_points(grid, table, pts, d_enc)
    assert live.all()
    # table: steps of about 2^-6 (the float32 values actually reached) on touched and untouched entries
    touched = np.flatnonzero(n)
    picks = list(rs.choice(touched, 12)) + list(np.flatnonzero(n == 0)[:3])
    h = 2.0 ** -6
    for e in picks:
        f = rs.randint(F)
        tp, tm = table.copy(), table.copy()
        tp[e, f] += h
        tm[e, f] -= h
        num = (_objective(grid, tp, pts, d_enc) - _objective(grid, tm, pts, d_enc)) / (float(tp[e, f]) - float(tm[e, f]))
        assert abs(num - want[e, f]) <= 1e-9 * (1 + abs(want[e, f])), (e, f, num, want[e, f])
    # points: float32-exact steps; skip a coordinate within two steps of a cell face of the finest level
    for a in range(3):
        step = np.float32(2.0 ** -12)
        pp, pm = pts.copy(), pts.copy()
        pp[:, a] += step
        pm[:, a] -= step
        ok = np.ones(len(pts), bool)
        for l in range(grid.levels):
            ok &= (hr.cells(grid, pp, l)[0][:, a] == hr.cells(grid, pm, l)[0][:, a])
        assert ok.sum() >= 20
        for r in np.flatnonzero(ok):
            num = (_objective(grid, table, pp[r:r + 1], d_enc[r:r + 1])
                   - _objective(grid, table, pm[r:r + 1], d_enc[r:r + 1])) / (float(pp[r, a]) - float(pm[r, a]))
            assert abs(num - dp[r, a]) <= 1e-7 * (1 + abs(dp[r, a])), (r, a, num, dp[r, a])


def test_checker_scale_and_clamped_coordinates():
    w = hw.build(hw.ALL[-1])
    g = w["grid"]
    one, _, _ = hr.grad_table(g, w["points"], w["d_encoded"], 1.0)
    np.testing.assert_allclose(w["d_table"], float(w["scale"]) * one, rtol=1e-12, atol=0)
    dp, live = w["d_points"], w["live"]
    assert (dp[~live] == 0).all() and (dp[live] != 0).mean() > 0.99


@pytest.mark.parametrize("case", hw.ALL + [hw.hashable(hw.E2E)], ids=hw.case_id)
def test_cases_cannot_pass_vacuously(case):
    w = hw.build(case)
    g, pts, n = w["grid"], w["points"], w["d_table_n"]
    R = case[0]
    assert n.sum() == R * 8 * g.levels
    if g.levels > 1:
        assert any(g.dense) and not all(g.dense), "a dense and a hashed level"
    else:
        assert g.dense == [True]                      # res 2: eight entries, dense at any T
    if R < 63:
        return
    # the planted points: on lo, on hi, on an interior grid plane, outside on each side, one NaN
    assert (pts[hw.ROW_LO] == g.lo).all() and (pts[hw.ROW_HI] == g.hi).all()
    live = w["live"]
    assert live[hw.ROW_LO].all() and live[hw.ROW_HI].all()
    for l in range(g.levels):
        i, wgt, _ = hr.cells(g, pts[[hw.ROW_LO, hw.ROW_HI]], l)
        assert (i[0] == 0).all() and (wgt[0] == 0).all()
        assert (i[1] == g.res[l] - 2).all() and (wgt[1] == 1).all()      # hi: the last cell, weight 1
    odd = [l for l in range(g.levels) if g.res[l] % 2 == 1]
    for l in odd:
        i, wgt, _ = hr.cells(g, pts[[hw.ROW_PLANE]], l)
        assert (wgt[0] == 0).all() and (i[0] == (g.res[l] - 1) // 2).all()
    for q in range(6):
        a, up = q // 2, q % 2
        row = hw.ROW_OUT0 + q
        assert not live[row, a] and live[row].sum() == 2
        assert pts[row, a] > g.hi[a] if up else pts[row, a] < g.lo[a]
    assert np.isnan(pts[hw.ROW_NAN, 1]) and not live[hw.ROW_NAN, 1] and np.isnan(pts[hw.ROW_NAN]).sum() == 1
    assert np.isfinite(w["enc"]).all() and np.isfinite(w["d_points"]).all()
    # neighbouring rows share cells: fewer than half of the touched entries have a single term
    touched = n[n > 0]
    assert (touched == 1).sum() < 0.5 * len(touched), ((touched == 1).sum(), len(touched))
    if not all(g.dense):
        # at some hashed level one entry receives terms from two distinct cells
        collided = False
        for l in range(g.levels):
            if g.dense[l]:
                continue
            i, _, _ = hr.cells(g, pts, l)
            ent = hr.corner_entries(g, i, l).ravel()
            lin = hr.corner_cells(g, i, l)[3].ravel()
            pairs = np.unique(np.stack([ent, lin], 1), axis=0)
            collided |= len(pairs) > len(np.unique(pairs[:, 0]))
        assert collided
    # adjacent rows repeat an entry within a wave (what the run merging works on) ...
    i, _, _ = hr.cells(g, pts, 0)
    ent = hr.corner_entries(g, i, 0)
    assert (ent[1:] == ent[:-1]).any()
    # ... and at the finest level some do not (lone lanes: the plain per-corner atomic)
    i, _, _ = hr.cells(g, pts, g.levels - 1)
    ent = hr.corner_entries(g, i, g.levels - 1)
    if g.levels > 1:
        assert (ent[1:] != ent[:-1]).any()


def test_ref_grid_matches_the_binding_and_init():
    """hashgrid_ref.Grid, lnerf.HashGrid.from_levels and lnerf_hashgrid_init agree on resolutions and
    offsets; init is host-only, so this needs no GPU."""
    for case in hw.ALL:
        _, F, res, lt = case
        g = hr.Grid(res, F, lt, hw.LO, hw.HI)
        b = lnerf.HashGrid.from_levels(res, F, lt, hw.LO, hw.HI)
        assert (b.res, b.offsets, b.total_entries, b.width) == (g.res, g.offset, g.total, g.width)
    for levels, F, lt, base, top in [(16, 2, 19, 16, 2048), (1, 4, 4, 2, 2), (5, 8, 12, 4, 64), (32, 1, 24, 16, 4096)]:
        b = lnerf.HashGrid(levels, F, lt, base, top, hw.LO, hw.HI)
        g = hr.Grid(hr.init_res(levels, base, top), F, lt, hw.LO, hw.HI)
        assert (b.res, b.offsets) == (g.res, g.offset)
        assert b.res[0] == base and b.res[-1] == top and b.total_entries == g.total
        assert all(o % 4 == 0 for o in b.offsets)
        assert b.lo == [float(np.float32(v)) for v in hw.LO]


@pytest.mark.parametrize("args", [
    (0, 2, 19, 16, 2048), (33, 2, 19, 16, 2048), (16, 3, 19, 16, 2048), (16, 2, 3, 16, 2048),
    (16, 2, 25, 16, 2048), (16, 2, 19, 1, 2048), (16, 2, 19, 32, 16),
])
def test_init_rejects_bad_arguments_and_leaves_the_struct(args):
    lib = lnerf.load_library()
    g = lnerf.LnerfHashGrid()
    g.levels = 77
    lo, hi = (ctypes.c_float * 3)(*hw.LO), (ctypes.c_float * 3)(*hw.HI)
    assert lib.lnerf_hashgrid_init(ctypes.byref(g), *args, lo, hi) < 0
    assert lnerf.last_error() != "" and g.levels == 77
    assert lib.lnerf_hashgrid_init(ctypes.byref(g), 4, 2, 12, 4, 32, hi, lo) < 0      # hi <= lo
    assert lib.lnerf_hashgrid_init(None, 4, 2, 12, 4, 32, lo, hi) < 0
    assert g.levels == 77
