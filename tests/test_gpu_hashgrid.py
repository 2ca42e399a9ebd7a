"""GPU tests of the multiresolution hash grid (include/lnerf.h "Multiresolution hash grid"):
lnerf_hashgrid_encode and lnerf_hashgrid_grad against the float64 checker of tests/hashgrid_ref.py on
the cases of tests/hashgrid_workloads.py (which tests/test_hashgrid_ref.py qualifies on the CPU), their
error paths, and the end-to-end chain scene.hashgrid_step / lnerf.hashgrid_autograd.

Bars (hashgrid_ref.forward_bar / points_bar / table_bar):
  * encoded: 2^-23 |ref| + 8 2^-52 sum |term|; the checker keeps the kernel's operation order, so the
    tests also print whether the result was bit-equal;
  * d_points: one float32 rounding, 2^-24 |ref|, plus the float64 order term
    (levels (9 F + 3) + 1) 2^-52 sum |term|; exactly 0 for a clamped or NaN coordinate; the same bits
    on a repeated call;
  * d_table, per entry with n terms: 2^-23 |want| + (n + 2) 2^-24 sum |term| (one float32 rounding per
    term, at most n float32 adds in any order). Under LNERF_ACCUMULATE the value the buffer held is one
    more term. Untouched entries: +0, or the buffer's own bits under LNERF_ACCUMULATE.
Every output sits between two 64-float guard bands that must come back untouched.

Worst error / bar measured on an MI355X over the 15 cases (the tests print them): encoded 0.24-0.50
and bit-equal to the checker in every case; d_points 0.29-0.995 (the float32 rounding alone: the bar's
first term is exactly half an ulp at a power of two); d_table 0.014-0.31 (second call the same to three
digits, without scale 0.005-0.30, under LNERF_ACCUMULATE 0.008-0.25) with up to 1253 terms per entry;
end to end d_table 0.18, d_points 0.98, d_rays 0.32. The timings are in DESIGN.md section 3 "kh".
"""
import ctypes
import functools

import numpy as np
import pytest

import hashgrid_ref as hr
import hashgrid_workloads as hw

pytestmark = pytest.mark.gpu

SENT = -7.25       # guard bands and not-yet-written outputs
HELD = 1.25        # what a d_table holds before an LNERF_ACCUMULATE call
BAND = 64
ACCUMULATE = 2


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Banded:
    """A float32 device buffer of `shape` between two guard bands."""

    def __init__(self, shape, fill=SENT):
        import torch
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * BAND,), SENT, dtype=torch.float32, device="cuda:0")
        self.view = self.whole[BAND:BAND + n].view(*shape)
        self.view.fill_(fill)
        self.n = n

    def get(self):
        """The payload as numpy, after asserting that both bands still hold the sentinel."""
        w = _np(self.whole)
        assert (_bits(w[:BAND]) == _bits(np.float32(SENT))).all(), "guard band before the buffer was written"
        assert (_bits(w[BAND + self.n:]) == _bits(np.float32(SENT))).all(), "guard band after the buffer was written"
        return w[BAND:BAND + self.n].reshape(tuple(self.view.shape)).copy()


def _grid_struct(g):
    import lnerf
    b = lnerf.HashGrid.from_levels(g.res, g.features, g.log2_table, hw.LO, hw.HI)
    assert b.offsets == g.offset
    return b


def _encode(eng, b, table, points, R, out):
    return eng.lib.lnerf_hashgrid_encode(ctypes.byref(b.struct) if b is not None else None, _p(table), _p(points), R,
                                         _p(out), eng._stream())


def _grad(eng, b, table, points, R, d_enc, scale, flags, d_table, d_points):
    return eng.lib.lnerf_hashgrid_grad(ctypes.byref(b.struct) if b is not None else None, _p(table), _p(points), R,
                                       _p(d_enc), _p(scale), flags, _p(d_table), _p(d_points), eng._stream())


_ENGINE = None


@functools.lru_cache(maxsize=None)
def _run(case):
    """Every call the per-case tests look at, made once."""
    import lnerf
    eng = _ENGINE
    w = hw.build(case)
    g = w["grid"]
    R = case[0]
    b = _grid_struct(g)
    table, pts, d_enc = _dev(w["table"]), _dev(w["points"]), _dev(w["d_encoded"])
    scale = _dev(np.array([w["scale"]], np.float32))
    out = {}
    enc = Banded((R, g.width))
    assert _encode(eng, b, table, pts, R, enc.view) == 0, lnerf.last_error()
    out["enc"] = enc.get()
    out["enc_wrapper"] = _np(eng.hashgrid_encode(b, table, pts))
    dt, dp = Banded((g.total, g.features)), Banded((R, 3))
    assert _grad(eng, b, table, pts, R, d_enc, scale, 0, dt.view, dp.view) == 0, lnerf.last_error()
    out["d_table"], out["d_points"] = dt.get(), dp.get()
    assert _grad(eng, b, table, pts, R, d_enc, scale, 0, dt.view, dp.view) == 0, lnerf.last_error()
    out["d_table_again"], out["d_points_again"] = dt.get(), dp.get()
    held = Banded((g.total, g.features), HELD)
    assert _grad(eng, b, None, pts, R, d_enc, scale, ACCUMULATE, held.view, None) == 0, lnerf.last_error()
    out["d_table_acc"] = held.get()
    plain = Banded((g.total, g.features))
    assert _grad(eng, b, None, pts, R, d_enc, None, 0, plain.view, None) == 0, lnerf.last_error()
    out["d_table_unscaled"] = plain.get()
    only = Banded((R, 3))
    assert _grad(eng, b, table, pts, R, d_enc, scale, 0, None, only.view) == 0, lnerf.last_error()
    out["d_points_only"] = only.get()
    return out


@pytest.fixture
def run(engine):
    global _ENGINE
    _ENGINE = engine
    return _run


def _ratio(err, bar):
    """max err / bar; an exact value with a zero bar (every term 0) counts as 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bar).max())


def _check_table(got, want, mag, n, what):
    bar = hr.table_bar(want, mag, n)
    touched = n > 0
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all(), what
    assert (err[touched] <= bar[touched]).all(), (what, _ratio(err[touched], bar[touched]))
    return _ratio(err[touched], bar[touched])


@pytest.mark.parametrize("case", hw.ALL, ids=hw.case_id)
def test_encode_matches_the_checker(run, case):
    w, o = hw.build(case), run(case)
    bar = hr.forward_bar(w["enc"], w["enc_mag"])
    err = np.abs(o["enc"].astype(np.float64) - w["enc"])
    equal = bool((_bits(o["enc"]) == _bits(w["enc"].astype(np.float32))).all())
    print(f"encode {hw.case_id(case)}: worst error / bar {_ratio(err, bar):.3f}, bit-equal {equal}")
    assert np.isfinite(o["enc"]).all()
    assert (err <= bar).all(), _ratio(err, bar)
    assert (_bits(o["enc_wrapper"]) == _bits(o["enc"])).all()


@pytest.mark.parametrize("case", hw.ALL, ids=hw.case_id)
def test_d_points_matches_the_checker(run, case):
    w, o = hw.build(case), run(case)
    bar = hr.points_bar(w["grid"], w["d_points"], w["d_points_mag"])
    err = np.abs(o["d_points"].astype(np.float64) - w["d_points"])
    print(f"d_points {hw.case_id(case)}: worst error / bar {_ratio(err, bar):.3f}")
    assert (err <= bar).all(), _ratio(err, bar)
    assert (_bits(o["d_points"])[~w["live"]] == 0).all()          # exactly +0: clamped or NaN
    assert (_bits(o["d_points_again"]) == _bits(o["d_points"])).all()
    assert (_bits(o["d_points_only"]) == _bits(o["d_points"])).all()


@pytest.mark.parametrize("case", hw.ALL, ids=hw.case_id)
def test_d_table_matches_the_checker(run, case):
    w, o = hw.build(case), run(case)
    want, mag, n = w["d_table"], w["d_table_mag"], w["d_table_n"]
    s = float(w["scale"])
    r0 = _check_table(o["d_table"], want, mag, n, "d_table")
    r1 = _check_table(o["d_table_again"], want, mag, n, "d_table, second call")
    r2 = _check_table(o["d_table_unscaled"], want / s, mag / s, n, "d_table without scale")
    r3 = _check_table(o["d_table_acc"], HELD + want, abs(HELD) + mag, n + 1, "d_table under LNERF_ACCUMULATE")
    print(f"d_table {hw.case_id(case)}: worst error / bar {r0:.3f} (again {r1:.3f}, unscaled {r2:.3f}, "
          f"accumulate {r3:.3f}); terms per entry up to {int(n.max())}")
    untouched = n == 0
    for key in ("d_table", "d_table_again", "d_table_unscaled"):
        assert (_bits(o[key])[untouched] == 0).all(), key                       # exactly +0
    assert (_bits(o["d_table_acc"])[untouched] == _bits(np.float32(HELD))).all()
    # the scale is multiplied in (the two bars overlap only if it was)
    big = (n > 0) & (np.abs(want).max(1) > 16 * hr.table_bar(want, mag, n).max(1))
    assert big.any()
    np.testing.assert_allclose(o["d_table"][big], s * o["d_table_unscaled"][big].astype(np.float64), rtol=0.05)


@pytest.mark.parametrize("case,rows", [(hw.ALL[12], (40, hw.ROW_LO)), (hw.ALL[6], (64,)), (hw.ALL[4], (700,))],
                         ids=lambda v: hw.case_id(v) if len(v) == 4 else str(v))
def test_a_nan_row_reaches_exactly_its_own_entries(engine, case, rows):
    w = hw.build(case)
    g, R = w["grid"], case[0]
    b = _grid_struct(g)
    pts = _dev(w["points"])
    for row in rows:
        d_enc = w["d_encoded"].copy()
        d_enc[row] = np.nan
        dt = Banded((g.total, g.features))
        assert _grad(engine, b, None, pts, R, _dev(d_enc), None, 0, dt.view, None) == 0
        got = dt.get()
        mine = sorted(hr.row_entries(g, w["points"], row))
        assert len(mine) <= 8 * g.levels
        want_nan = np.zeros((g.total, g.features), bool)
        want_nan[mine] = True
        assert (np.isnan(got) == want_nan).all(), (row, np.isnan(got).sum(), want_nan.sum())


def test_error_paths_write_nothing(engine):
    import lnerf
    case = hw.ALL[5]                      # R 63, F 2, three levels
    w = hw.build(case)
    g, R = w["grid"], case[0]
    table, pts, d_enc = _dev(w["table"]), _dev(w["points"]), _dev(w["d_encoded"])
    enc, dt, dp = Banded((R, g.width)), Banded((g.total, g.features)), Banded((R, 3))

    def untouched():
        for buf in (enc, dt, dp):
            assert (_bits(buf.get()) == _bits(np.float32(SENT))).all()

    def bad_grid(edit):
        b = _grid_struct(g)
        edit(b.struct)
        return b

    def set_(name, value, index=None):
        def edit(s):
            if index is None:
                setattr(s, name, value)
            else:
                getattr(s, name)[index] = value
        return edit

    good = _grid_struct(g)
    grids = [None, bad_grid(set_("levels", 0)), bad_grid(set_("levels", 33)), bad_grid(set_("features", 3)),
             bad_grid(set_("features", 0)), bad_grid(set_("log2_table", 3)), bad_grid(set_("log2_table", 25)),
             bad_grid(set_("res", 1, 1)), bad_grid(set_("offset", g.offset[2] + g.entries[2] - 1, 3)),
             bad_grid(set_("offset", g.offset[1] - 1, 2)), bad_grid(set_("offset", -4, 0)),
             bad_grid(set_("hi", hw.LO[0], 0)), bad_grid(set_("hi", float("nan"), 2)),
             bad_grid(set_("lo", float("inf"), 1))]
    for i, b in enumerate(grids):
        assert _encode(engine, b, table, pts, R, enc.view) < 0, i
        assert lnerf.last_error() != ""
        assert _grad(engine, b, table, pts, R, d_enc, None, 0, dt.view, dp.view) < 0, i
        assert lnerf.last_error() != ""
    # encode's own arguments
    assert _encode(engine, good, None, pts, R, enc.view) < 0
    assert _encode(engine, good, table, None, R, enc.view) < 0
    assert _encode(engine, good, table, pts, R, None) < 0
    assert _encode(engine, good, table, pts, -1, enc.view) < 0
    assert _encode(engine, good, table.view(-1)[1:], pts, R, enc.view) < 0        # F = 2: 8-byte rows
    # grad's own arguments
    assert _grad(engine, good, table, pts, R, d_enc, None, 0, None, None) < 0      # both outputs NULL
    assert _grad(engine, good, table, None, R, d_enc, None, 0, dt.view, dp.view) < 0
    assert _grad(engine, good, table, pts, R, None, None, 0, dt.view, dp.view) < 0
    assert _grad(engine, good, None, pts, R, d_enc, None, 0, dt.view, dp.view) < 0   # d_points needs the table
    assert _grad(engine, good, None, pts, R, d_enc, None, 0, None, dp.view) < 0
    assert _grad(engine, good, table, pts, -1, d_enc, None, 0, dt.view, dp.view) < 0
    assert _grad(engine, good, table, pts, R, d_enc, None, 4, dt.view, dp.view) < 0  # a flag that is not ACCUMULATE
    assert _grad(engine, good, table, pts, R, d_enc, None, ACCUMULATE | 1, dt.view, dp.view) < 0
    assert _grad(engine, good, table.view(-1)[1:], pts, R, d_enc, None, 0, dt.view, dp.view) < 0
    assert lnerf.last_error() != ""
    untouched()
    # R == 0 succeeds and launches nothing
    assert _encode(engine, good, table, pts, 0, enc.view) == 0
    assert _grad(engine, good, table, pts, 0, d_enc, None, 0, dt.view, dp.view) == 0
    untouched()
    # and the Python surface refuses what it can see
    with pytest.raises(ValueError):
        engine.hashgrid_encode(good, table[:-1], pts)
    with pytest.raises(ValueError):
        engine.hashgrid_grad(good, table, pts, d_enc[:, :-1].contiguous())
    with pytest.raises(ValueError):
        engine.hashgrid_grad(good, table, pts, d_enc, accumulate=True)


def test_end_to_end_step_and_autograd(engine):
    """24 rays x 32 samples through ray_points -> encode -> train_step (32 -> 30 -> 30 -> 4) -> grad:
    scene.hashgrid_step's d_table, d_points and d_rays against the checker fed the engine's own d_x, and
    lnerf.hashgrid_autograd through torch.autograd.grad gives the same tensors."""
    import torch
    import lnerf
    import scene
    R, F, res, lt = hw.E2E
    w = hw.build(hw.hashable(hw.E2E))
    g = w["grid"]
    n, S = R // hw.S, hw.S
    b = _grid_struct(g)
    assert b.width == 32
    shapes, wp, bp = scene.init_mlp(32, 4, 3, 30)
    mlp = lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2])
    rs = np.random.RandomState(5)
    table = _dev((0.5 * rs.normal(size=(g.total, F))).astype(np.float32))
    target = _dev(rs.uniform(0, 1, (n, 3)).astype(np.float32))
    rays, t = _dev(w["rays"]), _dev(w["sample_t"])
    out = scene.hashgrid_step(engine, b, table, mlp, _dev(wp), _dev(bp), rays, t, target)
    loss = float(_np(out["loss"]))
    assert np.isfinite(loss) and loss > 0
    d_x = _np(out["d_x"])
    assert np.isfinite(d_x).all() and np.abs(d_x).max() > 0
    points, _ = engine.ray_points(rays, t)
    pts = _np(points)
    # the checker on the engine's own points and d_x
    want, mag, cnt = hr.grad_table(g, pts, d_x)
    r_t = _check_table(_np(out["d_table"]), want, mag, cnt, "hashgrid_step d_table")
    dp, dp_mag, live = hr.grad_points(g, _np(table), pts, d_x)
    bar_p = hr.points_bar(g, dp, dp_mag)
    err_p = np.abs(_np(out["d_points"]).astype(np.float64) - dp)
    assert (err_p <= bar_p).all(), _ratio(err_p, bar_p)
    assert np.abs(dp).max() > 0
    # d_rays = [sum_j d_p, sum_j t_j d_p] of the checker's d_points: the d_points bar summed along the
    # ray, plus ray_points_grad's own rounding and float64 order term
    tt = w["sample_t"].astype(np.float64)
    dp3, bar3 = dp.reshape(n, S, 3), bar_p.reshape(n, S, 3)
    want_r = np.concatenate([dp3.sum(1), (tt[:, :, None] * dp3).sum(1)], 1)
    mag_r = np.concatenate([np.abs(dp3).sum(1), (tt[:, :, None] * np.abs(dp3)).sum(1)], 1)
    bar_r = (np.concatenate([bar3.sum(1), (tt[:, :, None] * bar3).sum(1)], 1) + 2.0 ** -23 * np.abs(want_r)
             + S * 2.0 ** -52 * mag_r)
    err_r = np.abs(_np(out["d_rays"]).astype(np.float64) - want_r)
    assert (err_r <= bar_r).all(), _ratio(err_r, bar_r)
    print(f"end to end: loss {loss:.6f}; worst error / bar d_table {r_t:.3f}, d_points {_ratio(err_p, bar_p):.3f}, "
          f"d_rays {_ratio(err_r, bar_r):.3f}")
    # autograd: the same encode, and one hashgrid_grad call behind torch.autograd.grad
    tab, pt = table.clone().requires_grad_(True), points.clone().requires_grad_(True)
    x = lnerf.hashgrid_autograd(engine, b, tab, pt)
    assert (_bits(_np(x)) == _bits(_np(engine.hashgrid_encode(b, table, points)))).all()
    g_t, g_p = torch.autograd.grad(x, [tab, pt], grad_outputs=out["d_x"])
    assert (_bits(_np(g_p)) == _bits(_np(out["d_points"]))).all()
    _check_table(_np(g_t), want, mag, cnt, "hashgrid_autograd d_table")
    g_only, = torch.autograd.grad(lnerf.hashgrid_autograd(engine, b, tab, points), [tab], grad_outputs=out["d_x"])
    _check_table(_np(g_only), want, mag, cnt, "hashgrid_autograd d_table alone")
