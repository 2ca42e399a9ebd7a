"""GPU tests of lnerf_hashgrid_grad under LNERF_HASHGRID_REPRODUCIBLE (include/lnerf.h): d_table as
float64 sums in a fixed order, BIT-EQUAL to the numpy checker of tests/hashgrid_ordered_ref.py (which
tests/test_hashgrid_ordered_ref.py qualifies on the CPU, and shows to be out of reach of float32 sums in
any order) on the 15 cases of tests/hashgrid_workloads.py and on the pile (768 rows at one point: eight
entries per level with 768 terms each, segments that span every block of the sort and take the sum
kernel's whole-wave path). Every output sits between two guard bands that must come back untouched.

Per case: the same bits on a second call, on a non-default stream and with d_points requested in the
same call; LNERF_ACCUMULATE | REPRODUCIBLE over a buffer of 1.25 is float32(1.25) + float32(sum) and
leaves untouched entries alone (a planted -0 included); scale == NULL is 1; d_points has the same bits
with and without the flag. Then: a NaN row reaches exactly its own entries, the atomic mode still meets
its bar, unknown flag bits and R > 2^28 are refused and write nothing, and end to end two
scene.hashgrid_step(reproducible=True) calls, two five-step training runs and hashgrid_autograd agree
bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest

import hashgrid_ordered_ref as orf
import hashgrid_ref as hr
import hashgrid_workloads as hw

pytestmark = pytest.mark.gpu

SENT = -7.25       # guard bands and not-yet-written outputs
HELD = 1.25        # what a d_table holds before an LNERF_ACCUMULATE call
BAND = 64
ACCUMULATE = 2
REPRODUCIBLE = 65536
CASES = hw.ALL + [orf.PILE]


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


def _grad(eng, b, table, points, R, d_enc, scale, flags, d_table, d_points):
    return eng.lib.lnerf_hashgrid_grad(ctypes.byref(b.struct), _p(table), _p(points), R, _p(d_enc), _p(scale), flags,
                                       _p(d_table), _p(d_points), eng._stream())


def _held(w):
    """The buffer an accumulating call adds into: 1.25 everywhere, -0 in one entry no sample touches
    (where the case leaves one free)."""
    g = w["grid"]
    held = np.full((g.total, g.features), HELD, np.float32)
    free = np.flatnonzero(w["d_table_n"] == 0)
    if len(free):
        held[free[len(free) // 2]] = -0.0
    return held


_ENGINE = None


@functools.lru_cache(maxsize=None)
def _run(case):
    """Every call the per-case tests look at, made once."""
    import lnerf
    import torch
    eng = _ENGINE
    w = orf.workload(case)
    g = w["grid"]
    R = case[0]
    b = _grid_struct(g)
    table, pts, d_enc = _dev(w["table"]), _dev(w["points"]), _dev(w["d_encoded"])
    scale = _dev(np.array([w["scale"]], np.float32))
    shape = (g.total, g.features)
    out = {}
    dt = Banded(shape)
    assert _grad(eng, b, None, pts, R, d_enc, scale, REPRODUCIBLE, dt.view, None) == 0, lnerf.last_error()
    out["d_table"] = dt.get()
    assert _grad(eng, b, None, pts, R, d_enc, scale, REPRODUCIBLE, dt.view, None) == 0, lnerf.last_error()
    out["d_table_again"] = dt.get()
    side = Banded(shape)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert _grad(eng, b, None, pts, R, d_enc, scale, REPRODUCIBLE, side.view, None) == 0, lnerf.last_error()
    stream.synchronize()
    out["d_table_stream"] = side.get()
    both_t, both_p = Banded(shape), Banded((R, 3))
    assert _grad(eng, b, table, pts, R, d_enc, scale, REPRODUCIBLE, both_t.view, both_p.view) == 0, lnerf.last_error()
    out["d_table_both"], out["d_points_both"] = both_t.get(), both_p.get()
    held = Banded(shape)
    held.view.copy_(_dev(_held(w)))
    assert _grad(eng, b, None, pts, R, d_enc, scale, ACCUMULATE | REPRODUCIBLE, held.view, None) == 0, lnerf.last_error()
    out["d_table_acc"] = held.get()
    plain = Banded(shape)
    assert _grad(eng, b, None, pts, R, d_enc, None, REPRODUCIBLE, plain.view, None) == 0, lnerf.last_error()
    out["d_table_unscaled"] = plain.get()
    only = Banded((R, 3))
    assert _grad(eng, b, table, pts, R, d_enc, scale, REPRODUCIBLE, None, only.view) == 0, lnerf.last_error()
    out["d_points_flag_only"] = only.get()
    base = Banded((R, 3))
    assert _grad(eng, b, table, pts, R, d_enc, scale, 0, None, base.view) == 0, lnerf.last_error()
    out["d_points_default"] = base.get()
    out["wrapper"] = _np(eng.hashgrid_grad(b, None, pts, d_enc, scale=scale, reproducible=True)[0])
    return out


@pytest.fixture
def run(engine):
    global _ENGINE
    _ENGINE = engine
    return _run


def _same(got, want, what):
    assert np.shape(got) == np.shape(want), (what, np.shape(got), np.shape(want))
    g, w = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    diff = np.flatnonzero(_bits(g) != _bits(w))
    assert len(diff) == 0, (what, f"{len(diff)} of {len(g)} values differ; first at {int(diff[0])}: "
                                  f"{g[diff[0]]!r} against {w[diff[0]]!r}")


@pytest.mark.parametrize("case", CASES, ids=orf.case_id)
def test_d_table_is_bit_equal_to_the_checker(run, case):
    o = run(case)
    acc, n = orf.expected(case)
    want = orf.stored(acc, n)                      # +0 where no term lands
    print(f"ordered d_table {orf.case_id(case)}: {int((n > 0).sum())} entries, terms per entry up to {int(n.max())}")
    _same(o["d_table"], want, "d_table")
    _same(o["d_table_again"], want, "d_table, second call")
    _same(o["d_table_stream"], want, "d_table on a non-default stream")
    _same(o["d_table_both"], want, "d_table with d_points in the same call")
    _same(o["wrapper"], want, "Engine.hashgrid_grad(reproducible=True)")


@pytest.mark.parametrize("case", CASES, ids=orf.case_id)
def test_accumulate_adds_once_and_skips_untouched_entries(run, case):
    o = run(case)
    acc, n = orf.expected(case)
    held = _held(orf.workload(case))
    _same(o["d_table_acc"], orf.stored(acc, n, held), "d_table under LNERF_ACCUMULATE | REPRODUCIBLE")
    if (n == 0).any():
        assert (_bits(o["d_table_acc"])[n == 0] == _bits(held)[n == 0]).all()
        assert (_bits(held)[n == 0] == 0x80000000).any()           # the planted -0 was there to keep


@pytest.mark.parametrize("case", CASES, ids=orf.case_id)
def test_a_null_scale_is_one(run, case):
    o = run(case)
    acc, n = orf.expected(case, False)
    _same(o["d_table_unscaled"], orf.stored(acc, n), "d_table without scale")


@pytest.mark.parametrize("case", CASES, ids=orf.case_id)
def test_d_points_has_the_same_bits_with_and_without_the_flag(run, case):
    o = run(case)
    _same(o["d_points_flag_only"], o["d_points_default"], "d_points, flagged call with d_table == NULL")
    _same(o["d_points_both"], o["d_points_default"], "d_points beside a flagged d_table")


@pytest.mark.parametrize("case,rows", [(hw.ALL[12], (40, hw.ROW_LO)), (hw.ALL[6], (64,)), (orf.PILE, (700,))],
                         ids=lambda v: orf.case_id(v) if len(v) >= 4 else str(v))
def test_a_nan_row_reaches_exactly_its_own_entries(engine, case, rows):
    w = orf.workload(case)
    g, R = w["grid"], case[0]
    b = _grid_struct(g)
    pts = _dev(w["points"])
    for row in rows:
        d_enc = w["d_encoded"].copy()
        d_enc[row] = np.nan
        dt = Banded((g.total, g.features))
        assert _grad(engine, b, None, pts, R, _dev(d_enc), None, REPRODUCIBLE, dt.view, None) == 0
        got = dt.get()
        mine = sorted(hr.row_entries(g, w["points"], row))
        assert len(mine) <= 8 * g.levels
        want_nan = np.zeros((g.total, g.features), bool)
        want_nan[mine] = True
        assert (np.isnan(got) == want_nan).all(), (row, np.isnan(got).sum(), want_nan.sum())
        # and every other entry holds what the checker says for this d_encoded
        acc, n = orf.grad_table_ordered(g, w["points"], d_enc, None)
        want = orf.stored(acc, n)
        assert (_bits(got)[~want_nan] == _bits(want)[~want_nan]).all()


def test_the_atomic_mode_still_meets_its_bar(engine):
    case = hw.ALL[12]
    w = hw.build(case)
    g, R = w["grid"], case[0]
    b = _grid_struct(g)
    dt = Banded((g.total, g.features))
    scale = _dev(np.array([w["scale"]], np.float32))
    assert _grad(engine, b, None, _dev(w["points"]), R, _dev(w["d_encoded"]), scale, 0, dt.view, None) == 0
    got = dt.get()
    want, mag, n = w["d_table"], w["d_table_mag"], w["d_table_n"]
    bar = hr.table_bar(want, mag, n)
    err = np.abs(got.astype(np.float64) - want)
    t = n > 0
    assert np.isfinite(got).all() and (err[t] <= bar[t]).all(), float((err[t] / bar[t]).max())
    assert (_bits(got)[~t] == 0).all()


def test_refused_calls_write_nothing(engine):
    import lnerf
    case = hw.ALL[5]                      # R 63, F 2, three levels
    w = hw.build(case)
    g, R = w["grid"], case[0]
    good = _grid_struct(g)
    table, pts, d_enc = _dev(w["table"]), _dev(w["points"]), _dev(w["d_encoded"])
    dt, dp = Banded((g.total, g.features)), Banded((R, 3))

    def untouched():
        for buf in (dt, dp):
            assert (_bits(buf.get()) == _bits(np.float32(SENT))).all()

    for flags in (REPRODUCIBLE | 1, REPRODUCIBLE | 4, REPRODUCIBLE | ACCUMULATE | 8, 2 * REPRODUCIBLE, 32768):
        assert _grad(engine, good, table, pts, R, d_enc, None, flags, dt.view, dp.view) < 0, flags
        assert lnerf.last_error() != ""
    untouched()
    # more than 2^28 rows: the count alone is refused, before anything is read
    for rows in ((1 << 28) + 1, 1 << 30):
        assert _grad(engine, good, table, pts, rows, d_enc, None, REPRODUCIBLE, dt.view, dp.view) < 0
        assert "2^28" in lnerf.last_error()
        assert _grad(engine, good, table, pts, rows, d_enc, None, REPRODUCIBLE | ACCUMULATE, dt.view, None) < 0
    untouched()
    # the other error paths are what they were
    assert _grad(engine, good, table, pts, R, d_enc, None, REPRODUCIBLE, None, None) < 0       # both outputs NULL
    assert _grad(engine, good, table, None, R, d_enc, None, REPRODUCIBLE, dt.view, dp.view) < 0
    assert _grad(engine, good, None, pts, R, d_enc, None, REPRODUCIBLE, dt.view, dp.view) < 0   # d_points needs the table
    assert _grad(engine, good, table, pts, -1, d_enc, None, REPRODUCIBLE, dt.view, dp.view) < 0
    untouched()
    assert _grad(engine, good, table, pts, 0, d_enc, None, REPRODUCIBLE, dt.view, dp.view) == 0   # R == 0: nothing
    untouched()
    with pytest.raises(ValueError):
        engine.hashgrid_grad(good, table, pts, d_enc, accumulate=True, reproducible=True)
    assert engine.hashgrid_grad_scratch(good, R) >= 192 * R


def _e2e(engine):
    import lnerf
    import scene
    R, F, res, lt = hw.E2E
    w = hw.build(hw.hashable(hw.E2E))
    g = w["grid"]
    b = _grid_struct(g)
    assert b.width == 32
    shapes, wp, bp = scene.init_mlp(32, 4, 3, 30)
    mlp = lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2])
    rs = np.random.RandomState(5)
    table = (0.5 * rs.normal(size=(g.total, F))).astype(np.float32)
    target = rs.uniform(0, 1, (R // hw.S, 3)).astype(np.float32)
    return dict(w=w, g=g, b=b, shapes=shapes, wp=wp, bp=bp, mlp=mlp, table=table, target=target)


def test_end_to_end_steps_agree_bit_for_bit(engine):
    """24 rays x 32 samples through ray_points -> encode -> train_step (32 -> 30 -> 30 -> 4) -> grad: two
    scene.hashgrid_step(reproducible=True) calls return the same bits in every tensor, d_table is the
    checker's value for the step's own points and d_x, and hashgrid_autograd(reproducible=True) returns
    the direct call's table gradient."""
    import torch
    import lnerf
    import scene
    e = _e2e(engine)
    w, g, b = e["w"], e["g"], e["b"]
    table, target = _dev(e["table"]), _dev(e["target"])
    ws, bs = _dev(e["wp"]), _dev(e["bp"])
    rays, t = _dev(w["rays"]), _dev(w["sample_t"])
    outs = [scene.hashgrid_step(engine, b, table, e["mlp"], ws, bs, rays, t, target, reproducible=True)
            for _ in range(2)]
    first = {k: _np(v).copy() for k, v in outs[0].items() if torch.is_tensor(v)}
    second = {k: _np(v).copy() for k, v in outs[1].items() if torch.is_tensor(v)}
    assert set(first) >= {"loss", "acc_color", "d_ws", "d_bs", "d_x", "d_table", "d_points", "d_rays"}
    for k in first:
        _same(second[k], first[k], f"hashgrid_step {k}, second call")
    assert np.isfinite(first["loss"]).all() and np.abs(first["d_table"]).max() > 0
    points, _ = engine.ray_points(rays, t)
    acc, n = orf.grad_table_ordered(g, _np(points), first["d_x"], None)
    _same(first["d_table"], orf.stored(acc, n), "hashgrid_step d_table against the checker")
    # autograd: one flagged hashgrid_grad call behind torch.autograd.grad
    tab, pt = table.clone().requires_grad_(True), points.clone().requires_grad_(True)
    x = lnerf.hashgrid_autograd(engine, b, tab, pt, reproducible=True)
    g_t, g_p = torch.autograd.grad(x, [tab, pt], grad_outputs=outs[0]["d_x"])
    _same(_np(g_t), first["d_table"], "hashgrid_autograd d_table")
    _same(_np(g_p), first["d_points"], "hashgrid_autograd d_points")
    g_only, = torch.autograd.grad(lnerf.hashgrid_autograd(engine, b, tab, points, reproducible=True), [tab],
                                  grad_outputs=outs[0]["d_x"])
    _same(_np(g_only), first["d_table"], "hashgrid_autograd d_table alone")


def test_two_training_runs_agree_bit_for_bit(engine):
    """Five steps of table + MLP training (Engine.adam_update on both) from the same seeds, twice in one
    process: identical tables, weights and losses."""
    import torch
    import scene
    e = _e2e(engine)
    w, b, mlp = e["w"], e["b"], e["mlp"]
    rays, t, target = _dev(w["rays"]), _dev(w["sample_t"]), _dev(e["target"])
    nW = e["wp"].size

    def train():
        table = _dev(e["table"]).clone()
        params = _dev(np.concatenate([e["wp"].ravel(), e["bp"].ravel()])).clone()
        ws, bs = params[:nW].view(e["wp"].shape), params[nW:].view(e["bp"].shape)
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        mt, vt = torch.zeros_like(table), torch.zeros_like(table)
        grads = engine.alloc_grads(len(e["shapes"]), e["wp"].shape[1], e["wp"].shape[2])
        losses = []
        for it in range(1, 6):
            out = scene.hashgrid_step(engine, b, table, mlp, ws, bs, rays, t, target, grads=grads,
                                      want_d_rays=False, reproducible=True)
            losses.append(_np(out["loss"]).copy())
            engine.adam_update(params, grads[0][:-1], m, v, it, 5e-4)
            engine.adam_update(table.view(-1), out["d_table"].view(-1), mt, vt, it, 1e-2)
        return _np(table).copy(), _np(params).copy(), np.concatenate([l.ravel() for l in losses])

    a, c = train(), train()
    assert np.isfinite(a[2]).all() and (_bits(a[0]) != _bits(e["table"])).any()
    for x, y, what in zip(a, c, ("table", "weights", "losses")):
        _same(y, x, f"second training run, {what}")
    print(f"five reproducible steps: losses {a[2].tolist()}")
