"""The call contract of the native API (include/lnerf.h), as opposed to the kernels' arithmetic:
LNERF_ACCUMULATE, NULL outputs, a render without a target, explicit streams, what one call leaves in
a context's workspace for the next, the workspace bound, and the declared limits (16 layers x 256).

Most checks compare one run of the library with another, bit for bit: the kernels sum in fixed orders,
so equal inputs give equal bits (test_full_size_seed_linearity_and_determinism relies on the same).
Two runs that are wrong in the same way would pass such a comparison, so every workload's baseline is
first anchored: fused_parity.check_fused (float64 at the GPU's own ReLU decisions, then the C oracle)
must pass, and the baseline must equal check_fused's own run bit for bit. The edge fixture is anchored
against its golden float64 results with test_gpu_edge's bars, the generic path against the C oracle.

Calls go through `raw_call`, which hands lnerf_train_step / lnerf_render exactly the pointers, flags
and stream a test names (Engine.train_step always passes every output and the current stream).
"""
import ctypes
import time

import numpy as np
import pytest

import nerf_np
from fused_parity import TOL64, check_fused
from loma_calls import assert_close
from test_gpu_edge import close_grouped, dw_over_bar, load as load_golden
from test_gpu_native import _deep, compare, oracle_ref

pytestmark = pytest.mark.gpu

OUT_KEYS = ("loss", "acc_color", "d_ws", "d_bs", "d_x", "d_dists", "d_target")
PER_RAY = ("acc_color", "d_x", "d_dists", "d_target")
# check_fused's names for the same outputs
PARITY_KEYS = dict(acc_color="acc", d_ws="dW", d_bs="dB", d_x="dX", d_dists="d_dists", d_target="d_target")
SENTINEL = np.float32(-1.2345678e30)   # no kernel output comes near it


def _t():
    import torch
    return torch


def dev(a):
    return _t().from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Job:
    """One workload on the device: the arguments of a step that do not change between its calls."""

    def __init__(self, w, *, points=False, name=""):
        import lnerf
        self.w, self.points, self.name = w, points, name
        self.shapes = [tuple(int(v) for v in x.shape) for x in w.ws]
        self.L = len(self.shapes)
        self.mlp = lnerf.make_mlp(self.shapes, w.wp.shape[1], w.wp.shape[2])
        self.rays, self.S, self.F = int(w.N), int(w.S), int(w.F)
        self.mode = lnerf.INPUT_POINTS if points else lnerf.INPUT_ENCODED
        self.host = dict(ws=np.asarray(w.wp, np.float32), bs=np.asarray(w.bp, np.float32),
                         x=np.asarray(w.pts32.reshape(-1, 3) if points else w.X, np.float32),
                         dists=np.asarray(w.dists, np.float32), target=np.asarray(w.target, np.float32))
        self.t = {k: dev(v) for k, v in self.host.items()}

    def out_shapes(self, dinput=False):
        R = self.rays * self.S
        return dict(loss=(1,), acc_color=(self.rays, 3), d_ws=tuple(self.w.wp.shape), d_bs=tuple(self.w.bp.shape),
                    d_x=tuple(self.host["x"].shape) if dinput else (R, self.shapes[0][0]),
                    d_dists=(self.rays, self.S), d_target=(self.rays, 3))

    def outs(self, fill=SENTINEL, dinput=False):
        torch = _t()
        return {k: torch.full(s, float(fill), dtype=torch.float32, device="cuda:0")
                for k, s in self.out_shapes(dinput).items()}


def golden_workload(g):
    """A committed fixture (tests/golden/*.npz: ENCODED rows, padded weights) as a Workload."""
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    ws = [np.asarray(g["wp"][l, :k, :n], np.float32) for l, (k, n) in enumerate(shapes)]
    bs = [np.asarray(g["bp"][l, :n], np.float32) for l, (_, n) in enumerate(shapes)]
    S = int(g["S"])
    N = g["target"].shape[0]
    return nerf_np.Workload(None, None, np.asarray(g["X"], np.float32), np.asarray(g["dists"], np.float32),
                            np.asarray(g["target"], np.float32), ws, bs, np.asarray(g["wp"], np.float32),
                            np.asarray(g["bp"], np.float32), 0, S, N)


def raw_call(eng, job, *, flags=0, seed=1.0, outs=None, null_out=False, stream=None, render=False,
             tensors=None, target="given"):
    """lnerf_train_step / lnerf_render with exactly these arguments. `outs` maps output names to device
    tensors; a name that is missing or None goes in as NULL, null_out passes NULL for the struct itself.
    `stream` is a torch stream (None: the NULL stream, torch's default). `tensors` replaces the job's
    device inputs, target=None passes a NULL target. Returns the call's return code."""
    import lnerf
    t = tensors or job.t
    ptr = lambda v: None if v is None else v.data_ptr()
    b = lnerf.LnerfBatch(job.rays, job.S, job.mode, job.F, ptr(t["x"]), ptr(t["dists"]),
                         ptr(t["target"]) if target == "given" else None, 2.0, 6.0)
    outs = outs or {}
    o = lnerf.LnerfOutputs(*[ptr(outs.get(k)) for k in OUT_KEYS])
    op = None if null_out else ctypes.byref(o)
    s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    if render:
        return eng.lib.lnerf_render(eng.ctx, ctypes.byref(job.mlp), ptr(t["ws"]), ptr(t["bs"]), ctypes.byref(b),
                                    flags, op, s)
    return eng.lib.lnerf_train_step(eng.ctx, ctypes.byref(job.mlp), ptr(t["ws"]), ptr(t["bs"]), ctypes.byref(b),
                                    float(seed), flags, op, s)


def fetch(outs):
    _t().cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items() if v is not None}


def run_all(eng, job, flags, seed=1.0, dinput=False, **kw):
    """A step with every output passed in; returns them as numpy arrays."""
    import lnerf
    outs = job.outs(dinput=dinput)
    if flags & lnerf.SEED_LOSS:
        seed = 1.0
    rc = raw_call(eng, job, flags=flags, seed=seed, outs=outs, **kw)
    assert rc == 0, lnerf.last_error()
    return fetch(outs)


def anchored_baseline(engine, job, prec, seed_loss, c_oracle=True):
    """The baseline of (job, precision, seed kind): every output, LNERF_WANT_DX on ENCODED input.
    check_fused passes on the workload and the raw call's bits are those of check_fused's own run.
    c_oracle=False: float64 only (the loma-order fp32 oracle takes seconds on 4096 rows of cfg3)."""
    import lnerf
    got, _ = check_fused(engine, job.w, points=job.points, seed=None if seed_loss else 1.0, flags=prec,
                         want_dx=not job.points, c_oracle=c_oracle)
    flags = prec | (lnerf.SEED_LOSS if seed_loss else 0) | (0 if job.points else lnerf.WANT_DX)
    base = run_all(engine, job, flags)
    assert bits(base["loss"])[0] == bits(np.float32(got["loss"]))
    for k, pk in PARITY_KEYS.items():
        if pk in got:
            assert same_bits(base[k], got[pk]), (job.name, prec, k)
    return base, flags


# ---------------------------------------------------------------------------------------------------
# 1. LNERF_ACCUMULATE
# ---------------------------------------------------------------------------------------------------

def _pattern(g, seed):
    """A prefill for an adjoint buffer: mixed signs, magnitudes within 2^+-3 of the gradient's own mean
    magnitude, no zeros, the padded entries included."""
    rng = np.random.RandomState(seed)
    live = np.abs(g[g != 0])
    m = float(live.mean()) if live.size else 1.0
    p = m * np.exp2(rng.uniform(-3.0, 3.0, g.shape)) * rng.choice([-1.0, 1.0], g.shape)
    p = p.astype(np.float32)
    assert (p != 0).all() and np.isfinite(p).all()
    return p


def _real_masks(job):
    mw = np.zeros(job.w.wp.shape, bool)
    mb = np.zeros(job.w.bp.shape, bool)
    for l, (k, n) in enumerate(job.shapes):
        mw[l, :k, :n] = True
        mb[l, :n] = True
    return dict(d_ws=mw, d_bs=mb)


def _check_add(name, got, before, g, exact):
    """got = before + g from one fp32 add: bit for bit (exact), or, where the seed product v * loss may
    be fused into the add, within 2^-23 (|before| + |g|) of the float64 sum -- the add's own rounding
    (2^-24 |before + g|) plus one rounding of the product more or less (2^-24 |g|): derived, not measured."""
    if exact:
        want = np.float32(before) + np.float32(g)
        assert same_bits(got, want), f"{name}: {(bits(got) != bits(want)).sum()} elements differ from fl(P + g)"
        return
    s = before.astype(np.float64) + g.astype(np.float64)
    err = np.abs(got.astype(np.float64) - s)
    lim = 2.0 ** -23 * (np.abs(before.astype(np.float64)) + np.abs(g.astype(np.float64)))
    assert (err <= lim).all(), f"{name}: worst error / bound {(err / np.maximum(lim, 1e-300)).max():.3g}"


def _accumulate_checks(engine, job, prec, guard_want):
    import lnerf
    real = _real_masks(job)
    for seed_loss in (False, True):
        if job.name == "edge":
            base, flags = _edge_baseline(engine, job, prec, seed_loss)
        else:
            base, flags = anchored_baseline(engine, job, prec, seed_loss)
        assert engine.guard_fired() == guard_want
        # without the flag the padded entries are written +0.0
        for k in ("d_ws", "d_bs"):
            assert (bits(base[k])[~real[k]] == 0).all(), k
            assert np.abs(base[k][real[k]]).max() > 0, k
        P = {k: _pattern(base[k], 11 + i) for i, k in enumerate(("d_ws", "d_bs"))}
        outs = job.outs()
        for k in P:
            outs[k].copy_(dev(P[k]))
        assert raw_call(engine, job, flags=flags | lnerf.ACCUMULATE, outs=outs) == 0, lnerf.last_error()
        one = fetch(outs)
        # (added once also where the step ran twice: g is the guarded, non-accumulating step's)
        assert engine.guard_fired() == guard_want
        for k in P:
            assert same_bits(one[k][~real[k]], P[k][~real[k]]), f"{k}: padded entries moved"
            _check_add(f"{job.name} {prec} {k}", one[k][real[k]], P[k][real[k]], base[k][real[k]], not seed_loss)
        for k in ("loss", "acc_color", "d_dists", "d_target", "d_x"):
            assert same_bits(one[k], base[k]), k
        # a second accumulating step on top: P + g + g, the same bound per add
        assert raw_call(engine, job, flags=flags | lnerf.ACCUMULATE, outs=outs) == 0, lnerf.last_error()
        two = fetch(outs)
        for k in P:
            assert same_bits(two[k][~real[k]], P[k][~real[k]]), f"{k}: padded entries moved"
            _check_add(f"{job.name} {prec} {k} twice", two[k][real[k]], one[k][real[k]], base[k][real[k]],
                       not seed_loss)


def _edge_baseline(engine, job, prec, seed_loss):
    """edge_finite_6x8 against its golden float64 results (seed 1.0) with test_gpu_edge's bars; the
    loss-seeded run against the same gradients times the loss (linear in the seed)."""
    import lnerf
    g = job.golden
    flags = prec | lnerf.WANT_DX | (lnerf.SEED_LOSS if seed_loss else 0)
    base = run_all(engine, job, flags)
    sc = float(g["loss"]) if seed_loss else 1.0
    assert abs(float(base["loss"][0]) - g["loss"]) <= 1e-6 * abs(g["loss"])
    close_grouped("acc", base["acc_color"], g["acc"])
    close_grouped("d_target", base["d_target"], g["d_target"] * sc)
    close_grouped("d_dists", base["d_dists"], g["d_dists"] * sc)
    close_grouped("dX", base["d_x"], g["dX"] * sc)
    close_grouped("dB", base["d_bs"], g["dB"] * sc)
    if prec == 0:
        dw_over_bar(base["d_ws"], g["dW"] * sc, g["shapes"])
    else:
        close_grouped("dW", base["d_ws"], g["dW"] * sc)
    return base, flags


@pytest.fixture(scope="module")
def nonuniform_job():
    # (test_gpu_native's _nonuniform weights leave sigma = 0 on all of these 5 rays -- every gradient zero;
    # this seed has sigma > 0 on 99 % of the samples)
    return Job(_mlp_workload([33, 128, 256, 64, 100, 4], 5, 30, 6, pad=(256, 256)), name="nonuniform")


@pytest.fixture(scope="module")
def edge_job():
    g = load_golden("edge_finite_6x8.npz")
    j = Job(golden_workload(g), name="edge")
    j.golden = g
    return j


@pytest.mark.parametrize("prec", [0, 512, 4096])
def test_accumulate_nonuniform(engine, nonuniform_job, prec):
    """[33,128,256,64,100,4] in a 256 x 256 padded layout, 5 rays x 30 samples; default, bf16x6, K16_W4."""
    _accumulate_checks(engine, nonuniform_job, prec, 0 if prec == 0 else -1)


@pytest.mark.parametrize("prec", [0, 512])
def test_accumulate_guard_fired_fixture(engine, edge_job, prec):
    """edge_finite_6x8: under the default precision the floor guard fires and the step runs twice on the
    device; the gradient is added once. (K16_W4 has no guard and runs this fixture as plain fp16x3, which
    misses the fixture's bars by design -- test_gpu_edge -- so it has no anchored baseline here.)"""
    _accumulate_checks(engine, edge_job, prec, 1 if prec == 0 else -1)


def test_accumulate_is_rejected_on_the_generic_path(engine, nonuniform_job):
    import lnerf
    job = nonuniform_job
    outs = job.outs()
    P = {k: _pattern(np.ones(job.out_shapes()[k], np.float32), 5 + i) for i, k in enumerate(("d_ws", "d_bs"))}
    for k in P:
        outs[k].copy_(dev(P[k]))
    rc = raw_call(engine, job, flags=lnerf.GENERIC | lnerf.ACCUMULATE | lnerf.WANT_DX, outs=outs)
    assert rc < 0
    assert "LNERF_ACCUMULATE" in lnerf.last_error()
    got = fetch(outs)
    for k in OUT_KEYS:
        want = P[k] if k in P else np.full(job.out_shapes()[k], SENTINEL, np.float32)
        assert same_bits(got[k], want), k


# ---------------------------------------------------------------------------------------------------
# 2. NULL outputs
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cfg2_job():
    return Job(nerf_np.make_workload("cfg2", rays=5, samples=30), name="cfg2")


@pytest.fixture(scope="module")
def cfg2_points_job():
    return Job(nerf_np.make_workload("cfg2", rays=5, samples=30), points=True, name="cfg2 points")


def _null_case(engine, job, base, flags, null, *, null_out=False, dinput=False, what=""):
    """The step with the outputs in `null` passed as NULL: rc 0, every output asked for has the
    baseline's bits, every buffer not passed in still holds its sentinel."""
    import lnerf
    outs = job.outs(dinput=dinput)
    passed = {} if null_out else {k: v for k, v in outs.items() if k not in null}
    rc = raw_call(engine, job, flags=flags, outs=passed, null_out=null_out)
    assert rc == 0, (what, lnerf.last_error())
    got = fetch(outs)
    for k in OUT_KEYS:
        if k in passed:
            assert same_bits(got[k], base[k]), f"{what}: {k} differs from the baseline"
        else:
            assert (bits(got[k]) == bits(SENTINEL)).all(), f"{what}: {k} was written"


@pytest.mark.parametrize("seed_loss", [False, True])
def test_null_outputs_fused(engine, cfg2_job, cfg2_points_job, seed_loss):
    import lnerf
    job = cfg2_job
    base, flags = anchored_baseline(engine, job, 0, seed_loss)
    assert flags & lnerf.WANT_DX
    _null_case(engine, job, base, flags, set(OUT_KEYS), null_out=True, what="out == NULL")
    for k in OUT_KEYS:   # (d_x alone: LNERF_WANT_DX with a NULL d_x, k1 skips layer 0's backward pass)
        _null_case(engine, job, base, flags, {k}, what=f"{k} NULL")
    _null_case(engine, job, base, flags, set(PER_RAY), what="per-ray outputs NULL")
    _null_case(engine, job, base, flags, {"d_ws"}, what="d_ws NULL, d_bs set")
    _null_case(engine, job, base, flags, {"d_bs"}, what="d_bs NULL, d_ws set")
    _null_case(engine, job, base, flags, set(OUT_KEYS), what="every pointer NULL")
    # a d_x that was not asked for (no LNERF_WANT_DX) is not written either
    outs = job.outs()
    assert raw_call(engine, job, flags=flags & ~lnerf.WANT_DX, outs=outs) == 0
    got = fetch(outs)
    assert (bits(got["d_x"]) == bits(SENTINEL)).all()
    for k in OUT_KEYS:
        assert k == "d_x" or same_bits(got[k], base[k]), k
    # POINTS input with LNERF_WANT_DINPUT
    pj = cfg2_points_job
    pbase, pflags = anchored_baseline(engine, pj, 0, seed_loss)
    dflags = pflags | lnerf.WANT_DINPUT
    dbase = run_all(engine, pj, dflags, dinput=True)
    for k in OUT_KEYS:   # asking for the input gradient moves no other output
        assert k == "d_x" or same_bits(dbase[k], pbase[k]), k
    assert np.isfinite(dbase["d_x"]).all() and np.abs(dbase["d_x"]).max() > 0
    _null_case(engine, pj, dbase, dflags, {"d_x"}, dinput=True, what="WANT_DINPUT, d_x NULL")
    _null_case(engine, pj, dbase, dflags, {"d_ws", "d_bs"}, dinput=True, what="WANT_DINPUT, d_ws and d_bs NULL")


def test_null_outputs_generic(engine, cfg2_job):
    import lnerf
    job = cfg2_job
    for seed_loss in (False, True):
        flags = lnerf.GENERIC | lnerf.WANT_DX | (lnerf.SEED_LOSS if seed_loss else 0)
        base = run_all(engine, job, flags)
        assert engine.last_path()["generic"]
        want = oracle_ref(job.w, points=False, seed=None if seed_loss else 1.0, dX=True)
        got = dict(loss=float(base["loss"][0]), acc=base["acc_color"], dW=base["d_ws"], dB=base["d_bs"],
                   d_dists=base["d_dists"], d_target=base["d_target"], dX=base["d_x"])
        compare(got, want, keys=("dW", "dB", "d_dists", "d_target", "dX"), tol=dict(rtol=2e-6, atol_scale=2e-6))
        _null_case(engine, job, base, flags, {"d_x"}, what="generic, d_x NULL")
        _null_case(engine, job, base, flags, {"acc_color"}, what="generic, acc_color NULL")
        _null_case(engine, job, base, flags, set(OUT_KEYS), null_out=True, what="generic, out == NULL")


# ---------------------------------------------------------------------------------------------------
# 3. lnerf_render needs a target
# ---------------------------------------------------------------------------------------------------

def test_render_without_target_is_an_error(engine, cfg2_job):
    import lnerf
    job = cfg2_job
    for flags in (0, lnerf.MFMA_BF16, lnerf.GENERIC):
        outs = job.outs()
        rc = raw_call(engine, job, flags=flags, outs=outs, render=True, target=None)
        assert rc < 0
        assert "target" in lnerf.last_error(), lnerf.last_error()
        got = fetch(outs)
        for k in OUT_KEYS:
            assert (bits(got[k]) == bits(SENTINEL)).all(), k
        # the next valid render on this context: the bits of a fresh context's
        outs = job.outs()
        assert raw_call(engine, job, flags=flags, outs=outs, render=True) == 0, lnerf.last_error()
        here = fetch(outs)
        fresh = lnerf.Engine(0)
        try:
            outs = job.outs()
            assert raw_call(fresh, job, flags=flags, outs=outs, render=True) == 0, lnerf.last_error()
            there = fetch(outs)
        finally:
            fresh.close()
        for k in OUT_KEYS:
            assert same_bits(here[k], there[k]), k
        assert np.isfinite(here["loss"]).all() and np.isfinite(here["acc_color"]).all()
        for k in OUT_KEYS[2:]:   # a render writes no gradient
            assert (bits(here[k]) == bits(SENTINEL)).all(), k
        # and its two outputs are optional like a step's
        for null, null_out in (({"acc_color"}, False), ({"loss"}, False), (set(OUT_KEYS), True)):
            outs = job.outs()
            passed = {} if null_out else {k: v for k, v in outs.items() if k not in null}
            assert raw_call(engine, job, flags=flags, outs=passed, null_out=null_out, render=True) == 0
            got = fetch(outs)
            for k in ("loss", "acc_color"):
                want = here[k] if k in passed else np.full(job.out_shapes()[k], SENTINEL, np.float32)
                assert same_bits(got[k], want), (flags, null, k)
    # the fused render of the default precision is the training forward (anchored there)
    base, _ = anchored_baseline(engine, job, 0, False)
    outs = job.outs()
    assert raw_call(engine, job, flags=0, outs=outs, render=True) == 0
    r = fetch(outs)
    assert same_bits(r["acc_color"], base["acc_color"]) and same_bits(r["loss"], base["loss"])


# ---------------------------------------------------------------------------------------------------
# 4. Streams
# ---------------------------------------------------------------------------------------------------

# The delay queued on the side stream ahead of the work under test: DELAY_MATMULS fp32 products of
# DELAY_N x DELAY_N matrices (plain torch), 5.7 - 6.1 ms on an MI355X. The calls under test return on the
# host in 46 - 133 us (test_side_stream_train_step_and_render's docstring), so a tenfold margin would be
# 1.3 ms; the delay is four times that because its failure mode is a false alarm (premise() fails when
# the host was held up past the delay's end), never a vacuous pass.
DELAY_N = 2048
DELAY_MATMULS = 40


class SideStream:
    """A side stream with delay work queued on it and an event recorded behind the delay. `premise()`
    asserts the delay was still running when the call under test returned on the host: only then did
    the call's device work sit behind it in a queue, and only then can a kernel, memset or copy that
    went to another stream have run early (on NaN inputs or into NaN-prefilled outputs)."""

    def __init__(self):
        torch = _t()
        self.stream = torch.cuda.Stream(device=0)
        self.a = torch.randn(DELAY_N, DELAY_N, device="cuda:0")
        self.b = torch.randn(DELAY_N, DELAY_N, device="cuda:0")
        self.c = torch.empty_like(self.a)
        torch.mm(self.a, self.b, out=self.c)   # (the BLAS library's first-call setup happens here)
        torch.cuda.synchronize()

    def delay(self):
        torch = _t()
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record(self.stream)
            for _ in range(DELAY_MATMULS):
                torch.mm(self.a, self.b, out=self.c)
            self.event = torch.cuda.Event(enable_timing=True)
            self.event.record(self.stream)

    def delay_ms(self):
        """The delay's length on the device (after a synchronise)."""
        return self.start.elapsed_time(self.event)

    def premise(self, what):
        assert not self.event.query(), (f"{what}: the delay queued ahead of it had finished when the call "
                                        "returned, so the stream order was not under test")


def _nan_like(t):
    return _t().full_like(t, float("nan"))


@pytest.fixture(scope="module")
def side():
    return SideStream()


@pytest.fixture(scope="module")
def cfg3_job():
    return Job(nerf_np.make_workload("cfg3", rays=8, samples=64), points=True, name="cfg3")


def _other_inputs(job, seed):
    """Inputs of the same shapes and different values: a step on them leaves a workspace whose stale
    contents are not this job's (a kernel that ran early would otherwise find the right partials)."""
    rng = np.random.RandomState(seed)
    t = dict(job.t)
    t["ws"] = dev((job.host["ws"] * rng.uniform(0.5, 1.5, job.host["ws"].shape)).astype(np.float32))
    t["bs"] = dev((job.host["bs"] + rng.uniform(-0.2, 0.2, job.host["bs"].shape)).astype(np.float32))
    t["target"] = dev(rng.uniform(0, 1, job.host["target"].shape).astype(np.float32))
    return t


def _on_side_stream(engine, side, job, *, flags, render, what):
    """The call on the side stream behind the delay, its inputs copied in on that stream from staging
    tensors (NaN before), its outputs NaN before; returns the outputs cloned on that stream."""
    torch = _t()
    live = {k: _nan_like(v) for k, v in job.t.items()}
    outs = job.outs(fill=float("nan"))
    side.delay()
    with torch.cuda.stream(side.stream):
        for k in live:
            live[k].copy_(job.t[k], non_blocking=True)
        t0 = time.perf_counter()
        rc = raw_call(engine, job, flags=flags, outs=outs, stream=side.stream, render=render, tensors=live)
        host_s = time.perf_counter() - t0
        side.premise(what)
        got = {k: v.clone() for k, v in outs.items()}
    assert rc == 0
    side.stream.synchronize()
    print(f"{what}: host return {host_s * 1e6:.0f} us, delay {side.delay_ms():.2f} ms")
    return {k: v.cpu().numpy() for k, v in got.items()}


def test_side_stream_train_step_and_render(engine, side, cfg3_job):
    """cfg3's MLP (33 -> 256 x 7 -> 4), 8 rays x 64 samples: the step (default flags, loss-seeded and
    constant-seeded) and the bf16 kr render on a side stream, behind delay work, with inputs that arrive
    on that stream and outputs that are NaN until the call's own kernels write them. Every output equals
    the default-stream result bit for bit.

    Measured on an MI355X (this test's own printout, one run): the step returned on the host after 92 us
    (seed = loss) and 79 us (constant seed), the render after 46 us, test_side_stream_context_free_entry_points'
    four calls together after 133 us; the delay ran 5.7 - 6.1 ms on the device, 45 to 130 times those."""
    import lnerf
    job = cfg3_job
    base, _ = anchored_baseline(engine, job, 0, True)
    for flags, render, what in ((lnerf.SEED_LOSS, False, "train step (seed = loss)"),
                                (0, False, "train step (seed 1.0)"),
                                (lnerf.MFMA_BF16, True, "kr render")):
        ref = job.outs(fill=float("nan"))
        assert raw_call(engine, job, flags=flags, outs=ref, render=render) == 0, lnerf.last_error()
        ref = fetch(ref)
        if render:
            assert engine.last_path()["kr"]
        elif flags & lnerf.SEED_LOSS:
            for k in OUT_KEYS:
                assert k == "d_x" or same_bits(ref[k], base[k]), k
        # leave another problem's partials, loss and packed weights in the workspace
        assert raw_call(engine, job, flags=flags, outs=job.outs(), render=render,
                        tensors=_other_inputs(job, 3)) == 0
        _t().cuda.synchronize()
        got = _on_side_stream(engine, side, job, flags=flags, render=render, what=what)
        written = ("loss", "acc_color") if render else tuple(k for k in OUT_KEYS if k != "d_x")
        for k in OUT_KEYS:
            if k in written:
                assert np.isfinite(ref[k]).all(), (what, k)
                assert same_bits(got[k], ref[k]), f"{what}: {k} differs from the default-stream result"
            else:
                assert np.isnan(got[k]).all(), (what, k)


def test_side_stream_context_free_entry_points(engine, side):
    """lnerf_input_grad, lnerf_pose_grad, lnerf_adam_update and lnerf_scale_by_device_scalar at the stream
    test's shape (8 rays x 64 samples, F = 5) on the side stream behind the delay: inputs copied in on
    that stream, results equal to the default stream's bit for bit."""
    import lnerf
    torch = _t()
    rng = np.random.RandomState(2)
    rays, S, F = 8, 64, 5
    w = nerf_np.make_workload("cfg3", rays=rays, samples=S)
    pts = dev(w.pts32.reshape(-1, 3))
    dE = dev(rng.standard_normal((rays * S, 3 + 6 * F)).astype(np.float32))
    scale = dev(np.array([0.37], np.float32))
    focal = 0.5 / np.tan(0.5 * 0.6911112)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]], np.float64)
    d_rays = dev(rng.standard_normal((rays, 6)).astype(np.float32))
    pixels = dev(rng.randint(0, 400 * 400, rays).astype(np.int32))
    n = rays * S * 33
    p0, g0, m0, v0 = (dev(a.astype(np.float32)) for a in
                      (rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n) * 0.1,
                       rng.uniform(0.0, 0.1, n)))

    def ops(src):
        """Each entry point on the current stream, on fresh copies of its inputs."""
        out = {}
        out["input_grad"] = engine.input_grad(src["pts"], src["dE"], samples=S, input_mode=lnerf.INPUT_POINTS,
                                              num_freqs=F, scale=src["scale"])
        out["pose_grad"] = engine.pose_grad(400, K, src["d_rays"], src["pixels"])
        engine.adam_update(src["p"], src["g"], src["m"], src["v"], 3, 5e-4)
        out["adam_p"], out["adam_m"], out["adam_v"] = src["p"], src["m"], src["v"]
        engine.scale_by_device_scalar(src["buf"], src["scale"])
        out["scaled"] = src["buf"]
        return out

    staged = dict(pts=pts, dE=dE, scale=scale, d_rays=d_rays, pixels=pixels, p=p0, g=g0, m=m0, v=v0, buf=g0)
    ref = ops({k: v.clone() for k, v in staged.items()})
    torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    # anchor: the scaling and Adam against numpy, the gradients as test_gpu_input_grad checks them
    assert np.array_equal(ref["scaled"], g0.cpu().numpy() * np.float32(0.37))
    assert np.isfinite(ref["input_grad"]).all() and np.isfinite(ref["pose_grad"]).all()

    def blank(v):
        return _nan_like(v) if v.dtype.is_floating_point else torch.full_like(v, -1)

    live = {k: blank(v) for k, v in staged.items()}
    side.delay()
    with torch.cuda.stream(side.stream):
        for k in live:
            live[k].copy_(staged[k], non_blocking=True)
        t0 = time.perf_counter()
        got = ops(live)
        host_s = time.perf_counter() - t0
        side.premise("context-free entry points")
        got = {k: v.clone() for k, v in got.items()}
    side.stream.synchronize()
    print(f"context-free entry points: host return {host_s * 1e6:.0f} us, delay {side.delay_ms():.2f} ms")
    for k in ref:
        a, b = got[k].cpu().numpy(), ref[k]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def test_two_contexts_on_two_streams(engine, cfg3_job, nonuniform_job):
    """Two contexts, each on its own side stream, three steps each, interleaved with no synchronisation in
    between: each workload's three results equal its serial result bit for bit."""
    import lnerf
    torch = _t()
    jobs = (cfg3_job, nonuniform_job)
    flags = (lnerf.SEED_LOSS, lnerf.SEED_LOSS | lnerf.WANT_DX)
    serial = []
    for job, f in zip(jobs, flags):
        base, bf = anchored_baseline(engine, job, 0, True)
        serial.append(base)
    engines = [lnerf.Engine(0), lnerf.Engine(0)]
    try:
        streams = [torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)]
        outs = [[job.outs(fill=float("nan")) for _ in range(3)] for job in jobs]
        torch.cuda.synchronize()
        for step in range(3):
            for i, job in enumerate(jobs):
                assert raw_call(engines[i], job, flags=flags[i], outs=outs[i][step], stream=streams[i]) == 0
        torch.cuda.synchronize()
        for i, job in enumerate(jobs):
            for step in range(3):
                got = {k: v.cpu().numpy() for k, v in outs[i][step].items()}
                for k in OUT_KEYS:
                    if k == "d_x" and job.points:
                        continue
                    assert same_bits(got[k], serial[i][k]), (job.name, step, k)
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------------------------------------------
# 5. Context reuse
# ---------------------------------------------------------------------------------------------------

def _state(eng):
    """What the context reports about its last call."""
    out = dict(guard=eng.guard_fired(), path=eng.last_path())
    try:
        out["xrows"] = eng.exceptional_rows(split=True)
    except RuntimeError:
        out["xrows"] = "n/a"
    return out


def test_context_reuse_sequence(engine, cfg2_job, cfg3_job, nonuniform_job, edge_job):
    """One context through a fixed sequence of calls of different shapes, MLPs, precisions and kinds:
    after each one, every output and what the context reports (guard_fired, exceptional_rows, last_path)
    equal those of the same call on a context created for that call alone. The workspace is grow-only and
    holds state each step must reset or rewrite (the guard word, xcount, wmax_part, the packed weight
    planes, the masks); a step that read what an earlier one left would differ here."""
    import lnerf
    cfg3_64 = Job(nerf_np.make_workload("cfg3", rays=64, samples=64), points=True, name="cfg3 x64")
    deep = Job(_deep(nerf_np.make_workload("cfg2", rays=32, samples=32)), points=True, name="deep")
    # anchors (on the session context): each workload at the precision it runs below
    anchored_baseline(engine, cfg3_64, 0, True, c_oracle=False)
    anchored_baseline(engine, cfg2_job, lnerf.MFMA_BF16X6, True)
    _edge_baseline(engine, edge_job, 0, False)
    anchored_baseline(engine, cfg2_job, 0, True)
    anchored_baseline(engine, nonuniform_job, lnerf.K16_W4, True)
    deep6, _ = anchored_baseline(engine, deep, lnerf.MFMA_BF16X6, True)
    deep1 = run_all(engine, deep, lnerf.SEED_LOSS | lnerf.MFMA_BF16)   # plain bf16: test_fused_deep_mlp's loose bound
    assert abs(float(deep1["loss"][0]) - float(deep6["loss"][0])) <= 2e-2 * float(deep6["loss"][0])
    assert_close("deep bf16 dW", deep1["d_ws"], deep6["d_ws"], rtol=0.0, atol_scale=5e-2)

    SL, DX = lnerf.SEED_LOSS, lnerf.WANT_DX
    train = lambda job, flags, **kw: dict(job=job, flags=flags, **kw)
    seq = [
        train(cfg3_64, SL),                                       # 1
        train(cfg2_job, SL | DX | lnerf.MFMA_BF16X6),             # 2
        train(edge_job, DX, guard=1),                             # 3: the guard fires
        train(cfg2_job, SL | DX, guard=0),                        # 4: and reports 0 again
        train(nonuniform_job, SL | DX | lnerf.K16_W4),            # 5
        train(deep, SL | lnerf.MFMA_BF16),                        # 6
        train(cfg3_64, lnerf.MFMA_BF16, render=True, kr=True),    # 7: a bf16 kr render
        train(cfg2_job, SL | DX | lnerf.GENERIC),                 # 8
        train(cfg3_64, SL, dw_grid=16),                           # 9
        train(cfg3_64, SL, dw_grid=0),
        train(cfg2_job, lnerf.K16_W4 | lnerf.MFMA_BF16X6, fails=True),   # 10: fails after the lock
        train(cfg3_64, SL),                                       # 11: the first step again
    ]

    def call(eng, c):
        job = c["job"]
        if "dw_grid" in c:
            eng.set_option(lnerf.OPT_DW_GRID, c["dw_grid"])
        outs = job.outs()
        rc = raw_call(eng, job, flags=c["flags"], outs=outs, render=c.get("render", False))
        if c.get("fails"):
            assert rc < 0
            return fetch(outs), None
        assert rc == 0, lnerf.last_error()
        return fetch(outs), _state(eng)

    ctx = lnerf.Engine(0)
    try:
        first = None
        for i, c in enumerate(seq):
            got, st = call(ctx, c)
            masks_ok = not (c.get("fails") or c.get("render") or c["flags"] & lnerf.GENERIC)
            if masks_ok:
                m = ctx.relu_masks(c["job"].L, c["job"].rays * c["job"].S)
            else:
                with pytest.raises(RuntimeError):
                    ctx.relu_masks(c["job"].L, c["job"].rays * c["job"].S)
            fresh = lnerf.Engine(0)
            try:
                want, wst = call(fresh, c)
                if masks_ok:
                    assert np.array_equal(m, fresh.relu_masks(c["job"].L, c["job"].rays * c["job"].S)), i
            finally:
                fresh.close()
            assert st == wst, (i, st, wst)
            for k in OUT_KEYS:
                assert same_bits(got[k], want[k]), f"call {i} ({c['job'].name}): {k} depends on the context's past"
            if c.get("fails"):
                for k in OUT_KEYS:
                    assert (bits(got[k]) == bits(SENTINEL)).all(), k
                continue
            if "guard" in c:
                assert st["guard"] == c["guard"], (i, st)
            if c.get("kr"):
                assert st["path"]["kr"], st
            if i == 0:
                first = got
        for k in OUT_KEYS:
            assert same_bits(got[k], first[k]), k
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------
# 6. The workspace bound
# ---------------------------------------------------------------------------------------------------

WS_WIDTHS = (1, 4, 30, 33, 100, 256)
WS_AXES = dict(L=(1, 2, 8, 16), rays=(1, 3, 129), S=(1, 7, 30, 64, 128), prec=(0, 256, 512, 128, 4096),
               dw_grid=(0, 16, 4096))


def _sweep_cases(n=30):
    """n combinations drawn (fixed seed) from the axes; together they cover every value of every axis,
    every width, and the corner 16 x 256 at 129 rays x 128 samples."""
    rng = np.random.RandomState(6)
    cases = [dict(L=16, widths=[256] * 16, rays=129, S=128, prec=512, dw_grid=4096),
             dict(L=16, widths=[256] * 16, rays=129, S=64, prec=4096, dw_grid=0),
             dict(L=1, widths=[33], rays=1, S=1, prec=0, dw_grid=16)]
    while len(cases) < n:
        c = {k: v[rng.randint(len(v))] for k, v in WS_AXES.items()}
        c["widths"] = [int(WS_WIDTHS[rng.randint(len(WS_WIDTHS))]) for _ in range(c["L"])]   # k[0], hidden ...
        cases.append(c)
    for c in cases:
        if c["prec"] == 4096 and c["S"] > 64:
            c["prec"] = 0   # LNERF_K16_W4 needs whole rays in 64 samples
    return cases


def _sweep_workload(c, seed):
    """He-scaled weights, positive hidden biases and positive, small sigma weights, so that narrow layers
    stay alive and the colours are not trivially zero."""
    rng = np.random.RandomState(seed)
    dims = list(c["widths"]) + [4]
    ws = [(rng.randn(k, n) * np.sqrt(2.0 / k)).astype(np.float32) for k, n in zip(dims, dims[1:])]
    bs = [rng.uniform(0.1, 0.6, n).astype(np.float32) for n in dims[1:]]
    ws[-1][:, 3] = np.abs(ws[-1][:, 3]) * 0.05   # sigma > 0 and moderate: every sample contributes
    wp, bp = nerf_np.pad_weights(ws, bs)
    N, S = c["rays"], c["S"]
    X = rng.uniform(-1, 1, (N * S, dims[0])).astype(np.float32)
    dists = np.full((N, S), 4.0 / max(S - 1, 1), np.float32)
    dists[:, -1] = 1e8
    target = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    return nerf_np.Workload(None, None, X, dists, target, ws, bs, wp, bp, 0, S, N)


def _forward64(w):
    """The forward half of nerf_np.nerf_forward_backward (scripts/nerf.py:1-304) in float64: the loss and
    the colours (the sweep's largest shapes would spend seconds in the reverse half it does not need)."""
    A = np.asarray(w.X, np.float64)
    for l, (W, b) in enumerate(zip(w.ws, w.bs)):
        z = A @ np.asarray(W, np.float64) + np.asarray(b, np.float64)[None, :]
        A = np.maximum(z, 0.0) if l < len(w.ws) - 1 else z
    rgb = (1.0 / (1.0 + np.exp(-A[:, :3]))).reshape(w.N, w.S, 3)
    sigma = np.maximum(A[:, 3], 0.0).reshape(w.N, w.S)
    alpha = 1.0 - np.exp(-sigma * np.asarray(w.dists, np.float64))
    T = np.cumprod((1.0 - alpha) + 1e-10, axis=1)
    T[:, 0] = 1.0
    C = ((alpha * T)[:, :, None] * rgb).sum(1)
    return dict(loss=((C - np.asarray(w.target, np.float64)) ** 2).sum(), acc=C)


def test_workspace_bound_sweep(engine):
    """Shapes x precisions x dW grids, training and rendering: every call succeeds (the library holds the
    plan's carve against the bytes it allocated before it launches anything), the split precisions'
    loss and colours agree with float64, and lnerf_workspace_bytes covers what the default-grid training
    plan laid out. (On a context of its own: the sweep moves LNERF_OPT_DW_GRID.)"""
    import lnerf
    cases = _sweep_cases()
    for axis, values in WS_AXES.items():
        assert {c[axis] for c in cases} >= set(values) - ({4096} if axis == "prec" else set()), axis
    assert {wd for c in cases for wd in c["widths"]} == set(WS_WIDTHS)
    assert any(c["prec"] == 4096 for c in cases)
    eng = lnerf.Engine(0)
    try:
        for i, c in enumerate(cases):
            job = Job(_sweep_workload(c, 100 + i), name=f"sweep {c}")
            w = job.w
            eng.set_option(lnerf.OPT_DW_GRID, c["dw_grid"])
            ref = _forward64(w)
            for render in (False, True):
                outs = job.outs()
                rc = raw_call(eng, job, flags=lnerf.FAST | c["prec"], outs=outs, render=render)
                assert rc == 0, (c, render, lnerf.last_error())
                got = fetch(outs)
                used = eng.workspace_used()
                assert used > 0
                if not render and c["dw_grid"] == 0:
                    assert eng.workspace_bytes(job.mlp, job.rays, job.S) >= used, (c, used)
                assert np.isfinite(got["loss"]).all() and np.isfinite(got["acc_color"]).all(), (c, render)
                if c["prec"] != lnerf.MFMA_BF16:
                    assert abs(float(got["loss"][0]) - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (c, render)
                    assert_close(f"acc {c}", got["acc_color"], ref["acc"], **TOL64)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------
# 7. The declared limits
# ---------------------------------------------------------------------------------------------------

def _mlp_workload(dims, rays, S, seed, pad=None):
    """cfg2's rays under an MLP of these widths, He-scaled weights as in test_gpu_native._deep (activations
    stay O(1)); pad: the padded layout's (w_k, w_n) where it is to be larger than the widest layer."""
    w = nerf_np.make_workload("cfg2", rays=rays, samples=S)
    rng = np.random.RandomState(seed)
    ws = [(rng.randn(k, n) * np.sqrt(2.0 / k)).astype(np.float32) for k, n in zip(dims, dims[1:])]
    bs = [(rng.randn(n) * 0.5).astype(np.float32) for n in dims[1:]]
    wp, bp = nerf_np.pad_weights(ws, bs)
    if pad is not None:
        wp2 = np.zeros((len(ws),) + tuple(pad), np.float32)
        bp2 = np.zeros((len(ws), pad[1]), np.float32)
        wp2[:, :wp.shape[1], :wp.shape[2]] = wp
        bp2[:, :bp.shape[1]] = bp
        wp, bp = wp2, bp2
    return nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)


@pytest.mark.parametrize("prec", [0, 512, 4096])
@pytest.mark.parametrize("dims,rays,S", [([33] + [256] * 15 + [4], 4, 16), ([33, 4], 5, 30), ([33, 1, 4], 5, 30)],
                         ids=["16x256", "head-only", "width-1"])
def test_limits_all_rays(engine, dims, rays, S, prec):
    """LNERF_MAX_LAYERS layers of the widest width together (bf16x6 with d_x: 243 of k16's 256 chunk-table
    entries), a head-only MLP (no hidden layer: lnerf_ctx_relu_masks writes nothing) and a one-feature
    hidden layer: every ray against float64 and the C oracle, ENCODED input, d_x included."""
    import lnerf
    w = _mlp_workload(dims, rays, S, 17)
    check_fused(engine, w, points=False, seed=1.0, flags=prec, want_dx=True)
    path = engine.last_path()
    assert path["k16"] and path["dw16"] and path["k16_w4"] == bool(prec & lnerf.K16_W4), path
