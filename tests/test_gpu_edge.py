"""Edge numerics of the reference path on every kernel pair, against the
loma-order fp32 C oracle's own values (tests/golden/edge_*.npz, made by make_golden.py):

  sigma exactly 0, tiny sigma with the trailing delta = 1e8 (dsigma ~ 1e8 g_alpha), alpha -> 1
  with the inclusive transmittance running through fp32 subnormals into 0, saturated sigmoids,
  and an rgb pre-activation below -88.7 whose loma sigmoid adjoint is NaN
  (scripts/nerf.py:157-165,200-232; train_nerf.py:306-311,486-489).

Checks: the NaN pattern of every output equals the oracle's; finite values agree per element
within 1e-5 of |want| plus 1e-5 of the largest |want| in the same ray (per-ray outputs) or the
same dW/dB column (the dsigma ~ 1e8 column would otherwise swamp the others); subnormal outputs
stay subnormal and nonzero where the oracle's are.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PRECS = {"fp16x3": 0, "bf16x6": 512, "generic": 8}
# fp16x3 dW per element: |err| <= 1e-5 |want| + 1e-4 x the column's own max (the bar of
# test_gpu_native.py::test_full_size_all_rays_float64), with no a-priori-bound term (VERDICT r5 item
# 1). Of edge_finite_6x8's two columns that round 5's fp16x3 lost, round 6 fixed the one k2 lost (a
# column made only of rows whose products sit 2^30 .. 2^110 below the layer's largest, pushed into
# fp16's subnormals by k2's balanced split: those rows are multiplied on the bf16x6 split now,
# lnerf_internal.h kXrowD0). The other (layers 0-1, column 6, ~0.3-0.7 %) is made of G elements
# 2^28 .. 2^42 below their own row's maximum (an rgb adjoint beside a 1e6 sigma adjoint, carried
# through the fixture's permutation weights): k1's reverse chain splits each G row at that row's
# shift, so the smallest of them fall below fp16's last subnormal and are gone before k2 sees them.
# The floor guard (lnerf_internal.h kGuardExp) finds them in k1 and re-runs the step on the bf16x6
# split on the device; this fixture's step is therefore bf16x6's, bit for bit.
F16X3_COL_TOL = 1e-4


def load(name):
    return dict(np.load(os.path.join(HERE, "golden", name), allow_pickle=False))


def run(engine, g, flags):
    import lnerf
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    mlp = lnerf.make_mlp(shapes, g["wp"].shape[1], g["wp"].shape[2])
    r = engine.train_step(mlp, d(g["wp"]), d(g["bp"]), d(g["X"]), d(g["dists"]), d(g["target"]),
                          samples=int(g["S"]), input_mode=lnerf.INPUT_ENCODED, seed=1.0,
                          want_per_ray=True, want_dx=flags != lnerf.GENERIC,
                          flags=flags | (0 if flags == lnerf.GENERIC else lnerf.FAST))
    torch.cuda.synchronize()
    out = dict(loss=float(r.loss.item()), acc=r.acc_color.cpu().numpy(), dW=r.d_ws.cpu().numpy(),
               dB=r.d_bs.cpu().numpy(), d_dists=r.d_dists.cpu().numpy(),
               d_target=r.d_target.cpu().numpy())
    if r.d_x is not None:
        out["dX"] = r.d_x.cpu().numpy()
    return out, engine.last_path()


def close_grouped(name, got, want, rtol=1e-5, gtol=1e-5):
    """NaN patterns equal; finite |got - want| <= rtol |want| + gtol max|want| over axis 1 (per
    ray / sample row for per-ray outputs, per layer and column for dW, per layer for dB)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, name
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{name}: NaN pattern differs ({gn.sum()} vs {wn.sum()} NaNs)"
    a = np.where(wn, 0.0, np.abs(want))
    gmax = a.max(axis=1, keepdims=True)
    err = np.abs(np.where(wn, 0.0, got - want))
    bad = err > rtol * a + gtol * gmax
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err, -1)), err.shape)
        raise AssertionError(f"{name}: {bad.sum()} mismatches, worst at {i}: got {got[i]!r} want {want[i]!r}")


def dw_over_bar(got, want, shapes, check=True):
    """dW per element against the plain column bar, |err| <= 1e-5 |want| + F16X3_COL_TOL x the
    column's own max |want|, with no a-priori term: the NaN patterns are equal and (check) every
    finite element is inside the bar. Returns the worst error over its bar."""
    worst = 0.0
    for l, (k, n) in enumerate(tuple(int(v) for v in s) for s in shapes):
        w = np.asarray(want[l, :k, :n], np.float64)
        fin = ~np.isnan(w)
        assert np.array_equal(np.isnan(got[l, :k, :n]), ~fin), l
        w = np.where(fin, w, 0.0)
        err = np.abs(np.where(fin, got[l, :k, :n] - w, 0.0))
        cm = np.abs(w).max(axis=0, keepdims=True)
        lim = 1e-5 * np.abs(w) + F16X3_COL_TOL * cm
        over = float((err / np.maximum(lim, 1e-300)).max())
        if check:
            assert (err <= lim).all(), (l, over)
        worst = max(worst, over)
    return worst


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("name", ["edge_finite_6x8.npz", "edge_nan_3x8.npz"])
def test_edge_numerics(engine, name, prec):
    g = load(name)
    got, path = run(engine, g, PRECS[prec])
    if prec in ("fp16x3", "bf16x6"):
        assert path["k16"] and path["dw16"] and path["planes"] == (2 if prec == "fp16x3" else 3), path
    want_nan = "nan" in name
    assert np.isnan(g["dW"]).any() == want_nan
    assert abs(got["loss"] - g["loss"]) <= 1e-6 * abs(g["loss"])
    close_grouped("acc", got["acc"], g["acc"])
    close_grouped("d_target", got["d_target"], g["d_target"])
    close_grouped("d_dists", got["d_dists"], g["d_dists"])
    if prec == "fp16x3":
        # the default precision: per element against the column bar, no a-priori term
        fired = engine.guard_fired()
        assert fired == 1, fired   # both fixtures hold rgb adjoints ~2^40 below a sigma adjoint (delta = 1e8)
        worst = dw_over_bar(got["dW"], g["dW"], g["shapes"])
        print(f"{name} fp16x3 default: guard fired {fired}, worst dW error / column bar {worst:.3g}, "
              f"exceptional rows {engine.exceptional_rows()}")
        if fired:
            # the re-run is the bf16x6 step itself: every output equals an explicit LNERF_MFMA_BF16X6 step's
            ref, _ = run(engine, g, PRECS["bf16x6"])
            for key in ("dW", "dB", "acc", "d_dists", "d_target", "dX"):
                assert np.array_equal(got[key], ref[key], equal_nan=True), key
            assert got["loss"] == ref["loss"]
    else:
        close_grouped("dW", got["dW"], g["dW"])
    close_grouped("dB", got["dB"], g["dB"])
    if "dX" in got:
        close_grouped("dX", got["dX"], g["dX"])
    # subnormal outputs (transmittance underflow) stay nonzero subnormals of the same sign
    sub = (np.abs(g["d_dists"]) > 0) & (np.abs(g["d_dists"]) < np.finfo(np.float32).tiny)
    if not want_nan:
        assert sub.any()
    assert (np.sign(got["d_dists"][sub]) == np.sign(g["d_dists"][sub])).all()


def test_floor_guard_only_under_the_default_precision(engine):
    """The floor guard (lnerf_internal.h kGuardExp) belongs to the default precision: an explicit
    LNERF_MFMA_F16X3 runs fp16x3 exactly (no re-run; lnerf_ctx_guard_fired reports -1) and so do the
    other explicit precisions and the generic path; the default on the same fixture fires it."""
    import lnerf
    g = load("edge_finite_6x8.npz")
    for flags in (lnerf.MFMA_F16X3, lnerf.MFMA_BF16X6, lnerf.GENERIC):
        run(engine, g, flags)
        assert engine.guard_fired() == -1, flags
    run(engine, g, 0)
    assert engine.guard_fired() == 1


BAND_PRECS = {"default": 0, "bf16x6": 512, "generic": 8, "fp16x3 explicit": 256}


@pytest.fixture(scope="module")
def band_runs(engine):
    """edge_band_4x8 once under each precision: prec -> (outputs, path, guard state, exceptional rows)."""
    import lnerf
    assert BAND_PRECS == {"default": 0, "bf16x6": lnerf.MFMA_BF16X6, "generic": lnerf.GENERIC,
                          "fp16x3 explicit": lnerf.MFMA_F16X3}
    g = load("edge_band_4x8.npz")
    runs = {}
    for prec, flags in BAND_PRECS.items():
        got, path = run(engine, g, flags)
        runs[prec] = (got, path, engine.guard_fired(), engine.exceptional_rows() if prec != "generic" else None)
    return g, runs


@pytest.mark.parametrize("prec", list(BAND_PRECS))
def test_band_below_row_max_default_precision(band_runs, prec):
    """The band between fp16x3's full precision and the floor guard's floor (oracle/edge_band.py,
    edge_band_4x8.npz): every rgb adjoint of every head G row sits 2^31.7 .. 2^35.2 below its row's
    sigma adjoint -- in fp16's subnormals after k1's row shift (a few bits in hi, nothing in lo), above
    the floor (2^-37.5 of the row maximum) -- and the identity weights carry them into dW columns of
    their own (layers 0-1, columns 0-2 and 4-6). A plain fp16x3 split of the head row puts those columns
    0.3 % .. 1.7 % away from float64 (CPU emulation, 32 .. 165 bars; the generator asserts >= 10).
    Under every precision the path, loss, acc, d_target, d_dists, dB and dX are checked as
    test_edge_numerics checks them; bf16x6 and the generic path also meet the plain dW column bar
    (0.0057 bar, one fp32 ulp of the oracle's value). The default's dW bar is the separate
    test_band_dw_column_bar_default_precision. While the guard stays silent the default step is the
    fp16x3 step itself (the re-run's kernels exit at once), so its dW equals the explicit
    LNERF_MFMA_F16X3 run's bit for bit; that run is fp16x3 exactly, and its error is the measured
    size of the hole, printed and not asserted."""
    g, runs = band_runs
    got, path, fired, xrows = runs[prec]
    if prec in ("default", "fp16x3 explicit", "bf16x6"):
        assert path["k16"] and path["dw16"] and path["planes"] == (3 if prec == "bf16x6" else 2), path
    worst = dw_over_bar(got["dW"], g["dW"], g["shapes"], check=False)
    print(f"edge_band_4x8 {prec}: guard {fired}, exceptional rows {xrows}, worst dW error / column bar {worst:.3g}")
    assert fired == -1 if prec != "default" else fired in (0, 1), fired
    assert abs(got["loss"] - g["loss"]) <= 1e-6 * abs(g["loss"])
    close_grouped("acc", got["acc"], g["acc"])
    close_grouped("d_target", got["d_target"], g["d_target"])
    close_grouped("d_dists", got["d_dists"], g["d_dists"])
    close_grouped("dB", got["dB"], g["dB"])
    if "dX" in got:
        close_grouped("dX", got["dX"], g["dX"])
    if prec in ("bf16x6", "generic"):
        dw_over_bar(got["dW"], g["dW"], g["shapes"])
    if prec == "default" and fired == 0:
        for key in ("dW", "dB", "acc", "d_dists", "d_target", "dX"):
            assert np.array_equal(got[key], runs["fp16x3 explicit"][0][key], equal_nan=True), key
    if prec == "default" and fired == 1:
        for key in ("dW", "dB", "acc", "d_dists", "d_target", "dX"):
            assert np.array_equal(got[key], runs["bf16x6"][0][key], equal_nan=True), key


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=(
    "the floor guard's blind band: the default precision leaves dW_0 / dW_1 columns 0-2 and 4-6 of "
    "edge_band_4x8 up to 165 x the plain column bar from the oracle (1.7 % of the column; measured on "
    "the MI355X, bit-equal to the explicit fp16x3 run and matching the CPU emulation) with guard_fired() == 0"))
def test_band_dw_column_bar_default_precision(band_runs):
    """Nothing but the plain dW column bar on the default precision's step on edge_band_4x8 (every
    other output of that step is asserted in test_band_below_row_max_default_precision): 165 bars
    today, a strict xfail until the guard covers the band (DESIGN.md §5 has the measured candidate)."""
    g, runs = band_runs
    dw_over_bar(runs["default"][0]["dW"], g["dW"], g["shapes"])


@pytest.mark.parametrize("prec", ["fp16x3", "bf16x6"])
def test_uniform_tiny_sigma_from_small_head_weights(engine, prec):
    """The realistic route to a tiny sigma on EVERY row: small head weights (cfg2, 33 -> 30 -> 30 -> 4,
    24 rays x 16 samples; the head's sigma column scaled and its bias set so that every sigma lies in
    [4e-10, 8e-10]; oracle/edge_band.py uniform_tiny_sigma_workload). The raw head G rows span 2^30 .. 2^40, but
    the head's per-column weight shift (lnerf_k16.hip head_col_shift / head_bscale) leaves k1 a row
    spanning under 2^9 to split: every dW column of every layer meets the plain bar against float64 at
    the GPU's ReLU decisions (CPU emulation: 7e-8 of the column), and the default precision has no
    reason to leave fp16x3 (the smallest head-row element sits at 2^5 after the shift, the head
    columns' split loss at 2^-22 of their magnitude: scripts/xcheck_study.py --head), so whatever
    later widens the guard to the band must leave it silent here."""
    import edge_band
    import nerf_np
    from fused_parity import FLIP_MARGIN, encoded_input, padded, run_fused
    from loma_calls import assert_close
    w = edge_band.uniform_tiny_sigma_workload()
    got = run_fused(engine, w, seed=1.0, flags=PRECS[prec])
    fired = engine.guard_fired()
    X = encoded_input(w, True)
    sig = nerf_np.nerf_forward_backward(X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0, masks=got["masks"])["sigma"]
    assert 4e-10 <= sig.min() and sig.max() <= 8e-10, (sig.min(), sig.max())
    ref = nerf_np.nerf_forward_backward_chunked(X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0,
                                                masks=got["masks"])
    want = padded(ref["dW"], w.wp.shape)
    worst = dw_over_bar(got["dW"], want, [x.shape for x in w.ws], check=False)
    print(f"uniform tiny sigma ({prec}): guard {fired}, worst dW error / column bar {worst:.3g}")
    tol = dict(rtol=1e-5, atol_scale=1e-5)
    assert abs(got["loss"] - ref["loss"]) <= 1e-6 * ref["loss"]
    assert_close("acc", got["acc"], ref["acc"], **tol)
    assert_close("d_dists", got["d_dists"], ref["d_dists"], **tol)
    assert_close("d_target", got["d_target"], ref["d_target"], **tol)
    assert_close("dB", got["dB"], padded(ref["db"], w.bp.shape), **tol)
    assert max((float(f.max()) for f in ref["flip_margins"] if len(f)), default=0.0) <= FLIP_MARGIN
    dw_over_bar(got["dW"], want, [x.shape for x in w.ws])
    assert fired == (0 if prec == "fp16x3" else -1), fired


def test_shards_with_mixed_guard_outcomes_sum_to_the_full_batch(engine):
    """Data-parallel shards decide the guard each for itself: shard A (the rays of edge_finite_6x8)
    re-runs on bf16x6, shard B (edge_plain_4x8, the same 8 -> 8 -> 8 -> 4 MLP) stays on fp16x3. The sum
    of their gradients and the step on the concatenated batch (which re-runs as a whole) must both be
    the float64 gradient of the concatenated batch within the plain bar, and their losses agree."""
    import edge_band
    A, B = load("edge_finite_6x8.npz"), load("edge_plain_4x8.npz")
    assert np.array_equal(A["wp"], B["wp"]) and np.array_equal(A["bp"], B["bp"]) and int(A["S"]) == int(B["S"])
    cat = dict(A)
    for k in ("X", "dists", "target"):
        cat[k] = np.concatenate([A[k], B[k]])
    ga, _ = run(engine, A, 0)
    assert engine.guard_fired() == 1
    gb, _ = run(engine, B, 0)
    assert engine.guard_fired() == 0
    gc, _ = run(engine, cat, 0)
    assert engine.guard_fired() == 1
    f = edge_band.float64_of(cat)
    from fused_parity import padded
    dW, dB = padded(f["dW"], A["wp"].shape), padded(f["db"], A["bp"].shape)
    for name, w_, b_, loss in (("shard sum", ga["dW"].astype(np.float64) + gb["dW"], ga["dB"].astype(np.float64) + gb["dB"],
                                ga["loss"] + gb["loss"]), ("whole batch", gc["dW"], gc["dB"], gc["loss"])):
        print(f"{name}: worst dW error / column bar {dw_over_bar(w_, dW, A['shapes'], check=False):.3g}")
        dw_over_bar(w_, dW, A["shapes"])
        close_grouped(name + " dB", b_, dB, rtol=1e-5, gtol=F16X3_COL_TOL)
        assert abs(loss - f["loss"]) <= 1e-6 * abs(f["loss"]), name
    assert abs(ga["loss"] + gb["loss"] - gc["loss"]) <= 1e-6 * abs(gc["loss"])


@pytest.mark.parametrize("name", ["chunk_4x30.npz", "deep8_w64_2x64.npz", "trained_weights_8x16.npz"])
def test_floor_guard_silent_on_benign_fixtures(engine, name):
    """Ordinary inputs never pay the bf16x6 re-run: the three benign golden fixtures under default
    flags (test_gpu_native.py checks their values). Only chunk_4x30 and trained_weights_8x16 constrain
    a wider guard: deep8_w64_2x64 has sigma = 0 on every sample, so its G is all zero and no guard
    can fire on it. trained_weights_8x16 is the one a wider guard has
    to respect: 11 of its 128 head rows hold an element below 2^-12 after the shift (the smallest at
    2^-20, as deep as the band fixture's), but rows with well-represented elements feed the same
    columns -- its worst head column loses 2^-16.2 of its magnitude to the split, the band fixture's
    2^-5.3 (scripts/xcheck_study.py --head)."""
    g = load(name)
    run(engine, g, 0)
    assert engine.guard_fired() == 0


@pytest.mark.parametrize("prec", list(PRECS))
def test_nan_input_row_propagates(engine, prec):
    """a NaN in the encoded input (ENCODED mode, the loma layer_input) must leave dW
    non-finite exactly where the float64 restatement's is. ReLU turns the NaN pre-activations
    into 0 (nerf.py:141-144: z > 0 is false), so the loss and every other output stay finite, and
    dW_0[k, :] = X[s, k] G_0[s, :] = NaN * 0 = NaN for the NaN input features only. fp16x3 training
    keeps activation slabs as int24, which cannot hold a NaN: k1 marks the row (kSexpNonFinite) and
    k2 decodes its NaN code back to NaN."""
    import lnerf
    import nerf_np
    w = nerf_np.make_workload("cfg2", rays=24, samples=16)
    X = w.X.copy()
    X[5, 7] = np.nan
    X[200, 0] = np.nan
    shapes = [x.shape for x in w.ws]
    g = dict(X=X, wp=w.wp, bp=w.bp, dists=w.dists, target=w.target, S=w.S, shapes=np.array(shapes))
    got, path = run(engine, g, PRECS[prec])
    if prec == "fp16x3":
        assert path["a24"], path
    with np.errstate(all="ignore"):
        r = nerf_np.nerf_forward_backward(X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0)
    assert np.isfinite(r["loss"]) and np.isfinite(got["loss"])
    for l, (k, n) in enumerate(shapes):
        want = r["dW"][l]
        assert np.array_equal(np.isnan(got["dW"][l, :k, :n]), np.isnan(want)), (l, prec)
        fin = np.isfinite(want)
        scale = np.abs(np.where(fin, want, 0)).max()
        err = np.abs(np.where(fin, got["dW"][l, :k, :n] - want, 0))
        assert (err <= 1e-5 * np.abs(np.where(fin, want, 0)) + 1e-5 * scale).all(), (l, prec, float(err.max()))
    assert np.isnan(r["dW"][0][7]).all() and np.isnan(r["dW"][0][0]).all()
    close_grouped("acc", got["acc"], r["acc"])


@pytest.mark.parametrize("prec", ["fp16x3", "bf16x6"])
def test_tiny_sigma_delta_1e8_at_bench_size(engine, prec):
    """the delta = 1e8 / tiny-sigma pattern of edge_finite_6x8 injected into
    a bench-sized batch (1024 rays x 64 samples, the cfg3 MLP 33->256x7->4): the head's sigma
    column is scaled by 1e-8 and its bias centred on the median of the result, so half of the
    sigmas are 0 and the rest spread from ~1e-14 to ~1e-8. Most rays' last samples (delta = 1e8,
    train_nerf.py:306-311) land at sigma delta ~ 0.01..10, where dsigma ~ 1e8 g_alpha; every other
    positive-sigma sample has alpha ~ sigma 0.06 and an rgb gradient that small against its sigma
    gradient: the head's G rows span up to ~2^45 (CPU-measured). Two engine features carry it: the
    head's weight planes carry a shift per column (round 5, lnerf_k16.hip head_col_shift; the sigma
    weights sit ~2^-27 below the layer's largest), and under fp16x3 the rows whose products sit above
    the layer's scale -- the last samples behind the delta = 1e8 -- are multiplied on the bf16x6
    split (round 6, lnerf_internal.h kXrowD0; round 5 ran the whole head's dW on bf16x6).

    Checked, with NO a-priori-bound term:
      * against float64 at the GPU's ReLU decisions: every output within 1e-5 of its array's max;
      * fp16x3 (the default): per dW column against the loma-order fp32 evaluation of the same
        step (the generic path, itself within 1e-6 of the C oracle, test_gpu_native): within 1e-5
        of |want| + 1e-4 of the column's max. Not against float64 per column: many hidden columns here are sums of terms
        that cancel to ~1e-11 of the layer's scale, where any fp32 evaluation -- the reference's
        own loma C included -- is 4 % to 290 % away from float64 (measured: the generic path and
        both fused precisions agree with each other to 1e-5 of the column there)."""
    import lnerf
    import nerf_np
    from fused_parity import FLIP_MARGIN, encoded_input, padded, run_fused, _dev
    from loma_calls import assert_close
    import torch
    w = nerf_np.make_workload("cfg3", rays=1024)
    ws = [x.copy() for x in w.ws]
    bs = [x.copy() for x in w.bs]
    ws[-1][:, 3] *= 1e-8
    bs[-1][3] = 0.0
    sub = nerf_np.subset_rays(w, range(256))
    r0 = nerf_np.nerf_forward_backward(sub.X, ws, bs, sub.dists, sub.target, sub.S, seed=1.0)
    bs[-1][3] = np.float32(-np.median(r0["A"][-1] @ ws[-1][:, 3].astype(np.float64)))
    wp, bp = nerf_np.pad_weights(ws, bs)
    w = nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)
    got = run_fused(engine, w, seed=1.0, flags=PRECS[prec])
    X = encoded_input(w, True)
    ref = nerf_np.nerf_forward_backward_chunked(X, ws, bs, w.dists, w.target, w.S, seed=1.0,
                                                masks=got["masks"], rays_per_chunk=256)
    tol = dict(rtol=1e-5, atol_scale=1e-5)
    assert abs(got["loss"] - ref["loss"]) <= 1e-6 * ref["loss"]
    assert_close("acc", got["acc"], ref["acc"], **tol)
    assert_close("d_dists", got["d_dists"], ref["d_dists"], **tol)
    assert_close("d_target", got["d_target"], ref["d_target"], **tol)
    assert_close("dW", got["dW"], padded(ref["dW"], w.wp.shape), **tol)
    assert_close("dB", got["dB"], padded(ref["db"], w.bp.shape), **tol)
    worst = max((float(f.max()) for f in ref["flip_margins"] if len(f)), default=0.0)
    assert worst <= FLIP_MARGIN
    if prec != "fp16x3":
        return
    rows, last = engine.exceptional_rows(split=True)
    print(f"tiny-sigma batch: exceptional rows {rows} of {len(ws) * w.N * w.S} (of them last samples {last})")
    assert last > 0   # last samples whose sigma gradients put them above the layer's product scale
    # per column against the loma-order fp32 evaluation (GENERIC: the reference's operation order);
    # the default split only: bf16x6 drops a different set of tiny partial products and on the
    # cancelling columns (4 % of float64 away for every fp32 evaluation) sits up to 3e-4 of the
    # column from the loma order (measured), inside that shared fp32 error
    mlp = lnerf.make_mlp([x.shape for x in ws], wp.shape[1], wp.shape[2])
    g = engine.train_step(mlp, _dev(engine, wp), _dev(engine, bp), _dev(engine, w.pts32.reshape(-1, 3)),
                          _dev(engine, w.dists), _dev(engine, w.target), samples=w.S,
                          input_mode=lnerf.INPUT_POINTS, seed=1.0, flags=lnerf.GENERIC)
    torch.cuda.synchronize()
    gdW = g.d_ws.cpu().numpy()
    worst_col = 0.0
    for l, (k, n) in enumerate(x.shape for x in ws):
        want = gdW[l, :k, :n].astype(np.float64)
        err = np.abs(got["dW"][l, :k, :n] - want)
        cmax = np.abs(want).max(axis=0, keepdims=True)
        lim = 1e-5 * np.abs(want) + F16X3_COL_TOL * cmax
        assert (err <= lim).all(), (l, float((err / np.maximum(lim, 1e-300)).max()))
        live = cmax[0] > 0
        worst_col = max(worst_col, float((err.max(axis=0)[live] / cmax[0][live]).max(initial=0.0)))
    print(f"tiny-sigma batch ({prec}): worst per-column dW error vs the loma-order fp32 path "
          f"{worst_col:.3g} of the column max")


def test_exceptional_rows_on_the_bench_batch(engine):
    """how often the fp16x3 default multiplies a row on the bf16x6 split instead
    (lnerf_internal.h kXrowD0) on the bench's own batch (cfg3: 4096 rays x 64 samples, the cfg3 MLP,
    seed 215): never here -- every ray's last sample sits below the layer's product scale and every
    other row within kXrowD0 binades of it (CPU-emulated: 0 of 262 144 rows per layer) -- so the
    default path pays only the bitmap pass. The same count on the tiny-sigma pattern (the last
    samples' sigma gradients far above every other row) is nonzero."""
    import nerf_np
    from fused_parity import run_fused
    w = nerf_np.make_workload("cfg3")
    run_fused(engine, w, seed=1.0)
    rows, last = engine.exceptional_rows(split=True)
    total = len(w.ws) * w.N * w.S
    print(f"cfg3 bench batch: exceptional rows {rows} of {total} (of them last samples {last}), "
          f"floor guard {engine.guard_fired()}")
    assert rows <= 1e-4 * total
    assert engine.guard_fired() == 0   # the bench batch never pays the bf16x6 re-run
