"""The dW kernel's int24 decode and db sums (lnerf_dw16.hip decode_a24, db_add) on activation rows that
sit at the ends of the code range, at the smallest shape of test_gpu_dw_pipeline.py: MLP 33 -> 256 ->
256 -> 4 on 20 rays x 8 samples with LNERF_OPT_DW_GRID 16 (the hidden layer runs the FULL 2 x 4 loop
on splits of 3 3 3 3 3 1 0 half-blocks).

k1 stores a hidden activation row x as 24-bit codes q = rint(x 2^(xa + 8)), xa the shift that puts the
row's maximum in [2^13, 2^14), so |q| <= 2^22 - 1; k2 reassembles float(0x4B000000 | bits) - 1.5 2^23
from three dwords per four values, each of the four by its own instruction sequence. The input is
chosen so that the layer-1 activation row of two samples is known exactly: their encoded input is the
unit vector e_0, layer 0 has no bias, and row 0 of W_0 is the pattern P below, multiples of 2^-22 in
(-1, 1) with the largest (2^22 - 1) 2^-22. Every |W_0| < 1 and P's maximum lies in [0.5, 1), so the
fp16 hi/lo split of the weights (11 + 11 bits below 2^14 after the shift) holds P exactly, 1 x P sums
exactly in fp32, and ReLU(P) is the activation row: its maximum takes xa = 14 and every value x the
code x 2^22. The row then holds

  * the largest code, 2^22 - 1 (P[0]), and its negative before the ReLU (P[1]: an exact zero after);
  * exact zeros (P[2:10]);
  * codes one apart: 2^21 - 1, 2^21, 2^21 + 1 (P[10:13]) and 1, 2 (P[13:15]);
  * random codes in every position of the four-value groups (the rest).

One sample sits inside a split's range (row 5), one is the first row of split 1 (row 48). Row 47, the
last of split 0, has a NaN in encoded input 7, as test_gpu_dw_pipeline.py::test_nan_row_at_range_ends:
the X slab carries it as k1's non-finite mark and dW_0's row 7 is NaN, nothing else.

dW and dB against the float64 restatement at the GPU's ReLU decisions, at the project's bars (dW per
element 1e-5 |want| + 1e-4 x its column's max, dB TOL64), under fp16x3 and under the default flags, and
two runs equal bit for bit."""
import numpy as np
import pytest

import nerf_np
from fused_parity import TOL64, encoded_input, padded, run_fused
from loma_calls import assert_close

pytestmark = pytest.mark.gpu

F16X3 = 256   # lnerf.MFMA_F16X3
DW_COL_TOL = 1e-4
DIMS = [33, 256, 256, 4]
RAYS, S, GRID = 20, 8, 16
PATTERN_ROWS, NAN_ROW, NAN_COL = (5, 48), 47, 7
CODE = 2.0 ** -22


def pattern():
    rng = np.random.RandomState(7)
    p = rng.randint(-(2 ** 22 - 1), 2 ** 22, size=DIMS[1]).astype(np.float64) * CODE
    p[0], p[1] = (2 ** 22 - 1) * CODE, -(2 ** 22 - 1) * CODE
    p[2:10] = 0.0
    p[10:13] = 0.5 - CODE, 0.5, 0.5 + CODE
    p[13:15] = CODE, 2 * CODE
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p) and np.abs(p).max() == p[0]
    return p32


@pytest.fixture(scope="module")
def workload():
    w = nerf_np.make_workload("cfg2", rays=RAYS, samples=S)
    assert DIMS[0] == w.X.shape[1] and w.N * w.S == 160
    rng = np.random.RandomState(13)
    ws = [(rng.randn(k, n) * np.sqrt(2.0 / k)).astype(np.float32) for k, n in zip(DIMS, DIMS[1:])]
    bs = [(rng.randn(n) * 0.5).astype(np.float32) for n in DIMS[1:]]
    ws[0] = np.clip(ws[0] * 0.5, -0.99, 0.99).astype(np.float32)
    ws[0][0] = pattern()
    bs[0][:] = 0.0
    X = np.ascontiguousarray(w.X, np.float32).copy()
    for r in PATTERN_ROWS:
        X[r] = 0.0
        X[r, 0] = 1.0
    X[NAN_ROW, NAN_COL] = np.nan
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(None, None, X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)


_REF = {}


def reference(w, masks):
    """float64 at the GPU's ReLU decisions, once (k1 takes the decisions; the flags tested here share
    them, which the assertion checks)."""
    if not _REF:
        with np.errstate(all="ignore"):
            r = nerf_np.nerf_forward_backward_chunked(encoded_input(w, False), w.ws, w.bs, w.dists, w.target, w.S,
                                                      seed=1.0, masks=masks, rays_per_chunk=256)
        _REF.update(dW=padded(r["dW"], w.wp.shape), dB=padded(r["db"], w.bp.shape), masks=[m.copy() for m in masks])
    for a, b in zip(_REF["masks"], masks):
        assert np.array_equal(a, b)
    return _REF["dW"], _REF["dB"]


def dw_inside_bar(got, want, shapes):
    """Equal NaN patterns and every finite element inside 1e-5 |want| + DW_COL_TOL x its column's max."""
    worst = 0.0
    for l, (k, n) in enumerate(shapes):
        w = np.asarray(want[l, :k, :n], np.float64)
        fin = ~np.isnan(w)
        assert np.array_equal(np.isnan(got[l, :k, :n]), ~fin), l
        w = np.where(fin, w, 0.0)
        err = np.abs(np.where(fin, got[l, :k, :n] - w, 0.0))
        lim = 1e-5 * np.abs(w) + DW_COL_TOL * np.abs(w).max(axis=0, keepdims=True)
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (l, worst)
    return worst


@pytest.mark.parametrize("flags", [F16X3, 0])
def test_codes_at_the_ends_of_the_range(engine, workload, flags):
    import lnerf
    w = workload
    shapes = [x.shape for x in w.ws]
    engine.set_option(lnerf.OPT_DW_GRID, GRID)
    try:
        a = run_fused(engine, w, points=False, seed=1.0, flags=flags)
        path = engine.last_path()
        b = run_fused(engine, w, points=False, seed=1.0, flags=flags)
    finally:
        engine.set_option(lnerf.OPT_DW_GRID, 0)
    assert path["k16"] and path["dw16"] and path["a24"], path
    for k in ("dW", "dB"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, "run to run")
    # the pattern rows' ReLU decisions are the pattern's signs: what reached the slab is ReLU(P)
    for r in PATTERN_ROWS:
        assert np.array_equal(a["masks"][0][r].astype(bool), pattern() > 0), r
    dW, dB = reference(w, a["masks"])
    # the NaN input reaches dW_0's row NAN_COL and nothing else
    nan = np.isnan(dW)
    assert nan[0, NAN_COL, :shapes[0][1]].all() and nan.sum() == shapes[0][1]
    worst = dw_inside_bar(a["dW"], dW, shapes)
    assert_close("dB", a["dB"], dB, **TOL64)
    print(f"flags {flags}: worst dW error / column bar {worst:.3g}")
