"""CPU conditions on the workloads of tests/tile_workloads.py (no GPU), after the pattern of
tests/test_width_workloads.py and with its thresholds: a parity test on a cell whose gradients are
dead, or whose outputs do not depend on the tile a kernel might drop, passes vacuously; and the claim
that the 25 cells reach every instantiation has to be shown, not said. The GPU tests that run these
workloads are in tests/test_gpu_tiles.py.

  * liveness      every layer's dW has a nonzero entry in >= 80 % of its columns (the head: of its
                  columns 0..3); every ray's opacity lies in (0.01, 0.99).
  * sensitivity   zeroing one output feature (weight column and bias) of a hidden layer -- the first,
                  the middle one and the last, the one a dropped last tile would lose -- moves the
                  colours, or the dW of a layer not adjacent to it, by >= 100 x the TOL64 bar and the
                  colours by >= 10 x the 3e-4 bar the bf16 render is held to.
  * no ties       the smallest |z| / T over every hidden pre-activation is >= 4e-6, twice
                  fused_parity.FLIP_MARGIN: neither the GPU nor the C oracle can legitimately decide a
                  ReLU differently from float64, so the GPU tests assert that no ray is set aside
                  (four rays leave no room to set one aside). The loma-order fp32 C oracle and float64
                  agree within TOLC and on every decision.
  * scaled cells  the ten T0 > HT cells under the down24 gains: the rescale is exact and every
                  nonzero |A|, |G|, |dW|, |db| stays in [2^-100, 2^100] (test_scale_workloads.py).
  * coverage      asserted on plan(): every ht16, every to16_b[0], kr exactly where k0 <= 64, each
                  dW block shape with all eight waves and with idle ones, both sides of both shape
                  boundaries.
Measured here: live columns >= 0.88, opacities 0.70 .. 0.90, one dropped hidden feature moves the
outputs by >= 2356 x TOL64 (HT 8, T0 16) and the colours by >= 3.03e-3 (HT 2, T0 4), smallest
|z| / T 4.12e-6 (HT 16, T0 1), the rescaled cells within [2^-52.8, 2^23.3].
"""
import functools

import numpy as np
import pytest

import nerf_np
import scale_workloads as sw
import tile_workloads as tw
import width_workloads as ww
from fused_parity import FLIP_MARGIN, TOL64, TOLC, padded
from loma_calls import assert_close

COLOUR_BAR = 3e-4     # test_gpu_render.test_kr_vs_float64_per_element's bar against the bf16 emulation
TIE = 2 * FLIP_MARGIN

cells = pytest.mark.parametrize("c", tw.CELLS, ids=tw.cell_id)


@functools.lru_cache(maxsize=None)
def _ref(c):
    w = tw.cell(*c)
    return w, nerf_np.nerf_forward_backward(w.X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0)


def test_the_cells_are_the_ones_asked_for():
    assert len(tw.CELLS) == 25 and len(tw.WIDE_INPUT_CELLS) == 10
    assert [tw.cell_dims(1, t0)[0] for t0 in tw.TILES] == [13, 29, 61, 125, 253]
    assert [tw.cell_dims(ht, 1)[1:] for ht in tw.TILES] == [[16, 9, 16, 4], [32, 17, 32, 4], [64, 33, 64, 4],
                                                            [128, 65, 128, 4], [256, 129, 256, 4]]
    for c in tw.CELLS:
        w, dims = tw.cell(*c), tw.cell_dims(*c)
        assert [x.shape for x in w.ws] == list(zip(dims, dims[1:]))
        assert (w.N, w.S, w.X.shape, w.dists.shape) == (4, 40, (160, dims[0]), (4, 40))
        p = tw.cell_plan(c)
        # three rays per 128-sample workgroup: two workgroups, the second with one ray
        assert p["rays_per_wg"] == 3 and tw.cell_plan(c, tw.K16_W4)["rays_per_wg"] == 1
    assert set(tw.SEEDS) == set(tw.CELLS)


def test_pow2_16_against_the_band_edges():
    """Which hidden widths select which HT: the top of each band and the first width past it."""
    ht = lambda hidden: tw.plan([33, hidden, hidden, 4], 40)["ht16"]
    assert [ht(n) for n in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [tw.pow2_16(t) for t in range(1, 17)] == [1, 2, 4, 4, 8, 8, 8, 8] + [16] * 8
    # three, five..seven and nine..fifteen tiles round up to the next instantiation
    assert (ht(48), ht(80), ht(112), ht(144), ht(240)) == (4, 8, 8, 16, 16)
    # the widest HIDDEN layer counts, neither the input nor the head
    assert tw.plan([253, 16, 9, 16, 4], 40)["ht16"] == 1 and tw.plan([13, 16, 16], 40)["ht16"] == 1
    assert tw.plan([13, 16, 129, 16, 4], 40)["ht16"] == 16
    for c in tw.CELLS:
        p = tw.cell_plan(c)
        assert (p["ht16"], p["to16_b0"]) == c


@cells
def test_liveness(c):
    w, r = _ref(c)
    L = len(w.ws)
    lives = []
    for l, dW in enumerate(r["dW"]):
        cols = dW[:, :4] if l == L - 1 else dW
        lives.append(float((np.abs(cols) > 0).any(axis=0).mean()))
        assert lives[-1] >= 0.8, (l, lives[-1])
    opacity = r["weights"].sum(axis=1)
    print(f"{tw.cell_id(c)}: live columns >= {min(lives):.3g}, opacity {opacity.min():.3g} .. {opacity.max():.3g}")
    assert (opacity < 0.99).all() and (opacity > 0.01).all(), (opacity.min(), opacity.max())


def probed_features(n):
    return sorted({0, n // 2, n - 1})


@cells
def test_one_dropped_hidden_feature_shows(c):
    w, r = _ref(c)
    L = len(w.ws)
    worst_v, worst_c = np.inf, np.inf
    for l in range(L - 1):
        for f in probed_features(w.ws[l].shape[1]):
            ws, bs = [x.copy() for x in w.ws], [x.copy() for x in w.bs]
            ws[l][:, f] = 0.0
            bs[l][f] = 0.0
            r2 = nerf_np.nerf_forward_backward(w.X, ws, bs, w.dists, w.target, w.S, seed=1.0)
            # (dW[l]'s column f and dW[l + 1]'s row f are zero by construction: the adjacent layers are left out)
            v = max([ww.violation(r2["acc"], r["acc"], **TOL64)] +
                    [ww.violation(r2["dW"][m], r["dW"][m], **TOL64) for m in range(L) if m not in (l, l + 1)])
            col = float(np.abs(r2["acc"] - r["acc"]).max())
            worst_v, worst_c = min(worst_v, v), min(worst_c, col)
            assert v >= 100.0, (l, f, v)
            assert col >= 10 * COLOUR_BAR, (l, f, col)
    print(f"{tw.cell_id(c)}: one dropped hidden feature moves the outputs by >= {worst_v:.0f} x TOL64, "
          f"the colours by >= {worst_c:.3g}")


@cells
def test_no_relu_decision_is_a_tie(c):
    w, r = _ref(c)
    margin = min(float((np.abs(r["Z"][l]) / r["T"][l]).min()) for l in range(len(w.ws) - 1))
    print(f"{tw.cell_id(c)}: smallest |z| / T {margin:.3g}")
    assert TIE == 4e-6 and margin >= TIE, margin


@cells
def test_references_agree(c, oracle_lib):
    w, r = _ref(c)
    shapes = [x.shape for x in w.ws]
    o = oracle_lib.standard_forward_backward(w.X, w.wp, w.bp, shapes, w.dists, w.target, w.S, seed=1.0, dX=True)
    assert abs(o["loss"] - r["loss"]) <= 1e-5 * abs(r["loss"])
    assert_close("acc", o["acc"], r["acc"], **TOLC)
    assert_close("dW", o["dW"], padded(r["dW"], w.wp.shape), **TOLC)
    assert_close("dB", o["dB"], padded(r["db"], w.bp.shape), **TOLC)
    assert_close("dX", o["dX"], r["dX"], **TOLC)
    assert_close("d_dists", o["d_dists"], r["d_dists"], **TOLC)
    assert_close("d_target", o["d_target"], r["d_target"], **TOLC)
    R = w.N * w.S
    for l in range(len(shapes) - 1):
        assert ((o["io"][l, :R, :shapes[l][1]] > 0) == (r["Z"][l] > 0)).all(), l


@pytest.mark.parametrize("c", tw.WIDE_INPUT_CELLS, ids=tw.cell_id)
def test_scaled_cells_are_exact_and_in_range(c):
    w, (s, lw, lb) = tw.cell(*c), tw.scaled(*c)
    L = len(w.ws)
    assert sw.log2_gains(tw.SCALE_PATTERN, L) == [-24] * (L - 1)
    assert (lw, lb) == ([24, 0, 0, -24], [24, 24, 24, 0])
    for l in range(L):
        assert np.array_equal(s.ws[l].astype(np.float64) * 2.0 ** lw[l], w.ws[l].astype(np.float64))
        assert np.array_equal(s.bs[l].astype(np.float64) * 2.0 ** lb[l], w.bs[l].astype(np.float64))
    assert s.wp.shape == w.wp.shape and np.array_equal(s.wp == 0, w.wp == 0)
    r0 = _ref(c)[1]
    r = nerf_np.nerf_forward_backward(s.X, s.ws, s.bs, s.dists, s.target, s.S, seed=1.0)
    assert r["loss"] == r0["loss"] and np.array_equal(r["acc"], r0["acc"]) and np.array_equal(r["dX"], r0["dX"])
    lo, hi = np.inf, 0.0
    for l in range(L):
        assert np.array_equal(r["dW"][l] * 2.0 ** -lw[l], r0["dW"][l]), l
        assert np.array_equal(r["db"][l] * 2.0 ** -lb[l], r0["db"][l]), l
        if l < L - 1:
            assert np.array_equal(r["Z"][l] > 0, r0["Z"][l] > 0), l
        for a in (r["A"][l], r["G"][l], r["dW"][l], r["db"][l]):
            nz = np.abs(a[a != 0])
            lo, hi = min(lo, float(nz.min())), max(hi, float(nz.max()))
    print(f"{tw.cell_id(c)} {tw.SCALE_PATTERN}: nonzero |A|, |G|, |dW|, |db| in [2^{np.log2(lo):.1f}, 2^{np.log2(hi):.1f}]")
    assert 2.0 ** -sw.RANGE_LOG2 <= lo and hi <= 2.0 ** sw.RANGE_LOG2, (np.log2(lo), np.log2(hi))


# ---- coverage, asserted on plan() -----------------------------------------------------------------

def test_plan_restates_the_launch_rules():
    """plan() on shapes whose launch the existing GPU tests already assert through last_path."""
    p = tw.plan([33, 30, 30, 4], 32)
    assert (p["ht16"], p["to16_b0"], p["planes"], p["tile"], p["rays_per_wg"]) == (2, 4, 2, 128, 4)
    assert not p["kr_supported"] and not p["kr"]                     # a training plan: two planes
    p = tw.plan([33] + [256] * 7 + [4], 128, tw.MFMA_BF16)
    assert (p["ht16"], p["planes"], p["kr_supported"], p["kr"], p["rays_per_wg"]) == (16, 1, True, True, 1)
    assert not tw.plan([33] + [256] * 7 + [4], 128, tw.MFMA_BF16 | tw.RENDER_K16)["kr"]
    assert not tw.plan([69, 30, 30, 4], 32, tw.MFMA_BF16)["kr"]      # test_gpu_widths: k0 = 69 renders on k16
    assert tw.plan([64, 30, 30, 4], 32, tw.MFMA_BF16)["kr"]
    assert tw.plan([33, 30, 30, 4], 32, tw.MFMA_BF16X6)["planes"] == 3
    assert tw.plan([33, 30, 30, 4], 32, tw.K16_W4)["tile"] == 64
    # the 8 x 8-tile hidden layers of cfg3 run 2x4 blocks on all eight waves, its head 1x1 on eight
    dw = p["dw"]
    assert dw[0] == (2, 8, (1, 2), 8) and dw[1] == (8, 8, (2, 4), 8) and dw[-1] == (8, 1, (1, 1), 8)
    assert tw.dw_shape(1, 1) == ((1, 1), 1) and tw.dw_shape(3, 3) == ((1, 2), 6) and tw.dw_shape(5, 5) == ((2, 4), 6)


def test_the_cells_reach_every_instantiation():
    plans = {c: tw.cell_plan(c, tw.MFMA_BF16) for c in tw.CELLS}
    assert {p["ht16"] for p in plans.values()} == set(tw.TILES)
    assert {p["to16_b0"] for p in plans.values()} == set(tw.TILES)
    assert {(p["ht16"], p["to16_b0"]) for p in plans.values()} == set(tw.CELLS)        # the whole square
    for c, p in plans.items():
        k0 = tw.cell_dims(*c)[0]
        assert p["kr"] == (k0 <= 64) == (c[1] <= 4), c
        assert not tw.cell_plan(c, tw.MFMA_BF16 | tw.RENDER_K16)["kr"]
        assert not tw.cell_plan(c)["kr_supported"]
    # kr runs in every HT, and so does its fallback to k16's bf16 forward
    assert {c[0] for c, p in plans.items() if p["kr"]} == set(tw.TILES)
    assert {c[0] for c, p in plans.items() if not p["kr"]} == set(tw.TILES)
    assert {tw.cell_dims(ht, 4)[0] for ht in tw.TILES} == {61} and {tw.cell_dims(ht, 8)[0] for ht in tw.TILES} == {125}
    # planes and tiles of the four training paths
    for fl, planes, tile in ((0, 2, 128), (tw.MFMA_F16X3, 2, 128), (tw.MFMA_BF16X6, 3, 128), (tw.K16_W4, 2, 64)):
        assert {(p["planes"], p["tile"]) for p in (tw.cell_plan(c, fl) for c in tw.CELLS)} == {(planes, tile)}


def test_the_layers_reach_every_dw_shape_and_boundary():
    layers = {d for c in tw.CELLS for d in tw.cell_plan(c)["dw"]}
    for shape in tw.DW_SHAPES:
        waves = {wv for _, _, s, wv in layers if s == shape}
        assert tw.DW_WAVES in waves, (shape, "never with every wave active")
        assert min(waves) < tw.DW_WAVES, (shape, "never with an idle wave")
    # 1x1 against 1x2: kt nt = 8 stays 1x1, more leaves it
    assert any(kt * nt == 8 and s == (1, 1) for kt, nt, s, _ in layers)
    assert any(kt * nt > 8 and s == (1, 2) for kt, nt, s, _ in layers)
    # 1x2 against 2x4: kt ceil(nt / 2) = 8 stays 1x2, more leaves it
    assert any(kt * nt > 8 and kt * -(-nt // 2) == 8 and s == (1, 2) for kt, nt, s, _ in layers)
    assert any(kt * -(-nt // 2) > 8 and s == (2, 4) for kt, nt, s, _ in layers)
    # odd tile counts: a 1x2 block whose second tile and a 2x4 block whose rows and columns run out
    assert (3, 4, (1, 2), 6) in layers and (4, 3, (1, 2), 8) in layers
    assert (8, 5, (2, 4), 8) in layers and (5, 8, (2, 4), 6) in layers
    print(sorted(layers))
