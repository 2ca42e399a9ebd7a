"""CPU conditions on the workloads of tests/width_workloads.py (no GPU): a parity test on a batch whose
gradients are all zero, or whose outputs do not depend on the feature a kernel might drop, passes
vacuously. These are conditions on the inputs, met by the float64 restatement alone; the GPU tests
that run these workloads are test_gpu_widths.py, test_gpu_render_maps.py and test_gpu_input_grad.py.

  * liveness      every layer's dW has a nonzero entry in >= 80 % of its columns (a wide head: of its
                  columns 0..3, and columns 4.. are exactly 0); every ray's opacity sum_j w_j lies in
                  (0.01, 0.99). One exception, stated where it is asserted: the F = 1 scene.
  * sensitivity   zeroing one probed feature (both sides of every 16-wide tile edge up to 64, and
                  k0 - 1) moves the colours or a hidden layer's dW by >= 100 x the fused_parity.TOL64
                  bar and the colours by >= 10 x the 3e-4 bar the bf16 render is held to; scaling a
                  wide head's columns 4.. moves nothing.
  * references    the loma-order fp32 C oracle and the float64 restatement agree within
                  fused_parity.TOLC on every tensor, no row's ReLU decisions differ, no decision is
                  a tie at fp32 resolution (so the GPU tests set no ray aside).
Measured here: live columns >= 0.93, opacities 0.146 .. 0.88 (F = 1 aside), smallest violation of
one dropped feature 3233 x TOL64, smallest colour shift 5.2e-3 (k0 = 256; 9.6e-3 over the F
workloads), worst oracle / float64 error 7.5e-7 of |want| + max|want|.
"""
import functools

import numpy as np
import pytest

import nerf_np
import width_workloads as ww
from fused_parity import TOL64, TOLC, padded
from loma_calls import assert_close

COLOUR_BAR = 3e-4     # test_gpu_render.test_kr_vs_float64_per_element's bar against the bf16 emulation
TIE = 5e-7            # nerf_np.relu_tie_rays' threshold: |z| < TIE sum|terms|


@functools.lru_cache(maxsize=None)
def _ref(case):
    w, _, X, dists = ww.case_workload(case)
    return w, X, dists, nerf_np.nerf_forward_backward(X, w.ws, w.bs, dists, w.target, w.S, seed=None)


cases = pytest.mark.parametrize("case", ww.CASES, ids=ww.case_id)


def test_the_cases_are_the_ones_asked_for():
    assert [3 + 6 * F for F in ww.FREQS] == [3, 9, 63, 69, 123]
    for F in ww.FREQS:
        w, rays32 = ww.freq_workload(F)
        assert (w.N, w.S, w.X.shape) == (24, 32, (768, 3 + 6 * F)) and rays32.shape == (24, 6)
        # the rays are the ones behind the points
        t = np.linspace(2.0, 6.0, w.S)
        o, d = rays32[:, :3].astype(np.float64), rays32[:, 3:].astype(np.float64)
        np.testing.assert_allclose(o[:, None, :] + d[:, None, :] * t[None, :, None], w.pts, rtol=0, atol=1e-6)
    for k0 in ww.ENCODED_K0:
        w = ww.encoded_workload(k0)
        assert [x.shape for x in w.ws] == [(k0, 30), (30, 30), (30, 4)] and w.X.shape == (768, k0)
    for n in ww.HEADS:
        w = ww.head_workload(n)
        assert [x.shape for x in w.ws] == [(33, 30), (30, 30), (30, n)] and w.pts32.shape == (24, 32, 3)


@cases
def test_liveness(case):
    w, X, dists, r = _ref(case)
    L = len(w.ws)
    for l, dW in enumerate(r["dW"]):
        cols = dW[:, :4] if l == L - 1 else dW
        live = float((np.abs(cols) > 0).any(axis=0).mean())
        assert live >= 0.8, (l, live)
    assert (r["dW"][-1][:, 4:] == 0).all() and (r["db"][-1][4:] == 0).all()
    opacity = r["weights"].sum(axis=1)
    print(f"{ww.case_id(case)}: opacity {opacity.min():.3g} .. {opacity.max():.3g}")
    assert (opacity < 0.99).all(), opacity.max()
    if case[:2] == ("freq", 1):
        # make_workload's N(0, 0.5)-bias MLP under nine features leaves 11 of these 24 rays in empty
        # space (sigma = 0 on every sample: opacity, colour and d_dists exactly 0) and the workload is
        # fixed, weights included. The other rays carry the gradient (every dW column is live); the
        # empty ones are a case of their own for the parity tests (exact zeros out).
        assert (opacity > 0.01).sum() >= 12, opacity
    else:
        assert (opacity > 0.01).all(), opacity.min()


@cases
def test_one_dropped_feature_shows(case):
    w, X, dists, r = _ref(case)
    k0 = X.shape[1]
    worst_v, worst_c = np.inf, np.inf
    for f in ww.probed_features(k0):
        X2 = np.array(X, np.float64)
        X2[:, f] = 0.0
        r2 = nerf_np.nerf_forward_backward(X2, w.ws, w.bs, dists, w.target, w.S, seed=None)
        # (dW[0] is left out: its row f is zero by construction, whatever the rest of the step does)
        v = max([ww.violation(r2["acc"], r["acc"], **TOL64)] +
                [ww.violation(r2["dW"][l], r["dW"][l], **TOL64) for l in range(1, len(w.ws) - 1)])
        c = float(np.abs(r2["acc"] - r["acc"]).max())
        worst_v, worst_c = min(worst_v, v), min(worst_c, c)
        assert v >= 100.0, (f, v)
        assert c >= 10 * COLOUR_BAR, (f, c)
    print(f"{ww.case_id(case)}: one dropped feature moves the outputs by >= {worst_v:.0f} x TOL64, "
          f"the colours by >= {worst_c:.3g}")


@pytest.mark.parametrize("case", [c for c in ww.CASES if c[0] == "head"], ids=ww.case_id)
def test_wide_head_columns_do_not_reach_the_outputs(case):
    """The reference reads head columns 0..3 only: cutting the head to them, or scaling columns 4..,
    moves no output, so whatever a kernel lets through from columns 4.. (8 x louder than 0..3) is an
    error against it."""
    w, X, dists, r = _ref(case)
    L = len(w.ws)
    quiet = ww.scale_wide_head(w, 0.125)
    for other in (ww.narrow_head(w), quiet):
        q = nerf_np.nerf_forward_backward(X, other.ws, other.bs, dists, other.target, other.S, seed=None)
        # float64 sums of the same terms (another matrix shape may add them in another order)
        same = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max())
        assert abs(r["loss"] - q["loss"]) <= 1e-12 * q["loss"]
        for k in ("acc", "dX", "d_dists", "d_target"):
            assert same(r[k], q[k]), k
        for l in range(L):
            assert same(r["dW"][l][:, :4] if l == L - 1 else r["dW"][l], q["dW"][l][:, :4] if l == L - 1 else q["dW"][l]), l
            assert same(r["db"][l][:4] if l == L - 1 else r["db"][l], q["db"][l][:4] if l == L - 1 else q["db"][l]), l
    assert np.abs(w.ws[-1][:, 4:]).mean() > 4 * np.abs(w.ws[-1][:, :3]).mean()   # the gain is there


@cases
def test_references_agree(case, oracle_lib):
    w, X, dists, r = _ref(case)
    shapes = [x.shape for x in w.ws]
    c = oracle_lib.standard_forward_backward(X, w.wp, w.bp, shapes, dists, w.target, w.S, seed=None, dX=True)
    assert abs(c["loss"] - r["loss"]) <= 1e-5 * abs(r["loss"])
    assert_close("acc", c["acc"], r["acc"], **TOLC)
    assert_close("dW", c["dW"], padded(r["dW"], w.wp.shape), **TOLC)
    assert_close("dB", c["dB"], padded(r["db"], w.bp.shape), **TOLC)
    assert_close("dX", c["dX"], r["dX"], **TOLC)
    assert_close("d_dists", c["d_dists"], r["d_dists"], **TOLC)
    assert_close("d_target", c["d_target"], r["d_target"], **TOLC)
    R = w.N * w.S
    for l in range(len(shapes) - 1):
        assert ((c["io"][l, :R, :shapes[l][1]] > 0) == (r["Z"][l] > 0)).all(), l
        assert not (np.abs(r["Z"][l]) < TIE * r["T"][l]).any(), l
