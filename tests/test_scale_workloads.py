"""CPU conditions on the rescaled workloads of tests/scale_workloads.py (no GPU). The GPU tests of
tests/test_gpu_scale.py assert that a step on weights rescaled by powers of two equals the unscaled
step bit for bit, and float64 per layer and per column; that means something only if, on the
references alone,

  * the float32 rescale is exact, and the float64 restatement is itself equivariant bit for bit
    (same loss and colours, dW_l / fW[l] and db_l / fB[l] the unscaled values);
  * every nonzero |A|, |G|, |dW| and |db| of the rescaled network lies in [2^-100, 2^100]: float32
    stays normal with 26 binades to spare for intermediates, so an exact implementation has no
    excuse (measured: (a)-(d) within [2^-96.1, 2^84.5], (e) within [2^-98.6, 2^42.8]; (e) under alt40
    reaches 2^-139 and is not used);
  * every layer's dW is live and the rays are semi-transparent, as in test_width_workloads.py;
  * under up24, down24 and alt40 the layers' max|dW| span >= 2^40: a whole-tensor bar then sees
    the loudest layer only;
  * the loma-order fp32 C oracle is equivariant bit for bit as well.

The last test shows the gap the per-column bar closes: a 1 % error in the smallest layer of (a)
under alt40 passes the whole-tensor assert_close(..., **TOL64) and fails the per-column bar.
"""
import functools

import numpy as np
import pytest

import nerf_np
import scale_workloads as sw
from fused_parity import TOL64, padded
from loma_calls import assert_close

CASES = [(n, p, sw.base(n)[1]) for n, p in sw.PAIRS] + \
        [(n, p, "rays") for n, p in sw.PAIRS if n in sw.RAYS_WORKLOADS]
cases = pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c))


@functools.lru_cache(maxsize=None)
def _ref(name, pattern, mode):
    w = sw.scaled(name, pattern)[0]
    X, dists, _ = sw.inputs(w, mode)
    return w, X, dists, nerf_np.nerf_forward_backward(X, w.ws, w.bs, dists, w.target, w.S, seed=None)


def test_the_pairs_are_the_ones_asked_for():
    assert len(sw.PAIRS) == 29 and ("e", "alt40") not in sw.PAIRS
    assert sw.log2_gains("up24", 5) == [24] * 4 and sw.log2_gains("down24", 3) == [-24] * 2
    assert sw.log2_gains("alt40", 5) == [40, -40, 40, -40]
    assert sw.log2_gains("ramp8", 8) == [8, 16, 24, 32, 40, 40, 40]
    assert sw.log2_gains("one_up40", 5) == [0, 0, 40, 0] and sw.log2_gains("one_down40", 3) == [0, -40]
    assert sw.factors([40, -40, 40, -40], 5) == ([-40, 80, -80, 80, -40], [-40, 40, -40, 40, 0])
    dims = lambda w: [w.ws[0].shape[0]] + [x.shape[1] for x in w.ws]
    assert dims(sw.base("a")[0]) == [64, 30, 30, 4] and sw.base("a")[0].pts32 is None
    assert dims(sw.base("b")[0]) == [33, 64, 64, 64, 64, 4] and sw.base("b")[0].pts32.shape == (24, 32, 3)
    assert dims(sw.base("c")[0]) == [33, 30, 30, 16]
    assert dims(sw.base("d")[0]) == [33, 30, 30, 4]
    assert dims(sw.base("e")[0]) == [33] + [256] * 7 + [4]
    assert all(sw.base(n)[0].N * sw.base(n)[0].S <= 768 for n in sw.WORKLOADS)
    assert dims(sw.head20_workload()) == [33, 30, 30, 20]


@pytest.mark.parametrize("name,pattern", sw.PAIRS, ids=lambda v: v)
def test_rescale_is_exact(name, pattern):
    w = sw.base(name)[0]
    L = len(w.ws)
    g = sw.log2_gains(pattern, L)
    s, fW, fB = sw.rescale(w, g)
    assert sw.scaled(name, pattern)[1:] == ([int(np.log2(f)) for f in fW], [int(np.log2(f)) for f in fB])
    assert fW[0] == 2.0 ** -g[0] and fB[-1] == 1.0 and fW[-1] == 2.0 ** g[-1]
    for l in range(L):
        for a, b, f in ((s.ws[l], w.ws[l], fW[l]), (s.bs[l], w.bs[l], fB[l])):
            assert a.dtype == np.float32
            assert np.array_equal(a.astype(np.float64) * f, b.astype(np.float64))
            assert (np.abs(a[a != 0]) >= np.finfo(np.float32).tiny).all()
        assert np.array_equal(s.wp[l, :w.ws[l].shape[0], :w.ws[l].shape[1]], s.ws[l])
        assert np.array_equal(s.bp[l, :len(s.bs[l])], s.bs[l])
    assert s.wp.shape == w.wp.shape and s.bp.shape == w.bp.shape
    assert np.array_equal(s.wp == 0, w.wp == 0) and np.array_equal(s.bp == 0, w.bp == 0)
    # the padded form the mlp_fit tests use agrees
    wq, bq, _, _ = sw.rescale_padded(w.wp, w.bp, [x.shape for x in w.ws], g)
    assert np.array_equal(wq, s.wp) and np.array_equal(bq, s.bp)
    assert np.array_equal(sw.unscale(s.bp, [-int(np.log2(f)) for f in fB]), w.bp)


@cases
def test_float64_is_equivariant_and_in_range(case):
    name, pattern, mode = case
    w0, _, _, r0 = _ref(name, None, mode)
    w, _, _, r = _ref(name, pattern, mode)
    _, lw, lb = sw.scaled(name, pattern)
    assert r["loss"] == r0["loss"] and np.array_equal(r["acc"], r0["acc"])
    for k in ("dX", "d_dists", "d_target"):
        assert np.array_equal(r[k], r0[k]), k
    lo, hi = np.inf, 0.0
    for l in range(len(w.ws)):
        assert np.array_equal(r["dW"][l] * 2.0 ** -lw[l], r0["dW"][l]), l
        assert np.array_equal(r["db"][l] * 2.0 ** -lb[l], r0["db"][l]), l
        if l < len(w.ws) - 1:
            assert np.array_equal(r["Z"][l] > 0, r0["Z"][l] > 0), l
        for a in (r["A"][l], r["G"][l], r["dW"][l], r["db"][l]):
            nz = np.abs(a[a != 0])
            if nz.size:
                lo, hi = min(lo, float(nz.min())), max(hi, float(nz.max()))
    print(f"{'-'.join(case)}: nonzero |A|, |G|, |dW|, |db| in [2^{np.log2(lo):.1f}, 2^{np.log2(hi):.1f}]")
    assert 2.0 ** -sw.RANGE_LOG2 <= lo and hi <= 2.0 ** sw.RANGE_LOG2, (np.log2(lo), np.log2(hi))


@cases
def test_liveness_and_spread(case):
    name, pattern, mode = case
    w, _, _, r = _ref(name, pattern, mode)
    L = len(w.ws)
    for l, dW in enumerate(r["dW"]):
        cols = dW[:, :4] if l == L - 1 else dW
        assert np.abs(cols).max() > 0, l
        live = float((np.abs(cols) > 0).any(axis=0).mean())
        # (a)-(d) keep test_width_workloads' 80 %; cfg3's N(0, 0.5) biases leave a quarter of a
        # 256-wide layer's units dead on all of (e)'s 192 rows (measured >= 0.785): a majority there
        assert live >= (0.5 if name == "e" else 0.8), (l, live)
    opacity = r["weights"].sum(axis=1)
    assert (opacity < 0.99).all() and (opacity > 0.01).all(), (opacity.min(), opacity.max())
    mx = [float(np.abs(d).max()) for d in r["dW"]]
    print(f"{'-'.join(case)}: per-layer max|dW| 2^{np.round(np.log2(mx), 1).tolist()}, opacity "
          f"{opacity.min():.3g} .. {opacity.max():.3g}")
    if pattern in sw.SPREAD_PATTERNS:
        assert max(mx) / min(mx) >= 2.0 ** 40, np.log2(mx)


@pytest.mark.parametrize("name,pattern", sw.PAIRS + [("head20", p) for p in sw.PATTERNS], ids=lambda v: v)
def test_c_oracle_is_equivariant(name, pattern, oracle_lib):
    if name == "head20":
        w0 = sw.head20_workload()
        g = sw.log2_gains(pattern, len(w0.ws))
        w = sw.rescale(w0, g)[0]
        lw, lb = sw.factors(g, len(w0.ws))
        mode = "points"
    else:
        w0, mode = sw.base(name)
        w, lw, lb = sw.scaled(name, pattern)
    shapes = [x.shape for x in w.ws]
    X = sw.inputs(w, mode)[0]
    run = lambda v: oracle_lib.standard_forward_backward(X, v.wp, v.bp, shapes, v.dists, v.target, v.S,
                                                         seed=None, dX=True)
    c0, c = _c_unscaled(name, mode, run, w0), run(w)
    assert c["loss"] == c0["loss"]
    for k in ("acc", "dX", "d_dists", "d_target", "rgba"):
        assert np.array_equal(c[k], c0[k]), k
    assert np.array_equal(sw.unscale(c["dW"], lw), c0["dW"])
    assert np.array_equal(sw.unscale(c["dB"], lb), c0["dB"])
    R = w.N * w.S
    for l in range(len(shapes) - 1):
        assert np.array_equal(c["io"][l, :R] > 0, c0["io"][l, :R] > 0), l


_C0 = {}


def _c_unscaled(name, mode, run, w0):
    if (name, mode) not in _C0:
        _C0[(name, mode)] = run(w0)
    return _C0[(name, mode)]


def test_whole_tensor_bar_is_blind_where_the_column_bar_is_not():
    w, _, _, r = _ref("a", "alt40", "encoded")
    shapes = [x.shape for x in w.ws]
    mx = [float(np.abs(d).max()) for d in r["dW"]]
    small = int(np.argmin(mx))
    assert max(mx) / mx[small] >= 2.0 ** 40
    bad = [d.copy() for d in r["dW"]]
    bad[small] *= 1.01
    # the bar check_fused applies without per_layer: accepts
    assert_close("dW", padded(bad, w.wp.shape), padded(r["dW"], w.wp.shape), **TOL64)
    # the per-column bar: 1 % is 1e-2 / (1e-5 + 1e-4) = 90.9 bars at the column's largest entry
    over = sw.dw_col_over_bar(bad, r["dW"], shapes)
    assert over[small] > 50 and all(v == 0 for l, v in enumerate(over) if l != small), over
    with pytest.raises(AssertionError):
        sw.assert_per_layer(bad, r["db"], r["dW"], r["db"], shapes)
    sw.assert_per_layer(r["dW"], r["db"], r["dW"], r["db"], shapes)
