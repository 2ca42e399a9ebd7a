"""tests/render_vjp_ref.py, the float64 reference of lnerf_render_maps_vjp, before it judges the GPU
(tests/test_gpu_render_vjp.py), and the conditions its workloads (tests/render_vjp_workloads.py) must
meet for a comparison on them to mean anything. CPU only.

  1. With d_color = 2 (C - target) and nothing else it is nerf_np.nerf_forward_backward(seed=1), the
     derivative the training step computes, to float64 rounding.
  2. Each adjoint kind alone agrees with central differences of the float64 forward's pairing
     sum(map * adjoint), with respect to weights, biases, inputs and dists -- on a workload with the
     inclusive transmittance's corners: T_0 = 1, a 1e8 last delta and sigma = 0 samples.
  3. Non-vacuity, on every GPU workload, with the unit-scale adjoints the GPU test draws:
     * at least a quarter of the rays are semi-transparent (0.05 < opacity < 0.95);
     * each adjoint kind ALONE gives, in every layer, a dW whose largest element is >= 1000 of the bars
       the GPU test applies to that comparison (per column 1e-5 |want| + 1e-4 x the column's max), a
       nonzero db, and -- every kind but rgba, which d_dists does not depend on (rgba is no function
       of dists, and dRGBA enters neither dw nor dal) -- a d_dists >= 1000 TOL64 bars of the all-five
       result: no layer is dead, so no comparison on these workloads can pass on zeros;
     * in the all-five comparison, where the unit-scale dRGBA (one adjoint per sample and channel,
       straight into the head) is the loudest term, each kind's own contribution is still >= 10 of the
       all-five per-column bars in every layer: a kind whose term went missing (or lost its t_j, or its
       dO) shifts the all-five result by its whole contribution, and the GPU's own error is at most one
       bar, so ten bars cannot hide. (Measured, float64: colour >= 117, depth >= 151, opacity >= 57,
       weights >= 73, rgba >= 9138 bars, the smallest at S = 128 / 129.)
"""
import numpy as np
import pytest

import nerf_np
import render_vjp_ref as ref
import render_vjp_workloads as wl
from fused_parity import TOL64


def _small():
    """6 rays x 8 samples, 9 -> 12 -> 12 -> 4, with sigma = 0 samples and the 1e8 last delta."""
    rng = np.random.RandomState(3)
    dims, N, S = [9, 12, 12, 4], 6, 8
    ws = [rng.randn(k, n) * np.sqrt(2.0 / k) for k, n in zip(dims, dims[1:])]
    bs = [rng.uniform(0.1, 0.6, n) for n in dims[1:]]
    ws[-1][:, 3] *= 0.3
    bs[-1][3] = -0.35                                    # sigma of both signs: ReLU zeros some samples
    X = rng.uniform(-1, 1, (N * S, dims[0]))
    dists = np.full((N, S), 4.0 / (S - 1))
    dists[:, -1] = 1e8
    t = np.sort(rng.uniform(2, 6, (N, S)), axis=1)
    return ws, bs, X, dists, t, N, S


def test_color_adjoint_is_the_training_step():
    ws, bs, X, dists, t, N, S = _small()
    target = np.random.RandomState(4).uniform(0, 1, (N, 3))
    want = nerf_np.nerf_forward_backward(X, ws, bs, dists, target, S, seed=1.0)
    got = ref.render_vjp64(X, ws, bs, dists, S, dict(color=2.0 * (want["acc"] - target)))
    assert (want["sigma"] == 0).any() and (want["sigma"] > 0).any()
    close = lambda a, b: np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1e-300)
    for l in range(len(ws)):
        assert close(got["dW"][l], want["dW"][l]) and close(got["db"][l], want["db"][l]), l
    assert close(got["dX"], want["dX"]) and close(got["d_dists"], want["d_dists"])
    assert close(got["maps"]["color"], want["acc"]) and close(got["maps"]["weights"], want["weights"])


@pytest.mark.parametrize("kind", ref.ADJOINTS + ("all",))
def test_each_adjoint_against_central_differences(kind):
    ws, bs, X, dists, t, N, S = _small()
    kinds = ref.ADJOINTS if kind == "all" else (kind,)
    adj = {k: v.astype(np.float64) for k, v in ref.random_adjoints(N, S, 11, kinds).items()}
    f0 = ref.forward64(X, ws, bs, dists, S, t)
    masks = [z > 0 for z in f0["Z"][:-1]]                # frozen decisions: the pairing is smooth
    got = ref.render_vjp64(X, ws, bs, dists, S, adj, t, masks)
    assert (f0["sigma"] == 0).any() and (f0["sigma"] > 0).any()

    def pairing(ws_, bs_, X_, d_):
        return ref.pairing(ref.forward64(X_, ws_, bs_, d_, S, t, masks), adj)

    rng = np.random.RandomState(12)
    worst = 0.0

    def probe(name, arr, grad, rebuild, n=6, h=1e-6, live=None):
        nonlocal worst
        idx = [tuple(rng.randint(0, s) for s in arr.shape) for _ in range(n)]
        for i in idx:
            if live is not None and not live[i]:
                continue
            a = arr.copy()
            step = h * max(abs(arr[i]), 1.0)
            a[i] = arr[i] + step
            up = pairing(*rebuild(a))
            a[i] = arr[i] - step
            dn = pairing(*rebuild(a))
            fd = (up - dn) / (2 * step)
            scale = max(np.abs(grad).max(), 1e-30)
            worst = max(worst, abs(fd - grad[i]) / scale)

    for l in range(len(ws)):
        probe(f"W{l}", ws[l], got["dW"][l], lambda a, l=l: (ws[:l] + [a] + ws[l + 1:], bs, X, dists))
        probe(f"b{l}", bs[l], got["db"][l], lambda a, l=l: (ws, bs[:l] + [a] + bs[l + 1:], X, dists))
    probe("X", X, got["dX"], lambda a: (ws, bs, a, dists))
    # (the 1e8 delta's derivative is ~0 and its finite difference meaningless at any step: interior only)
    live = np.ones(dists.shape, bool)
    live[:, -1] = False
    probe("dists", dists, got["d_dists"], lambda a: (ws, bs, X, a), n=12, live=live)
    print(f"{kind}: worst |fd - vjp| / max|grad| = {worst:.3g}")
    assert worst <= 1e-6, worst


def _alone_and_all(c):
    out = {}
    full = ref.random_adjoints(c.w.N, c.w.S, 21)
    for kind in ref.ADJOINTS + ("all",):
        adj = full if kind == "all" else {kind: full[kind]}
        out[kind] = ref.render_vjp64(c.X, c.w.ws, c.w.bs, c.dists, c.w.S, adj, c.t)
    return out


@pytest.mark.parametrize("name", wl.ALL)
def test_gpu_workloads_are_not_vacuous(name):
    c = wl.case(name)
    r = _alone_and_all(c)
    op = r["all"]["maps"]["opacity"]
    semi = float(((op > 0.05) & (op < 0.95)).mean())
    assert semi >= 0.25, f"{name}: {semi:.2f} of the rays are semi-transparent"
    shapes = [x.shape for x in c.w.ws]
    allr = r["all"]
    dd_bar = TOL64["rtol"] * np.abs(allr["d_dists"]) + TOL64["atol_scale"] * np.abs(allr["d_dists"]).max()
    report = {}
    for kind in ref.ADJOINTS:
        g = r[kind]
        own, mixed = [], []
        for l, (k, n) in enumerate(shapes):
            assert np.abs(g["db"][l]).max() > 0, (name, kind, l)
            for want, out in ((g["dW"][l], own), (allr["dW"][l], mixed)):
                bar = 1e-5 * np.abs(want) + 1e-4 * np.abs(want).max(axis=0, keepdims=True)
                out.append(float((np.abs(g["dW"][l]) / np.maximum(bar, 1e-300)).max()))
        dd = float((np.abs(g["d_dists"]) / np.maximum(dd_bar, 1e-300)).max())
        report[kind] = (min(own), min(mixed), dd)
        assert min(own) >= 1000, f"{name}: {kind} alone moves dW by {own} of its own bars per layer"
        assert min(mixed) >= 10, f"{name}: {kind} alone moves dW by {mixed} of the all-five bars per layer"
        if kind == "rgba":
            assert dd == 0.0, "d_dists does not depend on dRGBA"
        else:
            assert dd >= 1000, f"{name}: {kind} alone moves d_dists by {dd:.3g} bars"
    print(name, f"semi-transparent {semi:.2f}", {k: tuple(round(v) for v in t) for k, t in report.items()})
