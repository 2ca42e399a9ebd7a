"""The float64 compositing helper of the render-maps tests (tests/render_maps_ref.py) against the
float64 restatement of scripts/nerf.py (oracle/nerf_np.py): the checker is right before it judges
the GPU (CPU only)."""
import os

import numpy as np

import nerf_np
import render_maps_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _against_nerf_np(X, ws, bs, dists, target, S):
    r = nerf_np.nerf_forward_backward(X, ws, bs, dists, target, S)
    N = r["rgb"].shape[0]
    t = np.tile(ref.ray_t(S), (N, 1))
    got = ref.composite64(r["rgb"], r["sigma"], dists, t)
    np.testing.assert_allclose(got["weights"], r["weights"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(got["color"], r["acc"], rtol=1e-13, atol=1e-300)
    # the extension's maps are the plain sums of those weights
    np.testing.assert_allclose(got["opacity"], r["weights"].sum(1), rtol=1e-13)
    np.testing.assert_allclose(got["depth"], (r["weights"] * t).sum(1), rtol=1e-13)
    return r, got


def test_composite64_matches_nerf_np_on_cfg2():
    w = nerf_np.make_workload("cfg2", rays=37, samples=100)
    r, got = _against_nerf_np(w.X, w.ws, w.bs, w.dists, w.target, w.S)
    # inclusive transmittance: opacity below 1, depth inside [0, far]
    assert (got["opacity"] > 0.01).all() and (got["opacity"] < 0.99).all()
    assert (got["depth"] >= 0).all() and (got["depth"] <= 6.0).all()


def _fixture(name):
    g = dict(np.load(os.path.join(HERE, "golden", name), allow_pickle=False))
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    ws = [g["wp"][l, :k, :n] for l, (k, n) in enumerate(shapes)]
    bs = [g["bp"][l, :n] for l, (_, n) in enumerate(shapes)]
    return g, ws, bs, int(g["S"])


def test_composite64_on_sigma0_and_delta_1e8_rays():
    """edge_plain_4x8 (every ray ends in the reference's delta = 1e8 sample) and edge_finite_6x8 (which
    also holds the sigma = 0 rays, an opaque and a denormal-transmittance one)."""
    g, ws, bs, S = _fixture("edge_plain_4x8.npz")
    r, got = _against_nerf_np(g["X"], ws, bs, g["dists"], g["target"], S)
    np.testing.assert_allclose(got["color"], g["f64_acc"], rtol=1e-12, atol=1e-300)
    assert (g["dists"][:, -1] == np.float32(1e8)).all()
    # the delta = 1e8 sample has alpha = 1 but the inclusive T_j carries its own (1 - alpha + 1e-10)
    assert (r["sigma"][:, -1] > 0).all() and (got["weights"][:, -1] < 2e-10).all()
    g, ws, bs, S = _fixture("edge_finite_6x8.npz")
    r, got = _against_nerf_np(g["X"], ws, bs, g["dists"], g["target"], S)
    np.testing.assert_allclose(got["color"], g["f64_acc"], rtol=1e-12, atol=1e-300)
    # a sigma = 0 ray is fully transparent: every weight, the opacity and the depth are exactly 0
    z = (r["sigma"] == 0).all(axis=1)
    assert z.any(), "the fixture holds a sigma = 0 ray"
    assert (got["weights"][z] == 0).all() and (got["opacity"][z] == 0).all() and (got["depth"][z] == 0).all()
    assert (got["opacity"] <= 1.0).all()


def test_bars_hold_for_an_fp32_sequential_sum():
    """The summation bar admits a plain fp32 left-to-right sum of fp32-rounded terms (the generic
    path's order), and the weights bar an fp32 evaluation of the weights (numpy float32)."""
    w = nerf_np.make_workload("cfg2", rays=37, samples=100)
    r = nerf_np.nerf_forward_backward(w.X, w.ws, w.bs, w.dists, w.target, w.S)
    rgb32, sg32 = r["rgb"].astype(np.float32), r["sigma"].astype(np.float32)
    t = np.tile(ref.ray_t(w.S), (w.N, 1))
    f = np.float32
    al = f(1) - np.exp(-sg32 * w.dists)
    c = (f(1) - al) + f(1e-10)
    T = np.cumprod(c, axis=1, dtype=np.float32)
    T[:, 0] = 1
    w32 = (al * T).astype(np.float32)
    w64 = ref.composite64(rgb32, sg32, w.dists)["weights"]
    assert (np.abs(w32 - w64) <= ref.weights_bar(w64, w.S)).all()
    sums = ref.sums_from_weights(w32, rgb32, t)
    dep = np.zeros(w.N, np.float32)
    for j in range(w.S):
        dep = dep + w32[:, j] * t[:, j]
    s, bar = sums["depth"]
    assert (np.abs(dep - s) <= bar).all()
