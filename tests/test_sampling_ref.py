"""CPU tests of the per-ray sampling: the float64 checker (tests/sampling_ref.py) against its own
definitions and against scene.make_batch, and the library's and the binding's new surface. The GPU
is judged with this checker in tests/test_gpu_sampling.py."""
import ctypes
import subprocess

import numpy as np
import pytest

import lnerf
import sampling_ref as sref

SHAPES = [(1, 3, 1), (3, 4, 5), (65, 17, 64), (7, 64, 64), (5, 128, 200)]


def _sorted_t(rng, rays, S, lo=2.0):
    return (lo + np.cumsum(rng.uniform(0.03, 0.1, (rays, S)), axis=1)).astype(np.float32)


def _u(rng, rays, n):
    u = rng.uniform(0, 1, (rays, n)).astype(np.float32)
    u.flat[:: 7] = np.array([0.0, np.float32(1) - np.float32(2.0 ** -24), 1.5, -1.0, np.nan], np.float32)[
        np.arange(u.flat[:: 7].size) % 5]
    return u


@pytest.mark.parametrize("kind", sref.WEIGHT_KINDS)
@pytest.mark.parametrize("rays,S,n_fine", SHAPES)
def test_reference_inverts_its_own_cdf(rays, S, n_fine, kind):
    """z lies in [m_0, m_{S-2}] and the cdf is strictly increasing from 0 to exactly 1, on the engine's
    linspace and on random sorted depths; and cdf(z) = u within S 2^-52 on the linspace. Evaluating
    the cdf at z magnifies z's own rounding, 2^-53 |z|, by the bin's (cdf step) / (width): on
    linspace(2, 6, S) that is at most 2^-53 6 (S - 1) / 4 < 0.75 S 2^-52, and the handful of other
    roundings act on quantities below 1. (On depths whose spacing is a small fraction of their
    magnitude the same evaluation loses more than that to z's rounding alone, whatever the inverse
    does, so the identity is held to this bound on the linspace only.)"""
    rng = np.random.RandomState(S * 1000 + n_fine)
    w = sref.make_weights(kind, rays, S, rng)
    for tc in (None, _sorted_t(rng, rays, S)):
        for u in (None, _u(rng, rays, n_fine)):
            r = sref.importance(w, n_fine, tc, u)
            assert np.isfinite(r["z"]).all()
            assert (r["z"] >= r["m"][:, :1]).all() and (r["z"] <= r["m"][:, -1:]).all()
            assert (np.diff(r["cdf"], axis=1) > 0).all() and (r["cdf"][:, 0] == 0).all() and (r["cdf"][:, -1] == 1).all()
            assert (r["u"] >= 0).all() and (r["u"] <= 1).all()
            assert (r["slope"] > 0).all() and np.isfinite(r["slopes"]).all()
            if tc is None:
                err = np.abs(sref.cdf_at(r, r["z"]) - r["u"])
                assert err.max() <= S * 2.0 ** -52, (err.max(), S * 2.0 ** -52)


def test_importance_follows_the_weights():
    """A one-hot interior weight draws (nearly) every sample into that sample's bin; all-zero weights
    spread the midpoint u evenly over [m_0, m_{S-2}]."""
    S, n = 16, 64
    w = np.zeros((1, S), np.float32)
    w[0, 5] = 1.0
    r = sref.importance(w, n)
    m = r["m"][0]
    inside = (r["z"][0] >= m[4]) & (r["z"][0] <= m[5])
    assert inside.mean() > 0.95
    r = sref.importance(np.zeros((1, S), np.float32), n)
    want = m[0] + (np.arange(n) + 0.5) / n * (m[-1] - m[0])
    # (the bin edges come from float32 depths: each sits within 2^-24 6 of the exact linspace's)
    np.testing.assert_allclose(r["z"][0], want, rtol=0, atol=6 * 2.0 ** -23)


@pytest.mark.parametrize("rays,S", [(1, 1), (3, 2), (65, 17), (130, 64), (2, 200)])
def test_stratified_depths_stay_in_their_cells(rays, S):
    rng = np.random.RandomState(S)
    u = _u(rng, rays, S)
    t = sref.stratified(u, 2.0, 6.0).astype(np.float64)
    lower, upper = sref.stratified_cells(S, 2.0, 6.0)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    # the one float32 rounding is monotonic: inside the cell's own float32 roundings
    assert (t >= f32(lower)[None, :]).all() and (t <= f32(upper)[None, :]).all()
    assert (np.diff(t, axis=1) >= 0).all()
    assert (sref.stratified(np.zeros((1, S)))[0] == lower.astype(np.float32)).all()
    if S == 1:
        assert (t == 2.0).all()
    # the grid itself is numpy's linspace
    assert np.array_equal(sref.linspace64(S), np.linspace(2.0, 6.0, S))


@pytest.mark.parametrize("name,S", [("cfg2", None), ("cfg3", 7)])
def test_ray_points_reproduces_make_batch(name, S):
    """With the linspace depths, ray_points is scene.make_batch's own sampling, bit for bit (fed the
    float64 rays make_batch samples from; its `rays` output is their float32 rounding)."""
    import scene
    b = scene.make_batch(name, rays=50, samples=S)
    side = scene.CONFIGS[name][0]
    focal = 0.5 / np.tan(0.5 * scene.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]]).astype(np.float32)
    o, d = scene.get_rays(side, K, scene.look_at_pose())
    sel = np.random.RandomState(0).choice(o.shape[0], size=50, replace=False)
    rays64 = np.concatenate([o[sel], d[sel]], axis=1)
    assert np.array_equal(rays64.astype(np.float32), b["rays"])
    t = np.tile(np.linspace(2.0, 6.0, b["S"]), (50, 1))
    pts, dists = sref.ray_points(rays64, t)
    assert pts.dtype == np.float32 and np.array_equal(pts, b["pts"])
    assert dists.dtype == np.float32 and np.array_equal(dists, b["dists"])


def test_rays_bwd_generalises_input_grad_ref():
    import input_grad_ref as igr
    rng = np.random.RandomState(4)
    dp = rng.normal(size=(6, 9, 3))
    t = np.linspace(2.0, 6.0, 9)
    np.testing.assert_allclose(sref.rays_bwd(dp, np.tile(t, (6, 1))), igr.rays_bwd(dp, t), rtol=1e-14)
    np.testing.assert_allclose(sref.rays_bwd_l1(dp, np.tile(t, (6, 1))), igr.rays_bwd_l1(np.abs(dp), t), rtol=1e-14)


def test_merge_is_a_sort():
    a = np.array([[1.0, 2.0, 2.0, 3.0]], np.float32)
    b = np.array([[2.5, 2.0, 0.5]], np.float32)
    assert np.array_equal(sref.merge(a, b), np.array([[0.5, 1, 2, 2, 2, 2.5, 3]], np.float32))


NEW = {"lnerf_sample_stratified": 7, "lnerf_sample_importance": 11, "lnerf_ray_points": 7,
       "lnerf_ray_points_grad": 7}


def test_library_exports_and_binds_the_sampling_calls():
    import scene
    lib = lnerf.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lnerf.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name, nargs in NEW.items():
        assert name in lnerf.EXPORTED_SYMBOLS, name
        assert name in exported, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    for method in ("sample_stratified", "sample_importance", "ray_points", "ray_points_grad"):
        assert callable(getattr(lnerf.Engine, method)), method
    assert callable(scene.render_hierarchical_image)


def test_argument_errors_need_no_device():
    """The argument checks come first: a negative code and a message, with or without a GPU (host
    arrays stand in for device memory; nothing is launched, so nothing reads them)."""
    lib = lnerf.load_library()
    a = np.zeros((2, 8), np.float32)
    p = a.ctypes.data
    assert lib.lnerf_sample_stratified(2, 8, 2.0, 6.0, None, p, None) < 0 and "u is NULL" in lnerf.last_error()
    assert lib.lnerf_sample_stratified(2, 0, 2.0, 6.0, p, p, None) < 0
    assert lib.lnerf_sample_importance(2, 2, None, 2.0, 6.0, p, 4, None, p, p, None) < 0 and "S = 2" in lnerf.last_error()
    assert lib.lnerf_sample_importance(2, 1025, None, 2.0, 6.0, p, 4, None, p, p, None) < 0
    assert lib.lnerf_sample_importance(2, 8, None, 2.0, 6.0, p, 0, None, p, p, None) < 0 and "n_fine" in lnerf.last_error()
    assert lib.lnerf_sample_importance(2, 8, None, 2.0, 6.0, p, 1025, None, p, p, None) < 0
    assert lib.lnerf_sample_importance(2, 8, None, 2.0, 6.0, p, 4, None, None, None, None) < 0 and "both NULL" in lnerf.last_error()
    assert lib.lnerf_sample_importance(-1, 8, None, 2.0, 6.0, p, 4, None, p, p, None) < 0
    assert lib.lnerf_ray_points(None, 2, 8, p, p, p, None) < 0
    assert lib.lnerf_ray_points_grad(2, 8, p, None, None, p, None) < 0
    # no rays: success, nothing to launch
    assert lib.lnerf_sample_stratified(0, 8, 2.0, 6.0, p, p, None) == 0
    assert lib.lnerf_sample_importance(0, 8, None, 2.0, 6.0, p, 4, None, p, p, None) == 0
    assert lib.lnerf_ray_points(p, 0, 8, p, p, p, None) == 0
    assert lib.lnerf_ray_points_grad(0, 8, p, p, None, p, None) == 0
    assert lnerf.last_error() == ""
