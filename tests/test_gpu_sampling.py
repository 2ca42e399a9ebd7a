"""GPU tests of the per-ray sampling entry points (include/lnerf.h "Per-ray sample depths"):
lnerf_sample_stratified, lnerf_sample_importance, lnerf_ray_points and lnerf_ray_points_grad against
the float64 checker of tests/sampling_ref.py, their error paths, and three end-to-end flows
(hierarchical render, a training step on stratified depths, the gradient chain back to the rays).

Bars:
  * stratified depths, points and dists are float64 formulas of a few operations rounded once: the
    checker evaluates the same formulas, so they are bit-equal;
  * a fine depth: 2^-23 |ref| (its one float32 rounding, which may flip on a float64 tie) +
    S 2^-52 slope (the cdf is a sum of S - 2 terms whose order is free; an error e in a cdf entry moves
    the inverse by e times the bin's slope (m_{i+1} - m_i) / (cdf_{i+1} - cdf_i); a u that close to a
    bin edge may fall in the neighbouring bin, hence the largest slope of the three);
  * t_all is a sort of values the GPU itself produced: bit-equal;
  * d_rays: 2^-23 |want| + S 2^-52 sum_j |term_j| (one rounding, any float64 summation order).
Measured on an MI355X (the tests print them): fine-depth error / bar 0.46-0.50 over the 30 cases (the
float32 rounding alone), ray_points_grad 0.20-0.49; the end-to-end figures are in DESIGN.md §3 "ks".
"""
import dataclasses
import os

import numpy as np
import pytest

import sampling_ref as sref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENT = -7.25          # no depth, point coordinate of these scenes or dist can hold it
U32 = 2.0 ** -23
U64 = 2.0 ** -52
RANGES = [(2.0, 6.0), (0.5, 3.25)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _u(rng, rays, n):
    """Uniform numbers with 0, the float32 just under 1, 1.5, -1 and NaN planted every few entries."""
    u = rng.uniform(0, 1, (rays, n)).astype(np.float32)
    special = np.array([0.0, np.float32(1) - np.float32(2.0 ** -24), 1.5, -1.0, np.nan], np.float32)
    flat = u.reshape(-1)
    idx = np.arange(0, flat.size, 3)
    flat[idx] = special[np.arange(idx.size) % 5]
    return u


def _sorted_t(rng, rays, S, lo=2.0):
    """Random non-decreasing depths per ray; odd rays repeat their first depth, so m_0 is a coarse
    depth and u = 0 makes a fine depth tie with it."""
    t = (lo + np.cumsum(rng.uniform(0.03, 0.1, (rays, S)), axis=1)).astype(np.float32)
    t[1::2, 1] = t[1::2, 0]
    return t


def _sentinel(*shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.float32, device="cuda:0")


# ---- 1. stratified depths, points and dists: bit-equal ---------------------------------------------

STRAT = [(1, 1), (3, 2), (65, 17), (130, 64), (2, 200)]


@pytest.mark.parametrize("near,far", RANGES)
@pytest.mark.parametrize("rays,S", STRAT)
def test_stratified_is_the_reference_bit_for_bit(engine, rays, S, near, far):
    u = _u(np.random.RandomState(S), rays, S)
    got = _np(engine.sample_stratified(rays, S, _dev(u), near=near, far=far))
    want = sref.stratified(u, near, far)
    assert got.shape == (rays, S) and np.array_equal(_bits(got), _bits(want))
    assert (np.diff(got, axis=1) >= 0).all()
    again = _np(engine.sample_stratified(rays, S, _dev(u), near=near, far=far))
    assert np.array_equal(_bits(got), _bits(again))


@pytest.mark.parametrize("rays,S", STRAT)
def test_ray_points_is_the_reference_bit_for_bit(engine, rays, S):
    import lnerf
    rng = np.random.RandomState(100 + S)
    rays6 = np.concatenate([rng.normal(size=(rays, 3)) * 3, rng.normal(size=(rays, 3))], axis=1).astype(np.float32)
    t = sref.stratified(_u(rng, rays, S))
    pts, dists = engine.ray_points(_dev(rays6), _dev(t))
    want_p, want_d = sref.ray_points(rays6, t)
    assert tuple(pts.shape) == (rays * S, 3) and tuple(dists.shape) == (rays, S)
    assert np.array_equal(_bits(_np(pts)), _bits(want_p))
    assert np.array_equal(_bits(_np(dists)), _bits(want_d))
    assert (want_d[:, -1] == np.float32(1e8)).all()
    # either output may be NULL: the other one is the same, and rows past the end stay untouched
    p2, d2 = _sentinel(rays * S + 2, 3), _sentinel(rays + 1, S)
    r6, td = _dev(rays6), _dev(t)
    assert engine.lib.lnerf_ray_points(r6.data_ptr(), rays, S, td.data_ptr(), p2.data_ptr(), None, None) == 0, lnerf.last_error()
    assert engine.lib.lnerf_ray_points(r6.data_ptr(), rays, S, td.data_ptr(), None, d2.data_ptr(), None) == 0, lnerf.last_error()
    p2, d2 = _np(p2), _np(d2)
    assert np.array_equal(_bits(p2[:rays * S]), _bits(want_p)) and (p2[rays * S:] == SENT).all()
    assert np.array_equal(_bits(d2[:rays]), _bits(want_d)) and (d2[rays:] == SENT).all()


# ---- 2. importance sampling ------------------------------------------------------------------------

IMPORTANCE = [(1, 3, 1), (3, 4, 5), (65, 17, 64), (130, 64, 64), (5, 128, 200), (2, 1024, 1024)]


def _importance_case(engine, w, n_fine, tc, u, near, far):
    """One call against the checker; returns the worst error / bar of the fine depths."""
    rays, S = w.shape
    ref = sref.importance(w, n_fine, tc, u, near, far)
    args = dict(t_coarse=None if tc is None else _dev(tc), u=None if u is None else _dev(u), near=near, far=far)
    fine, both = engine.sample_importance(_dev(w), n_fine, **args)
    fine2, both2 = engine.sample_importance(_dev(w), n_fine, **args)
    tf, ta = _np(fine), _np(both)
    assert tf.shape == (rays, n_fine) and ta.shape == (rays, S + n_fine)
    assert np.array_equal(_bits(tf), _bits(_np(fine2))) and np.array_equal(_bits(ta), _bits(_np(both2)))
    assert np.isfinite(tf).all() and np.isfinite(ta).all()
    z = tf.astype(np.float64)
    assert (z >= ref["m"][:, :1]).all() and (z <= ref["m"][:, -1:]).all()
    bound = U32 * np.abs(ref["z"]) + S * U64 * sref.neighbour_slope(ref)
    ratio = float((np.abs(z - ref["z"]) / bound).max())
    assert ratio <= 1.0, ratio
    coarse = sref.linspace32(rays, S, near, far) if tc is None else tc
    assert np.array_equal(_bits(ta), _bits(sref.merge(coarse, tf)))
    return ratio


@pytest.mark.parametrize("kind", sref.WEIGHT_KINDS)
@pytest.mark.parametrize("rays,S,n_fine", IMPORTANCE)
def test_importance_sampling(engine, rays, S, n_fine, kind):
    """Every weight kind at every shape, with the linspace and with per-ray sorted depths, with the
    deterministic and with random u (0, just under 1, 1.5, -1 and NaN among them)."""
    rng = np.random.RandomState(S * 1000 + n_fine)
    w = sref.make_weights(kind, rays, S, rng)
    worst = 0.0
    for tc in (None, _sorted_t(rng, rays, S)):
        for u in (None, _u(rng, rays, n_fine)):
            near, far = RANGES[0] if u is None else RANGES[1]
            worst = max(worst, _importance_case(engine, w, n_fine, tc, u, near, far))
    print(f"importance {kind} {(rays, S, n_fine)}: worst fine-depth error / bar {worst:.3g}")


def test_importance_single_outputs(engine):
    """t_fine alone and t_all alone are the two-output call's, bit for bit."""
    rng = np.random.RandomState(7)
    w, u = _dev(sref.make_weights("composited", 65, 17, rng)), _dev(_u(rng, 65, 40))
    fine, both = engine.sample_importance(w, 40, u=u)
    only_fine, none_all = engine.sample_importance(w, 40, u=u, want=("fine",))
    none_fine, only_all = engine.sample_importance(w, 40, u=u, want=("all",))
    assert none_all is None and none_fine is None
    assert np.array_equal(_bits(_np(fine)), _bits(_np(only_fine)))
    assert np.array_equal(_bits(_np(both)), _bits(_np(only_all)))
    with pytest.raises(ValueError):
        engine.sample_importance(w, 40, u=u[:, :39].contiguous())
    with pytest.raises(ValueError):
        engine.sample_importance(w.double(), 40)


# ---- 3. the reverse of ray_points ------------------------------------------------------------------

@pytest.mark.parametrize("scale", [None, 0.37])
@pytest.mark.parametrize("n,S", STRAT + [(5, 128)])
def test_ray_points_grad(engine, n, S, scale):
    rng = np.random.RandomState(10 * n + S)
    t = _sorted_t(rng, n, S) if S > 1 else np.full((n, 1), 3.0, np.float32)
    dp = rng.normal(size=(n * S, 3)).astype(np.float32)
    sc = None if scale is None else _dev(np.array([scale], np.float32))
    got = engine.ray_points_grad(_dev(t), _dev(dp), scale=sc)
    again = engine.ray_points_grad(_dev(t), _dev(dp), scale=sc)
    got = _np(got)
    assert got.shape == (n, 6) and np.array_equal(_bits(got), _bits(_np(again)))
    s = 1.0 if scale is None else float(np.float32(scale))
    want = sref.rays_bwd(dp.reshape(n, S, 3), t) * s
    bound = U32 * np.abs(want) + S * U64 * sref.rays_bwd_l1(dp.reshape(n, S, 3), t) * abs(s)
    ratio = float((np.abs(got - want) / bound).max())
    print(f"ray_points_grad {(n, S)} scale {scale}: worst error / bar {ratio:.3g}")
    assert np.isfinite(got).all() and ratio <= 1.0, ratio


# ---- 4. error paths ---------------------------------------------------------------------------------

def test_errors_write_nothing(engine):
    import lnerf
    import torch
    lib = engine.lib
    rays, S, nf = 5, 8, 8
    w = _dev(np.random.RandomState(0).uniform(0, 1, (rays, 1100)).astype(np.float32))
    fine, both, strat = _sentinel(rays, 1100), _sentinel(rays, 2200), _sentinel(rays, S)
    p = lambda t: None if t is None else t.data_ptr()

    def imp(S, nf, fine, both):
        return lib.lnerf_sample_importance(rays, S, None, 2.0, 6.0, p(w), nf, None, p(fine), p(both), None)

    for what, rc in (("S = 2", imp(2, nf, fine, both)), ("n_fine = 0", imp(S, 0, fine, both)),
                     ("n_fine = 1025", imp(S, 1025, fine, both)), ("both outputs NULL", imp(S, nf, None, None)),
                     ("stratified without u", lib.lnerf_sample_stratified(rays, S, 2.0, 6.0, None, p(strat), None))):
        assert rc != 0 and lnerf.last_error(), what
    torch.cuda.synchronize()
    for name, t in (("t_fine", fine), ("t_all", both), ("sample_t", strat)):
        assert (t.cpu().numpy() == SENT).all(), f"{name} was written by a failing call"
    # and the same buffers take a valid call afterwards
    assert imp(S, nf, fine, both) == 0, lnerf.last_error()
    assert (_np(fine).reshape(-1)[:rays * nf] != SENT).all() and (_np(fine).reshape(-1)[rays * nf:] == SENT).all()


# ---- 5. end to end -----------------------------------------------------------------------------------

def _trained():
    import lnerf
    g = dict(np.load(os.path.join(HERE, "golden", "trained_weights_8x16.npz"), allow_pickle=False))
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    mlp = lnerf.make_mlp(shapes, g["wp"].shape[1], g["wp"].shape[2])
    return mlp, _dev(g["wp"].astype(np.float32)), _dev(g["bp"].astype(np.float32)), int(g["F"])


def test_hierarchical_render(engine):
    """Coarse render (S = 16, weights) -> sample_importance (16 more) -> ray_points -> fine render on
    POINTS with sample_t, on 64 rays of a 16 x 16 frame with the trained fixture's MLP. The fine maps
    are held to test_gpu_render_maps' bars for POINTS input with sample_t, the float64 compositing
    fed the GPU's own t_all, dists and rgba; scene.render_hierarchical_image is the same calls."""
    import lnerf
    import scene
    import torch
    import test_gpu_render_maps as trm
    mlp, ws, bs, F = _trained()
    focal = 0.5 / np.tan(0.5 * scene.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]])
    rays = engine.get_rays(16, K, scene.look_at_pose())[96:160].contiguous()
    N, S, NF = 64, 16, 16
    coarse = engine.render_maps(mlp, ws, bs, rays, None, None, samples=S, input_mode=lnerf.INPUT_RAYS, num_freqs=F,
                                want=("weights", "opacity"))
    t_fine, t_all = engine.sample_importance(coarse.weights, NF)
    points, dists = engine.ray_points(rays, t_all)
    w_np, tf_np, ta_np, d_np, p_np = _np(coarse.weights), _np(t_fine), _np(t_all), _np(dists), _np(points)
    # the pieces, each against the checker
    ref = sref.importance(w_np, NF)
    bound = U32 * np.abs(ref["z"]) + S * U64 * sref.neighbour_slope(ref)
    assert (np.abs(tf_np - ref["z"]) <= bound).all()
    assert np.array_equal(_bits(ta_np), _bits(sref.merge(sref.linspace32(N, S), tf_np)))
    want_p, want_d = sref.ray_points(_np(rays), ta_np)
    assert np.array_equal(_bits(p_np), _bits(want_p)) and np.array_equal(_bits(d_np), _bits(want_d))
    # the fine render
    inp = trm.Inputs(mlp, ws, bs, points, dists, torch.zeros(N, 3, dtype=torch.float32, device="cuda:0"), t_all,
                     lnerf.INPUT_POINTS, S + NF, N, F, d_np, ta_np)
    out, _ = trm.run_maps(engine, inp, 0)
    r = trm.compositing_ratios(out, inp)
    print(f"hierarchical render: coarse opacity {float(_np(coarse.opacity).min()):.3g}..{float(_np(coarse.opacity).max()):.3g},"
          " fine maps worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    m = scene.render_hierarchical_image(engine, (mlp, ws, bs), (mlp, ws, bs), 16, K, scene.look_at_pose(), S, NF, F,
                                        rays=rays)
    assert m.weights is None and m.rgba is None
    for k in ("color", "depth", "opacity"):
        assert np.array_equal(_bits(_np(getattr(m, k))), _bits(out[k])), k


def _cfg2_stratified(engine):
    """cfg2, 64 rays: the workload's own rays at stratified depths; points and dists from ray_points."""
    import nerf_np
    import test_gpu_input_grad as tig
    w = nerf_np.make_workload("cfg2", rays=64)
    rays32, pix = tig._select_rays32(nerf_np.CONFIGS["cfg2"][0], 64)
    u = np.random.RandomState(21).uniform(0, 1, (w.N, w.S)).astype(np.float32)
    t = engine.sample_stratified(w.N, w.S, _dev(u))
    pts, dists = engine.ray_points(_dev(rays32), t)
    t_np, p_np, d_np = _np(t), _np(pts), _np(dists)
    assert np.array_equal(_bits(t_np), _bits(sref.stratified(u)))
    want_p, want_d = sref.ray_points(rays32, t_np)
    assert np.array_equal(_bits(p_np), _bits(want_p)) and np.array_equal(_bits(d_np), _bits(want_d))
    return w, rays32, pix, t, t_np, pts, dists, p_np, d_np


def test_training_step_on_stratified_depths(engine, oracle_lib):
    """The fused step on POINTS from ray_points against the C oracle on the same float32 points and
    dists, at smoke()'s bars: loss 1e-4 relative, dW 1e-4 of its maximum."""
    import lnerf
    import nerf_np
    w, _, _, _, _, pts, dists, p_np, d_np = _cfg2_stratified(engine)
    shapes = [x.shape for x in w.ws]
    r = engine.train_step(lnerf.make_mlp(shapes, w.wp.shape[1], w.wp.shape[2]), _dev(w.wp), _dev(w.bp), pts, dists,
                          _dev(w.target), samples=w.S, num_freqs=w.F, seed=None, flags=lnerf.FAST)
    loss, dW = float(r.loss.item()), _np(r.d_ws)
    assert engine.last_path()["fused"]
    X = oracle_lib.positional_encoding_3d(p_np.reshape(w.N, w.S, 3).astype(np.float64), w.F)
    ref = oracle_lib.standard_forward_backward(X, w.wp, w.bp, shapes, d_np, w.target, w.S)
    print(f"stratified step: loss {loss:.6f} (oracle {ref['loss']:.6f}), max|dW err| / max|dW| "
          f"{np.abs(dW - ref['dW']).max() / np.abs(ref['dW']).max():.3g}")
    assert abs(loss - ref["loss"]) <= 1e-4 * abs(ref["loss"]), (loss, ref["loss"])
    assert np.abs(dW - ref["dW"]).max() <= 1e-4 * np.abs(ref["dW"]).max()
    # the jitter really moved the batch: not the linspace batch's loss
    assert not np.array_equal(p_np, w.pts32.reshape(-1, 3))


def test_gradient_chain_to_the_rays(engine):
    """train_step(want_dinput) on POINTS -> ray_points_grad -> pose_grad. d_points is held to
    test_gpu_input_grad's bar for POINTS mode; that per-element bar, carried through the linear map
    [sum_j, sum_j t_j] by its L1 companion, plus one float32 rounding of the result, bounds d_rays --
    what test_gpu_input_grad propagates for RAYS mode, with per-ray depths; d_c2w likewise."""
    import input_grad_ref as igr
    import lnerf
    import test_gpu_input_grad as tig
    w, rays32, pix, t, t_np, _, _, p_np, d_np = _cfg2_stratified(engine)
    w2 = dataclasses.replace(w, pts=None, X=None, pts32=p_np.reshape(w.N, w.S, 3), dists=d_np)
    got_p, want_p, bound_p, _ = tig._step_case(engine, w2, False, lnerf.FAST, 1.0)
    tig._assert_within("chain d_points", got_p, want_p, bound_p)
    d_rays = engine.ray_points_grad(t, _dev(got_p))
    want_r = sref.rays_bwd(want_p.reshape(w.N, w.S, 3), t_np)
    bound_r = sref.rays_bwd_l1(bound_p.reshape(w.N, w.S, 3), t_np) + U32 * np.abs(want_r)
    tig._assert_within("chain d_rays", _np(d_rays), want_r, bound_r)
    side = 100
    d_c2w = engine.pose_grad(side, tig.K32, d_rays, _dev(pix.astype(np.int32)))
    dirs = igr.cam_dirs(side, tig.K32, pix)
    tig._assert_within("chain d_c2w", _np(d_c2w), igr.pose_bwd(want_r, dirs), igr.pose_bwd_l1(bound_r, dirs))
