"""GPU tests of the input gradients: lnerf_input_grad's kernel alone, LNERF_WANT_DINPUT on the fused
and the generic training step, lnerf_pose_grad, and the chain get_rays -> train_step -> pose_grad,
each against the float64 checker of input_grad_ref.py within a bound derived from the number
formats (the kernel alone) or propagated from the bar the encoded gradient already meets."""
import os

import numpy as np
import pytest

import input_grad_ref as igr
import nerf_np
from fused_parity import TOL64

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U32 = 2.0 ** -23      # one float32 rounding
TRIG = 2.0 ** -40     # 16 x the recurrence's 2^-44 absolute error per sin / cos value (lnerf_composite.h)
CASES = [(5, 30, 5), (3, 128, 5), (9, 17, 0), (7, 1, 2), (130, 2, 5), (2, 200, 3)]
FOCAL = 0.5 / np.tan(0.5 * 0.6911112)
K32 = np.array([[FOCAL, 0, 0.5], [0, FOCAL, 0.5], [0, 0, 1]], np.float32)


def _dev(engine, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{engine.device}")


def _sync():
    import torch
    torch.cuda.synchronize()


def _select_rays32(side, n, seed=0):
    """float32 rays [o, d] chosen the way nerf_np.make_workload chooses them, and their pixels."""
    o, d = nerf_np.get_rays(side, side, K32, nerf_np.look_at_pose())
    sel = np.random.RandomState(seed).choice(o.shape[0], size=n, replace=n > o.shape[0])
    return np.concatenate([o[sel], d[sel]], 1).astype(np.float32), sel


def _ray_points(rays32, t):
    """The float64 sample points o + d t of float32 rays: (n * S, 3)."""
    o, d = rays32[:, :3].astype(np.float64), rays32[:, 3:].astype(np.float64)
    return (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3)


def _assert_within(name, got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    assert np.isfinite(got).all(), name
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{name}: worst error / bound = {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)
    return ratio


# ---- 1. the kernel alone ---------------------------------------------------------------------------

def _kernel_case(engine, rays_mode, rays, S, F, near=2.0, far=6.0, scale=None, seed=0):
    import lnerf
    rs = np.random.RandomState(1000 * rays + 10 * S + F + seed)
    dE = rs.normal(size=(rays * S, 3 + 6 * F)).astype(np.float32)
    t = np.linspace(near, far, S)
    if rays_mode:
        x, _ = _select_rays32(100, rays, seed=rays + S)
        p = _ray_points(x, t)
    else:
        x = rs.uniform(-6, 6, size=(rays * S, 3)).astype(np.float32)
        p = x.astype(np.float64)
    sc = None if scale is None else _dev(engine, np.array([scale], np.float32))
    got = engine.input_grad(_dev(engine, x), _dev(engine, dE), samples=S,
                            input_mode=lnerf.INPUT_RAYS if rays_mode else lnerf.INPUT_POINTS, num_freqs=F,
                            near=near, far=far, scale=sc)
    _sync()
    want = igr.pe_bwd(p, dE, F)
    slack = igr.freq_weighted_l1(dE, F)
    if rays_mode:
        want = igr.rays_bwd(want.reshape(rays, S, 3), t)
        slack = igr.rays_bwd_l1(slack.reshape(rays, S, 3), t)
    s = 1.0 if scale is None else float(np.float32(scale))
    want, slack = want * s, slack * abs(s)
    return got, want, U32 * np.abs(want) + TRIG * slack, (x, dE)


@pytest.mark.parametrize("rays,S,F", CASES)
@pytest.mark.parametrize("rays_mode", [False, True])
def test_kernel_alone(engine, rays_mode, rays, S, F):
    """Random dE ~ N(0, 1) on random points in [-6, 6]^3 or on get_rays rays, against float64:
    |got - want| <= 2^-23 |want| + 2^-40 sum_k 2^f(k) |dE_k| (for rays summed over j, weight 1 for
    d_o and t_j for d_d). The shapes cover a partial last workgroup, several rays per workgroup and
    rays across waves, S = 1, F = 0 and S above the fused path's 128."""
    got, want, bound, _ = _kernel_case(engine, rays_mode, rays, S, F)
    assert tuple(got.shape) == ((rays, 6) if rays_mode else (rays * S, 3))
    _assert_within(f"input_grad {'RAYS' if rays_mode else 'POINTS'} {(rays, S, F)}", got.cpu().numpy(), want, bound)


@pytest.mark.parametrize("rays_mode", [False, True])
def test_kernel_scale_and_sampling_range(engine, rays_mode):
    got, want, bound, _ = _kernel_case(engine, rays_mode, 5, 30, 5, scale=0.37)
    _assert_within("input_grad scaled", got.cpu().numpy(), want, bound)
    got, want, bound, _ = _kernel_case(engine, rays_mode, 9, 17, 5, near=0.5, far=3.25, scale=-3.0)
    _assert_within("input_grad near/far", got.cpu().numpy(), want, bound)


# ---- 2. NaN containment, 3. determinism ------------------------------------------------------------

@pytest.mark.parametrize("rays_mode", [False, True])
def test_nan_stays_in_its_row_or_ray(engine, rays_mode):
    import lnerf
    rays, S, F = 130, 2, 5
    clean, _, _, (x, dE) = _kernel_case(engine, rays_mode, rays, S, F)
    clean = clean.cpu().numpy()
    row = 2 * 77 + 1
    bad = dE.copy()
    bad[row, :] = np.nan
    got = engine.input_grad(_dev(engine, x), _dev(engine, bad), samples=S,
                            input_mode=lnerf.INPUT_RAYS if rays_mode else lnerf.INPUT_POINTS, num_freqs=F)
    _sync()
    got = got.cpu().numpy()
    hit = row // S if rays_mode else row
    assert np.isnan(got[hit]).all()
    others = np.ones(got.shape[0], bool)
    others[hit] = False
    assert np.isfinite(got[others]).all()
    assert np.array_equal(got[others], clean[others])


def test_repeated_calls_give_the_same_bits(engine):
    a, _, _, _ = _kernel_case(engine, True, 130, 2, 5)
    b, _, _, _ = _kernel_case(engine, True, 130, 2, 5)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    rs = np.random.RandomState(3)
    d_rays = _dev(engine, rs.normal(size=(100 * 100, 6)).astype(np.float32))
    p = engine.pose_grad(100, K32, d_rays)
    q = engine.pose_grad(100, K32, d_rays)
    _sync()
    assert np.array_equal(p.cpu().numpy(), q.cpu().numpy())


# ---- 4. the fused training step --------------------------------------------------------------------

def _step_case(engine, w, rays_mode, flags, seed, rays32=None, tol=TOL64, masks_from_gpu=True):
    """One training step with want_dinput on workload w (POINTS: its float32 points; RAYS: rays32,
    sampled at linspace(2, 6, S)) and the float64 reference at the GPU's ReLU decisions, passed
    through the checker. bound = sum_k |J_k| e_k + 2^-23 |want| with e_k = rtol |dX_k| + atol_scale
    max|dX|, the bar the encoded gradient is already held to."""
    import lnerf
    shapes = [x.shape for x in w.ws]
    L = len(shapes)
    mlp = lnerf.make_mlp(shapes, w.wp.shape[1], w.wp.shape[2])
    t = np.linspace(2.0, 6.0, w.S)
    if rays_mode:
        p = _ray_points(rays32, t)
        dists = np.concatenate((t[1:] - t[:-1], [1e8]))[None, :].repeat(w.N, 0).astype(np.float32)
        x, dd = rays32, None
    else:
        p = w.pts32.reshape(-1, 3).astype(np.float64)
        dists = w.dists
        x, dd = w.pts32.reshape(-1, 3), _dev(engine, w.dists)
    X = nerf_np.positional_encoding_3d(p.reshape(w.N, w.S, 3), w.F).reshape(-1, 3 + 6 * w.F)
    r = engine.train_step(mlp, _dev(engine, w.wp), _dev(engine, w.bp), _dev(engine, x), dd,
                          _dev(engine, w.target), samples=w.S,
                          input_mode=lnerf.INPUT_RAYS if rays_mode else lnerf.INPUT_POINTS, num_freqs=w.F,
                          seed=seed, flags=flags, want_dinput=True)
    _sync()
    assert r.d_x is None
    got = r.d_input.cpu().numpy()
    assert got.shape == x.shape
    path = engine.last_path()
    if masks_from_gpu:
        assert path["k16"], path
        m = engine.relu_masks(L, w.N * w.S)
        masks = [m[l, :, :shapes[l][1]] for l in range(L - 1)]
        dX = nerf_np.nerf_forward_backward(X, w.ws, w.bs, dists, w.target, w.S, seed=seed, masks=masks)["dX"]
    else:
        import oracle
        dX = oracle.standard_forward_backward(X, w.wp, w.bp, shapes, dists, w.target, w.S, seed=seed, dX=True)["dX"]
    want = igr.pe_bwd(p, dX, w.F)
    bound = igr.pe_bwd_l1(p, igr.dx_bound(dX, **tol), w.F)
    if rays_mode:
        want = igr.rays_bwd(want.reshape(w.N, w.S, 3), t)
        bound = igr.rays_bwd_l1(bound.reshape(w.N, w.S, 3), t)
    return got, want, bound + U32 * np.abs(want), path


WORKLOADS = {"cfg2": 64, "chunk": 5, "cfg3": 8}


@pytest.fixture(scope="module")
def workloads():
    return {name: (nerf_np.make_workload(name, rays=n), _select_rays32(nerf_np.CONFIGS[name][0], n)[0])
            for name, n in WORKLOADS.items()}


@pytest.mark.parametrize("seed", [1.0, None])
@pytest.mark.parametrize("flags", [0, 512, 4096])     # default fp16x3, MFMA_BF16X6, K16_W4
@pytest.mark.parametrize("rays_mode", [False, True])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_fused_step_input_gradient(engine, workloads, name, rays_mode, flags, seed):
    """d_input of the fused step against the float64 dX at the GPU's masks passed through the
    checker; the bar is fused_parity.TOL64 on dX carried through the linear map, plus one float32
    rounding. A dropped or mis-signed frequency term is three orders of magnitude above it."""
    import lnerf
    w, rays32 = workloads[name]
    got, want, bound, _ = _step_case(engine, w, rays_mode, lnerf.FAST | flags, seed, rays32)
    _assert_within(f"d_input {name} {'RAYS' if rays_mode else 'POINTS'} flags={flags} seed={seed}", got, want, bound)


FREQ_WORKLOADS = (0, 10, 11, 20)    # k[0] = 3, 63 | 69, 123: both of k16's encoders, either side of 64


@pytest.fixture(scope="module")
def freq_workloads():
    rays32, _ = _select_rays32(nerf_np.CONFIGS["cfg2"][0], 8)
    return {F: (nerf_np.make_workload("cfg2", rays=8, num_functions=F), rays32) for F in FREQ_WORKLOADS}


@pytest.mark.parametrize("flags", [0, 512, 4096])
@pytest.mark.parametrize("rays_mode", [False, True])
@pytest.mark.parametrize("F", FREQ_WORKLOADS)
def test_fused_step_input_gradient_across_frequencies(engine, freq_workloads, F, rays_mode, flags):
    """The step's own d_input (k16's d_x store into the scratch, k0 columns wide, then the encoding's
    reverse) at F = 0, 10, 11 and 20 on 8 rays x 32 samples, seed = loss: the bound of
    test_fused_step_input_gradient. The term of frequency 2^19 carries the weight 2^19 here."""
    import lnerf
    w, rays32 = freq_workloads[F]
    got, want, bound, _ = _step_case(engine, w, rays_mode, lnerf.FAST | flags, None, rays32)
    assert np.abs(want).max() > 0
    _assert_within(f"d_input F={F} {'RAYS' if rays_mode else 'POINTS'} flags={flags}", got, want, bound)


# ---- 5. the generic path ---------------------------------------------------------------------------

GENERIC_TOL = dict(rtol=1e-4, atol_scale=1e-4)   # test_gpu_native.TOL, against the loma-order C oracle


@pytest.mark.parametrize("rays_mode", [False, True])
def test_generic_step_input_gradient(engine, workloads, oracle_lib, rays_mode):
    import lnerf
    w, rays32 = workloads["chunk"]
    got, want, bound, path = _step_case(engine, w, rays_mode, lnerf.GENERIC, None, rays32, tol=GENERIC_TOL,
                                        masks_from_gpu=False)
    assert path["generic"], path
    _assert_within(f"d_input generic {'RAYS' if rays_mode else 'POINTS'}", got, want, bound)


def test_long_rays_take_the_generic_path(engine, oracle_lib):
    """S = 200 is past the fused path's 128 samples: no path flag, the generic kernels, (rays, 6)."""
    w = nerf_np.make_workload("chunk", rays=3, samples=200)
    rays32, _ = _select_rays32(64, 3)
    got, want, bound, path = _step_case(engine, w, True, 0, None, rays32, tol=GENERIC_TOL, masks_from_gpu=False)
    assert path["generic"] and not path["fused"], path
    assert got.shape == (3, 6)
    _assert_within("d_input S=200", got, want, bound)


# ---- 6. ENCODED input: the LNERF_WANT_DX code path -------------------------------------------------

def test_encoded_input_equals_want_dx_bit_for_bit(engine):
    import lnerf
    g = dict(np.load(os.path.join(HERE, "golden", "edge_finite_6x8.npz"), allow_pickle=False))
    d = lambda a: _dev(engine, np.ascontiguousarray(a, np.float32))
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    mlp = lnerf.make_mlp(shapes, g["wp"].shape[1], g["wp"].shape[2])

    def run(**kw):
        r = engine.train_step(mlp, d(g["wp"]), d(g["bp"]), d(g["X"]), d(g["dists"]), d(g["target"]),
                              samples=int(g["S"]), input_mode=lnerf.INPUT_ENCODED, seed=1.0, flags=lnerf.FAST, **kw)
        _sync()
        assert engine.guard_fired() == 1      # the gated bf16x6 re-run rewrote d_x
        return r

    a = run(want_dx=True)
    b = run(want_dinput=True)
    assert a.d_input is None and b.d_x is None
    assert tuple(b.d_input.shape) == tuple(g["X"].shape)
    assert np.array_equal(a.d_x.cpu().numpy(), b.d_input.cpu().numpy())
    c = run(want_dx=True, want_dinput=True)
    assert np.array_equal(a.d_x.cpu().numpy(), c.d_input.cpu().numpy())


def test_want_dx_with_points_input_still_raises(engine, workloads):
    import lnerf
    w, _ = workloads["chunk"]
    shapes = [x.shape for x in w.ws]
    mlp = lnerf.make_mlp(shapes, w.wp.shape[1], w.wp.shape[2])
    args = (mlp, _dev(engine, w.wp), _dev(engine, w.bp), _dev(engine, w.pts32.reshape(-1, 3)),
            _dev(engine, w.dists), _dev(engine, w.target))
    kw = dict(samples=w.S, input_mode=lnerf.INPUT_POINTS, num_freqs=w.F, flags=lnerf.FAST)
    with pytest.raises(RuntimeError, match="LNERF_WANT_DINPUT"):
        engine.train_step(*args, want_dx=True, want_dinput=True, **kw)
    with pytest.raises(RuntimeError, match="LNERF_WANT_DX needs ENCODED input"):
        engine.train_step(*args, want_dx=True, **kw)


# ---- 7. the pose gradient --------------------------------------------------------------------------

@pytest.mark.parametrize("width,picked", [(7, None), (100, 64)])
def test_pose_gradient(engine, width, picked):
    """Against pose_bwd in float64; the output is float64, so only the summation order differs:
    |got - want| <= 2^-40 sum |terms|."""
    rs = np.random.RandomState(width)
    pix = None
    if picked:
        first = rs.choice(width * width, size=picked - 8, replace=False)
        pix = np.concatenate([first, first[:8]]).astype(np.int32)      # 8 of the 64 repeat a pixel
        rs.shuffle(pix)
    n = width * width if pix is None else len(pix)
    d_rays = rs.normal(size=(n, 6)).astype(np.float32)
    got = engine.pose_grad(width, K32, _dev(engine, d_rays), None if pix is None else _dev(engine, pix))
    _sync()
    dirs = igr.cam_dirs(width, K32, pix)
    assert got.dtype.is_floating_point and got.element_size() == 8 and tuple(got.shape) == (3, 4)
    _assert_within(f"pose_grad width {width}", got.cpu().numpy(), igr.pose_bwd(d_rays, dirs),
                   TRIG * igr.pose_bwd_l1(d_rays, dirs))


def test_pose_gradient_skips_pixels_outside_the_grid(engine):
    """The documented behaviour: an index outside the width x width grid contributes nothing."""
    width = 9
    rs = np.random.RandomState(9)
    pix = rs.choice(width * width, size=40, replace=False).astype(np.int32)
    d_rays = rs.normal(size=(40, 6)).astype(np.float32)
    inside = engine.pose_grad(width, K32, _dev(engine, d_rays), _dev(engine, pix))
    more_pix = np.concatenate([pix[:20], np.array([-1, width * width, 2 ** 31 - 1], np.int32), pix[20:]])
    more_rays = np.concatenate([d_rays[:20], 1e6 * np.ones((3, 6), np.float32), d_rays[20:]])
    got = engine.pose_grad(width, K32, _dev(engine, more_rays), _dev(engine, more_pix))
    _sync()
    dirs = igr.cam_dirs(width, K32, pix)
    _assert_within("pose_grad with outside pixels", got.cpu().numpy(), igr.pose_bwd(d_rays, dirs),
                   TRIG * igr.pose_bwd_l1(d_rays, dirs))
    _assert_within("pose_grad without them", inside.cpu().numpy(), igr.pose_bwd(d_rays, dirs),
                   TRIG * igr.pose_bwd_l1(d_rays, dirs))


# ---- 8. get_rays -> train_step -> pose_grad --------------------------------------------------------

def test_pose_refinement_chain(engine, workloads):
    import lnerf
    w, _ = workloads["cfg2"]
    side = nerf_np.CONFIGS["cfg2"][0]
    c2w = nerf_np.look_at_pose(azimuth_deg=20.0, elevation_deg=35.0)
    all_rays = engine.get_rays(side, K32, c2w)
    pix = np.random.RandomState(8).choice(side * side, size=w.N, replace=False).astype(np.int32)
    rays = all_rays[_dev(engine, pix.astype(np.int64))].contiguous()
    _sync()
    rays32 = rays.cpu().numpy()
    got_rays, want_rays, bound_rays, _ = _step_case(engine, w, True, lnerf.FAST, 1.0, rays32)
    _assert_within("chain d_rays", got_rays, want_rays, bound_rays)
    got = engine.pose_grad(side, K32, _dev(engine, got_rays), _dev(engine, pix))
    _sync()
    dirs = igr.cam_dirs(side, K32, pix)
    _assert_within("chain d_c2w", got.cpu().numpy(), igr.pose_bwd(want_rays, dirs),
                   igr.pose_bwd_l1(bound_rays, dirs))
