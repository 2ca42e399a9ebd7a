"""CPU tests of the input gradients (LNERF_WANT_DINPUT, lnerf_input_grad, lnerf_pose_grad): the
float64 checker chain against a finite difference of the loss, the flag and the exports, and the
failure modes that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import input_grad_ref as igr
import lnerf
import nerf_np
from conftest import REPO, gpu_available

HEADER = os.path.join(REPO, "include", "lnerf.h")
FD_BAR = 1e-7


def _chain_case(rays, S, F, width=16):
    """loss(c2w) in float64 -- get_rays, o + d t, the unrounded encoding, the cfg2 MLP, compositing --
    and d_c2w from the checker chain, both at ReLU masks held at the unperturbed decisions."""
    w = nerf_np.make_workload("cfg2", rays=rays, samples=S, num_functions=F)
    focal = 0.5 / np.tan(0.5 * 0.6911112)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]], np.float64)
    c2w = nerf_np.look_at_pose()[:3, :4].copy()
    rs = np.random.RandomState(100 + rays + S + F)
    pix = rs.choice(width * width, size=rays, replace=rays > width * width)
    t = np.linspace(2.0, 6.0, S)
    dists = np.concatenate((t[1:] - t[:-1], [1e8]))[None, :].repeat(rays, 0)
    dirs = igr.cam_dirs(width, K, pix)

    def points(c):
        o = c[:, 3][None, :].repeat(rays, 0)
        d = dirs @ c[:, :3].T
        return (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3)

    def run(c, masks):
        return nerf_np.nerf_forward_backward(igr.encode64(points(c), F), w.ws, w.bs, dists, w.target, S,
                                             seed=1.0, masks=masks)

    r0 = run(c2w, None)
    masks = [z > 0 for z in r0["Z"]]
    dp = igr.pe_bwd(points(c2w), r0["dX"], F)
    d_rays = igr.rays_bwd(dp.reshape(rays, S, 3), t)
    d_c2w = igr.pose_bwd(d_rays, dirs)
    V = rs.normal(size=(3, 4))
    V /= np.linalg.norm(V)
    return (lambda h: (run(c2w + h * V, masks)["loss"] - run(c2w - h * V, masks)["loss"]) / (2 * h)), \
        float((d_c2w * V).sum())


@pytest.mark.parametrize("rays,S,F", [(5, 30, 5), (3, 128, 5), (9, 17, 0), (64, 32, 5)])
def test_checker_chain_matches_central_difference(rays, S, F):
    """dX of nerf_np.nerf_forward_backward -> pe_bwd -> rays_bwd -> pose_bwd against the central
    difference of the float64 loss along a random unit direction of c2w[:3, :4], h = 1e-6, the ReLU
    masks held at the unperturbed decisions and the encoding fed unrounded. The bar is 1e-7.
    Measured relative differences (this file's cases, in order) at h = 1e-6: 2.5e-10, 1.5e-9,
    2.2e-9, 2.9e-10. At h = 1e-5: 2.0e-8, 1.6e-7, 1.1e-9, 3.0e-8; at h = 1e-4: 2.0e-6, 1.6e-5,
    8.9e-9, 2.5e-2 (the last one moves a head sigma across its ReLU, which the hidden masks do not
    hold). The truncation term falls as h^2; the F = 0 case sits at the rounding floor of the
    difference quotient from h = 1e-5 down."""
    fd, analytic = _chain_case(rays, S, F)
    num = fd(1e-6)
    rel = abs(analytic - num) / abs(num)
    print(f"chain vs central difference ({rays}, {S}, {F}): analytic {analytic:.12g} numeric {num:.12g} rel {rel:.3g}")
    assert rel <= FD_BAR, (analytic, num, rel)


def test_flag_value_is_part_of_the_abi():
    assert lnerf.WANT_DINPUT == 32768
    assert re.search(r"LNERF_WANT_DINPUT\s*=\s*32768\b", open(HEADER).read())


def test_library_exports_and_binds_the_input_gradients():
    lib = lnerf.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lnerf.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in ("lnerf_input_grad", "lnerf_pose_grad"):
        assert name in exported, name
        assert name in lnerf.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    assert len(lib.lnerf_input_grad.argtypes) == 5 and len(lib.lnerf_pose_grad.argtypes) == 7
    for method in ("input_grad", "pose_grad"):
        assert callable(getattr(lnerf.Engine, method))
    assert "d_input" in lnerf.StepResult.__dataclass_fields__


def _batch(x, rays, S, mode, F):
    return lnerf.LnerfBatch(rays, S, mode, F, x.ctypes.data, None, None, 2.0, 6.0)


def _K():
    return (ctypes.c_double * 9)(1.4, 0, 0.5, 0, 1.4, 0.5, 0, 0, 1)


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU failure mode")
def test_input_gradients_without_gpu_fail_loudly():
    """No CPU fallback: with valid arguments and no device both calls return a negative code."""
    lib = lnerf.load_library()
    x = np.zeros((4, 3), np.float32)
    dE = np.zeros((4, 9), np.float32)
    out = np.zeros((4, 3), np.float32)
    b = _batch(x, 2, 2, lnerf.INPUT_POINTS, 1)
    assert lib.lnerf_input_grad(ctypes.byref(b), dE.ctypes.data, None, out.ctypes.data, None) < 0
    assert lnerf.last_error() != ""
    d_rays = np.zeros((4, 6), np.float32)
    d_c2w = np.zeros(12, np.float64)
    assert lib.lnerf_pose_grad(2, _K(), None, 4, d_rays.ctypes.data, d_c2w.ctypes.data, None) < 0
    assert lnerf.last_error() != ""


def test_argument_errors_need_no_device():
    lib = lnerf.load_library()
    x = np.zeros((4, 3), np.float32)
    dE = np.zeros((4, 9), np.float32)
    out = np.zeros((4, 3), np.float32)
    px, pe, po = x.ctypes.data, dE.ctypes.data, out.ctypes.data

    def ig(b, e=pe, o=po):
        rc = lib.lnerf_input_grad(None if b is None else ctypes.byref(b), e, None, o, None)
        assert rc < 0 and lnerf.last_error() != ""
        return lnerf.last_error()

    assert "input_mode" in ig(_batch(x, 2, 2, lnerf.INPUT_ENCODED, 1))
    assert "num_freqs" in ig(_batch(x, 2, 2, lnerf.INPUT_POINTS, -1))
    assert "num_freqs" in ig(_batch(x, 2, 2, lnerf.INPUT_RAYS, 40))
    assert "null" in ig(None)
    assert "null" in ig(_batch(x, 2, 2, lnerf.INPUT_POINTS, 1), e=None)
    assert "null" in ig(_batch(x, 2, 2, lnerf.INPUT_POINTS, 1), o=None)
    assert "null" in ig(lnerf.LnerfBatch(2, 2, lnerf.INPUT_POINTS, 1, None, None, None, 2.0, 6.0))
    assert "empty" in ig(_batch(x, 0, 2, lnerf.INPUT_POINTS, 1))

    d_rays = np.zeros((4, 6), np.float32)
    d_c2w = np.zeros(12, np.float64)
    pr, pc = d_rays.ctypes.data, d_c2w.ctypes.data

    def pg(width, K, pixels, n, r, c):
        rc = lib.lnerf_pose_grad(width, K, pixels, n, r, c, None)
        assert rc < 0 and lnerf.last_error() != ""
        return lnerf.last_error()

    assert "width * width" in pg(2, _K(), None, 3, pr, pc)       # NULL pixels: n must be width^2
    pg(2, None, None, 4, pr, pc)
    pg(2, _K(), None, 4, None, pc)
    pg(2, _K(), None, 4, pr, None)
    pg(0, _K(), None, 0, pr, pc)
