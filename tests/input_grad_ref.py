"""TEST INFRASTRUCTURE ONLY -- float64 numpy restatement of the input gradients (the checker of
lnerf_input_grad / lnerf_pose_grad / LNERF_WANT_DINPUT): the reverse of positional_encoding_3d
(pos_encoding.py:38-69), of the ray sampling o + d t (train_nerf.py:289-299) and of get_rays
(train_nerf.py:23-62), each with its L1 companion -- the same linear map with the absolute values
of its Jacobian entries, which carries a per-element error bound on the map's input to a bound on
its output.
"""
from __future__ import annotations

import numpy as np


def encode64(p: np.ndarray, F: int) -> np.ndarray:
    """positional_encoding_3d in float64, NOT rounded to float32: (R, 3) -> (R, 3 + 6F),
    block-major [p, sin(2^0 p), cos(2^0 p), ...]."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    parts = [p]
    for f in range(F):
        parts += [np.sin((2.0 ** f) * p), np.cos((2.0 ** f) * p)]
    return np.concatenate(parts, axis=1)


def pe_bwd(p: np.ndarray, dE: np.ndarray, F: int) -> np.ndarray:
    """d_p[c] = dE[c] + sum_f 2^f (cos(2^f p_c) dE[3+6f+c] - sin(2^f p_c) dE[6+6f+c]); (R, 3)."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    dE = np.asarray(dE, np.float64)
    out = dE[:, :3].copy()
    for f in range(F):
        s = 2.0 ** f
        out += s * (np.cos(s * p) * dE[:, 3 + 6 * f:6 + 6 * f] - np.sin(s * p) * dE[:, 6 + 6 * f:9 + 6 * f])
    return out


def pe_bwd_l1(p: np.ndarray, e: np.ndarray, F: int) -> np.ndarray:
    """pe_bwd's L1 companion: sum_k |J_k| e_k for per-element bounds e >= 0 on dE."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    e = np.asarray(e, np.float64)
    out = e[:, :3].copy()
    for f in range(F):
        s = 2.0 ** f
        out += s * (np.abs(np.cos(s * p)) * e[:, 3 + 6 * f:6 + 6 * f]
                    + np.abs(np.sin(s * p)) * e[:, 6 + 6 * f:9 + 6 * f])
    return out


def freq_weighted_l1(dE: np.ndarray, F: int) -> np.ndarray:
    """sum_k 2^f(k) |dE_k| per coordinate (f = 0 for the identity block): the scale of an absolute
    error in the sin / cos values themselves; (R, 3)."""
    a = np.abs(np.asarray(dE, np.float64))
    out = a[:, :3].copy()
    for f in range(F):
        out += (2.0 ** f) * (a[:, 3 + 6 * f:6 + 6 * f] + a[:, 6 + 6 * f:9 + 6 * f])
    return out


def rays_bwd(dp: np.ndarray, t: np.ndarray) -> np.ndarray:
    """points = o + d t: d_o = sum_j d_p[j], d_d = sum_j t_j d_p[j]; dp (N, S, 3), t (S,) -> (N, 6)."""
    dp = np.asarray(dp, np.float64)
    t = np.asarray(t, np.float64)
    return np.concatenate([dp.sum(1), (t[None, :, None] * dp).sum(1)], axis=1)


def rays_bwd_l1(e: np.ndarray, t: np.ndarray) -> np.ndarray:
    e = np.asarray(e, np.float64)
    t = np.abs(np.asarray(t, np.float64))
    return np.concatenate([e.sum(1), (t[None, :, None] * e).sum(1)], axis=1)


def cam_dirs(width: int, K: np.ndarray, pixels=None) -> np.ndarray:
    """The float64 camera-frame directions get_rays forms (train_nerf.py:36-48) for the pixels
    (indices into the width x width grid; None: every pixel in order); (n, 3)."""
    K = np.asarray(K, np.float64)
    rng = np.linspace(0, 1, width)
    i, j = np.meshgrid(rng, rng, indexing="xy")
    i, j = i.flatten(), j.flatten()
    dirs = np.stack([(i - K[0, 2]) / K[0, 0], -(j - K[1, 2]) / K[1, 1], -np.ones_like(i)], axis=-1)
    return dirs if pixels is None else dirs[np.asarray(pixels, np.int64)]


def pose_bwd(d_rays: np.ndarray, dirs_cam: np.ndarray) -> np.ndarray:
    """rays[p] = [c2w[:, 3], c2w[:, :3] dir(p)]: d_c2w[a][3] = sum_p d_o[p][a],
    d_c2w[a][b] = sum_p d_d[p][a] dir_b(p); (3, 4)."""
    d_rays = np.asarray(d_rays, np.float64)
    out = np.zeros((3, 4))
    out[:, :3] = d_rays[:, 3:].T @ np.asarray(dirs_cam, np.float64)
    out[:, 3] = d_rays[:, :3].sum(0)
    return out


def pose_bwd_l1(e_rays: np.ndarray, dirs_cam: np.ndarray) -> np.ndarray:
    return pose_bwd(np.abs(np.asarray(e_rays, np.float64)), np.abs(np.asarray(dirs_cam, np.float64)))


def dx_bound(dX: np.ndarray, rtol: float, atol_scale: float) -> np.ndarray:
    """The per-element bar an encoded gradient is held to (loma_calls.assert_close's:
    rtol |dX_k| + atol_scale max|dX|), as an array for the L1 companions."""
    a = np.abs(np.asarray(dX, np.float64))
    return rtol * a + atol_scale * a.max(initial=0.0)
