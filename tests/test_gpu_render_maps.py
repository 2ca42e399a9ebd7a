"""lnerf_render_maps (include/lnerf.h): colour, depth, opacity, per-sample weights and rgba from one
forward render, with or without a target -- on kr, on k16's forward in every precision, and on the
generic path. An extension: the reference (scripts/nerf.py:176-302) computes the per-sample arrays
but never a depth or an opacity; the weights are its own (inclusive transmittance).

What is held to what:
  * acc_color and the loss are lnerf_render's bit for bit (same arithmetic, same order);
  * the compositing is recomputed in float64 from the RETURNED rgba, the float32 dists the forward
    used and t (tests/render_maps_ref.py), so the bars do not depend on the MLP's precision:
    weights within 2^-22 (1 + (S + 1) w64); opacity, depth and each colour channel within
    S 2^-23 sum|term| + 2^-23 |sum| of the float64 sums of the returned weights;
  * rgba against the float64 restatement (oracle/nerf_np.py) for the fp32-class paths.
The shapes are the smallest at which the scans and carries can go wrong: S = 100 with 37 rays (rays
straddle waves, partial tiles, a ragged last workgroup) and S = 7 with 50 rays (many rays per wave,
256 % 7 != 0), on the cfg2-sized MLP (33->30x3->4, HT = 2).

Worst error / bar measured on an MI355X (the tests print them; DESIGN.md §3 "kr / k16 MAPS
instantiations"): weights 0.134, opacity 0.146, depth 0.113, colour 0.182 over every path and shape
of test_compositing; 0.027 / 0.112 / 0.075 / 0.147 on the edge fixtures.
"""
import ctypes
import functools
import os
from dataclasses import dataclass

import numpy as np
import pytest

import nerf_np
import render_maps_ref as ref
import width_workloads as ww

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENT = -7.25    # no map can hold it: colours, weights, opacities lie in [0, 1], depths and sigma are >= 0
ALL = ("color", "depth", "opacity", "weights", "rgba", "loss")
MAPS5 = ALL[:5]


def _flags():
    import lnerf
    return {
        "kr": lnerf.FAST | lnerf.MFMA_BF16,
        "k16_bf16": lnerf.FAST | lnerf.MFMA_BF16 | lnerf.RENDER_K16,
        "fp16x3": lnerf.FAST,
        "bf16x6": lnerf.FAST | lnerf.MFMA_BF16X6,
        "w4": lnerf.FAST | lnerf.K16_W4,
        "generic": lnerf.GENERIC,
    }


PATHS = ("kr", "k16_bf16", "fp16x3", "bf16x6", "w4", "generic")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@dataclass
class Inputs:
    mlp: object
    ws: object
    bs: object
    x: object
    dists: object        # device (N, S) or None (RAYS)
    target: object       # device (N, 3)
    sample_t: object     # device (N, S) or None (RAYS)
    mode: int
    S: int
    N: int
    F: int
    dists_np: np.ndarray   # (N, S) float32: what the forward uses
    t_np: np.ndarray       # (N, S) float32


@functools.lru_cache(maxsize=None)
def _cfg2(N, S):
    """The cfg2 workload (oracle/nerf_np.py) and the rays behind its points (make_workload's own
    selection), so RAYS and POINTS input render the same scene."""
    w = nerf_np.make_workload("cfg2", rays=N, samples=S)
    focal = 0.5 / np.tan(0.5 * 0.6911112)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]]).astype(np.float32)
    o, d = nerf_np.get_rays(100, 100, K, nerf_np.look_at_pose())
    sel = np.random.RandomState(0).choice(o.shape[0], size=N, replace=N > o.shape[0])
    rays6 = np.concatenate([o[sel], d[sel]], axis=1).astype(np.float32)
    return w, rays6


def _inputs(w, mode, rays6=None, sample_t=None):
    import lnerf
    shapes = [x.shape for x in w.ws]
    mlp = lnerf.make_mlp(shapes, w.wp.shape[1], w.wp.shape[2])
    t_np = np.tile(ref.ray_t(w.S), (w.N, 1)) if sample_t is None else np.asarray(sample_t, np.float32)
    if mode == lnerf.INPUT_RAYS:
        x, dists, st = _dev(rays6), None, None
        dists_np = nerf_np.sample_rays(rays6[:, :3].astype(np.float64), rays6[:, 3:].astype(np.float64),
                                       w.S)[1].astype(np.float32)
    else:
        x = _dev(w.pts32.reshape(-1, 3) if mode == lnerf.INPUT_POINTS else w.X)
        dists, st, dists_np = _dev(w.dists), _dev(t_np), w.dists
    return Inputs(mlp, _dev(w.wp), _dev(w.bp), x, dists, _dev(w.target), st, mode, w.S, w.N, w.F, dists_np, t_np)


def _cfg2_inputs(N, S, mode):
    w, rays6 = _cfg2(N, S)
    return _inputs(w, mode, rays6)


def _shapes(inp):
    return dict(color=(inp.N, 3), depth=(inp.N,), opacity=(inp.N,), weights=(inp.N, inp.S),
                rgba=(inp.N * inp.S, 4), loss=(1,))


def _sentinels(inp, names, pad=3):
    import torch
    full = {k: torch.full((s[0] + pad,) + s[1:], SENT, dtype=torch.float32, device="cuda:0")
            for k, s in _shapes(inp).items() if k in names}
    return full, {k: v[:_shapes(inp)[k][0]] for k, v in full.items()}


def run_maps(engine, inp, flags, want=ALL, target=True, sample_t="own"):
    """Engine.render_maps into sentinel-filled buffers with padding rows past the end; returns the maps
    as numpy arrays (the loss as a float32 scalar array) after checking the padding is untouched."""
    import torch
    full, bufs = _sentinels(inp, want)
    st = inp.sample_t if isinstance(sample_t, str) else sample_t
    engine.render_maps(inp.mlp, inp.ws, inp.bs, inp.x, inp.dists, inp.target if target else None, samples=inp.S,
                       input_mode=inp.mode, num_freqs=inp.F, sample_t=st, flags=flags, want=want, buffers=bufs)
    path = engine.last_path()
    torch.cuda.synchronize()
    out = {}
    for k, v in full.items():
        a = v.cpu().numpy()
        n = _shapes(inp)[k][0]
        assert (a[n:] == SENT).all(), f"{k}: rows past the end were written"
        out[k] = a[:n].copy()
    return out, path


def run_render(engine, inp, flags):
    import torch
    loss, acc = engine.render(inp.mlp, inp.ws, inp.bs, inp.x, inp.dists, inp.target, samples=inp.S,
                              input_mode=inp.mode, num_freqs=inp.F, flags=flags)
    path = engine.last_path()
    torch.cuda.synchronize()
    return np.float32(loss.item()), acc.cpu().numpy().copy(), path


def _expect_error(engine, inp, flags, fragment, **kw):
    """The call fails, lnerf_last_error() says why, and every sentinel-filled output stays untouched."""
    import lnerf
    import torch
    want = kw.pop("want", ALL)
    full, bufs = _sentinels(inp, want)
    target = inp.target if kw.pop("target", True) else None
    st = kw.pop("sample_t", inp.sample_t)
    with pytest.raises(RuntimeError) as e:
        engine.render_maps(inp.mlp, inp.ws, inp.bs, inp.x, inp.dists, target, samples=inp.S, input_mode=inp.mode,
                           num_freqs=inp.F, sample_t=st, flags=flags, want=want, buffers=bufs)
    assert lnerf.last_error() and fragment in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for k, v in full.items():
        assert (v.cpu().numpy() == SENT).all(), f"{k} was written by a failing call"


# ---- the compositing bars (case 2) ----------------------------------------------------------

def compositing_ratios(out, inp, rays=None, need_nondegenerate=False):
    """Worst |error| / bar of the weights, opacity, depth and colour of `out` (all five maps) against
    float64 from the returned rgba (render_maps_ref); asserts every one is within its bar."""
    sel = slice(None) if rays is None else rays
    N, S = inp.N, inp.S
    rgba = out["rgba"].reshape(N, S, 4)[sel].astype(np.float64)
    dists, t = inp.dists_np[sel], inp.t_np[sel]
    w64 = ref.composite64(rgba[:, :, :3], rgba[:, :, 3], dists, t)
    if need_nondegenerate:
        assert ((w64["opacity"] > 0.01) & (w64["opacity"] < 0.99)).all(), w64["opacity"]
        pos = (rgba[:, :, 3] > 0).mean()
        assert 0.10 <= pos <= 0.90, f"sigma > 0 on {pos:.1%} of the samples"
    ratios = {}
    werr = np.abs(out["weights"][sel].astype(np.float64) - w64["weights"])
    ratios["weights"] = float((werr / ref.weights_bar(w64["weights"], S)).max())
    sums = ref.sums_from_weights(out["weights"][sel], rgba[:, :, :3], t)
    for k in ("opacity", "depth", "color"):
        s, bar = sums[k]
        err = np.abs(out[k][sel].astype(np.float64) - s)
        # a sum of exact zeros (a sigma = 0 ray) has a zero bar and must be exactly zero
        ratios[k] = float(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)).max())
    for k, v in ratios.items():
        assert v <= 1.0, (k, v, ratios)
    return ratios


# ---- 1. same picture -------------------------------------------------------------------------

# S = 200 exceeds the fused kernels' 128 samples: the generic path's case alone
SAME_PICTURE = [(p, S) for p in PATHS for S in (1, 7, 64, 100, 128)] + [("generic", 200)]


@pytest.mark.parametrize("mode", ["rays", "points"])
@pytest.mark.parametrize("path,S", SAME_PICTURE)
def test_same_picture_as_lnerf_render(engine, path, S, mode):
    """acc_color and the loss are lnerf_render's bit for bit under the same flags and inputs, and
    last_path shows the same kernels plus `maps`. K16_W4 takes S <= 64: above, it is lnerf_render's own
    error, and this call's too."""
    import lnerf
    fl = _flags()[path]
    inp = _cfg2_inputs(37, S, lnerf.INPUT_RAYS if mode == "rays" else lnerf.INPUT_POINTS)
    if path == "w4" and S > 64:
        with pytest.raises(RuntimeError):
            run_render(engine, inp, fl)
        _expect_error(engine, inp, fl, "LNERF_K16_W4")
        return
    loss, acc, rpath = run_render(engine, inp, fl)
    out, mpath = run_maps(engine, inp, fl)
    assert mpath == {**rpath, "maps": True}, (mpath, rpath)
    assert mpath["kr"] == (path == "kr") and mpath["generic"] == (path == "generic")
    assert mpath["k16_w4"] == (path == "w4")
    assert np.array_equal(out["color"], acc)
    assert out["loss"][0] == loss, (out["loss"][0], loss)


# ---- 2. compositing --------------------------------------------------------------------------

# every path at S = 100 / 37 rays and S = 7 / 50 rays; K16_W4 takes S <= 64 (S = 100 is an error there,
# which test_same_picture_as_lnerf_render checks), so its largest ray, S = 64, stands in for it
COMPOSITING = [(p, N, S) for p in PATHS for N, S in ((37, 100), (50, 7)) if not (p == "w4" and S > 64)] + \
              [("w4", 37, 64)]


@pytest.mark.parametrize("mode", ["rays", "points"])
@pytest.mark.parametrize("path,N,S", COMPOSITING)
def test_compositing(engine, path, N, S, mode):
    import lnerf
    inp = _cfg2_inputs(N, S, lnerf.INPUT_RAYS if mode == "rays" else lnerf.INPUT_POINTS)
    out, _ = run_maps(engine, inp, _flags()[path])
    r = compositing_ratios(out, inp, need_nondegenerate=True)
    print(f"render maps {path} {mode} {N}x{S}: worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))


# ---- 3. rgba against the float64 restatement -----------------------------------------------

def _rgba64(X, ws, bs, dists, target, S):
    r = nerf_np.nerf_forward_backward(X, ws, bs, dists, target, S)
    return np.concatenate([r["rgb"].reshape(-1, 3), r["sigma"].reshape(-1, 1)], axis=1)


def _assert_tol64(got, want):
    # fused_parity.TOL64's form: rtol 1e-5, atol 1e-5 max|want| per channel
    for c in range(4):
        atol = 1e-5 * np.abs(want[:, c]).max()
        np.testing.assert_allclose(got[:, c], want[:, c], rtol=1e-5, atol=atol, err_msg=f"channel {c}")


@functools.lru_cache(maxsize=None)
def _cfg2_300():
    w = nerf_np.without_relu_ties(nerf_np.make_workload("cfg2", rays=300))
    X = nerf_np.positional_encoding_3d(w.pts32.astype(np.float64), w.F).reshape(-1, 3 + 6 * w.F)
    return w, _rgba64(X, w.ws, w.bs, w.dists, w.target, w.S)


@pytest.mark.parametrize("path", ["fp16x3", "bf16x6", "generic"])
def test_rgba_against_float64(engine, path):
    import lnerf
    w, want = _cfg2_300()
    out, _ = run_maps(engine, _inputs(w, lnerf.INPUT_POINTS), _flags()[path], want=("rgba",), target=False)
    _assert_tol64(out["rgba"], want)


@pytest.mark.parametrize("path", ["fp16x3", "bf16x6", "generic"])
def test_rgba_against_float64_deep8(engine, path):
    import lnerf
    g = dict(np.load(os.path.join(HERE, "golden", "deep8_w64_2x64.npz"), allow_pickle=False))
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    ws = [g["wp"][l, :k, :n] for l, (k, n) in enumerate(shapes)]
    bs = [g["bp"][l, :n] for l, (_, n) in enumerate(shapes)]
    S = int(g["S"])
    w = nerf_np.Workload(g["pts"], g["pts"].astype(np.float32), g["X"], g["dists"], g["target"], ws, bs, g["wp"],
                         g["bp"], int(g["F"]), S, g["dists"].shape[0])
    out, _ = run_maps(engine, _inputs(w, lnerf.INPUT_ENCODED), _flags()[path], want=("rgba",), target=False)
    _assert_tol64(out["rgba"], _rgba64(g["X"], ws, bs, g["dists"], g["target"], S))


def test_kr_rgba_matches_k16_bf16(engine):
    """kr's rgba against RENDER_K16's at the tolerance test_kr_matches_k16_bf16_forward holds the
    colours to (same operands, another MFMA order), sigma scaled by its range."""
    import lnerf
    w, _ = _cfg2_300()
    inp = _inputs(w, lnerf.INPUT_POINTS)
    a, pa = run_maps(engine, inp, _flags()["kr"], want=("rgba",), target=False)
    b, pb = run_maps(engine, inp, _flags()["k16_bf16"], want=("rgba",), target=False)
    assert pa["kr"] and not pb["kr"]
    np.testing.assert_allclose(a["rgba"], b["rgba"], rtol=2e-5, atol=2e-6 * max(1.0, np.abs(b["rgba"][:, 3]).max()))


# ---- 3b. other first-layer widths and a wide head: the MAPS code objects ---------------------------

WIDTH_PATHS = ("kr", "k16_bf16", "fp16x3", "bf16x6")


@pytest.mark.parametrize("mode", ["rays", "points"])
@pytest.mark.parametrize("path", WIDTH_PATHS)
@pytest.mark.parametrize("F", [0, 10, 11])
def test_same_picture_across_encoding_frequencies(engine, F, path, mode):
    """The MAPS instantiations of kr and k16 are code objects of their own: k[0] = 3, 63 (k16's
    recurrence encoder, kr) and 69 (the per-tile encoder, kr's fallback to k16) on 24 rays x 32
    samples (tests/width_workloads.py). The colour and the loss are lnerf_render's bit for bit, the
    path is the render's plus `maps`, and the fp32-class rgba is float64's."""
    import lnerf
    fl = _flags()[path]
    w, rays6, X, dists = ww.case_workload(("freq", F, mode))
    inp = _inputs(w, lnerf.INPUT_RAYS if mode == "rays" else lnerf.INPUT_POINTS, rays6)
    loss, acc, rpath = run_render(engine, inp, fl)
    out, mpath = run_maps(engine, inp, fl)
    assert mpath == {**rpath, "maps": True}, (mpath, rpath)
    assert mpath["kr"] == (path == "kr" and 3 + 6 * F <= 64) and mpath["k16"] and not mpath["generic"], mpath
    assert mpath["planes"] == dict(kr=1, k16_bf16=1, fp16x3=2, bf16x6=3)[path]
    assert np.array_equal(out["color"], acc)
    assert out["loss"][0] == loss, (out["loss"][0], loss)
    if path in ("fp16x3", "bf16x6"):
        _assert_tol64(out["rgba"], _rgba64(X, w.ws, w.bs, dists, w.target, w.S))


def test_head16_maps(engine):
    """A 16-output head (columns 4.. eight times louder than 0..3): rgba is (rows, 4) of columns 0..3 --
    float64's, with the rows past the end untouched (run_maps) -- and the picture is lnerf_render's."""
    import lnerf
    fl = _flags()["fp16x3"]
    w, _, X, dists = ww.case_workload(("head", 16, "points"))
    inp = _inputs(w, lnerf.INPUT_POINTS)
    loss, acc, rpath = run_render(engine, inp, fl)
    out, mpath = run_maps(engine, inp, fl)
    assert mpath == {**rpath, "maps": True} and mpath["planes"] == 2, (mpath, rpath)
    assert out["rgba"].shape == (w.N * w.S, 4)
    assert np.array_equal(out["color"], acc) and out["loss"][0] == loss
    _assert_tol64(out["rgba"], _rgba64(X, w.ws, w.bs, dists, w.target, w.S))
    compositing_ratios(out, inp)


# ---- 4. no target ----------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["kr", "fp16x3", "generic"])
def test_no_target(engine, path):
    import lnerf
    import torch
    fl = _flags()[path]
    inp = _cfg2_inputs(37, 100, lnerf.INPUT_RAYS)
    with_t, _ = run_maps(engine, inp, fl)
    spare = torch.full((4,), SENT, dtype=torch.float32, device="cuda:0")   # a loss buffer nobody is given
    without, pth = run_maps(engine, inp, fl, want=MAPS5, target=False)
    assert pth["maps"]
    for k in MAPS5:
        assert np.array_equal(with_t[k], without[k]), k
    assert (spare.cpu().numpy() == SENT).all()
    _expect_error(engine, inp, fl, "loss", target=False)


# ---- 5. NULL outputs -------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["kr", "fp16x3", "generic"])
def test_null_outputs(engine, path):
    """Each output alone equals its value in the all-outputs call (nothing else is passed, so nothing
    else can change; rows past the end stay untouched), and out == NULL runs and writes nothing."""
    import lnerf
    import torch
    fl = _flags()[path]
    inp = _cfg2_inputs(50, 7, lnerf.INPUT_POINTS)
    full, _ = run_maps(engine, inp, fl)
    for k in ALL:
        one, _ = run_maps(engine, inp, fl, want=(k,))
        assert list(one) == [k] and np.array_equal(one[k], full[k]), k
    # out == NULL, straight through the C ABI; bystander buffers stay as they were
    bystanders, _ = _sentinels(inp, ALL)
    b = lnerf.LnerfBatch(inp.N, inp.S, inp.mode, inp.F, inp.x.data_ptr(), inp.dists.data_ptr(), inp.target.data_ptr(),
                         2.0, 6.0)
    rc = engine.lib.lnerf_render_maps(engine.ctx, ctypes.byref(inp.mlp), inp.ws.data_ptr(), inp.bs.data_ptr(),
                                      ctypes.byref(b), inp.sample_t.data_ptr(), fl, None, None)
    assert rc == 0, lnerf.last_error()
    assert engine.last_path()["maps"]
    torch.cuda.synchronize()
    for k, v in bystanders.items():
        assert (v.cpu().numpy() == SENT).all(), k


# ---- 6. sample_t -----------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["kr", "fp16x3", "generic"])
def test_sample_t_depth(engine, path):
    import lnerf
    w, _ = _cfg2(37, 100)
    rng = np.random.RandomState(11)
    st = np.cumsum(rng.uniform(0.01, 0.2, (w.N, w.S)), axis=1).astype(np.float32) + 1.5   # increasing per ray
    inp = _inputs(w, lnerf.INPUT_POINTS, sample_t=st)
    out, _ = run_maps(engine, inp, _flags()[path])
    r = compositing_ratios(out, inp)
    # and the depth really is this t's: far from the linspace depths' one
    lin, _ = run_maps(engine, _inputs(w, lnerf.INPUT_POINTS), _flags()[path], want=("depth",), target=False)
    assert np.abs(out["depth"] - lin["depth"]).max() > 0.1
    print(f"render maps {path} sample_t depth: worst error / bar {r['depth']:.3g}")


def test_sample_t_and_head_errors(engine):
    import lnerf
    fl = _flags()["fp16x3"]
    pts = _cfg2_inputs(37, 7, lnerf.INPUT_POINTS)
    _expect_error(engine, pts, fl, "sample_t", sample_t=None)
    w, rays6 = _cfg2(37, 7)
    _expect_error(engine, _inputs(w, lnerf.INPUT_ENCODED), fl, "sample_t", sample_t=None)
    # without depth nothing reads sample_t: no error
    run_maps(engine, pts, fl, want=("color", "opacity"), sample_t=None)
    rays = _inputs(w, lnerf.INPUT_RAYS, rays6)
    _expect_error(engine, rays, fl, "RAYS", sample_t=pts.sample_t)
    _expect_error(engine, pts, fl | lnerf.HEAD_FIT, "HEAD_FIT")
    _expect_error(engine, pts, lnerf.GENERIC | lnerf.HEAD_FIT, "HEAD_FIT")


# ---- 7. edge numerics ------------------------------------------------------------------------

def _edge_inputs(name, nan_dist=None):
    import lnerf
    g = dict(np.load(os.path.join(HERE, "golden", name), allow_pickle=False))
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    ws = [g["wp"][l, :k, :n] for l, (k, n) in enumerate(shapes)]
    bs = [g["bp"][l, :n] for l, (_, n) in enumerate(shapes)]
    S, N = int(g["S"]), g["dists"].shape[0]
    dists = g["dists"].copy()
    if nan_dist is not None:
        dists[nan_dist] = np.nan
    w = nerf_np.Workload(None, None, g["X"], dists, g["target"], ws, bs, g["wp"], g["bp"], 0, S, N)
    return g, _inputs(w, lnerf.INPUT_ENCODED)


def _check_edge(g, inp, out, path, name, nan):
    """Rays outside `nan` (a bool per ray): finite and inside test_compositing's bars; sigma = 0 rays
    exactly transparent."""
    for k in ("color", "depth", "opacity", "weights"):
        assert np.isfinite(out[k].reshape(inp.N, -1)[~nan]).all(), k
    assert np.isfinite(out["rgba"]).all()
    r = compositing_ratios(out, inp, rays=np.nonzero(~nan)[0])
    z = np.array([k == "sigma0" for k in g["kinds"]])
    assert (out["opacity"][z] == 0).all() and (out["depth"][z] == 0).all() and (out["weights"][z] == 0).all()
    print(f"render maps {path} {name}: worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))


@pytest.mark.parametrize("path", ["fp16x3", "bf16x6", "generic"])
@pytest.mark.parametrize("name", ["edge_plain_4x8.npz", "edge_finite_6x8.npz", "edge_nan_3x8.npz"])
def test_edge_numerics(engine, name, path):
    """sigma = 0 rays, delta = 1e8, denormal transmittance, an opaque ray: the bars of test_compositing,
    and the fixture's own colours. (edge_nan's NaN is the sigmoid ADJOINT's, expf(100) in the reverse
    pass: its forward is finite, golden acc included, and so are its maps.)"""
    g, inp = _edge_inputs(name)
    out, _ = run_maps(engine, inp, _flags()[path])
    _check_edge(g, inp, out, path, name, np.zeros(inp.N, bool))
    np.testing.assert_allclose(out["color"], g["acc"], rtol=1e-5, atol=1e-5 * np.abs(g["acc"]).max())


@pytest.mark.parametrize("path", ["fp16x3", "bf16x6", "generic"])
def test_nan_stays_in_its_ray(engine, path):
    """edge_nan_3x8 with a NaN delta on sample 3 of its `nan` ray, so that the compositing itself meets
    one (a NaN input feature would not do: the hidden ReLUs take z > 0, nerf.py:141-144, and turn it
    into 0). That ray's colour, depth and opacity are NaN and its weights from the NaN sample on (the
    scan is a prefix: the samples in front keep finite weights); the other rays' maps are the clean
    run's bit for bit, finite and inside the bars."""
    g, clean_inp = _edge_inputs("edge_nan_3x8.npz")
    ray = list(g["kinds"]).index("nan")
    S = clean_inp.S
    g, inp = _edge_inputs("edge_nan_3x8.npz", nan_dist=(ray, 3))
    clean, _ = run_maps(engine, clean_inp, _flags()[path])
    out, _ = run_maps(engine, inp, _flags()[path])
    nan = np.arange(inp.N) == ray
    for k in ("color", "depth", "opacity"):
        assert np.isnan(out[k].reshape(inp.N, -1)[nan]).all(), k
    assert np.array_equal(out["rgba"], clean["rgba"])
    assert np.isnan(out["weights"][ray, 3:]).all() and np.isfinite(out["weights"][ray, :3]).all()
    for k in MAPS5:
        a, b = out[k].reshape(inp.N, -1), clean[k].reshape(inp.N, -1)
        assert np.array_equal(a[~nan], b[~nan]), k
    _check_edge(g, inp, out, path, "edge_nan_3x8.npz + NaN delta", nan)


# ---- 8. frame sanity -------------------------------------------------------------------------

def _config5():
    import lnerf
    import scene
    shapes, wp, bp = scene.init_mlp(33, 4, 8, 256)
    focal = 0.5 / np.tan(0.5 * scene.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]])
    return lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2]), _dev(wp), _dev(bp), K, scene.look_at_pose()


def test_frame_16x16(engine):
    import lnerf
    import scene
    import torch
    mlp, ws, bs, K, c2w = _config5()
    fl = lnerf.FAST | lnerf.MFMA_BF16
    m = scene.render_maps_image(engine, mlp, ws, bs, 16, K, c2w, 128, 5, flags=fl)
    p = engine.last_path()
    assert p["kr"] and p["maps"], p
    assert m.weights is None and m.rgba is None and m.loss is None
    img = scene.render_image(engine, mlp, ws, bs, 16, K, c2w, 128, 5, flags=fl)
    torch.cuda.synchronize()
    assert np.array_equal(m.color.cpu().numpy(), img.cpu().numpy())
    d, o = m.depth.cpu().numpy(), m.opacity.cpu().numpy()
    assert d.shape == o.shape == (256,)
    assert (d >= 0).all() and (d <= 6.0).all() and (o >= 0).all() and (o <= 1.0).all()


def test_full_frame_is_its_ray_subset(engine):
    """The config-5 frame (800 x 800 rays x 128 samples), per-ray outputs only: on a seeded 512-ray
    subset, depth and opacity equal a second call on just those rays bit for bit (a ray's maps depend
    on its own samples only; test_kr_full_frame_is_its_row_shards checks this for the colour)."""
    import lnerf
    import scene
    import torch
    mlp, ws, bs, K, c2w = _config5()
    fl = lnerf.FAST | lnerf.MFMA_BF16
    rays = engine.get_rays(800, K, c2w)
    m = scene.render_maps_image(engine, mlp, ws, bs, 800, K, c2w, 128, 5, flags=fl, rays=rays)
    assert engine.last_path()["kr"]
    sel = torch.from_numpy(np.sort(np.random.RandomState(5).choice(rays.shape[0], 512, replace=False))).to("cuda:0")
    sub = engine.render_maps(mlp, ws, bs, rays[sel].contiguous(), None, None, samples=128, input_mode=lnerf.INPUT_RAYS,
                             flags=fl)
    torch.cuda.synchronize()
    for k in ("color", "depth", "opacity"):
        a, b = getattr(m, k)[sel].cpu().numpy(), getattr(sub, k).cpu().numpy()
        assert np.isfinite(a).all() and np.array_equal(a, b), k
    d, o = m.depth.cpu().numpy(), m.opacity.cpu().numpy()
    assert (d >= 0).all() and (d <= 6.0).all() and (o >= 0).all() and (o <= 1.0).all()
