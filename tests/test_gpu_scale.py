"""Weight-scale equivariance of the fused, generic and render paths (tests/scale_workloads.py;
tests/test_scale_workloads.py holds the CPU conditions that make these runs worth doing).

Much of the fused path exists to handle magnitude -- the per-layer weight shift, the head's
per-column shift, k1's per-sample row shifts and their signed bytes in the slab word, the int24
activation slabs, dw16's per-layer product shift and exceptional rows, the floor guard, the shift
clamp -- and every other GPU parity workload has O(1) weights, so all of it runs within a few binades
of 2^0. Rescaling a ReLU MLP's layers by powers of two (W_l g_l / g_{l-1}, b_l g_l) moves the hidden
activations by 2^+-24 .. 2^+-40 and the layers' dW up to 2^160 apart while the loss, the colours,
d_dists, d_target, dX and every ReLU decision stay what they were, dW_l scales by fW[l] = g_{l-1} / g_l
and db_l by fB[l] = 1 / g_l, exactly.

Training step (default = guarded fp16x3, MFMA_F16X3, MFMA_BF16X6, K16_W4), per (workload, pattern):
  A. against float64 at the GPU's own ReLU decisions on the rescaled weights: check_fused with
     per_layer=True -- loss 1e-6, acc / d_dists / d_target / dX within TOL64, every flipped decision a
     tie, and dW per layer and per COLUMN within 1e-5 |want| + 1e-4 x the column's max, dB per layer
     within 1e-5 |want| + 1e-4 x the layer's max. (The whole-tensor bar alone leaves a layer 2^-40
     below the loudest one unchecked: test_scale_workloads.py.) The unscaled workloads go through the
     same check.
  B. against the unscaled run on the same path, bit for bit: loss, acc, d_dists, d_target, dX, the
     ReLU masks, dW[l] / fW[l] and dB[l] / fB[l] (np.ldexp on float32), +0 in every padded entry,
     last_path, guard_fired (0 under the default flags) and the exceptional-row counts.
GENERIC on (a), (d) and (d) under a 20-output head: the C oracle at 2e-6 per layer, and B.
Forward only, (d) and (e): lnerf_render on kr, on k16's bf16 forward and in fp16x3, and
lnerf_render_maps' rgba / weights / depth / opacity in fp16x3 and bf16x6, each bit-identical to its
unscaled run. mlp_fit_step (HEAD_FIT): outputs and loss bit-identical, gradients exactly rescaled,
float64 at test_gpu_fit's bar per layer. The measured worst ratios are in DESIGN.md §5.
"""
import numpy as np
import pytest

import scale_workloads as sw
from fused_parity import check_fused
from loma_calls import assert_close

pytestmark = pytest.mark.gpu

PATHS = {"default": 0, "f16x3": 256, "bf16x6": 512, "w4": 4096}   # lnerf.MFMA_F16X3, MFMA_BF16X6, K16_W4
STEP_MODES = [(n, sw.base(n)[1]) for n in sw.WORKLOADS] + [(n, "rays") for n in sw.RAYS_WORKLOADS]
STEP_CASES = [(n, p, m) for n, m in STEP_MODES for p in sw.PATTERNS if (n, p) in sw.PAIRS]
WORST = {}     # path -> [worst dW / column bar, worst dB / layer bar] over the cases run so far


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _expected_path(prec):
    import lnerf
    planes = 3 if prec & lnerf.MFMA_BF16X6 else 2
    return dict(generic=False, fused=True, k16=True, dw16=True, kr=False, k16_w4=bool(prec & lnerf.K16_W4),
                planes=planes, a24=planes == 2)


def _padding_is_plus_zero(a, shapes, name):
    """Every entry of the padded (L, K, N) / (L, N) array outside the layers' own blocks is +0."""
    pad = np.ones(a.shape, bool)
    for l, (k, n) in enumerate(shapes):
        if a.ndim == 3:
            pad[l, :k, :n] = False
        else:
            pad[l, :n] = False
    assert (a[pad] == 0).all() and not np.signbit(a[pad]).any(), name


_STEPS = {}


def _step(engine, name, pattern, mode, path):
    """One checked step (assertion A) of a (workload, pattern or None, input mode, path); kept for the
    run-against-run comparisons. What the engine reports is read right after the step (c_oracle=False:
    check_fused runs the GPU once)."""
    key = (name, pattern, mode, path)
    if key not in _STEPS:
        w, lw, lb = sw.scaled(name, pattern)
        shapes = [x.shape for x in w.ws]
        prec = PATHS[path]
        got, stats = check_fused(engine, w, points=mode != "encoded", seed=None, flags=prec,
                                 want_dx=mode == "encoded", rays32=sw.rays32(w) if mode == "rays" else None,
                                 c_oracle=False, per_layer=True)
        got["last_path"] = engine.last_path()
        got["guard_fired"] = engine.guard_fired()
        got["exceptional_rows"] = engine.exceptional_rows(split=True)
        assert got["last_path"] == _expected_path(prec), got["last_path"]
        _padding_is_plus_zero(got["dW"], shapes, "dW")
        _padding_is_plus_zero(got["dB"], shapes, "dB")
        if name == "c":   # the head's columns 4.. are never seeded: sums of exact zeros
            assert (got["dW"][-1][:, 4:] == 0).all() and (got["dB"][-1][4:] == 0).all()
        worst = WORST.setdefault(path, [0.0, 0.0])
        worst[0] = max(worst[0], stats["dW_over_col_bar"])
        worst[1] = max(worst[1], stats["dB_over_layer_bar"])
        print(f"scale step {name}-{pattern}-{mode}-{path}: dW / column bar {stats['dW_over_col_bar']:.3g}, "
              f"dB / layer bar {stats['dB_over_layer_bar']:.3g}, flips {stats['flips_vs_f64']}, guard "
              f"{got['guard_fired']}, exceptional rows {got['exceptional_rows']}; worst so far on {path}: "
              f"{worst[0]:.3g}, {worst[1]:.3g}")
        got["log2_f"] = (lw, lb)
        _STEPS[key] = got
    return _STEPS[key]


def _assert_same_step(a, b, dx):
    """Assertion B: a (rescaled) against b (unscaled), bit for bit."""
    assert a["loss"] == b["loss"], (a["loss"], b["loss"])
    for k in ("acc", "d_dists", "d_target") + (("dX",) if dx else ()):
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
    for l, (ma, mb) in enumerate(zip(a["masks"], b["masks"])):
        assert np.array_equal(ma, mb), (l, int((ma != mb).sum()))
    lw, lb = a["log2_f"]
    for k, e in (("dW", lw), ("dB", lb)):
        back = sw.unscale(a[k], e)
        for l in range(len(e)):
            diff = back[l] != b[k][l]
            assert not diff.any(), (k, l, int(diff.sum()), float(np.abs(back[l][diff].astype(np.float64) / b[k][l][diff] - 1).max()))
    assert a["last_path"] == b["last_path"]
    assert a["guard_fired"] == b["guard_fired"], (a["guard_fired"], b["guard_fired"])
    assert a["exceptional_rows"] == b["exceptional_rows"], (a["exceptional_rows"], b["exceptional_rows"])


# ---- the training step ----------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name,mode", STEP_MODES, ids=lambda v: v)
def test_unscaled_step_per_column(engine, name, mode, path):
    """The per-column and per-layer bars hold at scale 1 (and this is the run the rescaled ones are
    compared with)."""
    import lnerf
    assert PATHS == dict(default=0, f16x3=lnerf.MFMA_F16X3, bf16x6=lnerf.MFMA_BF16X6, w4=lnerf.K16_W4)
    got = _step(engine, name, None, mode, path)
    assert got["guard_fired"] == (0 if path == "default" else -1)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "-".join(c))
def test_rescaled_step(engine, case, path):
    name, pattern, mode = case
    got = _step(engine, name, pattern, mode, path)           # A
    assert got["guard_fired"] == (0 if path == "default" else -1)
    _assert_same_step(got, _step(engine, name, None, mode, path), mode == "encoded")   # B


# ---- the generic path -----------------------------------------------------------------------------

GENERIC_TOL = dict(rtol=2e-6, atol_scale=2e-6)    # test_gpu_native.test_generic_native_matches_oracle
_GENERIC = {}


def _generic_workload(name, pattern):
    if name != "head20":
        w, lw, lb = sw.scaled(name, pattern)
        return w, lw, lb, sw.base(name)[1]
    w = sw.head20_workload()
    if pattern is None:
        return w, [0] * len(w.ws), [0] * len(w.ws), "points"
    g = sw.log2_gains(pattern, len(w.ws))
    lw, lb = sw.factors(g, len(w.ws))
    return sw.rescale(w, g)[0], lw, lb, "points"


def _generic(engine, oracle_lib, name, pattern):
    key = (name, pattern)
    if key in _GENERIC:
        return _GENERIC[key]
    import lnerf
    import torch
    w, lw, lb, mode = _generic_workload(name, pattern)
    shapes = [x.shape for x in w.ws]
    dx = mode == "encoded"
    mlp = lnerf.make_mlp(shapes, w.wp.shape[1], w.wp.shape[2])
    x = _dev(w.X if dx else w.pts32.reshape(-1, 3))
    r = engine.train_step(mlp, _dev(w.wp), _dev(w.bp), x, _dev(w.dists), _dev(w.target), samples=w.S,
                          input_mode=lnerf.INPUT_ENCODED if dx else lnerf.INPUT_POINTS, num_freqs=w.F,
                          seed=None, flags=lnerf.GENERIC, want_per_ray=True, want_dx=dx)
    torch.cuda.synchronize()
    path = engine.last_path()
    assert path["generic"] and not path["fused"], path
    got = dict(loss=float(r.loss.item()), acc=r.acc_color.cpu().numpy(), dW=r.d_ws.cpu().numpy(),
               dB=r.d_bs.cpu().numpy(), d_dists=r.d_dists.cpu().numpy(), d_target=r.d_target.cpu().numpy(),
               last_path=path, log2_f=(lw, lb))
    if dx:
        got["dX"] = r.d_x.cpu().numpy()
    X = sw.inputs(w, mode)[0]
    want = oracle_lib.standard_forward_backward(X, w.wp, w.bp, shapes, w.dists, w.target, w.S, seed=None, dX=dx)
    assert abs(got["loss"] - want["loss"]) <= 1e-5 * abs(want["loss"]), (got["loss"], want["loss"])
    for k in ("acc", "d_dists", "d_target") + (("dX",) if dx else ()):
        assert_close(k, got[k], want[k], **GENERIC_TOL)
    for l in range(len(shapes)):
        assert_close(f"dW[{l}]", got["dW"][l], want["dW"][l], **GENERIC_TOL)
        assert_close(f"dB[{l}]", got["dB"][l], want["dB"][l], **GENERIC_TOL)
    _padding_is_plus_zero(got["dW"], shapes, "dW")
    _padding_is_plus_zero(got["dB"], shapes, "dB")
    _GENERIC[key] = got
    return got


@pytest.mark.parametrize("pattern", list(sw.PATTERNS))
@pytest.mark.parametrize("name", ["a", "d", "head20"])
def test_generic_step(engine, oracle_lib, name, pattern):
    a = _generic(engine, oracle_lib, name, pattern)
    b = _generic(engine, oracle_lib, name, None)
    assert a["loss"] == b["loss"]
    for k in ("acc", "d_dists", "d_target") + (("dX",) if "dX" in b else ()):
        assert np.array_equal(a[k], b[k]), k
    lw, lb = a["log2_f"]
    assert np.array_equal(sw.unscale(a["dW"], lw), b["dW"])
    assert np.array_equal(sw.unscale(a["dB"], lb), b["dB"])
    assert a["last_path"] == b["last_path"]


# ---- forward only ---------------------------------------------------------------------------------

FORWARD_PATTERNS = ("up24", "down24", "ramp8", "one_down40")
MAPS = ("rgba", "weights", "depth", "opacity")
_FORWARD = {}


def _forward_flags():
    import lnerf
    return {"render-kr": lnerf.FAST | lnerf.MFMA_BF16, "render-k16_bf16": lnerf.FAST | lnerf.MFMA_BF16 | lnerf.RENDER_K16,
            "render-fp16x3": lnerf.FAST, "maps-fp16x3": lnerf.FAST, "maps-bf16x6": lnerf.FAST | lnerf.MFMA_BF16X6}


FORWARD_KINDS = ("render-kr", "render-k16_bf16", "render-fp16x3", "maps-fp16x3", "maps-bf16x6")


def _forward(engine, name, pattern, kind):
    key = (name, pattern, kind)
    if key in _FORWARD:
        return _FORWARD[key]
    import lnerf
    import torch
    w = sw.scaled(name, pattern)[0]
    fl = _forward_flags()[kind]
    mlp = lnerf.make_mlp([x.shape for x in w.ws], w.wp.shape[1], w.wp.shape[2])
    x, dists = _dev(w.pts32.reshape(-1, 3)), _dev(w.dists)
    if kind.startswith("render"):
        loss, acc = engine.render(mlp, _dev(w.wp), _dev(w.bp), x, dists, _dev(w.target), samples=w.S,
                                  input_mode=lnerf.INPUT_POINTS, num_freqs=w.F, flags=fl)
        path = engine.last_path()
        torch.cuda.synchronize()
        out = dict(loss=np.float32(loss.item()), acc=acc.cpu().numpy().copy())
        assert path["kr"] == (kind == "render-kr") and path["fused"] and not path["generic"], path
        assert path["planes"] == (2 if kind == "render-fp16x3" else 1), path
    else:
        t = np.tile(np.linspace(2.0, 6.0, w.S).astype(np.float32), (w.N, 1))
        m = engine.render_maps(mlp, _dev(w.wp), _dev(w.bp), x, dists, None, samples=w.S, input_mode=lnerf.INPUT_POINTS,
                               num_freqs=w.F, sample_t=_dev(t), flags=fl, want=MAPS)
        path = engine.last_path()
        torch.cuda.synchronize()
        out = {k: getattr(m, k).cpu().numpy().copy() for k in MAPS}
        assert path.get("maps") and path["k16"] and path["planes"] == (3 if kind == "maps-bf16x6" else 2), path
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    assert np.abs(out["acc" if "acc" in out else "opacity"]).max() > 0.01   # a picture, not a blank
    out["last_path"] = path
    _FORWARD[key] = out
    return out


@pytest.mark.parametrize("kind", FORWARD_KINDS)
@pytest.mark.parametrize("pattern", FORWARD_PATTERNS)
@pytest.mark.parametrize("name", ["d", "e"])
def test_forward_only(engine, name, pattern, kind):
    a, b = _forward(engine, name, pattern, kind), _forward(engine, name, None, kind)
    assert a["last_path"] == b["last_path"]
    for k in b:
        if k != "last_path":
            assert np.array_equal(a[k], b[k]), (k, float(np.abs(np.asarray(a[k], np.float64) - b[k]).max()))


# ---- mlp_fit_step (HEAD_FIT) -------------------------------------------------------------------------

FIT_CASE = (22, 4, 300)     # test_gpu_fit.HEAD_CASES: whole tiles and a ragged third one, the widest head


def _fit(engine, wp, bp, shapes, X, T, seed):
    import lnerf
    import torch
    mlp = lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2])
    loss, out, g = engine.mlp_fit_step(mlp, _dev(wp), _dev(bp), _dev(X), _dev(T), seed=seed, flags=lnerf.FAST)
    torch.cuda.synchronize()
    path = engine.last_path()
    assert path["k16"] and path["dw16"] and path["planes"] == 2, path
    gd = g.cpu().numpy()
    return dict(loss=float(loss), out=out.cpu().numpy(), dW=gd[:wp.size].reshape(wp.shape).copy(),
                dB=gd[wp.size:-1].reshape(bp.shape).copy(), last_path=path)


@pytest.mark.parametrize("pattern", ["up24", "down24"])
def test_mlp_fit_step(engine, pattern):
    import scene
    from test_gpu_fit import HEAD_CASES, TOL, f64_fit
    assert FIT_CASE in HEAD_CASES
    k0, n_out, rows = FIT_CASE
    shapes, wp, bp = scene.init_mlp(k0, n_out, 3, 16, seed=215)
    rng = np.random.RandomState(1000 * k0 + 10 * n_out + rows)
    X = rng.uniform(-1, 1, (rows, k0)).astype(np.float32)
    T = rng.uniform(0, 1, (rows, n_out)).astype(np.float32)
    seed = 1.7
    wq, bq, lw, lb = sw.rescale_padded(wp, bp, shapes, sw.log2_gains(pattern, len(shapes)))
    for l, (k, n) in enumerate(shapes):   # the rescale is exact
        assert np.array_equal(wq[l].astype(np.float64) * 2.0 ** lw[l], wp[l].astype(np.float64))
        assert np.array_equal(bq[l].astype(np.float64) * 2.0 ** lb[l], bp[l].astype(np.float64))
    b = _fit(engine, wp, bp, shapes, X, T, seed)
    a = _fit(engine, wq, bq, shapes, X, T, seed)
    for got, (ws_, bs_) in ((b, (wp, bp)), (a, (wq, bq))):
        want_loss, want_out, want_dW, want_dB = f64_fit(X, T, ws_, bs_, shapes, seed)
        assert abs(got["loss"] - want_loss) <= TOL["rtol"] * abs(want_loss), (got["loss"], want_loss)
        assert_close("outputs", got["out"], want_out, **TOL)
        for l in range(len(shapes)):
            assert np.abs(want_dW[l]).max() > 0
            assert_close(f"dW[{l}]", got["dW"][l], want_dW[l], **TOL)
            assert_close(f"dB[{l}]", got["dB"][l], want_dB[l], **TOL)
    assert a["loss"] == b["loss"] and np.array_equal(a["out"], b["out"])
    assert np.array_equal(sw.unscale(a["dW"], lw), b["dW"])
    assert np.array_equal(sw.unscale(a["dB"], lb), b["dB"])
    assert a["last_path"] == b["last_path"]
