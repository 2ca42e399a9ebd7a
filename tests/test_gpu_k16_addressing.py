"""k1's and kr's LDS-DMA pieces and slab stores from scalar bases (loma-nerf_amd/csrc/lnerf_wave_addr.h):
one small shape per addressing path, each against the float64 oracle and each run twice, bit for bit.

The change is addressing only, so what can go wrong is a piece or a store landing somewhere else: a
weight fragment, a bias, an A or G slab row that k2 then reads. Every shape reaches a path the others do
not:

  ragged   2 rays x 5 samples, 33 -> 24 -> 40 -> 4, RAYS, fp16x3 and bf16x6: ragged widths (partial chunks
           of 4 and 6 KiB: one piece on some waves, none on others), a tile with 10 of 128 samples
           valid, int24 (fp16x3) and f32 (bf16x6) A slabs; bf16x6 is the staggered ring that issues its
           chunks whole
  full     3 rays x 64 samples, 33 -> 256 -> 256 -> 4, fp16x3: FULL hidden passes whose pieces take their
           source from the pass base, a half-filled second tile, bias pieces
  encoded  4 rays x 8 samples, ENCODED input 70 wide, 48-wide layers, d_x requested: the tile-by-tile input
           path, three layer-0 k-steps, the backward layer-0 pass that also writes the G_0 slab
  w4       the ragged batch on the 4-wave ring (K16_W4)
  deep     12 layers x 16 wide, 2 rays x 4 samples: a long chunk table of one-chunk passes
  render   a 16 x 16 frame x 16 samples: kr, RENDER_K16 (k16's bf16 forward) and the fp16x3 forward
  maps     one small render_maps call (the MAPS objects of k16 and kr) and one render_maps_vjp call

Bars: fused_parity.check_fused with per_layer=True -- loss within 1e-6, colours and the ray outputs within
TOL64 (1e-5 |want| + 1e-5 max|want|), dW per layer and column within 1e-5 |want| + 1e-4 x the column's max,
dB per layer likewise -- against float64 at the GPU's own ReLU decisions, then the C oracle. The bf16
render cannot meet a 1e-5 bar against float64 (its operands keep 8 significant bits, whatever the kernel):
it is held to test_gpu_render's bars, which come from that format (the float64 sums of kr's own bf16-rounded
operands within 3e-4, plain float64 within bf16_render_bound), kr and k16's bf16 forward to each other
within 2e-5, and the fp16x3 forward of the same frame to 1e-5 against float64.
"""
import functools

import numpy as np
import pytest

import nerf_np
import width_workloads as ww
from fused_parity import check_fused, run_fused

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _workload(dims, rays, samples, seed, F):
    """width_workloads' recipe (He-scaled weights, hidden biases in [0.1, 0.6], a small positive sigma
    column, X uniform in [-1, 1], dists 4 / (S - 1) with 1e8 last) under any widths."""
    ws, bs, X, dists, target = ww._recipe(list(dims), rays, samples, seed)
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(None, None, X, dists, target, ws, bs, wp, bp, F, samples, rays)


RAGGED = ((33, 24, 40, 4), 2, 5, 3, 5)
FULL = ((33, 256, 256, 4), 3, 64, 2, 5)
ENCODED = ((70, 48, 48, 4), 4, 8, 1, 0)
DEEP = ((33,) + (16,) * 11 + (4,), 2, 4, 1, 5)

# (id, workload, input, flags by name, d_x)
CASES = [
    ("ragged-fp16x3", RAGGED, "rays", (), False),
    ("ragged-bf16x6", RAGGED, "rays", ("MFMA_BF16X6",), False),
    ("full-fp16x3", FULL, "rays", (), False),
    ("encoded70-dx", ENCODED, "encoded", (), True),
    ("ragged-w4", RAGGED, "rays", ("K16_W4",), False),
    ("deep12x16", DEEP, "rays", (), False),
]


@pytest.mark.parametrize("name,spec,mode,flag_names,want_dx", CASES, ids=[c[0] for c in CASES])
def test_train_step_paths(engine, name, spec, mode, flag_names, want_dx):
    import lnerf
    w = _workload(*spec)
    flags = 0
    for f in flag_names:
        flags |= getattr(lnerf, f)
    rays32 = ww.select_rays32(w.N) if mode == "rays" else None
    got, stats = check_fused(engine, w, points=mode != "encoded", seed=None, flags=flags, want_dx=want_dx,
                             rays32=rays32, per_layer=True)
    path = engine.last_path()
    planes = 3 if "MFMA_BF16X6" in flag_names else 2
    assert path["k16"] and path["dw16"] and not path["generic"] and path["planes"] == planes, path
    assert path["k16_w4"] == ("K16_W4" in flag_names) and path["a24"] == (planes == 2), path
    # the batch is alive in every layer (a dead one would pass any parity check)
    for l, (k, n) in enumerate(x.shape for x in w.ws):
        assert np.abs(got["dW"][l, :k, :n]).max() > 0, f"layer {l}: dW is all zeros"
    if want_dx:
        assert got["dX"].shape == (w.N * w.S, w.ws[0].shape[0]) and np.abs(got["dX"]).max() > 0
    # the same call again: every output bit for bit
    again = run_fused(engine, w, points=mode != "encoded", seed=None, flags=flags, want_dx=want_dx, rays32=rays32)
    assert _bits(np.float32(again["loss"])) == _bits(np.float32(got["loss"]))
    for k in ("acc", "dW", "dB", "d_dists", "d_target") + (("dX",) if want_dx else ()):
        same = _bits(again[k]) == _bits(got[k])
        assert same.all(), f"{k}: {(~same).sum()} of {same.size} values differ between two runs"
    for a, b in zip(again["masks"], got["masks"]):
        assert np.array_equal(a, b)
    print(f"{name}: {stats}")


# ---- the render: kr, k16's bf16 forward, the fp16x3 forward ------------------------------------------

@functools.lru_cache(maxsize=None)
def _frame():
    """A 16 x 16 frame (every ray of it) x 16 samples under cfg2's camera and a 33 -> 256 -> 256 -> 4 MLP."""
    side, S = 16, 16
    focal = 0.5 / np.tan(0.5 * 0.6911112)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]]).astype(np.float32)
    o, d = nerf_np.get_rays(side, side, K, nerf_np.look_at_pose())
    rays32 = np.concatenate([o, d], axis=1).astype(np.float32)
    w = _workload((33, 256, 256, 4), side * side, S, 2, 5)
    from fused_parity import rays_reference
    X, dists = rays_reference(rays32, S, 5)
    return w, rays32, np.asarray(X, np.float32), dists


def _render(engine, w, rays32, flags):
    import lnerf
    import torch
    mlp = lnerf.make_mlp([x.shape for x in w.ws], w.wp.shape[1], w.wp.shape[2])
    loss, acc = engine.render(mlp, _dev(w.wp), _dev(w.bp), _dev(rays32), None, _dev(w.target), samples=w.S,
                              input_mode=lnerf.INPUT_RAYS, num_freqs=w.F, flags=flags)
    path = engine.last_path()
    torch.cuda.synchronize()
    return np.float32(loss.item()), acc.cpu().numpy().copy(), path


def test_render_frame_16x16(engine):
    import lnerf
    from test_gpu_render import bf16_render_bound, render_np
    w, rays32, X, dists = _frame()
    ref, _ = render_np(X, w.ws, w.bs, dists, w.S)
    emu, _ = render_np(X, w.ws, w.bs, dists, w.S, operands="bf16")
    bound = bf16_render_bound(X, w.ws, w.bs, dists, w.S, ref)
    loss_ref = float(((ref - w.target.astype(np.float64)) ** 2).sum())
    assert ref.min() > 1e-3 and ref.max() < 1 - 1e-3 and np.ptp(ref) > 0.05, "a frame with something on it"
    out = {}
    for name, fl, kr in (("kr", lnerf.FAST | lnerf.MFMA_BF16, True),
                         ("k16_bf16", lnerf.FAST | lnerf.MFMA_BF16 | lnerf.RENDER_K16, False)):
        loss, acc, path = _render(engine, w, rays32, fl)
        assert path["kr"] == kr and path["k16"] and path["planes"] == 1 and not path["generic"], path
        err_emu, err = np.abs(acc - emu), np.abs(acc - ref)
        print(f"{name}: vs bf16-operand float64 max err {err_emu.max():.3g}; vs float64 max err {err.max():.3g}, "
              f"max err / bound {(err / bound).max():.3g}")
        assert np.isfinite(acc).all()
        assert err_emu.max() <= 3e-4, err_emu.max()
        assert (err <= bound).all(), float((err / bound).max())
        loss2, acc2, _ = _render(engine, w, rays32, fl)
        assert (_bits(acc2) == _bits(acc)).all() and _bits(loss2) == _bits(loss), f"{name}: two runs differ"
        out[name] = (loss, acc)
    np.testing.assert_allclose(out["kr"][1], out["k16_bf16"][1], rtol=2e-5, atol=2e-6)
    assert abs(out["kr"][0] - out["k16_bf16"][0]) <= 1e-4 * abs(out["k16_bf16"][0])
    # the fp32-class forward of the same frame (k16 fp16x3, forward only): 1e-5 against float64
    loss, acc, path = _render(engine, w, rays32, lnerf.FAST)
    assert path["k16"] and path["planes"] == 2 and not path["kr"] and not path["generic"], path
    err = np.abs(acc - ref)
    print(f"fp16x3: vs float64 max err {err.max():.3g}, loss {loss:.7g} vs {loss_ref:.7g}")
    assert (err <= 1e-5 * np.abs(ref) + 1e-5 * np.abs(ref).max()).all(), float(err.max())
    loss2, acc2, _ = _render(engine, w, rays32, lnerf.FAST)
    assert (_bits(acc2) == _bits(acc)).all() and _bits(loss2) == _bits(loss)


# ---- the other two translation units: render_maps and render_maps_vjp --------------------------------

def test_render_maps_small(engine):
    """7 rays x 7 samples through the MAPS objects: k16 fp16x3's rgba against float64 at TOL64's form, kr's
    against k16's bf16 forward, each twice."""
    import lnerf
    import test_gpu_render_maps as tm
    w = nerf_np.without_relu_ties(nerf_np.make_workload("cfg2", rays=7, samples=7))
    X = nerf_np.positional_encoding_3d(w.pts32.astype(np.float64), w.F).reshape(-1, 3 + 6 * w.F)
    want = tm._rgba64(X, w.ws, w.bs, w.dists, w.target, w.S)
    inp = tm._inputs(w, lnerf.INPUT_POINTS)
    out, path = tm.run_maps(engine, inp, tm._flags()["fp16x3"])
    assert path["k16"] and not path["generic"], path
    tm._assert_tol64(out["rgba"], want)
    tm.compositing_ratios(out, inp)
    again, _ = tm.run_maps(engine, inp, tm._flags()["fp16x3"])
    for k in out:
        assert (_bits(again[k]) == _bits(out[k])).all(), k
    a, pa = tm.run_maps(engine, inp, tm._flags()["kr"], want=("rgba", "color"), target=False)
    b, pb = tm.run_maps(engine, inp, tm._flags()["k16_bf16"], want=("rgba", "color"), target=False)
    assert pa["kr"] and not pb["kr"], (pa, pb)
    np.testing.assert_allclose(a["rgba"], b["rgba"], rtol=2e-5, atol=2e-6 * max(1.0, np.abs(b["rgba"][:, 3]).max()))
    a2, _ = tm.run_maps(engine, inp, tm._flags()["kr"], want=("rgba", "color"), target=False)
    assert (_bits(a2["rgba"]) == _bits(a["rgba"])).all() and (_bits(a2["color"]) == _bits(a["color"])).all()


def test_render_maps_vjp_small(engine):
    """30 rays x 5 samples (render_vjp_workloads "s5") through the VJP object: the colour adjoint reproduces
    the training step bit for bit, every adjoint together is within the float64 bars, twice the same bits."""
    import lnerf
    import render_vjp_ref as ref
    import test_gpu_render_vjp as tv
    j = tv.job("s5")
    step = tv.run_step(engine, j, lnerf.FAST, "dx")
    vjp = tv.run_vjp(engine, j, dict(color=tv.color_adjoint(step, j["c"].w.target)), lnerf.FAST, "dx")
    tv.assert_same_bits(step, vjp)
    assert np.abs(step["dW"]).max() > 0
    adj = ref.random_adjoints(j["N"], j["S"], tv.ADJ_SEED)
    got = tv.run_vjp(engine, j, adj, lnerf.FAST, "dx")
    assert got["path"]["k16"] and not got["path"]["generic"], got["path"]
    tv.check_against_f64("s5", got, adj, "default", "dx")
    again = tv.run_vjp(engine, j, adj, lnerf.FAST, "dx")
    for k in ("acc", "dW", "dB", "d_dists", "dX"):
        assert (_bits(again[k]) == _bits(got[k])).all(), k
