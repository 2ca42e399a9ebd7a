"""Every hidden-tile instantiation of the fused kernels against float64 (tests/tile_workloads.py;
tests/test_tile_workloads.py holds the CPU conditions that make these runs worth doing, and the proof
that the 25 cells reach every ht16, every to16_b[0], kr's k0 <= 64 boundary and every dW block shape).

k16_launch and kr_launch switch on ht16 = pow2_16(ceil(max hidden width / 16)), so HT in {1, 2, 4, 8,
16} crossed with the operand planes, the sample tile and the three translation units (plain, MAPS,
VJP) is some 75 kernels, and every other sweep in tests/ holds the hidden width at 30. The cells are
HT x T0 (layer-0 input tiles), k0 -> 16 HT -> 8 HT + 1 -> 16 HT -> 4 on 4 rays x 40 samples.

  1. Training step, 25 cells x {default = guarded fp16x3, MFMA_F16X3, MFMA_BF16X6, K16_W4}, seed 1,
     with d_x (the layer-0 backward pass then runs with to16_b[0] tiles): fused_parity.check_fused
     with per_layer -- loss 1e-6, ray outputs and dX within TOL64, dW per layer and column within
     1e-5 |want| + 1e-4 x the column's max, dB per layer, every ReLU decision float64's or a tie, then
     the C oracle within TOLC with no ray set aside. last_path shows the planes and the tile
     tile_workloads.plan predicts, guard_fired is 0 on the default path, and a second run gives the
     same bits.
  2. The ten T0 > HT cells under the down24 gains, default and MFMA_F16X3: the same bars, and the
     unscaled run bit for bit (test_gpu_scale's check B, its own helper).
  3. bf16 renders of every cell: kr (k0 <= 64) and RENDER_K16 within 3e-4 of the float64 sums of
     bf16-rounded operands and within bf16_render_bound of float64, kr against k16 within 2e-5; the
     fp16x3 forward render within 1e-5 of float64. last_path's kr bit is plan's.
  4. MAPS objects, each HT at T0 = 2 and 16 (so kr and its k16 fallback both run) on kr, RENDER_K16
     and the fp16x3 forward: colour and loss are lnerf_render's bits; weights, depth, opacity and
     colour within test_gpu_render_maps' compositing bars of float64 from the returned rgba; the
     fp16x3 rgba within TOL64 of float64, kr's rgba within 2e-5 of k16's.
  5. VJP objects, each HT at T0 = 2 and 16: with d_acc_color = fp32(2 (C - target)) alone the call is
     the seed-1 training step bit for bit (test_gpu_render_vjp's check A) in the default precision,
     MFMA_F16X3, MFMA_BF16X6 and MFMA_BF16; in the default precision each adjoint kind and all five
     together against render_vjp_ref at check B's bars.

Every test prints the worst error / bar so far per quantity and path. Measured on an MI355X (the
table is in DESIGN.md section 5, "Hidden-tile instantiations"): the step, worst over the four paths,
loss 0.181 of 1e-6, acc 0.0098, d_dists 0.095, d_target 0.018, dX 0.050, dW 0.041 of the column
bar, dB 0.017; no decision flipped and no ray set aside in 120 steps; renders kr 4.9e-4 and k16
0.042 of 3e-4, 0.21 of bf16_render_bound, kr vs k16 0.0054, fp16x3 0.0099 of 1e-5; maps weights
0.047, opacity 0.020, depth 0.025, colour 0.023, fp16x3 rgba 0.038; VJP dW 0.062, dB 0.015, d_dists
0.11, d_x 0.16, acc 0.0098. Three mutations of the kernels (layer-0 tiles past HT left in place;
the bias of tile 7 skipped at HT = 8 in k16; the ReLU of tile 3 skipped at HT = 4 in kr) each turn
these tests red; the last two left every earlier GPU test green.
"""
import functools

import numpy as np
import pytest

import nerf_np
import tile_workloads as tw
import width_workloads as ww
from fused_parity import TOL64, check_fused, run_fused

pytestmark = pytest.mark.gpu

PATHS = {"default": 0, "f16x3": tw.MFMA_F16X3, "bf16x6": tw.MFMA_BF16X6, "w4": tw.K16_W4}
TWO_T0 = [(ht, t0) for ht in tw.TILES for t0 in (2, 16)]       # kr runs at k0 = 29, k16 at k0 = 253
WORST = {}      # (what, path, quantity) -> worst error / bar over the cases run so far
_STEPS = {}


def _note(what, path, ratios):
    for k, v in ratios.items():
        WORST[(what, path, k)] = max(WORST.get((what, path, k), 0.0), float(v))
    print(f"worst error / bar so far, {what} {path}: " +
          ", ".join(f"{k} {v:.3g}" for (a, b, k), v in sorted(WORST.items()) if (a, b) == (what, path)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flags_are_lnerfs():
    import lnerf
    assert (tw.MFMA_BF16, tw.MFMA_F16X3, tw.MFMA_BF16X6, tw.K16_W4, tw.HEAD_FIT, tw.RENDER_K16) == \
        (lnerf.MFMA_BF16, lnerf.MFMA_F16X3, lnerf.MFMA_BF16X6, lnerf.K16_W4, lnerf.HEAD_FIT, lnerf.RENDER_K16)


# ---- 1, 2. the training step ---------------------------------------------------------------------

def _step(engine, c, scaled, path):
    """One checked step of a cell (or of the cell under the down24 gains) on a path, kept for the
    run-against-run comparison. The context's reports are read right after check_fused, which runs
    the GPU once when no ray is set aside -- and none may be."""
    key = (c, scaled, path)
    if key in _STEPS:
        return _STEPS[key]
    _flags_are_lnerfs()
    w, lw, lb = tw.scaled(*c) if scaled else (tw.cell(*c), [0] * 4, [0] * 4)
    prec = PATHS[path]
    kw = dict(points=False, seed=1.0, flags=prec, want_dx=True)
    got, stats = check_fused(engine, w, per_layer=True, **kw)
    got["last_path"] = engine.last_path()
    got["guard_fired"] = engine.guard_fired()
    got["exceptional_rows"] = engine.exceptional_rows(split=True)
    got["log2_f"] = (lw, lb)
    assert stats["rays_vs_c_oracle_set_aside"] == 0, stats
    assert stats["flips_vs_f64"] == 0, stats            # no tie to flip (test_tile_workloads.py)
    p = tw.cell_plan(c, prec)
    assert (p["ht16"], p["to16_b0"]) == c
    assert got["last_path"] == dict(generic=False, fused=True, k16=True, dw16=True, kr=False,
                                    k16_w4=p["tile"] == 64, planes=p["planes"], a24=p["planes"] == 2), got["last_path"]
    assert got["guard_fired"] == (0 if path == "default" else -1), got["guard_fired"]
    assert got["dX"].shape == (w.N * w.S, w.X.shape[1])
    # the figures check_fused asserted on, for the record
    ref = nerf_np.nerf_forward_backward(w.X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0, masks=got["masks"])
    ratios = dict(loss=abs(got["loss"] - ref["loss"]) / (1e-6 * abs(ref["loss"])),
                  dW=stats["dW_over_col_bar"], dB=stats["dB_over_layer_bar"])
    for k in ("acc", "d_dists", "d_target", "dX"):
        ratios[k] = ww.violation(got[k], ref[k], **TOL64)
    _note("scaled step" if scaled else "step", path, ratios)
    # a second run: the same bits
    again = run_fused(engine, w, **kw)
    assert again["loss"] == got["loss"]
    for k in ("acc", "dW", "dB", "d_dists", "d_target", "dX"):
        assert np.array_equal(_bits(again[k]), _bits(got[k])), k
    for l, (ma, mb) in enumerate(zip(again["masks"], got["masks"])):
        assert np.array_equal(ma, mb), l
    _STEPS[key] = got
    return got


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("c", tw.CELLS, ids=tw.cell_id)
def test_step(engine, c, path):
    _step(engine, c, False, path)


@pytest.mark.parametrize("path", ["default", "f16x3"])
@pytest.mark.parametrize("c", tw.WIDE_INPUT_CELLS, ids=tw.cell_id)
def test_scaled_step_with_a_wide_input(engine, c, path):
    """T0 > HT: layer 0 leaves its tiles past HT in the registers. Under the down24 gains a row shift
    that followed them would keep no bits of activations 2^-24 below the input."""
    from test_gpu_scale import _assert_same_step
    a = _step(engine, c, True, path)
    _assert_same_step(a, _step(engine, c, False, path), True)


# ---- 3. the renders -------------------------------------------------------------------------------

@pytest.mark.parametrize("c", tw.CELLS, ids=tw.cell_id)
def test_renders(engine, c):
    import lnerf
    from test_gpu_render import bf16_render_bound, render_np
    from test_gpu_widths import _render
    _flags_are_lnerfs()
    w = tw.cell(*c)
    k0 = w.X.shape[1]
    fl = lnerf.FAST | lnerf.MFMA_BF16
    emu, _ = render_np(w.X, w.ws, w.bs, w.dists, w.S, operands="bf16")
    ref, _ = render_np(w.X, w.ws, w.bs, w.dists, w.S)
    bound = bf16_render_bound(w.X, w.ws, w.bs, w.dists, w.S, ref)
    la, a, pa = _render(engine, w, None, "encoded", fl)
    lb, b, pb = _render(engine, w, None, "encoded", fl | lnerf.RENDER_K16)
    assert pa["kr"] == tw.cell_plan(c, tw.MFMA_BF16)["kr"] == (k0 <= 64), pa
    assert not pb["kr"] and not tw.cell_plan(c, tw.MFMA_BF16 | tw.RENDER_K16)["kr"], pb
    for p in (pa, pb):
        assert p["planes"] == 1 and p["k16"] and p["fused"] and not p["generic"], p
    ratios = {}
    for name, got in (("kr" if pa["kr"] else "k16", a), ("k16", b)):
        assert np.isfinite(got).all()
        err_emu, err = np.abs(got - emu), np.abs(got - ref)
        ratios[f"{name} vs bf16 operands / 3e-4"] = err_emu.max() / 3e-4
        ratios[f"{name} vs float64 / bound"] = (err / bound).max()
        assert err_emu.max() <= 3e-4, (name, err_emu.max())
        assert (err <= bound).all(), (name, float((err / bound).max()))
    if pa["kr"]:
        ratios["kr vs k16 / (2e-5 |b| + 2e-6)"] = (np.abs(a - b) / (2e-5 * np.abs(b) + 2e-6)).max()
        np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-6)
        assert abs(la - lb) <= 1e-4 * abs(lb)
    else:       # the same kernel both times
        assert np.array_equal(a, b) and la == lb
    lf, f, pf = _render(engine, w, None, "encoded", lnerf.FAST)
    assert not pf["kr"] and pf["planes"] == 2 and pf["k16"] and not pf["generic"], pf
    ratios["fp16x3 vs float64 / 1e-5"] = np.abs(f - ref).max() / 1e-5
    assert np.abs(f - ref).max() <= 1e-5, float(np.abs(f - ref).max())
    _note("render", "all", ratios)


# ---- 4. the MAPS objects --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rgba64(c):
    from test_gpu_render_maps import _rgba64 as rgba64
    w = tw.cell(*c)
    return rgba64(w.X, w.ws, w.bs, w.dists, w.target, w.S)


@pytest.mark.parametrize("path", ["kr", "k16_bf16", "fp16x3"])
@pytest.mark.parametrize("c", TWO_T0, ids=tw.cell_id)
def test_maps_objects(engine, c, path):
    import lnerf
    import test_gpu_render_maps as rm
    fl = rm._flags()[path]
    w = tw.cell(*c)
    inp = rm._inputs(w, lnerf.INPUT_ENCODED)
    loss, acc, rpath = rm.run_render(engine, inp, fl)
    out, mpath = rm.run_maps(engine, inp, fl)
    assert mpath == {**rpath, "maps": True}, (mpath, rpath)
    p = tw.cell_plan(c, fl)
    assert mpath["kr"] == p["kr"] == (path == "kr" and c[1] == 2) and mpath["planes"] == p["planes"], mpath
    assert mpath["k16"] and mpath["fused"] and not mpath["generic"], mpath
    assert np.array_equal(_bits(out["color"]), _bits(acc))
    assert out["loss"][0] == loss, (out["loss"][0], loss)
    ratios = rm.compositing_ratios(out, inp)
    if path == "fp16x3":
        want = _rgba64(c)
        ratios["rgba"] = max(ww.violation(out["rgba"][:, ch], want[:, ch], **TOL64) for ch in range(4))
        rm._assert_tol64(out["rgba"], want)
    elif mpath["kr"]:
        b, pb = rm.run_maps(engine, inp, rm._flags()["k16_bf16"], want=("rgba",), target=False)
        assert not pb["kr"]
        atol = 2e-6 * max(1.0, np.abs(b["rgba"][:, 3]).max())
        ratios["rgba vs k16"] = (np.abs(out["rgba"] - b["rgba"]) / (2e-5 * np.abs(b["rgba"]) + atol)).max()
        np.testing.assert_allclose(out["rgba"], b["rgba"], rtol=2e-5, atol=atol)
    _note("maps", path if mpath["kr"] or path != "kr" else "kr -> k16", ratios)


# ---- 5. the VJP objects ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _vjp_job(c):
    """test_gpu_render_vjp.job for a cell: ENCODED input, sorted random depths."""
    import lnerf
    import render_vjp_workloads as wl
    from test_gpu_render_vjp import _dev
    w = tw.cell(*c)
    case = wl.Case(tw.cell_id(c), w, "encoded", w.X, w.X, w.dists, wl._sorted_t(w.N, w.S, 3))
    return dict(c=case, mlp=lnerf.make_mlp([x.shape for x in w.ws], w.wp.shape[1], w.wp.shape[2]), ws=_dev(w.wp),
                bs=_dev(w.bp), x=_dev(w.X), dists=_dev(w.dists), target=_dev(w.target), sample_t=_dev(case.t),
                mode=lnerf.INPUT_ENCODED, S=w.S, N=w.N, F=0, L=len(w.ws))


@pytest.mark.parametrize("prec", ["default", "f16x3", "bf16x6", "bf16"])
@pytest.mark.parametrize("c", TWO_T0, ids=tw.cell_id)
def test_vjp_color_adjoint_equals_train_step(engine, c, prec):
    import test_gpu_render_vjp as tv
    j = _vjp_job(c)
    flags = tv._precisions()[prec]
    step = tv.run_step(engine, j, flags, "dx")
    p = tw.cell_plan(c, flags)
    assert step["path"]["k16"] and step["path"]["dw16"] and not step["path"]["generic"], step["path"]
    assert step["path"]["planes"] == p["planes"] == dict(default=2, f16x3=2, bf16x6=3, bf16=1)[prec]
    vjp = tv.run_vjp(engine, j, dict(color=tv.color_adjoint(step, j["c"].w.target)), flags, "dx")
    tv.assert_same_bits(step, vjp)
    assert np.abs(step["dW"]).max() > 0 and np.abs(step["d_dists"]).max() > 0 and np.abs(step["dX"]).max() > 0


@pytest.mark.parametrize("c", TWO_T0, ids=tw.cell_id)
def test_vjp_each_adjoint_against_float64(engine, c):
    import render_vjp_ref as ref
    import test_gpu_render_vjp as tv
    j = _vjp_job(c)
    case = j["c"]
    full = ref.random_adjoints(case.w.N, case.w.S, tv.ADJ_SEED)
    for kind in tv.KINDS_B:
        adj = full if kind == "all" else {kind: full[kind]}
        got = tv.run_vjp(engine, j, adj, tv._precisions()["default"], "dx")
        assert got["path"]["k16"] and got["path"]["planes"] == 2 and not got["path"]["generic"], got["path"]
        tv.check_against_f64(case, got, adj, "tiles", "dx")
    _note("vjp", "default", {k: v for (p, k), v in tv.WORST.items() if p == "tiles"})
