"""lnerf_render_maps_vjp (include/lnerf.h): the reverse of the render maps, seeded with the caller's
adjoints of colour, depth, opacity, sample weights and rgba -- on the fused path in every training
precision and on the generic path. An extension (the reference reverses its colour loss only).

Workloads: tests/render_vjp_workloads.py (tests/test_render_vjp_ref.py holds them to the conditions
that make these comparisons mean something, and the float64 reference to central differences).

  A  With d_acc_color = fp32(2 (acc_color - target)) formed on the host from the training step's own
     colour (exact: at seed 1 the kernel's a1 + a1 has no contraction choice) and every other adjoint
     NULL, every output has the bits of lnerf_train_step(LNERF_SEED_CONST, 1.0): d_ws with its padding,
     d_bs, d_dists, d_x (WANT_DX and WANT_DINPUT), acc_color, the ReLU masks, the exceptional rows and
     guard_fired -- under the default precision, MFMA_F16X3, MFMA_BF16X6, MFMA_BF16, GENERIC, with
     ACCUMULATE into a non-zero buffer, and on edge_finite_6x8, where the floor guard fires.
  B  depth, opacity, weights, rgba alone and all five together (unit-scale random adjoints) against
     tests/render_vjp_ref.py at the GPU's own ReLU decisions: dW per layer and column within
     1e-5 |want| + 1e-4 x the column's max, dB per layer (scale_workloads.assert_per_layer), d_dists and
     the encoded d_x at fused_parity.TOL64, d_x of POINTS / RAYS input within TOL64 carried through the
     encoding's reverse (input_grad_ref's L1 companions). The generic path has no mask readback: it is
     held to float64 at float64's own decisions by the same bars.
     Worst error / bar measured on an MI355X: see DESIGN.md section 5.
  C  A ray whose adjoints are all zero gets exact +0 in d_dists and its d_x rows while every other ray
     keeps its bits; NaN in sample_t without a depth adjoint changes no bit.
  D  The call contract: every refused flag and argument returns a negative code, sets lnerf_last_error
     and leaves poisoned outputs untouched; NULL outputs are fine; last_path carries LNERF_PATH_VJP.
  E  torch autograd through lnerf.render_maps_autograd: bit-identical to a direct render_maps_vjp call
     fed torch.autograd.grad of the same loss, and within B's bars of the float64 reference.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import input_grad_ref as igr
import render_vjp_ref as ref
import render_vjp_workloads as wl
from fused_parity import TOL64, padded
from loma_calls import assert_close
from scale_workloads import assert_per_layer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ADJ_SEED = 21          # the adjoints tests/test_render_vjp_ref.py vets the workloads with
POISON = -7.25
WORST = {}             # worst error / bar per (path, quantity), printed by every case B test


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _precisions():
    import lnerf
    return {"default": lnerf.FAST, "f16x3": lnerf.FAST | lnerf.MFMA_F16X3, "bf16x6": lnerf.FAST | lnerf.MFMA_BF16X6,
            "bf16": lnerf.FAST | lnerf.MFMA_BF16, "generic": lnerf.GENERIC}


@functools.lru_cache(maxsize=None)
def job(name):
    """The device-side inputs of a workload (uploaded once, never written)."""
    import lnerf
    c = wl.case(name)
    w = c.w
    mode = dict(rays=lnerf.INPUT_RAYS, points=lnerf.INPUT_POINTS, encoded=lnerf.INPUT_ENCODED)[c.mode]
    rays = mode == lnerf.INPUT_RAYS
    return dict(c=c, mlp=lnerf.make_mlp([x.shape for x in w.ws], w.wp.shape[1], w.wp.shape[2]), ws=_dev(w.wp),
                bs=_dev(w.bp), x=_dev(c.x), dists=None if rays else _dev(c.dists), target=_dev(w.target),
                sample_t=None if rays else _dev(c.t), mode=mode, S=w.S, N=w.N, F=w.F, L=len(w.ws))


def _state(engine, j, fused):
    """What the context reports after a step: the ReLU masks, the exceptional rows and the guard."""
    if not fused:
        return dict(masks=None, xrows=None, guard=engine.guard_fired())
    return dict(masks=engine.relu_masks(j["L"], j["N"] * j["S"]) if j["L"] > 1 else None,
                xrows=engine.exceptional_rows(split=True), guard=engine.guard_fired())


def _dx_kw(j, dx):
    """dx: None, "dx" (WANT_DX, ENCODED input) or "dinput" (WANT_DINPUT, x's own layout)."""
    return dict(want_dx=dx == "dx", want_dinput=dx == "dinput")


def run_step(engine, j, flags, dx=None, grads=None):
    import torch
    r = engine.train_step(j["mlp"], j["ws"], j["bs"], j["x"], j["dists"], j["target"], samples=j["S"],
                          input_mode=j["mode"], num_freqs=j["F"], seed=1.0, flags=flags, want_per_ray=True,
                          grads=grads, **_dx_kw(j, dx))
    torch.cuda.synchronize()
    out = dict(acc=r.acc_color.cpu().numpy(), dW=r.d_ws.cpu().numpy(), dB=r.d_bs.cpu().numpy(),
               d_dists=r.d_dists.cpu().numpy(), path=engine.last_path())
    out["dX"] = None if dx is None else (r.d_x if dx == "dx" else r.d_input).cpu().numpy()
    out.update(_state(engine, j, out["path"]["fused"]))
    return out


def run_vjp(engine, j, adj, flags, dx=None, grads=None, sample_t="own"):
    """adj: numpy arrays by name; returns the outputs as numpy arrays plus the context's state."""
    import torch
    st = j["sample_t"] if isinstance(sample_t, str) else sample_t
    r = engine.render_maps_vjp(j["mlp"], j["ws"], j["bs"], j["x"], j["dists"],
                               {k: _dev(np.asarray(v, np.float32)) for k, v in adj.items()}, samples=j["S"],
                               input_mode=j["mode"], num_freqs=j["F"], sample_t=st, flags=flags, grads=grads,
                               **_dx_kw(j, dx))
    torch.cuda.synchronize()
    out = dict(acc=r.acc_color.cpu().numpy(), dW=r.d_ws.cpu().numpy(), dB=r.d_bs.cpu().numpy(),
               d_dists=r.d_dists.cpu().numpy(), path=engine.last_path())
    out["dX"] = None if dx is None else (r.d_x if dx == "dx" else r.d_input).cpu().numpy()
    assert out["path"].get("vjp"), out["path"]
    out.update(_state(engine, j, out["path"]["fused"]))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(step, vjp, what=("dW", "dB", "d_dists", "acc", "dX")):
    for k in what:
        if step[k] is None:
            assert vjp[k] is None, k
            continue
        same = bits(step[k]) == bits(vjp[k])
        assert same.all(), f"{k}: {(~same).sum()} of {same.size} values differ in bits"
    if step["masks"] is not None:
        assert np.array_equal(step["masks"], vjp["masks"]), "ReLU masks"
    assert step["xrows"] == vjp["xrows"], ("exceptional rows", step["xrows"], vjp["xrows"])
    assert step["guard"] == vjp["guard"], ("guard_fired", step["guard"], vjp["guard"])
    a, b = dict(step["path"]), dict(vjp["path"])
    b.pop("vjp")
    assert a == b, (a, b)


def color_adjoint(step, target):
    """fp32(2 (acc_color - target)), as the training step's own seed at 1.0."""
    d = np.asarray(step["acc"], np.float32) - np.asarray(target, np.float32)
    return (d + d).astype(np.float32)


def _dx_mode(j, prec):
    import lnerf
    return "dx" if j["mode"] == lnerf.INPUT_ENCODED else "dinput"


# ---- A: the training step, bit for bit -------------------------------------------------------------

CASES_A = [(n, "default") for n in wl.FUSED] + \
          [(n, p) for n in ("rays", "encoded", "s128") for p in ("f16x3", "bf16x6", "bf16", "generic")] + \
          [(n, "generic") for n in wl.GENERIC_ONLY]


@pytest.mark.parametrize("name,prec", CASES_A, ids=[f"{n}-{p}" for n, p in CASES_A])
def test_color_adjoint_equals_train_step(engine, name, prec):
    import lnerf
    j = job(name)
    flags = _precisions()[prec]
    if name in wl.GENERIC_ONLY:
        flags = 0          # the shape itself sends the call down the generic path
    dx = _dx_mode(j, prec)
    step = run_step(engine, j, flags, dx)
    assert step["path"]["generic"] == (prec == "generic"), step["path"]
    vjp = run_vjp(engine, j, dict(color=color_adjoint(step, j["c"].w.target)), flags, dx)
    assert_same_bits(step, vjp)
    assert np.abs(step["dW"]).max() > 0 and np.abs(step["d_dists"]).max() > 0
    if j["mode"] == lnerf.INPUT_ENCODED:     # WANT_DINPUT on ENCODED input is WANT_DX's code path
        v2 = run_vjp(engine, j, dict(color=color_adjoint(step, j["c"].w.target)), flags, "dinput")
        assert (bits(v2["dX"]) == bits(step["dX"])).all()


def test_color_adjoint_accumulates_like_train_step(engine):
    import lnerf
    import torch
    j = job("encoded")
    first = run_step(engine, j, lnerf.FAST)
    adj = dict(color=color_adjoint(first, j["c"].w.target))

    def grads():
        g = engine.alloc_grads(j["L"], j["mlp"].w_k, j["mlp"].w_n)
        g[0].copy_(_dev(np.random.RandomState(5).randn(g[0].numel()).astype(np.float32)))
        return g
    step = run_step(engine, j, lnerf.FAST | lnerf.ACCUMULATE, "dx", grads())
    vjp = run_vjp(engine, j, adj, lnerf.FAST | lnerf.ACCUMULATE, "dx", grads())
    assert_same_bits(step, vjp)
    assert not (bits(step["dW"]) == bits(first["dW"])).all()       # the buffer's contents were added to
    torch.cuda.synchronize()


def test_color_adjoint_equals_train_step_where_the_guard_fires(engine):
    import lnerf
    g = dict(np.load(os.path.join(HERE, "golden", "edge_finite_6x8.npz"), allow_pickle=False))
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    S = int(g["S"])
    N = g["target"].shape[0]
    j = dict(mlp=lnerf.make_mlp(shapes, g["wp"].shape[1], g["wp"].shape[2]), ws=_dev(g["wp"].astype(np.float32)),
             bs=_dev(g["bp"].astype(np.float32)), x=_dev(g["X"].astype(np.float32)),
             dists=_dev(g["dists"].astype(np.float32)), target=_dev(g["target"].astype(np.float32)), sample_t=None,
             mode=lnerf.INPUT_ENCODED, S=S, N=N, F=0, L=len(shapes))
    step = run_step(engine, j, lnerf.FAST, "dx")
    vjp = run_vjp(engine, j, dict(color=color_adjoint(step, g["target"])), lnerf.FAST, "dx")
    assert step["guard"] == 1 and vjp["guard"] == 1, (step["guard"], vjp["guard"])
    assert_same_bits(step, vjp)


# ---- B: each new adjoint against float64 -----------------------------------------------------------

KINDS_B = ("depth", "opacity", "weights", "rgba", "all")


def _ratio(got, want, rtol, atol_scale):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(np.abs(want).max(initial=0.0), 1e-30)
    return float((np.abs(got - want) / (rtol * np.abs(want) + atol_scale * scale)).max())


def _note(path, what, r):
    WORST[(path, what)] = max(WORST.get((path, what), 0.0), r)


def check_against_f64(name, got, adj, prec, dx):
    """got: run_vjp's result; the float64 reference takes the GPU's ReLU decisions when it has them.
    name: a workload of render_vjp_workloads, or a Case of the caller's own."""
    c = name if isinstance(name, wl.Case) else wl.case(name)
    name = c.name
    w = c.w
    shapes = [x.shape for x in w.ws]
    masks = None
    if got["masks"] is not None:
        masks = [got["masks"][l][:, :shapes[l][1]] for l in range(len(shapes) - 1)]
    want = ref.render_vjp64(c.X, w.ws, w.bs, c.dists, w.S, adj, c.t, masks)
    rw, rb = assert_per_layer(got["dW"], got["dB"], want["dW"], want["db"], shapes)
    _note(prec, "dW", rw)
    _note(prec, "dB", rb)
    for k, a, b in (("d_dists", got["d_dists"], want["d_dists"]), ("acc", got["acc"], want["maps"]["color"])):
        _note(prec, k, _ratio(a, b, **TOL64))
        assert_close(f"{name} {k}", a, b, **TOL64)
    # the padding of d_ws / d_bs is written +0
    pw = np.ones(got["dW"].shape, bool)
    for l, (k, n) in enumerate(shapes):
        pw[l, :k, :n] = False
    assert (bits(got["dW"])[pw] == 0).all()
    if dx is None:
        return
    if c.mode == "encoded":
        _note(prec, "d_x", _ratio(got["dX"], want["dX"], **TOL64))
        assert_close(f"{name} d_x", got["dX"], want["dX"], **TOL64)
        return
    # POINTS / RAYS: the encoded gradient's TOL64 bar carried through the encoding's reverse
    p64 = (c.x if c.mode == "points" else None)
    if c.mode == "rays":
        r64 = c.x.astype(np.float64)
        p64 = (r64[:, None, :3] + r64[:, None, 3:] * np.linspace(2.0, 6.0, w.S)[None, :, None]).reshape(-1, 3)
    p64 = np.asarray(p64, np.float64)
    dp = igr.pe_bwd(p64, want["dX"], w.F)
    bar = igr.pe_bwd_l1(p64, igr.dx_bound(want["dX"], TOL64["rtol"], TOL64["atol_scale"]), w.F)
    if c.mode == "rays":
        t = np.linspace(2.0, 6.0, w.S)
        dp, bar = igr.rays_bwd(dp.reshape(w.N, w.S, 3), t), igr.rays_bwd_l1(bar.reshape(w.N, w.S, 3), t)
    bar = bar + 2.0 ** -23 * np.abs(dp)                   # the one rounding to float32 at the store
    err = np.abs(got["dX"].astype(np.float64) - dp)
    r = float((err / np.maximum(bar, 1e-300)).max())
    _note(prec, "d_input", r)
    assert r <= 1.0, f"{name} d_input: {r:.3g} of the bar"


CASES_B = [(n, p) for p in ("default", "f16x3", "bf16x6") for n in wl.FUSED] + [(n, "generic") for n in wl.ALL]


@pytest.mark.parametrize("name,prec", CASES_B, ids=[f"{n}-{p}" for n, p in CASES_B])
def test_each_adjoint_against_float64(engine, name, prec):
    j = job(name)
    c = j["c"]
    flags = 0 if name in wl.GENERIC_ONLY else _precisions()[prec]
    full = ref.random_adjoints(c.w.N, c.w.S, ADJ_SEED)
    dx = _dx_mode(j, prec)
    for kind in KINDS_B:
        adj = full if kind == "all" else {kind: full[kind]}
        got = run_vjp(engine, j, adj, flags, dx)
        assert got["path"]["generic"] == (prec == "generic"), got["path"]
        check_against_f64(name, got, adj, prec, dx)
    print("worst error / bar so far:", {f"{p}:{k}": round(v, 4) for (p, k), v in sorted(WORST.items())})


def test_points_depths_are_the_stratified_kernels(engine):
    """The "points" workload's sample_t is what lnerf_sample_stratified returns, bit for bit, and its
    points and dists are lnerf_ray_points' (so the depth term there ran on the device's own depths)."""
    import torch
    c = wl.case("points")
    rays32 = wl.ww.freq_workload(5)[1]
    t = engine.sample_stratified(c.w.N, c.w.S, _dev(c.u))
    pts, dists = engine.ray_points(_dev(rays32), t)
    torch.cuda.synchronize()
    assert (bits(t.cpu().numpy()) == bits(c.t)).all()
    assert (bits(pts.cpu().numpy()) == bits(c.x)).all() and (bits(dists.cpu().numpy()) == bits(c.dists)).all()
    assert np.abs(np.diff(c.t, axis=1) - np.diff(c.t, axis=1).mean()).max() > 1e-3      # non-uniform


# ---- C: linearity and isolation --------------------------------------------------------------------

# s24: 5 rays per 120-sample tile -- ray 0 opens a tile, ray 2 (samples 48..71) straddles lane 63, ray 4
# closes it; ray 5 opens the second tile
@pytest.mark.parametrize("prec", ["default", "generic"])
@pytest.mark.parametrize("ray", [0, 2, 4, 5])
def test_zero_adjoint_ray_is_isolated(engine, ray, prec):
    j = job("s24")
    c = j["c"]
    N, S = c.w.N, c.w.S
    full = ref.random_adjoints(N, S, ADJ_SEED)
    a = run_vjp(engine, j, full, _precisions()[prec], "dx")
    z = {k: v.copy() for k, v in full.items()}
    for k in ("color", "depth", "opacity", "weights"):
        z[k][ray] = 0.0
    z["rgba"].reshape(N, S, 4)[ray] = 0.0
    b = run_vjp(engine, j, z, _precisions()[prec], "dx")
    k0 = c.X.shape[1]
    dxa, dxb = a["dX"].reshape(N, S, k0), b["dX"].reshape(N, S, k0)
    assert (bits(b["d_dists"][ray]) == 0).all() and (bits(dxb[ray]) == 0).all()      # exact +0
    others = np.arange(N) != ray
    assert (bits(a["d_dists"][others]) == bits(b["d_dists"][others])).all()
    assert (bits(dxa[others]) == bits(dxb[others])).all()
    assert np.abs(a["d_dists"][ray]).max() > 0 and np.abs(dxa[ray]).max() > 0


@pytest.mark.parametrize("prec", ["default", "generic"])
def test_nan_sample_t_without_depth_adjoint(engine, prec):
    j = job("encoded")
    c = j["c"]
    full = ref.random_adjoints(c.w.N, c.w.S, ADJ_SEED)
    adj = {k: full[k] for k in ("color", "opacity", "weights", "rgba")}
    a = run_vjp(engine, j, adj, _precisions()[prec], "dx")
    b = run_vjp(engine, j, adj, _precisions()[prec], "dx", sample_t=_dev(np.full((c.w.N, c.w.S), np.nan, np.float32)))
    n = run_vjp(engine, j, adj, _precisions()[prec], "dx", sample_t=None)
    for o in (b, n):
        for k in ("dW", "dB", "d_dists", "dX", "acc"):
            assert (bits(a[k]) == bits(o[k])).all(), k


# ---- D: the contract -------------------------------------------------------------------------------

def raw_vjp(engine, j, adj, flags, outs, sample_t="own", mlp=None, null_adj=False, null_out=False):
    """The C call itself on device tensors (adj / outs: name -> tensor or None); returns its code."""
    import lnerf
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = j["sample_t"] if isinstance(sample_t, str) else sample_t
    b = lnerf.LnerfBatch(j["N"], j["S"], j["mode"], j["F"], j["x"].data_ptr(), p(j["dists"]), None, 2.0, 6.0)
    a = lnerf.LnerfRenderAdjoints(*[p(adj.get(k)) for k in ("color", "depth", "opacity", "weights", "rgba")])
    o = lnerf.LnerfOutputs(*[p(outs.get(k)) for k in ("loss", "acc_color", "d_ws", "d_bs", "d_x", "d_dists",
                                                       "d_target")])
    return engine.lib.lnerf_render_maps_vjp(engine.ctx, ctypes.byref(mlp or j["mlp"]), j["ws"].data_ptr(),
                                            j["bs"].data_ptr(), ctypes.byref(b), p(st),
                                            None if null_adj else ctypes.byref(a), flags,
                                            None if null_out else ctypes.byref(o), engine._stream())


def _poisoned(j):
    import torch
    f = lambda *s: torch.full(s, POISON, dtype=torch.float32, device="cuda:0")
    k0 = j["c"].X.shape[1]
    return dict(acc_color=f(j["N"], 3), d_ws=f(j["L"], j["mlp"].w_k, j["mlp"].w_n), d_bs=f(j["L"], j["mlp"].w_n),
                d_x=f(j["N"] * j["S"], k0), d_dists=f(j["N"], j["S"]))


def test_errors_write_nothing(engine):
    import lnerf
    import torch
    j, jr = job("encoded"), job("rays")
    c = j["c"]
    full = {k: _dev(v) for k, v in ref.random_adjoints(c.w.N, c.w.S, ADJ_SEED).items()}
    fr = {k: _dev(v) for k, v in ref.random_adjoints(jr["N"], jr["S"], ADJ_SEED).items()}
    one = torch.zeros(1, dtype=torch.float32, device="cuda:0")
    misaligned = torch.zeros(c.w.N * c.w.S * 4 + 1, dtype=torch.float32, device="cuda:0")[1:]
    cases = [
        ("SEED_LOSS", j, full, lnerf.SEED_LOSS, {}, {}),
        ("HEAD_FIT", j, full, lnerf.HEAD_FIT, {}, {}),
        ("K16_W4", j, full, lnerf.K16_W4, {}, {}),
        ("RENDER_K16", j, full, lnerf.RENDER_K16, {}, {}),
        ("every adjoint NULL", j, {}, 0, {}, {}),
        ("null adjoints", j, full, 0, {}, dict(null_adj=True)),
        ("out->loss", j, full, 0, dict(loss=one), {}),
        ("out->d_target", j, full, 0, dict(d_target=torch.zeros(c.w.N, 3, device="cuda:0")), {}),
        ("d_rgba alignment", j, dict(rgba=misaligned), 0, {}, {}),
        ("sample_t in RAYS mode", jr, fr, 0, {}, dict(sample_t=jr["x"])),
        ("d_depth without sample_t", j, full, 0, {}, dict(sample_t=None)),
        ("ACCUMULATE on the generic path", j, full, lnerf.GENERIC | lnerf.ACCUMULATE, {}, {}),
        ("GENERIC with a fused flag", j, full, lnerf.GENERIC | lnerf.MFMA_BF16X6, {}, {}),
        ("two precisions", j, full, lnerf.MFMA_F16X3 | lnerf.MFMA_BF16X6, {}, {}),
        ("FAST on a generic-only shape", job("head20"), {k: _dev(v) for k, v in ref.random_adjoints(
            24, 32, ADJ_SEED).items()}, lnerf.FAST, {}, {}),
        ("WANT_DX | WANT_DINPUT on RAYS input", jr, fr, lnerf.WANT_DX | lnerf.WANT_DINPUT, {}, {}),
    ]
    for what, jj, adj, flags, extra, kw in cases:
        outs = _poisoned(jj)
        outs.update(extra)
        rc = raw_vjp(engine, jj, adj, flags, outs, **kw)
        torch.cuda.synchronize()
        assert rc < 0, what
        assert lnerf.last_error(), what
        for k in ("acc_color", "d_ws", "d_bs", "d_x", "d_dists"):
            assert (outs[k] == POISON).all(), (what, k)


def test_null_outputs_and_last_path(engine):
    import lnerf
    import torch
    j = job("encoded")
    c = j["c"]
    full = {k: _dev(v) for k, v in ref.random_adjoints(c.w.N, c.w.S, ADJ_SEED).items()}
    for flags in (lnerf.FAST, lnerf.GENERIC):
        assert raw_vjp(engine, j, full, flags, {}, null_out=True) == 0, lnerf.last_error()
        assert raw_vjp(engine, j, full, flags, {}) == 0, lnerf.last_error()
        every = _poisoned(j)
        assert raw_vjp(engine, j, full, flags | lnerf.WANT_DX, every) == 0, lnerf.last_error()
        for name in every:                       # each output alone gives the bits it has among the others
            outs = _poisoned(j)
            solo = {name: outs[name]}
            assert raw_vjp(engine, j, full, flags | lnerf.WANT_DX, solo) == 0, (name, lnerf.last_error())
            torch.cuda.synchronize()
            assert torch.equal(solo[name], every[name]), name
            assert not (every[name] == POISON).any(), name
        v = engine.lib.lnerf_ctx_last_path(engine.ctx)
        assert v & lnerf.PATH_VJP
        assert bool(v & lnerf.PATH_GENERIC) == (flags == lnerf.GENERIC)
        if flags == lnerf.FAST:
            assert v & lnerf.PATH_DW16 and v & lnerf.PATH_K16 and v & lnerf.PATH_A24 and (v >> 8) & 3 == 2
            assert engine.workspace_used() > 0 and engine.guard_fired() == 0
    # d_x is not written without WANT_DX / WANT_DINPUT
    outs = _poisoned(j)
    assert raw_vjp(engine, j, full, lnerf.FAST, outs) == 0
    torch.cuda.synchronize()
    assert (outs["d_x"] == POISON).all() and not (outs["d_dists"] == POISON).any()
    # LNERF_TIMING: the step's six values
    assert raw_vjp(engine, j, full, lnerf.FAST | lnerf.TIMING, {}) == 0
    t = engine.timings()
    assert set(t) == {"pack", "fused", "loss", "dw", "reduce", "total"} and t["total"] > 0
    # a train step afterwards clears the bit
    run_step(engine, j, lnerf.FAST)
    assert not engine.lib.lnerf_ctx_last_path(engine.ctx) & lnerf.PATH_VJP


# ---- E: autograd -----------------------------------------------------------------------------------

def _losses():
    import torch
    import torch.nn.functional as F

    def supervised(maps, tgt):
        color, depth, opacity = maps
        return (F.mse_loss(color, tgt["color"]) + 0.1 * F.smooth_l1_loss(depth, tgt["depth"])
                + 0.01 * F.binary_cross_entropy(opacity.clamp(1e-6, 1 - 1e-6), tgt["mask"]))

    def white_background(maps, tgt):
        color, depth, opacity = maps
        return F.mse_loss(color + (1.0 - opacity)[:, None] * 1.0, tgt["color"])    # depth: no gradient, NULL

    return dict(supervised=supervised, white_background=white_background)


@pytest.mark.parametrize("loss_name", ["supervised", "white_background"])
@pytest.mark.parametrize("name", ["points", "rays"])
def test_autograd_wrapper(engine, name, loss_name):
    import lnerf
    import torch
    j = job(name)
    c = j["c"]
    N, S = c.w.N, c.w.S
    rng = np.random.RandomState(9)
    tgt = dict(color=j["target"], depth=_dev(rng.uniform(2, 6, N).astype(np.float32)),
               mask=_dev((rng.uniform(0, 1, N) > 0.5).astype(np.float32)))
    loss_fn = _losses()[loss_name]
    want_maps = ("color", "depth", "opacity")
    kw = dict(samples=S, input_mode=j["mode"], num_freqs=j["F"], sample_t=j["sample_t"], flags=lnerf.FAST)
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    ws, bs, x, dists = leaf(j["ws"]), leaf(j["bs"]), leaf(j["x"]), leaf(j["dists"])
    maps = lnerf.render_maps_autograd(engine, j["mlp"], ws, bs, x, dists, want=want_maps, **kw)
    loss_fn(maps, tgt).backward()
    torch.cuda.synchronize()
    # the same loss on detached maps: torch's own adjoints, fed to ONE direct call
    m = engine.render_maps(j["mlp"], j["ws"], j["bs"], j["x"], j["dists"], None, want=want_maps, **kw)
    leaves = [getattr(m, k).clone().requires_grad_(True) for k in want_maps]
    gs = torch.autograd.grad(loss_fn(leaves, tgt), leaves, allow_unused=True)
    adj = {k: g for k, g in zip(want_maps, gs) if g is not None}
    r = engine.render_maps_vjp(j["mlp"], j["ws"], j["bs"], j["x"], j["dists"], adj, want_dinput=True, **kw)
    torch.cuda.synchronize()
    same = lambda a, b: (bits(a.detach().cpu().numpy()) == bits(b.detach().cpu().numpy())).all()
    assert same(ws.grad, r.d_ws) and same(bs.grad, r.d_bs) and same(x.grad, r.d_input)
    if dists is not None:
        assert same(dists.grad, r.d_dists)
    for a, b in zip(maps, leaves):
        assert same(a, b)
    # and against float64 at the GPU's decisions
    got = dict(acc=r.acc_color.cpu().numpy(), dW=r.d_ws.cpu().numpy(), dB=r.d_bs.cpu().numpy(),
               d_dists=r.d_dists.cpu().numpy(), dX=r.d_input.cpu().numpy(),
               masks=engine.relu_masks(j["L"], N * S))
    check_against_f64(name, got, {k: g.cpu().numpy() for k, g in adj.items()}, "autograd", "dinput")


def test_autograd_sample_t_gradient(engine):
    """d loss / d sample_t = weights * d_depth[:, None] (a torch op on the forward's weights)."""
    import lnerf
    import torch
    j = job("points")
    c = j["c"]
    st = j["sample_t"].clone().requires_grad_(True)
    ws = j["ws"].clone().requires_grad_(True)
    depth, = lnerf.render_maps_autograd(engine, j["mlp"], ws, j["bs"], j["x"], j["dists"], samples=c.w.S,
                                        input_mode=j["mode"], num_freqs=j["F"], sample_t=st, flags=lnerf.FAST,
                                        want=("depth",))
    coef = _dev(np.random.RandomState(2).randn(c.w.N).astype(np.float32))
    (depth * coef).sum().backward()
    m = engine.render_maps(j["mlp"], j["ws"], j["bs"], j["x"], j["dists"], None, samples=c.w.S, input_mode=j["mode"],
                           num_freqs=j["F"], sample_t=j["sample_t"], flags=lnerf.FAST, want=("weights",))
    torch.cuda.synchronize()
    assert torch.equal(st.grad, m.weights * coef[:, None])
    assert ws.grad is not None and ws.grad.abs().max() > 0
