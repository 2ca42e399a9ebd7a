"""The compositing swept along the ray: every sample count S in 1 .. 128 (the generic path also 129,
200 and 257) times the opacity profiles of tests/composite_workloads.py, on every path that scans
along rays -- composite_tile_wave (the training step and the k16 render maps), composite_fwd_wave<256>
(kr) and the sequential generic kernels (lnerf_composite.h, lnerf_generic.hip).
tests/test_composite_workloads.py holds the CPU conditions (coverage of the tile positions, opacity,
C oracle against float64, exact inputs) that keep these runs from passing vacuously.

Each test loops over S inside, collects every failing (S, ray, profile, output) and asserts once, so a
failure shows its pattern; the worst error / bar per output is printed.

  A  forward: render_maps against render_maps_ref's a-priori bars from the returned rgba
     (test_gpu_render_maps.compositing_ratios' bars, per ray); rgba's sigma is the input's bit for bit
     (the exactness the workloads are built for); colour and loss are lnerf_render's bit for bit; empty
     rays are exactly zero.
  B  training step, seed 1, against float64 with bars PER RAY: acc, d_target, d_dists within
     1e-5 |want| + 1e-5 x the ray's max; dX rgb columns the same over the ray's rgb group, dX sigma
     columns within 1e-5 |want| + 1e-4 x the ray's column max (the unguarded fp16x3 split -- explicit
     LNERF_MFMA_F16X3, and LNERF_K16_W4 -- plus 2^-20 of the sample row's max, lnerf.h); dW / dB per layer and column (scale_workloads.assert_per_layer); the
     loss within 1e-6. Under the default flags a fired floor guard means the step is the explicit bf16x6
     step bit for bit.
  C  the edge fixtures' kinds at 11 sample counts, against the C oracle through test_gpu_edge's
     close_grouped (NaN patterns equal, per-ray bar), subnormal d_dists keeping their sign.
  D  neighbour isolation: replacing the first ray of a tile, a ray straddling a wave boundary and the last
     whole ray of a tile by an opaque, an empty or a NaN ray leaves every output row of every other ray
     bit-identical.

Worst error / bar measured on an MI355X (the tests print them; DESIGN.md §5 "The along-ray sweep"):
  A  weights 0.112, opacity 0.137 (generic 0.156), depth 0.163, colour 0.176 on every path (the worst
     rays are the short ones, S = 2 .. 5, where one rounding is a larger share of the bar);
  B  the fused paths: acc 0.059, d_target 0.011, d_dists 0.179, dX rgb 0.058, dX sigma 0.032, dW 0.105
     (K16_W4 0.121), dB 0.196, loss 0.18; generic: 0.059, 0.028, 0.187, 0.069, 0.034, 0.104, 0.22 and the
     loss 0.98 of its 1e-6 at S = 1 (513 rays' losses added one after the other). The floor guard fires
     at 89 of the 128 sample counts (a wall at a ray's first sample leaves its sigma adjoint 2^57 below
     the row's rgb adjoints), and the step is then the explicit bf16x6 step bit for bit;
  C  forward: weights 0.172, opacity 0.122 (generic 0.153), depth 0.121, colour 0.162; the step's dW on
     the CPU-decidable columns 0.068 of the 1e-4 column bar under the default flags; the unguarded
     fp16x3 split 9.1e3 (explicit) and 28.9 (K16_W4) on the finite batch, printed (see test_semantic_step);
  D  no row of any neighbour changed.
No kernel changed: the sweep found no bug in the scans.
"""
import numpy as np
import pytest

import composite_workloads as cw
import nerf_np
import render_maps_ref as ref
import scale_workloads as sw

pytestmark = pytest.mark.gpu

FUSED_S = tuple(S for S in cw.SWEEP if S <= 128)
W4_S = tuple(S for S in cw.SWEEP if S <= 64)
FORWARD_PATHS = ("kr", "k16_bf16", "fp16x3", "bf16x6", "w4", "generic")
STEP_PATHS = ("default", "f16x3", "bf16x6", "w4", "generic")
F16X3_ROW_TERM = 2.0 ** -20
# the fp16x3 split with no floor guard behind it: the explicit flag, and LNERF_K16_W4 ("fp16x3 or plain
# bf16", lnerf_ctx_guard_fired == -1: lnerf.h). Its documented row-relative loss is part of both's dX bar.
UNGUARDED_F16X3 = ("f16x3", "w4")


def _sweep(path):
    return cw.SWEEP if path == "generic" else W4_S if path == "w4" else FUSED_S


def _step_flags(path):
    import lnerf
    return {"default": lnerf.FAST, "f16x3": lnerf.FAST | lnerf.MFMA_F16X3, "bf16x6": lnerf.FAST | lnerf.MFMA_BF16X6,
            "w4": lnerf.FAST | lnerf.K16_W4, "generic": lnerf.GENERIC}[path]


def _check_step_path(p, path):
    if path == "generic":
        assert p["generic"] and not p["fused"], p
    else:
        assert p["k16"] and p["dw16"] and p["k16_w4"] == (path == "w4") and p["planes"] == (3 if path == "bf16x6" else 2), p


def _sync():
    """A sweep is hundreds of launches: after a device error nothing more is started."""
    import torch
    try:
        torch.cuda.synchronize()
    except Exception as e:   # noqa: BLE001
        pytest.exit(f"device error, the sweep stops here: {e}", returncode=3)


_DEV = {}


def _device(w):
    """The device tensors of a workload, uploaded once (keyed by the object: workloads are cached)."""
    import lnerf
    import torch
    if id(w) not in _DEV:
        d = lambda a: torch.from_numpy(np.array(a, np.float32)).to("cuda:0")   # (a copy: the workloads are read-only)
        _DEV[id(w)] = (w, lnerf.make_mlp(w.shapes, w.wp.shape[1], w.wp.shape[2]), d(w.wp), d(w.bp), d(w.X), d(w.dists),
                       d(w.target))
    return _DEV[id(w)][1:]


def run_step(engine, w, path):
    import lnerf
    mlp, wp, bp, x, dists, target = _device(w)
    r = engine.train_step(mlp, wp, bp, x, dists, target, samples=w.S, input_mode=lnerf.INPUT_ENCODED, seed=1.0,
                          flags=_step_flags(path), want_per_ray=True, want_dx=True)
    _sync()
    _check_step_path(engine.last_path(), path)
    return dict(loss=float(r.loss.item()), acc=r.acc_color.cpu().numpy(), dW=r.d_ws.cpu().numpy(),
                dB=r.d_bs.cpu().numpy(), d_dists=r.d_dists.cpu().numpy(), d_target=r.d_target.cpu().numpy(),
                dX=r.d_x.cpu().numpy())


_INP = {}


def _maps_inputs(w):
    import lnerf
    from test_gpu_render_maps import _inputs
    if id(w) not in _INP:
        # (copies: the workloads are read-only and _inputs wraps its arrays without copying)
        shim = nerf_np.Workload(None, None, w.X.copy(), w.dists.copy(), w.target.copy(), w.ws, w.bs, w.wp, w.bp, 0,
                                w.S, w.N)
        _INP[id(w)] = (w, _inputs(shim, lnerf.INPUT_ENCODED, sample_t=w.sample_t.copy()))
    return _INP[id(w)][1]


def run_forward(engine, w, path, render=True):
    """(maps, lnerf_render's (loss, colour) or None) of a workload on a forward path."""
    from test_gpu_render_maps import _flags, run_maps, run_render
    inp, fl = _maps_inputs(w), _flags()[path]
    _sync()
    out, p = run_maps(engine, inp, fl)
    assert p["maps"] and p["kr"] == (path == "kr") and p["generic"] == (path == "generic"), p
    assert p["k16_w4"] == (path == "w4"), p
    return out, (run_render(engine, inp, fl)[:2] if render else None)


def _report(title, worst, failures):
    print(f"{title}: worst error / bar " + ", ".join(f"{k} {v[0]:.3g} (S = {v[1]})" for k, v in worst.items()))
    if failures:
        by = {}
        for f in failures:
            by.setdefault((f[3], f[2]), []).append(f[0])
        lines = [f"  {out} on {prof}: S = {sorted(set(Ss))}" for (out, prof), Ss in sorted(by.items())]
        raise AssertionError(f"{title}: {len(failures)} failures (S, ray, profile, output, error / bar), first 20: "
                             f"{failures[:20]}\nby output and profile:\n" + "\n".join(lines))


def _collect(ratios, w, worst, failures):
    for k, v in ratios.items():
        v = np.where(np.isnan(v), np.inf, v)
        i = int(np.argmax(v))
        if v[i] > worst.get(k, (0.0, 0))[0]:
            worst[k] = (float(v[i]), w.S)
        failures += [(w.S, int(r), w.profiles[r], k, float(v[r])) for r in np.nonzero(v > 1.0)[0]]


def _empty_rays(w):
    return np.nonzero(~(w.sigma > 0).any(axis=1))[0]


# ---- A. forward ------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", FORWARD_PATHS)
def test_forward_sweep(engine, path):
    worst, failures = {}, []
    for S in _sweep(path):
        w = cw.workload(S)
        out, (loss, acc) = run_forward(engine, w, path)
        sig = out["rgba"][:, 3].reshape(w.N, S)
        if not np.array_equal(sig, w.sigma):
            failures += [(S, int(r), w.profiles[r], "rgba sigma != input", 0.0) for r in np.nonzero((sig != w.sigma).any(axis=1))[0]]
        _collect(ref.map_ratios(out, w.dists, w.sample_t, S), w, worst, failures)
        if not (np.array_equal(out["color"], acc) and out["loss"][0] == loss):
            failures.append((S, -1, "*", "colour / loss differ from lnerf_render", 0.0))
        for r in _empty_rays(w):
            if any((out[k][r] != 0).any() for k in ("color", "depth", "opacity", "weights")):
                failures.append((S, int(r), w.profiles[r], "empty ray not zero", 0.0))
    _report(f"forward sweep {path}", worst, failures)


# ---- B. training step --------------------------------------------------------------------------------

def _bf16x6_step(engine, w, cache={}):
    if id(w) not in cache:
        cache[id(w)] = (w, run_step(engine, w, "bf16x6"))
    return cache[id(w)][1]


def _step_failures(got, w, f64, c, row_term, worst, failures):
    S = w.S
    ratios = cw.step_ratios(got, w, f64, row_term)
    by_c = cw.step_ratios(got, w, c, row_term)
    for prof, out in cw.C_ORACLE_ONLY:
        m = np.array([p == prof for p in w.profiles])
        for k in ratios:
            if k == out or (out == "dX" and k.startswith("dX")):
                ratios[k] = np.where(m, by_c[k], ratios[k])
    _collect(ratios, w, worst, failures)
    try:
        rw, rb = sw.assert_per_layer(got["dW"], got["dB"], f64["dW"], f64["dB"], w.shapes)
    except AssertionError as e:
        failures.append((S, -1, "*", f"dW / dB: {e}", np.inf))
        rw = max(sw.dw_col_over_bar(got["dW"], f64["dW"], w.shapes))
        rb = max(sw.db_layer_over_bar(got["dB"], f64["dB"], w.shapes))
    for k, v in (("dW", rw), ("dB", rb), ("loss", abs(got["loss"] - f64["loss"]) / (1e-6 * abs(f64["loss"])))):
        if v > worst.get(k, (0.0, 0))[0]:
            worst[k] = (float(v), S)
    if not abs(got["loss"] - f64["loss"]) <= 1e-6 * abs(f64["loss"]):
        failures.append((S, -1, "*", "loss", abs(got["loss"] - f64["loss"]) / (1e-6 * abs(f64["loss"]))))
    for r in _empty_rays(w):
        rows = slice(r * S, (r + 1) * S)
        zero = (got["acc"][r] == 0).all() and (got["d_dists"][r] == 0).all() and (got["dX"][rows] == 0).all()
        if not (zero and np.array_equal(got["d_target"][r], np.float32(2.0) * w.target[r])):
            failures.append((S, int(r), w.profiles[r], "empty ray not zero", 0.0))


@pytest.mark.parametrize("path", STEP_PATHS)
def test_step_sweep(engine, path):
    worst, failures, fired = {}, [], {}
    for S in _sweep(path):
        w = cw.workload(S)
        f64, c = cw.references(S)
        got = run_step(engine, w, path)
        if path == "default":
            fired[S] = engine.guard_fired()
            if fired[S] == 1:
                x6 = _bf16x6_step(engine, w)
                if not (got["loss"] == x6["loss"] and all(np.array_equal(got[k], x6[k]) for k in x6 if k != "loss")):
                    failures.append((S, -1, "*", "guard fired, step != explicit bf16x6", np.inf))
        if path != "generic" and S in cw.SEMANTIC_S:
            # the ReLU decisions float64 is evaluated at are the GPU's own: x > 0 on exact inputs
            m = engine.relu_masks(3, w.N * S)
            if not all(np.array_equal(m[l, :, :8], w.X > 0) for l in range(2)):
                failures.append((S, -1, "*", "ReLU masks differ from x > 0", np.inf))
        _step_failures(got, w, f64, c, F16X3_ROW_TERM if path in UNGUARDED_F16X3 else 0.0, worst, failures)
    if path == "default":
        print(f"step sweep default: guard_fired == 1 at S = {[S for S, v in fired.items() if v == 1]}, "
              f"other states {sorted(set(fired.values()) - {1})}")
        assert set(fired.values()) <= {0, 1}
    _report(f"step sweep {path}", worst, failures)


# ---- C. the semantic kinds -----------------------------------------------------------------------------

def _grouped(failures, S, name, got, want):
    from test_gpu_edge import close_grouped
    try:
        close_grouped(name, got, want)
    except AssertionError as e:
        failures.append((S, -1, "*", str(e), np.inf))


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("path", STEP_PATHS)
def test_semantic_step(engine, path, nan):
    """Every per-ray output through close_grouped, unchanged. Two outputs are sums over the whole batch that
    fp32 itself does not pin down on these batches, and get test C's rule (composite_workloads
    .semantic_decidable, from CPU evaluations only): the loss (up to 257 rays' losses added in another order:
    the bar is max(1e-6, 4 x the CPU re-association distance), 5.4e-6 at most) and dW, held to the oracle on
    the columns where two more CPU fp32 evaluations agree with it (14 .. 20 of the 20 live columns). The
    unguarded fp16x3 split (LNERF_MFMA_F16X3, LNERF_K16_W4) drops what lies 2^17 and more below a G row's
    maximum (lnerf.h), which is most of these batches' rgb adjoints: its dW ratio on the finite batch is
    printed and not asserted, as test_gpu_edge does for the explicit split on its band fixture."""
    from test_gpu_edge import dw_over_bar
    failures, worst_dw = [], 0.0
    for S in cw.SEMANTIC_S:
        if path == "w4" and S > 64:
            continue
        w, c = cw.semantic(S, nan), cw.semantic_reference(S, nan)
        cols, loss_bar = (None, cw.semantic_nan_loss_bar(S)) if nan else cw.semantic_decidable(S)
        got = run_step(engine, w, path)
        if not abs(got["loss"] - c["loss"]) <= loss_bar * abs(c["loss"]):
            failures.append((S, -1, "*", "loss", abs(got["loss"] - c["loss"]) / (loss_bar * abs(c["loss"]))))
        for k, shape in (("acc", (w.N, 3)), ("d_target", (w.N, 3)), ("d_dists", (w.N, S)), ("dX", (w.N, S * 8)), ("dB", None)):
            _grouped(failures, S, k, got[k].reshape(shape) if shape else got[k], c[k].reshape(shape) if shape else c[k])
        gdw, cdw = got["dW"].copy(), c["dW"].copy()
        if cols is not None:
            gdw[np.broadcast_to(~cols[:, None, :], gdw.shape)] = 0
            cdw[np.broadcast_to(~cols[:, None, :], cdw.shape)] = 0
        if path in ("default", "f16x3", "w4"):
            # the fp16x3 family: per element against the plain column bar (test_gpu_edge.test_edge_numerics)
            unguarded = path != "default" and not nan
            try:
                worst_dw = max(worst_dw, dw_over_bar(gdw, cdw, np.array(w.shapes), check=not unguarded))
            except AssertionError as e:
                failures.append((S, -1, "*", f"dW column bar: {e}", np.inf))
        else:
            _grouped(failures, S, "dW", gdw, cdw)
        sub = (np.abs(c["d_dists"]) > 0) & (np.abs(c["d_dists"]) < np.finfo(np.float32).tiny)
        if not (np.sign(got["d_dists"][sub]) == np.sign(c["d_dists"][sub])).all():
            failures.append((S, -1, "*", "a subnormal d_dists lost its sign", np.inf))
    if path in ("default", "f16x3", "w4"):
        print(f"semantic step {path} {'nan' if nan else 'finite'}: worst dW error / the 1e-4 column bar {worst_dw:.3g}")
    _report(f"semantic step {path} {'nan' if nan else 'finite'}", {}, failures)


@pytest.mark.parametrize("path", FORWARD_PATHS)
def test_semantic_forward(engine, path):
    worst, failures = {}, []
    for S in cw.SEMANTIC_S:
        if path == "w4" and S > 64:
            continue
        for nan in (False, True):     # (the nan kind's forward is finite: its NaN is the sigmoid adjoint's)
            w, c = cw.semantic(S, nan), cw.semantic_reference(S, nan)
            out, _ = run_forward(engine, w, path, render=False)
            if not all(np.isfinite(out[k]).all() for k in ("color", "depth", "opacity", "weights", "rgba")):
                failures.append((S, -1, "*", "a map is not finite", np.inf))
                continue
            _collect(ref.map_ratios(out, w.dists, w.sample_t, S), w, worst, failures)
            _grouped(failures, S, "color", out["color"], c["acc"])   # (bf16-exact inputs: kr's rgba is everyone's)
            z = np.array([k == "sigma0" for k in w.profiles])
            if any((out[k][z] != 0).any() for k in ("color", "depth", "opacity", "weights")):
                failures.append((S, -1, "sigma0", "empty ray not zero", 0.0))
    _report(f"semantic forward {path}", worst, failures)


# ---- D. neighbour isolation -------------------------------------------------------------------------------

def _isolation_rays(S, tile, N):
    pc = cw.position_classes(S, tile, N)
    return sorted({r for r in pc.values() if r is not None})


def _rows_differ(a, b, N, keep):
    return [int(r) for r in np.nonzero(keep)[0]
            if not np.array_equal(a.reshape(N, -1)[r], b.reshape(N, -1)[r], equal_nan=True)]


@pytest.mark.parametrize("kind", ["opaque", "empty", "nan"])
def test_neighbours_step(engine, kind):
    """The default training step. Its floor guard re-runs the WHOLE batch on the bf16x6 split, so a replaced
    ray may change the split the other rays are computed on; the modified run is compared with the base run
    of the split it ended on (a fired default step is the explicit bf16x6 step, an unfired one the explicit
    fp16x3 step, bit for bit: test B and test_gpu_edge)."""
    failures = []
    for S in cw.SEMANTIC_S:
        w = cw.workload(S)
        rays = _isolation_rays(S, 128, w.N)
        keep = ~np.isin(np.arange(w.N), rays)
        assert keep.sum() >= 2, S
        base = run_step(engine, w, "default")
        fired0 = engine.guard_fired()
        got = run_step(engine, cw.replace_rays(w, rays, kind), "default")
        fired1 = engine.guard_fired()
        if fired1 != fired0:
            base = run_step(engine, w, "bf16x6" if fired1 == 1 else "f16x3")
        for k in ("acc", "d_target", "d_dists", "dX"):
            bad = _rows_differ(got[k], base[k], w.N, keep)
            failures += [(S, r, w.profiles[r], f"{k} changed (replaced {rays}, guard {fired0} -> {fired1})", np.inf) for r in bad]
    _report(f"neighbours of {kind} rays, default step", {}, failures)


@pytest.mark.parametrize("kind", ["opaque", "empty", "nan"])
@pytest.mark.parametrize("path", ["kr", "fp16x3"])
def test_neighbours_maps(engine, path, kind):
    failures = []
    for S in cw.SEMANTIC_S:
        w = cw.workload(S)
        rays = _isolation_rays(S, 256 if path == "kr" else 128, w.N)
        keep = ~np.isin(np.arange(w.N), rays)
        assert keep.sum() >= 2, S
        base, _ = run_forward(engine, w, path, render=False)
        got, _ = run_forward(engine, cw.replace_rays(w, rays, kind), path, render=False)
        for k in ("color", "depth", "opacity", "weights", "rgba"):
            bad = _rows_differ(got[k], base[k], w.N, keep)
            failures += [(S, r, w.profiles[r], f"{k} changed (replaced {rays})", np.inf) for r in bad]
        if kind == "nan":   # and the NaN did arrive: the replaced rays' colour is NaN
            if not np.isnan(got["color"][rays]).all():
                failures.append((S, -1, "nan", "the replaced rays' colour is not NaN", np.inf))
    _report(f"neighbours of {kind} rays, {path} maps", {}, failures)
