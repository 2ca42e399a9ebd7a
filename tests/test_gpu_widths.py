"""The fused training step and the bf16 render across first-layer widths, encoding frequencies and head
widths (tests/width_workloads.py; tests/test_width_workloads.py holds the CPU conditions that make these
workloads worth running): the quantities k16, kr and dw16 branch on.

  * k16's POINTS / RAYS input has two encoders, split at k[0] = 64: F = 10 (63 features, standard
    NeRF) takes the float64 double-angle recurrence, F = 11 (69) the direct sin(ldexp(x, q));
  * kr takes k[0] <= 64 only; wider inputs render on k16's bf16 forward;
  * the d_x store, the layer-0 slabs and dw16's layer-0 ranges follow k[0]: 1, 15 | 16 | 17, 64 | 65, 256;
  * a head of 5 or 16 outputs sits in one 16-wide tile whose columns 4.. the reverse pass never seeds:
    their dW / dB must come out as exact zeros, and nothing of them (8 x louder than columns 0..3)
    may reach any other output.

Training (1): fused_parity.check_fused in the three fp32-class precisions, seed = loss -- every ray
against float64 at the GPU's own ReLU decisions within TOL64, every flipped decision a tie, and the C
oracle within TOLC. Render (2): kr / k16's bf16 forward against each other where kr runs, against the
float64 sums of kr's own bf16-rounded operands within test_kr_vs_float64_per_element's 3e-4 (one
dropped feature moves these colours by >= 5.2e-3, test_width_workloads.py), and against plain float64
within bf16_render_bound. The worst measured errors are in DESIGN.md §5.
"""
import numpy as np
import pytest

import width_workloads as ww
from fused_parity import check_fused
from test_gpu_render import bf16_render_bound, render_np

pytestmark = pytest.mark.gpu

FUSED = [0, 512, 4096]    # lnerf.MFMA_F16X3 by default, lnerf.MFMA_BF16X6, lnerf.K16_W4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _assert_fused_path(engine, prec):
    import lnerf
    planes = 3 if prec & lnerf.MFMA_BF16X6 else 2
    assert engine.last_path() == dict(generic=False, fused=True, k16=True, dw16=True, kr=False,
                                      k16_w4=bool(prec & lnerf.K16_W4), planes=planes, a24=planes == 2)


# ---- 1. the training step ----------------------------------------------------------------------

@pytest.mark.parametrize("prec", FUSED)
@pytest.mark.parametrize("case", ww.CASES, ids=ww.case_id)
def test_fused_step(engine, case, prec):
    """ENCODED cases with d_x: compared over all k0 columns of a (rows, k0) buffer, so a store gated one
    feature short, or one past the row, shows. Head cases: the padded references hold zeros in dW / dB
    columns 4.., so assert_close against them is the check that nothing leaks."""
    import lnerf
    assert FUSED == [0, lnerf.MFMA_BF16X6, lnerf.K16_W4]
    kind, _, mode = case
    w, rays32, X, _ = ww.case_workload(case)
    want_dx = mode == "encoded"
    got, stats = check_fused(engine, w, points=mode != "encoded", seed=None, flags=prec, want_dx=want_dx,
                             rays32=rays32)
    _assert_fused_path(engine, prec)
    if want_dx:
        assert got["dX"].shape == (w.N * w.S, X.shape[1])
    if kind == "head":
        # G's columns 4.. are zeros, so these are sums of exact zeros: not merely below the tolerance
        assert (got["dW"][-1][:, 4:] == 0).all() and (got["dB"][-1][4:] == 0).all()


# ---- 2. the bf16 render: kr and its fallback -----------------------------------------------------

RENDER_CASES = [c for c in ww.CASES if c[0] == "freq"] + \
               [("encoded", k0, "encoded") for k0 in (1, 16, 17, 64, 65, 256)]


def _render(engine, w, rays32, mode, flags):
    import lnerf
    import torch
    mlp = lnerf.make_mlp([x.shape for x in w.ws], w.wp.shape[1], w.wp.shape[2])
    if mode == "rays":
        x, dists, im = _dev(rays32), None, lnerf.INPUT_RAYS
    elif mode == "points":
        x, dists, im = _dev(w.pts32.reshape(-1, 3)), _dev(w.dists), lnerf.INPUT_POINTS
    else:
        x, dists, im = _dev(w.X), _dev(w.dists), lnerf.INPUT_ENCODED
    loss, acc = engine.render(mlp, _dev(w.wp), _dev(w.bp), x, dists, _dev(w.target), samples=w.S, input_mode=im,
                              num_freqs=w.F, flags=flags)
    path = engine.last_path()
    torch.cuda.synchronize()
    return float(loss), acc.cpu().numpy().copy(), path


@pytest.mark.parametrize("case", RENDER_CASES, ids=ww.case_id)
def test_bf16_render(engine, case):
    import lnerf
    w, rays32, X, dists = ww.case_workload(case)
    k0, mode = X.shape[1], case[2]
    fl = lnerf.FAST | lnerf.MFMA_BF16
    la, a, pa = _render(engine, w, rays32, mode, fl)
    # widths past kr's 64 report k16's forward: not an error, not the generic path
    assert pa["kr"] == (k0 <= 64) and pa["planes"] == 1 and pa["k16"] and pa["fused"] and not pa["generic"], pa
    assert np.isfinite(a).all()
    vs_k16 = None
    if k0 <= 64:
        lb, b, pb = _render(engine, w, rays32, mode, fl | lnerf.RENDER_K16)
        assert not pb["kr"] and pb["k16"] and pb["planes"] == 1, pb
        vs_k16 = float(np.abs(a - b).max())
    emu, _ = render_np(X, w.ws, w.bs, dists, w.S, operands="bf16")
    ref, _ = render_np(X, w.ws, w.bs, dists, w.S)
    bound = bf16_render_bound(X, w.ws, w.bs, dists, w.S, ref)
    err_emu, err = np.abs(a - emu), np.abs(a - ref)
    print(f"bf16 render {ww.case_id(case)} (k0 = {k0}, {'kr' if pa['kr'] else 'k16'}): vs bf16-operand float64 max err "
          f"{err_emu.max():.3g}; vs k16 {'-' if vs_k16 is None else format(vs_k16, '.3g')}; vs float64 max err "
          f"{err.max():.3g}, max err / bound {(err / bound).max():.3g}")
    if k0 <= 64:
        np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-6)
        assert abs(la - lb) <= 1e-4 * abs(lb)
    assert err_emu.max() <= 3e-4, err_emu.max()
    assert (err <= bound).all(), float((err / bound).max())
