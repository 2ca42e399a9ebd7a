"""TEST INFRASTRUCTURE ONLY -- the fp16x3 band below a G row's maximum: CPU helpers shared by
tests/golden/make_golden.py (which asserts these properties before it writes edge_band_4x8.npz /
edge_plain_4x8.npz), tests/test_oracle.py (which re-checks them from the committed files),
tests/test_gpu_edge.py and scripts/xcheck_study.py (the head-row table of DESIGN.md).

k1's reverse chain splits each G row into fp16 hi + lo at the row's own shift (the row maximum in
[2^13, 2^14), lnerf_internal.h fp16x3_shift / split_h2). An element 2^26 .. 2^37 below its row's
maximum lands in fp16's subnormals after that shift: hi keeps a few bits, lo nothing, and the
absolute error is 2^-25 after the shift -- percent level for the element. Everything here is numpy
on the float64 restatement (oracle/nerf_np.py); nothing touches the GPU.
"""
import numpy as np

import nerf_np

# the project's bar on a dW element: |err| <= COL_RTOL |want| + COL_TOL x (the column's max |want|)
COL_RTOL = 1e-5
COL_TOL = 1e-4
BAND = (30.0, 36.0)      # log2(row max / element) of every nonzero rgb-descended G element (band fixture)
PLAIN_SPAN = 20.0        # the same for every nonzero G element of the plain fixture, at most
CAN_FAIL = 10.0          # the emulated fp16x3 loss on the band fixture, in bars, at least
REF_SLACK = 0.1          # the C oracle against float64 on the band fixture, in bars, at most


def fp16x3_shift(m):
    """lnerf_internal.h fp16x3_shift, elementwise: e with m 2^e in [2^13, 2^14); 0 for m = 0 or
    non-finite m; clamped to 127."""
    m = np.asarray(m, np.float32)
    ok = (m > 0) & np.isfinite(m)
    e = np.frexp(np.where(ok, m, np.float32(1)))[1]
    return np.where(ok, np.minimum(14 - e, 127), 0).astype(np.int64)


def split_f16x3(G):
    """split_h2 on each row of G at the row's own shift: (hi + lo) 2^-e in float64, with
    hi = float16(x 2^e), lo = float16(x 2^e - hi) (x 2^e and the remainder are exact in fp32)."""
    x = np.asarray(G, np.float32)
    e = fp16x3_shift(np.abs(x).max(axis=1))[:, None]
    xs = np.ldexp(x, e).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return np.ldexp(hi.astype(np.float64) + lo.astype(np.float64), -e)


def head_row_scaled(Ghead, Whead):
    """The head's G row as k1's backward pass splits it (lnerf_k16.hip head_bscale): column n times
    2^(ew - head_col_shift(n)), ew the head's layer shift and head_col_shift(n) column n's own (the
    layer's for an all-zero column)."""
    W = np.abs(np.asarray(Whead, np.float32))
    ew = int(fp16x3_shift(W.max()))
    cm = W.max(axis=0)
    cs = np.where(cm > 0, fp16x3_shift(cm), ew)
    return np.ldexp(np.asarray(Ghead, np.float32), (ew - cs)[None, :]).astype(np.float32)


def row_floor(G):
    """Per row of G: the smallest frexp exponent of a nonzero element plus the row's shift, i.e. the
    binade in which the row's smallest element sits after the shift (what k1's floor guard compares
    with its threshold); +inf for an all-zero row."""
    x = np.asarray(G, np.float32)
    e = fp16x3_shift(np.abs(x).max(axis=1))
    fe = np.where(x != 0, np.frexp(np.where(x != 0, x, np.float32(1)))[1], 1 << 20)
    out = (fe.min(axis=1) + e).astype(np.float64)
    out[fe.min(axis=1) == 1 << 20] = np.inf
    return out


def head_col_sums(Gs):
    """Per column of the column-scaled head rows Gs: (what k1's split of each row at its own shift can
    lose -- 2^-25 after the shift for an element in fp16's subnormals, 2^-22 of a normal one --, the
    magnitudes), summed over the rows. Their ratio separates a column made only of band elements (the
    band fixture: 2^-5.3) from deep elements in columns that other rows feed at full precision (the
    reference's trained weights: 2^-16.2; any batch without band elements: 2^-22), which one
    element's depth cannot."""
    x = np.abs(np.nan_to_num(np.asarray(Gs, np.float32))).astype(np.float64)
    e = fp16x3_shift(x.max(axis=1))[:, None]
    err = np.where(x > 0, np.maximum(np.ldexp(1.0, -25 - e), x * 2.0 ** -22), 0.0)
    return err.sum(axis=0), x.sum(axis=0)


def mlp_of(g):
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    ws = [g["wp"][l, :k, :n] for l, (k, n) in enumerate(shapes)]
    bs = [g["bp"][l, :n] for l, (_, n) in enumerate(shapes)]
    return shapes, ws, bs


def float64_of(g):
    _, ws, bs = mlp_of(g)
    with np.errstate(all="ignore"):
        return nerf_np.nerf_forward_backward(g["X"], ws, bs, g["dists"], g["target"], int(g["S"]), seed=1.0)


def bars(got, want):
    """Per element, |got - want| over the bar COL_RTOL |want| + COL_TOL x the column's max |want|
    (0 where the bar and the error are both 0)."""
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want)
    lim = COL_RTOL * np.abs(want) + COL_TOL * np.abs(want).max(axis=0, keepdims=True)
    return np.where(err > 0, err / np.maximum(lim, 1e-300), 0.0)


def depths(G, cols=None):
    """log2(row max / |element|) of the nonzero elements of G (of its columns `cols`)."""
    a = np.abs(np.asarray(G, np.float64))
    m = a.max(axis=1, keepdims=True) * np.ones_like(a)
    if cols is not None:
        a, m = a[:, cols], m[:, cols]
    nz = a > 0
    return np.log2(m[nz] / a[nz])


def check_band(g):
    """The properties of the band fixture (8 -> 8 -> 8 -> 4 identity MLP); returns what was measured."""
    r = float64_of(g)
    _, ws, _ = mlp_of(g)
    G = r["G"]
    lo, hi = np.inf, -np.inf
    for l, cols in ((2, [0, 1, 2]), (1, [0, 1, 2, 4, 5, 6]), (0, [0, 1, 2, 4, 5, 6])):
        assert (np.abs(G[l]).argmax(axis=1) == 3).all(), f"layer {l}: a row's maximum is not its sigma element"
        d = depths(G[l], cols)
        assert len(d) and BAND[0] <= d.min() and d.max() <= BAND[1], (l, float(d.min()), float(d.max()))
        lo, hi = min(lo, float(d.min())), max(hi, float(d.max()))
    # the head row through k1's split, W2^T and the ReLU mask into dW_1
    G1 = np.where(r["Z"][1] > 0, split_f16x3(head_row_scaled(G[2], ws[2])) @ ws[2].astype(np.float64).T, 0.0)
    emu = bars(r["A"][1].T @ G1, r["dW"][1]).max(axis=0)
    assert emu.max() >= CAN_FAIL, emu
    # the reference of the GPU test (the loma-order fp32 C oracle) against float64
    ref = max(float(bars(g["dW"][l, :k, :n], g["f64_dW"][l, :k, :n]).max())
              for l, (k, n) in enumerate(mlp_of(g)[0]))
    assert ref <= REF_SLACK, ref
    floor = float(row_floor(head_row_scaled(G[2], ws[2])).min())
    return dict(depth_min=lo, depth_max=hi, emulated_dw1_bars=emu, c_oracle_bars=ref, head_floor=floor)


def check_plain(g):
    """No nonzero G element of any layer more than 2^PLAIN_SPAN below its row's maximum."""
    r = float64_of(g)
    worst = max(float(depths(G).max()) for G in r["G"])
    assert worst <= PLAIN_SPAN, worst
    _, ws, _ = mlp_of(g)
    return dict(depth_max=worst, head_floor=float(row_floor(head_row_scaled(r["G"][-1], ws[-1])).min()))


def uniform_tiny_sigma_workload(lo=4.5e-10, hi=7.5e-10):
    """The realistic route to a tiny sigma on every row: cfg2 (33 -> 30 -> 30 -> 4) on 24 rays x 16
    samples with the head's sigma column scaled down and its bias set so that every sigma lies in
    [lo, hi] (float64; the fp32 weights move the ends by ~1e-7 of that). The raw head G rows then span
    2^30 .. 2^40, and the column-scaled row k1 splits (head_row_scaled) under 2^9."""
    w = nerf_np.make_workload("cfg2", rays=24, samples=16)
    ws = [x.copy() for x in w.ws]
    bs = [x.copy() for x in w.bs]
    r = nerf_np.nerf_forward_backward(w.X, ws, bs, w.dists, w.target, w.S, seed=1.0)
    p = r["A"][-1] @ ws[-1][:, 3].astype(np.float64)
    a = (hi - lo) / (p.max() - p.min())
    ws[-1][:, 3] = (ws[-1][:, 3].astype(np.float64) * a).astype(np.float32)
    bs[-1][3] = np.float32(lo - a * p.min())
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)
