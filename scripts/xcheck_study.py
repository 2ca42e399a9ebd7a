"""CPU study for the fp16x3 column guard (round 6): per layer, the column-independent bound of what
k1's fp16x3 reverse chain can lose in a dW element, E_l = sum_s 2^(14 - xa_s) 2^(14 - xg_s) (the
row scales k1's shifts imply), against each live column's max |dW|. Prints, per layer, the smallest
live column max over E_l -- the guard fires (whole step re-run on the bf16x6 split) when that falls
below 1e-4^-1 x 2^-38 x the guard's safety factor -- for the cfg3 bench batch and the edge fixtures.

With --head: per workload, where the smallest nonzero element of the column-scaled head G row (the
row k1's head backward pass splits, lnerf_k16.hip head_bscale) sits after the row's shift -- the
number k1's floor test (lnerf_internal.h kGuardExp) compares with its threshold --, the same for the
hidden G rows, and the head columns' summed split loss over their summed magnitude
(oracle/edge_band.py head_col_sums). The table of DESIGN.md §5.

  python scripts/xcheck_study.py [--rays 4096] [--head]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import nerf_np  # noqa: E402
import edge_band  # noqa: E402


def scale_of(X):
    m = np.abs(X).max(axis=1).astype(np.float32)
    out = np.zeros(len(m))
    ok = (m > 0) & np.isfinite(m)
    out[ok] = np.ldexp(1.0, np.frexp(m[ok])[1])   # 2^(14 - xa): the power of two above the row max
    return out


def study(X, ws, bs, dists, target, S, chunk=256):
    L = len(ws)
    E = np.zeros(L)
    dW = [0.0] * L
    N = X.shape[0] // S
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        rows = slice(lo * S, hi * S)
        with np.errstate(all="ignore"):
            r = nerf_np.nerf_forward_backward(X[rows], ws, bs, dists[lo:hi], target[lo:hi], S)
        for l in range(L):
            E[l] += float((scale_of(r["A"][l]) * scale_of(r["G"][l])).sum())
            dW[l] = dW[l] + np.nan_to_num(r["dW"][l])
    out = []
    for l in range(L):
        cm = np.abs(dW[l]).max(axis=0)
        live = cm > 0
        out.append((float(cm[live].min() / E[l]) if live.any() and E[l] > 0 else float("inf"),
                    float(np.median(cm[live]) / E[l]) if live.any() and E[l] > 0 else float("inf")))
    return out


def floors(X, ws, bs, dists, target, S, chunk=256):
    """(head, hidden): the smallest row_floor over the column-scaled head rows and over every hidden
    G row, how many head rows sit at or below 2^-12 / 2^-24 after their shift, and log2 of the worst
    head column's split loss over its magnitude."""
    N = X.shape[0] // S
    head, hid, n12, n24 = np.inf, np.inf, 0, 0
    E, M = 0.0, 0.0
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        with np.errstate(all="ignore"):
            r = nerf_np.nerf_forward_backward(X[lo * S:hi * S], ws, bs, dists[lo:hi], target[lo:hi], S)
        hs = np.nan_to_num(edge_band.head_row_scaled(r["G"][-1], ws[-1]))
        f = edge_band.row_floor(hs)
        e, m = edge_band.head_col_sums(hs)
        E, M = E + e, M + m
        head = min(head, float(f.min()))
        n12 += int((f <= -12).sum())
        n24 += int((f <= -24).sum())
        for G in r["G"][:-1]:
            hid = min(hid, float(edge_band.row_floor(np.nan_to_num(G)).min()))
    live = M > 0
    return head, hid, n12, n24, (float(np.log2((E[live] / M[live]).max())) if live.any() else -np.inf)


def tiny_sigma_batch():
    """tests/test_gpu_edge.py::test_tiny_sigma_delta_1e8_at_bench_size's batch"""
    w = nerf_np.make_workload("cfg3", rays=1024)
    ws = [x.copy() for x in w.ws]
    bs = [x.copy() for x in w.bs]
    ws[-1][:, 3] *= 1e-8
    bs[-1][3] = 0.0
    sub = nerf_np.subset_rays(w, range(256))
    r0 = nerf_np.nerf_forward_backward(sub.X, ws, bs, sub.dists, sub.target, sub.S, seed=1.0)
    bs[-1][3] = np.float32(-np.median(r0["A"][-1] @ ws[-1][:, 3].astype(np.float64)))
    return w.X, ws, bs, w.dists, w.target, w.S


def head_table(rays):
    gold = os.path.join(os.path.dirname(HERE), "tests", "golden")
    cases = []
    w = nerf_np.make_workload("cfg3", rays=rays)
    cases.append((f"cfg3 bench batch ({rays} rays)", (w.X, w.ws, w.bs, w.dists, w.target, w.S)))
    for name in ("chunk_4x30", "deep8_w64_2x64", "trained_weights_8x16", "edge_plain_4x8", "edge_band_4x8",
                 "edge_finite_6x8", "edge_nan_3x8"):
        g = dict(np.load(os.path.join(gold, name + ".npz"), allow_pickle=False))
        _, ws, bs = edge_band.mlp_of(g)
        cases.append((name, (g["X"], ws, bs, g["dists"], g["target"], int(g["S"]))))
    cases.append(("tiny-sigma 1024 x 64 batch", tiny_sigma_batch()))
    w = edge_band.uniform_tiny_sigma_workload()
    cases.append(("uniform tiny sigma 24 x 16", (w.X, w.ws, w.bs, w.dists, w.target, w.S)))
    print("smallest nonzero element after the row's shift, log2 binade: head rows (column-scaled), hidden rows;"
          " head rows at or below 2^-12, 2^-24; log2(worst head column's split loss / magnitude)")
    for name, c in cases:
        head, hid, n12, n24, loss = floors(*c)
        print(f"  {name:32s} {head:6.0f} {hid:6.0f} {n12:8d} {n24:6d} {loss:7.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--head", action="store_true")
    a = ap.parse_args()
    if a.head:
        return head_table(a.rays)
    w = nerf_np.make_workload("cfg3", rays=a.rays)
    print("cfg3 bench batch: per layer log2(min live colmax / E_l), log2(median colmax / E_l)")
    for l, (mn, md) in enumerate(study(w.X, w.ws, w.bs, w.dists, w.target, w.S)):
        print(f"  layer {l}: {np.log2(mn):7.2f} {np.log2(md):7.2f}")
    for name in ("edge_finite_6x8.npz", "deep8_w64_2x64.npz", "trained_weights_8x16.npz", "chunk_4x30.npz"):
        g = dict(np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", name), allow_pickle=False))
        if "shapes" not in g:
            continue
        shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
        ws = [g["wp"][l, :k, :n] for l, (k, n) in enumerate(shapes)]
        bs = [g["bp"][l, :n] for l, (_, n) in enumerate(shapes)]
        res = study(g["X"], ws, bs, g["dists"], g["target"], int(g["S"]))
        print(name, " ".join(f"{np.log2(mn):.1f}" for mn, _ in res))


if __name__ == "__main__":
    main()
