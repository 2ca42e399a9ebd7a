#!/usr/bin/env python3
"""Times the hash-grid kernels at the config-3 batch with HIP events after warm-up (one process, the
versions interleaved round by round, median and range):

  1. lnerf_hashgrid_encode and lnerf_hashgrid_grad on R = 4096 x 64 rows (a config-3 batch's rays at
     linspace(2, 6, 64)), 16 levels, F = 2, T = 2^19, res 16..2048 over the box [-2, 2]^3, beside a
     plain torch implementation of the same encode (gather) and its backward (index_add_), written
     below: what a user of the engine did before these kernels existed;
  2. how many atomics the wave-level run merging leaves per level (counted on the same points);
  3. scene.hashgrid_step with a 32 -> 64 -> 64 -> 4 MLP beside the config-3 step (256 x 8 MLP on the
     positional encoding).

Prints one JSON line and, with --out, writes it to a file (profiles/hashgrid_timing.json is the
committed run). Needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "loma-nerf_amd"))


def interleaved(torch, fns, warmup, rounds):
    """{name: (median, min, max) ms}: every round times each fn once, between its own events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


class TorchGrid:
    """The same encoding in plain torch (float32): per level the eight corner indices and weights,
    a gather for the forward and index_add_ for the table gradient."""

    def __init__(self, torch, grid, device):
        self.torch, self.grid = torch, grid
        self.lo = torch.tensor(grid.lo, device=device)
        self.ext = torch.tensor(grid.hi, device=device) - self.lo
        self.T = 1 << grid.log2_table

    def corners(self, points, l):
        torch = self.torch
        res = self.grid.res[l]
        u = ((points - self.lo) / self.ext).nan_to_num(0.0).clamp(0.0, 1.0)
        pos = u * (res - 1)
        i = pos.floor().clamp(max=res - 2)
        w = pos - i
        i = i.long()
        idx, wk = [], []
        for k in range(8):
            b = [(k >> c) & 1 for c in range(3)]
            g = [i[:, c] + b[c] for c in range(3)]
            if res ** 3 <= self.T:
                e = g[0] + res * (g[1] + res * g[2])
            else:
                e = (g[0] ^ ((g[1] * 2654435761) & 0xFFFFFFFF) ^ ((g[2] * 805459861) & 0xFFFFFFFF)) & (self.T - 1)
            f = [w[:, c] if b[c] else 1.0 - w[:, c] for c in range(3)]
            idx.append(e + self.grid.offsets[l])
            wk.append(f[0] * f[1] * f[2])
        return torch.stack(idx, 1), torch.stack(wk, 1)          # (R, 8) each

    def encode(self, table, points):
        out = []
        for l in range(self.grid.levels):
            idx, wk = self.corners(points, l)
            out.append((table[idx] * wk[:, :, None]).sum(1))
        return self.torch.cat(out, 1)

    def grad_table(self, points, d_encoded):
        F = self.grid.features
        d_table = self.torch.zeros(self.grid.total_entries, F, device=points.device)
        for l in range(self.grid.levels):
            idx, wk = self.corners(points, l)
            contrib = wk[:, :, None] * d_encoded[:, None, l * F:(l + 1) * F]
            d_table.index_add_(0, idx.reshape(-1), contrib.reshape(-1, F))
        return d_table


def merge_stats(torch, tg, grid, points, lds_floats=8192):
    """Per level: the atomics the d_table kernel issues per feature after merging runs of equal
    entries across adjacent lanes of a 64-lane wave, out of R * 8 (LDS-summed levels: the flush)."""
    R = points.shape[0]
    lane0 = (torch.arange(R, device=points.device) % 64 == 0)
    out = []
    for l in range(grid.levels):
        res = grid.res[l]
        idx, _ = tg.corners(points, l)
        head = torch.ones_like(idx, dtype=torch.bool)
        head[1:] = (idx[1:] != idx[:-1]) | lane0[1:, None]
        dense = res ** 3 <= (1 << grid.log2_table)
        rec = dict(level=l, res=res, dense=dense, adds=R * 8, after_merge=int(head.sum()))
        if dense and res ** 3 * grid.features <= lds_floats and R >= res ** 3:
            per = max(res ** 3, 2048)
            blocks = min(-(-R // per), -(-R // 256))
            rec.update(path="lds", lds_workgroups=blocks, global_atomics=int(blocks * res ** 3))
        else:
            rec.update(path="merge", global_atomics=rec["after_merge"])
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lnerf
    import scene
    if not torch.cuda.is_available():
        raise SystemExit("time_hashgrid.py needs a GPU")
    eng = lnerf.Engine(0)
    dev = "cuda:0"
    n, S = a.rays, a.samples
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    batch = scene.make_batch("cfg3", rays=n, samples=S)
    rays, target = t(batch["rays"]), t(batch["target"])
    sample_t = torch.linspace(2.0, 6.0, S, device=dev).repeat(n, 1).contiguous()
    points, dists = eng.ray_points(rays, sample_t)
    R = points.shape[0]
    grid = lnerf.HashGrid(16, 2, 19, 16, 2048, (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))
    F, L = grid.features, grid.levels
    table = grid.new_table(std=1e-1, seed=0, device=dev)
    tg = TorchGrid(torch, grid, dev)
    d_enc = torch.randn(R, grid.width, device=dev, generator=torch.Generator(dev).manual_seed(1))
    d_table = torch.empty(grid.total_entries, F, device=dev)
    enc = torch.empty(R, grid.width, device=dev)

    res = dict(rows=R, rays=n, samples=S, levels=L, features=F, log2_table=grid.log2_table, res=grid.res,
               entries=grid.total_entries, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0),
               unit="ms, (median, min, max) over interleaved rounds")
    # agreement first: the two implementations compute the same thing (float32 torch against float64 kernels)
    e_k, e_t = eng.hashgrid_encode(grid, table, points), tg.encode(table, points)
    g_k, g_t = eng.hashgrid_grad(grid, None, points, d_enc)[0], tg.grad_table(points, d_enc)
    res["max_abs_diff_encode_vs_torch"] = float((e_k - e_t).abs().max())
    res["max_rel_diff_d_table_vs_torch"] = float((g_k - g_t).abs().max() / g_t.abs().max())

    fns = {
        "encode": lambda: eng.hashgrid_encode(grid, table, points, out=enc),
        "torch_encode": lambda: tg.encode(table, points),
        "grad_d_table": lambda: eng.hashgrid_grad(grid, None, points, d_enc, d_table=d_table),
        "torch_grad_d_table": lambda: tg.grad_table(points, d_enc),
        "grad_d_points": lambda: eng.hashgrid_grad(grid, table, points, d_enc, want_d_table=False, want_d_points=True),
        "grad_both": lambda: eng.hashgrid_grad(grid, table, points, d_enc, d_table=d_table, want_d_points=True),
        "zero_d_table": lambda: d_table.zero_(),
    }
    res.update(interleaved(torch, fns, a.warmup, a.rounds))
    moved = 4.0 * R * L * 8 * F
    res["gathered_bytes"] = res["atomic_bytes_unmerged"] = moved
    res["encode_gathered_TBps"] = moved / (res["encode"][0] * 1e-3) / 1e12
    stats = merge_stats(torch, tg, grid, points)
    res["merge"] = stats
    issued = 4.0 * F * sum(s["global_atomics"] for s in stats)
    res["atomic_bytes_issued"] = issued
    kernel_ms = res["grad_d_table"][0] - res["zero_d_table"][0]
    res["d_table_kernel_ms_less_zeroing"] = kernel_ms
    res["d_table_unmerged_TBps"] = moved / (kernel_ms * 1e-3) / 1e12
    res["d_table_issued_TBps"] = issued / (kernel_ms * 1e-3) / 1e12
    res["speedup_encode_vs_torch"] = res["torch_encode"][0] / res["encode"][0]
    res["speedup_d_table_vs_torch"] = res["torch_grad_d_table"][0] / res["grad_d_table"][0]

    # the whole step: hash grid + 64 x 2 MLP beside config 3's 256 x 8 MLP on the positional encoding
    hs, hw_, hb = scene.init_mlp(grid.width, 4, 3, 64)
    hmlp = lnerf.make_mlp(hs, hw_.shape[1], hw_.shape[2])
    hws, hbs = t(hw_), t(hb)
    cs, cw, cb = scene.init_mlp(3 + 6 * batch["F"], 4, batch["L"], batch["H"])
    cmlp = lnerf.make_mlp(cs, cw.shape[1], cw.shape[2])
    cws, cbs = t(cw), t(cb)
    pts, cd = t(batch["pts"]), t(batch["dists"])
    hg = eng.alloc_grads(hmlp.num_layers, hmlp.w_k, hmlp.w_n)
    cg = eng.alloc_grads(cmlp.num_layers, cmlp.w_k, cmlp.w_n)
    x = eng.hashgrid_encode(grid, table, points)
    steps = {
        "hashgrid_step": lambda: scene.hashgrid_step(eng, grid, table, hmlp, hws, hbs, rays, sample_t, target,
                                                     grads=hg, d_table=d_table),
        "hashgrid_step_mlp_part": lambda: eng.train_step(hmlp, hws, hbs, x, dists, target, samples=S,
                                                         input_mode=lnerf.INPUT_ENCODED, grads=hg, want_dx=True),
        "cfg3_step": lambda: eng.train_step(cmlp, cws, cbs, pts, cd, target, samples=S, num_freqs=batch["F"],
                                            grads=cg),
    }
    steps["hashgrid_step_mlp_part"]()
    res["hashgrid_step_mlp_path"] = eng.last_path()
    res.update(interleaved(torch, steps, a.warmup, a.rounds))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
