#!/usr/bin/env python3
"""Times d_table of lnerf_hashgrid_grad in its two modes -- float32 atomics (the default) and
LNERF_HASHGRID_REPRODUCIBLE (stable sort + ordered float64 sums) -- with the method and the shape of
scripts/time_hashgrid.py: R = 4096 x 64 rows of config-3 rays at linspace(2, 6, 64), 16 levels, F = 2,
T = 2^19, res 16..2048 over [-2, 2]^3; HIP events, warm-up, then interleaved rounds in one process,
median and range.

  1. d_table alone, atomic against reproducible (zeroing included in both), and with d_points;
  2. scene.hashgrid_step (32 -> 64 -> 64 -> 4 MLP) in both modes;
  3. the scratch the reproducible mode takes from the stream's pool (lnerf_hashgrid_grad_scratch);
  4. the pile: every row at one point (eight entries per level receive R terms each);
  5. with --kernel-stats FILE (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of
     `time_hashgrid_ordered.py --calls-only N`, taken in a run of its own): the split of one
     reproducible call between the keys kernel, the sort's kernels and the sum kernel.

Prints one JSON line and, with --out, writes it to a file (profiles/hashgrid_ordered_timing.json is the
committed run). Needs a GPU: there is no CPU path to time."""
import argparse
import csv
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "loma-nerf_amd"))
sys.path.insert(0, HERE)

from time_hashgrid import interleaved  # noqa: E402


def kernel_split(path, calls):
    """{keys, sort, sum: ms per call} from a rocprofv3 kernel_stats.csv of `calls` reproducible calls."""
    ns = dict(keys=0.0, sort=0.0, sum=0.0, other=0.0)
    kinds = 0
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name, total = row["Name"], float(row["TotalDurationNs"])
            if "hg_keys_kernel" in name:
                ns["keys"] += total
            elif "hg_sum_kernel" in name:
                ns["sum"] += total
            elif "rocprim" in name:
                ns["sort"] += total
                kinds += 1
            else:
                ns["other"] += total
    out = {k + "_ms_per_call": v * 1e-6 / calls for k, v in ns.items()}
    out["sort_kernel_kinds"] = kinds   # rocPRIM's histogram, scan and onesweep kernels
    out["calls"] = calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls-only", type=int, default=0,
                    help="make this many reproducible d_table calls and exit (the profiler's subject)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-stats-calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lnerf
    import scene
    if not torch.cuda.is_available():
        raise SystemExit("time_hashgrid_ordered.py needs a GPU")
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
    d_enc = torch.randn(R, grid.width, device=dev, generator=torch.Generator(dev).manual_seed(1))
    d_table = torch.empty(grid.total_entries, F, device=dev)
    d_table_o = torch.empty(grid.total_entries, F, device=dev)

    if a.calls_only:
        for _ in range(a.calls_only):
            eng.hashgrid_grad(grid, None, points, d_enc, d_table=d_table_o, reproducible=True)
        torch.cuda.synchronize()
        eng.close()
        return

    res = dict(rows=R, rays=n, samples=S, levels=L, features=F, log2_table=grid.log2_table, res=grid.res,
               entries=grid.total_entries, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0),
               unit="ms, (median, min, max) over interleaved rounds")
    # agreement first: the two modes compute the same sums, and the reproducible one repeats its bits
    g_a = eng.hashgrid_grad(grid, None, points, d_enc)[0]
    g_o = eng.hashgrid_grad(grid, None, points, d_enc, reproducible=True)[0].clone()
    g_o2 = eng.hashgrid_grad(grid, None, points, d_enc, reproducible=True)[0]
    res["max_rel_diff_atomic_vs_reproducible"] = float((g_a - g_o).abs().max() / g_o.abs().max())
    res["reproducible_repeats_its_bits"] = bool(torch.equal(g_o.view(torch.int32), g_o2.view(torch.int32)))
    res["atomic_repeats_its_bits"] = bool(torch.equal(g_a.view(torch.int32),
                                                      eng.hashgrid_grad(grid, None, points, d_enc)[0].view(torch.int32)))
    res["scratch_bytes"] = eng.hashgrid_grad_scratch(grid, R)
    res["scratch_bytes_per_row"] = res["scratch_bytes"] / R

    fns = {
        "d_table_atomic": lambda: eng.hashgrid_grad(grid, None, points, d_enc, d_table=d_table),
        "d_table_reproducible": lambda: eng.hashgrid_grad(grid, None, points, d_enc, d_table=d_table_o,
                                                          reproducible=True),
        "both_atomic": lambda: eng.hashgrid_grad(grid, table, points, d_enc, d_table=d_table, want_d_points=True),
        "both_reproducible": lambda: eng.hashgrid_grad(grid, table, points, d_enc, d_table=d_table_o,
                                                       want_d_points=True, reproducible=True),
    }
    res.update(interleaved(torch, fns, a.warmup, a.rounds))
    res["reproducible_over_atomic"] = res["d_table_reproducible"][0] / res["d_table_atomic"][0]

    # the pile: every row at one point inside the box
    pile = points[:1].repeat(R, 1).contiguous()
    piles = {
        "pile_d_table_atomic": lambda: eng.hashgrid_grad(grid, None, pile, d_enc, d_table=d_table),
        "pile_d_table_reproducible": lambda: eng.hashgrid_grad(grid, None, pile, d_enc, d_table=d_table_o,
                                                               reproducible=True),
    }
    res.update(interleaved(torch, piles, 1, 5))

    hs, hw_, hb = scene.init_mlp(grid.width, 4, 3, 64)
    hmlp = lnerf.make_mlp(hs, hw_.shape[1], hw_.shape[2])
    hws, hbs = t(hw_), t(hb)
    hg = eng.alloc_grads(hmlp.num_layers, hmlp.w_k, hmlp.w_n)
    steps = {
        "hashgrid_step_atomic": lambda: scene.hashgrid_step(eng, grid, table, hmlp, hws, hbs, rays, sample_t, target,
                                                            grads=hg, d_table=d_table),
        "hashgrid_step_reproducible": lambda: scene.hashgrid_step(eng, grid, table, hmlp, hws, hbs, rays, sample_t,
                                                                  target, grads=hg, d_table=d_table_o,
                                                                  reproducible=True),
    }
    res.update(interleaved(torch, steps, a.warmup, a.rounds))
    if a.kernel_stats:
        res["kernel_split"] = kernel_split(a.kernel_stats, a.kernel_stats_calls)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
