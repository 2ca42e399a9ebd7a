#!/usr/bin/env python3
"""Times lnerf_render_maps_vjp beside lnerf_train_step at cfg3 (4096 rays x 64 samples, RAYS input,
the default guarded fp16x3 precision), in one process with the variants interleaved round by round,
HIP events after warm-up:

  step            lnerf_train_step, LNERF_SEED_CONST (the work the VJP repeats, plus the loss)
  vjp_color       d_acc_color alone
  vjp_ray         d_acc_color + d_depth + d_opacity (the per-ray adjoints)
  vjp_all         all five (d_weights: 4 B per sample, d_rgba: 16 B per sample)
  copy_5MB        a device-to-device copy of the bytes the two per-sample adjoints add, for the rate

Each per-sample adjoint may add at most its own bytes at the measured copy rate; the script reports
the excess of every variant over the step. Prints one JSON line and, with --out, writes it to a file
(profiles/render_vjp_timing.json is the committed run). Needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "loma-nerf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lnerf
    import scene
    if not torch.cuda.is_available():
        raise SystemExit("time_render_vjp.py needs a GPU")
    eng = lnerf.Engine(0)
    dev = "cuda:0"
    N, S, F = a.rays, a.samples, 5
    shapes, wp, bp = scene.init_mlp(3 + 6 * F, 4, 8, 256)
    mlp = lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2])
    ws, bs = torch.from_numpy(wp).to(dev), torch.from_numpy(bp).to(dev)
    focal = 0.5 / np.tan(0.5 * scene.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]])
    rays = eng.get_rays(100, K, scene.look_at_pose())
    g = torch.Generator(dev).manual_seed(0)
    rays = rays[torch.randint(0, rays.shape[0], (N,), device=dev, generator=g)].contiguous()
    target = torch.rand(N, 3, device=dev, generator=g)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    adj = dict(color=rnd(N, 3), depth=rnd(N), opacity=rnd(N), weights=rnd(N, S), rgba=rnd(N * S, 4))
    grads = eng.alloc_grads(mlp.num_layers, mlp.w_k, mlp.w_n)
    acc = torch.empty(N, 3, device=dev)
    kw = dict(samples=S, input_mode=lnerf.INPUT_RAYS, num_freqs=F, flags=lnerf.FAST, grads=grads, acc_color=acc)
    src, dst = torch.empty(5 * N * S, device=dev), torch.empty(5 * N * S, device=dev)

    def vjp(names):
        sub = {k: adj[k] for k in names}
        return lambda: eng.render_maps_vjp(mlp, ws, bs, rays, None, sub, want_dists=False, **kw)

    variants = dict(
        step=lambda: eng.train_step(mlp, ws, bs, rays, None, target, seed=1.0, **kw),
        vjp_color=vjp(("color",)),
        vjp_ray=vjp(("color", "depth", "opacity")),
        vjp_all=vjp(("color", "depth", "opacity", "weights", "rgba")),
        copy_5MB=lambda: dst.copy_(src),
    )
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):                      # interleaved: every round times each variant once
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    stat = lambda v: (float(np.median(v)), float(min(v)), float(max(v)))
    res = dict(rays=N, samples=S, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0),
               guard_fired=eng.guard_fired(), unit="ms, (median, min, max) over interleaved rounds")
    for k, v in ms.items():
        res[k] = stat(v)
    rate = 2 * 4.0 * src.numel() / (res["copy_5MB"][0] * 1e-3) / 1e9       # read + write
    res["copy_GBps"] = rate
    res["per_sample_adjoint_bytes"] = 4.0 * N * S * 5
    res["per_sample_adjoint_ms_at_copy_rate"] = 4.0 * N * S * 5 / (rate * 1e9) * 1e3
    for k in ("vjp_color", "vjp_ray", "vjp_all"):
        res[k + "_minus_step_ms"] = res[k][0] - res["step"][0]
    # the kernels' own times under LNERF_TIMING (pack, fused, loss, dw, reduce, total): medians over
    # alternating calls (one timed call alone, right after the host-side work above, is noisy)
    kt = dict(flags=lnerf.FAST | lnerf.TIMING)
    per = dict(step_kernels=[], vjp_all_kernels=[])
    for _ in range(a.warmup + 10):
        eng.train_step(mlp, ws, bs, rays, None, target, seed=1.0, **dict(kw, **kt))
        per["step_kernels"].append(eng.timings())
        eng.render_maps_vjp(mlp, ws, bs, rays, None, adj, want_dists=False, **dict(kw, **kt))
        per["vjp_all_kernels"].append(eng.timings())
    for k, v in per.items():
        res[k] = {name: float(np.median([t[name] for t in v[a.warmup:]])) for name in v[0]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
