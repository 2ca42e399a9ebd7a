#!/usr/bin/env python3
"""Times the per-ray sampling kernels at the config-5 frame, and the hierarchical frame beside the
single render_maps frame, with HIP events after warm-up (one process, the versions alternating):

  1. lnerf_sample_importance + lnerf_ray_points on 640 000 rays, S = 64 coarse depths, 64 fine ones
     (the weights are a coarse render's own, so the cdfs are a frame's, not a toy's);
  2. scene.render_hierarchical_image (coarse S = 64, 64 fine, the fine pass on 128 samples) beside
     scene.render_maps_image at S = 128, and the hierarchical frame's parts one by one.

Prints one JSON line and, with --out, writes it to a file (profiles/sampling_timing.json is the
committed run). Needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "loma-nerf_amd"))


def timed(torch, fn, warmup, iters):
    """Milliseconds per call of fn(): `iters` calls each between its own pair of events, after
    `warmup` untimed ones. Returns (median, min, max)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--n-fine", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lnerf
    import scene
    if not torch.cuda.is_available():
        raise SystemExit("time_sampling.py needs a GPU")
    eng = lnerf.Engine(0)
    dev = "cuda:0"
    S, NF, F = a.samples, a.n_fine, 5
    shapes, wp, bp = scene.init_mlp(3 + 6 * F, 4, 8, 256)
    mlp = lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2])
    ws, bs = torch.from_numpy(wp).to(dev), torch.from_numpy(bp).to(dev)
    net = (mlp, ws, bs)
    focal = 0.5 / np.tan(0.5 * scene.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]])
    c2w = scene.look_at_pose()
    fl = lnerf.FAST | lnerf.MFMA_BF16            # the config-5 render precision
    rays = eng.get_rays(a.width, K, c2w)
    n = rays.shape[0]
    u = torch.rand(n, NF, device=dev, generator=torch.Generator(dev).manual_seed(0))

    def coarse():
        return eng.render_maps(mlp, ws, bs, rays, None, None, samples=S, input_mode=lnerf.INPUT_RAYS, num_freqs=F,
                               flags=fl, want=("weights",)).weights

    w = coarse()
    state = {}

    def importance():
        state["t_all"] = eng.sample_importance(w, NF, u=u, want=("all",))[1]

    def points():
        state["pd"] = eng.ray_points(rays, state["t_all"])

    def both():
        importance()
        points()

    def fine():
        p, d = state["pd"]
        return eng.render_maps(mlp, ws, bs, p, d, None, samples=S + NF, input_mode=lnerf.INPUT_POINTS, num_freqs=F,
                               sample_t=state["t_all"], flags=fl)

    def hierarchical():
        return scene.render_hierarchical_image(eng, net, net, a.width, K, c2w, S, NF, F, flags=fl, rays=rays, u=u)

    def single():
        return scene.render_maps_image(eng, mlp, ws, bs, a.width, K, c2w, S + NF, F, flags=fl, rays=rays)

    t = lambda fn: timed(torch, fn, a.warmup, a.iters)
    res = dict(rays=n, samples=S, n_fine=NF, warmup=a.warmup, iters=a.iters, device=torch.cuda.get_device_name(0),
               unit="ms, (median, min, max) over iters")
    res["sample_importance"] = t(importance)
    res["ray_points"] = t(points)
    res["sample_importance+ray_points"] = t(both)
    res["coarse_render_maps_rays"] = t(coarse)
    res["fine_render_maps_points"] = t(fine)
    # the two frames, alternating, twice
    for rnd in (0, 1):
        res[f"render_hierarchical_image#{rnd}"] = t(hierarchical)
        res[f"render_maps_image_S{S + NF}#{rnd}"] = t(single)
    mlp_ms = res["coarse_render_maps_rays"][0] + res["fine_render_maps_points"][0]
    res["sampling_share_of_mlp_passes"] = res["sample_importance+ray_points"][0] / mlp_ms
    # bytes the two sampling kernels must move (weights and u in, t_all out and in again, rays in,
    # points + dists out)
    moved = 4.0 * n * (S + NF + 2 * (S + NF) + 6 + 4 * (S + NF))
    res["sampling_min_bytes"] = moved
    res["sampling_achieved_GBps"] = moved / (res["sample_importance+ray_points"][0] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
