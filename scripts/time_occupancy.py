#!/usr/bin/env python3
"""Times the occupancy-grid entry points with HIP events after warm-up (one process, the versions
interleaved round by round, median and range), each beside the baseline it is measured against:

  1. lnerf_sample_occupancy at the config-3 batch (4096 rays, M = 1024 steps, S = 64, res = 128, a
     sphere-shaped bitfield) beside a plain torch implementation of the same sampler, written below
     (float64 march, cumsum, searchsorted): what a user of the engine would write without the kernel.
     Also bit lookups per second (rays x M per call).
  2. the config-5 frame (640 000 rays, S = 128 and 64) beside one lnerf_render_maps frame at S = 128
     (RAYS input), and beside the 0.983 ms sample_importance + ray_points was measured at (DESIGN.md
     section 3 "ks"); sample_occupancy + ray_points is timed here too, so like stands beside like.
  3. scene.occgrid_refresh at res = 128 (2 097 152 cells, the config-3 MLP) beside the render_maps call
     it contains.
  4. scene.render_occupancy_image on the 800 x 800 frame at S = 32 and S = 64 beside the uniform
     S = 128 frame. TIMES ONLY: the MLP is untrained, image quality is not measured here.
Every MLP pass runs at the config-5 render precision (FAST | MFMA_BF16), as scripts/time_sampling.py.

The LDS-staged bitfield (res <= 64) was not tried; "lds_staging" in the output says so.

Prints one JSON line and, with --out, writes it to a file (profiles/occupancy_timing.json is the
committed run). Needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "loma-nerf_amd"))

LO, HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)


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


def sphere_bits(torch, res, radius, dev):
    """(bool per cell, int32 words): cells whose centre is within `radius` (in half-extents) of the centre."""
    g = (torch.arange(res, device=dev, dtype=torch.float64) + 0.5) * 2.0 / res - 1.0
    on = (g[None, None, :] ** 2 + g[None, :, None] ** 2 + g[:, None, None] ** 2 < radius * radius).reshape(-1)
    w = (on.reshape(-1, 32).long() << torch.arange(32, device=dev)).sum(1)
    return on, torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def torch_sampler(torch, on, rays, S, M, near, far, res):
    """lnerf_sample_occupancy's formulas (u = None) in plain torch, float64."""
    dev = rays.device
    lo = torch.tensor(LO, device=dev, dtype=torch.float64)
    ext = torch.tensor(HI, device=dev, dtype=torch.float64) - lo
    h = (far - near) / M
    c = near + (torch.arange(M, device=dev, dtype=torch.float64) + 0.5) * h
    r = rays.double()
    w = ((r[:, None, :3] + r[:, None, 3:] * c[None, :, None]) - lo) / ext
    ok = (w >= 0) & (w < 1)
    g = torch.where(ok, w * res, torch.zeros_like(w)).long().clamp(max=res - 1)
    occ = ok.all(-1) & on[g[..., 0] + res * (g[..., 1] + res * g[..., 2])]
    N = occ.sum(1)
    eff = occ | (N == 0)[:, None]
    Np = eff.sum(1)
    q = (torch.arange(S, device=dev, dtype=torch.float64)[None, :] + 0.5) * Np[:, None].double() / S
    k = torch.minimum(q.long(), Np[:, None] - 1)
    f = q - k.double()
    idx = torch.searchsorted(eff.cumsum(1), k + 1)
    t = (near + (idx.double() + f) * h).float()
    dists = (Np.double() * h / S).float()[:, None].expand(-1, S).contiguous()
    return t, dists, N.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--frame-rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lnerf
    import scene
    if not torch.cuda.is_available():
        raise SystemExit("time_occupancy.py needs a GPU")
    eng = lnerf.Engine(0)
    dev = "cuda:0"
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    near, far = 2.0, 6.0
    fl = lnerf.FAST | lnerf.MFMA_BF16            # the config-5 render precision, as scripts/time_sampling.py
    res = dict(warmup=a.warmup, rounds=a.rounds, frame_rounds=a.frame_rounds, device=torch.cuda.get_device_name(0),
               box=[LO, HI], render_flags="FAST | MFMA_BF16", unit="ms, (median, min, max) over interleaved rounds",
               lds_staging="not tried: the bitfield is read through L2 at every res")

    # ---- 1. the sampler at config 3 ------------------------------------------------------------------
    n, M, S, R = 4096, 1024, 64, 128
    occ = lnerf.OccGrid(R, LO, HI)
    on, bits = sphere_bits(torch, R, 0.7, dev)
    rays = t(scene.make_batch("cfg3", rays=n, samples=S)["rays"])
    t_k, d_k, n_k = eng.sample_occupancy(occ, bits, rays, S, steps=M, near=near, far=far)
    t_t, d_t, n_t = torch_sampler(torch, on, rays, S, M, near, far, R)
    res["cfg3"] = dict(rays=n, steps=M, samples=S, res=R, occupied_cells=int(on.sum()),
                       mean_occupied_steps=float(n_k.float().mean()), rays_without_a_step=int((n_k == 0).sum()),
                       bit_equal_to_torch=bool(torch.equal(t_k, t_t) and torch.equal(d_k, d_t) and torch.equal(n_k, n_t)))
    fns = {"sample_occupancy": lambda: eng.sample_occupancy(occ, bits, rays, S, steps=M, near=near, far=far),
           "torch_sampler": lambda: torch_sampler(torch, on, rays, S, M, near, far, R)}
    r = interleaved(torch, fns, a.warmup, a.rounds)
    res["cfg3"].update(r)
    res["cfg3"]["speedup_vs_torch"] = r["torch_sampler"][0] / r["sample_occupancy"][0]
    res["cfg3"]["bit_lookups_per_s"] = n * M / (r["sample_occupancy"][0] * 1e-3)

    # ---- 2. the config-5 frame -----------------------------------------------------------------------
    side, _, S5, F, L, H = scene.CONFIGS["cfg5"]
    focal = 0.5 / np.tan(0.5 * scene.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]])
    c2w = scene.look_at_pose()
    frame = eng.get_rays(side, K, c2w)
    shapes, wp, bp = scene.init_mlp(3 + 6 * F, 4, L, H)
    mlp, ws, bs = lnerf.make_mlp(shapes, wp.shape[1], wp.shape[2]), t(wp), t(bp)

    def sample_and_points(samples):
        tt, _, _ = eng.sample_occupancy(occ, bits, frame, samples, steps=M, near=near, far=far)
        return eng.ray_points(frame, tt)

    fns = {
        "sample_occupancy_S128": lambda: eng.sample_occupancy(occ, bits, frame, 128, steps=M, near=near, far=far),
        "sample_occupancy_S64": lambda: eng.sample_occupancy(occ, bits, frame, 64, steps=M, near=near, far=far),
        "sample_occupancy_S64_plus_ray_points": lambda: sample_and_points(64),
        "render_maps_frame_S128": lambda: scene.render_maps_image(eng, mlp, ws, bs, side, K, c2w, S5, F, flags=fl, rays=frame),
    }
    r = interleaved(torch, fns, 2, a.frame_rounds)
    _, _, n5 = eng.sample_occupancy(occ, bits, frame, 64, steps=M, near=near, far=far)
    res["cfg5_frame"] = dict(rays=int(frame.shape[0]), steps=M, res=R, sample_importance_plus_ray_points_ms=0.983,
                             rays_without_a_step=int((n5 == 0).sum()), mean_occupied_steps=float(n5.float().mean()), **r)
    res["cfg5_frame"]["bit_lookups_per_s"] = frame.shape[0] * M / (r["sample_occupancy_S64"][0] * 1e-3)

    # ---- 3. the refresh at res 128 -------------------------------------------------------------------
    density, new_bits = occ.new_density(dev), occ.new_bits(dev)
    ones = torch.ones(occ.num_cells, 1, device=dev)
    rgba = torch.empty(occ.num_cells, 4, device=dev)

    def sigma_fn(p):
        return eng.render_maps(mlp, ws, bs, p, ones, None, samples=1, input_mode=lnerf.INPUT_POINTS, num_freqs=F,
                               flags=fl, want=("rgba",), buffers=dict(rgba=rgba)).rgba[:, 3]

    centres = eng.occgrid_cell_points(occ)
    u3 = torch.rand(occ.num_cells, 3, device=dev)
    fns = {
        "occgrid_refresh": lambda: scene.occgrid_refresh(eng, occ, density, new_bits, sigma_fn, u=u3),
        "render_maps_it_contains": lambda: sigma_fn(centres),
        "cell_points": lambda: eng.occgrid_cell_points(occ, None, u3),
        "update_stride4": lambda: eng.occgrid_update(occ, density, rgba.flatten()[3:], sigma_stride=4),
        "threshold": lambda: eng.occgrid_threshold(occ, density, 0.01, bits=new_bits),
    }
    res["refresh_res128"] = dict(cells=occ.num_cells, **interleaved(torch, fns, a.warmup, a.rounds))

    # ---- 4. the frame with empty-space skipping: times only -----------------------------------------
    fns = {
        "render_occupancy_image_S32": lambda: scene.render_occupancy_image(eng, mlp, ws, bs, occ, bits, side, K, c2w, 32,
                                                                           F, steps=M, flags=fl, rays=frame),
        "render_occupancy_image_S64": lambda: scene.render_occupancy_image(eng, mlp, ws, bs, occ, bits, side, K, c2w, 64,
                                                                           F, steps=M, flags=fl, rays=frame),
        "uniform_frame_S128": lambda: scene.render_maps_image(eng, mlp, ws, bs, side, K, c2w, S5, F, flags=fl, rays=frame),
    }
    res["frame_times_only"] = dict(note="times only: untrained MLP, image quality on a trained scene is not measured",
                                   **interleaved(torch, fns, 2, a.frame_rounds))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
