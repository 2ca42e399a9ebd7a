"""The workloads of tests/test_gpu_render_vjp.py (lnerf_render_maps_vjp), built on the CPU from
oracle/ and numpy alone, so that tests/test_render_vjp_ref.py can hold them to the conditions a GPU
comparison on them needs (semi-transparent rays, every adjoint kind loud in every layer) without a GPU.

The smallest shapes at which the VJP compositing can go wrong, all under a k[0] -> 30 -> 30 -> n MLP:

  rays       24 x 32, cfg2's MLP, INPUT_RAYS on the rays behind width_workloads.freq_workload(5)
             (the engine's own t and dists)
  points     the same rays at stratified depths (sampling_ref.stratified, what
             lnerf_sample_stratified returns bit for bit), INPUT_POINTS with sample_t
  encoded    width_workloads.encoded_workload(17), INPUT_ENCODED, sorted random depths
  head16     width_workloads.head_workload(16), INPUT_ENCODED
  s1         130 rays x 1 sample (one ray per lane, two tiles, the second nearly empty)
  s24        11 x 24 (five rays per tile: rays straddle lane 63)
  s64        5 x 64  (a ray per wave, the last tile half empty)
  s128       3 x 128 (one ray over two waves: both carries)
  s5         30 x 5  (25 rays per tile, the last tile holds 5)
  s129       3 x 129 and head20 (24 x 32 under a 20-output head): shapes only the generic path takes

The sample-count variants are encoded_workload(17)'s recipe at other (rays, samples); s1 has no
1e8 last delta (one sample of delta 1e8 is opaque wherever sigma > 0): its dists are 0.2..1.0.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import nerf_np
import render_maps_ref
import sampling_ref
import scale_workloads as sw
import width_workloads as ww
from fused_parity import rays_reference

FUSED = ("rays", "points", "encoded", "head16", "s1", "s24", "s64", "s128", "s5")
GENERIC_ONLY = ("s129", "head20")
ALL = FUSED + GENERIC_ONLY
SHAPES = dict(s1=(130, 1), s24=(11, 24), s64=(5, 64), s128=(3, 128), s5=(30, 5), s129=(3, 129))


@dataclass
class Case:
    name: str
    w: object              # nerf_np.Workload (ws, bs, wp, bp, target, S, N, F)
    mode: str              # "rays" / "points" / "encoded"
    x: np.ndarray          # what the device is handed: rays (N, 6), points (N S, 3) or X (N S, k0); float32
    X: np.ndarray          # (N S, k0) float32: the encoding the device computes or is handed
    dists: np.ndarray      # (N, S) float32: what the forward uses
    t: np.ndarray          # (N, S) float32 sample depths
    u: np.ndarray = None   # points: the (N, S) float32 numbers behind the stratified depths


def _sorted_t(N, S, seed):
    rng = np.random.RandomState(seed)
    return np.sort(rng.uniform(2.0, 6.0, (N, S)), axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    if name in ("rays", "points"):
        w, rays32 = ww.freq_workload(5)
        if name == "rays":
            X, dists = rays_reference(rays32, w.S, w.F)
            t = np.tile(render_maps_ref.ray_t(w.S), (w.N, 1))
            return Case(name, w, "rays", rays32, np.asarray(X, np.float32), dists, t)
        u = np.random.RandomState(7).uniform(0, 1, (w.N, w.S)).astype(np.float32)
        t = sampling_ref.stratified(u)
        pts, dists = sampling_ref.ray_points(rays32, t)
        X = nerf_np.positional_encoding_3d(pts.astype(np.float64).reshape(w.N, w.S, 3), w.F).reshape(w.N * w.S, -1)
        return Case(name, w, "points", pts, np.asarray(X, np.float32), dists, t, u)
    if name == "encoded":
        w = ww.encoded_workload(17)
    elif name == "head16":
        w = ww.head_workload(16)
    elif name == "head20":
        w = sw.head20_workload()
        X = nerf_np.positional_encoding_3d(w.pts32.astype(np.float64), w.F).reshape(w.N * w.S, -1)
        return Case(name, w, "points", w.pts32.reshape(-1, 3), np.asarray(X, np.float32), w.dists,
                    _sorted_t(w.N, w.S, 3))
    else:
        rays, S = SHAPES[name]
        w = ww.encoded_workload(17, rays=rays, samples=S)
        if S == 1:
            d = np.random.RandomState(5).uniform(0.2, 1.0, (rays, 1)).astype(np.float32)
            w = nerf_np.Workload(None, None, w.X, d, w.target, w.ws, w.bs, w.wp, w.bp, 0, S, rays)
    return Case(name, w, "encoded", w.X, w.X, w.dists, _sorted_t(w.N, w.S, 3))
