"""Workloads that move the hidden tile count HT the fused kernels are instantiated on, crossed with
the layer-0 input tiles T0, and a Python restatement of what the library launches for a shape.

make_layout computes ht16 = pow2_16(ceil(max hidden width / 16)) in {1, 2, 4, 8, 16}; k16_launch and
kr_launch switch on it, so every (HT, operand planes, sample tile, translation unit) is a kernel of
its own. HT sets the bytes per weight chunk, the register tiles a pass writes and the tiles a wider
layer-0 input (T0 > HT) leaves behind. Every other sweep in tests/ holds the hidden width at 30.

  * cell(HT, T0)   ENCODED input of k0 = 16 T0 - 3 features (a ragged last tile) under
                   k0 -> hi -> lo -> hi -> 4 with hi = 16 HT (the top of HT's band) and lo = 8 HT + 1
                   (its lower edge plus one): both hidden -> hidden directions run forward and
                   backward with a ragged layer between two full ones. width_workloads._recipe on
                   4 rays x 40 samples: on the 128-sample tile three rays per workgroup, so two
                   workgroups, the second with one ray, 120 of 128 samples valid; under K16_W4 one
                   ray per 64-sample tile.
  * scaled(HT, T0) the cell under scale_workloads.rescale with the down24 gains, for the ten cells
                   with T0 > HT: at unit scale a layer-0 tile left in the registers moves the row
                   shift too little to show.
  * plan(dims, S, flags)  what the library will launch, restated.

Only oracle/ and numpy are used; tests/test_tile_workloads.py holds the conditions these inputs must
meet, and the coverage claim, before the GPU tests of tests/test_gpu_tiles.py mean anything.
"""
from __future__ import annotations

import functools

import numpy as np

import nerf_np
import scale_workloads as sw
import width_workloads as ww

TILES = (1, 2, 4, 8, 16)
RAYS, SAMPLES = 4, 40
CELLS = [(ht, t0) for ht in TILES for t0 in TILES]
WIDE_INPUT_CELLS = [(ht, t0) for ht, t0 in CELLS if t0 > ht]      # layer 0 leaves tiles past HT
SCALE_PATTERN = "down24"

# the flags plan() reads (include/lnerf.h)
MFMA_BF16, MFMA_F16X3, MFMA_BF16X6, K16_W4, HEAD_FIT, RENDER_K16 = 128, 256, 512, 4096, 8192, 16384
DW_WAVES = 8                       # kWavesDw of the shipped build (LNERF_DW16_WAVES)
DW_SHAPES = ((1, 1), (1, 2), (2, 4))

# weight / input seed per cell, chosen on the CPU so that the float64 reference alone meets the
# conditions of tests/test_tile_workloads.py: the first seed from 1 up that meets all of them. Seed 1
# meets liveness, opacity and the TOL64 sensitivity nearly everywhere; what sends a cell further is
# the colour condition (one of up to 256 hidden features must move a colour by 3e-3) and, from HT = 8
# on, the tie condition (of ~10^5 pre-activations none within 4e-6 of a tie).
SEEDS = {(1, 1): 1, (1, 2): 4, (1, 4): 1, (1, 8): 2, (1, 16): 1,
         (2, 1): 3, (2, 2): 1, (2, 4): 1, (2, 8): 1, (2, 16): 2,
         (4, 1): 4, (4, 2): 2, (4, 4): 1, (4, 8): 1, (4, 16): 1,
         (8, 1): 15, (8, 2): 8, (8, 4): 6, (8, 8): 3, (8, 16): 21,
         (16, 1): 3, (16, 2): 19, (16, 4): 17, (16, 8): 125, (16, 16): 10}


def cell_id(c):
    return f"HT{c[0]}-T0_{c[1]}"


def cell_dims(ht, t0):
    hi, lo = 16 * ht, 8 * ht + 1
    return [16 * t0 - 3, hi, lo, hi, 4]


@functools.lru_cache(maxsize=None)
def cell(ht, t0, seed=None):
    seed = SEEDS[(ht, t0)] if seed is None else seed
    ws, bs, X, dists, target = ww._recipe(cell_dims(ht, t0), RAYS, SAMPLES, seed)
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(None, None, X, dists, target, ws, bs, wp, bp, 0, SAMPLES, RAYS)


@functools.lru_cache(maxsize=None)
def scaled(ht, t0):
    """(the cell under the down24 gains, log2 fW, log2 fB): dW_l of the rescaled run is fW[l] times
    the cell's, db_l fB[l] times (scale_workloads.rescale)."""
    w = cell(ht, t0)
    L = len(w.ws)
    g = sw.log2_gains(SCALE_PATTERN, L)
    return (sw.rescale(w, g)[0],) + sw.factors(g, L)


def pow2_16(t):
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 8 if t <= 8 else 16


def dw_shape(kt, nt, waves=DW_WAVES):
    """(TI, TJ) of the dW block a (kt, nt) layer runs on, and its active waves."""
    assert waves == 8
    blocks = lambda ti, tj: -(-kt // ti) * -(-nt // tj)
    for ti, tj in DW_SHAPES[:2]:
        if blocks(ti, tj) <= waves:
            return (ti, tj), blocks(ti, tj)
    return DW_SHAPES[2], min(waves, blocks(*DW_SHAPES[2]))


def plan(dims, S, flags=0):
    """What the library launches for an MLP of widths dims (dims[0] = k[0], dims[-1] the head) at S
    samples per ray under flags, restated from

      lnerf_fused.hip   pow2_16 (line 141); make_layout's ht16 and to16_b[0] (170-178: ht16 is
                        pow2_16 of the widest HIDDEN layer's 16-wide tiles, the head not counted;
                        to16_b[0] = pow2_16(ceil(k[0] / 16))) and rays per workgroup (184);
                        fused_plan_tile's planes (271: MFMA_BF16 1, MFMA_BF16X6 3, else 2) and its
                        kt / nt (281-282: 32-wide tiles); fused_plan's tile (345-355: 64 under
                        K16_W4, else 128); fused_render_uses_kr (459)
      lnerf_render.hip  kr_supported (471-473) and kr_launch's switch on ht16 (523-529)
      lnerf_dw16.hip    dw_shape (978-984, the 8-wave build: the first of 1x1, 1x2 whose block count
                        is <= 8, else 2x4) and dw_split's active waves (864-865: wave < block count)

    Returns ht16, to16_b0, planes, tile, rays_per_wg, kr_supported (the plan's own property),
    kr (a render under these flags runs kr) and dw: per layer (kt, nt, (TI, TJ), active waves)."""
    L = len(dims) - 1
    k, n = dims[:-1], dims[1:]
    mx16 = max([1] + [-(-n[l] // 16) for l in range(L - 1)])
    planes = 1 if flags & MFMA_BF16 else 3 if flags & MFMA_BF16X6 else 2
    tile = 64 if flags & K16_W4 else 128
    kr_supported = (planes == 1 and not flags & HEAD_FIT and S <= 128 and n[-1] <= 16 and tile == 128
                    and k[0] <= 64)
    dw = []
    for l in range(L):
        kt, nt = -(-k[l] // 32), -(-n[l] // 32)
        dw.append((kt, nt) + dw_shape(kt, nt))
    return dict(ht16=pow2_16(mx16), to16_b0=pow2_16(-(-k[0] // 16)), planes=planes, tile=tile,
                rays_per_wg=1 if S >= tile else tile // S, kr_supported=kr_supported,
                kr=kr_supported and not flags & RENDER_K16, dw=dw)


def cell_plan(c, flags=0):
    return plan(cell_dims(*c), SAMPLES, flags)
