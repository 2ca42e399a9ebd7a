"""Where the dW kernel's pipelined half-block loop (lnerf_dw16.hip) can go wrong, at the smallest
shapes that reach each case: the three-step load rotation over ranges of every length, the per-sample
scale table at the ends of a range, the fragment read-ahead across the image toggle, the non-FULL
2 x 4 loop, and the 1 x 2 / 1 x 1 shapes (layer 0 and the head of every case).

Every case compares dW and dB with the float64 restatement (oracle/nerf_np.py) at the GPU's own ReLU
decisions, at the project's bars -- dW per element |err| <= 1e-5 |want| + 1e-4 x the column's own max
(test_gpu_native.py::test_full_size_all_rays_float64, test_gpu_edge.py), dB within TOL64
(fused_parity.py) -- and runs twice for bitwise run-to-run equality.

The split of a layer (lnerf_fused.hip make_layout): a batch is padded to whole 128-sample workgroups,
blocks = 4 ceil(rays / (128 / S)), half-blocks hbs = 2 blocks; layer l gets
splits_l = clamp(floor(grid (kt_l + nt_l) / sum_l (kt_l + nt_l)), 1, blocks) workgroups of
per_l = ceil(hbs / splits_l) half-blocks each, the last ones shorter or empty. LNERF_OPT_DW_GRID
accepts 16 .. 4096. `split_lengths` below restates that formula, and the tests assert the lengths
they claim to cover."""
import os

import numpy as np
import pytest

import nerf_np
from fused_parity import TOL64, encoded_input, padded, run_fused
from loma_calls import assert_close

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F16X3, BF16X6 = 256, 512   # lnerf.MFMA_F16X3 (fp16x3 exactly, no floor guard), lnerf.MFMA_BF16X6
DW_COL_TOL = 1e-4


def split_lengths(dims, rays, S, grid, tile=128):
    """Per layer, the half-blocks each dW split holds (make_layout's formula; dw_split's ranges)."""
    kt = [(k + 31) // 32 for k in dims[:-1]]
    nt = [(n + 31) // 32 for n in dims[1:]]
    rpw = 1 if S >= tile else tile // S
    blocks = -(-rays // rpw) * (tile // 32)
    hbs = 2 * blocks
    tiles_sum = sum(k + n for k, n in zip(kt, nt))
    out = []
    for k, n in zip(kt, nt):
        sp = min(max(grid * (k + n) // tiles_sum, 1), blocks)
        per = -(-hbs // sp)
        out.append([min(hbs, min(hbs, i * per) + per) - min(hbs, i * per) for i in range(sp)])
    return out


def mlp_workload(dims, rays, samples, seed):
    """The cfg2 rays (33 encoded inputs) with an MLP of the given widths."""
    w = nerf_np.make_workload("cfg2", rays=rays, samples=samples)
    assert dims[0] == w.X.shape[1] and dims[-1] == 4
    rng = np.random.RandomState(seed)
    ws = [(rng.randn(k, n) * np.sqrt(2.0 / k)).astype(np.float32) for k, n in zip(dims, dims[1:])]
    bs = [(rng.randn(n) * 0.5).astype(np.float32) for n in dims[1:]]
    wp, bp = nerf_np.pad_weights(ws, bs)
    return nerf_np.Workload(w.pts, w.pts32, w.X, w.dists, w.target, ws, bs, wp, bp, w.F, w.S, w.N)


def dw_inside_bar(got, want, shapes):
    """Equal NaN patterns and every finite element inside 1e-5 |want| + DW_COL_TOL x its column's max."""
    worst = 0.0
    for l, (k, n) in enumerate(shapes):
        w = np.asarray(want[l, :k, :n], np.float64)
        fin = ~np.isnan(w)
        assert np.array_equal(np.isnan(got[l, :k, :n]), ~fin), l
        w = np.where(fin, w, 0.0)
        err = np.abs(np.where(fin, got[l, :k, :n] - w, 0.0))
        lim = 1e-5 * np.abs(w) + DW_COL_TOL * np.abs(w).max(axis=0, keepdims=True)
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (l, worst)
    return worst


_REFS = {}


def reference(key, w, masks):
    """float64 at the GPU's ReLU decisions, computed once per workload and precision; k1 takes the
    decisions, which no dW grid changes."""
    if key not in _REFS:
        r = nerf_np.nerf_forward_backward_chunked(encoded_input(w, True), w.ws, w.bs, w.dists, w.target, w.S,
                                                  seed=1.0, masks=masks, rays_per_chunk=256)
        _REFS[key] = (padded(r["dW"], w.wp.shape), padded(r["db"], w.bp.shape), [m.copy() for m in masks])
    dW, dB, m0 = _REFS[key]
    for a, b in zip(m0, masks):
        assert np.array_equal(a, b)
    return dW, dB


def check(engine, key, w, flags, grid):
    import lnerf
    engine.set_option(lnerf.OPT_DW_GRID, grid)
    try:
        a = run_fused(engine, w, seed=1.0, flags=flags)
        path = engine.last_path()
        b = run_fused(engine, w, seed=1.0, flags=flags)
    finally:
        engine.set_option(lnerf.OPT_DW_GRID, 0)
    assert path["k16"] and path["dw16"] and path["planes"] == (3 if flags & BF16X6 else 2), path
    for k in ("dW", "dB"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, "run to run")
    dW, dB = reference((key, flags), w, a["masks"])
    worst = dw_inside_bar(a["dW"], dW, [x.shape for x in w.ws])
    assert_close("dB", a["dB"], dB, **TOL64)
    print(f"{key} flags {flags} grid {grid}: worst dW error / column bar {worst:.3g}")


DIMS_RANGE = [33, 256, 256, 4]
# (rays, grid) -> the half-blocks of the hidden layer's (256 -> 256, the FULL 2 x 4 loop) splits
RANGE_CASES = {
    (20, 16): [3, 3, 3, 3, 3, 1, 0],
    (20, 18): [2] * 8,
    (128, 16): [10] * 6 + [4],
    (128, 32): [5] * 12 + [4, 0],
    (128, 35): [4] * 16,
    (128, 50): [3] * 21 + [1],
}


@pytest.mark.parametrize("flags", [F16X3, BF16X6])
@pytest.mark.parametrize("rays,grid", list(RANGE_CASES))
def test_range_lengths(engine, rays, grid, flags):
    """MLP 33 -> 256 -> 256 -> 4 at 8 samples per ray. 20 rays are 160 samples, padded to two
    128-sample workgroups: 8 blocks, 16 half-blocks, of which the last six hold only padding. The
    weights (kt + nt) are 10, 16, 9 of 35, so at the smallest accepted grid the hidden layer already
    gets floor(16 x 16 / 35) = 7 splits of ceil(16 / 7) = 3 half-blocks (3 3 3 3 3 1 0: a whole triple,
    a range shorter than the rotation's depth, an empty split) and from grid 18 on 8 splits of 2:
    ranges of 4, 5 and 10 half-blocks do not exist at 20 rays under any accepted grid. 128 rays x 8
    samples (32 blocks, 64 half-blocks) reach them in the same hidden layer:

      grid 16 -> 7 splits  of 10 (the last 4)        grid 35 -> 16 splits of 4
      grid 32 -> 14 splits of 5 (then 4, then empty)  grid 50 -> 22 splits of 3 (the last 1)

    which is every residue of the three-step rotation (10 = 3 x 3 + 1, 5 = 3 + 2, 3), ranges shorter
    than its depth (2, 1, 0) and last splits shorter than the rest. Layer 0 (1 x 2 tile blocks) and
    the head (1 x 1) run through the same loop in every case, at their own range lengths."""
    lens = split_lengths(DIMS_RANGE, rays, 8, grid)
    assert lens[1] == RANGE_CASES[(rays, grid)], lens
    w = mlp_workload(DIMS_RANGE, rays, 8, seed=11)
    check(engine, ("range", rays), w, flags, grid)


# half-blocks of a split's range that one fill of the scale table covers (lnerf_dw16.hip dw_chunk_hb:
# what 160 KiB of LDS leave beside the images, at most 720); a longer range runs chunk by chunk
CHUNK_HB = {F16X3: 720, BF16X6: 504}


@pytest.mark.parametrize("flags", [F16X3, BF16X6])
def test_ranges_longer_than_the_scale_table(engine, flags):
    """The bench MLP (33 -> 256 x 7 -> 4, weights 10, 16 x 6, 9 of 115) on 1024 rays x 64 samples =
    4096 half-blocks at the smallest grid, 16: every hidden layer gets floor(16 x 16 / 115) = 2 splits
    of 2048 half-blocks, i.e. 3 chunks under fp16x3 (720 + 720 + 608) and 5 under bf16x6 (4 x 504 +
    32); layer 0 (1 x 2 blocks) and the head (1 x 1) get one split of 4096 each, 6 and 9 chunks. What
    a chunk boundary can break: the next chunk's prologue starts on image 0 (chunks are even and
    whole triples), overwrites the zero planes the previous chunk's last step left there, the db sums
    take the boundary half-block once, and the accumulators live through the re-entered prologue."""
    dims = [33] + [256] * 7 + [4]
    lens = split_lengths(dims, 1024, 64, 16)
    assert lens[1] == [2048, 2048] and lens[0] == [4096] and lens[-1] == [4096], lens
    ch = CHUNK_HB[flags]
    assert ch % 6 == 0 and -(-2048 // ch) == (3 if flags == F16X3 else 5) and -(-4096 // ch) >= 6
    w = nerf_np.make_workload("cfg3", rays=1024)
    assert [x.shape[0] for x in w.ws] + [4] == dims
    check(engine, "chunks", w, flags, 16)


@pytest.mark.parametrize("flags", [F16X3, BF16X6])
def test_non_full_widths(engine, flags):
    """Widths 160 and 96 (33 -> 160 -> 96 -> 160 -> 4) at 64 samples: 5 and 3 feature tiles, so the
    hidden layers take the non-FULL 2 x 4 loop with tiles past the layer (never split, never read)
    and inactive waves (160 -> 96: 3 x 1 tile blocks on 3 of the 8 waves; 96 -> 160: 2 x 2 on 4);
    layer 0 runs 1 x 2 blocks on 6 waves and the head 1 x 1 on 5."""
    dims = [33, 160, 96, 160, 4]
    w = mlp_workload(dims, 8, 8, seed=12)
    for grid in (16, 0):
        check(engine, "widths", w, flags, grid)


def load(name):
    return dict(np.load(os.path.join(HERE, "golden", name), allow_pickle=False))


def run_fixture(engine, g, flags):
    import lnerf
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    mlp = lnerf.make_mlp(shapes, g["wp"].shape[1], g["wp"].shape[2])
    r = engine.train_step(mlp, d(g["wp"]), d(g["bp"]), d(g["X"]), d(g["dists"]), d(g["target"]),
                          samples=int(g["S"]), input_mode=lnerf.INPUT_ENCODED, seed=1.0, want_per_ray=True,
                          flags=flags | lnerf.FAST)
    torch.cuda.synchronize()
    return dict(dW=r.d_ws.cpu().numpy(), dB=r.d_bs.cpu().numpy()), shapes


# (fixture, flags) -> (exceptional_rows(split=True), guard_fired()) of the parent commit's kernel on
# the MI355X (the scale table and the branch-free shifts must classify every row as it did). Under
# an explicit precision the step has no guard (-1 by construction); the default flags (0) run it:
# edge_finite_6x8 fires it (the step re-runs on bf16x6; the counts are the primary fp16x3 step's),
# edge_band_4x8 does not.
PARENT_SPECIAL = {
    ("edge_finite_6x8.npz", F16X3): ((69, 0), -1),
    ("edge_finite_6x8.npz", BF16X6): ((0, 0), -1),
    ("edge_finite_6x8.npz", 0): ((69, 0), 1),
    ("edge_band_4x8.npz", F16X3): ((12, 12), -1),
    ("edge_band_4x8.npz", BF16X6): ((0, 0), -1),
    ("edge_band_4x8.npz", 0): ((12, 12), 0),
}
# edge_finite_6x8's dW columns that fp16x3's k1 loses before k2 sees them (test_gpu_edge.py: layers
# 0-1, column 6, made of G elements 2^28 .. 2^42 below their row's maximum, 0.3-0.7 % of the column)
K1_LOST = {(0, 6), (1, 6)}


@pytest.mark.parametrize("name,flags", list(PARENT_SPECIAL))
def test_special_rows_at_range_ends(engine, name, flags):
    """The edge fixtures (8 -> 8 -> 8 -> 4; 48 and 32 samples, i.e. 3 and 2 half-blocks of real rows
    in splits of 2): all-zero rows, rows above the layer's scale (every ray's last sample, the row
    that ends a half-block) and rows below it sit at the first and last positions of a split's
    range. The exceptional-row counts and the guard state equal the parent commit's, and both runs
    agree bit for bit. dW: under bf16x6, and under the default flags where the guard re-ran the
    step on bf16x6, the column bar against the fixture's oracle values. Under fp16x3 on
    edge_finite_6x8 -- where the main loop must drop the 69 exceptional rows the table zeroes, or
    they are multiplied twice -- the column bar against the explicit bf16x6 run of the same step,
    except the two columns k1 loses (K1_LOST), which stay within 1 % of their column's maximum (the
    documented loss is 0.3-0.7 %; a row counted twice is an error of the size of the row)."""
    g = load(name)
    a, shapes = run_fixture(engine, g, flags)
    rows, fired = engine.exceptional_rows(split=True), engine.guard_fired()
    b, _ = run_fixture(engine, g, flags)
    for k in ("dW", "dB"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, "run to run")
    assert (rows, fired) == PARENT_SPECIAL[(name, flags)], (rows, fired)
    if flags == BF16X6 or fired == 1:
        dw_inside_bar(a["dW"], g["dW"], shapes)
        assert_close("dB", a["dB"], g["dB"], **TOL64)
    if flags == F16X3 and name == "edge_finite_6x8.npz":
        ref, _ = run_fixture(engine, g, BF16X6)
        for l, (k, n) in enumerate(shapes):
            want = ref["dW"][l, :k, :n].astype(np.float64)
            err = np.abs(a["dW"][l, :k, :n] - want)
            cmax = np.abs(want).max(axis=0, keepdims=True)
            over = err / np.maximum(1e-5 * np.abs(want) + DW_COL_TOL * cmax, 1e-300)
            print(f"fp16x3 vs bf16x6 layer {l}: worst error / column bar per column {np.round(over.max(axis=0), 3)}")
            for j in range(n):
                if (l, j) in K1_LOST:
                    assert (err[:, j] <= 1e-2 * cmax[0, j]).all(), (l, j, float(over[:, j].max()))
                else:
                    assert (over[:, j] <= 1.0).all(), (l, j, float(over[:, j].max()))


@pytest.mark.parametrize("flags", [0, F16X3, BF16X6])
def test_nan_row_at_range_ends(engine, flags):
    """test_gpu_edge.py::test_nan_input_row_propagates' pattern at 32 samples (cfg2, 4 rays x 8): the
    splits hold 2 half-blocks, so samples 0 and 31 are the first and the last row of split 0's
    range. dW_0 is NaN in exactly the float64 restatement's rows, everything else finite and close.
    Under fp16x3 the int24 slabs carry the rows as k1's non-finite mark, which the scale table hands
    to the split."""
    w = nerf_np.make_workload("cfg2", rays=4, samples=8)
    shapes = [x.shape for x in w.ws]
    # (one 128-sample workgroup = 8 half-blocks, the last 6 padding: 4 splits of 2 per layer)
    assert all(n == [2, 2, 2, 2] for n in split_lengths([33, 30, 30, 4], 4, 8, 256))
    X = w.X.copy()
    X[0, 7] = np.nan
    X[31, 0] = np.nan
    g = dict(X=X, wp=w.wp, bp=w.bp, dists=w.dists, target=w.target, S=w.S, shapes=np.array(shapes))
    a, _ = run_fixture(engine, g, flags)
    path = engine.last_path()
    b, _ = run_fixture(engine, g, flags)
    assert np.array_equal(a["dW"], b["dW"], equal_nan=True)
    if not flags & BF16X6:
        assert path["a24"], path
    with np.errstate(all="ignore"):
        r = nerf_np.nerf_forward_backward(X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0)
    assert np.isnan(r["dW"][0][7]).all() and np.isnan(r["dW"][0][0]).all()
    for l, (k, n) in enumerate(shapes):
        want = r["dW"][l]
        assert np.array_equal(np.isnan(a["dW"][l, :k, :n]), np.isnan(want)), (l, flags)
        fin = np.isfinite(want)
        scale = np.abs(np.where(fin, want, 0)).max()
        err = np.abs(np.where(fin, a["dW"][l, :k, :n] - want, 0))
        assert (err <= 1e-5 * np.abs(np.where(fin, want, 0)) + 1e-5 * scale).all(), (l, flags, float(err.max()))
