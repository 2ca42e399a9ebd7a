"""The conditions tests/composite_workloads.py must meet before the GPU tests built on it
(tests/test_gpu_composite.py) mean anything -- CPU only, about 1 s for the whole sweep (every S in
1 .. 128 and 129, 200, 257):

  coverage    every profile starts in each of the k16 tile's two waves and each of kr's four; every
              walled profile has its wall in a later wave than its ray's first sample; a wall sits on
              the last lane of a wave (the transmittance dies exactly at the boundary) and on the first
              lane of the next; S = 63, 64, 65, 127, 128 are swept;
  opacity     every ray with a sample of sigma > 0 has a float64 opacity in (0.01, 1 + 1e-9] -- but
              last_only, see test_opacity -- and an empty ray is exactly 0 in every output;
  references  the loma-order fp32 C oracle is within half of every bar of test_gpu_composite.py from the
              float64 restatement, which is why float64 may referee the tau profiles;
  exactness   every input is bf16-representable and no row spans more than 2^14.

Worst C oracle / float64 error over its bar, measured on this sweep (the draft of the profiles had
0.06 / 0.22 / 0.27 / 0.21 / 0.18 / 0.083): acc 0.059, d_target 0.027, d_dists 0.26, dX rgb group
0.069, dX sigma columns 0.034, dW per column 0.104, dB per layer 0.091; the loss 9.8e-7 of itself (a
sequential fp32 sum of up to 513 rays' losses, printed and not asserted).
"""
import numpy as np
import pytest

import composite_workloads as cw
import scale_workloads as sw

HALF = 0.5
WALLED = ("mid_wall", "wall63", "wall64", "two_walls")
FUSED_SWEEP = tuple(S for S in cw.SWEEP if S <= 128)


def test_sweep_and_ray_counts():
    assert set(range(1, 129)) | {129, 200, 257} == set(cw.SWEEP)
    assert {63, 64, 65, 127, 128} <= set(cw.SWEEP)
    assert set(cw.SEMANTIC_S) <= set(cw.SWEEP)
    for S in cw.SWEEP:
        w = cw.workload(S)
        assert w.N == (2 * (256 // S) + 1 if S <= 256 else 3)
        assert w.X.shape == (w.N * S, 8) and w.dists.shape == w.sample_t.shape == w.sigma.shape == (w.N, S)
        assert w.profiles == tuple(cw.PROFILES[(i + S) % len(cw.PROFILES)] for i in range(w.N))
        # non-uniform dists behind the reference's trailing 1e8, sample_t their running sum from 2
        assert (w.dists[:, -1] == np.float32(1e8)).all()
        assert ((w.dists[:, :-1] >= 0.25) & (w.dists[:, :-1] <= 1.0)).all()
        if S >= 8:
            assert (np.ptp(w.dists[:, :-1], axis=1) > 0).all()
        assert (w.sample_t[:, 0] == 2.0).all()
        assert np.allclose(np.diff(w.sample_t.astype(np.float64), axis=1), w.dists[:, :-1], rtol=1e-5, atol=0)
        assert cw.workload(S) is w   # one object per S: shared, read-only
        assert not w.X.flags.writeable


@pytest.mark.parametrize("tile,waves", [(128, 2), (256, 4)])
def test_coverage(tile, waves):
    starts = {p: set() for p in cw.PROFILES}
    later = {p: 0 for p in WALLED}
    dies_at_boundary = starts_next_wave = straddlers = 0
    for S in FUSED_SWEEP:
        w = cw.workload(S)
        for i, p in enumerate(w.profiles):
            w0, w1, rl, _ = cw.tile_position(i, S, tile)
            starts[p].add(w0)
            straddlers += w1 > w0
            for j in w.walls[i]:
                lane, wave = (rl * S + j) & 63, (rl * S + j) >> 6
                if p in later and wave > w0:
                    later[p] += 1
                if j < S - 1 and w1 > wave:          # the ray goes on into another wave behind the wall
                    dies_at_boundary += lane == 63
                if j > 0 and lane == 0 and wave > w0:
                    starts_next_wave += 1
    for p, s in starts.items():
        assert s == set(range(waves)), (p, s)
    for p, n in later.items():
        assert n >= 1, p
    assert dies_at_boundary >= 1 and starts_next_wave >= 1 and straddlers >= 100
    print(f"tile {tile}: walls in a later wave {later}, on lane 63 with the ray going on {dies_at_boundary}, "
          f"on lane 0 of a later wave {starts_next_wave}, rays straddling waves {straddlers}")


def test_position_classes():
    for S in cw.SEMANTIC_S:
        for tile in (128, 256):
            pc = cw.position_classes(S, tile, cw.num_rays(S))
            rpw = tile // S
            assert cw.tile_position(pc["first"], S, tile)[2] == 0
            assert cw.tile_position(pc["last"], S, tile)[2] == rpw - 1
            if pc["straddle"] is not None:
                w0, w1, _, _ = cw.tile_position(pc["straddle"], S, tile)
                assert w1 > w0
            else:
                assert all(cw.tile_position(i, S, tile)[0] == cw.tile_position(i, S, tile)[1] for i in range(rpw))


def test_opacity():
    """(0.01, 1) of the float64 opacity, with the two things the reference's inclusive transmittance and its
    c = (1 - alpha) + 1e-10 force: a ray opaque at its FIRST sample (T_0 = 1 by definition) has w_0 = 1 and
    every later w_j ~ 1e-10 on top, so the upper end is 1 + 1e-9; and a ray whose one non-empty sample is
    its last (last_only; gaps at S = 2) has
    alpha = 1 behind delta = 1e8, T = c = 1e-10: opacity 1e-10, asserted as such (S = 1: w_0 = 1)."""
    for S in cw.SWEEP:
        w = cw.workload(S)
        f, c = cw.reference64(w), cw.reference_c(w)
        for i, p in enumerate(w.profiles):
            o = f["opacity"][i]
            rows = slice(i * S, (i + 1) * S)
            if not (w.sigma[i] > 0).any():           # empty, and gaps at S = 1
                assert p in ("empty", "gaps")
                for r in (f, c):
                    assert (np.asarray(r["acc"][i]) == 0).all() and (np.asarray(r["d_dists"][i]) == 0).all()
                    assert (np.asarray(r["dX"][rows]) == 0).all()
                    assert np.array_equal(np.asarray(r["d_target"][i], np.float64), 2.0 * w.target[i].astype(np.float64))
                assert o == 0 and (f["weights"][i] == 0).all()
            elif S > 1 and not (w.sigma[i, :-1] > 0).any():   # last_only, and gaps at S = 2
                assert p in ("last_only", "gaps") and 0.9e-10 < o < 1.1e-10, (S, i, p, o)
            else:
                assert 0.01 < o <= 1.0 + 1e-9, (S, i, p, o)
        assert all(p != "empty" or not (w.sigma[i] > 0).any() for i, p in enumerate(w.profiles))


def test_c_oracle_within_half_of_every_bar_of_float64():
    assert set(cw.C_ORACLE_ONLY) <= {("front_wall", "d_dists")}
    worst, loss = {}, 0.0
    for S in cw.SWEEP:
        w = cw.workload(S)
        f, c = cw.reference64(w), cw.reference_c(w)
        for k, v in cw.step_ratios(c, w, f).items():
            out = "dX" if k.startswith("dX") else k
            keep = np.array([(p, out) not in cw.C_ORACLE_ONLY for p in w.profiles])
            worst[k] = max(worst.get(k, 0.0), float(v[keep].max(initial=0.0)))
        worst["dW"] = max(worst.get("dW", 0.0), max(sw.dw_col_over_bar(c["dW"], f["dW"], w.shapes)))
        worst["dB"] = max(worst.get("dB", 0.0), max(sw.db_layer_over_bar(c["dB"], f["dB"], w.shapes)))
        loss = max(loss, abs(c["loss"] - f["loss"]) / abs(f["loss"]))
    # (the loss is not held to half its 1e-6: the oracle adds up to 513 rays' losses one after the other)
    print("C oracle / float64, worst error over the bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f"; loss {loss:.3g} of itself")
    for k, v in worst.items():
        assert v <= HALF, (k, v, worst)


def test_exactness():
    """Every input is bf16-representable (the trailing 1e8 of dists is the reference's and goes through no
    MLP), every row's largest / smallest nonzero element at most 2^14 apart, and the identity MLP's float32
    forward gives z_c = x_c - x_{c+4} bit for bit."""
    for S in cw.SWEEP:
        w = cw.workload(S)
        assert np.array_equal(cw.bf16(w.X), w.X) and np.array_equal(cw.bf16(w.target), w.target)
        assert np.array_equal(cw.bf16(w.dists[:, :-1]), w.dists[:, :-1])
        a = np.abs(w.X)
        lo = np.where(a > 0, a, np.inf).min(axis=1)
        assert (a.max(axis=1) > 0).all() and (a.max(axis=1) <= 2.0 ** 14 * lo).all(), S
        rgb = a[:, cw.RGB_COLS]
        assert ((rgb == 0) | ((rgb >= 2.0 ** -6) & (rgb <= 2.0))).all()
        assert ((a[:, 3] == 0) | ((a[:, 3] >= 2.0 ** -5) & (a[:, 3] <= 160.0))).all()
        assert ((w.X[:, 3] > 0) != (w.X[:, 7] == 1)).all()      # sigma > 0, or empty through x7 = 1
        h = w.X
        for l in range(2):
            h = np.maximum(h @ w.ws[l] + w.bs[l], np.float32(0))
        z = h @ w.ws[2] + w.bs[2]
        assert z.dtype == np.float32 and np.array_equal(z, w.X[:, :4] - w.X[:, 4:])
        assert np.array_equal(np.maximum(z[:, 3], 0).reshape(w.N, S), w.sigma)


@pytest.mark.parametrize("nan", [False, True])
def test_semantic_kinds_are_what_they_say(nan):
    """The C oracle on semantic(S): the finite list is finite everywhere and runs the transmittance into
    fp32's subnormals (subnormal d_dists exist from S = 8 on); the nan list has NaN in dX exactly on its
    `nan` rays' marked samples and in dW; sigma0 rays are exactly empty."""
    for S in cw.SEMANTIC_S:
        w = cw.semantic(S, nan)
        assert w.N == cw.num_rays(S) and set(w.profiles) <= set(cw.SEMANTIC_NAN if nan else cw.SEMANTIC_FINITE)
        with np.errstate(all="ignore"):
            c = cw.reference_c(w)
        kinds = np.array(w.profiles)
        assert (c["acc"][kinds == "sigma0"] == 0).all() and np.isfinite(c["acc"]).all() and np.isfinite(c["loss"])
        dX = c["dX"].reshape(w.N, S, 8)
        if nan:
            bad = np.isnan(dX).any(axis=(1, 2))
            assert np.array_equal(bad, kinds == "nan") and np.isnan(c["dW"]).any()
            assert (np.isnan(dX).any(axis=2).sum(axis=1)[bad] == 1).all()
        else:
            for k in ("dX", "dW", "dB", "d_dists", "d_target"):
                assert np.isfinite(c[k]).all(), (S, k)
            sub = (np.abs(c["d_dists"]) > 0) & (np.abs(c["d_dists"]) < np.finfo(np.float32).tiny)
            assert sub.any() or S < 8, S
            # tiny and sigma_tiny: alpha underflows in front of the last sample, whose delta = 1e8 carries the ray
            for kind in ("tiny", "sigma_tiny"):
                assert (np.abs(dX[kinds == kind][:, -1, 3]) > 1e6 * np.abs(dX[kinds == kind][:, :-1, 3]).max(initial=0)).all()


def test_map_ratios_are_compositing_ratios_bars():
    """render_maps_ref.map_ratios (per ray, what the sweep reports) and
    test_gpu_render_maps.compositing_ratios (the worst ray, asserted) are the same bars: on float32
    roundings of the float64 maps their worst ratios are equal."""
    import types
    import render_maps_ref as ref
    from test_gpu_render_maps import compositing_ratios
    for S in (1, 7, 65, 128):
        w = cw.workload(S)
        z = (w.X[:, :4] - w.X[:, 4:]).astype(np.float64)
        rgba = np.concatenate([1 / (1 + np.exp(-z[:, :3])), np.maximum(z[:, 3:], 0)], axis=1).astype(np.float32)
        m = ref.composite64(rgba[:, :3].reshape(w.N, S, 3), rgba[:, 3].reshape(w.N, S), w.dists, w.sample_t)
        out = {k: np.asarray(v, np.float32) for k, v in m.items()}
        out["rgba"] = rgba
        inp = types.SimpleNamespace(N=w.N, S=S, dists_np=w.dists, t_np=w.sample_t)
        a = compositing_ratios(out, inp)
        b = ref.map_ratios(out, w.dists, w.sample_t, S)
        assert set(a) == set(b) and all(a[k] == b[k].max() for k in a), (S, a, {k: v.max() for k, v in b.items()})
        assert max(a.values()) <= 1.0 and (S == 1 or max(a.values()) > 0)


def test_semantic_decidable_columns_and_loss_bars():
    """Test C's rule leaves most of dW checked (every live column up to S = 30, 14 of 20 at worst) and the
    loss bar within 6e-6; the sequential CPU evaluation is the C oracle's own order and stays within half
    of close_grouped's bar of it on every per-ray output, so composite_fp32 restates the oracle."""
    for S in cw.SEMANTIC_S:
        w, c = cw.semantic(S), cw.semantic_reference(S, False)
        cols, loss_bar = cw.semantic_decidable(S)
        live = np.array([[n < k[1] for n in range(cols.shape[1])] for k in w.shapes])
        n = int((cols & live).sum())
        assert n >= 14 and (S > 30 or n == live.sum()), (S, n)
        assert 1e-6 <= loss_bar <= 6e-6 and 1e-6 <= cw.semantic_nan_loss_bar(S) <= 6e-6, S
        e = cw.composite_fp32(w, False)
        for k, v in cw.step_ratios(e, w, c).items():
            assert v.max() <= 0.5, (S, k, float(v.max()))
