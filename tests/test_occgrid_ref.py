"""CPU tests of the occupancy-grid checker (tests/occgrid_ref.py) and of the workloads the GPU tests run
(tests/occgrid_workloads.py): properties the formulas of include/lnerf.h "Occupancy grid" must have,
checked against a separate brute-force march written in scalar Python, and the conditions the inputs
must meet before a bit-for-bit comparison on them means anything. No GPU is needed.
"""
import math

import numpy as np
import pytest

import occgrid_ref as oref
import occgrid_workloads as owl

ALL_CASES = range(len(owl.SAMPLER_CASES))


def _f32(x):
    return float(np.float32(x))


def brute_march(c, ray):
    """The occupied steps of one ray, scalar Python floats (float64), one step at a time."""
    res, M = c["res"], c["M"]
    near, far = _f32(c["near"]), _f32(c["far"])
    on = oref.unpack_bits(c["bits"], res)
    o = [float(v) for v in ray[:3]]
    d = [float(v) for v in ray[3:]]
    h = (far - near) / M
    out = []
    for i in range(M):
        t = near + (i + 0.5) * h
        cell, inside = 0, True
        for a in range(3):
            w = ((o[a] + d[a] * t) - (-1.0)) / 2.0
            if not (0.0 <= w < 1.0):         # a NaN fails
                inside = False
                break
            cell += min(int(w * res), res - 1) * res ** a
        if inside and on[cell]:
            out.append(i)
    return out


def _sample(c, u=None, flags=0):
    return oref.sample(c["res"], owl.LO, owl.HI, c["bits"], c["rays"], c["S"], c["M"], c["near"], c["far"], u, flags)


@pytest.mark.parametrize("M,S", [(64, 1), (64, 2), (64, 64), (128, 64), (128, 128), (192, 3), (1024, 64)])
def test_all_bits_set_is_the_midpoint_linspace(M, S):
    """All bits set, u = None, M a multiple of S: t_j = (float)(near + (j + 0.5) (far - near) / S), and
    n_occ = M for a ray inside the box."""
    res = 8
    bits = owl.bitfield(res, "all")
    rays = np.array([owl.planted_ray("inside", res, M, 2.0, 6.0)], np.float32)
    for near, far in owl.RANGES:
        t, dists, n_occ = oref.sample(res, owl.LO, owl.HI, bits, rays, S, M, near, far)
        want = (near + (np.arange(S) + 0.5) * (far - near) / S).astype(np.float32)
        assert np.array_equal(t[0], want)
        assert n_occ[0] == M
        assert np.array_equal(dists[0], np.full(S, np.float32((far - near) / S)))


@pytest.mark.parametrize("index", ALL_CASES, ids=[owl.case_id(c) for c in owl.SAMPLER_CASES])
def test_depths_lie_in_occupied_steps_and_do_not_decrease(index):
    c = owl.sampler_case(index)
    near, far, M = _f32(c["near"]), _f32(c["far"]), c["M"]
    h = (far - near) / M
    for u in (None, c["u"]):
        for flags in (0, oref.OCC_LAST_OPAQUE):
            t, dists, n_occ = _sample(c, u, flags)
            assert t.dtype == np.float32 and dists.dtype == np.float32 and n_occ.dtype == np.int32
            assert (np.diff(t, axis=1) >= 0).all()
            for r in range(c["n"]):
                steps = brute_march(c, c["rays"][r])
                assert n_occ[r] == len(steps)
                steps = steps or list(range(M))
                lo = near + np.array(steps) * h
                ulp = np.spacing(np.abs(t[r])).astype(np.float64)
                tt = t[r].astype(np.float64)
                inside = ((tt[:, None] >= lo[None, :] - ulp[:, None]) & (tt[:, None] <= lo[None, :] + h + ulp[:, None]))
                assert inside.any(axis=1).all(), (r, c["kinds"][r])
                share = np.float32(len(steps) * h / c["S"])
                want_d = np.full(c["S"], share)
                if flags:
                    want_d[-1] = np.float32(1e8)
                assert np.array_equal(dists[r], want_d)


@pytest.mark.parametrize("index", ALL_CASES, ids=[owl.case_id(c) for c in owl.SAMPLER_CASES])
def test_no_bit_set_gives_the_all_set_depths(index):
    c = dict(owl.sampler_case(index))
    full = dict(c, bits=owl.bitfield(c["res"], "all"))
    full["rays"] = np.tile(np.array([owl.planted_ray("inside", c["res"], c["M"], c["near"], c["far"])], np.float32),
                           (c["n"], 1))
    empty = dict(full, bits=owl.bitfield(c["res"], "none"))
    t1, d1, n1 = _sample(full, c["u"])
    t0, d0, n0 = _sample(empty, c["u"])
    assert (n1 == c["M"]).all() and (n0 == 0).all()
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and np.array_equal(d0, d1)


def test_workloads_hold_every_planted_kind():
    seen = set()
    axes = dict(res=set(), M=set(), S=set(), n=set())
    less, more, alternating = False, False, 0
    for index in ALL_CASES:
        c = owl.sampler_case(index)
        for k in axes:
            axes[k].add(c[k])
        occ = oref.march(c["res"], owl.LO, owl.HI, c["bits"], c["rays"], c["M"], c["near"], c["far"])
        every = oref.march(c["res"], owl.LO, owl.HI, owl.bitfield(c["res"], "all"), c["rays"], c["M"], c["near"],
                           c["far"])
        for r, kind in enumerate(c["kinds"]):
            N, box = int(occ[r].sum()), every[r]
            if kind == "miss":
                assert not box.any()
            elif kind == "inside":
                assert box.all()
            elif kind == "nan":
                assert np.isnan(c["rays"][r]).any() and not box.any()
            elif kind.startswith("only"):
                step = owl.planted_step(kind, c["M"])
                assert np.flatnonzero(box).tolist() == [step], (kind, np.flatnonzero(box))
                if c["kind"] in ("all", "checker"):
                    assert np.flatnonzero(occ[r]).tolist() == [step]
                    seen.add(kind + "-occupied")
            elif kind == "alt":
                assert box[:c["res"]].all()
                if c["kind"] == "checker":
                    run = occ[r][:c["res"]]
                    assert (run[::2]).all() and not run[1::2].any()
                    alternating = max(alternating, c["res"])
            seen.add(kind)
            if 0 < N < c["S"]:
                less = True
            if N > c["S"]:
                more = True
    assert axes == dict(res={4, 8, 32}, M={64, 128, 1024}, S={1, 3, 64, 65, 200}, n={1, 5, 130}), axes
    assert set(owl.PLANTED) <= seen and "camera" in seen, seen
    for k in ("only0", "only63", "only64", "onlylast"):
        assert k + "-occupied" in seen, k
    assert less and more and alternating == 32
    # 64 is a pass boundary only where M > 64
    assert any(owl.planted_step("only64", owl.sampler_case(i)["M"]) == 64 and "only64" in owl.sampler_case(i)["kinds"]
               and owl.sampler_case(i)["kind"] in ("all", "checker") for i in ALL_CASES)


def test_planted_u_holds_the_special_values():
    u = owl.planted_u(np.random.RandomState(0), 5, 64)
    below_one = np.float32(1) - np.float32(2.0 ** -24)
    assert (u == 0).any() and (u == below_one).any() and (u == 1.5).any() and (u == -1).any() and np.isnan(u).any()
    assert below_one < 1 and np.nextafter(below_one, np.float32(2)) == 1
    got = oref.unit_clamp(np.array([0.0, below_one, 1.5, -1.0, np.nan, 0.25], np.float32))
    assert got.tolist() == [0.0, float(below_one), 1.0, 0.0, 0.0, 0.25]


def test_bits_pack_and_unpack():
    rng = np.random.RandomState(3)
    on = rng.uniform(0, 1, 8 ** 3) < 0.5
    words = oref.pack_bits(on)
    assert words.dtype == np.uint32 and words.size == 8 ** 3 // 32
    assert np.array_equal(oref.unpack_bits(words, 8), on)
    c = 5 + 8 * (2 + 8 * 7)
    one = np.zeros(8 ** 3, bool)
    one[c] = True
    w = oref.pack_bits(one)
    assert w[c >> 5] == np.uint32(1) << np.uint32(c & 31) and np.count_nonzero(w) == 1


def test_cell_points():
    res = 8
    cells, u = owl.cell_list(res)
    p = oref.cell_points(res, owl.LO, owl.HI, cells, u)
    assert p.dtype == np.float32 and p.shape == (cells.size, 3)
    outside = (cells < 0) | (cells >= res ** 3)
    assert outside.sum() == 3 and (p[outside] == 0).all()          # the box centre
    g = np.stack([cells % res, (cells // res) % res, cells // (res * res)], axis=1)[~outside]
    w = (p[~outside].astype(np.float64) + 1.0) / 2.0 * res
    assert (w >= g - 1e-6).all() and (w <= g + 1 + 1e-6).all()
    centres = oref.cell_points(res, owl.LO, owl.HI)
    assert centres.shape == (res ** 3, 3)
    assert np.array_equal(centres[1], np.array([-1 + 3.0 / res, -1 + 1.0 / res, -1 + 1.0 / res], np.float32))
    # a NaN u is 0: the cell's lower corner
    assert np.array_equal(oref.cell_points(res, owl.LO, owl.HI, np.array([0]), np.full((1, 3), np.nan, np.float32))[0],
                          np.array([-1, -1, -1], np.float32))


@pytest.mark.parametrize("res,decay,stride", owl.UPDATE_CASES)
def test_update(res, decay, stride):
    d0 = owl.density(res)
    cells, buf, sigma = owl.update_list(res, stride)
    assert np.array_equal(buf[::stride], sigma, equal_nan=True)
    d1 = oref.update(res, d0, cells, sigma, decay)
    assert d1.dtype == np.float32 and np.isfinite(d1).all() and (d1 >= 0).all()
    base = d0 if decay == 1.0 else d0 * np.float32(decay)
    # scalar Python: the same maximum, one entry at a time
    want = base.copy()
    for c, s in zip(cells.tolist(), sigma.tolist()):
        if 0 <= c < res ** 3 and s > 0:
            want[c] = max(want[c], np.float32(min(s, float(oref.FLT_MAX))))
    assert np.array_equal(d1.view(np.uint32), want.view(np.uint32))
    half = res ** 3 // 2
    k = owl.SPECIAL_SIGMA.size
    alone = d1[half:half + k]
    for i, s in enumerate(owl.SPECIAL_SIGMA):
        if np.isnan(s) or s <= 0:
            assert alone[i] == base[half + i]                       # ignored
        elif np.isinf(s):
            assert alone[i] == oref.FLT_MAX
        else:
            assert alone[i] == max(base[half + i], s)
    uniq, counts = np.unique(cells[(cells >= 0) & (cells < half)], return_counts=True)
    assert (counts > 1).any()                                       # duplicates are there
    assert (d1[half + k:] == base[half + k:]).all()                 # cells nobody names keep the decayed value


@pytest.mark.parametrize("res", [4, 8, 32])
def test_threshold_and_the_mean_condition(res):
    """No cell of any test density lies within res^3 2^-52 mean of the mean (a condition on the inputs):
    the bits under OCC_MEAN cannot depend on the order the mean was summed in."""
    for d in (owl.density(res), oref.update(res, owl.density(res), *owl.update_list(res, 1)[::2], 0.95)
              if res < 32 else owl.density(res, 1)):
        assert oref.mean_margin(res, d) > 1e6
        bits, mean, occupied = oref.threshold(res, d, 0.01)
        assert occupied == int((d > np.float32(0.01)).sum()) == int(oref.unpack_bits(bits, res).sum())
        assert math.isclose(mean, float(d.astype(np.float64).mean()), rel_tol=1e-12)
        bits_m, mean_m, occ_m = oref.threshold(res, d, 1e9, oref.OCC_MEAN)
        assert mean_m == mean and occ_m == int((d.astype(np.float64) > mean).sum()) and 0 < occ_m < occupied
        assert np.array_equal(oref.threshold(res, d, 0.01, oref.OCC_MEAN)[0], bits)   # min(threshold, mean)
