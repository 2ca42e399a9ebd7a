"""GPU tests of the occupancy grid (include/lnerf.h "Occupancy grid"): lnerf_occgrid_cell_points,
lnerf_occgrid_update, lnerf_occgrid_threshold and lnerf_sample_occupancy against the numpy checker of
tests/occgrid_ref.py on the cases of tests/occgrid_workloads.py, their guard bands and error paths, and
one end-to-end flow (sample, render, refresh).

Bars:
  * sample_t, dists, n_occ, the cell points, the density and the bits are float64 / integer formulas of a
    few operations, rounded once at most: the checker evaluates the same operations, so they are
    bit-equal, and bit-equal again on a second call;
  * the mean: res^3 2^-52 mean (any float64 summation order of res^3 non-negative terms);
  * the end-to-end maps: tests/render_maps_ref.py's bars, from the GPU's own rgba.
Every test here fails on a library without the occupancy grid: Engine.lib has no such symbols.
"""
import ctypes

import numpy as np
import pytest

import occgrid_ref as oref
import occgrid_workloads as owl

pytestmark = pytest.mark.gpu

SENT = -7.25          # no depth, dist, point coordinate or density of these cases can hold it
ISENT = -77           # nor can a step count or a word of these bitfields
PAD = 3


def _dev(a):
    import torch
    a = np.array(a, order="C")          # a copy: the cached workloads are read-only
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _guarded(n, dtype="float32"):
    """(whole buffer, the n values in its middle): PAD sentinels on either side."""
    import torch
    dt = getattr(torch, dtype)
    full = torch.full((n + 2 * PAD,), ISENT if dtype != "float32" else SENT, dtype=dt, device="cuda:0")
    return full, full[PAD:PAD + n]


def _intact(full, n, what):
    a = _np(full)
    sent = SENT if a.dtype.kind == "f" else ISENT
    assert (a[:PAD] == sent).all() and (a[PAD + n:] == sent).all(), f"{what}: a guard band was written"
    return a[PAD:PAD + n].copy()


def _untouched(full, what):
    a = _np(full)
    assert (a == (SENT if a.dtype.kind == "f" else ISENT)).all(), f"{what} was written"


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _grid(res, lo=owl.LO, hi=owl.HI):
    import lnerf
    return lnerf.OccGrid(res, lo, hi)


# ---- 1. the sampler ---------------------------------------------------------------------------------

def _raw_sample(engine, occ, c, bits, rays, u, flags, t, d, k, S=None, M=None, near=None, far=None, n=None):
    return engine.lib.lnerf_sample_occupancy(
        ctypes.byref(occ.struct), _ptr(bits), _ptr(rays), c["n"] if n is None else n, c["S"] if S is None else S,
        c["M"] if M is None else M, c["near"] if near is None else near, c["far"] if far is None else far, _ptr(u),
        flags, _ptr(t), _ptr(d), _ptr(k), None)


@pytest.mark.parametrize("index", range(len(owl.SAMPLER_CASES)), ids=[owl.case_id(c) for c in owl.SAMPLER_CASES])
def test_sampler_is_the_checker_bit_for_bit(engine, index):
    """With and without u, with and without LNERF_OCC_LAST_OPAQUE: all three outputs bit-equal to the
    checker, again on a second call, behind intact guard bands; each NULL output leaves the others' bits
    unchanged."""
    import lnerf
    c = owl.sampler_case(index)
    n, S = c["n"], c["S"]
    occ = _grid(c["res"])
    bits, rays = _dev(c["bits"]), _dev(c["rays"])
    for u in (None, c["u"]):
        ud = None if u is None else _dev(u)
        for flags in (0, oref.OCC_LAST_OPAQUE):
            want_t, want_d, want_k = oref.sample(c["res"], owl.LO, owl.HI, c["bits"], c["rays"], S, c["M"], c["near"],
                                                 c["far"], u, flags)
            for call in range(2):
                (ft, t), (fd, d), (fk, k) = _guarded(n * S), _guarded(n * S), _guarded(n, "int32")
                assert _raw_sample(engine, occ, c, bits, rays, ud, flags, t, d, k) == 0, lnerf.last_error()
                got_t, got_d, got_k = _intact(ft, n * S, "sample_t"), _intact(fd, n * S, "dists"), _intact(fk, n, "n_occ")
                assert np.array_equal(got_k, want_k), (call, got_k, want_k)
                assert np.array_equal(_bits(got_t), _bits(want_t.reshape(-1))), call
                assert np.array_equal(_bits(got_d), _bits(want_d.reshape(-1))), call
            assert (np.diff(got_t.reshape(n, S), axis=1) >= 0).all()
            # each output alone
            for keep in range(3):
                (ft, t), (fd, d), (fk, k) = _guarded(n * S), _guarded(n * S), _guarded(n, "int32")
                outs = [t if keep == 0 else None, d if keep == 1 else None, k if keep == 2 else None]
                assert _raw_sample(engine, occ, c, bits, rays, ud, flags, *outs) == 0, lnerf.last_error()
                if keep == 0:
                    assert np.array_equal(_bits(_intact(ft, n * S, "sample_t")), _bits(want_t.reshape(-1)))
                    _untouched(fd, "dists"), _untouched(fk, "n_occ")
                elif keep == 1:
                    assert np.array_equal(_bits(_intact(fd, n * S, "dists")), _bits(want_d.reshape(-1)))
                    _untouched(ft, "sample_t"), _untouched(fk, "n_occ")
                else:
                    assert np.array_equal(_intact(fk, n, "n_occ"), want_k)
                    _untouched(ft, "sample_t"), _untouched(fd, "dists")


def test_sampler_engine_method(engine):
    """Engine.sample_occupancy is the same call: shapes, dtypes, `want`, and its argument checks."""
    c = owl.sampler_case(2)
    occ = _grid(c["res"])
    bits, rays, u = _dev(c["bits"]), _dev(c["rays"]), _dev(c["u"])
    t, d, k = engine.sample_occupancy(occ, bits, rays, c["S"], steps=c["M"], near=c["near"], far=c["far"], u=u,
                                      last_opaque=True)
    want_t, want_d, want_k = oref.sample(c["res"], owl.LO, owl.HI, c["bits"], c["rays"], c["S"], c["M"], c["near"],
                                         c["far"], c["u"], oref.OCC_LAST_OPAQUE)
    assert tuple(t.shape) == (c["n"], c["S"]) == tuple(d.shape) and tuple(k.shape) == (c["n"],)
    assert np.array_equal(_bits(_np(t)), _bits(want_t)) and np.array_equal(_bits(_np(d)), _bits(want_d))
    assert np.array_equal(_np(k), want_k)
    only_t, no_d, no_k = engine.sample_occupancy(occ, bits, rays, c["S"], steps=c["M"], near=c["near"], far=c["far"],
                                                 u=u, want=("t",))
    assert no_d is None and no_k is None and np.array_equal(_bits(_np(only_t)), _bits(want_t))
    with pytest.raises(ValueError):
        engine.sample_occupancy(occ, bits, rays, c["S"], u=u[:, :-1].contiguous())
    with pytest.raises(ValueError):
        engine.sample_occupancy(occ, bits[:-1], rays, c["S"])
    with pytest.raises(ValueError):
        engine.sample_occupancy(occ, bits, rays.double(), c["S"])


# ---- 2. cell points -----------------------------------------------------------------------------------

@pytest.mark.parametrize("res", [4, 8, 32])
def test_cell_points_are_the_checker_bit_for_bit(engine, res):
    import lnerf
    boxes = [(owl.LO, owl.HI), ((-1.5, 0.25, -3.0), (2.0, 0.75, 5.0))]
    cells, u = owl.cell_list(res)
    n = cells.size
    for lo, hi in boxes:
        occ = _grid(res, lo, hi)
        for cl, uu in ((cells, u), (cells, None), (None, None),
                       (None, owl.planted_u(np.random.RandomState(res), res ** 3, 3))):
            m = n if cl is not None else res ** 3
            want = oref.cell_points(res, lo, hi, cl, uu)
            full, p = _guarded(m * 3)
            cd, ud = None if cl is None else _dev(cl), None if uu is None else _dev(uu)
            rc = engine.lib.lnerf_occgrid_cell_points(ctypes.byref(occ.struct), _ptr(cd), m, _ptr(ud), _ptr(p), None)
            assert rc == 0, lnerf.last_error()
            assert np.array_equal(_bits(_intact(full, m * 3, "points")), _bits(want.reshape(-1)))
        got = engine.occgrid_cell_points(occ, _dev(cells), _dev(u))
        assert tuple(got.shape) == (n, 3) and np.array_equal(_bits(_np(got)), _bits(oref.cell_points(res, lo, hi, cells, u)))
    assert tuple(engine.occgrid_cell_points(_grid(res)).shape) == (res ** 3, 3)


# ---- 3. update ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("res,decay,stride", owl.UPDATE_CASES)
def test_update_is_the_checker_bit_for_bit(engine, res, decay, stride):
    import lnerf
    occ = _grid(res)
    d0 = owl.density(res)
    cells, buf, sigma = owl.update_list(res, stride)
    want = oref.update(res, d0, cells, sigma, decay)
    cd, sd = _dev(cells), _dev(buf)
    for call in range(2):
        full, d = _guarded(res ** 3)
        d.copy_(_dev(d0))
        rc = engine.lib.lnerf_occgrid_update(ctypes.byref(occ.struct), _ptr(d), _ptr(cd), cells.size, _ptr(sd), stride,
                                             decay, None)
        assert rc == 0, lnerf.last_error()
        got = _intact(full, res ** 3, "density")
        assert np.array_equal(_bits(got), _bits(want)), call
    assert np.isfinite(got).all() and (got >= 0).all()
    # a second update on top of the first, through the Engine method, every cell in order
    every = owl.density(res, 5)
    d = _dev(got)
    assert engine.occgrid_update(occ, d, _dev(every), decay=decay) is d
    assert np.array_equal(_bits(_np(d)), _bits(oref.update(res, want, None, every, decay)))
    if stride == 4:
        # sigma = rgba + 3: the view's own offset and stride
        rgba = np.random.RandomState(9).uniform(0, 60, (res ** 3, 4)).astype(np.float32)
        d = _dev(d0)
        engine.occgrid_update(occ, d, _dev(rgba).flatten()[3:], decay=decay, sigma_stride=4)
        assert np.array_equal(_bits(_np(d)), _bits(oref.update(res, d0, None, rgba[:, 3], decay)))


# ---- 4. threshold -------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", [4, 32])
def test_threshold(engine, res):
    """bits and occupied exact, the mean within res^3 2^-52 mean, with and without LNERF_OCC_MEAN, each
    output alone, twice. (tests/test_occgrid_ref.py asserts that no cell of these densities is near the
    mean.)"""
    import lnerf
    import torch
    occ = _grid(res)
    d_np = owl.density(res)
    assert oref.mean_margin(res, d_np) > 1
    d = _dev(d_np)
    words = res ** 3 // 32
    for thr, flags in ((0.01, 0), (1e9, oref.OCC_MEAN), (0.01, oref.OCC_MEAN), (2.9, 0), (50.0, 0)):
        want_bits, want_mean, want_occ = oref.threshold(res, d_np, thr, flags)
        for call in range(2):
            fb, b = _guarded(words, "int32")
            fm = torch.full((3,), SENT, dtype=torch.float64, device="cuda:0")
            fo = torch.full((3,), ISENT, dtype=torch.int64, device="cuda:0")
            rc = engine.lib.lnerf_occgrid_threshold(ctypes.byref(occ.struct), _ptr(d), thr, flags, _ptr(b), _ptr(fm[1:2]),
                                                    _ptr(fo[1:2]), None)
            assert rc == 0, lnerf.last_error()
            got_bits = _intact(fb, words, "bits").view(np.uint32)
            m, o = _np(fm), _np(fo)
            assert m[0] == SENT == m[2] and o[0] == ISENT == o[2]
            assert np.array_equal(got_bits, want_bits), (thr, flags)
            assert int(o[1]) == want_occ
            assert abs(m[1] - want_mean) <= res ** 3 * 2.0 ** -52 * want_mean
            if call:
                assert m[1] == first_mean
            first_mean = m[1]
        # each output alone, through the Engine method
        use_mean = bool(flags)
        only_b, no_m, no_o = engine.occgrid_threshold(occ, d, thr, use_mean=use_mean, want=("bits",))
        assert no_m is None and no_o is None and np.array_equal(_np(only_b).view(np.uint32), want_bits)
        no_b, only_m, no_o = engine.occgrid_threshold(occ, d, thr, use_mean=use_mean, want=("mean",))
        assert no_b is None and no_o is None and float(_np(only_m)) == first_mean
        no_b, no_m, only_o = engine.occgrid_threshold(occ, d, thr, use_mean=use_mean, want=("occupied",))
        assert no_b is None and no_m is None and int(_np(only_o)) == want_occ
    assert np.array_equal(_np(d), d_np)


# ---- 5. error paths -----------------------------------------------------------------------------------

def test_errors_write_nothing(engine):
    import lnerf
    import torch
    lib = engine.lib
    c = owl.sampler_case(3)          # res 8, M 64, S 65, 5 rays
    res, n = c["res"], c["n"]
    good = _grid(res)
    bits, rays = _dev(c["bits"]), _dev(c["rays"])
    (ft, t), (fd, d), (fk, k) = _guarded(n * 1100), _guarded(n * 1100), _guarded(n, "int32")
    (fp, p), (fden, den), (fb, b) = _guarded(res ** 3 * 3), _guarded(res ** 3), _guarded(res ** 3 // 32, "int32")
    fm = torch.full((1,), SENT, dtype=torch.float64, device="cuda:0")
    fo = torch.full((1,), ISENT, dtype=torch.int64, device="cuda:0")
    sigma = _dev(np.full(res ** 3, 5.0, np.float32))
    real_density = _dev(owl.density(res))

    def every_entry(occ):
        g = ctypes.byref(occ.struct)
        return [lib.lnerf_sample_occupancy(g, _ptr(bits), _ptr(rays), n, c["S"], c["M"], 2.0, 6.0, None, 0, _ptr(t),
                                           _ptr(d), _ptr(k), None),
                lib.lnerf_occgrid_cell_points(g, None, res ** 3, None, _ptr(p), None),
                lib.lnerf_occgrid_update(g, _ptr(den), None, res ** 3, _ptr(sigma), 1, 0.5, None),
                lib.lnerf_occgrid_threshold(g, _ptr(real_density), 0.01, 0, _ptr(b), _ptr(fm), _ptr(fo), None)]

    bad_grids = [("res not a power of two", _grid(12)), ("res below the range", _grid(2)),
                 ("res above the range", _grid(512)), ("hi == lo", _grid(res, (-1, -1, -1), (1, -1, 1))),
                 ("hi < lo", _grid(res, (-1, -1, -1), (1, 1, -2))),
                 ("a NaN box", _grid(res, (-1, float("nan"), -1), (1, 1, 1)))]
    for what, occ in bad_grids:
        for rc in every_entry(occ):
            assert rc < 0 and lnerf.last_error(), what

    def smp(**kw):
        outs = kw.pop("outs", (t, d, k))
        return _raw_sample(engine, good, c, bits, rays, None, kw.pop("flags", 0), *outs, **kw)

    g = ctypes.byref(good.struct)
    calls = [("M not a multiple of 64", smp(M=100)), ("M above 1024", smp(M=1088)), ("M = 0", smp(M=0)),
             ("S = 0", smp(S=0)), ("S above 1024", smp(S=1025)), ("far == near", smp(near=2.0, far=2.0)),
             ("far < near", smp(near=6.0, far=2.0)), ("far infinite", smp(far=float("inf"))),
             ("all sampler outputs NULL", smp(outs=(None, None, None))), ("an unknown flag", smp(flags=4)),
             ("negative rays", smp(n=-1)),
             ("decay > 1", lib.lnerf_occgrid_update(g, _ptr(den), None, res ** 3, _ptr(sigma), 1, 1.5, None)),
             ("decay < 0", lib.lnerf_occgrid_update(g, _ptr(den), None, res ** 3, _ptr(sigma), 1, -0.5, None)),
             ("decay NaN", lib.lnerf_occgrid_update(g, _ptr(den), None, res ** 3, _ptr(sigma), 1, float("nan"), None)),
             ("stride 0", lib.lnerf_occgrid_update(g, _ptr(den), None, res ** 3, _ptr(sigma), 0, 0.5, None)),
             ("n != res^3 without cells", lib.lnerf_occgrid_update(g, _ptr(den), None, 7, _ptr(sigma), 1, 0.5, None)),
             ("points n != res^3 without cells", lib.lnerf_occgrid_cell_points(g, None, 7, None, _ptr(p), None)),
             ("all threshold outputs NULL", lib.lnerf_occgrid_threshold(g, _ptr(real_density), 0.01, 0, None, None, None,
                                                                       None)),
             ("a sampler flag on the threshold", lib.lnerf_occgrid_threshold(g, _ptr(real_density), 0.01, 2, _ptr(b),
                                                                            _ptr(fm), _ptr(fo), None))]
    for what, rc in calls:
        assert rc < 0, what
    assert lnerf.last_error()
    for name, full in (("sample_t", ft), ("dists", fd), ("n_occ", fk), ("points", fp), ("density", fden), ("bits", fb),
                       ("mean", fm), ("occupied", fo)):
        _untouched(full, name)
    # n = 0 succeeds and writes nothing (update: no decay either)
    assert smp(n=0) == 0 and lib.lnerf_occgrid_cell_points(g, _ptr(k), 0, None, _ptr(p), None) == 0
    assert lib.lnerf_occgrid_update(g, _ptr(den), _ptr(k), 0, _ptr(sigma), 1, 0.5, None) == 0
    for name, full in (("sample_t", ft), ("dists", fd), ("n_occ", fk), ("points", fp), ("density", fden)):
        _untouched(full, name)
    # and the same buffers take a valid call afterwards
    assert smp() == 0, lnerf.last_error()
    assert (_intact(ft, n * 1100, "sample_t")[:n * c["S"]] != SENT).all()
    with pytest.raises(RuntimeError):
        engine.sample_occupancy(good, bits, rays, c["S"], steps=100)
    with pytest.raises(RuntimeError):
        engine.occgrid_update(good, _dev(owl.density(res)), sigma, decay=1.5)


# ---- 6. end to end ------------------------------------------------------------------------------------

def test_sample_render_refresh(engine):
    """24 rays, S = 16, res = 8, the 30-wide MLP of tests/width_workloads.py: sample_occupancy ->
    ray_points -> render_maps on POINTS with the sampler's dists and sample_t, held to
    tests/render_maps_ref.py's bars; scene.render_occupancy_image is the same calls; then
    scene.occgrid_refresh with a sigma_fn on render_maps' rgba, its density and bits bit-equal to the
    checker fed the GPU's own sigma."""
    import lnerf
    import render_maps_ref as rref
    import scene
    import width_workloads as ww
    w, rays32 = ww.freq_workload(10)
    N, S, res, M = w.N, 16, 8, 128
    assert N == 24
    mlp = lnerf.make_mlp([x.shape for x in w.ws], w.wp.shape[1], w.wp.shape[2])
    ws, bs, rays = _dev(w.wp), _dev(w.bp), _dev(rays32)
    lo, hi = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
    occ = _grid(res, lo, hi)
    bits_np = owl.bitfield(res, "sphere")
    bits = _dev(bits_np)
    u = owl.planted_u(np.random.RandomState(4), N, S)
    t, dists, n_occ = engine.sample_occupancy(occ, bits, rays, S, steps=M, u=_dev(u), last_opaque=True)
    want_t, want_d, want_k = oref.sample(res, lo, hi, bits_np, rays32, S, M, 2.0, 6.0, u, oref.OCC_LAST_OPAQUE)
    t_np, d_np, k_np = _np(t), _np(dists), _np(n_occ)
    assert np.array_equal(_bits(t_np), _bits(want_t)) and np.array_equal(_bits(d_np), _bits(want_d))
    assert np.array_equal(k_np, want_k) and (k_np > 0).any() and (k_np < M).all()
    points, _ = engine.ray_points(rays, t)
    names = ("color", "depth", "opacity", "weights", "rgba")
    maps = engine.render_maps(mlp, ws, bs, points, dists, None, samples=S, input_mode=lnerf.INPUT_POINTS,
                              num_freqs=w.F, sample_t=t, want=names)
    out = {k: _np(getattr(maps, k)) for k in names}
    ratios = {k: float(v.max()) for k, v in rref.map_ratios(out, d_np, t_np, S).items()}
    print("occupancy render: worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert np.isfinite(out["color"]).all() and (out["rgba"][:, 3] > 0).any()
    # the scene helper is the same calls (rays given, so no camera is needed)
    m2, k2 = scene.render_occupancy_image(engine, mlp, ws, bs, occ, bits, 0, None, None, S, w.F, steps=M, rays=rays,
                                          u=_dev(u), last_opaque=True)
    assert np.array_equal(_np(k2), k_np) and m2.weights is None
    for k in ("color", "depth", "opacity"):
        assert np.array_equal(_bits(_np(getattr(m2, k))), _bits(out[k])), k

    # refresh: sigma at jittered points of every cell, from render_maps' rgba
    seen = {}

    def sigma_fn(p):
        rgba = engine.render_maps(mlp, ws, bs, p, _dev(np.ones((p.shape[0], 1), np.float32)), None, samples=1,
                                  input_mode=lnerf.INPUT_POINTS, num_freqs=w.F, want=("rgba",)).rgba
        seen["points"], seen["sigma"] = _np(p), _np(rgba)[:, 3].copy()
        return rgba[:, 3]

    uc = owl.planted_u(np.random.RandomState(5), res ** 3, 3)
    d0 = owl.density(res)
    density, new_bits = _dev(d0), occ.new_bits()
    mean, occupied = scene.occgrid_refresh(engine, occ, density, new_bits, sigma_fn, u=_dev(uc), decay=0.95,
                                           threshold=0.01)
    assert np.array_equal(_bits(seen["points"]), _bits(oref.cell_points(res, lo, hi, None, uc)))
    want_density = oref.update(res, d0, None, seen["sigma"], 0.95)
    assert (seen["sigma"] > 0).any()
    assert np.array_equal(_bits(_np(density)), _bits(want_density))
    assert oref.mean_margin(res, want_density) > 1     # a condition on this input, as in test_occgrid_ref.py
    want_bits, want_mean, want_occ = oref.threshold(res, want_density, 0.01, oref.OCC_MEAN)
    assert np.array_equal(_np(new_bits).view(np.uint32), want_bits) and int(_np(occupied)) == want_occ
    assert abs(float(_np(mean)) - want_mean) <= res ** 3 * 2.0 ** -52 * want_mean
    # a subset of the cells, repeats and an outside index among them
    cells, ul = owl.cell_list(res)
    scene.occgrid_refresh(engine, occ, density, new_bits, sigma_fn, cells=_dev(cells), u=_dev(ul), decay=1.0,
                          threshold=0.5, use_mean=False)
    want2 = oref.update(res, want_density, cells, seen["sigma"], 1.0)
    assert np.array_equal(_bits(_np(density)), _bits(want2))
    assert np.array_equal(_np(new_bits).view(np.uint32), oref.threshold(res, want2, 0.5)[0])
