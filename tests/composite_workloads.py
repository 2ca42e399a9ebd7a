"""Workloads that sweep the along-ray axis of the compositing (lnerf_composite.h): every sample
count and a set of opacity profiles, on the edge fixtures' identity MLP (tests/golden/make_golden.py:
8 -> 8 -> 8 -> 4, W0 = W1 = I, W2[c][c] = 1, W2[c + 4][c] = -1, zero biases), so that each sample's
head pre-activation is z_c = relu(x_c) - relu(x_{c+4}) and is set directly by its ENCODED input row.

The three scans -- composite_tile_wave (training and the k16 render maps, 128- or 64-sample tiles),
composite_fwd_wave<256> (kr) and the sequential generic kernels -- carry partial products and sums
across the 64-lane waves a ray straddles; which waves those are depends on S and on the ray's place
in the tile, and what the carry holds on how the opacity is spread along the ray. workload(S) gives
N(S) = 2 (256 // S) + 1 rays (two kr tiles' worth and a ragged last workgroup on every path; 3 rays
for S > 256), ray i with profile PROFILES[(i + S) % len(PROFILES)], so every profile visits every
in-tile position as S sweeps.

Profiles are stated in optical depth tau_j = sigma_j delta_j, so they mean the same at every S; the
dists are non-uniform (delta = 2^U(-2, 0) per sample, the reference's trailing 1e8 on the last one:
an off-by-one in dists[gs] shows on every sample), sample_t is their cumulative sum from 2.0. The
last sample (delta = 1e8) has sigma = 0 where its profile is empty there and U(0.5, 2) otherwise.

Exactness: sigma, delta (but the 1e8), every rgb pre-activation and the targets are
bf16-representable float32, |rgb| in [2^-6, 2], sigma in [2^-5, 160]: a row's largest and smallest
nonzero elements are at most 2^14 apart, so bf16, fp16x3, bf16x6 and fp32 products with the identity
weights all reproduce x bit for bit and nothing in a compositing comparison depends on the MLP's
precision. tests/test_composite_workloads.py holds the conditions these inputs must meet before the
GPU tests of tests/test_gpu_composite.py mean anything.

semantic(S) restates the edge fixtures' kinds (make_golden.py: tiny, denormal, opaque, saturated,
sigma_tiny, nan, sigma0) in tau at any S on the same dists; fp32's expf and 1 - alpha rounding
decide their results, so their reference is the loma-order fp32 C oracle.

The workloads use numpy alone; the references at the end import oracle/ when they are called.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

PROFILES = ("mixed", "thin", "empty", "gaps", "front_wall", "mid_wall", "wall63", "wall64", "back_wall",
            "two_walls", "only_one", "last_only")
WALL_TAU = 40.0
SWEEP = tuple(range(1, 129)) + (129, 200, 257)      # the fused paths take S <= 128 (K16_W4 S <= 64)
SEMANTIC_S = (2, 3, 8, 30, 43, 63, 64, 65, 100, 127, 128)
SEMANTIC_FINITE = ("tiny", "denormal", "opaque", "saturated", "sigma_tiny", "sigma0")
SEMANTIC_NAN = ("sigma0", "nan", "saturated")
RGB_COLS = (0, 1, 2, 4, 5, 6)
SIGMA_COLS = (3, 7)


def bf16(a):
    """float32 values rounded to the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def identity_mlp():
    """(ws, bs) of the edge fixtures' 8 -> 8 -> 8 -> 4 identity MLP."""
    I = np.eye(8, dtype=np.float32)
    W2 = np.zeros((8, 4), np.float32)
    for c in range(4):
        W2[c, c], W2[c + 4, c] = 1.0, -1.0
    return [I, I.copy(), W2], [np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(4, np.float32)]


def pad_weights(ws, bs):
    L, k, n = len(ws), max(w.shape[0] for w in ws), max(w.shape[1] for w in ws)
    wp, bp = np.zeros((L, k, n), np.float32), np.zeros((L, n), np.float32)
    for l, (w, b) in enumerate(zip(ws, bs)):
        wp[l, :w.shape[0], :w.shape[1]] = w
        bp[l, :b.shape[0]] = b
    return wp, bp


@dataclass
class CompositeWorkload:
    X: np.ndarray          # (N * S, 8) float32 ENCODED input rows
    dists: np.ndarray      # (N, S) float32
    sample_t: np.ndarray   # (N, S) float32
    target: np.ndarray     # (N, 3) float32
    ws: list
    bs: list
    wp: np.ndarray
    bp: np.ndarray
    profiles: tuple        # per ray: its profile (workload) or kind (semantic)
    sigma: np.ndarray      # (N, S) float32: the sigma the head produces (0 on empty samples)
    walls: tuple           # per ray: the sample indices of its tau = 40 walls
    S: int
    N: int

    @property
    def shapes(self):
        return [w.shape for w in self.ws]

    def subset(self, rays):
        rays = np.asarray(rays, np.int64)
        rows = (rays[:, None] * self.S + np.arange(self.S)[None, :]).ravel()
        return CompositeWorkload(self.X[rows], self.dists[rays], self.sample_t[rays], self.target[rays], self.ws,
                                 self.bs, self.wp, self.bp, tuple(self.profiles[r] for r in rays), self.sigma[rays],
                                 tuple(self.walls[r] for r in rays), self.S, len(rays))


def num_rays(S):
    return 2 * (256 // S) + 1 if S <= 256 else 3


def wall_indices(profile, S):
    """The samples a profile puts its tau = 40 walls on (clamped into the ray)."""
    at = {"front_wall": (0,), "mid_wall": (S // 2,), "wall63": (min(63, S - 1),), "wall64": (min(64, S - 1),),
          "back_wall": (max(S - 2, 0),), "two_walls": (S // 3, (2 * S) // 3)}.get(profile, ())
    return tuple(sorted(set(at)))


def profile_tau(profile, S, rng):
    """(tau (S,), walls): the optical depth per sample, 0 on an empty sample. Every profile draws the same
    numbers from rng, so a ray's dists and colours do not depend on its profile."""
    thin = 2.0 ** rng.uniform(-5, -3)
    mixed = 2.0 ** rng.uniform(-5, 2, S)
    one = int(rng.randint(max(S - 1, 1)))          # never the last sample of a ray of two or more
    walls = wall_indices(profile, S)
    j = np.arange(S)
    if profile == "mixed":
        tau = mixed
    elif profile == "thin":
        tau = np.full(S, thin)
    elif profile == "empty":
        tau = np.zeros(S)
    elif profile == "gaps":
        tau = np.where(j % 2 == 1, mixed, 0.0)
    elif profile == "only_one":
        tau = np.where(j == one, 1.0, 0.0)
    elif profile == "last_only":
        tau = np.where(j == S - 1, 1.0, 0.0)
    elif walls:
        tau = np.full(S, thin)
        tau[list(walls)] = WALL_TAU
    else:
        raise KeyError(profile)
    return tau, walls


def _dists(rng, N, S):
    d = bf16(2.0 ** rng.uniform(-2, 0, (N, S)))
    d[:, -1] = np.float32(1e8)
    t = np.float32(2.0) + np.concatenate([np.zeros((N, 1), np.float32), np.cumsum(d[:, :-1], axis=1, dtype=np.float32)],
                                         axis=1)
    return d, t.astype(np.float32)


def _rows(rgb_pre, sigma, empty):
    """(S, 8) input rows of one ray: rgb pre-activations, sigma >= 0, empty samples through x7 = 1."""
    S = len(sigma)
    x = np.zeros((S, 8), np.float32)
    x[:, 0:3] = np.maximum(rgb_pre, 0)
    x[:, 4:7] = np.maximum(-rgb_pre, 0)
    x[:, 3] = np.where(empty, 0.0, sigma)
    x[:, 7] = np.where(empty, 1.0, 0.0)
    return x


def _pack(X, d, t, target, names, sigma, walls, S):
    ws, bs = identity_mlp()
    wp, bp = pad_weights(ws, bs)
    for a in (X, d, t, target, sigma):
        a.setflags(write=False)
    return CompositeWorkload(X, d, t, target, ws, bs, wp, bp, tuple(names), sigma, tuple(walls), S, len(names))


def _colour64(rgb_pre, sigma, d):
    """Float64 colours (N, 3) of rays given per-sample rgb pre-activations (N, S, 3), sigma and dists (N, S):
    the reference's inclusive transmittance (scripts/nerf.py:200-288), as render_maps_ref.composite64."""
    rgb = 1.0 / (1.0 + np.exp(-np.asarray(rgb_pre, np.float64)))
    alpha = 1.0 - np.exp(-np.asarray(sigma, np.float64) * np.asarray(d, np.float64))
    T = np.cumprod((1.0 - alpha) + 1e-10, axis=1)
    T[:, 0] = 1.0
    return ((alpha * T)[:, :, None] * rgb).sum(1)


def _targets(rng, colour):
    """Targets a residual of 0.25 .. 0.75 away from the float64 colour in every channel, on one side of it
    per ray, rounded to bf16. Every adjoint of a ray carries dL/dC = 2 (C - t), the opacity adjoints through
    dL/dw_j = sum_k rgb_jk dL/dC_k: a target that happens to sit next to the colour, or residuals of mixed
    sign, turn the colour's fp32 rounding into a relative error of every gradient of that ray in any fp32
    implementation (on U(0, 1) targets the C oracle was 0.63 of the d_dists bar from float64, with
    residuals of mixed sign 2.2 bars on a two-sample ray), which says nothing about the scans.
    (make_golden.py picks its band fixture's seed for the same reason.)"""
    n = colour.shape
    return bf16(colour + rng.uniform(0.25, 0.75, n) * np.where(rng.uniform(size=(n[0], 1)) < 0.5, -1.0, 1.0))


@functools.lru_cache(maxsize=None)
def workload(S, seed=None):
    rng = np.random.RandomState(1000 + S if seed is None else seed)
    N = num_rays(S)
    d, t = _dists(rng, N, S)
    names, rows, sigmas, walls, pres = [], [], [], [], []
    for i in range(N):
        name = PROFILES[(i + S) % len(PROFILES)]
        rgb_pre = bf16(2.0 ** rng.uniform(-6, 1, (S, 3)) * np.where(rng.uniform(size=(S, 3)) < 0.5, -1.0, 1.0))
        last_sigma = bf16(rng.uniform(0.5, 2))
        tau, wl = profile_tau(name, S, rng)
        empty = tau == 0
        sigma = bf16(np.where(empty, 0.0, tau / d[i].astype(np.float64)))
        if not empty[-1]:
            sigma[-1] = last_sigma
        names.append(name)
        rows.append(_rows(rgb_pre, sigma, empty))
        sigmas.append(sigma)
        walls.append(wl)
        pres.append(rgb_pre)
    sigma = np.stack(sigmas)
    target = _targets(rng, _colour64(np.stack(pres), sigma, d))
    return _pack(np.concatenate(rows), d, t, target, names, sigma, walls, S)


@functools.lru_cache(maxsize=None)
def semantic(S, nan=False, seed=None):
    """The edge fixtures' kinds at any S (make_golden.edge_ray, sigma restated as tau / delta on this file's
    dists): nan=False cycles SEMANTIC_FINITE, nan=True SEMANTIC_NAN (a NaN adjoint reaches every dW column,
    so the finite kinds' dW is only checkable without it)."""
    kinds = SEMANTIC_NAN if nan else SEMANTIC_FINITE
    rng = np.random.RandomState((3000 if nan else 2000) + S if seed is None else seed)
    N = num_rays(S)
    d, t = _dists(rng, N, S)
    j = np.arange(S)
    names, rows, sigmas, pres = [], [], [], []
    for i in range(N):
        kind = kinds[(i + S) % len(kinds)]
        rgb_pre = bf16(rng.uniform(-2, 2, (S, 3)))
        plain = rng.uniform(0.5, 2, S)
        sat = np.where(rng.uniform(size=(S, 3)) < 0.5, 30.0, -30.0)
        where = int(rng.randint(S))
        dd = d[i].astype(np.float64)
        tau = {"tiny": (j + 1) * 1e-9, "denormal": np.full(S, 13.8), "opaque": np.full(S, 50.0),
               "saturated": np.where(j % 2 == 0, 0.0, 1.7), "sigma0": np.zeros(S)}.get(kind)
        if kind == "sigma_tiny":
            sigma = np.full(S, 1e-30)
        elif kind == "nan":
            sigma = plain
        else:
            sigma = tau / dd
            if kind in ("denormal", "opaque"):
                sigma[-1] = 24.2 if kind == "denormal" else 50.0      # the fixtures' own sigma behind delta = 1e8
            if kind == "tiny":
                sigma[-1] = min(S, 8) * 1e-9                         # sigma 1e8 <= 0.8, the fixture's own
        sigma = bf16(sigma)
        empty = np.full(S, kind == "sigma0")
        if kind in ("tiny", "sigma_tiny"):        # the whole row as small as sigma
            rgb_pre = bf16(rgb_pre * np.float32(1e-30 if kind == "sigma_tiny" else 1e-9))
        if kind == "saturated":
            rgb_pre = sat.astype(np.float32)
        if kind == "nan":
            rgb_pre[where, 0] = -100.0
        names.append(kind)
        rows.append(_rows(rgb_pre, sigma, empty))
        sigmas.append(np.where(empty, np.float32(0), sigma).astype(np.float32))
        pres.append(rgb_pre)
    sigma = np.stack(sigmas)
    target = _targets(rng, _colour64(np.stack(pres), sigma, d))
    return _pack(np.concatenate(rows), d, t, target, names, sigma, [()] * N, S)


# ---- geometry: where a ray's samples sit in a tile ----------------------------------------------

def tile_position(i, S, tile):
    """(first sample's wave, last sample's wave, in-tile ray index, rays per tile) of ray i in a `tile`-sample
    tile of whole rays (lnerf_composite.h: 128 for k16, 64 for K16_W4, 256 for kr); S <= tile."""
    rpw = tile // S
    rl = i % rpw
    return (rl * S) >> 6, (rl * S + S - 1) >> 6, rl, rpw


def position_classes(S, tile, N):
    """One ray per tile-position class among rays 0 .. N - 1: the first ray of a tile, a ray straddling a
    wave boundary (None if no ray of this S does) and the last whole ray of a tile; the second tile's where
    the batch has one, so that a neighbour sits on both sides."""
    rpw = max(tile // S, 1)
    base = rpw if N >= 2 * rpw else 0
    out = {"first": base, "last": min(base + rpw - 1, N - 1), "straddle": None}
    for i in range(base, min(base + rpw, N)):
        w0, w1, _, _ = tile_position(i, S, tile) if S <= tile else (0, 1, 0, 1)
        if w1 > w0:
            out["straddle"] = i
            break
    return out


# ---- bars ---------------------------------------------------------------------------------------

def _ratio(err, bar):
    """err / bar per element; an error against a zero bar (a value that must be exact) is inf."""
    r = np.where(err > 0, err / np.where(bar > 0, bar, 1.0), 0.0)
    return np.where((err > 0) & (bar == 0), np.inf, r)


def per_ray_ratio(got, want, rtol=1e-5, gtol=1e-5):
    """(N, ...) arrays -> (N,) worst |got - want| / (rtol |want| + gtol max|want| over the ray): the form of
    test_gpu_edge.close_grouped, one bar per ray."""
    got = np.asarray(got, np.float64).reshape(len(want), -1)
    want = np.asarray(want, np.float64).reshape(len(want), -1)
    bar = rtol * np.abs(want) + gtol * np.abs(want).max(axis=1, keepdims=True)
    return _ratio(np.abs(got - want), bar).max(axis=1)


def dx_ratios(got, want, S, row_term=0.0):
    """dX (N * S, 8) -> (rgb (N,), sigma (N,)) worst error / bar per ray: the rgb columns {0, 1, 2, 4, 5, 6}
    against 1e-5 |want| + 1e-5 x the ray's max over those columns, the sigma columns {3, 7} against
    1e-5 |want| + 1e-4 x the ray's max of that column (the project's dW column form); row_term x the sample
    row's max |want| is added to both (explicit fp16x3: 2^-20, lnerf.h LNERF_MFMA_F16X3)."""
    got = np.asarray(got, np.float64).reshape(-1, S, 8)
    want = np.asarray(want, np.float64).reshape(-1, S, 8)
    err = np.abs(got - want)
    row = row_term * np.abs(want).max(axis=2, keepdims=True)
    a = np.abs(want[:, :, RGB_COLS])
    bar_rgb = 1e-5 * a + 1e-5 * a.max(axis=(1, 2), keepdims=True) + row
    a = np.abs(want[:, :, SIGMA_COLS])
    bar_sig = 1e-5 * a + 1e-4 * a.max(axis=1, keepdims=True) + row

    return (_ratio(err[:, :, RGB_COLS], bar_rgb).reshape(len(err), -1).max(axis=1),
            _ratio(err[:, :, SIGMA_COLS], bar_sig).reshape(len(err), -1).max(axis=1))


# ---- references ---------------------------------------------------------------------------------

def _padded(per_layer, shape):
    out = np.zeros(shape, np.float64)
    for l, a in enumerate(per_layer):
        a = np.asarray(a, np.float64)
        out[(l,) + tuple(slice(0, n) for n in a.shape)] = a
    return out


def reference64(w):
    """The float64 restatement (oracle/nerf_np.py) of the step on w, seed 1; the ReLU decisions are z > 0 on
    exact inputs (x > 0), every implementation's. dW / dB padded like the engine's."""
    import nerf_np
    with np.errstate(all="ignore"):
        r = nerf_np.nerf_forward_backward(w.X, w.ws, w.bs, w.dists, w.target, w.S, seed=1.0)
    return dict(loss=float(r["loss"]), acc=r["acc"], d_target=r["d_target"], d_dists=r["d_dists"], dX=r["dX"],
                dW=_padded(r["dW"], w.wp.shape), dB=_padded(r["db"], w.bp.shape), weights=r["weights"],
                opacity=r["weights"].sum(1), depth=(r["weights"] * w.sample_t.astype(np.float64)).sum(1))


def reference_c(w):
    """The loma-order fp32 C oracle (oracle/nerf_oracle.c) on w, seed 1."""
    import oracle
    c = oracle.standard_forward_backward(w.X, w.wp, w.bp, w.shapes, w.dists, w.target, w.S, seed=1.0, dX=True)
    return dict(loss=float(c["loss"]), acc=c["acc"], d_target=c["d_target"], d_dists=c["d_dists"], dX=c["dX"],
                dW=c["dW"], dB=c["dB"])


@functools.lru_cache(maxsize=None)
def references(S):
    """(reference64, reference_c) of workload(S), computed once."""
    return reference64(workload(S)), reference_c(workload(S))


@functools.lru_cache(maxsize=None)
def semantic_reference(S, nan):
    with np.errstate(all="ignore"):
        return reference_c(semantic(S, nan))


def composite_fp32(w, pairwise):
    """The step on w in float32 numpy with loma's per-sample expressions (lnerf_composite.h /
    oracle/nerf_oracle.c) and the along-ray product, sums and suffix recurrence either one after the other
    (the C oracle's order) or pairwise (Hillis-Steele doubling: the association of a scan). The head
    pre-activations are exact (z = x_c - x_{c+4}) and G_0 = dX, so dW and dB are float64 sums of float32
    rows. For test C's rule: how far re-association alone moves an fp32 result. Returns loss (a float32 sum
    of the rays' float32 losses, in the same association), acc, d_target, d_dists, dX, dW, dB."""
    f = np.float32
    N, S = w.N, w.S
    z = (w.X[:, :4] - w.X[:, 4:]).reshape(N, S, 4)
    d = w.dists
    with np.errstate(all="ignore"):
        rgb = f(1) / (f(1) + np.exp(f(0) - z[:, :, :3]))
        sigma = np.where(z[:, :, 3] > 0, z[:, :, 3], f(0))
        e = np.exp((f(0) - sigma) * d)
        al = f(1) - e
        cc = (f(1) - al) + f(1e-10)

        def scan(v, op):
            v = v.copy()
            if pairwise:
                k = 1
                while k < S:
                    v[:, k:] = op(v[:, :-k], v[:, k:])
                    k *= 2
            else:
                for j in range(1, S):
                    v[:, j] = op(v[:, j - 1], v[:, j])
            return v

        P = scan(cc, np.multiply)
        T = P.copy()
        T[:, 0] = 1
        wgt = al * T
        C = scan(wgt[:, :, None] * rgb, np.add)[:, -1]
        t = w.target
        per_ray = ((C - t) * (C - t))
        per_ray = (per_ray[:, 0] + per_ray[:, 1]) + per_ray[:, 2]
        loss = _tree_sum(per_ray) if pairwise else np.cumsum(per_ray, dtype=f)[-1]
        dacc = (C - t) * f(1.0)
        dacc = dacc + dacc
        dw = (rgb[:, :, 2] * dacc[:, None, 2] + rgb[:, :, 1] * dacc[:, None, 1]) + rgb[:, :, 0] * dacc[:, None, 0]
        drgb = wgt[:, :, None] * dacc[:, None, :]
        ga = al * dw
        ga[:, 0] = 0
        gb = np.concatenate([cc[:, 1:], np.zeros((N, 1), f)], axis=1)
        if pairwise:
            k = 1
            while k < S:
                ga[:, :-k], gb[:, :-k] = ga[:, :-k] + gb[:, :-k] * ga[:, k:], gb[:, :-k] * gb[:, k:]
                k *= 2
        else:
            for j in range(S - 2, -1, -1):
                ga[:, j] = ga[:, j] + gb[:, j] * ga[:, j + 1]
        dc = ga.copy()
        dc[:, 1:] = P[:, :-1] * ga[:, 1:]
        dal = T * dw + (f(0) - dc)
        adj2 = (f(0) - dal) * e
        gz = np.zeros((N, S, 4), f)
        gz[:, :, 3] = np.where(sigma > 0, f(0) - d * adj2, f(0))
        u = f(1) + np.exp(f(0) - z[:, :, :3])
        gz[:, :, :3] = f(0) - ((f(0) - drgb) / (u * u)) * np.exp(f(0) - z[:, :, :3])
        d_dists = (f(0) - sigma) * adj2
    x = w.X.reshape(N, S, 8)
    dX = np.concatenate([np.where(x[:, :, :4] > 0, gz, f(0)), np.where(x[:, :, 4:] > 0, f(0) - gz, f(0))], axis=2)
    G = [dX.reshape(-1, 8), dX.reshape(-1, 8), gz.reshape(-1, 4)]
    A = [w.X, np.maximum(w.X, 0), np.maximum(w.X, 0)]
    with np.errstate(all="ignore"):
        dW = _padded([a.astype(np.float64).T @ g.astype(np.float64) for a, g in zip(A, G)], w.wp.shape)
        dB = _padded([g.astype(np.float64).sum(0) for g in G], w.bp.shape)
    return dict(loss=float(loss), acc=C, d_target=f(0) - dacc, d_dists=d_dists, dX=dX.reshape(-1, 8), dW=dW, dB=dB)


@functools.lru_cache(maxsize=None)
def semantic_decidable(S):
    """For the finite semantic batch at S: (columns (L, n) bool, loss bar). Test C's rule for an output that
    fp32 itself does not pin down: the step is evaluated twice more in float32 on the CPU (composite_fp32,
    one sample after the other and pairwise) and compared with the C oracle.
      dW: a column made only of rows behind an underflowing transmittance is decided by single ulps of expf
          -- numpy's exp and the C library's, in the SAME order, put such columns up to 1.5e4 bars apart
          (S = 128) -- so a column is held to the oracle only where both CPU evaluations are within half of
          close_grouped's bar of it;
      loss: within max(1e-6, 4 x the farther CPU evaluation's distance) of the oracle's, relative."""
    w, c = semantic(S, False), semantic_reference(S, False)
    cols = np.ones(w.wp.shape[::2], bool)
    dist = 0.0
    for pairwise in (False, True):
        e = composite_fp32(w, pairwise)
        want = np.asarray(c["dW"], np.float64)
        bar = 1e-5 * np.abs(want) + 1e-5 * np.abs(want).max(axis=1, keepdims=True)
        cols &= (_ratio(np.abs(e["dW"] - want), bar).max(axis=1) <= 0.5)
        dist = max(dist, abs(e["loss"] - c["loss"]) / abs(c["loss"]))
    return cols, max(1e-6, 4.0 * dist)


@functools.lru_cache(maxsize=None)
def semantic_nan_loss_bar(S):
    """The loss bar of the nan batch (its forward is finite): as semantic_decidable's."""
    w, c = semantic(S, True), semantic_reference(S, True)
    return max(1e-6, 4.0 * max(abs(composite_fp32(w, p)["loss"] - c["loss"]) / abs(c["loss"]) for p in (False, True)))


def _tree_sum(v):
    v = np.asarray(v, np.float32)
    while len(v) > 1:
        if len(v) % 2:
            v = np.concatenate([v, np.zeros(1, np.float32)])
        v = v[0::2] + v[1::2]
    return v[0]


def replace_rays(w, rays, kind):
    """w with the input rows of `rays` replaced by a ray of `kind` (the neighbours of test D): `opaque`
    (tau = 50 on every sample), `empty` (sigma = 0 through x7 = 1) or `nan` (z_r = -100 and a NaN delta on
    sample S // 2: the sigmoid's adjoint and the compositing itself both meet a NaN). The targets, the other
    rays and the other dists stay what they were."""
    X = w.X.reshape(w.N, w.S, 8).copy()
    d = w.dists.copy()
    for i in rays:
        if kind == "opaque":
            sig = bf16(50.0 / d[i].astype(np.float64))
            sig[-1] = 50.0
            X[i, :, 3], X[i, :, 7] = sig, 0.0
        elif kind == "empty":
            X[i, :, 3], X[i, :, 7] = 0.0, 1.0
        elif kind == "nan":
            X[i, w.S // 2, 0], X[i, w.S // 2, 4] = 0.0, 100.0
            d[i, w.S // 2] = np.nan
        else:
            raise KeyError(kind)
    sigma = np.maximum(X[:, :, 3], 0).astype(np.float32)
    names = tuple(kind if i in set(rays) else p for i, p in enumerate(w.profiles))
    return CompositeWorkload(X.reshape(-1, 8), d, w.sample_t, w.target, w.ws, w.bs, w.wp, w.bp, names, sigma,
                             w.walls, w.S, w.N)


# (profile, output) pairs held to the C oracle instead of float64. Only ("front_wall", "d_dists") may ever be
# listed (a wall thin enough that fp32 rounds 1 - alpha to 0 and float64 does not puts everything behind it
# at fp32's mercy); at tau = 40 both agree that it is 0, the C oracle is 0.14 of the bar from float64 on those
# rays, and nothing is excluded.
C_ORACLE_ONLY = ()


def step_ratios(got, w, ref, row_term=0.0):
    """Per ray, the worst error / bar of each per-ray output of a training step against `ref`
    (reference64 / reference_c): {acc, d_target, d_dists, dX_rgb, dX_sigma} -> (N,)."""
    out = {k: per_ray_ratio(got[k], ref[k]) for k in ("acc", "d_target", "d_dists")}
    if got.get("dX") is not None:
        out["dX_rgb"], out["dX_sigma"] = dx_ratios(got["dX"], ref["dX"], w.S, row_term)
    return out
