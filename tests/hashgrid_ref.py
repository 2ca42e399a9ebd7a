"""Float64 numpy restatement of the multiresolution hash-grid entry points of include/lnerf.h
(lnerf_hashgrid_encode, lnerf_hashgrid_grad), written from the header's text and independent of the
library and of lnerf.py. Test infrastructure: tests/test_hashgrid_ref.py checks it against central
differences on the CPU, tests/test_gpu_hashgrid.py checks the kernels against it.

The forward keeps the header's operation order (so the kernels can match it bit for bit); d_table is
an order-free float64 sum that also returns, per entry, sum |term| and the number of terms n, which
is what the float32-atomic bar of the header is stated in; d_points keeps the header's order and
returns sum |term| for the float64 order term of its bar.
"""
from __future__ import annotations

import numpy as np

P1, P2 = 2654435761, 805459861


class Grid:
    """The fields of an lnerf_hashgrid, filled by hand: level l holds res^3 entries if that is at
    most T = 2^log2_table (dense), else T (hashed), rounded up to a multiple of 4."""

    def __init__(self, res, features, log2_table, lo, hi):
        self.res = [int(r) for r in res]
        self.levels = len(self.res)
        self.features = int(features)
        self.log2_table = int(log2_table)
        self.T = 1 << self.log2_table
        self.lo = np.asarray(lo, np.float32)
        self.hi = np.asarray(hi, np.float32)
        self.dense = [r ** 3 <= self.T for r in self.res]
        self.entries = [r ** 3 if d else self.T for r, d in zip(self.res, self.dense)]
        self.offset = [0]
        for e in self.entries:
            self.offset.append(self.offset[-1] + (e + 3) // 4 * 4)
        self.total = self.offset[-1]
        self.width = self.levels * self.features


def init_res(levels, base_res, max_res):
    """lnerf_hashgrid_init's resolutions: floor(base b^l + 0.5), b = exp(ln(max / base) / (levels - 1))."""
    b = np.exp(np.log(max_res / base_res) / (levels - 1)) if levels > 1 else 1.0
    return [int(np.floor(base_res * b ** l + 0.5)) for l in range(levels)]


def cells(grid, points, l):
    """Per row and axis at level l: cell i (int64), weight w (float64) and whether the coordinate is
    inside the box (the clamp left it alone; a NaN is not)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    lo = grid.lo.astype(np.float64)
    ext = grid.hi.astype(np.float64) - lo
    with np.errstate(invalid="ignore"):
        u_raw = (p - lo) / ext
        live = (u_raw >= 0.0) & (u_raw <= 1.0)
        u = np.where(u_raw > 0.0, np.where(u_raw < 1.0, u_raw, 1.0), 0.0)
    res = grid.res[l]
    pos = u * float(res - 1)
    i = np.minimum(np.floor(pos).astype(np.int64), res - 2)
    return i, pos - i, live


def corner_cells(grid, i, l):
    """(R, 8) linear ids res-independent of hashing: g_x + res (g_y + res g_z) of each corner."""
    res = grid.res[l]
    k = np.arange(8)
    gx = i[:, 0:1] + (k & 1)
    gy = i[:, 1:2] + ((k >> 1) & 1)
    gz = i[:, 2:3] + ((k >> 2) & 1)
    return gx, gy, gz, gx + res * (gy + res * gz)


def corner_entries(grid, i, l):
    """(R, 8) level-local entry index of each corner (dense or hashed in uint32)."""
    gx, gy, gz, lin = corner_cells(grid, i, l)
    if grid.dense[l]:
        return lin
    h = (gx.astype(np.uint64) ^ ((gy.astype(np.uint64) * P1) & 0xFFFFFFFF) ^ ((gz.astype(np.uint64) * P2) & 0xFFFFFFFF))
    return (h & np.uint64(grid.T - 1)).astype(np.int64)


def corner_weights(w):
    """(R, 8): (fx fy) fz with f_c = w_c where bit c of k is set, else 1 - w_c."""
    k = np.arange(8)
    fx = np.where(k & 1, w[:, 0:1], 1.0 - w[:, 0:1])
    fy = np.where(k & 2, w[:, 1:2], 1.0 - w[:, 1:2])
    fz = np.where(k & 4, w[:, 2:3], 1.0 - w[:, 2:3])
    return fx * fy * fz, (fx, fy, fz)


def encode(grid, table, points):
    """(enc (R, width) float64 before the one rounding, sum |term| of the same shape)."""
    table = np.asarray(table, np.float32).astype(np.float64).reshape(grid.total, grid.features)
    R, F = len(points), grid.features
    enc = np.zeros((R, grid.width))
    mag = np.zeros((R, grid.width))
    for l in range(grid.levels):
        i, w, _ = cells(grid, points, l)
        idx = corner_entries(grid, i, l) + grid.offset[l]
        wk, _ = corner_weights(w)
        acc = np.zeros((R, F))
        m = np.zeros((R, F))
        for k in range(8):
            term = wk[:, k:k + 1] * table[idx[:, k]]
            acc = acc + term
            m = m + np.abs(term)
        enc[:, l * F:(l + 1) * F] = acc
        mag[:, l * F:(l + 1) * F] = m
    return enc, mag


def grad_table(grid, points, d_encoded, scale=1.0):
    """(want (total, F) float64, sum |term| (total, F), n (total,) terms per entry)."""
    dE = np.asarray(d_encoded, np.float32).astype(np.float64)
    F = grid.features
    want = np.zeros((grid.total, F))
    mag = np.zeros((grid.total, F))
    n = np.zeros(grid.total, np.int64)
    for l in range(grid.levels):
        i, w, _ = cells(grid, points, l)
        idx = corner_entries(grid, i, l) + grid.offset[l]
        wk, _ = corner_weights(w)
        for k in range(8):
            term = float(scale) * wk[:, k:k + 1] * dE[:, l * F:(l + 1) * F]
            np.add.at(want, idx[:, k], term)
            np.add.at(mag, idx[:, k], np.abs(term))
            np.add.at(n, idx[:, k], 1)
    return want, mag, n


def row_entries(grid, points, row):
    """The set of global entries row `row` touches (at most 8 per level)."""
    out = set()
    for l in range(grid.levels):
        i, _, _ = cells(grid, points[row:row + 1], l)
        out |= set((corner_entries(grid, i, l)[0] + grid.offset[l]).tolist())
    return out


def grad_points(grid, table, points, d_encoded, scale=1.0):
    """(d_points (R, 3) float64 before the one rounding -- 0 where the coordinate is outside the box
    or NaN --, sum |term| (R, 3), live (R, 3))."""
    table = np.asarray(table, np.float32).astype(np.float64).reshape(grid.total, grid.features)
    dE = np.asarray(d_encoded, np.float32).astype(np.float64)
    R, F = len(points), grid.features
    ext = grid.hi.astype(np.float64) - grid.lo.astype(np.float64)
    acc = np.zeros((R, 3))
    mag = np.zeros((R, 3))
    live = np.ones((R, 3), bool)
    for l in range(grid.levels):
        i, w, live = cells(grid, points, l)
        idx = corner_entries(grid, i, l) + grid.offset[l]
        _, (fx, fy, fz) = corner_weights(w)
        k = np.arange(8)
        g = [np.where(k & 1, fy * fz, -(fy * fz)), np.where(k & 2, fx * fz, -(fx * fz)),
             np.where(k & 4, fx * fy, -(fx * fy))]
        de = dE[:, l * F:(l + 1) * F]
        for a in range(3):
            dw = np.zeros((R, F))
            dm = np.zeros((R, F))
            for kk in range(8):
                term = g[a][:, kk:kk + 1] * table[idx[:, kk]]
                dw = dw + term
                dm = dm + np.abs(term)
            s = np.zeros(R)
            sm = np.zeros(R)
            for f in range(F):
                s = s + de[:, f] * dw[:, f]
                sm = sm + np.abs(de[:, f]) * dm[:, f]
            acc[:, a] = acc[:, a] + s * float(grid.res[l] - 1) / ext[a]
            mag[:, a] = mag[:, a] + sm * float(grid.res[l] - 1) / ext[a]
    out = np.where(live, float(scale) * acc, 0.0)
    return out, abs(float(scale)) * mag, live


# ---- the bars of include/lnerf.h ----------------------------------------------------------------
def forward_bar(enc, mag):
    """2^-23 |ref| + 8 2^-52 sum |term|: one rounding to float32 and eight float64 products and sums."""
    return 2.0 ** -23 * np.abs(enc) + 8 * 2.0 ** -52 * mag


def points_bar(grid, dp, mag):
    """One rounding to float32 (2^-24 |ref|, or half the smallest subnormal) plus the float64 order
    term: at most levels (9 F + 3) + 1 float64 operations per value, each within 2^-53 of sum |term|
    (2^-52 allowed)."""
    ops = grid.levels * (9 * grid.features + 3) + 1
    return 2.0 ** -24 * np.abs(dp) + 2.0 ** -149 + ops * 2.0 ** -52 * mag


def table_bar(want, mag, n):
    """2^-23 |want| + (n + 2) 2^-24 sum |term|: n float32 terms added in any order."""
    return 2.0 ** -23 * np.abs(want) + (n[:, None] + 2) * 2.0 ** -24 * mag
