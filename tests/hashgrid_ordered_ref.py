"""Numpy restatement of d_table under LNERF_HASHGRID_REPRODUCIBLE (include/lnerf.h, lnerf_hashgrid_grad),
written from the header's text: the value every entry must hold BIT FOR BIT. Test infrastructure:
tests/test_hashgrid_ordered_ref.py qualifies it on the CPU against the order-free float64 sums of
tests/hashgrid_ref.py, tests/test_gpu_hashgrid_ordered.py compares the kernels with it.

The contract, per level l, entry e and feature f:
  * a term is t(r, k, f) = (float64(scale) weight_k(r)) float64(d_encoded[r][l F + f]), two float64
    products in that order, weight_k = (fx fy) fz in float64, never rounded to float32;
  * the entry's terms in ascending contribution id c = 8 r + k, t_0 .. t_{n-1}, are summed as
        partial_q = ((+0 + t_{8q}) + t_{8q+1}) + ...      runs of RUN = 8 consecutive positions
        sum       = ((+0 + partial_0) + partial_1) + ...  the partials in ascending order
    (n <= 8: the plain sequential sum);
  * d_table[e][f] = float32(sum), or held + float32(sum) in float32 under LNERF_ACCUMULATE; an entry
    without terms is +0, or keeps its bits under LNERF_ACCUMULATE.
np.add.at adds unbuffered, one index after the other in the order given, which is what makes both
stages sequential here.
"""
from __future__ import annotations

import functools

import numpy as np

import hashgrid_ref as hr
import hashgrid_workloads as hw
from hashgrid_ref import cells, corner_entries, corner_weights

RUN = 8


def level_terms(grid, points, d_encoded, scale, l):
    """(idx (8 R,) global entry of every contribution in ascending c = 8 r + k, term (8 R, F) float64)."""
    dE = np.asarray(d_encoded, np.float32).astype(np.float64)
    F = grid.features
    sc = np.float64(1.0) if scale is None else np.float64(np.float32(scale))
    i, w, _ = cells(grid, points, l)
    idx = corner_entries(grid, i, l) + grid.offset[l]
    wk, _ = corner_weights(w)
    with np.errstate(invalid="ignore", over="ignore"):
        term = (sc * wk)[:, :, None] * dE[:, None, l * F:(l + 1) * F]
    return idx.reshape(-1), term.reshape(-1, F)


def grad_table_ordered(grid, points, d_encoded, scale=None):
    """(sum (total, F) float64 in the shipped order, before the one rounding; n (total,) terms per entry)."""
    F = grid.features
    acc = np.zeros((grid.total, F))
    n = np.zeros(grid.total, np.int64)
    for l in range(grid.levels):
        idx, term = level_terms(grid, points, d_encoded, scale, l)
        order = np.argsort(idx, kind="stable")            # each entry's contributions, ascending c
        si, st = idx[order], term[order]
        at = np.arange(len(si))
        head = np.ones(len(si), bool)
        head[1:] = si[1:] != si[:-1]
        pos = at - np.maximum.accumulate(np.where(head, at, 0))   # position in the entry's list
        run_head = pos % RUN == 0
        run_id = np.cumsum(run_head) - 1
        partial = np.zeros((int(run_id[-1]) + 1, F))
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(partial, run_id, st)                        # +0, then the run's terms in order
            np.add.at(acc, si[run_head], partial)                 # +0, then the partials in order
        np.add.at(n, idx, 1)
    return acc, n


def stored(acc, n, held=None):
    """What d_table holds after the call: float32(sum), or held + float32(sum) where the entry has terms."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = acc.astype(np.float32)
    touched = (n > 0)[:, None]
    if held is None:
        return np.where(touched, s, np.float32(0.0)).astype(np.float32)
    held = np.asarray(held, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(touched, held + s, held).astype(np.float32)


def ordered_bar(want, mag, n):
    """2^-24 |want| + 2^-149 + (n + 1) 2^-52 sum |term|: one rounding to float32 (half an ulp, or half
    the smallest subnormal) and, per term, one float64 product pair and one float64 add, each within
    2^-53 of sum |term| (2^-52 allowed, as in hashgrid_ref.points_bar)."""
    return 2.0 ** -24 * np.abs(want) + 2.0 ** -149 + (n[:, None] + 1) * 2.0 ** -52 * mag


# ---- the case of this mode's own: one long segment per touched entry -------------------------------
PILE = (768, 2, tuple(hw.RES_5), 12, "pile")   # (a fifth field: the first four equal a hashgrid_workloads case)


@functools.lru_cache(maxsize=None)
def pile():
    """768 rows, all at ONE point outside the box (below lo on x, inside on y and z): eight entries per
    level receive 768 terms each -- segments that span every block of the sort and take the kernel's
    whole-wave path -- four of them with non-zero weights. Same keys as hashgrid_workloads.build."""
    R, F, res, lt, _ = PILE
    grid = hr.Grid(list(res), F, lt, hw.LO, hw.HI)
    lo32, hi32 = np.asarray(hw.LO, np.float32), np.asarray(hw.HI, np.float32)
    p = lo32 + (hi32 - lo32) * np.asarray([0.3, 0.61, 0.47], np.float32)   # off every grid plane
    p[0] = lo32[0] - np.float32(0.5)
    pts = np.tile(p, (R, 1)).astype(np.float32)
    rs = np.random.RandomState(768212)
    table = rs.normal(size=(grid.total, F)).astype(np.float32)
    d_enc = rs.normal(size=(R, grid.width)).astype(np.float32)
    scale = np.float32(0.37)
    want, mag, n = hr.grad_table(grid, pts, d_enc, scale)
    for a in (pts, table, d_enc, want, mag, n):
        a.setflags(write=False)
    return dict(case=PILE, grid=grid, points=pts, table=table, d_encoded=d_enc, scale=scale, d_table=want,
                d_table_mag=mag, d_table_n=n)


def workload(case):
    """hashgrid_workloads.build, or the pile."""
    return pile() if case == PILE else hw.build(case)


def case_id(case):
    return "pile-" + hw.case_id(case[:4]) if case == PILE else hw.case_id(case)


@functools.lru_cache(maxsize=None)
def expected(case, scaled=True):
    """(sum (total, F) float64, n) of the case in the shipped order, computed once (read-only)."""
    w = workload(case)
    acc, n = grad_table_ordered(w["grid"], w["points"], w["d_encoded"], w["scale"] if scaled else None)
    acc.setflags(write=False)
    n.setflags(write=False)
    return acc, n
