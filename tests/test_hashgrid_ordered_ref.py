"""CPU qualification of tests/hashgrid_ordered_ref.py, the bit-level checker of d_table under
LNERF_HASHGRID_REPRODUCIBLE, on every case tests/test_gpu_hashgrid_ordered.py runs (the 15 of
hashgrid_workloads.ALL, the end-to-end grid and the pile):

  * against the exact sums: the checker's result rounded to float32 is within
    2^-24 |want| + 2^-149 + (n + 1) 2^-52 sum |term| of hashgrid_ref.grad_table's order-free float64
    `want` -- one float32 rounding, n float64 products and adds;
  * not vacuous: from R = 63 up, float32 sequential sums of the same terms in ascending and in
    descending order differ in bits on at least 8 entries, and the float32 ascending sum differs from
    the checker on at least 8, so that bit-equality with the checker is something a float32 sum in
    arrival order cannot pass;
  * the order is the header's: runs of eight, checked against a plain Python loop on one case.

Measured (the tests print them): worst error / bar 0.775-0.997 over the 17 cases (the half-ulp of the
one rounding); over the 15 cases from R = 63 up, 8-1856 entries differ between the two float32 orders
and 8-2093 between the float32 ascending sum and the checker; 8-2488 touched entries, up to 1253 terms
on one.
"""
import numpy as np
import pytest

import hashgrid_ordered_ref as orf
import hashgrid_workloads as hw

CASES = hw.ALL + [hw.hashable(hw.E2E), orf.PILE]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=orf.case_id)
def test_checker_is_within_the_bar_of_the_exact_sums(case):
    w = orf.workload(case)
    acc, n = orf.expected(case)
    want, mag, cnt = w["d_table"], w["d_table_mag"], w["d_table_n"]
    assert (n == cnt).all()
    got = orf.stored(acc, n)
    touched = n > 0
    assert touched.any() and np.isfinite(got).all()
    bar = orf.ordered_bar(want, mag, cnt)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err[touched] / bar[touched]).max())
    print(f"ordered checker {orf.case_id(case)}: worst error / bar {ratio:.3f}; {int(touched.sum())} entries, "
          f"terms per entry up to {int(n.max())}")
    assert (err[touched] <= bar[touched]).all(), ratio
    assert (_bits(got)[~touched] == 0).all()                       # +0 where nothing lands


def _float32_sequential(grid, w, reverse):
    """The float32 sum a sequential float32 adder forms from the same terms, each rounded to float32
    first, in ascending (or descending) contribution id."""
    out = np.zeros((grid.total, grid.features), np.float32)
    for l in range(grid.levels):
        idx, term = orf.level_terms(grid, w["points"], w["d_encoded"], w["scale"], l)
        with np.errstate(invalid="ignore"):
            t32 = term.astype(np.float32)
        if reverse:
            idx, t32 = idx[::-1], t32[::-1]
        with np.errstate(invalid="ignore"):
            np.add.at(out, idx, t32)
    return out


@pytest.mark.parametrize("case", [c for c in CASES if c[0] >= 63], ids=orf.case_id)
def test_bit_equality_is_out_of_reach_of_float32_sums(case):
    w = orf.workload(case)
    grid = w["grid"]
    acc, n = orf.expected(case)
    ref = orf.stored(acc, n)
    up, down = _float32_sequential(grid, w, False), _float32_sequential(grid, w, True)
    assert np.isfinite(up).all() and np.isfinite(down).all() and np.isfinite(ref).all()
    orders = int((_bits(up) != _bits(down)).any(1).sum())
    against = int((_bits(up) != _bits(ref)).any(1).sum())
    print(f"{orf.case_id(case)}: float32 ascending vs descending differ on {orders} entries, float32 ascending vs "
          f"the checker on {against}, of {int((n > 0).sum())} touched")
    assert orders >= 8
    assert against >= 8


def test_the_order_is_runs_of_eight_then_partials_in_order():
    """The vectorised checker against the header's two lines written as plain loops, on the case with
    the longest lists (768 rows, F = 2, five levels)."""
    case = hw.ALL[12]
    w = hw.build(case)
    grid = w["grid"]
    acc, n = orf.expected(case)
    lists = {}
    for l in range(grid.levels):
        idx, term = orf.level_terms(grid, w["points"], w["d_encoded"], w["scale"], l)
        for c, e in enumerate(idx.tolist()):                     # ascending c
            lists.setdefault(e, []).append(term[c])
    assert sorted(lists) == np.flatnonzero(n > 0).tolist()
    assert max(len(v) for v in lists.values()) > 8 * orf.RUN and min(len(v) for v in lists.values()) < orf.RUN
    for e, terms in lists.items():
        total = np.zeros(grid.features)
        for q in range(0, len(terms), orf.RUN):
            partial = np.zeros(grid.features)
            for t in terms[q:q + orf.RUN]:
                partial = partial + t
            total = total + partial
        assert (total.view(np.uint64) == acc[e].view(np.uint64)).all(), e


def test_stored_under_accumulate_skips_untouched_entries():
    case = hw.ALL[5]
    acc, n = orf.expected(case)
    held = np.full(acc.shape, 1.25, np.float32)
    free = np.flatnonzero(n == 0)
    assert len(free)
    held[free[0]] = -0.0
    got = orf.stored(acc, n, held)
    assert (_bits(got)[n == 0] == _bits(held)[n == 0]).all()           # the -0 included
    t = n > 0
    assert (_bits(got)[t] == _bits(np.float32(1.25) + acc[t].astype(np.float32))).all()


def test_the_pile_is_what_it_says():
    w = orf.pile()
    n = w["d_table_n"]
    grid = w["grid"]
    for l in range(grid.levels):
        lv = n[grid.offset[l]:grid.offset[l + 1]]
        assert (lv > 0).sum() == 8 and (lv[lv > 0] == 768).all()
    assert (np.abs(w["d_table"]).max(1) > 0).sum() == 4 * grid.levels   # x is clamped: half the corners weigh 0
