"""No GPU: the expected values of tests/test_gpu_chol_info.py.  Every planted matrix of tests/chol_cases.py reports the
column the GPU tests expect from LAPACK's dpotrf and from the plain reference loop (first_failing_column); the cases are well
posed, i.e. far from the border between "fails" and "does not fail"; and the reference's behaviour on NaN is pinned, since
LAPACK is no reference there."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import chol_cases as cc
from band_cases import SLOTS, band_lib, band_spd

LOOP_MAX = 700  # first_failing_column is O(n^3) in numpy


def dpotrf_info(M):
    return int(sla.lapack.dpotrf(M, lower=1)[1])


@functools.lru_cache(maxsize=None)
def good_factor(n):
    return sla.cholesky(cc.good(n), lower=True)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_planted_columns_are_what_lapack_reports(case):
    n, cols = case
    M = cc.plant(cc.good(n), cols)
    assert np.array_equal(M, M.T) and not np.shares_memory(M, cc.good(n))
    expected = min(cols) + 1
    assert dpotrf_info(M) == expected
    if n <= LOOP_MAX:
        info, pivot = cc.first_failing_column(M)
        assert info == expected and pivot < 0.0


@pytest.mark.parametrize("n", list(cc.PD_TABLE))
def test_good_matrices_report_zero(n):
    K = cc.good(n)
    assert dpotrf_info(K) == 0
    if n <= LOOP_MAX:
        info, smallest = cc.first_failing_column(K)
        assert info == 0 and smallest > 0.0


@pytest.mark.parametrize("n", list(cc.PD_TABLE))
def test_cases_are_well_posed(n):
    """A condition, not a measurement: with d = max |diag K| every pivot of the good matrix is at least 1e-3 d and every
    failing pivot at most -1e-3 d, so no rounding of a correct factorisation can move a case across zero.  (The pivots of
    K are at least its smallest eigenvalue, 1, and d is at most its largest, 1e3; a planted -1 only goes down by the squares
    of the row left of it.)  The pivot at the planted column c is -1 - |L[c, :c]|^2 with L the factor of the good matrix: the
    columns left of c are untouched by the planting."""
    K, L = cc.good(n), good_factor(n)
    d = np.max(np.abs(np.diag(K)))
    pivots = np.diag(L) ** 2
    assert d <= 1e3 * (1 + 1e-12)
    assert pivots.min() >= 1e-3 * d, (pivots.min(), d)
    planted = sorted({c for m, cols in cc.CASES if m == n for c in cols})
    failing = []
    for c in planted:
        failing.append(-1.0 - float(L[c, :c] @ L[c, :c]))
        if n <= LOOP_MAX:
            info, pivot = cc.first_failing_column(cc.plant(K, [c]))
            assert info == c + 1 and abs(pivot - failing[-1]) <= 1e-9 * abs(pivot)
    print(f"n={n}: d={d:.4g}, smallest good pivot {pivots.min():.4g}, failing pivots {min(failing):.4g} .. {max(failing):.4g}")
    assert max(failing) <= -1e-3 * d, (failing, d)


def test_the_table_sits_on_the_panel_edges():
    """the edges the table is built around are those of the library's own rules"""
    lib = band_lib()
    for n in (1100, 2500):  # the first outer panel of the left-looking driver is 1024 columns wide at both orders
        assert min(lib.band_dense_outer_width(n, 0, SLOTS), n) == cc.FIRST_PANEL
    # ... and the second one takes all that remains of 2500: its last column is the matrix's, none comes after it
    assert cc.second_panel_end(2500) == 2500 and 2499 in cc.PD_TABLE[2500]
    assert cc.second_panel_end(1100) == 1100
    # the plan's halvings: 1024 -> 512 -> 256 -> 128 in the first panel, 1476 -> 768 + 708 in the second panel of 2500
    assert [cc.first_half(w) for w in (1024, 512, 256, 2500 - 1024, 300)] == [512, 256, 128, 768, 256]
    assert {511, 512} <= set(cc.PD_TABLE[1100]) and {1024 + 768 - 1, 1024 + 768} <= set(cc.PD_TABLE[2500])
    for n, cols in cc.PD_TABLE.items():
        assert all(0 <= c < n for c in cols)
        if n > cc.NB:  # what sends the unpadded layout past the mid-size schedule and the padded one into it
            assert n % cc.NB and cc.unpadded(n) < cc.ceil128(n) <= cc.padded(n) and cc.padded(n) % 2 == 0
    for n, cols in cc.TWO_FAILURES.items():
        assert len(cols) == 2 and cols[0] < cols[1] < n


@pytest.mark.parametrize("n,bw", cc.BAND_SHAPES)
def test_band_cases(n, bw):
    K = band_spd(n, bw)
    assert dpotrf_info(K) == 0
    cols = cc.band_columns(n, bw)
    assert cols[0] == 0 and cols[1] + 1 == cols[2] and cols[2] % cc.NB == 0 and cols[3] == n - 1 and cols[2] < n - 1
    for c in cols:
        assert dpotrf_info(cc.plant(K, [c])) == c + 1


@pytest.mark.parametrize("npos,nneg,c", cc.QD_SECOND_BLOCK)
def test_quasidefinite_second_block(npos, nneg, c):
    stored, M = cc.quasidefinite(npos, nneg, npos + nneg, c)
    assert cc.first_failing_column(M, npos)[0] == npos + c + 1
    assert np.array_equal(np.tril(stored)[npos:, npos:], -np.tril(M)[npos:, npos:]), "the device is given +Q"
    assert np.array_equal(np.tril(stored)[:, :npos], np.tril(M)[:, :npos])


@pytest.mark.parametrize("npos,nneg", [(128, 50), (256, 300)])
def test_quasidefinite_unplanted_and_first_block(npos, nneg):
    stored, M = cc.quasidefinite(npos, nneg, npos + nneg)
    info, smallest = cc.first_failing_column(M, npos)
    assert info == 0 and smallest > 0.0
    for c in (0, 127, npos - 1):
        assert cc.first_failing_column(cc.plant(M, [c]), npos)[0] == c + 1


@pytest.mark.parametrize("n", list(cc.NAN_ORDERS))
def test_nan_reference(n):
    """first_failing_column on NaN: at (c, c) it reports c + 1; at (r, c), r > c, it reports r + 1 -- column c of the factor
    carries the NaN in row r, and the first pivot that sees it is a_rr.  This is the reference of the GPU tests for NaN:
    OpenBLAS's dpotrf (behind scipy here) returned 0 for every one of these matrices when this test was written, so LAPACK
    is not.  Its answer is printed, not asserted: another LAPACK may well catch the NaN."""
    K = cc.good(n)
    for c in cc.NAN_ORDERS[n]:
        r = c + 3
        assert r < n
        Md, Mo = cc.plant(K, [c], np.nan), cc.plant_offdiag(K, r, c)
        info_d, pivot_d = cc.first_failing_column(Md)
        info_o, pivot_o = cc.first_failing_column(Mo)
        print(f"n={n} c={c}: NaN at (c, c) -> {info_d} (dpotrf {dpotrf_info(Md)}); NaN at ({r}, c) -> {info_o} "
              f"(dpotrf {dpotrf_info(Mo)})")
        assert info_d == c + 1 and np.isnan(pivot_d)
        assert info_o == r + 1 and np.isnan(pivot_o)
    blk = cc.NB if n > cc.NB else 16
    inside, across = cc.NAN_ORDERS[n]
    assert inside // blk == (inside + 3) // blk and across // blk < (across + 3) // blk, "r in the same block / in the next"
