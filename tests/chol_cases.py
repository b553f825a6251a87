"""Builders and host references of the Cholesky failure-report tests (tests/test_chol_cases.py without a GPU,
tests/test_gpu_chol_info.py on one): matrices with a planted non-positive or NaN pivot, the column a factorisation must
report for them, and the column-major layouts madqp_chol_factor is given.

The reference for a positive definite matrix with a planted diagonal entry is LAPACK's dpotrf (scipy.linalg.lapack).  For
quasi-definite matrices and for NaN it is first_failing_column below, a plain right-looking elimination with the kernel's
own rule ``not (s_j a_jj > 0)``: OpenBLAS's dpotrf, the one behind scipy here, returns 0 for a matrix that holds a NaN
(tests/test_chol_cases.py records it), so LAPACK is NOT the reference for NaN."""
import math

import numpy as np

NB = 128


# ---- matrices -------------------------------------------------------------------------------------------------------------
def spd(n, seed, cond=1e3):
    """the _spd of tests/test_gpu_dense.py, symmetrised: eigenvalues 1 .. cond, log-spaced, random orthogonal basis"""
    rng = np.random.default_rng(seed)
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0, math.log10(cond), n)
    K = (Qm * ev) @ Qm.T
    return 0.5 * (K + K.T)


def plant(K, cols, value=-1.0):
    """a copy of K with K[c, c] = value for each c of cols (the "repaired" matrix of a test is K itself)"""
    M = np.array(K, dtype=np.float64, copy=True)
    for c in cols:
        M[c, c] = value
    return M


def plant_offdiag(K, r, c, value=np.nan):
    """a copy of the symmetric K with K[r, c] = K[c, r] = value"""
    M = np.array(K, dtype=np.float64, copy=True)
    M[r, c] = M[c, r] = value
    return M


def first_failing_column(M, npos=None):
    """(info, pivot): the 1-based first column j + 1 with ``not (s_j a_jj > 0)`` in a right-looking elimination of the
    symmetric M without pivoting, s_j = +1 for j < npos and -1 from there on (npos None: all +1, plain Cholesky), and the
    pivot a_jj found there; (0, smallest s_j a_jj) when no column fails.  NaN fails the test like a non-positive pivot.
    float64, O(n^3) in numpy: for orders up to 700."""
    A = np.array(M, dtype=np.float64, copy=True)
    n = A.shape[0]
    npos = n if npos is None else npos
    smallest = np.inf
    with np.errstate(invalid="ignore"):
        for j in range(n):
            s = 1.0 if j < npos else -1.0
            a = A[j, j]
            if not (s * a > 0.0):
                return j + 1, float(a)
            smallest = min(smallest, s * a)
            l = A[j + 1:, j] / math.sqrt(s * a)
            A[j + 1:, j + 1:] -= s * np.outer(l, l)
    return 0, float(smallest)


def quasidefinite(npos, nneg, seed, c=None):
    """(stored, M): M = [P, B'; B, -Q] of order npos + nneg and what the device is given for it, [P, 0; B, +Q]
    (madqp_chol_set_signature).  P = spd(npos), B standard normal / sqrt(npos), Q = S_t - B P^-1 B' with S_t = spd(nneg):
    the Schur complement the factorisation forms in the second block, Q + B P^-1 B', is S_t up to rounding.  c: S_t[c, c]
    = -1 before Q is formed -- the first non-positive leading minor of S_t is then c + 1 (the minors before it are those
    of a positive definite matrix), and the column to report is npos + c + 1."""
    P = spd(npos, seed)
    St = spd(nneg, seed + 1)
    B = np.random.default_rng(seed + 2).standard_normal((nneg, npos)) / math.sqrt(npos)
    if c is not None:
        St = plant(St, [c])
    Qm = St - B @ np.linalg.solve(P, B.T)
    Qm = 0.5 * (Qm + Qm.T)
    stored = np.block([[P, np.zeros((npos, nneg))], [B, Qm]])
    return stored, np.block([[P, B.T], [B, -Qm]])


# ---- layouts: column-major, tensor row j = column j of the matrix -----------------------------------------------------------
def ceil128(n):
    return (n + NB - 1) // NB * NB


def unpadded(n):
    """leading dimension below the padded order (n > 128, n no multiple of 128): never the mid-size schedule"""
    return n + (3 if n % 2 else 2)


def padded(n):
    """leading dimension that covers the order rounded up to 128, as the KKT objects allocate K"""
    return ceil128(n) + 2


def poisoned(K, lda):
    """(n, lda) host array for madqp_chol_factor: the lower triangle of K, NaN in the strict upper triangle and in every
    row past n (tests/test_gpu_dense.py::test_cholesky_factor_and_solve)"""
    n = K.shape[0]
    host = np.full((n, lda), np.nan)
    host[:, :n] = np.where(np.triu(np.ones((n, n))) > 0, K.T, np.nan)
    return host


def lower_only(K, lda):
    """(n, lda) host array: the lower triangle of K, zeros everywhere else"""
    n = K.shape[0]
    host = np.zeros((n, lda))
    host[:, :n] = np.tril(K).T
    return host


# ---- the cases -------------------------------------------------------------------------------------------------------------
# Positive definite table: order -> planted columns (0-based; the report is c + 1).
# The 2500 row: the left-looking driver's first outer panel is 1024 columns wide and its second one, by the library's own
# rule (second_panel_end; tests/test_chol_cases.py asserts it), takes all the 1476 columns that remain -- so "the last column
# of the second outer panel" is 2499 and no column comes after it.  The plan halves that panel at 1024 + 768: 1791 and
# 1792 stand for the edge inside it.
FIRST_PANEL = 1024
PD_TABLE = {
    1: (0,),
    17: (0, 15, 16),
    128: (0, 127),
    129: (127, 128),  # a last block of one column
    300: (0, 16, 127, 128, 255, 256, 299),
    1100: (0, 511, 512, 1023, 1024, 1099),  # first halving of the first outer panel, its end, the ragged last block
    2500: (1023, 1024, 1791, 1792, 2499),
}
TWO_FAILURES = {300: (16, 256), 1100: (512, 1099), 2500: (1024, 2499)}  # the report is the first of the two
# every case as (order, planted columns)
CASES = [(n, (c,)) for n, cols in PD_TABLE.items() for c in cols] + list(TWO_FAILURES.items())
BAND_SHAPES = [(300, 40), (1100, 130), (1537, 300)]  # (n, bw): one block column of band, two, three
QD_SECOND_BLOCK = [(128, 50, 0), (128, 50, 49), (256, 300, 127), (256, 300, 128), (256, 300, 299)]  # (npos, nneg, c)
QD_FIRST_BLOCK = [(npos, nneg, c) for npos, nneg in ((128, 50), (256, 300)) for c in sorted({0, 127, npos - 1})]
NAN_ORDERS = {17: (3, 13), 300: (40, 126), 1100: (600, 1022)}  # order -> c: one inside a block, one whose r = c + 3 lies in the next
# (n = 17: the next 16-column sub-block; 1100: the next outer panel too)


def second_panel_end(n=2500):
    """first column past the second outer panel of the left-looking plan (chol_plan.inc) at order n"""
    from band_cases import SLOTS, band_lib

    lib = band_lib()
    assert min(lib.band_dense_outer_width(n, 0, SLOTS), n) == FIRST_PANEL
    return FIRST_PANEL + int(min(lib.band_dense_outer_width(n - FIRST_PANEL, 1, SLOTS), n - FIRST_PANEL))


def first_half(w):
    """columns of the first half of a w-column range in the plan's halving (chol_plan.inc): whole blocks, the larger half first"""
    return ((w + NB - 1) // NB + 1) // 2 * NB


def case_id(case):
    n, cols = case
    return "n%d-c%s" % (n, "+".join(str(c) for c in cols))


def band_columns(n, bw):
    """planted columns of a band case: column 0, 128 k - 1 and 128 k for one k, the last column"""
    k = (n // NB + 1) // 2
    return (0, NB * k - 1, NB * k, n - 1)


_cache = {}


def good(n):
    """the one positive definite matrix of order n every table case plants into (shared, never modified)"""
    if n not in _cache:
        K = spd(n, n)
        K.setflags(write=False)
        _cache[n] = K
    return _cache[n]
