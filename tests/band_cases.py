"""Helpers of the band tests (tests/test_band_plan.py, tests/test_gpu_band.py): the band matrices, the plan of
madqp_jl_amd/csrc/band_plan.inc through its CPU build, and banded QPs for the sparse front end."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 128
SLOTS = 512  # resident GEMM workgroups of one MI355X (madqp_ctx::gemm_slots): 2 per CU
UPDATE, BLOCK = 0, 1

_lib = None


def plan_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_band")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_band_plan.so"))
        _lib.band_plan_rows.restype = C.c_int64
        _lib.band_plan_rows.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.band_dense_outer_width.restype = C.c_int64
        _lib.band_dense_outer_width.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    return _lib


def plan(n, bw, slots=SLOTS, force_wt=0):
    """(operations as rows (kind, row0, rows, k0, kend, width), extent)"""
    lib = plan_lib()
    cap = 4 * (n // NB + 2) + 16
    rows = np.zeros((cap, 6), dtype=np.int64)
    cnt = C.c_int64(0)
    extent = lib.band_plan_rows(n, bw, slots, force_wt, rows.ctypes.data, cap, C.byref(cnt))
    assert 0 < cnt.value <= cap
    return rows[: cnt.value], int(extent)


def band_factor(n, bw, seed=None):
    """L0: standard-normal lower band with diagonal 1 + |.| + sqrt(bw + 1); K = L0 L0' has half-bandwidth bw and a
    condition number of at most 1.3e3 at every shape the band tests use."""
    rng = np.random.default_rng(1000 * n + bw if seed is None else seed)
    L0 = np.tril(rng.standard_normal((n, n)))
    i, j = np.indices((n, n))
    L0[i - j > bw] = 0.0
    L0[np.diag_indices(n)] = 1.0 + np.abs(np.diag(L0)) + np.sqrt(bw + 1.0)
    return L0


def band_spd(n, bw, seed=None):
    L0 = band_factor(n, bw, seed)
    K = L0 @ L0.T
    return 0.5 * (K + K.T)


def banded_qp(nx, m, abw, seed, n_eq=0, free_curvature=None):
    """A condensed-form QP whose KKT matrix is a band matrix: H tridiagonal and positive definite, row r of A holds
    `abw` + 1 consecutive variables starting where the rows are spread evenly over the variables; the first n_eq rows are
    equalities.  free_curvature: variable 3 becomes free with that (negative) curvature and leaves every row of A, so the
    first factorisation of a solve breaks down and the x100 regularisation retry succeeds.  Returns the fields of
    DeviceQP.from_numpy with H and A as scipy CSR."""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, nx))
    for r in range(m):
        c0 = int(round(r * (nx - abw - 1) / max(m - 1, 1)))
        A[r, c0: c0 + abw + 1] = rng.standard_normal(abw + 1)
    off = 0.3 * rng.standard_normal(nx - 1)
    H = np.diag(2.0 + rng.random(nx)) + np.diag(off, 1) + np.diag(off, -1)
    q = rng.standard_normal(nx)
    lvar, uvar = -1.0 - rng.random(nx), 1.0 + rng.random(nx)
    x0 = np.zeros(nx)
    lcon, ucon = -1.0 - rng.random(m), 1.0 + rng.random(m)
    if n_eq:
        lcon[:n_eq] = ucon[:n_eq] = 0.1 * rng.standard_normal(n_eq)
    if free_curvature is not None:
        f = 3
        A[:, f] = 0.0
        H[f, :] = H[:, f] = 0.0
        H[f, f] = free_curvature
        q[f] = 0.0
        lvar[f], uvar[f] = -np.inf, np.inf
    return dict(H=sp.csr_matrix(H), q=q, A=sp.csr_matrix(A), lvar=lvar, uvar=uvar, lcon=lcon, ucon=ucon, x0=x0)


def dense_pattern_bandwidth(A, H, form):
    """max (i - j) over the non-zeros of |A|'|A| + |H| (condensed) or |A||A|' (normal), dense numpy"""
    A = np.abs(np.asarray(A.todense() if sp.issparse(A) else A))
    G = A.T @ A if form == "condensed" else A @ A.T
    if H is not None and form == "condensed":
        G = G + np.abs(np.asarray(H.todense() if sp.issparse(H) else H))
    i, j = np.nonzero(G)
    return int(np.max(i - j)) if len(i) else 0
