"""Helpers of the band tests (tests/test_band_*.py, tests/test_gpu_band*.py): madqp_jl_amd/csrc/band_plan.inc through its
one CPU build (tests/csrc_band -> libmadqp_band.so) -- the plan of the factorisation, the job lists of the sweeps and what
the kernels make of a job, the layout of packed band storage --, the band matrices, banded QPs for the sparse front end,
and packed buffers with NaN in every slot that is no band entry."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 128
SLOTS = 512  # resident GEMM workgroups of one MI355X (madqp_ctx::gemm_slots): 2 per CU
UPDATE, BLOCK = 0, 1
NAN_BITS = np.float64(np.nan).view(np.uint64)

_lib = None


def band_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_band")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_band.so"))
        i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
        for name, args in (("band_plan_rows", [i64, i64, i64, i64, i64, vp, i64, vp]), ("band_dense_outer_width", [i64, i64, i64]),
                           ("band_sweep_blocks_c", [i64]), ("band_sweep_reach_c", [i64, i64]),
                           ("band_sweep_jobs_c", [i64, i64, i64, vp, i64, vp]),
                           ("band_packed_layout_c", [i64, i64, i64, i64, vp]), ("band_packed_default_pad_c", [])):
            getattr(_lib, name).restype = i64
            getattr(_lib, name).argtypes = args
        _lib.band_sweep_range_c.restype = None
        _lib.band_sweep_range_c.argtypes = [i32, i32, i32, i32, vp]
        _lib.chol_range_rows.restype = None
        _lib.chol_range_rows.argtypes = [i64, i64, i64, vp, i64, vp]
    return _lib


def _plan_rows(n, fill):
    cap = 4 * (n // NB + 2) + 16
    rows = np.zeros((cap, 7), dtype=np.int64)
    cnt = C.c_int64(0)
    out = fill(rows.ctypes.data, cap, C.byref(cnt))
    assert 0 < cnt.value <= cap
    return rows[: cnt.value], out


def plan(n, bw, slots=SLOTS, force_wt=0, npos=None):
    """(operations as rows (kind, row0, rows, k0, kend, width, sign), extent); npos: the signature, None for positive
    definite"""
    lib = band_lib()
    rows, extent = _plan_rows(n, lambda *out: lib.band_plan_rows(n, bw, n if npos is None else npos, slots, force_wt, *out))
    return rows, int(extent)


def range_plan(n, j0, w):
    """the operations of the bare halving of the columns [j0, j0 + w) of an order-n matrix, rows as above"""
    lib = band_lib()
    return _plan_rows(n, lambda *out: lib.chol_range_rows(n, j0, w, *out))[0]


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


# ---- the sweeps under a band ----
def sweep_jobs(nblk, kb, chunk):
    """((r, c) per ticket, maxc) of one sweep; kb < 0: the dense list"""
    lib = band_lib()
    cap = nblk * (nblk + 1) // 2 + nblk + 1
    out = np.zeros(cap, dtype=np.int32)
    cnt = C.c_int64(0)
    maxc = lib.band_sweep_jobs_c(nblk, kb, chunk, out.ctypes.data, cap, C.byref(cnt))
    assert 0 < cnt.value <= cap
    return [(int(j) & 0xFFFFF, int(j) >> 20) for j in out[: cnt.value]], int(maxc)


def dense_jobs(nblk, chunk):
    """the list madqp_chol_create builds"""
    return [(r, c) for r in range(nblk) for c in range(max(1, (r + chunk - 1) // chunk))]


def ranges(r, c, kb, chunk):
    """what the kernels make of job (r, c) -- band_sweep_range, the function they compile: its tiles [j0, j1), whether it
    owns the row, the first chunk it waits for"""
    out = (C.c_int32 * 4)()
    band_lib().band_sweep_range_c(r, c, chunk, kb, out)
    return out[0], out[1], bool(out[2]), out[3]


def workgroups(n, kb, chunk):
    """workgroups of one sweep of a handle of order n (madqp_chol_sweep_info): the job count where block rows are split"""
    nblk = max(1, (n + 127) // 128)
    return len(sweep_jobs(nblk, kb, chunk)[0]) if nblk - 1 > chunk else nblk


# ---- packed band storage ----
def layout(n, extent, ld_in=0, pad=-1):
    """(ld, doubles) of band_packed_layout, None where it refuses; ld_in <= 0: the library's choice"""
    out = (C.c_int64 * 2)()
    return (out[0], out[1]) if band_lib().band_packed_layout_c(n, extent, ld_in, pad, out) else None


def npad(n):
    return (max(n, 1) + NB - 1) // NB * NB


def band_index(n, extent):
    """(i, j) of every entry with 0 <= i - j <= extent, column by column"""
    cnt = np.minimum(extent + 1, n - np.arange(n))  # entries of column j
    j = np.repeat(np.arange(n), cnt)
    i = np.arange(len(j)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + j
    return i, j


def lds_to_test(n, extent):
    """the leading dimensions the issue asks for: the extent itself, extent + 1, the library's choice, extent + 37"""
    return [max(extent, 1), extent + 1, layout(n, extent)[0], extent + 37]


def pack(K, extent, ld, doubles):
    """A packed buffer of `doubles` doubles holding the entries 0 <= i - j <= extent of K at [i + j ld], NaN in every other
    slot (the gaps extent < i - j <= ld and the slack); returns (buffer, addresses of the band entries)."""
    n = K.shape[0]
    i, j = band_index(n, extent)
    addr = i + j * ld
    assert len(np.unique(addr)) == len(addr) and addr.max() < doubles
    buf = np.full(doubles, np.nan)
    buf[addr] = K[i, j]
    return buf, addr


def view(buf, n, ld):
    """the buffer as the column-major (npad, n) matrix the kernels address: [i, j] = buf[i + j ld].  Entries above the
    diagonal and beyond ld alias other columns -- what executes a plan through it must write neither."""
    assert (npad(n) - 1) + (n - 1) * ld < len(buf)
    return np.lib.stride_tricks.as_strided(buf, shape=(npad(n), n), strides=(8, 8 * ld))


def unpack(buf, n, extent, ld):
    """dense lower triangle from a packed buffer, zeros beyond the extent"""
    i, j = band_index(n, extent)
    L = np.zeros((n, n))
    L[i, j] = buf[i + j * ld]
    return L


def nan_kept(buf, addr):
    """every slot that is no band entry still holds the planted NaN, bit for bit"""
    mask = np.ones(len(buf), dtype=bool)
    mask[addr] = False
    return bool(np.all(buf.view(np.uint64)[mask] == NAN_BITS))
