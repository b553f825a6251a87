"""CPU: the plan of a blocked solve with many right-hand sides (madqp_jl_amd/csrc/solve_plan.inc, compiled for the CPU by
tests/csrc_solve).  The operations are executed in numpy float64 on real factors -- positive definite, quasi-definite,
banded with NaN beyond the sweeps' reach -- and held to scipy; their order and the byte count are checked; the refusals
of ``solve_many`` / ``HIPCholeskySolver.solve`` happen before any device call.  The kernels that run the plan are held in
tests/test_gpu_solve_many.py."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import chol_cases
from band_cases import band_lib, band_spd
from madqp_jl_amd.dist2d import HIPDistributedCondensedKKTSystem2D
from madqp_jl_amd.kkt import HIPCholeskySolver, HIPCondensedKKTSystem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 128
DIAG, UPDATE, NEGATE = 0, 1, 2
NS = (1, 17, 128, 129, 300, 640, 1100)
NRHS = (1, 2, 15, 16, 17, 33, 130)
SIGNATURES = ((128, 1), (128, 172), (256, 300))
BANDS = ((500, 0), (500, 127), (1537, 127), (1537, 129), (1537, 300), (2100, 640))  # (n, bw): shapes of tests/test_band_plan.py
RES_BOUND, SOL_BOUND = 1e-14, 1e-10  # tests/test_gpu_dense.py::test_cholesky_factor_and_solve

_lib = None


def solve_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_solve")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_solveplan.so"))
        i64, vp = C.c_int64, C.c_void_p
        _lib.solve_plan_rows.restype = None
        _lib.solve_plan_rows.argtypes = [i64, i64, i64, i64, i64, vp, i64, vp, vp]
        _lib.solve_looped_count_c.restype = None
        _lib.solve_looped_count_c.argtypes = [i64, i64, i64, i64, i64, vp]
        _lib.solve_plan_workspace_c.restype = i64
        _lib.solve_plan_workspace_c.argtypes = [i64, i64, i64]
    return _lib


def plan(n, npos, kb, nrhs, has_upper=False):
    """(operations as rows (kind, sweep, blk, row0, rows, k0, k1, bytes), launches, bytes)"""
    cap = 4 * (n // NB + 2) + 4
    rows = np.zeros((cap, 8), dtype=np.int64)
    cnt = C.c_int64(0)
    count = np.zeros(2, dtype=np.int64)
    solve_lib().solve_plan_rows(n, npos, kb, nrhs, int(has_upper), rows.ctypes.data, cap, C.byref(cnt), count.ctypes.data)
    assert cnt.value <= cap
    return rows[: cnt.value], int(count[0]), int(count[1])


def execute(ops, L, B):
    """The operations on the transposed block T = B' (what the device holds), L read where the operations say only."""
    T = np.array(B.T, dtype=np.float64, copy=True)  # (nrhs, n)
    for kind, sweep, _, row0, rows, k0, k1, _ in ops:
        if kind == DIAG:
            D = np.tril(L[k0:k1, k0:k1])
            T[:, k0:k1] = sla.solve_triangular(D, T[:, k0:k1].T, lower=True, trans="T" if sweep else "N").T
        elif kind == UPDATE:
            blockL = L[row0: row0 + rows, k0:k1].T if sweep == 0 else L[k0:k1, row0: row0 + rows]
            T[:, row0: row0 + rows] -= T[:, k0:k1] @ blockL
        else:
            assert kind == NEGATE
            T[:, row0: row0 + rows] *= -1.0
    return T.T


def check_structure(ops, n, npos, kb, total_bytes):
    nblk = (n + NB - 1) // NB
    reach = n - 1 if kb < 0 else min(n - 1, kb * NB + NB - 1)
    solved = np.zeros((2, nblk), dtype=int)
    touched = np.zeros((2, nblk), dtype=int)  # updates received
    negated = 0
    for kind, sweep, blk, row0, rows, k0, k1, _ in ops:
        if kind == NEGATE:
            negated += 1
            assert (row0, row0 + rows) == (npos, n) and solved[0].all() and not solved[1].any()
            continue
        assert k0 == blk * NB and k1 == min(n, k0 + NB) and rows >= 1 and 0 <= row0 and row0 + rows <= n
        if kind == DIAG:
            assert (row0, rows) == (k0, k1 - k0)
            solved[sweep, blk] += 1
            # every update of a block precedes its diagonal step: all the blocks within reach have been applied
            want = min(blk, nblk if kb < 0 else kb) if sweep == 0 else min(nblk - 1 - blk, nblk if kb < 0 else kb)
            assert touched[sweep, blk] == want, (sweep, blk, touched[sweep, blk], want)
        else:
            assert solved[sweep, blk] == 1, "a block's solution is applied after its diagonal step"
            for j in range(row0 // NB, (row0 + rows - 1) // NB + 1):
                assert solved[sweep, j] == 0, "an update after the diagonal step of its target"
                touched[sweep, j] += 1
            far = row0 + rows - 1 - k0 if sweep == 0 else k1 - 1 - row0
            assert far <= reach, "no entry beyond the reach of the band sweeps"
    assert (solved == 1).all(), "every block is solved once per sweep"
    assert negated == (1 if npos < n else 0)
    assert total_bytes == int(ops[:, 7].sum()), "the byte count is the sum over the operations"


def check_solution(X, Xref, K, B):
    normK = np.linalg.norm(K, 2)
    for c in range(B.shape[1]):
        x, xr = X[:, c], Xref[:, c]
        res = np.linalg.norm(K @ x - B[:, c]) / (normK * np.linalg.norm(x))
        err = np.linalg.norm(x - xr) / np.linalg.norm(xr)
        assert res < RES_BOUND, (c, res)
        assert err < SOL_BOUND, (c, err)


_factors = {}


def spd_factor(n):
    if n not in _factors:
        K = chol_cases.good(n)
        _factors[n] = (K, sla.cholesky(K, lower=True))
    return _factors[n]


def test_sanitized_walk_of_the_plan():
    solve_lib()
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "solve_plan_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAD" not in out.stdout and out.stdout.count(" ok") > 200


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("nrhs", NRHS)
def test_executed_plan_solves_spd(n, nrhs):
    K, L = spd_factor(n)
    B = np.random.default_rng(7 * n + nrhs).standard_normal((n, nrhs))
    for has_upper in (False, True):
        ops, launches, nbytes = plan(n, n, -1, nrhs, has_upper)
        check_structure(ops, n, n, -1, nbytes)
        assert launches == len(ops) + 2 + (0 if has_upper else int(((ops[:, 0] == UPDATE) & (ops[:, 1] == 1)).sum()))
    i, j = np.indices((n, n))
    X = execute(ops, np.where(i >= j, L, np.nan), B)  # nothing above the diagonal is read
    assert np.isfinite(X).all()
    check_solution(X, sla.cho_solve((L, True), B), K, B)


@pytest.mark.parametrize("npos,nneg", SIGNATURES)
def test_executed_plan_solves_quasidefinite(npos, nneg):
    stored, M = chol_cases.quasidefinite(npos, nneg, 100 + npos + nneg)
    n = npos + nneg
    L11 = sla.cholesky(stored[:npos, :npos], lower=True)
    W = sla.solve_triangular(L11, stored[npos:, :npos].T, lower=True).T
    L22 = sla.cholesky(stored[npos:, npos:] + W @ W.T, lower=True)
    L = np.block([[L11, np.zeros((npos, nneg))], [W, L22]])
    for nrhs in (1, 17, 33):
        B = np.random.default_rng(npos + nrhs).standard_normal((n, nrhs))
        ops, _, nbytes = plan(n, npos, -1, nrhs)
        check_structure(ops, n, npos, -1, nbytes)
        check_solution(execute(ops, L, B), np.linalg.solve(M, B), M, B)


@pytest.mark.parametrize("n,bw", BANDS)
def test_executed_plan_stays_inside_the_band(n, bw):
    K = band_spd(n, bw)
    L = sla.cholesky(K, lower=True)
    kb = int(band_lib().band_sweep_blocks_c(bw))
    reach = int(band_lib().band_sweep_reach_c(n, kb))
    i, j = np.indices((n, n))
    assert np.all(L[i - j > bw] == 0.0)
    Lnan = np.where((i >= j) & (i - j <= reach), L, np.nan)  # NaN beyond what the band sweeps may read
    nrhs = 17
    B = np.random.default_rng(n + bw).standard_normal((n, nrhs))
    ops, _, nbytes = plan(n, n, kb, nrhs)
    check_structure(ops, n, n, kb, nbytes)
    X = execute(ops, Lnan, B)
    assert np.isfinite(X).all(), "an entry beyond min(n - 1, 128 kb + 127) was read"
    check_solution(X, sla.cho_solve((L, True), B), K, B)
    dense_bytes = plan(n, n, -1, nrhs)[2]
    assert nbytes <= dense_bytes and (nbytes < dense_bytes or reach == n - 1)


def test_counts_of_the_two_paths():
    lib = solve_lib()
    n, nrhs = 1100, 64
    ops, launches, nbytes = plan(n, n, -1, nrhs, has_upper=True)
    tri = sum(8 * (w * (w + 1) // 2) for w in [128] * 8 + [76])  # diagonal blocks
    below = 8 * sum((n - min(n, (j + 1) * NB)) * min(NB, n - j * NB) for j in range(9))
    assert nbytes == 2 * (tri + below), "every block of L once per sweep"
    assert plan(n, n, -1, nrhs, has_upper=False)[2] == 2 * tri + 4 * below, "the strip: read, written, read again"
    cnt = np.zeros(2, dtype=np.int64)
    lib.solve_looped_count_c(n, n, -1, nrhs, 1, cnt.ctypes.data)
    assert cnt[1] == nrhs * nbytes and cnt[0] == 3 * nrhs
    assert plan(n, n, -1, 1, True)[2] == plan(n, n, -1, 130, True)[2], "the factor traffic does not grow with nrhs"
    assert lib.solve_plan_workspace_c(n, nrhs, 1) == 128 * 1152
    assert lib.solve_plan_workspace_c(n, 130, 0) == 256 * 1152 + 128 * 1152
    assert plan(0, 0, -1, 5)[0].shape[0] == 0 and plan(5, 5, -1, 0)[0].shape[0] == 0


# ---- the Python refusals: before any device call -----------------------------------------------------------------------------
class Recorder:
    """a backend that records what reaches it"""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def kkt_chol(self, h):
        return "chol", 12

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append(name)


def fake_kkt():
    k = HIPCondensedKKTSystem.__new__(HIPCondensedKKTSystem)
    k.be, k._h = Recorder(), "kkt"
    k.st = types.SimpleNamespace(n=6, m=3, nlb=2, nub=1)
    return k


BAD_BLOCKS = {
    "1-D": lambda: torch.zeros(12, dtype=torch.float64),
    "3-D": lambda: torch.zeros((2, 2, 12), dtype=torch.float64),
    "short rows": lambda: torch.zeros((4, 11), dtype=torch.float64),
    "float32": lambda: torch.zeros((4, 12), dtype=torch.float32),
    "row stride": lambda: torch.zeros((4, 24), dtype=torch.float64)[:, :12],
    "transposed": lambda: torch.zeros((12, 4), dtype=torch.float64).T,
    "numpy": lambda: np.zeros((4, 12)),
}


@pytest.mark.parametrize("what", sorted(BAD_BLOCKS))
def test_solve_many_refuses_before_a_device_call(what):
    k = fake_kkt()
    with pytest.raises(ValueError):
        k.solve_many(BAD_BLOCKS[what]())
    assert k.be.calls == []
    if what != "1-D":
        s = HIPCholeskySolver(k.be, "kkt")
        with pytest.raises(ValueError):
            s.solve(BAD_BLOCKS[what]())
        assert k.be.calls == []


def test_solve_many_passes_a_good_block_on():
    k = fake_kkt()
    W = torch.zeros((4, 13), dtype=torch.float64)
    assert k.solve_many(W) is W and k.be.calls == ["kkt_solve_many"]
    assert k.solve_many(W[:0]) is not None and k.be.calls == ["kkt_solve_many"], "no right-hand side: no call"
    s = HIPCholeskySolver(k.be, "kkt")
    s.solve(W)
    s.solve(W[0])
    assert k.be.calls == ["kkt_solve_many", "chol_solve_many", "chol_solve"]
    with pytest.raises(ValueError):
        s.solve(torch.zeros(11, dtype=torch.float64))


def test_a_grid_refuses_with_a_message():
    g = HIPDistributedCondensedKKTSystem2D.__new__(HIPDistributedCondensedKKTSystem2D)
    with pytest.raises(ValueError, match="grid"):
        g.solve_many(torch.zeros((4, 12), dtype=torch.float64))
    be = Recorder()
    with pytest.raises(ValueError, match="grid"):
        HIPCholeskySolver(be, None).solve(torch.zeros((4, 12), dtype=torch.float64))
    assert be.calls == []
