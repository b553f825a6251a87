"""CPU: the schedule of the left-looking Cholesky (madqp_jl_amd/csrc/chol_plan.inc, compiled for the CPU by
tests/csrc_band) -- band-limited, dense, quasi-definite, and the bare halving of a column range.  The plan is executed in
numpy float64 on band and quasi-definite matrices and held to LAPACK; its ranges are checked against the band and the extent
it reports; the dense, quasi-definite and range plans are held to restatements of their rules in Python;
``kkt.pattern_bandwidth`` is held to dense numpy; the refusals of ``kkt_bandwidth`` happen before any device call.  The
kernels that run the plan are held in tests/test_gpu_band.py."""
import math
import os
import subprocess
import types

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import torch

import madqp_jl_amd as M
from madqp_jl_amd import preprocess as P
from madqp_jl_amd.kkt import pattern_bandwidth
import chol_cases as cc
from band_cases import (BLOCK, NB, ROOT, SLOTS, UPDATE, band_spd, banded_qp, band_lib, dense_pattern_bandwidth, plan, range_plan)

CPU = torch.device("cpu")
NS = (1, 128, 129, 500, 1537, 2100)
SHAPES = [(n, bw) for n in NS for bw in sorted({0, 1, 127, 128, 129, 300, 640, n - 1}) if bw < n]
RANGE_ONLY = [(90000, 600), (22500, 300)]
# (npos, nneg): an empty positive block; panels cut at npos (768 / 800, 1280 / 2900); a first panel that ends at npos; a
# short cut panel (1152); a negative block of two outer panels, whose second receives the + and the - update (2561 is the
# smallest nneg with one at 512 slots)
SIGNATURES = [(0, 300), (128, 50), (256, 300), (768, 800), (1024, 129), (1152, 1300), (128, 2561), (1280, 2900), (2304, 1500)]
SIGNATURES_EXECUTED = [(128, 50), (256, 300), (768, 800), (128, 2561)]
RANGES = [(1, 0, 1), (128, 0, 128), (129, 0, 129), (640, 0, 640), (1000, 0, 1000), (900, 256, 644), (2100, 1024, 1076)]  # (n, j0, w)


def execute(ops, K, extent):
    """The operations on a copy of K (lower triangle; NaN above the diagonal and beyond the extent)."""
    n = K.shape[0]
    i, j = np.indices((n, n))
    W = np.where((i >= j) & (i - j <= extent), K, np.nan)
    for kind, row0, rows, k0, kend, width, sign in ops:
        if kind == UPDATE:
            X = W[row0: row0 + rows, k0: kend]
            Y = W[row0: row0 + width, k0: kend]
            low = i[row0: row0 + rows, row0: row0 + width] >= j[row0: row0 + rows, row0: row0 + width]
            C = W[row0: row0 + rows, row0: row0 + width]
            C[low] += sign * (X @ Y.T)[low]
        else:
            jb, w = row0, width
            D = np.tril(W[jb: jb + w, jb: jb + w])
            L = np.linalg.cholesky(D + np.tril(D, -1).T)
            W[jb: jb + w, jb: jb + w][np.tril_indices(w)] = L[np.tril_indices(w)]
            if rows:
                X = W[jb + w: jb + w + rows, jb: jb + w]
                X[:] = sla.solve_triangular(L, X.T, lower=True).T
    return W


@pytest.mark.parametrize("n,bw", SHAPES)
def test_executed_plan_factors_the_band_matrix(n, bw):
    K = band_spd(n, bw)
    ops, extent = plan(n, bw)
    L = executed_factor(ops, K, extent, K, np.ones(n), sla.cholesky(K, lower=True))
    i, j = np.indices((n, n))
    assert np.all(L[i - j > bw] == 0.0), "the factor stays inside the band: stored zeros stay zeros"


def executed_factor(ops, stored, extent, M, signs, Lref):
    """L of the plan executed on `stored`, held to M = L diag(signs) L' and to Lref"""
    n = M.shape[0]
    W = execute(ops, stored, extent)
    i, j = np.indices((n, n))
    outside = (i < j) | (i - j > extent)
    assert np.all(np.isnan(W[outside])), "nothing beyond the extent (or above the diagonal) is written"
    assert not np.any(np.isnan(W[~outside])), "nothing beyond the extent is read"
    L = np.where(outside, 0.0, W)
    rel = np.linalg.norm((L * signs) @ L.T - M) / np.linalg.norm(M)
    assert rel < 1e-14 * max(1, math.sqrt(n)), rel
    assert np.max(np.abs(L - Lref)) / np.max(np.abs(Lref)) < 1e-11
    return L


@pytest.mark.parametrize("npos,nneg", SIGNATURES_EXECUTED)
def test_executed_signature_plan_factors_the_quasidefinite_matrix(npos, nneg):
    """[P, B'; B, -Q] = L diag(I, -I) L'; the reference by blocks with LAPACK: L11 = chol(P), W = B L11^-T,
    L22 = chol(Q + W W')."""
    n = npos + nneg
    stored, M = cc.quasidefinite(npos, nneg, n)
    L11 = sla.cholesky(stored[:npos, :npos], lower=True)
    Wm = sla.solve_triangular(L11, stored[npos:, :npos].T, lower=True).T
    L22 = sla.cholesky(stored[npos:, npos:] + Wm @ Wm.T, lower=True)
    Lref = np.block([[L11, np.zeros((npos, nneg))], [Wm, L22]])
    ops, extent = plan(n, n - 1, npos=npos)
    assert extent == n - 1
    executed_factor(ops, stored, extent, M, np.where(np.arange(n) < npos, 1.0, -1.0), Lref)


def check_ranges(n, bw, ops, extent):
    """Every tile of the band receives every k it needs exactly once, before its column is factored."""
    nblk = (n + NB - 1) // NB
    up = lambda v: (v + NB - 1) // NB * NB
    applied = {}  # tile (I, J) -> k-ranges in the order applied
    done = 0
    seen_extent = 0
    for kind, row0, rows, k0, kend, width, sign in ops:
        assert row0 % NB == 0 and 0 <= rows and row0 + rows <= n and width >= 1 and sign == -1
        assert rows % NB == 0 or row0 + (width if kind == BLOCK else 0) + rows == n, "whole tiles, or clamped at n"
        if kind == UPDATE:
            assert k0 < kend == row0 <= done and k0 % NB == 0 and k0 >= max(0, (row0 - bw) // NB * NB)
            assert rows <= up(width + bw) and (rows >= width + bw or row0 + rows == n)
            assert row0 + width <= n
            seen_extent = max(seen_extent, row0 + rows - 1 - k0)
            for J in range(row0 // NB, (row0 + width - 1) // NB + 1):
                for I in range(J, (row0 + rows - 1) // NB + 1):
                    applied.setdefault((I, J), []).append((k0, kend))
        else:
            jb, w = row0, width
            assert jb == done and w <= NB and (w == NB or jb + w == n)
            assert rows <= up(bw) and (rows >= bw or jb + w + rows == n)
            seen_extent = max(seen_extent, w + rows - 1)
            J = jb // NB
            need0 = max(0, (jb - bw) // NB * NB)
            for I in range(J, nblk):
                r = applied.get((I, J), [])
                for a, b in zip(r, r[1:]):
                    assert a[1] <= b[0], ("k-ranges in ascending order, no k twice", I, J, r)
                in_band = I * NB - (jb + w - 1) <= bw
                if in_band and jb > 0 and need0 < jb:
                    # the k the band reaches from this column, [need0, jb): none skipped (a k further left may be: the
                    # columns of a wider update that need it lie to the left of this tile)
                    rr = [x for x in r if x[1] > need0]
                    assert rr and rr[0][0] <= need0 and rr[-1][1] == jb, (I, J, r, need0)
                    for a, b in zip(rr, rr[1:]):
                        assert a[1] == b[0], ("no k of the band skipped", I, J, r)
                if in_band and I > J:
                    assert I * NB < jb + w + rows, "the panel solve reaches every tile of the band"
            done += w
    assert done == n and seen_extent == extent
    assert min(bw, n - 1) <= extent <= n - 1


@pytest.mark.parametrize("n,bw", SHAPES + RANGE_ONLY)
def test_ranges_cover_the_band_once(n, bw):
    ops, extent = plan(n, bw)
    check_ranges(n, bw, ops, extent)
    for wt in (6, 10, 20):  # the widths of the measured record (MADQP_CHOL_BAND_W)
        ops, extent = plan(n, bw, force_wt=wt)
        check_ranges(n, bw, ops, extent)


def halving(n, j0, w, ops):
    """The recursive halving of the columns [j0, j0 + w) of a dense matrix of order n: the first half in whole blocks, the
    larger half first, one update of the second half with it."""
    if w <= NB:
        ops.append((BLOCK, j0, n - j0 - w, 0, 0, w, -1))
        return
    h = ((w + NB - 1) // NB + 1) // 2 * NB
    halving(n, j0, h, ops)
    ops.append((UPDATE, j0 + h, n - j0 - h, j0, j0 + h, w - h, -1))
    halving(n, j0 + h, w - h, ops)


def dense_schedule(n, slots=SLOTS):
    """What the dense left-looking schedule has to be, written down independently of chol_plan.inc: outer panels of the
    library's width rule, each updated with all columns to its left and then halved."""
    lib = band_lib()
    ops = []
    J0 = 0
    while J0 < n:
        W = min(lib.band_dense_outer_width(n - J0, 1 if J0 > 0 else 0, slots), n - J0)
        if J0 > 0:
            ops.append((UPDATE, J0, n - J0, 0, J0, W, -1))
        halving(n, J0, W, ops)
        J0 += W
    return np.array(ops, dtype=np.int64)


@pytest.mark.parametrize("n", NS + (13400, 30000))
def test_full_bandwidth_is_the_dense_schedule(n):
    ops, extent = plan(n, n - 1)
    assert extent == n - 1
    assert np.array_equal(ops, dense_schedule(n))


def quasidefinite_schedule(npos, nneg, slots=SLOTS):
    """What the schedule under a signature has to be: an outer panel never straddles npos; one that starts in [1, npos)
    receives the columns [0, J0); one at or beyond npos receives +[0, npos) (npos > 0) and then -[npos, J0) (J0 > npos)."""
    lib = band_lib()
    n = npos + nneg
    ops = []
    J0 = 0
    while J0 < n:
        W = min(lib.band_dense_outer_width(n - J0, 1 if J0 > 0 else 0, slots), n - J0)
        if J0 < npos < J0 + W:
            W = npos - J0
        if 0 < J0 < npos:
            ops.append((UPDATE, J0, n - J0, 0, J0, W, -1))
        elif J0 > 0:
            if npos > 0:
                ops.append((UPDATE, J0, n - J0, 0, npos, W, +1))
            if J0 > npos:
                ops.append((UPDATE, J0, n - J0, npos, J0, W, -1))
        halving(n, J0, W, ops)
        J0 += W
    return np.array(ops, dtype=np.int64)


@pytest.mark.parametrize("npos,nneg", SIGNATURES)
def test_signature_plan_is_the_quasidefinite_schedule(npos, nneg):
    n = npos + nneg
    ops, extent = plan(n, n - 1, npos=npos)
    assert extent == n - 1
    expected = quasidefinite_schedule(npos, nneg)
    assert np.array_equal(ops, expected)
    if (npos, nneg) in ((128, 2561), (1280, 2900)):  # the shapes chosen for it: a panel with both updates
        plus = expected[(expected[:, 0] == UPDATE) & (expected[:, 6] == 1)]
        assert any(np.any((expected[:, 0] == UPDATE) & (expected[:, 6] == -1) & (expected[:, 1] == r) & (expected[:, 4] == r)
                          & (expected[:, 3] == npos)) for r in plus[:, 1])


@pytest.mark.parametrize("n,j0,w", RANGES)
def test_range_plan_is_the_halving(n, j0, w):
    expected = []
    halving(n, j0, w, expected)
    assert np.array_equal(range_plan(n, j0, w), np.array(expected, dtype=np.int64))


def test_narrow_band_panels():
    """(2100, 200): three outer panels, the third starts its k range at 1280 -- below it a wrong k0 would not show."""
    ops, _ = plan(2100, 200)
    outer = [tuple(o) for o in ops if o[0] == UPDATE and o[1] in (768, 1536) and o[5] > 384]
    assert outer == [(UPDATE, 768, 1024, 512, 768, 768, -1), (UPDATE, 1536, 564, 1280, 1536, 564, -1)]
    ops, extent = plan(1600, 80)  # boundary_control_qp(40), normal equations
    assert [tuple(o[1:]) for o in ops if o[0] == UPDATE and o[5] > 384] == [(768, 832, 640, 768, 768, -1)]
    assert sum(1 for o in ops if o[0] == BLOCK) == 13


# ---- pattern_bandwidth ------------------------------------------------------------------------------------------------
def device_csr(A):
    A = sp.coo_matrix(A)
    return M.DeviceCSR(CPU, A.shape[0], A.shape[1], A.row, A.col, A.data)


@pytest.mark.parametrize("N,normal,condensed", [(12, 24, 170), (25, 50, 677)])
def test_pattern_bandwidth_of_boundary_control(N, normal, condensed):
    qp = P.boundary_control_qp(N)
    csr = device_csr(qp.A)
    hd = torch.as_tensor(qp.H.diagonal())
    assert pattern_bandwidth(csr, hd, "normal") == dense_pattern_bandwidth(qp.A, None, "normal") == normal
    assert pattern_bandwidth(csr, hd, "condensed") == dense_pattern_bandwidth(qp.A, qp.H, "condensed") == condensed
    hs = M.DeviceSymCSR.from_dense(CPU, qp.H.toarray())
    assert pattern_bandwidth(csr, hs, "condensed") == condensed


def test_pattern_bandwidth_of_banded_and_empty_matrices():
    for nx, m, abw, seed in ((60, 25, 4, 1), (200, 90, 11, 2), (33, 1, 7, 3)):
        q = banded_qp(nx, m, abw, seed)
        csr, hs = device_csr(q["A"]), M.DeviceSymCSR.from_dense(CPU, q["H"].toarray())
        for form in ("condensed", "normal"):
            H = q["H"] if form == "condensed" else None
            assert pattern_bandwidth(csr, hs if form == "condensed" else None, form) == dense_pattern_bandwidth(q["A"], H, form)
        assert pattern_bandwidth(csr, None, "condensed") == abw
    # H wider than A' A decides; an empty A and an empty H give 0
    H = np.eye(20)
    H[17, 2] = H[2, 17] = 0.5
    empty = device_csr(sp.csr_matrix((5, 20)))
    assert pattern_bandwidth(empty, M.DeviceSymCSR.from_dense(CPU, H), "condensed") == 15
    assert pattern_bandwidth(empty, None, "condensed") == pattern_bandwidth(empty, None, "normal") == 0
    assert pattern_bandwidth(empty, M.DeviceSymCSR.from_dense(CPU, np.zeros((20, 20))), "condensed") == 0
    with pytest.raises(ValueError):
        pattern_bandwidth(empty, None, "augmented")


# ---- refusals, before any device call -----------------------------------------------------------------------------------
def small_qp(sparse=True, hessian="csr"):
    q = banded_qp(12, 5, 3, 7)
    Hd = q["H"].toarray()
    dq = M.DeviceQP.from_numpy(CPU, Hd if hessian == "dense" else None, q["q"], q["A"].toarray(), q["lvar"], q["uvar"],
                               q["lcon"], q["ucon"], q["x0"], sparse=sparse)
    if hessian == "csr":
        dq.H = M.DeviceSymCSR.from_dense(CPU, Hd)
    return dq


@pytest.mark.parametrize("bw", ["auto", 5])
@pytest.mark.parametrize("kw,msg", [
    (dict(dense_A=True, hessian="dense"), "needs the sparse front end"),
    (dict(hessian="dense"), "not a dense one"),
    (dict(kkt_system="augmented"), "augmented"),
    (dict(kkt_system="scaled_augmented", hessian="none"), "augmented"),
    (dict(grid=True), "DistributedQP"),
])
def test_solver_refuses_a_bandwidth_it_cannot_use(kw, msg, bw):
    kw = dict(kw)
    dq = small_qp(sparse=not kw.pop("dense_A", False), hessian=kw.pop("hessian", "csr"))
    if kw.pop("grid", False):
        dq.grid = object()
    with pytest.raises(ValueError, match=msg):
        M.MPCSolver(dq, types.SimpleNamespace(device="cpu"), kkt_bandwidth=bw, **kw)


@pytest.mark.parametrize("bw", [-1, "wide", 2.5, True])
def test_solver_refuses_a_malformed_bandwidth(bw):
    with pytest.raises(ValueError, match="kkt_bandwidth"):
        M.MPCSolver(small_qp(), types.SimpleNamespace(device="cpu"), kkt_bandwidth=bw)


def test_batched_solver_refuses_a_bandwidth():
    dq = small_qp(sparse=False, hessian="dense")
    with pytest.raises(ValueError, match="kkt_bandwidth"):
        M.BatchedMPCSolver([dq], types.SimpleNamespace(device=CPU), kkt_bandwidth="auto")


def test_default_is_no_bandwidth():
    assert M.IPMOptions().kkt_bandwidth is None


# ---- the plan under the sanitizers ----------------------------------------------------------------------------------------
def test_plan_under_address_and_undefined_sanitizers():
    """tests/csrc_band/band_plan_main.cpp: a stand-alone program (never loaded into Python) that plans the shapes above --
    band, signature and range."""
    band_lib()  # (runs make)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "band_plan_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAD" not in out.stdout and out.stdout.count(" ok") >= len(SHAPES) + len(RANGE_ONLY) + len(SIGNATURES) + len(RANGES)
