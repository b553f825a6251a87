"""CPU: the schedule of the band-limited Cholesky (madqp_jl_amd/csrc/band_plan.inc, compiled for the CPU by
tests/csrc_band).  The plan is executed in numpy float64 on band matrices and held to scipy; its ranges are checked against
the band, the extent it reports and the dense schedule; ``kkt.pattern_bandwidth`` is held to dense numpy; the refusals of
``kkt_bandwidth`` happen before any device call.  The kernels that run the plan are held in tests/test_gpu_band.py."""
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
from band_cases import (BLOCK, NB, ROOT, SLOTS, UPDATE, band_spd, banded_qp, band_lib, dense_pattern_bandwidth, plan)

CPU = torch.device("cpu")
NS = (1, 128, 129, 500, 1537, 2100)
SHAPES = [(n, bw) for n in NS for bw in sorted({0, 1, 127, 128, 129, 300, 640, n - 1}) if bw < n]
RANGE_ONLY = [(90000, 600), (22500, 300)]


def execute(ops, K, extent):
    """The operations on a copy of K (lower triangle; NaN above the diagonal and beyond the extent)."""
    n = K.shape[0]
    i, j = np.indices((n, n))
    W = np.where((i >= j) & (i - j <= extent), K, np.nan)
    for kind, row0, rows, k0, kend, width in ops:
        if kind == UPDATE:
            X = W[row0: row0 + rows, k0: kend]
            Y = W[row0: row0 + width, k0: kend]
            low = i[row0: row0 + rows, row0: row0 + width] >= j[row0: row0 + rows, row0: row0 + width]
            C = W[row0: row0 + rows, row0: row0 + width]
            C[low] -= (X @ Y.T)[low]
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
    W = execute(ops, K, extent)
    i, j = np.indices((n, n))
    outside = (i < j) | (i - j > extent)
    assert np.all(np.isnan(W[outside])), "nothing beyond the extent (or above the diagonal) is written"
    assert not np.any(np.isnan(W[~outside])), "nothing beyond the extent is read"
    L = np.where(outside, 0.0, W)
    Lref = sla.cholesky(K, lower=True)
    rel = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
    assert rel < 1e-14 * max(1, math.sqrt(n)), rel
    assert np.max(np.abs(L - Lref)) / np.max(np.abs(Lref)) < 1e-11
    assert np.all(L[i - j > bw] == 0.0), "the factor stays inside the band: stored zeros stay zeros"


def check_ranges(n, bw, ops, extent):
    """Every tile of the band receives every k it needs exactly once, before its column is factored."""
    nblk = (n + NB - 1) // NB
    up = lambda v: (v + NB - 1) // NB * NB
    applied = {}  # tile (I, J) -> k-ranges in the order applied
    done = 0
    seen_extent = 0
    for kind, row0, rows, k0, kend, width in ops:
        assert row0 % NB == 0 and 0 <= rows and row0 + rows <= n and width >= 1
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


def dense_schedule(n, slots=SLOTS):
    """chol_factor_enqueue's left-looking schedule and factor_range's halving, as operations."""
    lib = band_lib()
    ops = []

    def rng(j0, w):
        if w <= NB:
            ops.append((BLOCK, j0, n - j0 - w, 0, 0, w))
            return
        h = ((w + NB - 1) // NB + 1) // 2 * NB
        rng(j0, h)
        ops.append((UPDATE, j0 + h, n - j0 - h, j0, j0 + h, w - h))
        rng(j0 + h, w - h)

    J0 = 0
    while J0 < n:
        W = min(lib.band_dense_outer_width(n - J0, 1 if J0 > 0 else 0, slots), n - J0)
        if J0 > 0:
            ops.append((UPDATE, J0, n - J0, 0, J0, W))
        rng(J0, W)
        J0 += W
    return np.array(ops, dtype=np.int64)


@pytest.mark.parametrize("n", NS + (13400, 30000))
def test_full_bandwidth_is_the_dense_schedule(n):
    ops, extent = plan(n, n - 1)
    assert extent == n - 1
    assert np.array_equal(ops, dense_schedule(n))


def test_narrow_band_panels():
    """(2100, 200): three outer panels, the third starts its k range at 1280 -- below it a wrong k0 would not show."""
    ops, _ = plan(2100, 200)
    outer = [tuple(o) for o in ops if o[0] == UPDATE and o[1] in (768, 1536) and o[5] > 384]
    assert outer == [(UPDATE, 768, 1024, 512, 768, 768), (UPDATE, 1536, 564, 1280, 1536, 564)]
    ops, extent = plan(1600, 80)  # boundary_control_qp(40), normal equations
    assert [tuple(o[1:]) for o in ops if o[0] == UPDATE and o[5] > 384] == [(768, 832, 640, 768, 768)]
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
    """tests/csrc_band/band_plan_main.cpp: a stand-alone program (never loaded into Python) that plans the shapes above."""
    band_lib()  # (runs make)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "band_plan_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAD" not in out.stdout and out.stdout.count(" ok") >= len(SHAPES) + len(RANGE_ONLY)
