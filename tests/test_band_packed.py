"""CPU: packed band storage for the band Cholesky (madqp_jl_amd/csrc/band_plan.inc: band_packed_layout; compiled for the
CPU by tests/csrc_band).  Entry (i, j) of the lower triangle lives at P[i + j ld], ld >= extent.  The plan of the
factorisation and the job lists of the sweeps are executed in numpy THROUGH that addressing, on buffers that hold NaN in
every slot that is no band entry within the extent: a store outside the band lands on another column's entry or on a
planted NaN, a read outside it brings a NaN into the band.  The layout arithmetic, LAPACK's band format and the refusals
of ``kkt_storage`` need no device either.  The kernels that run on the storage are held in tests/test_gpu_band_packed.py."""
import functools
import math
import os
import subprocess
import types

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import madqp_jl_amd as M
from band_cases import (ROOT, UPDATE, band_index, band_lib, band_spd, banded_qp, layout, lds_to_test, nan_kept, npad, pack,
                        plan, unpack, view)
from test_band_sweep_plan import run_sweep

CPU = torch.device("cpu")
NS = (129, 500, 1537, 2100)
SHAPES = [(n, bw) for n in NS for bw in sorted({0, 1, 127, 128, 129, 300, 640, n - 1}) if bw < n]
LARGE = [(90000, 600), (202500, 900)]


@functools.lru_cache(maxsize=2)
def reference(n, bw):
    """(K, its scipy factor, a right-hand side, cho_solve): computed once per shape, read-only"""
    K = band_spd(n, bw)
    L = sla.cholesky(K, lower=True, check_finite=False)
    b = np.random.default_rng(n + bw).standard_normal(n)
    x = sla.cho_solve((L, True), b, check_finite=False)
    for a in (K, L, b, x):
        a.setflags(write=False)
    return K, L, b, x


def execute(ops, W):
    """The operations of the plan in place on W, the packed buffer seen as a column-major matrix: what
    tests/test_band_plan.py does on a dense copy, with the same masks on every store."""
    for kind, row0, rows, k0, kend, width, _ in ops:  # (a band's updates all subtract)
        if kind == UPDATE:
            X = W[row0: row0 + rows, k0: kend]
            Y = W[row0: row0 + width, k0: kend]
            gi, gj = np.indices((rows, width))
            low = gi >= gj
            C = W[row0: row0 + rows, row0: row0 + width]
            C[low] = C[low] - (X @ Y.T)[low]
        else:
            jb, w = row0, width
            D = np.tril(W[jb: jb + w, jb: jb + w])
            L = np.linalg.cholesky(D + np.tril(D, -1).T)
            W[jb: jb + w, jb: jb + w][np.tril_indices(w)] = L[np.tril_indices(w)]
            if rows:
                X = W[jb + w: jb + w + rows, jb: jb + w]
                X[:] = sla.solve_triangular(L, X.T, lower=True).T


@pytest.mark.parametrize("n,bw", SHAPES)
def test_executed_plan_factors_the_packed_band(n, bw):
    K, Lref, _, _ = reference(n, bw)
    ops, extent = plan(n, bw)
    for ld in lds_to_test(n, extent):
        ld, doubles = layout(n, extent, ld)
        buf, addr = pack(K, extent, ld, doubles)
        execute(ops, view(buf, n, ld))
        assert nan_kept(buf, addr), (ld, "a store outside the band: a planted NaN is gone")
        assert not np.any(np.isnan(buf[addr])), (ld, "a read outside the band: NaN inside it")
        L = unpack(buf, n, extent, ld)
        rel = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
        assert rel < 1e-14 * max(1, math.sqrt(n)), (ld, rel)
        assert np.max(np.abs(L - Lref)) / np.max(np.abs(Lref)) < 1e-11, ld
        i, j = np.indices((n, n))
        assert np.all(L[i - j > bw] == 0.0), "the factor stays inside the band: stored zeros stay zeros"


@pytest.mark.parametrize("n,bw", SHAPES)
def test_executed_sweeps_on_the_packed_factor(n, bw):
    _, Lref, b, xref = reference(n, bw)
    extent = plan(n, bw)[1]
    kb = band_lib().band_sweep_blocks_c(bw)
    for ld in lds_to_test(n, extent):
        ld, doubles = layout(n, extent, ld)
        buf, addr = pack(Lref, extent, ld, doubles)
        W = view(buf, n, ld)
        for chunk in (1, 64):
            y = run_sweep(W, b, n, kb, chunk, backward=False)
            x = run_sweep(W, y, n, kb, chunk, backward=True)
            assert not np.any(np.isnan(y)) and not np.any(np.isnan(x)), (ld, "a read outside the band")
            assert np.linalg.norm(x - xref) / np.linalg.norm(xref) < 1e-10, (ld, chunk)
        assert nan_kept(buf, addr)


# ---- the layout arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bw", SHAPES)
def test_no_two_band_entries_share_an_address(n, bw):
    extent = plan(n, bw)[1]
    for ld in lds_to_test(n, extent):
        ld, doubles = layout(n, extent, ld)
        i, j = band_index(n, extent)
        addr = i + j * ld
        assert len(addr) == sum(min(extent + 1, n - c) for c in range(n))
        assert len(np.unique(addr)) == len(addr) and addr.min() == 0
        assert doubles == npad(n) * (ld + 1) + 128
        # the highest address a whole-tile read reaches: row and column up to the padded order
        assert (npad(n) - 1) * (ld + 1) + 2 <= doubles


@pytest.mark.parametrize("n,bw", SHAPES + LARGE)
def test_the_librarys_leading_dimension_and_size(n, bw):
    extent = plan(n, bw)[1]
    ld, doubles = layout(n, extent)
    pad = band_lib().band_packed_default_pad_c()
    assert ld % 2 == 0 and ld >= extent + 1 and ld == (extent + 1 + 15) // 16 * 16 + pad
    assert doubles == npad(n) * (ld + 1) + 128
    assert (npad(n) - 1) * (ld + 1) + 2 <= doubles, "whole-tile reads up to the padded order stay inside"
    if (n, bw) == (90000, 600):
        assert extent == 2047 and doubles * 8 < 1.6e9  # ~1.5 GB where the dense K has 65 GB
    if (n, bw) == (202500, 900):
        assert doubles * 8 < 8e9 and 8 * npad(n) ** 2 > 288e9  # the dense K exceeds one device's memory


def test_a_leading_dimension_below_the_extent_is_refused():
    for n, bw in ((2100, 640), (1537, 129), (500, 127)):
        extent = plan(n, bw)[1]
        assert extent > 1 and layout(n, extent, extent - 1) is None and layout(n, extent, 1) is None
        assert layout(n, extent, extent) == (extent, npad(n) * (extent + 1) + 128)
    assert layout(1, 0, 0)[0] >= 1 and layout(1, 0, 1) == (1, 128 * 2 + 128)


# ---- LAPACK's lower band storage ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bw", [(129, 1), (500, 127), (1537, 129), (2100, 200)])
def test_packed_storage_is_lapacks_lower_band_format(n, bw):
    """P seen with LDAB = ld + 1 is the `ab` array of scipy.linalg.cholesky_banded(lower=True): ab[i - j, j] = a[i, j]."""
    K, Lref, _, _ = reference(n, bw)
    extent = plan(n, bw)[1]
    for ld in lds_to_test(n, extent):
        ld, doubles = layout(n, extent, ld)
        buf, _ = pack(K, extent, ld, doubles)
        ab = np.lib.stride_tricks.as_strided(buf, shape=(bw + 1, n), strides=(8, 8 * (ld + 1)))
        want = np.zeros((bw + 1, n))
        for d in range(bw + 1):
            want[d, : n - d] = np.diagonal(K, -d)
        ours = np.array(ab)
        for d in range(1, bw + 1):
            ours[d, n - d:] = 0.0  # (LAPACK does not look at the corner beyond the matrix)
        assert np.array_equal(ours, want)
        c = sla.cholesky_banded(ours, lower=True, check_finite=False)
        fac, _ = pack(Lref, extent, ld, doubles)
        fb = np.array(np.lib.stride_tricks.as_strided(fac, shape=(bw + 1, n), strides=(8, 8 * (ld + 1))))
        for d in range(1, bw + 1):
            fb[d, n - d:] = c[d, n - d:]
        assert np.max(np.abs(fb - c)) / np.max(np.abs(c)) < 1e-11


# ---- the walk under the sanitizers --------------------------------------------------------------------------------------------
def test_packed_walk_under_address_and_undefined_sanitizers():
    """tests/csrc_band/band_packed_main.cpp: a stand-alone program (never loaded into Python) that makes every
    store and every whole-tile read of the plan and the sweeps on a buffer of exactly the reported size."""
    band_lib()  # (runs make)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "band_packed_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAD" not in out.stdout and out.stdout.count(" ok") >= 4 * len(SHAPES) + len(LARGE)


# ---- refusals, before any device call -----------------------------------------------------------------------------------
def small_qp(sparse=True, hessian="csr"):
    q = banded_qp(12, 5, 3, 7)
    Hd = q["H"].toarray()
    dq = M.DeviceQP.from_numpy(CPU, Hd if hessian == "dense" else None, q["q"], q["A"].toarray(), q["lvar"], q["uvar"],
                               q["lcon"], q["ucon"], q["x0"], sparse=sparse)
    if hessian == "csr":
        dq.H = M.DeviceSymCSR.from_dense(CPU, Hd)
    return dq


NO_DEVICE = types.SimpleNamespace(device="cpu")


def test_default_storage_is_dense():
    assert M.IPMOptions().kkt_storage == "dense"


def test_packed_storage_needs_a_bandwidth():
    with pytest.raises(ValueError, match="kkt_storage='packed' needs kkt_bandwidth"):
        M.MPCSolver(small_qp(), NO_DEVICE, kkt_storage="packed")


@pytest.mark.parametrize("storage", ["band", "", None, 1])
def test_solver_refuses_an_unknown_storage(storage):
    with pytest.raises(ValueError, match="kkt_storage"):
        M.MPCSolver(small_qp(), NO_DEVICE, kkt_storage=storage, kkt_bandwidth=5)


@pytest.mark.parametrize("kw,msg", [
    (dict(dense_A=True, hessian="dense"), "needs the sparse front end"),
    (dict(hessian="dense"), "not a dense one"),
    (dict(kkt_system="augmented"), "augmented"),
    (dict(grid=True), "DistributedQP"),
])
def test_packed_storage_is_refused_where_the_bandwidth_is(kw, msg):
    kw = dict(kw)
    dq = small_qp(sparse=not kw.pop("dense_A", False), hessian=kw.pop("hessian", "csr"))
    if kw.pop("grid", False):
        dq.grid = object()
    with pytest.raises(ValueError, match=msg):
        M.MPCSolver(dq, NO_DEVICE, kkt_bandwidth="auto", kkt_storage="packed", **kw)


def test_batched_solver_refuses_packed_storage():
    dq = small_qp(sparse=False, hessian="dense")
    with pytest.raises(ValueError, match="kkt_storage"):
        M.BatchedMPCSolver([dq], types.SimpleNamespace(device=CPU), kkt_storage="packed")
    with pytest.raises(ValueError, match="kkt_bandwidth"):
        M.BatchedMPCSolver([dq], types.SimpleNamespace(device=CPU), kkt_storage="packed", kkt_bandwidth=3)


def test_kkt_classes_refuse_packed_storage_without_a_bandwidth():
    """storage= at construction: refused before the backend is touched (None stands in for it)"""
    from madqp_jl_amd.kkt import HIPSparseCondensedKKTSystem, HIPSparseNormalKKTSystem, check_storage

    for cls in (HIPSparseCondensedKKTSystem, HIPSparseNormalKKTSystem):
        with pytest.raises(ValueError, match="needs a bandwidth"):
            cls(None, None, 4, [], None, None, storage="packed")
        with pytest.raises(ValueError, match="storage: one of"):
            cls(None, None, 4, [], None, None, bandwidth=2, storage="sparse")
    with pytest.raises(ValueError, match="not a dense one"):
        check_storage("packed", 3, "condensed", torch.zeros((4, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="condensed and normal"):
        check_storage("packed", 3, None)
    check_storage("dense", None)
    check_storage("packed", "auto", "normal", torch.zeros(4, dtype=torch.float64))
