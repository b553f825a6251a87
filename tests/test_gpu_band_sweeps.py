"""GPU: the triangular sweeps of ``madqp_chol_solve`` under a bandwidth (chol.hip, band form of trsv_*_sweep_kernel;
``MADQP_SWEEP_BAND``, ``madqp_chol_sweep_info``).  With a bandwidth set a solve reads nothing beyond the extent of the
factorisation: the storage holds NaN there, the solution meets the bars of tests/test_gpu_band.py::test_band_solve and every
NaN is still that NaN afterwards.  tests/test_band_sweep_plan.py holds the job lists themselves."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
from band_cases import workgroups
from test_gpu_band import FACTOR_SHAPES, assembly_cases, bits, dev, leading_dimension, reference, whole_matrix

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def environment(**kw):
    """the switches a handle reads in madqp_chol_create, set around the call and restored"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def create(hip, n, **env):
    with environment(**env):
        return hip.chol_create(n)


def planted(n, bw, lda, extent):
    """The storage of tests/test_gpu_band.py::test_band_factor: NaN above the diagonal, beyond the extent and in the rows past
    n; zeros for bw < i - j <= extent."""
    K, _ = reference(n, bw)
    i, j = np.indices((n, n))
    stored = np.where(i - j > bw, 0.0, K)
    stored[(i < j) | (i - j > extent)] = np.nan
    host = np.full((n, lda), np.nan)
    host[:, :n] = stored.T
    return host


def rhs(n, bw):
    return np.random.default_rng(n + bw).standard_normal(n)


def bars(n, bw, x, tag):
    import scipy.linalg as sla
    K, Lref = reference(n, bw)
    b = rhs(n, bw)
    xref = sla.cho_solve((Lref, True), b)
    assert not np.any(np.isnan(x)), f"{tag}: a NaN beyond the extent reached the solution"
    res = np.linalg.norm(K @ x - b) / (np.linalg.norm(K) * np.linalg.norm(x))
    err = np.linalg.norm(x - xref) / np.linalg.norm(xref)
    print(f"{tag}: residual {res:.2e}, distance to scipy {err:.2e}")
    assert res < 1e-14, res
    assert err < 1e-10, err


def factor_and_solve(hip, h, host, lda, n, bw):
    Kd, bd = dev(host, hip), dev(rhs(n, bw), hip)
    assert hip.chol_factor(h, Kd, lda) == 0
    hip.chol_solve(h, bd)
    return Kd.cpu().numpy(), bd.cpu().numpy()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,bw", FACTOR_SHAPES)
def test_solve_reads_nothing_beyond_the_extent(hip, n, bw, padded):
    lda = leading_dimension(n, padded)
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        extent = hip.chol_band_extent(h)
        kb = (bw + 127) // 128
        assert hip.chol_sweep_info(h) == (kb, (n + 127) // 128, 64)
        assert min(n - 1, kb * 128 + 127) <= extent
        host = planted(n, bw, lda, extent)
        out, x = factor_and_solve(hip, h, host, lda, n, bw)
        bars(n, bw, x, f"n={n} bw={bw} extent={extent} lda={lda}")
        was_nan = np.isnan(host)
        assert np.array_equal(bits(out[was_nan]), bits(host[was_nan])), "every NaN is still that NaN"
    finally:
        hip.chol_destroy(h)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,bw", FACTOR_SHAPES)
def test_switch_off_is_the_dense_sweep_bit_for_bit(hip, n, bw, padded):
    """One job per block row at these n: the tiles the band form skips are stored zeros, which the dense sweep adds as
    fma(0, x, a) = a in the same place of the same sum."""
    K, _ = reference(n, bw)
    lda = leading_dimension(n, padded)
    host = np.zeros((n, lda))
    host[:, :n] = K.T
    res = []
    for env in (None, "0"):
        h = create(hip, n, MADQP_SWEEP_BAND=env)
        try:
            hip.chol_set_bandwidth(h, bw)
            info = hip.chol_sweep_info(h)
            assert info == (((bw + 127) // 128 if env is None else -1), (n + 127) // 128, 64)
            res.append(factor_and_solve(hip, h, host, lda, n, bw))
        finally:
            hip.chol_destroy(h)
    assert np.array_equal(bits(res[0][0]), bits(res[1][0])), "the factors"
    assert np.array_equal(bits(res[0][1]), bits(res[1][1])), "the solutions"
    bars(n, bw, res[0][1], f"n={n} bw={bw} lda={lda}")


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,bw,chunk", [(1537, 300, 1), (1537, 300, 2), (2100, 640, 2), (2100, 640, 4)])
def test_split_block_rows_under_a_band(hip, n, bw, chunk, padded):
    """kb = 3 and 5 blocks with chunks of 1, 2 and 4 tiles: several jobs per block row, and in the later rows the first
    chunks are no jobs -- the owner must not wait for them."""
    lda = leading_dimension(n, padded)
    kb = (bw + 127) // 128
    xs = []
    for ch in (chunk, None):
        h = create(hip, n, MADQP_SWEEP_CHUNK=ch)
        try:
            dense_wg = hip.chol_sweep_info(h)[1]
            hip.chol_set_bandwidth(h, bw)
            extent = hip.chol_band_extent(h)
            info = hip.chol_sweep_info(h)
            assert info == (kb, workgroups(n, kb, ch or 64), ch or 64)
            if ch is not None:
                assert dense_wg == workgroups(n, -1, ch) and (n + 127) // 128 < info[1] < dense_wg
            host = planted(n, bw, lda, extent)
            out, x = factor_and_solve(hip, h, host, lda, n, bw)
            bars(n, bw, x, f"n={n} bw={bw} chunk={ch} workgroups={info[1]}")
            was_nan = np.isnan(host)
            assert np.array_equal(bits(out[was_nan]), bits(host[was_nan])), "every NaN is still that NaN"
            xs.append(x)
        finally:
            hip.chol_destroy(h)
    assert np.linalg.norm(xs[0] - xs[1]) / np.linalg.norm(xs[1]) < 1e-12


CASES = [c for c in assembly_cases() if c[0] in ("condensed-hcsr", "normal-bc25")]


@pytest.mark.parametrize("name,form,make,reg", CASES, ids=lambda c: c if isinstance(c, str) else "")
def test_kkt_solve_reads_nothing_beyond_the_extent(hip, name, form, make, reg):
    s = M.MPCSolver(make(hip), hip, kkt_system=form, regularization=reg)
    try:
        s.initialize()
        s.kkt.set_aug_diagonal_reg(1.0, -1e-8 if form == "condensed" else 0.0)
        order = s.m if form == "normal" else s.nx
        bw = s.kkt.set_bandwidth("auto")
        ch = hip.kkt_chol(s.kkt._h)[0]
        extent = hip.chol_band_extent(ch)
        kb = (bw + 127) // 128
        reach = min(order - 1, kb * 128 + 127)
        assert (order, bw) in ((300, 6), (625, 50)) and reach == 255 <= extent
        assert s.kkt.linear_solver.sweep_band_blocks == hip.chol_sweep_info(ch)[0] == kb
        s.kkt.build_kkt()
        s.kkt.factorize_wrapper()
        assert s.kkt.linear_solver.is_factorized()
        b = np.random.default_rng(3).standard_normal(s.st.ntot)

        def solve():
            s.st.d.copy_(torch.as_tensor(b))
            s.kkt.solve(s.st.d)
            return s.st.d.cpu().numpy().copy()

        x = solve()
        assert not np.any(np.isnan(x))
        ptr, ld = hip.kkt_matrix(s.kkt._h, order)
        # i - j = extent + 1 where the triangle has such an entry.  At order 300 the plan's extent is the whole triangle
        # (299) and nothing lies beyond it: there the NaN goes just beyond the sweeps' own reach, 255 <= extent, which
        # asks more of the solve, not less.
        jn = 1
        in_ = jn + (extent if extent < order - 1 else reach) + 1
        print(f"{name}: order {order}, bw {bw}, extent {extent}, reach {reach}, NaN at i - j = {in_ - jn}")
        assert in_ < order and in_ - jn > reach
        nan = np.array([np.nan])
        hip._ck(hip.lib.madqp_memcpy_h2d(hip.ctx, C.c_void_p(ptr + 8 * (in_ + jn * ld)), nan.ctypes.data, 8))
        assert np.isnan(whole_matrix(hip, s.kkt, order)[in_, jn])
        assert np.array_equal(bits(solve()), bits(x)), "the solve does not look beyond the extent"
    finally:
        s.close()


def test_sweep_info_refusals_and_clearing(hip):
    lib, ERR_ARG, ERR_STATE = hip.lib, -1, -4
    n, bw = 500, 127
    K, _ = reference(n, bw)
    lda = leading_dimension(n, True)
    host = np.zeros((n, lda))
    host[:, :n] = K.T
    out = (C.c_int64 * 3)()
    h, fresh = hip.chol_create(n), hip.chol_create(n)
    try:
        assert lib.madqp_chol_sweep_info(None, out) == ERR_ARG and lib.madqp_chol_sweep_info(h, None) == ERR_ARG
        assert hip.chol_sweep_info(h) == (-1, 4, 64)
        hip.chol_set_bandwidth(h, bw)
        assert hip.chol_sweep_info(h) == (1, 4, 64)
        _, xb = factor_and_solve(hip, h, host, lda, n, bw)
        hip.chol_set_bandwidth(h, -1)
        assert hip.chol_sweep_info(h) == (-1, 4, 64)
        # the stored factor belongs to the other form of the sweeps: no solve before the next factorisation
        bd = dev(rhs(n, bw), hip)
        assert lib.madqp_chol_solve(h, M._lib.ptr(bd)) == ERR_STATE
        hip.chol_set_bandwidth(h, bw)
        assert lib.madqp_chol_solve(h, M._lib.ptr(bd)) == ERR_STATE
        assert np.array_equal(bits(bd.cpu().numpy()), bits(rhs(n, bw))), "a refused solve leaves the right-hand side alone"
        hip.chol_set_bandwidth(h, -1)
        res = [factor_and_solve(hip, k, host, lda, n, bw) for k in (h, fresh)]
        assert np.array_equal(bits(res[0][0]), bits(res[1][0])) and np.array_equal(bits(res[0][1]), bits(res[1][1]))
        bars(n, bw, xb, "band")
        bars(n, bw, res[0][1], "cleared")
    finally:
        hip.chol_destroy(h)
        hip.chol_destroy(fresh)
