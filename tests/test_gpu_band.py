"""GPU: the band-limited Cholesky schedule (``madqp_chol_set_bandwidth``) and the band-limited assembly of the sparse front
end (``madqp_kkt_set_bandwidth``, option ``kkt_bandwidth``).  The factor is held to scipy with the bars of
tests/test_gpu_dense.py::test_cholesky_factor_and_solve, and must neither read nor write beyond the extent the plan reports
(tests/test_band_plan.py holds the plan itself); the assembled band has the bits of the dense assembly and zeros outside;
whole solves follow the oracle and the run without a bandwidth."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import madqp_jl_amd as M
from madqp_jl_amd import preprocess as P
from madqp_jl_amd.kkt import pattern_bandwidth
from oracle import mpc
from oracle import qp as Q
from parity import assert_parity, close
from band_cases import UPDATE, band_spd, banded_qp, plan

pytestmark = pytest.mark.gpu
REG = M.FixedRegularization(1e-8, -1e-8)
OREG = mpc.FixedRegularization(1e-8, -1e-8)
FACTOR_SHAPES = [(129, 0), (129, 1), (500, 127), (500, 128), (1537, 129), (1537, 300), (2100, 200), (2100, 640), (2100, 2099)]


def dev(a, be):
    return torch.as_tensor(np.ascontiguousarray(a), device=be.device)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(n, bw):
    K = band_spd(n, bw)
    return K, sla.cholesky(K, lower=True)


def leading_dimension(n, padded):
    return (n + 127) // 128 * 128 + 2 if padded else n + (3 if n % 2 else 2)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,bw", FACTOR_SHAPES)
def test_band_factor(hip, n, bw, padded):
    K, Lref = reference(n, bw)
    lda = leading_dimension(n, padded)
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        hip.chol_set_signature(h, n)  # accepted under a band (plain Cholesky): the band's schedule must stand
        extent = hip.chol_band_extent(h)
        ops, plan_extent = plan(n, bw)
        assert extent == plan_extent
        if (n, bw) == (2100, 200):  # three outer panels, the third starts its k range at 1280
            assert [tuple(o[1:]) for o in ops if o[0] == UPDATE and o[5] > 384][-1] == (1536, 564, 1280, 1536, 564, -1)
        i, j = np.indices((n, n))
        stored = np.where(i - j > bw, 0.0, K)  # zeros for bw < i - j <= extent
        stored[(i < j) | (i - j > extent)] = np.nan
        host = np.full((n, lda), np.nan)  # column-major: tensor row j = column j of K; the rows past n are NaN too
        host[:, :n] = stored.T
        Kd = dev(host, hip)
        assert hip.chol_factor(h, Kd, lda) == 0
        out = Kd.cpu().numpy()
        was_nan = np.isnan(host)
        assert np.array_equal(bits(out[was_nan]), bits(host[was_nan])), "every NaN is still that NaN"
        assert not np.any(np.isnan(out[~was_nan]))
        L = np.where((i < j) | (i - j > extent), 0.0, out[:, :n].T)
        rel = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
        print(f"n={n} bw={bw} extent={extent}: |LL'-K|/|K| = {rel:.2e}, max|L-Lref|/max|Lref| = "
              f"{np.max(np.abs(L - Lref)) / np.max(np.abs(Lref)):.2e}")
        assert rel < 1e-14 * max(1, math.sqrt(n)), rel
        assert np.max(np.abs(L - Lref)) / np.max(np.abs(Lref)) < 1e-11
        assert not np.any(L[i - j > bw]), "stored zeros stay zeros"
        hip.chol_set_bandwidth(h, -1)
        assert hip.chol_band_extent(h) == n - 1
    finally:
        hip.chol_destroy(h)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,bw", FACTOR_SHAPES)
def test_band_solve(hip, n, bw, padded):
    K, Lref = reference(n, bw)
    lda = leading_dimension(n, padded)
    host = np.zeros((n, lda))
    host[:, :n] = K.T  # zeros everywhere outside the band
    b = np.random.default_rng(n + bw).standard_normal(n)
    xref = sla.cho_solve((Lref, True), b)
    h = hip.chol_create(n)
    try:
        xs = []
        for band in (bw, -1):  # the band schedule, then the same handle with the bandwidth cleared: the dense schedule
            hip.chol_set_bandwidth(h, band)
            Kd, bd = dev(host, hip), dev(b, hip)
            assert hip.chol_factor(h, Kd, lda) == 0
            hip.chol_solve(h, bd)
            xs.append(bd.cpu().numpy())
        x = xs[0]
        assert np.linalg.norm(K @ x - b) / (np.linalg.norm(K) * np.linalg.norm(x)) < 1e-14
        assert np.linalg.norm(x - xref) / np.linalg.norm(xref) < 1e-10
        assert np.linalg.norm(x - xs[1]) / np.linalg.norm(xs[1]) < 1e-12
    finally:
        hip.chol_destroy(h)


def test_band_info_follows_lapack(hip):
    n, bw = 300, 40
    K = band_spd(n, bw).copy()
    K[200, 200] = -1.0
    _, info_ref = sla.lapack.dpotrf(K, lower=1)
    assert info_ref == 201
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        host = np.zeros((n, n + 2))
        host[:, :n] = K.T
        assert hip.chol_factor(h, dev(host, hip), n + 2) == info_ref
    finally:
        hip.chol_destroy(h)


def sparse_kkt(hip, mode, nx=40, m=15, abw=3):
    q = banded_qp(nx, m, abw, 5)
    csr = M.DeviceCSR.from_dense(hip.device, q["A"].toarray())
    st = hip.new_state(nx + m, m, [], [])
    cls = {0: M.HIPSparseCondensedKKTSystem, 2: M.HIPSparseAugmentedKKTSystem}[mode]
    return cls(hip, st, nx, list(range(m)), M.DeviceSymCSR.from_dense(hip.device, q["H"].toarray()), csr), q


def test_refusals_are_return_codes(hip):
    lib, ERR_ARG = hip.lib, -1
    n = 300
    h = hip.chol_create(n)
    try:
        assert lib.madqp_chol_set_bandwidth(h, n) == ERR_ARG and lib.madqp_chol_set_bandwidth(h, -2) == ERR_ARG
        assert lib.madqp_chol_set_bandwidth(None, 3) == ERR_ARG and lib.madqp_chol_band_extent(h, None) == ERR_ARG
        hip.chol_set_signature(h, 128)
        assert lib.madqp_chol_set_bandwidth(h, 10) == ERR_ARG  # a signature is set
        hip.chol_set_signature(h, n)
        hip.chol_set_bandwidth(h, 10)
        assert lib.madqp_chol_set_signature(h, 128) == ERR_ARG
        Kd = dev(np.eye(n), hip)
        assert lib.madqp_chol_factor_begin(h, M._lib.ptr(Kd), n) == ERR_ARG
        assert lib.madqp_chol_factor_panel(h, 0, 128) == ERR_ARG
        assert hip.chol_factor(h, Kd, n) == 0  # the handle and the context are usable afterwards
        hip.chol_set_bandwidth(h, -1)
        assert lib.madqp_chol_factor_begin(h, M._lib.ptr(Kd), n) == 0 and lib.madqp_chol_factor_panel(h, 0, 128) == 0
    finally:
        hip.chol_destroy(h)
    # KKT objects: a dense Jacobian, the augmented form, a bandwidth below the pattern's, set_hcsr / set_hdiag afterwards
    q = banded_qp(40, 15, 3, 5)
    st = hip.new_state(55, 15, [], [])
    A = dev(q["A"].toarray(), hip)
    dense = M.HIPCondensedKKTSystem(hip, st, 40, list(range(15)), None, A)
    aug, _ = sparse_kkt(hip, 2)
    cond, _ = sparse_kkt(hip, 0)
    try:
        assert lib.madqp_kkt_set_bandwidth(dense._h, 10) == ERR_ARG
        assert lib.madqp_kkt_set_bandwidth(aug._h, 10) == ERR_ARG
        own = pattern_bandwidth(cond.csr, cond.H, "condensed")
        assert own == 3
        assert lib.madqp_kkt_set_bandwidth(cond._h, own - 1) == ERR_ARG and b"half-bandwidth is 3" in lib.madqp_last_error(hip.ctx)
        assert lib.madqp_kkt_set_bandwidth(cond._h, 40) == ERR_ARG and lib.madqp_kkt_set_bandwidth(cond._h, -1) == ERR_ARG
        assert lib.madqp_kkt_set_bandwidth(None, 3) == ERR_ARG
        with pytest.raises(ValueError):
            aug.set_bandwidth("auto")
        assert cond.set_bandwidth("auto") == own and cond.linear_solver.bandwidth == own
        H = cond.H
        assert lib.madqp_kkt_set_hcsr(cond._h, M._lib.ptr(H.ptr), M._lib.ptr(H.col), M._lib.ptr(H.val)) == ERR_ARG
        assert lib.madqp_kkt_set_hdiag(cond._h, M._lib.ptr(st.x)) == ERR_ARG
        cond.initialize()
        cond.set_aug_diagonal_reg(1.0, -1e-8)
        cond.factorize_wrapper()
        assert cond.linear_solver.is_factorized()
    finally:
        for k in (dense, aug, cond):
            k.close()


# ---- assembly -----------------------------------------------------------------------------------------------------------
def whole_matrix(be, kkt, order):
    ptr, ld = be.kkt_matrix(kkt._h, order)
    return be.read_doubles(ptr, ld * order).reshape(order, ld).T  # [i, j] = K[i + j * ld]


def banded_device_qp(be, q):
    dq = M.DeviceQP.from_numpy(be.device, None, q["q"], q["A"].toarray(), q["lvar"], q["uvar"], q["lcon"], q["ucon"], q["x0"],
                               sparse=True)
    dq.H = M.DeviceSymCSR.from_dense(be.device, q["H"].toarray())
    return dq


def assembly_cases():
    # (inequality rows only: an equality row enters with Theta = 1e8, and the bound on K solve(b) - b below -- the one of
    # tests/test_gpu_sparse_hessian.py -- is for matrices with entries of order one; equality rows are in the whole solves)
    yield "condensed-hcsr", "condensed", lambda be: banded_device_qp(be, banded_qp(300, 120, 6, 11)), REG
    for N in (12, 25):
        yield f"normal-bc{N}", "normal", lambda be, N=N: P.to_device(P.boundary_control_qp(N), be), M.FixedRegularization(1e-8, 0.0)


@pytest.mark.parametrize("name,form,make,reg", list(assembly_cases()), ids=lambda c: c if isinstance(c, str) else "")
def test_band_assembly_and_solve(hip, name, form, make, reg):
    dq = make(hip)
    pair = [M.MPCSolver(dq, hip, kkt_system=form, regularization=reg) for _ in range(2)]
    for s in pair:
        s.initialize()
        s.kkt.set_aug_diagonal_reg(1.0, -1e-8 if form == "condensed" else 0.0)
    sb, sd = pair
    order = sb.m if form == "normal" else sb.nx
    try:
        sb.kkt.build_kkt()
        dense = whole_matrix(hip, sb.kkt, order)  # the same object's build without a bandwidth
        bw = sb.kkt.set_bandwidth("auto")
        assert bw == pattern_bandwidth(sb.A, sb.H, form) and 0 < bw < order // 4
        extent = hip.chol_band_extent(hip.kkt_chol(sb.kkt._h)[0])
        assert extent == plan(order, bw)[1] and bw < extent
        sb.kkt.build_kkt()
        band = whole_matrix(hip, sb.kkt, order)
        i, j = np.indices(band.shape)
        inside = (i >= j) & (i - j <= bw) & (i < order)
        assert np.array_equal(bits(band[inside]), bits(dense[inside])), "inside the band: the bits of the dense assembly"
        assert np.all(bits(band[(i - j > bw)]) == 0), "every stored double below the band is zero"
        assert np.any(dense[inside & (i - j == bw)] != 0.0), "the band is as wide as claimed"
        assert not np.any(dense[(i - j > bw) & (i < order)]), "the dense assembly has nothing outside it either"
        # a NaN inside the extent, as a factorisation that broke down leaves it: the next build removes it
        ptr, ld = hip.kkt_matrix(sb.kkt._h, order)
        jn = 1
        in_ = min(order - 1, jn + extent)
        assert in_ - jn > bw
        nan = np.array([np.nan])
        hip._ck(hip.lib.madqp_memcpy_h2d(hip.ctx, C.c_void_p(ptr + 8 * (in_ + jn * ld)), nan.ctypes.data, 8))
        assert np.isnan(whole_matrix(hip, sb.kkt, order)[in_, jn])
        sb.kkt.build_kkt()
        again = whole_matrix(hip, sb.kkt, order)
        assert np.array_equal(bits(again), bits(band))
        # solve! on the same state: the band object against the one without a bandwidth
        rng = np.random.default_rng(3)
        b = rng.standard_normal(sb.st.ntot)
        xs, ress = [], []
        for s in (sb, sd):
            s.kkt.factorize_wrapper()
            assert s.kkt.linear_solver.is_factorized()
            s.st.p.copy_(torch.as_tensor(b))
            hip.copy(s.st.p, s.st.d)
            s.kkt.solve(s.st.d)
            hip.fill(0.0, s.st.w1)
            s.kkt.mul(s.st.w1, s.st.d, 1.0, 0.0)
            res = np.max(np.abs(s.st.w1.cpu().numpy() - b)) / np.max(np.abs(b))
            print(f"{name}: |K solve(b) - b| / |b| = {res:.2e} ({'band' if s is sb else 'dense'})")
            ress.append(res)
            xs.append(s.st.d.cpu().numpy().copy())
        assert max(ress) < 1e-8, ress
        assert sd.kkt.linear_solver.bandwidth is None
        assert np.max(np.abs(xs[0] - xs[1])) <= 1e-8 * np.max(np.abs(xs[1]))
    finally:
        for s in pair:
            s.close()


# ---- whole solves -------------------------------------------------------------------------------------------------------
def run(hip, dq, form, reg, driver, bandwidth, **kw):
    s = M.MPCSolver(dq, hip, kkt_system=form, regularization=reg, driver=driver, kkt_bandwidth=bandwidth, **kw)
    r = s.solve()
    used = s.kkt.linear_solver.bandwidth
    s.close()
    return r, used


@functools.lru_cache(maxsize=None)
def boundary_control(N):
    h = P.boundary_control_qp(N)
    dense = Q.DenseQP(H=h.H.toarray(), q=h.c, A=h.A.toarray(), lvar=h.lvar, uvar=h.uvar, lcon=h.lcon, ucon=h.ucon, x0=h.x0,
                      c0=h.c0)
    return h, dense, mpc.solve(dense, kkt_system="K2", regularization=mpc.FixedRegularization(1e-8, 0.0))


@pytest.mark.parametrize("driver", ["python", "native"])
@pytest.mark.parametrize("N", [12, 25, 40])
def test_boundary_control_normal_equations(hip, N, driver):
    h, dense, ref = boundary_control(N)
    dq = P.to_device(h, hip)
    reg = M.FixedRegularization(1e-8, 0.0)
    r, used = run(hip, dq, "normal", reg, driver, "auto")
    r0, used0 = run(hip, dq, "normal", reg, driver, None)
    assert used == 2 * N and used0 is None
    assert r["status"] == r0["status"] == ref["status"] == M.SOLVE_SUCCEEDED
    assert r["iter"] == r0["iter"], (r["iter"], r0["iter"])
    assert_parity(r, ref, dense, f"boundary control N={N} {driver}", kkt_system="K2", regularization=mpc.FixedRegularization(1e-8, 0.0))


@functools.lru_cache(maxsize=None)
def condensed_case(i):
    q = banded_qp(300, 120, 6, 21) if i == 0 else banded_qp(200, 80, 9, 22, n_eq=1)
    dense = Q.DenseQP(H=q["H"].toarray(), q=q["q"], A=q["A"].toarray(), lvar=q["lvar"], uvar=q["uvar"], lcon=q["lcon"],
                      ucon=q["ucon"], x0=q["x0"], c0=0.0)
    return q, dense, mpc.solve(dense, kkt_system="condensed", regularization=OREG)


@pytest.mark.parametrize("driver", ["python", "native"])
@pytest.mark.parametrize("i", [0, 1])
def test_banded_condensed_qps(hip, i, driver):
    q, dense, ref = condensed_case(i)
    dq = banded_device_qp(hip, q)
    r, used = run(hip, dq, "condensed", REG, driver, "auto")
    r0, used0 = run(hip, dq, "condensed", REG, driver, None)
    assert used == (6, 9)[i] and used0 is None
    assert r["status"] == r0["status"] == ref["status"] == M.SOLVE_SUCCEEDED
    assert r["iter"] == r0["iter"], (r["iter"], r0["iter"])
    assert_parity(r, ref, dense, f"banded condensed {i} {driver}", regularization=OREG)


def test_auto_keeps_a_wide_band_dense(hip):
    q = banded_qp(40, 30, 12, 4)  # bw + 1 > order / 4
    r, used = run(hip, banded_device_qp(hip, q), "condensed", REG, "python", "auto")
    assert used is None and r["status"] == M.SOLVE_SUCCEEDED
    r, used = run(hip, banded_device_qp(hip, q), "condensed", REG, "python", 20)
    assert used == 20 and r["status"] == M.SOLVE_SUCCEEDED


@pytest.mark.parametrize("driver", ["python", "native"])
def test_regularization_retry_rewrites_the_extent(hip, driver):
    """A free variable with curvature -1e-7, as tests/test_gpu_batched.py::test_batched_regularization_retry builds it: the
    first factorisation breaks down, the x100 retry succeeds on the matrix the band assembly writes over the factor of
    the failed attempt; the retry count, the status and the last trace record follow the oracle's."""
    q = banded_qp(300, 120, 6, 31, free_curvature=-1e-7)
    dense = Q.DenseQP(H=q["H"].toarray(), q=q["q"], A=q["A"].toarray(), lvar=q["lvar"], uvar=q["uvar"], lcon=q["lcon"],
                      ucon=q["ucon"], x0=q["x0"], c0=0.0)
    ref = mpc.solve(dense, kkt_system="condensed", regularization=OREG, max_iter=4)
    r, used = run(hip, banded_device_qp(hip, q), "condensed", REG, driver, "auto", max_iter=4)
    assert used == 6
    assert ref["n_factorizations"] > ref["iter"] + 1, "the oracle retries"
    assert r["status"] == ref["status"] and r["iter"] == ref["iter"], (r["status"], ref["status"], r["iter"], ref["iter"])
    assert r["n_factorizations"] == ref["n_factorizations"], (r["n_factorizations"], ref["n_factorizations"])
    t, g = r["trace"][-1], ref["trace"][-1]
    for key in ("inf_pr", "inf_du", "mu", "alpha_p", "alpha_d"):
        assert close(t[key], g[key], 1e-6), (key, t[key], g[key])
    assert close(t["del_w"], g["del_w"], 1e-12)
    assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-6
