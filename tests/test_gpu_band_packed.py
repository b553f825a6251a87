"""GPU: packed band storage for the band Cholesky (``madqp_chol_set_packed``, ``madqp_chol_packed_layout``) and KKT objects
that never allocate the order^2 matrix (``madqp_kkt_create_sparse_packed``, option ``kkt_storage="packed"``).  Entry (i, j)
lives at P[i + j ld], ld >= extent; every other slot of the storage holds a planted NaN, so a store outside the band
shows as a NaN that is gone or as a wrong band entry, a read outside it as a NaN inside.  With an even ld the launches are
those of the dense storage with a padded leading dimension, argument for argument apart from the leading dimension: the
factor and the solution must have its bits.  The layout and the plan are held without a GPU in tests/test_band_packed.py."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import madqp_jl_amd as M
from madqp_jl_amd import preprocess as P
from oracle import mpc
from parity import TRACE_KEYS, assert_parity
from band_cases import band_index, band_spd, banded_qp, layout, nan_kept, pack, plan, unpack
from test_gpu_band import (OREG, REG, banded_device_qp, bits, boundary_control, condensed_case, dev, leading_dimension,
                           reference, whole_matrix)
from test_gpu_band_sweeps import bars, create, planted, rhs

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
SHAPES = [(129, 1), (500, 127), (1537, 129), (1537, 300), (2100, 200), (2100, 640), (2100, 2099)]
CASES = [(n, bw, kind) for n, bw in SHAPES for kind in ("library", "even")] + [(1537, 129, "odd")]


def test_the_shapes_leave_room_below_the_extent():
    """packed storage differs from dense only where the extent is well below the order"""
    assert sum(plan(n, bw)[1] < n - 129 for n, bw in SHAPES) >= 3


def packed_ld(hip, h, extent, kind):
    if kind == "library":
        return hip.chol_packed_layout(h)
    ld = extent + extent % 2 if kind == "even" else extent + 1 - extent % 2  # smallest even / odd ld >= extent
    assert ld >= extent and ld % 2 == (kind == "odd")
    return hip.chol_packed_layout(h, ld)


@pytest.mark.parametrize("n,bw,kind", CASES)
def test_packed_factor_and_solve(hip, n, bw, kind):
    K, Lref = reference(n, bw)
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        extent = hip.chol_band_extent(h)
        assert extent == plan(n, bw)[1]
        ld, doubles = packed_ld(hip, h, extent, kind)
        assert (ld, doubles) == layout(n, extent, ld) and doubles == (n + 127) // 128 * 128 * (ld + 1) + 128
        if kind == "library":
            assert ld % 2 == 0 and ld >= extent + 1
        i, j = np.indices((n, n))
        host, addr = pack(np.where(i - j > bw, 0.0, K), extent, ld, doubles)  # zeros for bw < i - j <= extent, NaN elsewhere
        hip.chol_set_packed(h, True)
        Pd, bd = dev(host, hip), dev(rhs(n, bw), hip)
        assert hip.chol_factor(h, Pd, ld) == 0
        hip.chol_solve(h, bd)
        out, x = Pd.cpu().numpy(), bd.cpu().numpy()
        assert nan_kept(out, addr), "every NaN is still that NaN"
        assert not np.any(np.isnan(out[addr])), "no NaN inside the band"
        L = unpack(out, n, extent, ld)
        rel = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
        far = np.max(np.abs(L - Lref)) / np.max(np.abs(Lref))
        print(f"n={n} bw={bw} extent={extent} ld={ld} ({doubles} doubles): |LL'-K|/|K| = {rel:.2e}, max|L-Lref|/max|Lref| = {far:.2e}")
        assert rel < 1e-14 * max(1, math.sqrt(n)), rel  # the bars of test_band_factor
        assert far < 1e-11
        assert not np.any(L[i - j > bw]), "stored zeros stay zeros"
        bars(n, bw, x, f"packed n={n} bw={bw} ld={ld}")  # the bars of test_band_solve
        # the same handle on dense storage with a padded leading dimension (set_bandwidth turns packed off)
        hip.chol_set_bandwidth(h, bw)
        if ld < n:  # ... and the packed leading dimension is refused again
            assert hip.lib.madqp_chol_factor(h, M._lib.ptr(Pd), ld, C.byref(C.c_int32())) == ERR_ARG
        lda = leading_dimension(n, True)
        Kd, b2 = dev(planted(n, bw, lda, extent), hip), dev(rhs(n, bw), hip)
        assert hip.chol_factor(h, Kd, lda) == 0
        hip.chol_solve(h, b2)
        x2 = b2.cpu().numpy()
        assert np.linalg.norm(x - x2) / np.linalg.norm(x2) < 1e-12
        if kind != "odd":
            bi, bj = band_index(n, extent)
            assert np.array_equal(bits(out[addr]), bits(Kd.cpu().numpy()[bj, bi])), "the factor: the bits of the dense storage"
            assert np.array_equal(bits(x), bits(x2)), "the solution: the bits of the dense storage"
    finally:
        hip.chol_destroy(h)


def test_packed_info_follows_lapack(hip):
    n, bw = 300, 40
    K = band_spd(n, bw).copy()
    K[200, 200] = -1.0
    _, info_ref = sla.lapack.dpotrf(K, lower=1)
    assert info_ref == 201
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        extent = hip.chol_band_extent(h)
        ld, doubles = hip.chol_packed_layout(h)
        hip.chol_set_packed(h)
        host, _ = pack(np.tril(K), extent, ld, doubles)
        assert hip.chol_factor(h, dev(host, hip), ld) == info_ref
    finally:
        hip.chol_destroy(h)


# ---- KKT objects ----------------------------------------------------------------------------------------------------------
def kkt_cases():
    yield "condensed-hcsr", "condensed", lambda be: banded_device_qp(be, banded_qp(300, 120, 6, 11)), REG
    for N in (12, 25):
        yield f"normal-bc{N}", "normal", lambda be, N=N: P.to_device(P.boundary_control_qp(N), be), M.FixedRegularization(1e-8, 0.0)


def poke_nan(hip, ptr, offset):
    nan = np.array([np.nan])
    hip._ck(hip.lib.madqp_memcpy_h2d(hip.ctx, C.c_void_p(ptr + 8 * offset), nan.ctypes.data, 8))


@pytest.mark.parametrize("name,form,make,reg", list(kkt_cases()), ids=lambda c: c if isinstance(c, str) else "")
def test_packed_kkt_object(hip, name, form, make, reg):
    dq = make(hip)
    sp = M.MPCSolver(dq, hip, kkt_system=form, regularization=reg, kkt_bandwidth="auto", kkt_storage="packed")
    sb = M.MPCSolver(dq, hip, kkt_system=form, regularization=reg, kkt_bandwidth="auto")  # the band path on dense storage
    try:
        for s in (sp, sb):
            s.initialize()
            s.kkt.set_aug_diagonal_reg(1.0, -1e-8 if form == "condensed" else 0.0)
            s.kkt.build_kkt()
        order = sp.m if form == "normal" else sp.nx
        ch = hip.kkt_chol(sp.kkt._h)[0]
        bw, extent = sp.kkt.linear_solver.bandwidth, hip.chol_band_extent(ch)
        assert bw == sb.kkt.linear_solver.bandwidth and 0 < bw < extent == plan(order, bw)[1]
        ld, doubles = hip.chol_packed_layout(ch)
        assert hip.kkt_storage(sp.kkt._h) == (True, ld, doubles), "exactly the doubles of madqp_chol_packed_layout"
        npad = (order + 127) // 128 * 128
        assert hip.kkt_storage(sb.kkt._h) == (False, npad, npad * npad + 128)
        ptr, ld_k = hip.kkt_matrix(sp.kkt._h, order)
        assert ld_k == ld
        i, j = band_index(order, extent)
        dense = whole_matrix(hip, sb.kkt, order)
        packed = hip.read_doubles(ptr, doubles)
        assert np.array_equal(bits(packed[i + j * ld]), bits(dense[i, j])), "the band: the bits of the dense-storage band object"
        assert np.any(dense[i, j][i - j == bw] != 0.0)
        lower = np.tril(dense[:order, :order])
        assert np.array_equal(bits(sp.kkt.dense_matrix()), bits(lower)), "madqp_band_expand = that object's lower triangle"
        assert np.array_equal(bits(sb.kkt.dense_matrix()), bits(lower))
        # a NaN inside the extent, as a factorisation that broke down leaves it: the next build removes it
        jn = 1
        in_ = min(order - 1, jn + extent)
        assert in_ - jn > bw
        poke_nan(hip, ptr, in_ + jn * ld)
        assert np.isnan(hip.read_doubles(ptr, doubles)[in_ + jn * ld])
        sp.kkt.build_kkt()
        assert np.array_equal(bits(hip.read_doubles(ptr, doubles)), bits(packed))
        # a NaN in a gap slot (extent < i - j <= ld: no entry of the band, nothing reads or writes it): kept, and changes nothing
        gap = (jn + extent + 1) + jn * ld
        assert ld > extent and gap not in set((i + j * ld)[(j >= jn) & (j <= jn + 2)])
        poke_nan(hip, ptr, gap)
        sp.kkt.build_kkt()
        b = np.random.default_rng(3).standard_normal(sp.st.ntot)
        xs = []
        for s in (sp, sb):
            s.kkt.factorize_wrapper()
            assert s.kkt.linear_solver.is_factorized()
            s.st.p.copy_(torch.as_tensor(b))
            hip.copy(s.st.p, s.st.d)
            s.kkt.solve(s.st.d)
            xs.append(s.st.d.cpu().numpy().copy())
        after = hip.read_doubles(ptr, doubles)
        assert np.isnan(after[gap]) and np.count_nonzero(np.isnan(after)) == 1, "the gap keeps its NaN, the band has none"
        assert np.array_equal(bits(after[i + j * ld]), bits(whole_matrix(hip, sb.kkt, order)[i, j])), "the factors"
        assert np.array_equal(bits(xs[0]), bits(xs[1])), "solve!: the bits of the dense-storage object"
        with pytest.raises(M.MadQPError):
            sp.kkt.set_bandwidth(bw)  # laid out once
    finally:
        sp.close()
        sb.close()


# ---- whole solves -----------------------------------------------------------------------------------------------------------
def solve(hip, dq, form, reg, driver, storage, **kw):
    s = M.MPCSolver(dq, hip, kkt_system=form, regularization=reg, driver=driver, kkt_bandwidth="auto", kkt_storage=storage, **kw)
    r = s.solve()
    r["_storage"] = hip.kkt_storage(s.kkt._h)
    r["_bandwidth"] = s.kkt.linear_solver.bandwidth
    s.close()
    return r


def assert_same_run(r, r0):
    """bitwise the results of the dense-storage run under the same bandwidth"""
    assert r["_storage"][0] and not r0["_storage"][0] and r["_bandwidth"] == r0["_bandwidth"]
    assert (r["status"], r["iter"], r["n_factorizations"]) == (r0["status"], r0["iter"], r0["n_factorizations"])
    assert np.array_equal(bits(r["solution"]), bits(r0["solution"]))
    assert np.array_equal(bits(r["multipliers"]), bits(r0["multipliers"]))
    assert bits(r["objective"]) == bits(r0["objective"])
    for t, t0 in zip(r["trace"], r0["trace"]):
        assert [bits(t[k]) for k in TRACE_KEYS] == [bits(t0[k]) for k in TRACE_KEYS], t["k"]


@pytest.mark.parametrize("driver", ["python", "native"])
@pytest.mark.parametrize("N", [12, 25])
def test_packed_boundary_control_normal_equations(hip, N, driver):
    h, dense, ref = boundary_control(N)
    dq = P.to_device(h, hip)
    reg = M.FixedRegularization(1e-8, 0.0)
    r, r0 = (solve(hip, dq, "normal", reg, driver, st) for st in ("packed", "dense"))
    assert r["_bandwidth"] == 2 * N and r["status"] == ref["status"] == M.SOLVE_SUCCEEDED
    assert_parity(r, ref, dense, f"packed boundary control N={N} {driver}", kkt_system="K2", regularization=mpc.FixedRegularization(1e-8, 0.0))
    assert_same_run(r, r0)


@pytest.mark.parametrize("driver", ["python", "native"])
def test_packed_banded_condensed_qp(hip, driver):
    q, dense, ref = condensed_case(0)
    dq = banded_device_qp(hip, q)
    r, r0 = (solve(hip, dq, "condensed", REG, driver, st) for st in ("packed", "dense"))
    assert r["_bandwidth"] == 6 and r["status"] == ref["status"] == M.SOLVE_SUCCEEDED
    assert_parity(r, ref, dense, f"packed banded condensed {driver}", regularization=OREG)
    assert_same_run(r, r0)


@pytest.mark.parametrize("driver", ["python", "native"])
def test_packed_regularization_retry(hip, driver):
    """tests/test_gpu_band.py::test_regularization_retry_rewrites_the_extent on packed storage: the first factorisation
    breaks down, the band assembly rewrites the packed band over the factor of the failed attempt."""
    from oracle import qp as Q
    from parity import close

    q = banded_qp(300, 120, 6, 31, free_curvature=-1e-7)
    dense = Q.DenseQP(H=q["H"].toarray(), q=q["q"], A=q["A"].toarray(), lvar=q["lvar"], uvar=q["uvar"], lcon=q["lcon"],
                      ucon=q["ucon"], x0=q["x0"], c0=0.0)
    ref = mpc.solve(dense, kkt_system="condensed", regularization=OREG, max_iter=4)
    r, r0 = (solve(hip, banded_device_qp(hip, q), "condensed", REG, driver, st, max_iter=4) for st in ("packed", "dense"))
    assert ref["n_factorizations"] > ref["iter"] + 1, "the oracle retries"
    assert r["status"] == ref["status"] and r["iter"] == ref["iter"] and r["n_factorizations"] == ref["n_factorizations"]
    t, g = r["trace"][-1], ref["trace"][-1]
    for key in ("inf_pr", "inf_du", "mu", "alpha_p", "alpha_d"):
        assert close(t[key], g[key], 1e-6), (key, t[key], g[key])
    assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-6
    assert_same_run(r, r0)


def test_auto_falls_back_to_dense_storage_with_the_schedule(hip):
    q = banded_qp(40, 30, 12, 4)  # bw + 1 > order / 4: the band rule declines
    r = solve(hip, banded_device_qp(hip, q), "condensed", REG, "python", "packed")
    assert r["_bandwidth"] is None and not r["_storage"][0] and r["status"] == M.SOLVE_SUCCEEDED


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_chol_refusals_are_return_codes(hip):
    lib, n, bw = hip.lib, 700, 40
    K = band_spd(n, bw)
    out2 = (C.c_int64 * 2)()
    h = hip.chol_create(n)
    try:
        assert lib.madqp_chol_set_packed(h, 1) == ERR_ARG and lib.madqp_chol_packed_layout(h, 0, out2) == ERR_ARG  # no bandwidth
        assert lib.madqp_chol_set_packed(None, 1) == ERR_ARG and lib.madqp_chol_packed_layout(None, 0, out2) == ERR_ARG
        assert lib.madqp_chol_set_packed(h, 0) == 0
        hip.chol_set_signature(h, 128)
        assert lib.madqp_chol_set_packed(h, 1) == ERR_ARG  # a signature (and therefore no bandwidth)
        hip.chol_set_signature(h, n)
        hip.chol_set_bandwidth(h, bw)
        extent = hip.chol_band_extent(h)
        assert extent < n - 129
        assert lib.madqp_chol_packed_layout(h, extent - 1, out2) == ERR_ARG and b"below the extent" in lib.madqp_last_error(hip.ctx)
        assert lib.madqp_chol_packed_layout(h, 0, None) == ERR_ARG
        ld, doubles = hip.chol_packed_layout(h)
        hip.chol_set_packed(h)
        assert lib.madqp_chol_set_signature(h, 128) == ERR_ARG
        host, addr = pack(np.tril(K), extent, ld, doubles)
        Pd = dev(host, hip)
        info = C.c_int32()
        assert lib.madqp_chol_factor(h, M._lib.ptr(Pd), extent - 1, C.byref(info)) == ERR_ARG  # ld < extent
        assert lib.madqp_chol_factor_begin(h, M._lib.ptr(Pd), ld) == ERR_ARG
        assert hip.chol_factor(h, Pd, ld) == 0  # the handle and the context are usable afterwards
        bd = dev(rhs(n, bw), hip)
        hip.chol_solve(h, bd)
        assert nan_kept(Pd.cpu().numpy(), addr)
        x = bd.cpu().numpy()
        assert np.linalg.norm(K @ x - rhs(n, bw)) / (np.linalg.norm(K) * np.linalg.norm(x)) < 1e-14
        hip.chol_set_bandwidth(h, bw)  # any value turns packed off: the lda is an ordinary one again
        assert lib.madqp_chol_factor(h, M._lib.ptr(Pd), ld, C.byref(info)) == ERR_ARG
        assert lib.madqp_chol_solve(h, M._lib.ptr(bd)) == ERR_STATE
    finally:
        hip.chol_destroy(h)
    h = create(hip, n, MADQP_SWEEP_BAND=0)  # the dense sweeps read the whole triangle
    try:
        hip.chol_set_bandwidth(h, bw)
        assert hip.chol_sweep_info(h)[0] == -1
        assert lib.madqp_chol_set_packed(h, 1) == ERR_ARG
        Kd = dev(np.ascontiguousarray(K), hip)
        assert hip.chol_factor(h, Kd, n) == 0
    finally:
        hip.chol_destroy(h)


def test_kkt_refusals_are_return_codes(hip):
    lib = hip.lib
    q = banded_qp(300, 120, 6, 11)
    nx, m = 300, 120
    csr = M.DeviceCSR.from_dense(hip.device, q["A"].toarray())
    H = M.DeviceSymCSR.from_dense(hip.device, q["H"].toarray())
    ineq = (C.c_int64 * m)(*range(m))
    ptr = M._lib.ptr
    args = (ptr(csr.ptr), ptr(csr.col), ptr(csr.val), ptr(csr.t_ptr), ptr(csr.t_col), ptr(csr.t_val))
    out = C.c_void_p()
    for mode in (2, 3, -1):
        assert lib.madqp_kkt_create_sparse_packed(hip.ctx, mode, nx, m, m, ineq, *args, C.byref(out)) == ERR_ARG
    assert lib.madqp_kkt_create_sparse_packed(None, 0, nx, m, m, ineq, *args, C.byref(out)) == ERR_ARG
    st = hip.new_state(nx + m, m, [], [])
    h = hip.kkt_create_sparse_packed(0, nx, m, list(range(m)), csr, csr.t_val)
    try:
        hip.kkt_set_hcsr(h, H)
        assert hip.kkt_storage(h) == (True, 0, 0)
        info, Kp, ld = C.c_int32(), C.c_void_p(), C.c_int64()
        cst = C.byref(st.cstruct)
        for rc in (lib.madqp_kkt_build(h, cst), lib.madqp_kkt_factorize(h, C.byref(info)),
                   lib.madqp_kkt_matrix(h, C.byref(Kp), C.byref(ld)), lib.madqp_kkt_solve(h, cst, ptr(st.d))):
            assert rc == ERR_STATE and b"before madqp_kkt_set_bandwidth" in lib.madqp_last_error(hip.ctx)
        assert lib.madqp_kkt_set_bandwidth(h, 2) == ERR_ARG and hip.kkt_storage(h) == (True, 0, 0)  # below the pattern's
        hip.kkt_set_bandwidth(h, 6)
        ch = hip.kkt_chol(h)[0]
        assert hip.kkt_storage(h) == (True,) + hip.chol_packed_layout(ch)
        assert lib.madqp_kkt_set_bandwidth(h, 6) == ERR_STATE and lib.madqp_kkt_set_bandwidth(h, 7) == ERR_STATE
        assert b"laid out already" in lib.madqp_last_error(hip.ctx)
        assert lib.madqp_kkt_set_hdiag(h, ptr(st.x)) == ERR_ARG
        assert lib.madqp_kkt_storage(None, None) == ERR_ARG and lib.madqp_kkt_storage(h, None) == ERR_ARG
        # the object and the context are usable afterwards
        hip.kkt_initialize(h, st)
        hip.kkt_build(h, st)
        assert hip.kkt_factorize(h) == 0
    finally:
        hip.kkt_destroy(h)
    # madqp_band_expand: its own argument checks
    D = torch.zeros((4, 4), dtype=torch.float64, device=hip.device)
    Pk = torch.zeros(64, dtype=torch.float64, device=hip.device)
    assert lib.madqp_band_expand(hip.ctx, 4, ptr(Pk), 2, 3, ptr(D), 4) == ERR_ARG  # reach > ld
    assert lib.madqp_band_expand(hip.ctx, 4, ptr(Pk), 2, 1, ptr(D), 3) == ERR_ARG  # ldd < n
    assert lib.madqp_band_expand(hip.ctx, 4, None, 2, 1, ptr(D), 4) == ERR_ARG
    assert lib.madqp_band_expand(None, 4, ptr(Pk), 2, 1, ptr(D), 4) == ERR_ARG
    hip.band_expand(4, Pk, 2, 1, D, 4)


def test_band_expand(hip):
    """reach below the stored extent: copied up to the reach, zeros below it, the upper triangle left alone"""
    n, extent, ld = 300, 70, 75
    rng = np.random.default_rng(5)
    full = np.tril(rng.standard_normal((n, n)))
    host, _ = pack(full, extent, ld, 384 * (ld + 1) + 128)
    for reach in (0, 33, extent):
        D = torch.full((n, n + 3), 7.0, dtype=torch.float64, device=hip.device)
        hip.band_expand(n, dev(host, hip), ld, reach, D, n + 3)
        got = D.cpu().numpy()[:, :n].T  # [i, j]
        i, j = np.indices((n, n))
        want = np.where(i < j, 7.0, np.where(i - j <= reach, full, 0.0))
        assert np.array_equal(bits(got), bits(want)) and np.all(D.cpu().numpy()[:, n:] == 7.0)
