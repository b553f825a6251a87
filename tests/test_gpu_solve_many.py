"""GPU: solves with a block of right-hand sides -- ``madqp_chol_solve_many`` (chol.hip: the blocked path of
csrc/solve_plan.inc forced with ``min_nrhs = 2``, and the column-by-column path) and ``madqp_kkt_solve_many`` on every KKT
form.  The linear-solver level is held to scipy with the bounds of tests/test_gpu_dense.py::test_cholesky_factor_and_solve,
per column; the KKT level to the one-vector ``solve`` of the same object.  The plan itself is held without a GPU in
tests/test_solve_plan.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import madqp_jl_amd as M
import chol_cases
from band_cases import band_index, banded_qp, pack
from test_gpu_band import bits, dev, leading_dimension, reference
from test_gpu_band_sweeps import planted
from test_solve_plan import RES_BOUND, SOL_BOUND, plan

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4


def check_columns(X, Xref, K, B, tag):
    """the two bounds of the issue, per column"""
    normK = np.linalg.norm(K, 2)
    worst = [0.0, 0.0]
    for c in range(B.shape[1]):
        x, xr = X[:, c], Xref[:, c]
        worst[0] = max(worst[0], np.linalg.norm(K @ x - B[:, c]) / (normK * np.linalg.norm(x)))
        worst[1] = max(worst[1], np.linalg.norm(x - xr) / np.linalg.norm(xr))
    print(f"{tag}: worst residual {worst[0]:.2e}, worst distance to the reference {worst[1]:.2e}")
    assert worst[0] < RES_BOUND, worst
    assert worst[1] < SOL_BOUND, worst


def rhs_block(n, nrhs, ldb, seed):
    """(B as n x nrhs, the (nrhs, ldb) host block with NaN in rows n .. ldb - 1 of every column)"""
    B = np.random.default_rng(seed).standard_normal((n, nrhs))
    host = np.full((nrhs, ldb), np.nan)
    host[:, :n] = B.T
    return B, host


def solve_block(hip, h, n, host):
    Bd = dev(host, hip)
    hip.chol_solve_many(h, Bd, host.shape[1])
    out = Bd.cpu().numpy()
    assert np.array_equal(bits(out[:, n:]), bits(host[:, n:])), "rows n .. ldb - 1 come back bitwise untouched"
    return out[:, :n].T


_spd_ref = {}


def spd_reference(n):
    if n not in _spd_ref:
        K = chol_cases.good(n)
        _spd_ref[n] = (K, sla.cholesky(K, lower=True))
    return _spd_ref[n]


class Factored:
    """a handle with the factor of the shared matrix of order n in the given layout, blocked path forced"""

    def __init__(self, hip, n, lda, host=None, setup=None):
        self.hip, self.n = hip, n
        self.h = hip.chol_create(n)
        try:
            if setup:
                setup(self.h)
            self.Kd = dev(chol_cases.poisoned(chol_cases.good(n), lda) if host is None else host, hip)
            assert hip.chol_factor(self.h, self.Kd, lda) == 0
            hip.chol_set_solve_many_min(self.h, 2)
        except BaseException:
            hip.chol_destroy(self.h)
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.chol_destroy(self.h)


@pytest.mark.parametrize("n", [1, 17, 128, 129, 300])
def test_blocked_unpadded(hip, n):
    """left-looking schedule, leading dimension below the padded order: rows beyond n do not exist"""
    K, Lref = spd_reference(n)
    with Factored(hip, n, chol_cases.unpadded(n)) as f:
        for nrhs in (2, 15, 16, 17, 33):
            for ldb in (n, n + 3):
                B, host = rhs_block(n, nrhs, ldb, 1000 * n + nrhs)
                ops, launches, nbytes = plan(n, n, -1, nrhs, has_upper=False)
                info = hip.chol_solve_many_info(f.h, nrhs)
                assert (info[0], info[1], info[3]) == (1, launches, nbytes)
                X = solve_block(hip, f.h, n, host)
                check_columns(X, sla.cho_solve((Lref, True), B), K, B, f"unpadded n={n} nrhs={nrhs} ldb={ldb}")
        assert hip.chol_solve_many_info(f.h, 2)[2] >= 128 * 128 * ((n + 127) // 128), "the workspace is the handle's"


@pytest.mark.parametrize("n", [300, 1100])
def test_blocked_padded_with_upper(hip, n):
    """the mid-size schedule keeps U = L': the backward updates multiply with it, no strip"""
    K, Lref = spd_reference(n)
    with Factored(hip, n, chol_cases.padded(n)) as f:
        for nrhs in (2, 17, 130):
            for ldb in (n, n + 3):
                B, host = rhs_block(n, nrhs, ldb, 1000 * n + nrhs)
                ops, launches, nbytes = plan(n, n, -1, nrhs, has_upper=True)
                info = hip.chol_solve_many_info(f.h, nrhs)
                assert (info[0], info[1], info[3]) == (1, launches, nbytes), "U present: one launch per operation"
                X = solve_block(hip, f.h, n, host)
                check_columns(X, sla.cho_solve((Lref, True), B), K, B, f"padded n={n} nrhs={nrhs} ldb={ldb}")


@pytest.mark.parametrize("n,lda_of", [(300, chol_cases.unpadded), (300, chol_cases.padded)], ids=["unpadded", "padded"])
def test_path_identities(hip, n, lda_of):
    with Factored(hip, n, lda_of(n)) as f:
        B, host = rhs_block(n, 5, n + 3, 77)
        looped = dev(host, hip)
        for c in range(5):
            hip.chol_solve(f.h, looped[c])
        looped = looped.cpu().numpy()
        # nrhs = 1 is chol_solve
        one = dev(host[:1], hip)
        assert hip.chol_solve_many_info(f.h, 1)[0] == 0
        hip.chol_solve_many(f.h, one, n + 3)
        assert np.array_equal(bits(one.cpu().numpy()), bits(looped[:1]))
        # the forced column-by-column path at nrhs = 5 is five chol_solve calls
        hip.chol_set_solve_many_min(f.h, 6)
        assert hip.chol_solve_many_info(f.h, 5)[0] == 0 and hip.chol_solve_many_info(f.h, 6)[0] == 1
        cols = dev(host, hip)
        hip.chol_solve_many(f.h, cols, n + 3)
        assert np.array_equal(bits(cols.cpu().numpy()), bits(looped))
        # the same blocked call twice gives the same bits
        hip.chol_set_solve_many_min(f.h, 2)
        assert hip.chol_solve_many_info(f.h, 5)[0] == 1
        twice = []
        for _ in range(2):
            Bd = dev(host, hip)
            hip.chol_solve_many(f.h, Bd, n + 3)
            twice.append(Bd.cpu().numpy())
        assert np.array_equal(bits(twice[0]), bits(twice[1]))
        assert np.max(np.abs(twice[0][:, :n] - looped[:, :n])) <= 1e-10 * np.max(np.abs(looped[:, :n]))


@pytest.mark.parametrize("npos,nneg", [(128, 1), (128, 172), (256, 300)])
def test_signatures(hip, npos, nneg):
    stored, Mfull = chol_cases.quasidefinite(npos, nneg, 100 + npos + nneg)
    n, nrhs = npos + nneg, 17
    lda = chol_cases.unpadded(n)
    with Factored(hip, n, lda, chol_cases.lower_only(stored, lda), lambda h: hip.chol_set_signature(h, npos)) as f:
        B, host = rhs_block(n, nrhs, n + 3, n)
        X = solve_block(hip, f.h, n, host)
        check_columns(X, np.linalg.solve(Mfull, B), Mfull, B, f"signature ({npos}, {nneg})")


@pytest.mark.parametrize("bw", [127, 129, 300])
def test_band_and_packed(hip, bw):
    n, nrhs = 1537, 17
    K, Lref = reference(n, bw)
    B, host = rhs_block(n, nrhs, n + 3, n + bw)
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        hip.chol_set_solve_many_min(h, 2)
        extent = hip.chol_band_extent(h)
        kb = hip.chol_sweep_info(h)[0]
        assert kb == (bw + 127) // 128
        # dense storage, NaN beyond the extent (and above the diagonal, and in the rows past n)
        lda = leading_dimension(n, True)
        Kd = dev(planted(n, bw, lda, extent), hip)
        assert hip.chol_factor(h, Kd, lda) == 0
        info = hip.chol_solve_many_info(h, nrhs)
        assert (info[0], info[1], info[3]) == (1,) + plan(n, n, kb, nrhs, has_upper=False)[1:]
        Xd = solve_block(hip, h, n, host)
        assert np.isfinite(Xd).all(), "a NaN beyond the extent reached the solution"
        check_columns(Xd, sla.cho_solve((Lref, True), B), K, B, f"band bw={bw} dense storage")
        # the unpadded leading dimension: rows past n do not exist
        lda_u = leading_dimension(n, False)
        Ku = dev(planted(n, bw, lda_u, extent), hip)
        assert hip.chol_factor(h, Ku, lda_u) == 0
        check_columns(solve_block(hip, h, n, host), sla.cho_solve((Lref, True), B), K, B, f"band bw={bw} unpadded")
        # packed storage: NaN in every slot that is no band entry; bitwise the dense-storage band results
        ld, doubles = hip.chol_packed_layout(h)
        i, j = np.indices((n, n))
        phost, addr = pack(np.where(i - j > bw, 0.0, K), extent, ld, doubles)
        hip.chol_set_packed(h, True)
        assert hip.lib.madqp_chol_solve_many(h, None, n, nrhs) == ERR_ARG
        Bnull = dev(host, hip)
        assert hip.lib.madqp_chol_solve_many(h, M._lib.ptr(Bnull), n + 3, nrhs) == ERR_STATE, "set_packed forgot the factor"
        Pd = dev(phost, hip)
        assert hip.chol_factor(h, Pd, ld) == 0
        Xp = solve_block(hip, h, n, host)
        assert np.array_equal(bits(Xp), bits(Xd)), "packed storage: the bits of the dense-storage band handle"
    finally:
        hip.chol_destroy(h)


def test_return_codes(hip):
    lib, n = hip.lib, 300
    K, Lref = spd_reference(n)
    B, host = rhs_block(n, 4, n, 5)
    Bd = dev(host, hip)
    h = hip.chol_create(n)
    try:
        p = M._lib.ptr(Bd)
        assert lib.madqp_chol_solve_many(None, p, n, 4) == ERR_ARG
        assert lib.madqp_chol_solve_many(h, p, n, 4) == ERR_STATE, "before a factorisation"
        assert lib.madqp_chol_set_solve_many_min(h, 1) == ERR_ARG and lib.madqp_chol_set_solve_many_min(None, 2) == ERR_ARG
        assert lib.madqp_chol_solve_many_info(h, 4, None) == ERR_ARG and lib.madqp_chol_solve_many_info(h, -1, (C.c_int64 * 4)()) == ERR_ARG
        lda = chol_cases.unpadded(n)
        Kd = dev(chol_cases.poisoned(K, lda), hip)
        assert hip.chol_factor(h, Kd, lda) == 0
        hip.chol_set_solve_many_min(h, 3)
        assert [hip.chol_solve_many_info(h, r)[0] for r in (0, 1, 2, 3, 4)] == [0, 0, 0, 1, 1]
        assert lib.madqp_chol_solve_many(h, p, n, -1) == ERR_ARG
        assert lib.madqp_chol_solve_many(h, p, n - 1, 4) == ERR_ARG
        assert lib.madqp_chol_solve_many(h, None, n, 4) == ERR_ARG
        assert lib.madqp_chol_solve_many(h, None, n, 0) == 0 and lib.madqp_chol_solve_many(h, p, n, 0) == 0
        assert np.array_equal(bits(Bd.cpu().numpy()), bits(host)), "nrhs = 0 does nothing"
        hip.chol_solve_many(h, Bd, n)  # the handle works afterwards
        check_columns(Bd.cpu().numpy().T, sla.cho_solve((Lref, True), B), K, B, "after the refusals")
        hip.chol_set_bandwidth(h, 40)
        assert lib.madqp_chol_solve_many(h, p, n, 4) == ERR_STATE, "set_bandwidth forgot the factor"
    finally:
        hip.chol_destroy(h)
    h0 = hip.chol_create(0)
    try:
        assert hip.chol_factor(h0, Bd, 1) == 0
        assert lib.madqp_chol_solve_many(h0, None, 1, 3) == 0, "n = 0 does nothing"
    finally:
        hip.chol_destroy(h0)


# ---- KKT level --------------------------------------------------------------------------------------------------------------
NX, MROWS = 200, 90  # condensed order 200, normal order 90, augmented order 256 + 90


def seeded_state(hip, st, nx, seed):
    """iterates well inside their bounds and multipliers of order one: Sigma between 1.4 and 4"""
    rng = np.random.default_rng(seed)
    t = lambda a: torch.as_tensor(a, device=hip.device)
    n = st.n
    x = rng.standard_normal(n)
    st.x.copy_(t(x))
    st.xl.copy_(t(x - (0.5 + rng.random(n))))
    st.xu.copy_(t(x + (0.5 + rng.random(n))))
    st.zl.copy_(t(0.3 + rng.random(n)))
    st.zu.copy_(t(0.3 + rng.random(n)))
    st.y.copy_(t(rng.standard_normal(st.m)))


def make_kkt(hip, which):
    """(object, del_c): one object of each form on a dense A, or a sparse condensed one with a bandwidth in packed storage"""
    rng = np.random.default_rng(2024)
    nx, m = NX, MROWS
    A = rng.standard_normal((m, nx)) / np.sqrt(nx)
    ineq = list(range(m))
    lb = list(range(0, nx, 2)) + list(range(nx, nx + m))  # every slack is bounded on both sides
    ub = list(range(1, nx, 3)) + list(range(nx, nx + m))
    st = hip.new_state(nx + m, m, lb, ub)
    Ad, Hd = dev(A, hip), dev(chol_cases.spd(nx, 9, cond=10.0), hip)
    if which == "condensed":
        return M.HIPCondensedKKTSystem(hip, st, nx, ineq, Hd, Ad), -1.0
    if which == "normal":
        return M.HIPNormalKKTSystem(hip, st, nx, ineq, None, dev(A.T, hip)), 0.0
    if which == "augmented":
        return M.HIPAugmentedKKTSystem(hip, st, nx, ineq, Hd, Ad), -1.0
    if which == "scaled-augmented":
        return M.HIPScaledAugmentedKKTSystem(hip, st, nx, ineq, Hd, Ad), -1.0
    assert which == "sparse-condensed-packed"
    q = banded_qp(300, 120, 6, 11)
    st = hip.new_state(420, 120, list(range(0, 300, 2)) + list(range(300, 420)), list(range(1, 300, 3)) + list(range(300, 420)))
    return M.HIPSparseCondensedKKTSystem(hip, st, 300, list(range(120)), M.DeviceSymCSR.from_dense(hip.device, q["H"].toarray()),
                                         M.DeviceCSR.from_dense(hip.device, q["A"].toarray()), bandwidth="auto",
                                         storage="packed"), -1.0


def explicit_condition(hip, kkt):
    """2-norm condition of the unreduced KKT operator of the state (kkt.mul on the unit vectors)"""
    st = kkt.st
    E = torch.eye(st.ntot, dtype=torch.float64, device=hip.device)
    out = torch.zeros_like(E)
    for c in range(st.ntot):
        kkt.mul(out[c], E[c], 1.0, 0.0)
    return np.linalg.cond(out.cpu().numpy().T)


# 2-norm condition of the explicit KKT matrix of the states above, measured on the MI355X (the test prints it): condensed,
# augmented and scaled augmented 19.5 (one matrix: order 727), normal 9.3, sparse condensed in packed storage 12.2 (order 1030)
COND_MAX = 1e4


@pytest.mark.parametrize("which", ["condensed", "normal", "augmented", "scaled-augmented", "sparse-condensed-packed"])
def test_kkt_solve_many(hip, which):
    name = which
    kkt, del_c = make_kkt(hip, which)
    try:
        st, nrhs = kkt.st, 5
        kkt.initialize()
        seeded_state(hip, st, kkt.nx, 31)
        kkt.set_aug_diagonal_reg(1.0, del_c)
        kkt.factorize_wrapper()
        assert kkt.linear_solver.is_factorized()
        cond = explicit_condition(hip, kkt)
        print(f"{name}: order {st.ntot}, condition of the explicit KKT matrix {cond:.3e}")
        assert cond < COND_MAX, cond
        ch = hip.kkt_chol(kkt._h)[0]
        hip.chol_set_solve_many_min(ch, 2)
        assert hip.chol_solve_many_info(ch, nrhs)[0] == 1
        ldw = st.ntot + 3
        W0 = np.full((nrhs, ldw), np.nan)
        W0[:, : st.ntot] = np.random.default_rng(4).standard_normal((nrhs, st.ntot))
        for refine in (0, 1):
            kkt.set_refine(refine)
            ref = np.zeros((nrhs, st.ntot))
            for c in range(nrhs):
                w = dev(W0[c, : st.ntot], hip)
                kkt.solve(w)
                ref[c] = w.cpu().numpy()
            W = dev(W0, hip)
            assert kkt.solve_many(W) is W
            out = W.cpu().numpy()
            assert np.array_equal(bits(out[:, st.ntot:]), bits(W0[:, st.ntot:])), "the padding of ldw is untouched"
            worst = max(np.max(np.abs(out[c, : st.ntot] - ref[c])) / np.max(np.abs(ref[c])) for c in range(nrhs))
            print(f"{name} refine={refine}: worst column distance to solve() {worst:.2e}")
            assert worst < 1e-10, worst
            # mul_solved after solve_many has nothing to reuse: it is mul
            a, b = dev(W0[0, : st.ntot], hip), dev(W0[0, : st.ntot], hip)
            kkt.mul_solved(a, W[nrhs - 1, : st.ntot], -1.0, 1.0)
            kkt.mul(b, W[nrhs - 1, : st.ntot], -1.0, 1.0)
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
            # one row is solve itself
            one = dev(W0[:1], hip)
            kkt.solve_many(one)
            assert np.array_equal(bits(one.cpu().numpy()[0, : st.ntot]), bits(ref[0]))
        kkt.set_refine(0)
        assert hip.lib.madqp_kkt_solve_many(kkt._h, C.byref(st.cstruct), M._lib.ptr(W), st.ntot - 1, nrhs) == ERR_ARG
        assert hip.lib.madqp_kkt_solve_many(kkt._h, C.byref(st.cstruct), None, ldw, nrhs) == ERR_ARG
        assert hip.lib.madqp_kkt_solve_many(kkt._h, C.byref(st.cstruct), M._lib.ptr(W), ldw, -1) == ERR_ARG
        assert hip.lib.madqp_kkt_solve_many(kkt._h, C.byref(st.cstruct), None, ldw, 0) == 0
    finally:
        kkt.close()
