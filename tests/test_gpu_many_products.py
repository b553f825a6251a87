"""GPU: the KKT products on a block of vectors -- ``madqp_gemv_many`` (csrc/gemv_many.hip; its launch decode is replayed
without a GPU in tests/test_many_plan.py), the CSR product on a block behind a sparse object's ``mul_many``
(csrc/sparse.hip), ``mul_many`` on every KKT form and ``solve_many`` with block products switched on.

Bounds.  The dense kernel on integers in [-8, 8] must EQUAL numpy (every product and sum is exact in float64).  On normal
data it is held per entry to ``gamma (|alpha| (|A||X|) + |beta||Y0|)``, ``gamma = (K + 4) u / (1 - (K + 4) u)``: the bound of a
sum of K products in ANY order plus the two scalings and their sum.  ``mul_many`` against the column loop over ``mul``:
``2 gamma_p (|alpha| (|K||v|) + |beta||w0|)``, ``p = nx + m + 8`` -- both sides carry at most ``gamma_p`` -- with the explicit
``|K|`` taken from ``mul`` on unit vectors; objects whose A and H are sparse are held bitwise.  ``solve_many`` in block mode:
``err_block <= SENS_FACTOR err_loop + ntot u cond`` against a host solve of the explicit system refined twice with
``np.longdouble`` residuals, ``err_loop`` from the same object with block products off."""
import ctypes as C

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
import gemm_paths
from parity import SENS_FACTOR
from test_gpu_band import bits, dev
from test_gpu_solve_many import COND_MAX, make_kkt, seeded_state
from test_many_plan import operands, plan

pytestmark = pytest.mark.gpu
ERR_ARG = -1
U = 2.0 ** -53
FORMS = ["condensed", "normal", "augmented", "scaled-augmented", "sparse-condensed-packed"]
# (rows, cols, nrhs) of the grid of tests/test_many_plan.py: every edge of the 64-output tile, the 16-column MFMA tile, the
# 128-column group, the 32-wide k step, and both forms of the k ranges (one: direct stores; two: partials and the chain)
EXACT_CASES = [(1, 1, 1), (1, 130, 2), (15, 3, 15), (16, 4, 16), (17, 5, 17), (127, 63, 33), (128, 64, 128), (129, 65, 130),
               (129, 130, 2), (129, 130, 130), (129, 1, 17), (1, 5, 130), (17, 130, 1), (128, 130, 16), (129, 4, 33),
               (15, 64, 128), (127, 63, 15), (127, 130, 17), (16, 65, 2), (128, 5, 33)]


def gamma(k):
    return k * U / (1.0 - k * U)


def run_gemv_many(hip, trans, rows, cols, nrhs, Abuf, lda, Xbuf, ldx, Ybuf, ldy, alpha, beta):
    """the call with A 8 bytes past a 16-byte boundary; returns the whole Y buffer"""
    Ad = gemm_paths.dev(Abuf, hip, shift=1)
    assert Ad.data_ptr() % 16 == 8
    Xd, Yd = dev(Xbuf, hip), dev(Ybuf, hip)
    hip.gemv_many(trans, rows, cols, nrhs, alpha, Ad, lda, Xd, ldx, beta, Yd, ldy)
    return Yd.cpu().numpy()


@pytest.mark.parametrize("trans", [0, 1])
def test_gemv_many_exact(hip, trans):
    for rows, cols, nrhs in EXACT_CASES:
        A, X, Y0, (Abuf, lda), (Xbuf, ldx), (Ybuf, ldy) = operands(trans, rows, cols, nrhs, 100 * rows + 10 * cols + nrhs)
        assert lda % 2 == 1 and lda > cols
        ylen = cols if trans else rows
        for alpha, beta in ((1.0, 0.0), (2.0, -1.0)):
            Yin = Ybuf.copy()
            if beta == 0.0:
                Yin.reshape(nrhs, ldy)[:, :ylen] = np.nan
            out = run_gemv_many(hip, trans, rows, cols, nrhs, Abuf, lda, Xbuf, ldx, Yin, ldy, alpha, beta).reshape(nrhs, ldy)
            want = (A.T if trans else A) @ X
            want = alpha * want if beta == 0.0 else alpha * want + beta * Y0
            tag = (trans, rows, cols, nrhs, alpha, beta, plan(trans, rows, cols, nrhs)["ksplit"])
            assert np.array_equal(out[:, :ylen], want.T), tag
            assert np.array_equal(bits(out[:, ylen:]), bits(Yin.reshape(nrhs, ldy)[:, ylen:])), tag


@pytest.mark.parametrize("trans", [0, 1])
def test_gemv_many_rounding(hip, trans):
    worst = 0.0
    for rows, cols, nrhs in ((200, 130, 17), (129, 65, 33), (17, 130, 130), (128, 64, 2)):
        A, X, Y0, (Abuf, lda), (Xbuf, ldx), (Ybuf, ldy) = operands(trans, rows, cols, nrhs, rows + cols + nrhs, integer=False)
        ylen, klen = (cols, rows) if trans else (rows, cols)
        opA = A.T if trans else A
        exact = opA.astype(np.longdouble) @ X.astype(np.longdouble)
        mag = np.abs(opA) @ np.abs(X)
        g = gamma(klen + 4)
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.3, -0.5)):
            Yin = Ybuf.copy()
            if beta == 0.0:
                Yin.reshape(nrhs, ldy)[:, :ylen] = np.nan  # beta == 0 assigns: the NaN does not survive
            out = run_gemv_many(hip, trans, rows, cols, nrhs, Abuf, lda, Xbuf, ldx, Yin, ldy, alpha, beta).reshape(nrhs, ldy)
            ref = np.longdouble(alpha) * exact + (np.longdouble(beta) * Y0.astype(np.longdouble) if beta else 0)
            bound = g * (abs(alpha) * mag + abs(beta) * np.abs(Y0))
            err = np.abs(out[:, :ylen].T.astype(np.longdouble) - ref)
            worst = max(worst, float(np.max(err / bound)))
            assert np.isfinite(out[:, :ylen]).all() and (err <= bound).all(), (trans, rows, cols, nrhs, alpha, beta)
            assert np.array_equal(bits(out[:, ylen:]), bits(Yin.reshape(nrhs, ldy)[:, ylen:]))
            if beta == 0.0:  # the outcome of madqp_gemv on the same column, its y pre-filled with NaN too
                Ad, xd = dev(A, hip), dev(X[:, 0].copy(), hip)
                yd = torch.full((ylen,), float("nan"), dtype=torch.float64, device=hip.device)
                hip.gemv(trans, rows, cols, alpha, Ad, cols, xd, 0.0, yd)
                one = yd.cpu().numpy()
                assert np.isfinite(one).all()
                assert (np.abs(one - out[0, :ylen]) <= 2 * bound[:, 0]).all()
    print(f"trans={trans}: worst error / bound {worst:.3f}")


def test_gemv_many_refusals_and_empty_shapes(hip):
    lib, p = hip.lib, M._lib.ptr
    A, X, Y = dev(np.ones(12), hip), dev(np.ones(12), hip), dev(np.full(12, np.nan), hip)
    call = lambda *a: lib.madqp_gemv_many(hip.ctx, *a)
    assert call(2, 3, 4, 1, 1.0, p(A), 4, p(X), 4, 0.0, p(Y), 3) == ERR_ARG
    assert call(0, 3, 4, -1, 1.0, p(A), 4, p(X), 4, 0.0, p(Y), 3) == ERR_ARG
    assert call(0, 3, 4, 2, 1.0, p(A), 3, p(X), 4, 0.0, p(Y), 3) == ERR_ARG, "lda < cols"
    assert call(0, 3, 4, 2, 1.0, p(A), 4, p(X), 3, 0.0, p(Y), 3) == ERR_ARG, "ldx < the contraction length"
    assert call(0, 3, 4, 2, 1.0, p(A), 4, p(X), 4, 0.0, p(Y), 2) == ERR_ARG, "ldy < the output length"
    assert call(0, 3, 4, 2, 1.0, None, 4, p(X), 4, 0.0, p(Y), 3) == ERR_ARG
    assert call(0, 3, 4, 0, 1.0, None, 4, None, 4, 0.0, None, 3) == 0, "nrhs = 0 does nothing"
    assert np.isnan(Y.cpu().numpy()).all()
    Y2 = dev(np.arange(12.0), hip)  # no contraction: Y <- beta Y on the stated lengths only
    assert call(0, 3, 0, 2, 1.0, None, 0, None, 0, 2.0, p(Y2), 5) == 0
    want = np.arange(12.0)
    want[[0, 1, 2, 5, 6, 7]] *= 2.0
    assert np.array_equal(Y2.cpu().numpy(), want)


# ---- KKT level ----------------------------------------------------------------------------------------------------------------
class Prepared:
    """an object of make_kkt after a factorisation, with the explicit matrix of its state (mul on unit vectors)"""

    def __init__(self, hip, which):
        self.kkt, del_c = make_kkt(hip, which)
        kkt, st = self.kkt, self.kkt.st
        kkt.initialize()
        seeded_state(hip, st, kkt.nx, 31)
        kkt.set_aug_diagonal_reg(1.0, del_c)
        kkt.factorize_wrapper()
        assert kkt.linear_solver.is_factorized()
        E = torch.eye(st.ntot, dtype=torch.float64, device=hip.device)
        out = torch.zeros_like(E)
        for c in range(st.ntot):
            kkt.mul(out[c], E[c], 1.0, 0.0)
        self.K = out.cpu().numpy().T.copy()
        self.cond = np.linalg.cond(self.K)


@pytest.fixture(scope="module")
def prepared(hip):
    made = {}

    def get(which):
        if which not in made:
            made[which] = Prepared(hip, which)
        return made[which]

    yield get
    for p in made.values():
        p.kkt.close()


def blocks(ntot, nrhs, ldw, ldv, seed):
    rng = np.random.default_rng(seed)
    W0, V0 = np.full((nrhs, ldw), np.nan), np.full((nrhs, ldv), np.nan)
    W0[:, :ntot], V0[:, :ntot] = rng.standard_normal((nrhs, ntot)), rng.standard_normal((nrhs, ntot))
    return W0, V0


def mul_loop(hip, kkt, W0, V0, alpha, beta):
    ntot = kkt.st.ntot
    ref = np.zeros((W0.shape[0], ntot))
    for c in range(W0.shape[0]):
        w, v = dev(W0[c, :ntot], hip), dev(V0[c, :ntot], hip)
        kkt.mul(w, v, alpha, beta)
        ref[c] = w.cpu().numpy()
    return ref


def mul_block(hip, kkt, W0, V0, alpha, beta):
    ntot = kkt.st.ntot
    W, V = dev(W0, hip), dev(V0, hip)
    assert kkt.mul_many(W, V, alpha, beta) is W
    out = W.cpu().numpy()
    assert np.array_equal(bits(out[:, ntot:]), bits(W0[:, ntot:])), "the padding of ldw is untouched"
    assert np.array_equal(bits(V.cpu().numpy()), bits(V0)), "V is read only"
    return out[:, :ntot]


def odd_sparse_object(hip):
    """a sparse condensed object whose CSR Hessian is not banded, has empty rows (100 .. 110) and a row of 41 entries, and
    whose Jacobian has empty rows and a row of 50 entries"""
    rng = np.random.default_rng(5)
    nx, m = 150, 60
    H = np.zeros((nx, nx))
    keep = np.r_[0:100, 111:nx]
    H[keep, keep] = 1.0 + rng.random(len(keep))
    H[40, :40] = rng.standard_normal(40)  # with its diagonal: 41 entries, and column 40 in the rows 0 .. 39
    for i, j in ((149, 3), (120, 7), (99, 0), (130, 60)):
        H[i, j] = rng.standard_normal()
    H = np.tril(H) + np.tril(H, -1).T
    A = np.zeros((m, nx))
    A[7, 50:100] = rng.standard_normal(50)
    for r in range(0, m, 3):
        if r != 6:  # (rows 1, 2, 4, 5, 6, .. stay empty)
            A[r, rng.choice(nx, 4, replace=False)] = rng.standard_normal(4)
    st = hip.new_state(nx + m, m, list(range(0, nx, 2)) + list(range(nx, nx + m)), list(range(1, nx, 3)) + list(range(nx, nx + m)))
    kkt = M.HIPSparseCondensedKKTSystem(hip, st, nx, list(range(m)), M.DeviceSymCSR.from_dense(hip.device, H),
                                        M.DeviceCSR.from_dense(hip.device, A))
    kkt.initialize()
    seeded_state(hip, st, nx, 8)
    kkt.set_aug_diagonal_reg(1.0, -1.0)
    return kkt


def test_csr_products_are_bitwise_the_column_loop(hip, prepared):
    odd = odd_sparse_object(hip)
    try:
        for kkt in (prepared("sparse-condensed-packed").kkt, odd):
            ntot = kkt.st.ntot
            for nrhs in (2, 5, 17):
                for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
                    W0, V0 = blocks(ntot, nrhs, ntot + 3, ntot + 5, nrhs)
                    assert np.array_equal(bits(mul_block(hip, kkt, W0, V0, alpha, beta)), bits(mul_loop(hip, kkt, W0, V0, alpha, beta)))
    finally:
        odd.close()


@pytest.mark.parametrize("which", FORMS)
def test_mul_many(hip, prepared, which):
    pre = prepared(which)
    kkt, st = pre.kkt, pre.kkt.st
    ntot, absK = st.ntot, np.abs(pre.K)
    g = gamma(kkt.nx + kkt.m + 8)
    for nrhs in (2, 5, 17):
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
            W0, V0 = blocks(ntot, nrhs, ntot + 3, ntot + 5, 10 * nrhs + 1)
            ref, out = mul_loop(hip, kkt, W0, V0, alpha, beta), mul_block(hip, kkt, W0, V0, alpha, beta)
            if which == "sparse-condensed-packed":
                assert np.array_equal(bits(out), bits(ref))
                continue
            bound = 2 * g * (abs(alpha) * (np.abs(V0[:, :ntot]) @ absK.T) + abs(beta) * np.abs(W0[:, :ntot]))
            ratio = float(np.max(np.abs(out - ref) / bound))
            print(f"{which} nrhs={nrhs} alpha={alpha} beta={beta}: worst |mul_many - mul| / bound {ratio:.3f}")
            assert np.isfinite(out).all() and ratio <= 1.0
    # one pair of columns IS mul
    W0, V0 = blocks(ntot, 1, ntot + 3, ntot + 5, 3)
    assert np.array_equal(bits(mul_block(hip, kkt, W0, V0, -1.0, 1.0)), bits(mul_loop(hip, kkt, W0, V0, -1.0, 1.0)))
    # the refusals
    W0, V0 = blocks(ntot, 4, ntot + 3, ntot + 5, 4)
    W, V = dev(W0, hip), dev(V0, hip)
    call = lambda *a: hip.lib.madqp_kkt_mul_many(kkt._h, C.byref(st.cstruct), *a)
    p = M._lib.ptr
    assert call(p(W), ntot - 1, p(V), ntot + 5, 4, 1.0, 0.0) == ERR_ARG
    assert call(p(W), ntot + 3, p(V), ntot - 1, 4, 1.0, 0.0) == ERR_ARG
    assert call(None, ntot + 3, p(V), ntot + 5, 4, 1.0, 0.0) == ERR_ARG
    assert call(p(W), ntot + 3, None, ntot + 5, 4, 1.0, 0.0) == ERR_ARG
    assert call(p(W), ntot + 3, p(W), ntot + 3, 4, 1.0, 0.0) == ERR_ARG, "W == V"
    assert call(p(W), ntot + 3, p(V), ntot + 5, -1, 1.0, 0.0) == ERR_ARG
    assert call(None, ntot + 3, None, ntot + 5, 0, 1.0, 0.0) == 0
    assert hip.lib.madqp_kkt_set_block_products(kkt._h, 2) == ERR_ARG
    assert hip.lib.madqp_kkt_many_info(kkt._h, -1, (C.c_int64 * 4)()) == ERR_ARG
    assert hip.lib.madqp_kkt_many_info(kkt._h, 4, None) == ERR_ARG
    hip.sync()
    assert np.array_equal(bits(W.cpu().numpy()), bits(W0)), "a refused call and nrhs = 0 write nothing"
    with pytest.raises(ValueError):
        kkt.mul_many(W, V[:3])
    with pytest.raises(ValueError):
        kkt.mul_many(W, W)
    with pytest.raises(ValueError):
        kkt.mul_many(W[:, : ntot - 1], V)
    # afterwards mul_solved has nothing to reuse: it is mul
    a, b = dev(W0[0, :ntot], hip), dev(W0[0, :ntot], hip)
    kkt.mul_many(W, V, 1.0, 0.0)
    kkt.mul_solved(a, V[0, :ntot], -1.0, 1.0)
    kkt.mul(b, V[0, :ntot], -1.0, 1.0)
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))


def host_reference(K, B):
    """float64 solve of the explicit system, two refinement steps with residuals in np.longdouble"""
    X = np.linalg.solve(K, B)
    Kl, Bl = K.astype(np.longdouble), B.astype(np.longdouble)
    for _ in range(2):
        R = (Bl - Kl @ X.astype(np.longdouble)).astype(np.float64)
        X = X + np.linalg.solve(K, R)
    return X


def worst_error(out, ref):
    return max(np.max(np.abs(out[c] - ref[c])) / np.max(np.abs(ref[c])) for c in range(out.shape[0]))


@pytest.mark.parametrize("which", FORMS)
def test_solve_many_block_products(hip, prepared, which):
    pre = prepared(which)
    kkt, st = pre.kkt, pre.kkt.st
    ntot = st.ntot
    print(f"{which}: order {ntot}, condition of the explicit KKT matrix {pre.cond:.3e}")
    assert pre.cond < COND_MAX, pre.cond
    has_stage_products = which not in ("augmented", "scaled-augmented")
    try:
        for refine in (0, 1):
            kkt.set_refine(refine)
            for nrhs in (5, 17):
                W0 = np.full((nrhs, ntot + 3), np.nan)
                W0[:, :ntot] = np.random.default_rng(40 + nrhs).standard_normal((nrhs, ntot))
                ref = host_reference(pre.K, W0[:, :ntot].T).T

                def solved():
                    W = dev(W0, hip)
                    kkt.solve_many(W)
                    out = W.cpu().numpy()
                    assert np.array_equal(bits(out[:, ntot:]), bits(W0[:, ntot:])), "the padding of ldw is untouched"
                    return out[:, :ntot]

                loop_info = hip.kkt_many_info(kkt._h, nrhs)
                assert loop_info[0] == 0
                loop = solved()  # (the first pass: before the switch was ever set on this object)
                kkt.set_block_products(True)
                info = hip.kkt_many_info(kkt._h, nrhs)
                assert info[0] == 1 and hip.kkt_many_info(kkt._h, 1)[0] == 0
                assert info[1:3] == hip.kkt_many_info(kkt._h, 2)[1:3], "the passes over A and H do not depend on nrhs"
                assert info[1] == (2 if has_stage_products else 0) + 2 * refine
                assert info[2] == (refine if which != "normal" else 0)
                assert loop_info[1] == nrhs * info[1] and loop_info[2] == nrhs * info[2], "in loop mode they grow with it"
                block = solved()
                assert hip.kkt_many_info(kkt._h, nrhs)[3] >= loop_info[3]
                kkt.set_block_products(False)
                assert hip.kkt_many_info(kkt._h, nrhs)[0] == 0
                assert np.array_equal(bits(solved()), bits(loop)), "switched back off: the bits of the loop path"
                err_loop, err_block = worst_error(loop, ref), worst_error(block, ref)
                print(f"{which} refine={refine} nrhs={nrhs}: err_loop {err_loop:.3e} err_block {err_block:.3e} cond {pre.cond:.3e}")
                assert np.isfinite(block).all()
                assert err_block <= SENS_FACTOR * err_loop + ntot * U * pre.cond
                if which == "sparse-condensed-packed":
                    assert np.array_equal(bits(block), bits(loop)), "sparse A and H: block mode is bitwise loop mode"
    finally:
        kkt.set_block_products(False)
        kkt.set_refine(0)
