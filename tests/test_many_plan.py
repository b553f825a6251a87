"""CPU: the launch decode of the dense product on a block of vectors (madqp_jl_amd/csrc/many_plan.inc, compiled for the CPU
by tests/csrc_many).  The kernel of madqp_jl_amd/csrc/gemv_many.hip is replayed in numpy FROM THE PLAN -- the jobs of the
workgroups, the staging slots of the threads, the k each lane feeds to the MFMA, the column each accumulator register
holds, the index functions -- with the one hardware fact the plan relies on stated here (``mfma_16x16x4``: lane l holds
A[l & 15][l >> 4] and B[l >> 4][l & 15], register g of lane l holds D[(l >> 4) + 4 g][l & 15]).  On small-integer data every
product and sum is exact in float64, so the replayed result must EQUAL ``A @ X``; the operands carry NaN in every padding
slot, every generated index is checked against rows x cols of A and the column lengths of X and Y, and every output is
owned by exactly one workgroup or one ordered chain of partial sums.  The kernel itself is held in
tests/test_gpu_many_products.py; the ABI refusals that need no device are here too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import madqp_jl_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 15, 16, 17, 127, 128, 129, 200)
COLS = (1, 3, 4, 5, 63, 64, 65, 130)
NRHS = (1, 2, 15, 16, 17, 33, 128, 130)
PLAN_FIELDS = ("trans", "ylen", "klen", "nrhs", "row_tiles", "col_groups", "ksplit", "kchunk", "workgroups", "partial_doubles")

_lib = None
_tab = None


def many_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_many")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_manyplan.so"))
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        for name, args in (("many_plan_c", [i32, i64, i64, i64, vp]), ("many_jobs_c", [i32, i64, i64, i64, vp]),
                           ("many_tables_c", [vp] * 6), ("many_a_index_c", [i32, i64, vp, vp, i64, vp]),
                           ("many_x_index_c", [i64, vp, vp, i64, vp]), ("many_y_index_c", [i64, vp, vp, i64, vp]),
                           ("many_partial_index_c", [i32, i64, i64, i64, i64, vp, vp, vp, vp])):
            getattr(_lib, name).restype = None
            getattr(_lib, name).argtypes = args
    return _lib


def plan(trans, rows, cols, nrhs):
    out = np.zeros(10, dtype=np.int64)
    many_lib().many_plan_c(trans, rows, cols, nrhs, out.ctypes.data)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def jobs(trans, rows, cols, nrhs):
    out = np.zeros((plan(trans, rows, cols, nrhs)["workgroups"], 7), dtype=np.int64)
    many_lib().many_jobs_c(trans, rows, cols, nrhs, out.ctypes.data)
    return out


def tables():
    global _tab
    if _tab is None:
        consts = np.zeros(6, dtype=np.int64)
        a_slot = np.zeros((2, 256, 8, 2), dtype=np.int32)
        x_slot = np.zeros((256, 16, 2), dtype=np.int32)
        lane_rc, lane_k, acc_col = (np.zeros(s, dtype=np.int32) for s in ((64,), (8, 64), (64, 4)))
        many_lib().many_tables_c(consts.ctypes.data, a_slot.ctypes.data, x_slot.ctypes.data, lane_rc.ctypes.data,
                                 lane_k.ctypes.data, acc_col.ctypes.data)
        assert tuple(consts) == (64, 128, 32, 8, 16, 8), "the table shapes above follow the constants of many_plan.inc"
        _tab = dict(TR=64, TC=128, TK=32, a_slot=a_slot, x_slot=x_slot, lane_rc=lane_rc, lane_k=lane_k, acc_col=acc_col)
    return _tab


def _index(fn, *args):
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in args if isinstance(a, np.ndarray)]
    out = np.zeros(len(arrs[0]), dtype=np.int64)
    fn(out, arrs)
    return out


def a_index(trans, y, k, lda):
    return _index(lambda out, a: many_lib().many_a_index_c(trans, len(out), a[0].ctypes.data, a[1].ctypes.data, lda, out.ctypes.data), y, k)


def x_index(k, c, ldx):
    return _index(lambda out, a: many_lib().many_x_index_c(len(out), a[0].ctypes.data, a[1].ctypes.data, ldx, out.ctypes.data), k, c)


def y_index(y, c, ldy):
    return _index(lambda out, a: many_lib().many_y_index_c(len(out), a[0].ctypes.data, a[1].ctypes.data, ldy, out.ctypes.data), y, c)


def partial_index(shape, split, y, c):
    trans, rows, cols, nrhs = shape
    return _index(lambda out, a: many_lib().many_partial_index_c(trans, rows, cols, nrhs, len(out), a[0].ctypes.data,
                                                                 a[1].ctypes.data, a[2].ctypes.data, out.ctypes.data), split, y, c)


LANE = np.arange(64)
MFMA_OUTER, MFMA_K = LANE & 15, LANE >> 4  # the operand maps of v_mfma_f64_16x16x4_f64 (one f64 per lane per operand)
MFMA_DROW = MFMA_K[:, None] + 4 * np.arange(4)[None, :]  # register g of lane l: row (l >> 4) + 4 g, column l & 15 of D


def store(y, alpha, s, beta):
    """madqp_gemv's rule: beta == 0 assigns"""
    return alpha * s if beta == 0.0 else alpha * s + beta * y


def replay(trans, rows, cols, nrhs, Abuf, lda, Xbuf, ldx, Ybuf, ldy, alpha, beta):
    """The kernels of gemv_many.hip from the plan; returns (Y buffer, ownership count per slot of the Y buffer)."""
    T = tables()
    TR, TC, TK = T["TR"], T["TC"], T["TK"]
    p = plan(trans, rows, cols, nrhs)
    ylen, klen, ksplit = p["ylen"], p["klen"], p["ksplit"]
    Y = Ybuf.copy()
    own_y = np.zeros(len(Y), dtype=np.int64)
    partial = np.full(p["partial_doubles"], np.nan)
    own_p = np.zeros(p["partial_doubles"], dtype=np.int64)
    ar, ak = T["a_slot"][trans, :, :, 0].ravel().astype(np.int64), T["a_slot"][trans, :, :, 1].ravel().astype(np.int64)
    xr, xk = T["x_slot"][:, :, 0].ravel().astype(np.int64), T["x_slot"][:, :, 1].ravel().astype(np.int64)
    rc, lk, ac = T["lane_rc"].astype(np.int64), T["lane_k"].astype(np.int64), T["acc_col"].astype(np.int64)
    waves = np.arange(4)
    for row0, jrows, col0, jcols, k0, k1, split in jobs(trans, rows, cols, nrhs):
        assert 0 <= row0 and row0 + jrows <= ylen and 0 <= col0 and col0 + jcols <= nrhs and 0 <= k0 < k1 <= klen
        nct = (jcols + 15) // 16
        tiles = np.arange(nct)
        acc = np.zeros((4, nct, 64, 4))
        for kb in range(k0, k1, TK):
            As, Xs = np.full((TR, TK), np.nan), np.full((TC, TK), np.nan)
            ok = (ar < jrows) & (kb + ak < k1)
            idx = a_index(trans, row0 + ar[ok], kb + ak[ok], lda)
            assert idx.min() >= 0 and (idx // lda).max() < rows and (idx % lda).max() < cols, "a load outside rows x cols of A"
            vals = np.zeros(len(ar))
            vals[ok] = Abuf[idx]
            As[ar, ak] = vals
            ok = (xr < jcols) & (kb + xk < k1)
            idx = x_index(kb + xk[ok], col0 + xr[ok], ldx)
            assert idx.min() >= 0 and (idx // ldx).max() < nrhs and (idx % ldx).max() < klen, "a load outside a column of X"
            vals = np.zeros(len(xr))
            vals[ok] = Xbuf[idx]
            wr = xr < 16 * nct
            Xs[xr[wr], xk[wr]] = vals[wr]
            # the MFMA steps: the columns are the instruction's first (row) operand, the outputs its second (column) operand
            a = As[16 * waves[:, None, None] + rc[None, None, :], lk[None, :, :]]  # (wave, step, lane)
            b = Xs[16 * tiles[:, None, None] + rc[None, None, :], lk[None, :, :]]  # (tile, step, lane)
            Aop, Bop = np.zeros((nct, 8, 16, 4)), np.zeros((4, 8, 4, 16))
            Aop[:, :, MFMA_OUTER, MFMA_K] = b
            Bop[:, :, MFMA_K, MFMA_OUTER] = a
            D = np.einsum("jsik,wskn->wjin", Aop, Bop)
            acc += D[:, :, MFMA_DROW, MFMA_OUTER[:, None]]
        yl = (16 * waves[:, None, None, None] + rc[None, None, :, None]) + np.zeros((4, nct, 64, 4), dtype=np.int64)
        c = (16 * tiles[None, :, None, None] + ac[None, None, :, :]) + np.zeros((4, nct, 64, 4), dtype=np.int64)
        ok = (yl < jrows) & (c < jcols)
        yy, cc, ss = row0 + yl[ok], col0 + c[ok], acc[ok]
        if ksplit == 1:
            idx = y_index(yy, cc, ldy)
            assert idx.min() >= 0 and (idx // ldy).max() < nrhs and (idx % ldy).max() < ylen, "a store outside a column of Y"
            np.add.at(own_y, idx, 1)
            Y[idx] = store(Y[idx], alpha, ss, beta)
        else:
            idx = partial_index((trans, rows, cols, nrhs), np.full(len(yy), split), yy, cc)
            assert idx.min() >= 0 and idx.max() < len(partial)
            np.add.at(own_p, idx, 1)
            partial[idx] = ss
    if ksplit > 1:  # the reduce kernel: the k ranges of one output in range order
        assert (own_p == 1).all(), "every (k range, output, column) is written by exactly one workgroup"
        yy, cc = (g.ravel() for g in np.meshgrid(np.arange(ylen), np.arange(nrhs), indexing="ij"))
        tot = np.zeros(len(yy))
        for s in range(ksplit):
            tot = tot + partial[partial_index((trans, rows, cols, nrhs), np.full(len(yy), s), yy, cc)]
        idx = y_index(yy, cc, ldy)
        np.add.at(own_y, idx, 1)
        Y[idx] = store(Y[idx], alpha, tot, beta)
    return Y, own_y


def operands(trans, rows, cols, nrhs, seed, integer=True):
    """(A, X, Y0) and their NaN-padded buffers (Abuf, lda), (Xbuf, ldx), (Ybuf, ldy)"""
    rng = np.random.default_rng(seed)
    draw = (lambda s: rng.integers(-8, 9, s).astype(np.float64)) if integer else rng.standard_normal
    ylen, klen = (cols, rows) if trans else (rows, cols)
    A, X, Y0 = draw((rows, cols)), draw((klen, nrhs)), draw((ylen, nrhs))
    lda, ldx, ldy = cols + 3 + (cols % 2), klen + 2, ylen + 5  # (an odd lda)
    Abuf, Xbuf, Ybuf = np.full(rows * lda, np.nan), np.full(nrhs * ldx, np.nan), np.full(nrhs * ldy, np.nan)
    Abuf.reshape(rows, lda)[:, :cols] = A
    Xbuf.reshape(nrhs, ldx)[:, :klen] = X.T
    Ybuf.reshape(nrhs, ldy)[:, :ylen] = Y0.T
    return A, X, Y0, (Abuf, lda), (Xbuf, ldx), (Ybuf, ldy)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
def test_plan_replay_is_exact(trans, rows):
    for cols in COLS:
        for nrhs in NRHS:
            A, X, Y0, (Abuf, lda), (Xbuf, ldx), (Ybuf, ldy) = operands(trans, rows, cols, nrhs, 7 * rows + cols + nrhs)
            alpha, beta = ((1.0, 0.0), (2.0, -1.0))[(cols + nrhs) % 2]
            ylen = cols if trans else rows
            if beta == 0.0:
                Ybuf.reshape(nrhs, ldy)[:, :ylen] = np.nan  # beta == 0 assigns: Y is not read
            p = plan(trans, rows, cols, nrhs)
            assert p["ylen"] == ylen and p["col_groups"] == (nrhs + 127) // 128, "A is read ceil(nrhs / 128) times"
            assert p["workgroups"] == p["row_tiles"] * p["col_groups"] * p["ksplit"] and p["kchunk"] % 32 == 0
            Y, own = replay(trans, rows, cols, nrhs, Abuf, lda, Xbuf, ldx, Ybuf, ldy, alpha, beta)
            tag = (trans, rows, cols, nrhs)
            assert np.array_equal(own.reshape(nrhs, ldy)[:, :ylen], np.ones((nrhs, ylen), dtype=np.int64)), tag
            assert not own.reshape(nrhs, ldy)[:, ylen:].any(), tag
            want = (A.T if trans else A) @ X
            want = alpha * want if beta == 0.0 else alpha * want + beta * Y0
            assert np.array_equal(Y.reshape(nrhs, ldy)[:, :ylen], want.T), tag
            assert np.isnan(Y.reshape(nrhs, ldy)[:, ylen:]).all(), tag


def test_k_ranges_split_and_chain():
    """shapes of the grid reach both forms: one k range (a direct store) and several (partials and the ordered chain)"""
    assert plan(0, 200, 130, 2)["ksplit"] == 2 and plan(1, 200, 130, 2)["ksplit"] == 2
    assert plan(0, 200, 65, 2)["ksplit"] == 1 and plan(0, 200, 65, 2)["partial_doubles"] == 0
    big = plan(0, 2000, 5000, 64)
    assert big["col_groups"] == 1 and big["ksplit"] > 1 and big["partial_doubles"] == big["ksplit"] * 64 * 2000
    assert plan(0, 0, 5, 3)["workgroups"] == 0 and plan(1, 5, 5, 0)["workgroups"] == 0


def test_plan_walk_under_sanitizers():
    """the stand-alone program of tests/csrc_many (address and undefined-behaviour sanitizers), once"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_many"), "check"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "many_plan_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]


def test_abi_refusals_without_a_device():
    lib = M.load_cdll()
    assert lib.madqp_gemv_many(None, 0, 1, 1, 1, 1.0, None, 1, None, 1, 0.0, None, 1) == -1  # MADQP_ERR_ARG
    assert lib.madqp_kkt_mul_many(None, None, None, 1, None, 1, 1, 1.0, 0.0) == -1
    assert lib.madqp_kkt_set_block_products(None, 1) == -1
    assert lib.madqp_kkt_many_info(None, 1, None) == -1
