"""GPU: the failure report of madqp_chol_factor -- the first column whose pivot is not positive, or NaN -- held to LAPACK's
dpotrf in every schedule, and what a failed factorisation leaves behind.  That word drives the x100 regularisation retry of
every driver and the inertia a KKT object reports; nothing crashes when it is wrong.  The matrices, the expected columns and
the proof that every case is far from the border are in tests/chol_cases.py and tests/test_chol_cases.py (no GPU).

How chol_factor_enqueue (chol.hip) is reached, in the order it decides:
  mid-size   no bandwidth, 128 < n <= MADQP_CHOL_MID_MAX (13 312), no signature, lda >= ceil128(n) and even, A 16-byte
             aligned: chol_mid_step_kernel, one step per 128-column block -- the `padded` layout;
  left       everything else, the handle's plan (chol_plan.inc): outer panels (1024 columns first) and their halvings -- the
             `unpadded` layout (lda < ceil128(n): no order of the table above 128 is a multiple of 128), a signature
             (quasi-definite mode), MADQP_CHOL_MID_MAX=0 in a process of its own, the panel pieces (madqp_chol_factor_panel),
             and, cut down to the band, a bandwidth (madqp_chol_set_bandwidth): dense or packed storage, every n;
  one block  n <= 128 is a single launch of the diagonal kernel in either layout."""
import functools
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import madqp_jl_amd as M
import chol_cases as cc
from band_cases import band_spd, banded_qp, pack
from oracle import qp as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"unpadded": cc.unpadded, "padded": cc.padded}
REG = M.FixedRegularization(1e-8, -1e-8)


def dev(a, be):
    return torch.as_tensor(np.ascontiguousarray(a), device=be.device)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dpotrf_info(K):
    return int(sla.lapack.dpotrf(K, lower=1)[1])


@functools.lru_cache(maxsize=None)
def expected(n, cols):
    """dpotrf's report for the table's matrix of order n planted at cols (computed once per case)"""
    info = dpotrf_info(cc.plant(cc.good(n), cols))
    assert info == min(cols) + 1
    return info


@functools.lru_cache(maxsize=None)
def good_factor(n):
    return sla.cholesky(cc.good(n), lower=True)


@functools.lru_cache(maxsize=None)
def rhs(n, k):
    return np.random.default_rng(1000 * n + k).standard_normal(n)


def lower_of(out, n):
    """the lower triangle of an (n, lda) buffer read back from the device"""
    return np.tril(out[:, :n].T)


_fresh = {}


def fresh(hip, n, layout):
    """(the whole buffer, the solutions of rhs(n, 0) and rhs(n, 1)) a NEW handle leaves for the good matrix of order n in
    this layout, on a poisoned buffer -- what every reused handle is compared with, bit for bit.  Computed once."""
    if (n, layout) not in _fresh:
        lda = LAYOUTS[layout](n)
        h = hip.chol_create(n)
        try:
            Kd = dev(cc.poisoned(cc.good(n), lda), hip)
            assert hip.chol_factor(h, Kd, lda) == 0
            xs = []
            for k in (0, 1):
                bd = dev(rhs(n, k), hip)
                hip.chol_solve(h, bd)
                xs.append(bd.cpu().numpy())
            _fresh[(n, layout)] = (Kd.cpu().numpy(), xs)
        finally:
            hip.chol_destroy(h)
    return _fresh[(n, layout)]


# ---- A: every schedule reports LAPACK's column -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_every_schedule_reports_lapacks_column(hip, case, layout):
    """The table of tests/chol_cases.py through madqp_chol_factor.  n <= 128: one block, in both layouts.  n > 128,
    `unpadded` (lda = n + 2 or 3 < ceil128(n)): the left-looking driver in this process.  n > 128, `padded`
    (lda = ceil128(n) + 2): the mid-size schedule -- 9 steps at 1100, 20 at 2500 (other unit lists from 20 blocks on).
    With two planted columns the report is the first: the launches of a factorisation are in stream order, and the word
    is written by atomicCAS(info, 0, column) only."""
    n, cols = case
    lda = LAYOUTS[layout](n)
    h = hip.chol_create(n)
    try:
        Kd = dev(cc.lower_only(cc.plant(cc.good(n), cols), lda), hip)
        assert hip.chol_factor(h, Kd, lda) == expected(n, cols)
    finally:
        hip.chol_destroy(h)


# ---- B: the left-looking driver at the padded layout -----------------------------------------------------------------------
def test_left_looking_driver_at_the_padded_layout():
    """MADQP_CHOL_MID_MAX=0 (read once per process, hence the child; tests/test_gpu_dense.py::
    test_left_looking_driver_at_small_orders) sends the padded layout to the left-looking driver: whole-tile reads up to the
    padded order, the rows 300, 1100 and 2500 of the table and their good matrices."""
    code = textwrap.dedent('''
        import json, sys
        import numpy as np, torch
        sys.path[:0] = [%r, %r]
        import madqp_jl_amd as M
        import chol_cases as cc
        be = M.HipBackend(0)
        out = {}
        for n in (300, 1100, 2500):
            lda = cc.padded(n)
            h = be.chol_create(n)
            for case in [c for c in cc.CASES if c[0] == n] + [(n, ())]:
                Kd = torch.as_tensor(cc.lower_only(cc.plant(cc.good(n), case[1]), lda), device=be.device)
                out[cc.case_id(case)] = int(be.chol_factor(h, Kd, lda))
            be.chol_destroy(h)
        be.close()
        print(json.dumps(out))
    ''') % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MADQP_CHOL_MID_MAX="0"), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    want = {cc.case_id(case): expected(*case) for case in cc.CASES if case[0] in (300, 1100, 2500)}
    want.update({cc.case_id((n, ())): 0 for n in (300, 1100, 2500)})
    print(res)
    assert res == want


# ---- C: the band schedule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["dense", "packed"])
@pytest.mark.parametrize("n,bw", cc.BAND_SHAPES)
def test_band_schedule_reports_lapacks_column(hip, n, bw, storage):
    """madqp_chol_set_bandwidth on dense storage (both layouts) and on packed storage (madqp_chol_packed_layout /
    madqp_chol_set_packed): column 0, both sides of a 128-column block edge, the last column; expected from dpotrf of the
    dense matrix.  One handle per shape and storage takes all the columns and then the good matrix."""
    K = band_spd(n, bw)
    cols = cc.band_columns(n, bw)
    want = {c: dpotrf_info(cc.plant(K, [c])) for c in cols}
    assert want == {c: c + 1 for c in cols}
    want[None] = 0
    h = hip.chol_create(n)
    try:
        hip.chol_set_bandwidth(h, bw)
        if storage == "packed":
            extent = hip.chol_band_extent(h)
            ld, doubles = hip.chol_packed_layout(h)
            hip.chol_set_packed(h)
            make = [(ld, lambda Mx: pack(np.tril(Mx), extent, ld, doubles)[0])]
        else:
            make = [(f(n), lambda Mx, lda=f(n): cc.lower_only(Mx, lda)) for f in LAYOUTS.values()]
        for lda, build in make:
            got = {c: hip.chol_factor(h, dev(build(K if c is None else cc.plant(K, [c])), hip), lda) for c in list(cols) + [None]}
            assert got == want, (storage, lda)
    finally:
        hip.chol_destroy(h)


# ---- D: quasi-definite mode ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quasidefinite(npos, nneg, c=None):
    return cc.quasidefinite(npos, nneg, npos + nneg, c)


def factor_quasidefinite(hip, stored, npos):
    n = stored.shape[0]
    lda = cc.ceil128(n)
    A = torch.zeros((lda, lda), dtype=torch.float64, device=hip.device)  # column-major: A[j, i] = element (i, j)
    A[:n, :n] = torch.as_tensor(np.tril(stored).T.copy(), device=hip.device)
    h = hip.chol_create(n)
    try:
        hip.chol_set_signature(h, npos)
        return hip.chol_factor(h, A, lda)
    finally:
        hip.chol_destroy(h)


@pytest.mark.parametrize("npos,nneg,c", cc.QD_SECOND_BLOCK)
def test_quasidefinite_failure_in_the_second_block(hip, npos, nneg, c):
    """[P, 0; B, +Q] with Q = S_t - B P^-1 B' and S_t[c, c] = -1: the Schur complement the second block is factored from
    is S_t, the report npos + c + 1 (tests/chol_cases.py: quasidefinite) -- the first and last column of a short second
    block, both sides of a block edge and the last column of a second block of three."""
    stored, Mfull = quasidefinite(npos, nneg, c)
    want = cc.first_failing_column(Mfull, npos)[0]
    assert want == npos + c + 1
    assert factor_quasidefinite(hip, stored, npos) == want


@pytest.mark.parametrize("npos,nneg,c", cc.QD_FIRST_BLOCK)
def test_quasidefinite_failure_in_the_positive_block(hip, npos, nneg, c):
    """a failure inside P -- column 0, the end of the first 128-column block, and npos - 1, the last column before the
    signs change"""
    stored, Mfull = quasidefinite(npos, nneg)
    want = cc.first_failing_column(cc.plant(Mfull, [c]), npos)[0]
    assert want == c + 1
    assert factor_quasidefinite(hip, cc.plant(stored, [c]), npos) == want
    if c == 0:
        assert factor_quasidefinite(hip, stored, npos) == cc.first_failing_column(Mfull, npos)[0] == 0


# ---- E: the panel pieces ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 128, 639])
def test_panel_pieces_report_lapacks_column(hip, c):
    """madqp_chol_factor_begin / _panel(0, 640) / madqp_chol_panel_pack(0, 640, buf): the header of the packed image is
    [info as a double, 0.0].  buf (include/madqp.h): 2 + ceil(w / 128) * 2 * 128 * 128 + w * (n - j0) doubles."""
    n = 640
    K = cc.spd(n, n)
    want = dpotrf_info(cc.plant(K, [c]))
    assert want == c + 1
    lib, ptr = hip.lib, M._lib.ptr
    h = hip.chol_create(n)
    try:
        for Mx, info in ((cc.plant(K, [c]), want), (K, 0)):  # ... and factor_begin clears the word for the next one
            Kd = dev(cc.lower_only(Mx, n), hip)
            buf = torch.full((2 + (n + 127) // 128 * 2 * 128 * 128 + n * n,), -7.0, dtype=torch.float64, device=hip.device)
            hip._ck(lib.madqp_chol_factor_begin(h, ptr(Kd), n))
            hip._ck(lib.madqp_chol_factor_panel(h, 0, n))
            hip._ck(lib.madqp_chol_panel_pack(h, 0, n, ptr(buf)))
            hip.sync()
            hdr = buf[:2].cpu().numpy()
            assert hdr[0] == float(info) and hdr[1] == 0.0 and not np.signbit(hdr[1]), hdr
    finally:
        hip.chol_destroy(h)


# ---- F: NaN ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", list(cc.NAN_ORDERS))
def test_nan_is_reported(hip, n, layout):
    """`!(akk > 0.0)` (diag16_factor_invert) catches NaN.  A NaN at (c, c) must report exactly c + 1: before pivot c it can
    only have reached row c.  A NaN at (r, c), r = c + 3, must report a column in [1, r + 1], never 0: r + 1 is what the
    reference loop gives (tests/test_chol_cases.py::test_nan_reference) -- the NaN enters column c of the factor in row r
    and meets its first pivot at a_rr -- while a tile product of a zero with the NaN may poison other entries of row r
    earlier, but no other row.  (On an MI355X every case here reports r + 1, in both layouts; the figures are printed.)
    LAPACK is no reference here (tests/chol_cases.py).  Columns: one inside a block, one whose r lies in the next block.
    The good matrix on the same handle afterwards reports 0."""
    K = cc.good(n)
    lda = LAYOUTS[layout](n)
    h = hip.chol_create(n)
    try:
        for c in cc.NAN_ORDERS[n]:
            r = c + 3
            info_d = hip.chol_factor(h, dev(cc.lower_only(cc.plant(K, [c], np.nan), lda), hip), lda)
            info_o = hip.chol_factor(h, dev(cc.lower_only(cc.plant_offdiag(K, r, c), lda), hip), lda)
            print(f"n={n} {layout} c={c}: NaN at (c, c) -> {info_d} (c + 1 = {c + 1}); NaN at ({r}, c) -> {info_o} (r + 1 = {r + 1})")
            assert info_d == c + 1
            assert 1 <= info_o <= r + 1
        assert hip.chol_factor(h, dev(cc.lower_only(K, lda), hip), lda) == 0
    finally:
        hip.chol_destroy(h)


# ---- G: what a failed factorisation leaves behind --------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["bad-good", "good-bad-good"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n,c", [(300, 200), (300, 290), (1100, 200), (1100, 1050)])  # c in the second block / in the last
def test_what_a_failed_factorisation_leaves_behind(hip, n, c, layout, order):
    """1. On a poisoned buffer every NaN of the strict upper triangle and of the rows past n is still that NaN, bit for
    bit: the failure path writes the lower triangle only.  2. The columns left of c are those of the good matrix's factor
    ("completed with unit pivots from column info on"), at the suite's 1e-11 relative to max |L_ref|.  3. The same handle
    then factors the good matrix: the report is 0, and the factor and the solution of one right-hand side have the bits of
    a fresh handle's -- d_info, upper_ok, the U = L' copy, the sweep images and the tickets all belong to the new factor."""
    K, Lref = cc.good(n), good_factor(n)
    lda = LAYOUTS[layout](n)
    ref_buf, ref_x = fresh(hip, n, layout)
    h = hip.chol_create(n)

    def good_round():
        Kd, bd = dev(cc.poisoned(K, lda), hip), dev(rhs(n, 0), hip)
        assert hip.chol_factor(h, Kd, lda) == 0
        hip.chol_solve(h, bd)
        assert np.array_equal(bits(Kd.cpu().numpy()), bits(ref_buf)), "the factor: the bits of a fresh handle's"
        assert np.array_equal(bits(bd.cpu().numpy()), bits(ref_x[0])), "the solution: the bits of a fresh handle's"

    try:
        if order == "good-bad-good":
            good_round()
        host = cc.poisoned(cc.plant(K, [c]), lda)
        Kd = dev(host, hip)
        assert hip.chol_factor(h, Kd, lda) == expected(n, (c,))
        out = Kd.cpu().numpy()
        was_nan = np.isnan(host)
        assert np.array_equal(bits(out[was_nan]), bits(host[was_nan])), "every NaN is still that NaN"
        L = lower_of(np.where(was_nan, 0.0, out), n)
        far = np.max(np.abs(L[:, :c] - Lref[:, :c])) / np.max(np.abs(Lref))
        print(f"n={n} c={c} {layout}: columns left of c, max|L - Lref| / max|Lref| = {far:.2e}")
        assert far < 1e-11
        good_round()
    finally:
        hip.chol_destroy(h)


# ---- H: one handle across schedules, no failure ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1100])
def test_one_handle_across_schedules(hip, n):
    """padded (mid-size), unpadded (left-looking), padded again on ONE handle; after each factorisation two right-hand sides
    and the first one again (tickets and partial-sum slots are reset per solve).  Every factor and every solution has the
    bits of a fresh handle's made for that layout alone, and every solution meets the bars of
    tests/test_gpu_dense.py::test_cholesky_factor_and_solve against scipy's cho_solve."""
    K, Lref = cc.good(n), good_factor(n)
    h = hip.chol_create(n)
    try:
        for layout in ("padded", "unpadded", "padded"):
            lda = LAYOUTS[layout](n)
            ref_buf, ref_x = fresh(hip, n, layout)
            Kd = dev(cc.poisoned(K, lda), hip)
            assert hip.chol_factor(h, Kd, lda) == 0
            assert np.array_equal(bits(Kd.cpu().numpy()), bits(ref_buf)), layout
            for k in (0, 1, 0):
                b = rhs(n, k)
                bd = dev(b, hip)
                hip.chol_solve(h, bd)
                x = bd.cpu().numpy()
                assert np.array_equal(bits(x), bits(ref_x[k])), (layout, k)
                xref = sla.cho_solve((Lref, True), b)
                assert np.linalg.norm(K @ x - b) / (np.linalg.norm(K) * np.linalg.norm(x)) < 1e-14
                assert np.linalg.norm(x - xref) / np.linalg.norm(xref) < 1e-10
    finally:
        hip.chol_destroy(h)


# ---- I: through a KKT object -----------------------------------------------------------------------------------------------
def free_variable(H, A, q, lvar, uvar, c):
    """variable c becomes free with curvature -1e3 and leaves every row of A and every other row of H (the retry_qp of
    tests/test_gpu_solver.py): column c of the condensed matrix is -1e3 + del_w on the diagonal and zero elsewhere"""
    A[:, c] = 0.0
    H[c, :] = H[:, c] = 0.0
    H[c, c] = -1e3
    q[c] = 0.0
    lvar[c], uvar[c] = -np.inf, np.inf


def assert_kkt_reports(hip, s, K, c, nx):
    Ks = np.tril(K) + np.tril(K, -1).T
    want = dpotrf_info(Ks)
    assert want == c + 1 and Ks[c, c] < -1.0
    ls = s.kkt.linear_solver
    ls.factorize()
    assert ls.info == want and not ls.is_factorized()
    assert ls.inertia(nx) == (c, 0, 1)
    s.kkt.set_aug_diagonal_reg(1e4, -1e-8)  # the next build and factorisation on the object start clean
    s.kkt.factorize_wrapper()
    assert ls.info == 0 and ls.inertia(nx) == (nx, 0, 0)


def test_dense_kkt_object_reports_the_column(hip):
    """HIPCondensedKKTSystem, nx = 200, m = 80: K is read back after set_aug_diagonal_reg(1e-8, -1e-8) and build_kkt,
    dpotrf runs on the host, linear_solver.factorize() must report that column and inertia() (c, 0, 1)."""
    nx, m, c = 200, 80, 130
    qp = Q.synthetic_qp(91, nx, m)
    free_variable(qp.H, qp.A, qp.q, qp.lvar, qp.uvar, c)
    dq = M.DeviceQP.from_numpy(hip.device, qp.H, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0)
    s = M.MPCSolver(dq, hip, kkt_system="condensed", regularization=REG)
    try:
        s.initialize()
        assert type(s.kkt) is M.HIPCondensedKKTSystem
        s.kkt.set_aug_diagonal_reg(1e-8, -1e-8)
        s.kkt.build_kkt()
        ptr, ld = hip.kkt_matrix(s.kkt._h, nx)
        K = hip.read_doubles(ptr, ld * nx).reshape(nx, ld)[:, :nx].T  # [i, j] = K[i + j * ld]
        assert_kkt_reports(hip, s, K, c, nx)
    finally:
        s.close()


def test_packed_sparse_kkt_object_reports_the_column(hip):
    """HIPSparseCondensedKKTSystem with storage="packed" on a banded QP: the band schedule on packed storage behind
    madqp_kkt_factorize; K through dense_matrix() (madqp_band_expand)."""
    nx, m, c = 300, 120, 200
    q = banded_qp(nx, m, 6, 41)
    H, A = q["H"].toarray(), q["A"].toarray()
    free_variable(H, A, q["q"], q["lvar"], q["uvar"], c)
    dq = M.DeviceQP.from_numpy(hip.device, None, q["q"], A, q["lvar"], q["uvar"], q["lcon"], q["ucon"], q["x0"], sparse=True)
    dq.H = M.DeviceSymCSR.from_dense(hip.device, H)
    s = M.MPCSolver(dq, hip, kkt_system="condensed", regularization=REG, kkt_bandwidth="auto", kkt_storage="packed")
    try:
        s.initialize()
        assert type(s.kkt) is M.HIPSparseCondensedKKTSystem and hip.kkt_storage(s.kkt._h)[0]
        s.kkt.set_aug_diagonal_reg(1e-8, -1e-8)
        s.kkt.build_kkt()
        assert_kkt_reports(hip, s, s.kkt.dense_matrix(), c, nx)
    finally:
        s.close()
