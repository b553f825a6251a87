"""GPU: the dense workgroup helpers of the batched engine (csrc/batch_wg.inc), the pre-write of a shared H (csrc/batch.hip)
and the batched Cholesky (csrc/chol.hip: madqp_chol_factor_batched), each on its own against a plain reference of the same
operation -- through the test seams madqp_debug_batch_op and madqp_debug_chol_factor_batched.

The end-to-end tests of the engine (tests/test_gpu_batched*.py) solve whole QPs: an interior-point iteration corrects
itself, so a product that drops a term at one shape still converges inside their tolerances.  Here
  * every product is held to the bound DERIVED in tests/batched_ops.py ((len + 4) u S against an extended-precision
    reference, twice that against float64 numpy), at the shapes where the helpers change form: the row-split and the G == 1
    form of wg_gemv_t, partial wave passes of wg_gemv_n, the two-rows-ahead prefetch of wg_gemv_n_then_t and its use of the
    whole LDS area at cols = 512, the clamped loads of wg_symv_lower, short last blocks of wg_chol_solve;
  * outputs, scratch and `raw` start as NaN (unless beta != 0), and everything an operation must not write -- the padding
    between slices, skipped problems, the strict upper triangle -- is compared bit for bit with what it held before;
  * the bitwise claims the source makes are asserted as such: u of wg_gemv_n_then_t is wg_gemv_n's, the multiply-on-load
    instantiations give the plain instantiation's bytes on fl(ms * M), a masked factorisation gives the
    unmasked one's bytes on the problems it works on;
  * the block solve and the factorisation are held to MARGIN x what a float64 numpy restatement of the same algorithm
    achieves, computed at run time (tests/batched_ops.py; DESIGN 4.5 has the measured ratios).
Every case runs with 256 and with 512 threads per problem, and where the multiply-on-load exists plain and shared.

Preconditions the tests state rather than probe: list entries lie in [0, B); winv is zero before the first factorisation
(potf2_inv_body writes the lower parts only, and the panel solve reads whole 16 x 16 diagonal tiles of the forward image)."""
import numpy as np
import pytest
import scipy.linalg as sla

import batched_ops as O
from batched_ops import FORMS, MS, NB, U, WBLK, same_bits

pytestmark = pytest.mark.gpu

AB = [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)]


def ms_of(shared):
    return MS if shared else 1.0


def eff(M, shared):
    """the matrix the kernel is specified to use: fl(ms * M), formed in float64"""
    return (MS * M) if shared else M


# ---------------------------------------------------------------------------------------------- wg_gemv_n
GEMV_N = [(1, 1), (3, 63), (4, 64), (5, 65), (16, 255), (17, 256), (31, 257), (33, 300), (5, 512), (17, 576), (1, 576),
          (33, 1), (4, 300), (16, 64)]


@pytest.mark.parametrize("k", range(len(GEMV_N)), ids=["%dx%d" % c for c in GEMV_N])
def test_gemv_n(hip, k):
    """4 rows per wave pass, 256 columns per lane pass: rows around the pass and the wave count, columns around the chunk of
    64 and the pass of 256.  beta = 0 with y = NaN must give finite results (y is not read)."""
    rows, cols = GEMV_N[k]
    M, x = O.matrix_operands(1000 + k, 3, rows, cols, cols)
    y0 = np.random.default_rng(k).standard_normal((3, rows))
    for f, (tpb, shared) in enumerate(FORMS):
        alpha, beta = AB[(k + f) % 3]
        label = f"gemv_n {rows}x{cols} tpb {tpb} shared {shared} alpha {alpha} beta {beta}"
        y = O.run_gemv_n(hip, tpb, shared, M, x, alpha, beta, y0, label)
        for b in range(3):
            O.check_product(y[b], M[b], x[b], alpha, beta, y0[b], f"{label} problem {b}")


# ---------------------------------------------------------------------------------------------- wg_gemv_n_then_t<8>
NT_COLS = [1, 63, 64, 65, 300, 511, 512, 512, 65]


def nt_rows(tpb):
    nw = tpb // 64
    return [1, nw - 1, nw, nw + 1, 2 * nw, 2 * nw + 1, 3 * nw + 1, 256, 256]


def nt_check(hip, tpb, shared, rows, cols, seed):
    M, x = O.matrix_operands(seed, 2, rows, cols, cols)
    rng = np.random.default_rng(seed + 1)
    theta, t = rng.standard_normal((2, rows)), rng.standard_normal((2, rows))
    label = f"gemv_n_then_t {rows}x{cols} tpb {tpb} shared {shared}"
    u, at = O.run_gemv_n_then_t(hip, tpb, shared, M, x, theta, t, label)
    un = O.run_gemv_n(hip, tpb, shared, M, x, 1.0, 0.0, None, label + " (gemv_n)")
    assert same_bits(u, un), f"{label}: u is not bitwise wg_gemv_n's ({int((O.bits(u) != O.bits(un)).sum())} entries differ)"
    for b in range(2):
        O.check_product(u[b], M[b], x[b], 1.0, 0.0, None, f"{label} u problem {b}")
        dy = theta[b] * (u[b] - t[b])  # fl(theta * fl(u_dev - t)): the device's own operand
        O.check_product(at[b], M[b].T.copy(), dy, 1.0, 0.0, None, f"{label} at problem {b}")
    return u, at


@pytest.mark.parametrize("tpb,shared", FORMS)
def test_gemv_n_then_t(hip, tpb, shared):
    """A row per wave and step, two rows ahead: rows around NW, 2 NW, 3 NW (the prefetch runs dry at different steps) and one
    long case; columns around the chunk of 64 up to the 8 chunks a lane holds."""
    for k, (rows, cols) in enumerate(zip(nt_rows(tpb), NT_COLS)):
        nt_check(hip, tpb, shared, rows, cols, 2000 + 10 * k)


def test_gemv_n_then_t_owns_the_whole_lds_area(hip):
    """cols = 512 at 256 threads: `tot` is exactly the LDS_DOUBLES = 512 doubles of the program.  Two runs in one process with
    another operation between them (which leaves its own data in LDS) must give the same bytes."""
    u1, at1 = nt_check(hip, 256, 0, 37, 512, 2500)
    M, x = O.matrix_operands(77, 2, 9, 64, 9)
    O.run_gemv_t(hip, 256, 0, M, x, 1.0, 0.0, None, 1.0, "between")  # (row-split form: partial sums in LDS)
    L, Ws, b = O.made_factor(78, 200)
    O.run_chol_solve(hip, 256, 0, O.colmajor(L, 256, 256, np.nan)[None], 256, O.images_of(Ws), 200, b[None], "between")
    u2, at2 = nt_check(hip, 256, 0, 37, 512, 2500)
    assert same_bits(u1, u2) and same_bits(at1, at2)


# ---------------------------------------------------------------------------------------------- wg_gemv_t
GEMV_T_COLS = [1, 63, 64, 65, 128, 129, 192, 200, 256, 257, 300, 512, 576]


def gemv_t_rows(tpb, cols):
    cpad = (cols + 63) // 64 * 64
    G = tpb // cpad if cpad < tpb else 1
    return G, ([0, 1, 7, 8, 15, 16, 17, 24, 25, 33] if G == 1 else [0, 1, G, 4 * G - 1, 4 * G, 4 * G + 1])


@pytest.mark.parametrize("cols", GEMV_T_COLS)
def test_gemv_t(hip, cols):
    """A thread per column (16 / 8 / 1 rows per step: rows around those) or, when the workgroup is wider than the matrix, G
    groups that split the rows four at a time (rows around G and 4 G).  rows = 0 is wg_kkt_mul at m = 0: out = beta out, or 0
    for beta = 0 with NaN in out.  out is bitwise fl(alpha raw + beta out0): raw is the unscaled sum itself."""
    k = 0
    for tpb, shared in FORMS:
        G, rows_list = gemv_t_rows(tpb, cols)
        for rows in rows_list:
            k += 1
            alpha, beta = AB[k % 3]
            M, v = O.matrix_operands(3000 + 7 * cols + rows, 2, rows, cols, max(rows, 1))
            y0 = np.random.default_rng(cols + rows).standard_normal((2, cols))
            label = f"gemv_t {rows}x{cols} tpb {tpb} shared {shared} G {G} alpha {alpha} beta {beta}"
            out, raw = O.run_gemv_t(hip, tpb, shared, M, v, alpha, beta, y0, ms_of(shared), label)
            for b in range(2):
                Mt = eff(M[b], shared).T.copy()
                O.check_product(raw[b], Mt, v[b, :rows], 1.0, 0.0, None, f"{label} raw problem {b}")
                O.check_product(out[b], Mt, v[b, :rows], alpha, beta, y0[b], f"{label} problem {b}")
                want = alpha * raw[b] if beta == 0.0 else alpha * raw[b] + beta * y0[b]
                assert same_bits(out[b], want), f"{label}: out is not fl(alpha raw + beta out0)"
                if rows == 0:
                    assert same_bits(out[b], np.zeros(cols) if beta == 0.0 else 0.0 * alpha + beta * y0[b]), label
            if rows == rows_list[-1]:  # raw is optional
                out2, _ = O.run_gemv_t(hip, tpb, shared, M, v, alpha, beta, y0, ms_of(shared), label, raw=False)
                assert same_bits(out, out2), f"{label}: the result depends on whether raw is kept"


# ---------------------------------------------------------------------------------------------- wg_symv_lower
SYMV_N = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300, 448, 449, 511, 512]


def sym_operands(seed, nprob, n):
    rng = np.random.default_rng(seed)
    low = np.tril(rng.standard_normal((nprob, n, n)))
    full = low + np.transpose(np.tril(low, -1), (0, 2, 1))
    poisoned = low.copy()
    poisoned[:, np.triu(np.ones((n, n), dtype=bool), 1)] = np.nan
    return poisoned, full, rng.standard_normal((nprob, n))


@pytest.mark.parametrize("n", SYMV_N)
def test_symv_lower(hip, n):
    """The strict upper triangle holds NaN: a finite result within the bound against the symmetric completion proves that the
    triangle alone is read (rows and columns are clamped into it, never branched around).  n around the group of 4 rows, the
    chunk of 64 columns, the wave count and SYM_MAX = 512."""
    Hp, Hf, x = sym_operands(4000 + n, 2, n)
    y0 = np.random.default_rng(n).standard_normal((2, n))
    for f, (tpb, shared) in enumerate(FORMS):
        alpha, beta = AB[(n + f) % 3]
        label = f"symv_lower n {n} tpb {tpb} shared {shared} alpha {alpha} beta {beta}"
        y, raw, _ = O.run_symv(hip, tpb, shared, Hp, x, alpha, beta, y0, ms_of(shared), label)
        for b in range(2):
            He = eff(Hf[b], shared)
            O.check_product(raw[b], He, x[b], 1.0, 0.0, None, f"{label} raw problem {b}")
            O.check_product(y[b], He, x[b], alpha, beta, y0[b], f"{label} problem {b}")
            want = alpha * raw[b] if beta == 0.0 else alpha * raw[b] + beta * y0[b]
            assert same_bits(y[b], want), f"{label}: y is not fl(alpha raw + beta y0)"
        y2, _, _ = O.run_symv(hip, tpb, shared, Hp, x, alpha, beta, y0, ms_of(shared), label, raw=False)
        assert same_bits(y, y2), f"{label}: the result depends on whether raw is kept"


# ---------------------------------------------------------------------------------------------- MS: bitwise the plain form
@pytest.mark.parametrize("tpb", [256, 512])
def test_multiply_on_load_is_bitwise_the_plain_program_on_the_scaled_matrix(hip, tpb):
    """the shared instantiation on (M, ms) reads fl(ms * M[i][j]) wherever the plain one reads M[i][j] and does
    nothing else differently -- the same bytes, for both H products."""
    for n in (5, 65, 300, 512):
        Hp, _, x = sym_operands(5000 + n, 2, n)
        a = O.run_symv(hip, tpb, 1, Hp, x, 0.5, 0.0, None, MS, f"ms symv {n} shared")
        b = O.run_symv(hip, tpb, 0, MS * Hp, x, 0.5, 0.0, None, 1.0, f"ms symv {n} plain")
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), f"wg_symv_lower n {n} tpb {tpb}"
    for rows, cols in ((33, 300), (17, 576), (9, 64), (33, 129), (25, 512)):
        M, v = O.matrix_operands(5100 + rows + cols, 2, rows, cols, rows)
        a = O.run_gemv_t(hip, tpb, 1, M, v, -1.0, 0.0, None, MS, f"ms gemv_t {rows}x{cols} shared")
        b = O.run_gemv_t(hip, tpb, 0, MS * M, v, -1.0, 0.0, None, 1.0, f"ms gemv_t {rows}x{cols} plain")
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), f"wg_gemv_t {rows}x{cols} tpb {tpb}"


# ---------------------------------------------------------------------------------------------- bq_prewrite_h_kernel
@pytest.mark.parametrize("nx", [1, 15, 16, 17, 255, 256, 257, 300])
def test_prewrite_h(hip, nx):
    """K_b's lower triangle <- fl(h_scale[b] * H), launched as the assembly launches it: blocks of 16 columns, 256 rows per
    pass.  Strict upper triangle, padding and the problems a mask leaves out keep their bytes."""
    B, ldk = 5, (nx + 127) // 128 * 128
    rng = np.random.default_rng(6000 + nx)
    H = rng.standard_normal((nx, nx))  # flat index i + j * nx, i >= j, is what the kernel reads
    hs = rng.uniform(0.05, 1.0, B)
    low = np.tril(np.ones((nx, nx), dtype=bool)).T  # [j][i]: i >= j
    variants = [("all", None, None, 0, range(B)), ("skip", [0, 1, 0, 7, 0], None, 0, [0, 2, 4]),
                ("list5", None, [4, 1, 3, 0, 2], 2, range(B)), ("list2", None, [3, 1], 2, [1, 3]), ("list0", None, [], 2, [])]
    for scaled in (False, True):
        for name, skip, lst, slots, touched in variants:
            K0 = rng.standard_normal((B, ldk, ldk))
            Kd = O.dev(K0, hip)
            f = {}
            if scaled:
                f["h_scale"] = O.dev(hs, hip)
            if skip is not None:
                f["skip"] = O.i32dev(skip, hip)
            if lst is not None:
                f.update(list=O.i32dev(lst if lst else [0], hip), count=O.i32dev([len(lst)], hip), slots=slots)
            rc = O.seam(hip, "prewrite_h", 256, 0, B, rows=nx, ld=ldk, M=O.dev(H, hip), y=Kd, **f)
            assert rc == 0, (name, rc, hip.lib.madqp_last_error(hip.ctx))
            K1 = O.host(Kd).reshape(K0.shape)
            for b in range(B):
                want = K0[b].copy()
                if b in touched:
                    want[:nx, :nx][low] = ((hs[b] * H) if scaled else H)[low]
                assert same_bits(K1[b], want), f"prewrite_h nx {nx} {name} h_scale {scaled}: problem {b} " \
                                               f"({int((O.bits(K1[b]) != O.bits(want)).sum())} doubles differ)"


# ---------------------------------------------------------------------------------------------- the seam refuses
def test_the_seam_refuses_what_could_read_out_of_bounds(hip):
    d = O.dev(np.zeros(600 * 600), hip)
    ok = dict(rows=4, cols=4, ld=4, M=d, x=d, y=d, theta=d, t=d, at=d, winv=d, sym=d)

    def rc(op, tpb=256, **f):
        return O.seam(hip, op, tpb, 0, 1, **{**ok, **f})

    assert rc("gemv_n", tpb=128) == O.ERR_ARG and rc("gemv_n", tpb=1024) == O.ERR_ARG
    assert rc("gemv_n_then_t", cols=513) == O.ERR_ARG
    for op in ("gemv_n", "gemv_n_then_t", "gemv_t"):  # (an empty matrix is rows == 0 only; the other helpers take no cols)
        assert rc(op, cols=0) == O.ERR_ARG, op
    assert rc("symv_lower", rows=513) == O.ERR_ARG and rc("symv_lower", rows=0) == O.ERR_ARG
    assert rc("chol_solve", rows=8, ld=7) == O.ERR_ARG and rc("prewrite_h", rows=8, ld=7) == O.ERR_ARG
    assert rc(6) == O.ERR_ARG and rc(-1) == O.ERR_ARG
    assert O.seam(hip, "gemv_n", 256, 0, 0, **ok) == O.ERR_ARG
    for op, field in (("gemv_n", "M"), ("gemv_n", "x"), ("gemv_n", "y"), ("gemv_n_then_t", "theta"), ("gemv_n_then_t", "t"),
                      ("gemv_n_then_t", "at"), ("symv_lower", "sym"), ("chol_solve", "winv"), ("prewrite_h", "y")):
        assert rc(op, **{field: None}) == O.ERR_ARG, (op, field)
    assert O.seam(hip, "prewrite_h", 256, 0, 2, rows=4, ld=4, M=d, y=d, list=O.i32dev([0], hip), slots=2) == O.ERR_ARG  # no count
    assert hip.lib.madqp_debug_chol_factor_batched(hip.ctx, d.data_ptr(), 7, 8, 64, d.data_ptr(), WBLK, d.data_ptr(), 1, None,
                                                   0, None, None) == O.ERR_ARG  # lda < n
    assert rc("gemv_n") == 0


# ---------------------------------------------------------------------------------------------- wg_chol_solve, made factors
SOLVE_N = [(1, 0), (2, 0), (64, 0), (65, 0), (127, 0), (128, 0), (129, 0), (200, 0), (200, 2), (256, 0), (257, 0), (384, 0),
           (400, 0), (512, 0), (513, 0), (640, 0)]


@pytest.mark.parametrize("n,extra", SOLVE_N, ids=["n%d%s" % (n, "_lda+2" if e else "") for n, e in SOLVE_N])
def test_chol_solve_on_made_factors(hip, n, extra):
    """The indexing of the two sweeps, not the inverse's conditioning: L well conditioned, the images of its diagonal blocks'
    inverses made in longdouble.  NaN in the halves of the images that are never fetched, in the strict upper triangle and in
    rows n .. of L; identity padding in a short block.  Device and float64 restatement against the same formula in
    longdouble, in units of u x its running magnitude."""
    B = 3
    npad, lda = O.npad_of(n), O.npad_of(n) + extra
    made = [O.made_factor(7000 + 10 * n + b, n) for b in range(B)]
    Lcm = np.stack([O.colmajor(np.where(np.tril(np.ones((n, n), dtype=bool)), L, np.nan), lda, npad, np.nan) for L, _, _ in made])
    winv = np.concatenate([O.images_of(Ws) for _, Ws, _ in made])
    rhs = np.stack([b for _, _, b in made])
    restated = [O.solve_ratio(O.sweep_formula(L, Ws, b, np.float64), L, Ws, b) for L, Ws, b in made]
    for tpb, shared in FORMS:
        x = O.run_chol_solve(hip, tpb, shared, Lcm, lda, winv, n, rhs, f"chol_solve n {n} tpb {tpb}")
        assert np.all(np.isfinite(x)), f"chol_solve n {n} tpb {tpb}: non-finite entries (a poisoned entry was read)"
        device = [O.solve_ratio(x[b], *made[b]) for b in range(B)]
        print(f"[batched-ops] chol_solve made n {n} lda {lda} tpb {tpb} shared {shared}: device / restated per problem " +
              ", ".join(f"{d:.3f} / {r:.3f}" for d, r in zip(device, restated)))
        for b in range(B):
            assert device[b] <= O.MARGIN * restated[b], (n, tpb, b, device[b], restated[b])


# ---------------------------------------------------------------------------------------------- batched factorisation
FACTOR_N = [1, 17, 127, 128, 129, 255, 256, 300, 384, 512, 640]


@pytest.fixture(scope="module")
def factor_case(hip):
    """factor_case(n): the batch of order n factored once without masks (zero padding, NaN in the strict upper triangle), with
    the restated and LAPACK figures of the same matrices -- made on first use, shared by the tests of this module."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = make_factor_case(hip, n)
        return made[n]

    return get


def make_factor_case(hip, n):
    As, rhs = O.spd_batch(8000 + n, n)
    lda = O.npad_of(n)
    K0 = O.k_storage(As, lda)
    rc, K1, W1, info, _ = O.factor_batched(hip, K0, lda, n)
    assert rc == 0, hip.lib.madqp_last_error(hip.ctx)
    cpu = []
    for A, b in zip(As, rhs):
        r = O.BlockCholRestated(A)
        Ll = np.linalg.cholesky(A)
        xl = sla.cho_solve((Ll, True), b)
        cpu.append(dict(res_restated=O.factor_residual(A, r.L), res_lapack=O.factor_residual(A, Ll),
                        res64_restated=O.factor_residual_f64(A, r.L),
                        bwd_restated=O.backward_error(A, r.solve(b), b), bwd_lapack=O.backward_error(A, xl, b)))
    return As, rhs, K0, K1, W1, info, cpu


@pytest.mark.parametrize("n", FACTOR_N)
def test_factor_batched_then_solve(hip, factor_case, n):
    """Residual of the factor and backward error of wg_chol_solve on it, device beside restatement beside LAPACK; the strict
    upper triangle (NaN) and the padding are never written; info = 0."""
    As, rhs, K0, K1, W1, info, cpu = factor_case(n)
    B, lda = len(As), O.npad_of(n)
    assert list(info) == [0] * B
    low = np.zeros(K0.shape[1:], dtype=bool)
    low[:n, :n] = np.tril(np.ones((n, n), dtype=bool)).T
    for b in range(B):
        assert np.array_equal(O.bits(K1[b])[~low], O.bits(K0[b])[~low]), f"n {n} problem {b}: written outside the lower triangle"
        assert np.all(np.isfinite(K1[b][low])), f"n {n} problem {b}: non-finite factor"
    res = [O.factor_residual(As[b], O.lower_of(K1[b], n)) for b in range(B)]
    res64 = [O.factor_residual_f64(As[b], O.lower_of(K1[b], n)) for b in range(B)]
    for b in range(B):  # every problem against the restatement of the SAME problem (the batch has mixed conditioning on purpose)
        c = cpu[b]
        print(f"[batched-ops] factor n {n} problem {b}: residual device {res[b]:.3f} restated {c['res_restated']:.3f} lapack "
              f"{c['res_lapack']:.3f} | every entry, float64 product: device {res64[b]:.3f} restated {c['res64_restated']:.3f}")
        assert res[b] <= O.MARGIN * c["res_restated"], (n, b, res[b], c["res_restated"])
        assert res64[b] <= O.MARGIN * c["res64_restated"], (n, b, res64[b], c["res64_restated"])
    for tpb in (256, 512):
        x = O.run_chol_solve(hip, tpb, 0, K1, lda, W1, n, rhs, f"factor+solve n {n} tpb {tpb}")
        for b in range(B):
            c, bwd = cpu[b], O.backward_error(As[b], x[b], rhs[b])
            print(f"[batched-ops] solve n {n} problem {b} tpb {tpb}: backward error device {bwd:.3f} restated {c['bwd_restated']:.3f} "
                  f"lapack {c['bwd_lapack']:.3f}")
            assert bwd <= O.MARGIN * c["bwd_restated"], (n, tpb, b, bwd, c["bwd_restated"])


@pytest.mark.parametrize("n", [129, 300, 640])
def test_factor_batched_ignores_what_the_padding_rows_hold(hip, factor_case, n):
    """lda = npad: the panel solve and the updates may READ rows n .. npad (whole tiles), but what they compute from them is
    never stored -- finite garbage there gives the bytes of the zero-padded run, and stays as it was."""
    As, rhs, K0, K1, W1, info, _ = factor_case(n)
    lda = O.npad_of(n)
    rng = np.random.default_rng(n)
    Kg = O.k_storage(As, lda, pad_rows=lambda shape: 1e3 * rng.standard_normal(shape))
    rc, K2, W2, info2, _ = O.factor_batched(hip, Kg, lda, n)
    assert rc == 0 and list(info2) == [0] * len(As)
    assert same_bits(K2[:, :, :n], K1[:, :, :n]) and same_bits(W2, W1)
    assert same_bits(K2[:, :, n:], Kg[:, :, n:])


@pytest.mark.parametrize("n", [17, 129, 384, 640])
def test_factor_batched_masks(hip, factor_case, n):
    """skip leaves a problem's K and winv alone and the others as they are without it; the compacted list with 2 slots for 3
    problems gives the unmasked bytes on the listed problems and leaves the fourth alone."""
    As, rhs, K0, K1, W1, info, _ = factor_case(n)
    lda, B = O.npad_of(n), len(As)
    W0 = np.random.default_rng(n).standard_normal(W1.shape)  # (a skipped problem's images: any bytes)
    for name, kw, on in (("skip", dict(skip=[0, 5, 0, 0]), [0, 2, 3]), ("list", dict(lst=[3, 0, 2], slots=2), [0, 2, 3])):
        Win = W0.copy()
        Win[on] = 0.0
        rc, K2, W2, info2, _ = O.factor_batched(hip, K0, lda, n, winv=Win, **kw)
        assert rc == 0, (name, hip.lib.madqp_last_error(hip.ctx))
        for b in range(B):
            if b in on:
                assert same_bits(K2[b], K1[b]) and same_bits(W2[b], W1[b]) and info2[b] == 0, (name, n, b)
            else:
                assert same_bits(K2[b], K0[b]) and same_bits(W2[b], W0[b]), (name, n, b)
    rc, K2, W2, info2, _ = O.factor_batched(hip, K0, lda, n, winv=W0, lst=[], slots=2)  # count = 0: nothing happens
    assert rc == 0 and same_bits(K2, K0) and same_bits(W2, W0)


@pytest.mark.parametrize("n,col", [(17, 5), (300, 1), (300, 128), (300, 200), (640, 400)])
def test_factor_batched_info(hip, factor_case, n, col):
    """One indefinite problem: info = the 1-based first failing column, its neighbours bitwise what they are without it; a
    second call on good matrices clears the stale word."""
    As, rhs, K0, K1, W1, info, _ = factor_case(n)
    lda = O.npad_of(n)
    bad = As.copy()
    bad[1, col - 1, col - 1] = -1.0  # the leading minor of order col is the first that is not positive definite
    rc, K2, W2, info2, (Kd, Wd) = O.factor_batched(hip, O.k_storage(bad, lda), lda, n)
    assert rc == 0
    assert list(info2) == [0, col, 0, 0], (n, col, list(info2))
    for b in (0, 2, 3):
        assert same_bits(K2[b], K1[b]) and same_bits(W2[b], W1[b]), (n, col, b)
    rc, K3, W3, info3, _ = O.factor_batched(hip, K0, lda, n, info0=info2)
    assert rc == 0 and list(info3) == [0, 0, 0, 0] and same_bits(K3, K1)
