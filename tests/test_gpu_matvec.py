"""GPU: every launch form of the dense mat-vec kernels (csrc/gemv.hip) against a plain extended-precision reference of the
same product, at the smallest shapes at which each form or edge exists.

The dispatcher picks among ten launch forms by shape, pointer alignment and parity of the leading dimension; two further
products read one side of a symmetric matrix.  Each case here
  * asserts from the dispatcher's own report (madqp_debug_gemv_form, for the very pointers passed) that the form under
    test runs -- a moved threshold fails the case by name instead of silently ending its coverage,
  * holds every entry to the bound DERIVED in tests/matvec.py ((len + 4) u S against the extended-precision reference,
    2 (len + 4) u S against float64 numpy; nothing is tuned from what a kernel gives),
  * keeps y in a NaN buffer with guards on both sides (bits compared) and NaN in every double of the operand that must
    not be read: the padding of the rows, the side of a symmetric matrix that is not held,
  * runs alpha / beta = (1, 0) over a NaN y, (-1, 1) and (0.5, -2).
The symmetric products go through madqp_debug_symv at orders 1 .. 1537 (the solver reaches those kernels from 2048 and
12288 only), each twice over a workspace freshly filled with NaN: the file claims a fixed summation order."""
import numpy as np
import pytest
import torch

import matvec as V
from matvec import ERR_ARG, Guarded, form, run_gemv, run_symv

pytestmark = pytest.mark.gpu


def even(n):
    return n + (n & 1)


W = lambda vec, wg: dict(form="n_wave", vec=vec, workgroups=wg, chunks=0)
B = lambda vec, wg: dict(form="n_block", vec=vec, workgroups=wg, chunks=0)
T1 = lambda vec, wg: dict(form="t_single", vec=vec, workgroups=wg, chunks=1)
TC = lambda vec, chunks, rpc, wg: dict(form="t_chunked", vec=vec, chunks=chunks, rows_per_chunk=rpc, workgroups=wg)
TS = lambda wg: dict(form="t_strip", vec=1, workgroups=wg, chunks=1)

# (label, rows, cols, lda, expected report, operands 8 bytes off)
N_CASES = [
    # one wave per row, 16-byte loads
    ("wave_1x1", 1, 1, 2, W(1, 1), {}),
    ("wave_rows_not_x4", 5, 3, 4, W(1, 2), {}),
    ("wave_odd_tail", 9, 65, 66, W(1, 3), {}),                 # 32 pairs + the lone last column (row_dot)
    ("wave_second_pair_trip", 9, 130, 130, W(1, 3), {}),       # 65 pairs: lane 0 takes a second one
    ("wave_y_off8", 7, 65, 66, W(1, 2), dict(y_off=1)),        # y is stored double by double: its address is no rule
    # one wave per row, scalar loads
    ("wave_scalar_odd_lda", 7, 65, 65, W(0, 2), {}),
    ("wave_scalar_A_off8", 7, 65, 66, W(0, 2), dict(a_off=1)),
    ("wave_scalar_x_off8", 7, 65, 66, W(0, 2), dict(x_off=1)),  # x alone drops the product to the scalar form
    ("wave_scalar_all_off8", 7, 65, 65, W(0, 2), dict(a_off=1, x_off=1, y_off=1)),
    # 8192 workgroups x 4 waves: rows 32768 .. 32772 are the second trip of the row loop
    ("wave_grid_stride", 32773, 3, 4, W(1, 8192), {}),
    ("wave_grid_stride_scalar", 32773, 3, 3, W(0, 8192), {}),
    # one workgroup per row: fewer than 2048 rows of more than 1024 columns
    ("block_vec", 3, 1026, 1026, B(1, 3), {}),
    ("block_vec_odd_cols", 3, 1027, 1028, B(1, 3), {}),
    ("block_scalar_odd_lda", 3, 1027, 1027, B(0, 3), {}),
    ("block_scalar_x_off8", 3, 1026, 1026, B(0, 3), dict(x_off=1)),
    ("block_scalar_A_off8", 3, 1026, 1026, B(0, 3), dict(a_off=1)),
    # the rule rows >= 2048 || cols <= 1024 from both sides
    ("rule_cols_1024_wave", 3, 1024, 1024, W(1, 1), {}),
    ("rule_cols_1025_block", 3, 1025, 1026, B(1, 3), {}),
    ("rule_rows_2047_block", 2047, 1025, 1026, B(1, 2047), {}),
    ("rule_rows_2048_wave", 2048, 1025, 1026, W(1, 512), {}),
]


@pytest.mark.parametrize("label,rows,cols,lda,want,off", N_CASES, ids=[c[0] for c in N_CASES])
def test_gemv_n_form(hip, label, rows, cols, lda, want, off):
    run_gemv(hip, 0, rows, cols, lda, want, label, **off)


T_CASES = [
    # one chunk of rows (fewer than 128): the product kernel writes y
    ("single_1x1", 1, 1, 2, T1(1, 1), {}),
    ("single_two_tiles", 127, 130, 130, T1(1, 2), {}),
    ("single_lone_last_column", 5, 129, 130, T1(1, 2), {}),    # column 128: the scalar branch of the vectorised form
    ("single_scalar", 5, 129, 129, T1(0, 2), {}),
    ("single_scalar_A_off8", 127, 130, 130, T1(0, 2), dict(a_off=1)),
    ("single_x_off8_stays_vec", 127, 130, 130, T1(1, 2), dict(x_off=1, y_off=1)),  # x is read double by double
    # chunks of rows, partials, reduce
    ("chunked_2x64", 128, 3, 4, TC(1, 2, 64, 2), {}),
    ("chunked_short_last_chunk", 131, 257, 258, TC(1, 2, 68, 6), {}),  # 68 + 63 rows, 3 tiles, odd cols, 2 reduce blocks
    ("chunked_scalar", 131, 257, 257, TC(0, 2, 68, 6), {}),
    ("chunked_4100", 4100, 5, 6, TC(1, 61, 68, 61), {}),       # 64 chunks of 65 rows, rounded to 68: 61 chunks
    ("chunked_cap_64", 4352, 5, 6, TC(1, 64, 68, 64), {}),     # rows / 64 = 68 chunks capped to 64, of 68 rows each
    # 16-column strips over all rows
    ("strip_smallest", 64, 2048, 2048, TS(128), {}),
    ("strip_lone_last_column", 65, 2049, 2050, TS(129), {}),
    ("strip_unrolled_plus_rest", 300, 2050, 2050, TS(129), {}),  # 9 or 10 rows per lane: one unrolled trip of 8 + a rest
    # just outside the strip window
    ("no_strip_63_rows", 63, 2048, 2048, T1(1, 16), {}),
    ("no_strip_2047_cols", 64, 2047, 2048, T1(1, 16), {}),
    ("no_strip_odd_lda", 64, 2049, 2049, T1(0, 17), {}),
]


@pytest.mark.parametrize("label,rows,cols,lda,want,off", T_CASES, ids=[c[0] for c in T_CASES])
def test_gemv_t_form(hip, label, rows, cols, lda, want, off):
    run_gemv(hip, 1, rows, cols, lda, want, label, **off)


def test_strip_window_far_edges_by_the_form_query(hip):
    """rows = 16384 / 16385 and rows * cols = 2^27 / beyond: asserted through the dispatcher's report alone (nothing of
    that size is allocated; the addresses are made up and never dereferenced)."""
    q = lambda rows, cols, lda: form(hip.lib, 1, rows, cols, V.ALIGNED, lda, V.ALIGNED)[1]
    assert q(16384, 2048, 2048)["form"] == "t_strip"
    assert q(16385, 2048, 2048)["form"] == "t_chunked"
    assert q(16384, 8192, 8192)["form"] == "t_strip"       # rows * cols = 2^27
    assert q(16384, 8193, 8194)["form"] == "t_chunked"
    assert q(8192, 16384, 16384)["form"] == "t_strip"
    assert q(8193, 16384, 16384)["form"] == "t_chunked"


@pytest.mark.parametrize("trans,rows,cols", [(0, 5, 0), (1, 0, 5), (0, 300, 0)])
def test_inner_length_zero_scales_y(hip, trans, rows, cols):
    """klen == 0: y = beta y by scale_kernel (300: two workgroups, the second ragged); beta = 0 clears NaN.  A and x are
    never read: null pointers are accepted."""
    n = rows + cols
    want = dict(form="scale", vec=0, chunks=0, workgroups=(n + 255) // 256)
    run_gemv(hip, trans, rows, cols, 2, want, f"scale_{trans}_{n}")
    rc, got = form(hip.lib, trans, rows, cols, None, 0, None)
    assert rc == 0 and got["form"] == "scale", (rc, got)
    y0 = V.operands(rows, cols)[3 + trans]
    for beta in (0.0, -2.0):
        y = Guarded(hip, n, values=None if beta == 0.0 else y0)
        assert hip.lib.madqp_gemv(hip.ctx, trans, rows, cols, 1.0, None, 0, None, beta, y.ptr()) == 0
        out = y.read(f"scale null operands beta {beta}")
        assert V.same_bits(out, np.zeros(n) if beta == 0.0 else beta * y0)


@pytest.mark.parametrize("trans,rows,cols", [(0, 0, 5), (1, 5, 0), (0, 0, 0)])
def test_output_length_zero_is_a_no_op(hip, trans, rows, cols):
    """ylen == 0: OK with every pointer null, nothing launched, nothing written (a y that is given stays as it was)."""
    rc, got = form(hip.lib, trans, rows, cols, None, 0, None)
    assert rc == 0 and got == dict(form="none", vec=0, chunks=0, rows_per_chunk=0, workgroups=0), (rc, got)
    assert hip.lib.madqp_gemv(hip.ctx, trans, rows, cols, 1.0, None, 0, None, 0.0, None) == 0
    y = Guarded(hip, 4, values=np.arange(4.0))
    A = V.dev(np.ones(16), hip)
    assert hip.lib.madqp_gemv(hip.ctx, trans, rows, cols, 1.0, A.data_ptr(), 8, A.data_ptr(), 0.0, y.ptr()) == 0
    assert V.same_bits(y.read("ylen 0"), np.arange(4.0))


def test_gemv_refusals_leave_y_untouched(hip):
    """What the dispatcher refuses, the form query refuses too -- and nothing is launched."""
    A = V.dev(np.ones(64), hip)
    for label, trans, rows, cols, a, lda, x in [("null A", 0, 4, 4, None, 4, A), ("null x", 1, 4, 4, A, 4, None),
                                                ("lda < cols", 0, 4, 4, A, 3, A), ("trans 2", 2, 4, 4, A, 4, A),
                                                ("rows < 0", 0, -1, 4, A, 4, A), ("cols < 0", 1, 4, -1, A, 4, A)]:
        y = Guarded(hip, 4, values=np.arange(4.0))
        ptr = lambda t: None if t is None else t.data_ptr()
        assert hip.lib.madqp_gemv(hip.ctx, trans, rows, cols, 1.0, ptr(a), lda, ptr(x), 0.0, y.ptr()) == ERR_ARG, label
        assert form(hip.lib, trans, rows, cols, ptr(a), lda, ptr(x))[0] == ERR_ARG, label
        assert V.same_bits(y.read(label), np.arange(4.0)), label
    assert hip.lib.madqp_gemv(hip.ctx, 0, 4, 4, 1.0, A.data_ptr(), 4, A.data_ptr(), 0.0, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- symmetric products
# 256-row x 512-column tiles: one row tile (<= 256), two row tiles of one column tile (257 .. 512), the second column tile
# with one ragged row tile (513 .. 768; 768: the first interior, unmasked tile (column tile 0, row tile 2)) or two
# (769 .. 1024: n % 512 > 256), and 1537 = 3 x 512 + 1
SYMV_ORDERS = [1, 2, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1537]


@pytest.fixture(scope="module")
def poison(hip):
    return V.WorkspacePoison(hip)


@pytest.mark.parametrize("n", SYMV_ORDERS)
@pytest.mark.parametrize("upper", [0, 1])
def test_symv_one_side(hip, poison, upper, n):
    for ldh in (even(n), even(n) + 6):
        run_symv(hip, poison, upper, n, ldh, f"symv_{'upper' if upper else 'lower'}_{n}_ld{ldh}")


def test_symv_refusals_leave_y_untouched(hip, poison):
    n = 8
    H, x = V.dev(np.ones(2 * n * n), hip), V.dev(np.ones(n), hip)
    Hoff = V.dev(np.ones(n * n), hip, 1)
    p = lambda t: None if t is None else t.data_ptr()
    for label, upper, nn, h, ldh, xx, has_y in [("null H", 0, n, None, n, x, True), ("null x", 1, n, H, n, None, True),
                                                ("null y", 0, n, H, n, x, False), ("ldh < n", 1, n, H, n - 2, x, True),
                                                ("ldh odd", 0, n, H, n + 1, x, True), ("H 8 bytes off", 1, n, Hoff, n, x, True),
                                                ("upper 2", 2, n, H, n, x, True), ("upper -1", -1, n, H, n, x, True),
                                                ("n < 0", 0, -1, H, n, x, True)]:
        y = Guarded(hip, n, values=np.arange(float(n)))
        rc = hip.lib.madqp_debug_symv(hip.ctx, upper, nn, 1.0, p(h), ldh, p(xx), 0.0, y.ptr() if has_y else None)
        assert rc == ERR_ARG, (label, rc)
        assert V.same_bits(y.read(label), np.arange(float(n))), label
    assert hip.lib.madqp_debug_symv(None, 0, n, 1.0, p(H), n, p(x), 0.0, p(x)) == ERR_ARG
    assert hip.lib.madqp_debug_symv(hip.ctx, 0, 0, 1.0, None, 0, None, 0.0, None) == 0  # n == 0: an accepted no-op
    torch.cuda.synchronize()
