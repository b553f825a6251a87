"""The host-side rules of the KKT object (madqp_jl_amd/csrc/kkt_form.inc, compiled for the CPU by tests/csrc): the slot map
of the inequality rows that kkt.hip, batch.hip and dist.hip share, the two orders of the factorised matrix by explicit
figures, and the half-bandwidth of a pattern held to ``madqp_jl_amd.kkt.pattern_bandwidth``.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import madqp_jl_amd as M
from madqp_jl_amd.kkt import pattern_bandwidth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONDENSED, NORMAL, AUGMENTED = 0, 1, 2
P64 = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_kkt_form.so"))
    lib.kkt_slot_map_c.restype = C.c_int
    lib.kkt_slot_map_c.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.kkt_orders_c.restype = None
    lib.kkt_orders_c.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    for f in (lib.kkt_pattern_halfbandwidth_c, lib.kkt_csr_halfbandwidth_c):
        f.restype = C.c_int64
        f.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    return lib


def slot_map(lib, ind, m):
    ind = np.asarray(ind, dtype=np.int64)
    out = np.full(max(m, 1) + 1, 77, dtype=np.int64)  # one guard entry behind the m the function may write
    ok = lib.kkt_slot_map_c(ind.ctypes.data, len(ind), m, out.ctypes.data)
    assert out[max(m, 1)] == 77 and (m > 0 or out[0] == 77)
    return bool(ok), out[:m]


@pytest.mark.parametrize("ind, m", [([0, 2, 3, 7], 8), ([5], 6), (list(range(6)), 6), ([], 5), ([], 0)],
                         ids=["valid", "last_row", "every_row", "ns0", "m0"])
def test_slot_map_of_a_valid_list(lib, ind, m):
    ok, slot = slot_map(lib, ind, m)
    want = [-1] * m
    for k, r in enumerate(ind):
        want[r] = k
    assert ok and slot.tolist() == want


@pytest.mark.parametrize("ind, m", [([1, 4], 4), ([0], 0), ([-1, 2], 4), ([1, 1], 4), ([2, 1], 4), ([0, 3, 2], 4)],
                         ids=["row_eq_m", "row_with_m0", "negative", "repeated", "decreasing", "decreasing_late"])
def test_slot_map_refuses(lib, ind, m):
    ok, _ = slot_map(lib, ind, m)
    assert not ok


def orders(lib, mode, nx, m):
    out = np.zeros(5, dtype=np.int64)
    lib.kkt_orders_c(mode, nx, m, out.ctypes.data)
    return dict(zip(("rule_order", "np", "stored_order", "ldk", "k_doubles"), (int(v) for v in out)))


@pytest.mark.parametrize("mode, rule, stored, ldk", [(CONDENSED, 130, 130, 256), (NORMAL, 12, 12, 128),
                                                     (AUGMENTED, 142, 268, 384)], ids=["condensed", "normal", "augmented"])
def test_orders_at_130_by_12(lib, mode, rule, stored, ldk):
    assert orders(lib, mode, 130, 12) == dict(rule_order=rule, np=256, stored_order=stored, ldk=ldk,
                                              k_doubles=ldk * ldk + 128)


def test_orders_at_the_edges(lib):
    # nx a multiple of 128: no padding, the two orders of the augmented form agree
    assert orders(lib, AUGMENTED, 128, 12) == dict(rule_order=140, np=128, stored_order=140, ldk=256, k_doubles=256 * 256 + 128)
    assert orders(lib, CONDENSED, 128, 12) == dict(rule_order=128, np=128, stored_order=128, ldk=128, k_doubles=128 * 128 + 128)
    # nx = 0 and m = 0: storage never shrinks below one tile
    for mode, nx, m, rule in [(CONDENSED, 0, 5, 0), (NORMAL, 0, 5, 5), (AUGMENTED, 0, 5, 5), (CONDENSED, 7, 0, 7),
                              (NORMAL, 7, 0, 0), (CONDENSED, 0, 0, 0), (AUGMENTED, 0, 0, 0)]:
        o = orders(lib, mode, nx, m)
        assert o["rule_order"] == rule and o["np"] == (128 if nx else 0) and o["ldk"] == 128, (mode, nx, m, o)
        assert o["k_doubles"] == 128 * 128 + 128
    assert orders(lib, AUGMENTED, 7, 0) == dict(rule_order=7, np=128, stored_order=128, ldk=128, k_doubles=128 * 128 + 128)
    assert orders(lib, AUGMENTED, 7, 1)["ldk"] == 256  # np + m = 129
    # the AUTO refinement rule of the drivers means the same order (tests/test_host_logic.py holds options.py)
    assert orders(lib, AUGMENTED, 1000, 24)["rule_order"] == 1024 and orders(lib, AUGMENTED, 1000, 24)["stored_order"] == 1048


def arr(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.int64)


def gram_bw(lib, A, form):
    """What madqp_kkt_set_bandwidth scans for the Jacobian: the rows of V' -- the CSR of A in the condensed form (V = A'),
    the CSR of A' in the normal form (V = A)."""
    ptr, col = (arr(A.ptr), arr(A.col)) if form == "condensed" else (arr(A.t_ptr), arr(A.t_col))
    return lib.kkt_pattern_halfbandwidth_c(len(ptr) - 1, ptr.ctypes.data, col.ctypes.data)


def sym_bw(lib, H):
    ptr, col = arr(H.ptr), arr(H.col)
    return lib.kkt_csr_halfbandwidth_c(H.n, ptr.ctypes.data, col.ctypes.data)


def dense(rows, shape):
    A = np.zeros(shape)
    for i, cols in enumerate(rows):
        A[i, cols] = 1.0 + i
    return A


JACOBIANS = {
    # rows with no entry, rows with one entry, a row that reaches 4 columns; its columns reach 3 rows
    "mixed": dense([[], [2], [1, 3, 5], [], [0, 1], [6], [3, 5]], (7, 8)),
    "one_entry_rows": dense([[3], [0], [7]], (3, 8)),
    "empty": np.zeros((4, 6)),
    "one_wide_row": dense([[0, 9]], (1, 10)),
    "one_long_column": dense([[2], [], [], [2], [2]], (5, 4)),
}


@pytest.mark.parametrize("form", ["condensed", "normal"])
@pytest.mark.parametrize("name", sorted(JACOBIANS))
def test_gram_factor_bandwidth(lib, name, form):
    A = M.DeviceCSR.from_dense("cpu", JACOBIANS[name])
    got = gram_bw(lib, A, form)
    assert got == pattern_bandwidth(A, None, form)
    explicit = {("mixed", "condensed"): 4, ("mixed", "normal"): 4, ("one_entry_rows", "condensed"): 0,
                ("one_entry_rows", "normal"): 0, ("empty", "condensed"): 0, ("empty", "normal"): 0,
                ("one_wide_row", "condensed"): 9, ("one_wide_row", "normal"): 0, ("one_long_column", "condensed"): 0,
                ("one_long_column", "normal"): 4}
    assert got == explicit[(name, form)]


def test_hessian_wider_than_the_jacobian(lib):
    A = M.DeviceCSR.from_dense("cpu", JACOBIANS["mixed"])  # reach 4
    H = np.diag(np.arange(1.0, 9.0))
    H[6, 0] = H[0, 6] = 0.5  # |col - row| = 6
    H[3, 2] = H[2, 3] = 0.25
    Hs = M.DeviceSymCSR.from_dense("cpu", H)
    assert sym_bw(lib, Hs) == 6
    assert max(gram_bw(lib, A, "condensed"), sym_bw(lib, Hs)) == pattern_bandwidth(A, Hs, "condensed") == 6
    # ... and narrower: the Jacobian decides; a diagonal H (a vector, or a CSR of the diagonal alone) adds nothing
    Hn = M.DeviceSymCSR.from_dense("cpu", np.diag(np.arange(1.0, 9.0)) + np.diag(np.ones(7), 1) + np.diag(np.ones(7), -1))
    assert sym_bw(lib, Hn) == 1
    assert max(gram_bw(lib, A, "condensed"), sym_bw(lib, Hn)) == pattern_bandwidth(A, Hn, "condensed") == 4
    Hd = M.DeviceSymCSR.from_dense("cpu", np.diag(np.arange(1.0, 9.0)))
    assert sym_bw(lib, Hd) == 0 and pattern_bandwidth(A, Hd, "condensed") == 4
    # rows of H without an entry
    He = np.zeros((8, 8))
    He[5, 1] = He[1, 5] = 2.0
    assert sym_bw(lib, M.DeviceSymCSR.from_dense("cpu", He)) == 4
