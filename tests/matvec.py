"""Helpers of tests/test_gpu_matvec.py and tests/test_gemv_form.py: the dispatcher's report through the seam
madqp_debug_gemv_form, one dense product through madqp_gemv or madqp_debug_symv on poisoned operands, and the checks every
case shares.

Layout (csrc/gemv.hip).  Row r of the operand is contiguous, A[r * lda + c]; trans = 0 gives y(rows) = alpha A x + beta y,
trans = 1 gives y(cols) = alpha A' x + beta y.  The symmetric products read one side of the diagonal only: upper = 0 the
entries H[r * ldh + c] with c <= r, upper = 1 those with c >= r.

Tolerance (derived, not measured; the rule of tests/gemm_paths.py and tests/batched_ops.py).  With u = 2^-53, len the inner
length and S = |alpha| sum |a| |x| + |beta y0|, any order of summation, with or without FMA, satisfies
|out - exact| <= (len + 4) u S: len products, at most len - 1 inexact additions, alpha, beta and the final addition (an FMA
only removes roundings).  batched_ops.check_product holds every entry to (len + 4) u S against numpy.longdouble (exact
rationals where longdouble is no wider than double) and to 2 (len + 4) u S against float64 numpy.

Poison.  y lives in a NaN buffer with GUARD doubles on both sides: everything outside the output must come back bit for
bit.  The padding lda - cols of every row of A is NaN, and so is the side of a symmetric matrix that is not held: a finite
result has read none of them."""
import ctypes as C
import functools

import numpy as np
import torch

from batched_ops import LD, U, bits, check_product, same_bits, wide_rows  # noqa: F401  (re-exported for the tests)
from gemm_paths import dev as _dev

GUARD = 6
ERR_ARG = -1
PAIRS = [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)]  # (alpha, beta); beta = 0 runs over a NaN y
ALIGNED, OFF8 = 0x7F0000001000, 0x7F0000001008  # made-up addresses for the form query (never dereferenced)


def dev(a, be, shift=0):
    """Device copy of a host array (a fresh one: the shared operands are read-only); shift = 1: 8 bytes past a 16-byte
    boundary."""
    return _dev(np.array(a, dtype=np.float64), be, shift)


def form(lib, trans, rows, cols, A, lda, x):
    """madqp_debug_gemv_form for the tensors (or plain addresses) A and x.  Returns (rc, dict); form by name."""
    from madqp_jl_amd._lib import GEMV_FORMS, CDebugGemvForm

    adr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t
    info = CDebugGemvForm()
    rc = lib.madqp_debug_gemv_form(trans, rows, cols, adr(A), lda, adr(x), C.byref(info))
    d = {k: int(getattr(info, k)) for k, _ in CDebugGemvForm._fields_}
    d["form"] = GEMV_FORMS[d["form"]]
    return rc, d


def expect_form(got, label, **want):
    for k, v in want.items():
        assert got[k] == v, f"{label}: the dispatcher no longer takes this path ({k} = {got[k]}, expected {v}): {got}"


class Guarded:
    """`length` doubles of output inside a NaN buffer with GUARD doubles on either side, at a 16-byte boundary or
    (shift = 1) 8 bytes past one.  values: what the output holds before the call (NaN when None)."""

    def __init__(self, be, length, values=None, shift=0):
        self.length = length
        self.before = np.full(length + 2 * GUARD, np.nan)
        if values is not None:
            self.before[GUARD:GUARD + length] = values
        self.buf = dev(self.before, be, shift)
        self.t = self.buf[GUARD:GUARD + length] if length else None
        assert length == 0 or self.t.data_ptr() % 16 == 8 * shift

    def ptr(self):
        return None if self.t is None else self.t.data_ptr()

    def read(self, label):
        after = self.buf.cpu().numpy()
        mask = np.ones(after.shape, dtype=bool)
        mask[GUARD:GUARD + self.length] = False
        changed = mask & (bits(after) != bits(self.before))
        assert not changed.any(), f"{label}: {int(changed.sum())} doubles outside the output were written, first at offset " \
                                  f"{int(np.argmax(changed)) - GUARD} from y[0] (length {self.length})"
        return after[GUARD:GUARD + self.length].copy()


@functools.lru_cache(maxsize=None)
def operands(rows, cols):
    """(A (rows, cols), x for trans = 0, x for trans = 1, y0 for trans = 0, y0 for trans = 1): seeded, shared by every
    case of the shape, never modified."""
    rng = np.random.default_rng(rows * 100003 + cols)
    out = (rng.standard_normal((rows, cols)), rng.standard_normal(cols), rng.standard_normal(rows),
           rng.standard_normal(rows), rng.standard_normal(cols))
    for a in out:
        a.setflags(write=False)
    return out


def padded(A, lda):
    """A (rows, cols) in storage (rows, lda) whose padding columns are NaN"""
    out = np.full((A.shape[0], lda), np.nan)
    out[:, :A.shape[1]] = A
    return out


def run_gemv(be, trans, rows, cols, lda, want, label, *, a_off=0, x_off=0, y_off=0):
    """One shape through madqp_gemv for every (alpha, beta) of PAIRS: the dispatcher's report for the very pointers passed
    must equal `want`, the guards must come back untouched and every entry must meet the derived bound.  Returns the
    worst err / bound against the extended-precision reference."""
    A, x0, x1, y0n, y0t = operands(rows, cols)
    x, y0 = (x1, y0t) if trans else (x0, y0n)
    Mx = A.T if trans else A
    Ad = dev(padded(A, lda), be, a_off) if A.size else dev(np.full(2, np.nan), be, a_off)
    xd = dev(x, be, x_off) if x.size else dev(np.full(2, np.nan), be, x_off)
    rc, got = form(be.lib, trans, rows, cols, Ad, lda, xd)
    assert rc == 0, (label, rc)
    expect_form(got, label, **want)
    wide = wide_rows(Mx, x)
    worst = 0.0
    for alpha, beta in PAIRS:
        y = Guarded(be, Mx.shape[0], values=y0 if beta != 0.0 else None, shift=y_off)
        rc = be.lib.madqp_gemv(be.ctx, trans, rows, cols, alpha, Ad.data_ptr(), lda, xd.data_ptr(), beta, y.ptr())
        assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
        out = y.read(f"{label} alpha {alpha} beta {beta}")
        worst = max(worst, check_product(out, Mx, x, alpha, beta, y0, f"{label} alpha {alpha} beta {beta}", wide=wide))
    print(f"[matvec] {label}: trans {trans} rows {rows} cols {cols} lda {lda} {got} err/bound {worst:.3e} (extended, "
          f"bound (len+4)uS)")
    return worst


# ---------------------------------------------------------------------------------------------- symmetric products
@functools.lru_cache(maxsize=None)
def sym_operands(n):
    """(H symmetric (n, n), x, y0, the extended-precision row sums of H x): seeded, shared by both sides and both leading
    dimensions of the order."""
    rng = np.random.default_rng(7 * n + 1)
    G = rng.standard_normal((n, n))
    H = G + G.T
    x, y0 = rng.standard_normal(n), rng.standard_normal(n)
    for a in (H, x, y0):
        a.setflags(write=False)
    return H, x, y0, wide_rows(H, x)


def one_side(H, ldh, upper):
    """storage (n, ldh): the held side of H (upper = 0: c <= r; 1: c >= r), NaN on the strict other side and in the padding"""
    n = H.shape[0]
    out = np.full((n, ldh), np.nan)
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    held = (c >= r) if upper else (c <= r)
    out[:, :n][held] = H[held]
    return out


def symv_work_doubles(n):
    """doubles of the context's workspace one symmetric product of order n uses: a row part per 512-column tile and a
    column part per 256-row tile (csrc/gemv.hip: symv_tri)"""
    return ((n + 255) // 256 + (n + 511) // 512) * n


class WorkspacePoison:
    """NaN into the context's workspace through the public API: the chunked A' x of an all-NaN matrix leaves chunks * cols
    NaN partials at its start -- the doubles the symmetric products then use for theirs (symv_tri and the chunked product
    share ctx->d_work).  A partial that is read but was never written then shows as NaN, not as a plausible stale number."""
    ROWS, COLS, LDA = 1024, 2047, 2048  # 16 tiles of 128 columns x 16 chunks of 64 rows: 32 752 partials

    def __init__(self, be):
        self.be = be
        self.A = torch.full((self.ROWS * self.LDA,), float("nan"), dtype=torch.float64, device=be.device)
        self.x = torch.ones(self.ROWS, dtype=torch.float64, device=be.device)
        self.y = torch.zeros(self.COLS, dtype=torch.float64, device=be.device)
        rc, got = form(be.lib, 1, self.ROWS, self.COLS, self.A, self.LDA, self.x)
        assert rc == 0 and got["form"] == "t_chunked", got
        self.doubles = got["chunks"] * self.COLS

    def apply(self, need):
        assert self.doubles >= need, (self.doubles, need)
        be = self.be
        rc = be.lib.madqp_gemv(be.ctx, 1, self.ROWS, self.COLS, 1.0, self.A.data_ptr(), self.LDA, self.x.data_ptr(), 0.0,
                               self.y.data_ptr())
        assert rc == 0, (rc, be.lib.madqp_last_error(be.ctx))


def run_symv(be, poison, upper, n, ldh, label):
    """One order and leading dimension through madqp_debug_symv for every (alpha, beta) of PAIRS, each twice over a freshly
    poisoned workspace: the same bits both times, guards untouched, every entry within (n + 4) u S of the full symmetric
    product.  Returns the worst err / bound against the extended-precision reference."""
    H, x, y0, wide = sym_operands(n)
    Hd, xd = dev(one_side(H, ldh, upper), be), dev(x, be)
    worst = 0.0
    for alpha, beta in PAIRS:
        outs = []
        for rep in range(2):
            poison.apply(symv_work_doubles(n))
            y = Guarded(be, n, values=y0 if beta != 0.0 else None)
            rc = be.lib.madqp_debug_symv(be.ctx, upper, n, alpha, Hd.data_ptr(), ldh, xd.data_ptr(), beta, y.ptr())
            assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
            outs.append(y.read(f"{label} alpha {alpha} beta {beta} run {rep}"))
        lab = f"{label} alpha {alpha} beta {beta}"
        worst = max(worst, check_product(outs[0], H, x, alpha, beta, y0, lab, wide=wide))
        assert same_bits(outs[0], outs[1]), \
            f"{lab}: two runs differ at {np.flatnonzero(bits(outs[0]) != bits(outs[1]))[:8]}: the summation order is not fixed"
    print(f"[matvec] {label}: upper {upper} n {n} ldh {ldh} err/bound {worst:.3e} (extended, bound (n+4)uS)")
    return worst
