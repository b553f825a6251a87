"""Helpers of tests/test_gpu_batched_ops.py: one workgroup helper of the batched engine (csrc/batch_wg.inc) through the seam
madqp_debug_batch_op, the batched Cholesky through madqp_debug_chol_factor_batched, their references and shared checks.

Layout.  The engine holds H and A row-major (row k contiguous), K and its factor column-major with a leading dimension; on
the host a column-major matrix is an array (columns, ld) whose row j is column j.

Products (derived, not measured; tests/gemm_paths.py has the same rule).  With S the same expression in absolute values,
u = 2^-53 and len the length of the inner sum, any order of summation without FMA (the library is built with
-ffp-contract=off), zero terms added or not, satisfies |out - exact| <= (len + 4) u S: len products, at most len - 1
inexact additions, alpha, beta and the final addition.  Every entry is held to (len + 4) u S against numpy.longdouble
(exact rationals where longdouble is no wider than double) and to 2 (len + 4) u S against float64 numpy.  For the
multiply-on-load instantiations the reference matrix is fl(ms * M) formed in float64: the double the kernel is specified to
use.

The block solve and the factorisation (measured).  Multiplying by a stored inverse is only conditionally stable, so their
figures are ratios: the componentwise error over the running magnitude of the same formula in absolute values (solve with
caller-made factors), the componentwise residual |A - L L'| / (u |L| |L|') and the normwise backward error of the solve
(factorisation), each computed in longdouble -- for the device AND for a float64 numpy restatement of the same algorithm
(128-column blocks, panel solve with 16 x 16 sub-block inverses, inverse-image sweeps), at run time.  The device is held to
MARGIN x the restatement's figure (both compute the same sums in different orders: the same worst-case bound covers each).
Every problem is compared with the restatement's figure for the SAME problem.  MARGIN is the smallest power of two at least
twice the worst device / restatement ratio seen over all cases and problems on an MI355X -- 3.43, the residual of the
well-conditioned problem of order 127 (DESIGN 4.5 has the table) -- and may not exceed 8."""
import ctypes as C
from fractions import Fraction

import numpy as np
import scipy.linalg as sla
import torch

U = 2.0 ** -53
NB = 128
SB = 16
WBLK = 2 * NB * NB
MS = 0.37109375 * np.pi  # the factor of the multiply-on-load cases: not a power of two
LD = np.longdouble
LD_OK = float(np.finfo(LD).eps) < 2.0 ** -60
MARGIN = 8.0  # smallest power of two >= 2 x 3.43
OPS = {"gemv_n": 0, "gemv_n_then_t": 1, "gemv_t": 2, "symv_lower": 3, "chol_solve": 4, "prewrite_h": 5}
FORMS = [(256, 0), (512, 0), (256, 1), (512, 1)]  # (tpb, shared)
ERR_ARG = -1


def sym_doubles(tpb):
    return (tpb // 64 + 1) * 512


# ---------------------------------------------------------------------------------------------- device plumbing
def dev(a, be):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel().copy()).to(be.device)


def i32dev(a, be):
    return torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.int32)), device=be.device)


def host(t):
    return t.cpu().numpy()


def seam(be, op, tpb, shared, nprob, **f):
    """One madqp_debug_batch_op.  Fields by name, tensors for device pointers.  Returns the return code."""
    from madqp_jl_amd._lib import CDebugBatchOp

    a = CDebugBatchOp(op=OPS[op] if isinstance(op, str) else op, tpb=tpb, shared=shared, nprob=nprob, alpha=1.0, beta=0.0, ms=1.0)
    keep = []
    for k, v in f.items():
        if isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        setattr(a, k, v)
    return be.lib.madqp_debug_batch_op(be.ctx, C.byref(a))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Slices:
    """nprob slices of `length` doubles at stride length + pad, three more doubles behind the last; NaN unless given.
    Everything outside [b * stride, b * stride + length) must come back bit for bit (assert_rest_untouched)."""

    def __init__(self, be, nprob, length, pad=3, values=None):
        self.nprob, self.length, self.stride = nprob, length, length + pad
        self.before = np.full(nprob * self.stride + 3, np.nan)
        if values is not None:
            self.view(self.before)[:] = values
        self.t = dev(self.before, be)

    def view(self, flat):
        return flat[:self.nprob * self.stride].reshape(self.nprob, self.stride)[:, :self.length]

    def read(self, label):
        after = host(self.t)
        mask = np.ones(after.shape, dtype=bool)
        self.view(mask)[:] = False
        changed = mask & (bits(after) != bits(self.before))
        assert not changed.any(), f"{label}: {int(changed.sum())} doubles outside the output slices were written, first at flat " \
                                  f"index {int(np.argmax(changed))} (stride {self.stride}, length {self.length})"
        return self.view(after).copy()


# ---------------------------------------------------------------------------------------------- product references
def wide_rows(Mx, x):
    """(sum_j M[i][j] x[j], sum_j |M[i][j] x[j]|) per row in extended precision."""
    if Mx.shape[1] == 0:
        return np.zeros(Mx.shape[0], dtype=LD), np.zeros(Mx.shape[0], dtype=LD)
    if LD_OK:
        p = Mx.astype(LD) * x.astype(LD)[None, :]
        return p.sum(axis=1), np.abs(p).sum(axis=1)
    F = Fraction
    ref, S = np.zeros(Mx.shape[0]), np.zeros(Mx.shape[0])
    for i in range(Mx.shape[0]):
        pr = [F(float(a)) * F(float(b)) for a, b in zip(Mx[i], x)]
        ref[i], S[i] = float(sum(pr, F(0))), float(sum(map(abs, pr), F(0)))
    return ref.astype(LD), S.astype(LD)


def check_product(out, Mx, x, alpha, beta, y0, label, wide=None):
    """out = alpha * Mx @ x + beta * y0 (y0 ignored when beta == 0), inner length Mx.shape[1]; returns the worst err / bound
    against the extended-precision reference.  wide: wide_rows(Mx, x) where the caller shares it among several checks."""
    n = Mx.shape[1]
    assert np.all(np.isfinite(out)), f"{label}: non-finite entries at {np.flatnonzero(~np.isfinite(out))[:8]}"
    add = beta * y0 if beta != 0.0 else np.zeros(Mx.shape[0])
    ref64 = alpha * (Mx @ x) + add
    S64 = abs(alpha) * (np.abs(Mx) @ np.abs(x)) + np.abs(add)
    err, bound = np.abs(out - ref64), 2.0 * (n + 4) * U * S64
    bad = ~(err <= bound)
    assert not bad.any(), f"{label}: {int(bad.sum())} entries beyond 2 (len + 4) u S against float64, first at {int(np.argmax(bad))}: " \
                          f"out {out[np.argmax(bad)]!r} ref {ref64[np.argmax(bad)]!r} bound {bound[np.argmax(bad)]:.3e}"
    w, Sw = wide_rows(Mx, x) if wide is None else wide
    ref = LD(alpha) * w + add.astype(LD)
    S = LD(abs(alpha)) * Sw + np.abs(add).astype(LD)
    err, bound = np.abs(out.astype(LD) - ref), LD((n + 4) * U) * S
    bad = ~(err <= bound)
    assert not bad.any(), f"{label}: {int(bad.sum())} entries beyond (len + 4) u S against the extended-precision reference, first " \
                          f"at {int(np.argmax(bad))}: out {out[np.argmax(bad)]!r} ref {float(ref[np.argmax(bad)])!r} " \
                          f"err {float(err[np.argmax(bad)]):.3e} bound {float(bound[np.argmax(bad)]):.3e}"
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def matrix_operands(seed, nprob, rows, cols, vec_len):
    """(M (nprob, rows, cols), x (nprob, vec_len)) from seeded standard_normal."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nprob, rows, cols)), rng.standard_normal((nprob, vec_len))


def run_gemv_n(be, tpb, shared, M, x, alpha, beta, y0, label):
    """y(rows) = alpha M x + beta y for every problem of the stack M (nprob, rows, cols); returns y (nprob, rows)."""
    nprob, rows, cols = M.shape
    y = Slices(be, nprob, rows, values=y0 if beta != 0.0 else None)
    Md, xd = dev(np.concatenate([M.reshape(nprob, rows * cols), np.full((nprob, 5), np.nan)], axis=1), be), dev(x, be)
    rc = seam(be, "gemv_n", tpb, shared, nprob, rows=rows, cols=cols, alpha=alpha, beta=beta, M=Md, sM=rows * cols + 5,
              x=xd, sx=x.shape[1], y=y.t, sy=y.stride)
    assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
    return y.read(label)


def run_gemv_n_then_t(be, tpb, shared, M, x, theta, t, label):
    """(u (nprob, rows), at (nprob, cols)) of wg_gemv_n_then_t<8>."""
    nprob, rows, cols = M.shape
    u, at = Slices(be, nprob, rows), Slices(be, nprob, cols, pad=1)
    Md, xd, thd, td = dev(M, be), dev(x, be), dev(theta, be), dev(t, be)
    rc = seam(be, "gemv_n_then_t", tpb, shared, nprob, rows=rows, cols=cols, M=Md, sM=rows * cols, x=xd, sx=x.shape[1],
              y=u.t, sy=u.stride, theta=thd, t=td, st=theta.shape[1], at=at.t, sat=at.stride)
    assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
    return u.read(label + " u"), at.read(label + " at")


def run_gemv_t(be, tpb, shared, M, v, alpha, beta, y0, ms, label, raw=True):
    """(out (nprob, cols), raw (nprob, cols) or None) of wg_gemv_t: out = alpha (ms M)' v + beta out."""
    nprob, rows, cols = M.shape
    out = Slices(be, nprob, cols, values=y0 if beta != 0.0 else None)
    rw = Slices(be, nprob, cols, pad=2) if raw else None
    Md, vd = dev(np.concatenate([M.reshape(nprob, rows * cols), np.full((nprob, 1), np.nan)], axis=1), be), dev(v, be)
    f = dict(raw=rw.t, sraw=rw.stride) if raw else {}
    rc = seam(be, "gemv_t", tpb, shared, nprob, rows=rows, cols=cols, alpha=alpha, beta=beta, ms=ms, M=Md, sM=rows * cols + 1,
              x=vd, sx=v.shape[1], y=out.t, sy=out.stride, **f)
    assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
    return out.read(label), (rw.read(label + " raw") if raw else None)


def run_symv(be, tpb, shared, Hlow, x, alpha, beta, y0, ms, label, raw=True):
    """(y, raw, sym scratch after the call) of wg_symv_lower on the stack Hlow (nprob, n, n) as given (the caller decides what
    the strict upper triangle holds)."""
    nprob, n, _ = Hlow.shape
    y = Slices(be, nprob, n, values=y0 if beta != 0.0 else None)
    rw = Slices(be, nprob, n, pad=2) if raw else None
    sym = Slices(be, nprob, sym_doubles(tpb), pad=4)
    Hd, xd = dev(Hlow, be), dev(x, be)
    f = dict(raw=rw.t, sraw=rw.stride) if raw else {}
    rc = seam(be, "symv_lower", tpb, shared, nprob, rows=n, cols=n, alpha=alpha, beta=beta, ms=ms, M=Hd, sM=n * n, x=xd,
              sx=x.shape[1], y=y.t, sy=y.stride, sym=sym.t, ssym=sym.stride, **f)
    assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
    return y.read(label), (rw.read(label + " raw") if raw else None), sym.read(label + " sym")


# ---------------------------------------------------------------------------------------------- the block solve
def npad_of(n):
    return (n + NB - 1) // NB * NB


def blocks_of(n):
    return [(j, min(n, j + NB)) for j in range(0, n, NB)]


def tri_inverse_ld(Ljj):
    """inverse of a lower triangular block by substitution in longdouble"""
    w = Ljj.shape[0]
    Ll = Ljj.astype(LD)
    Wl = np.eye(w, dtype=LD)
    for i in range(w):
        Wl[i, :] = (Wl[i, :] - Ll[i, :i] @ Wl[:i, :]) / Ll[i, i]
    return Wl


def images_of(Ws, poison=True):
    """The inverse images as potf2_inv_body lays them out, one WBLK per block: forward image img[i + c * 128] = W(i, c) for
    i >= c, then the backward image img[i + c * 128] = W(c, i) for i <= c; a short block is padded with the identity.
    poison: the zero halves of both images hold NaN (wg_block_matvec never fetches them)."""
    out = np.zeros((len(Ws), 2, NB, NB))  # [block][image][c][i]
    for k, W in enumerate(Ws):
        Wp = np.eye(NB)
        Wp[:W.shape[0], :W.shape[0]] = W
        Wp = np.tril(Wp)
        out[k, 0] = Wp.T  # [c][i] = W(i, c)
        out[k, 1] = Wp    # [c][i] = W(c, i)
        if poison:
            c, i = np.meshgrid(np.arange(NB), np.arange(NB), indexing="ij")
            out[k, 0][i < c] = np.nan
            out[k, 1][i > c] = np.nan
    return out.reshape(len(Ws) * WBLK)


def sweep_formula(L, Ws, b, dtype, mag=False):
    """x = (L L')^-1 b by the engine's block formula in `dtype`: x_J = W_J (b_J - sum_I L_JI x_I), then the transposed pass.
    mag: the same formula in absolute values (the running magnitude)."""
    n = L.shape[0]
    f = (lambda a: np.abs(a).astype(dtype)) if mag else (lambda a: a.astype(dtype))
    Lw, Ww = f(L), [f(W) for W in Ws]
    sgn = 1 if mag else -1
    mv = lambda A, v: (A * v[None, :]).sum(axis=1) if A.shape[1] else np.zeros(A.shape[0], dtype=dtype)  # (products rounded, then summed: no FMA)
    y = f(b).copy()
    blk = blocks_of(n)
    for k, (j0, j1) in enumerate(blk):
        y[j0:j1] = mv(Ww[k], y[j0:j1] + sgn * mv(Lw[j0:j1, :j0], y[:j0]))
    for k in range(len(blk) - 1, -1, -1):
        j0, j1 = blk[k]
        y[j0:j1] = mv(Ww[k].T, y[j0:j1] + sgn * mv(Lw[j1:, j0:j1].T, y[j1:]))
    return y


def solve_ratio(x, L, Ws, b):
    """max_i |x_i - x_ref_i| / (u mag_i): reference and magnitude by sweep_formula in longdouble"""
    ref = sweep_formula(L, Ws, b, LD)
    mag = sweep_formula(L, Ws, b, LD, mag=True)
    return float(np.max(np.abs(x.astype(LD) - ref) / (LD(U) * mag)))


def made_factor(seed, n):
    """A well-conditioned L (diagonal in [1, 2], strictly lower part standard_normal / sqrt(n)), the images of its diagonal
    blocks' inverses (longdouble, rounded once) and a right-hand side."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((n, n)) / np.sqrt(n), -1) + np.diag(rng.uniform(1.0, 2.0, n))
    Ws = [tri_inverse_ld(L[j0:j1, j0:j1]).astype(np.float64) for j0, j1 in blocks_of(n)]
    return L, Ws, rng.standard_normal(n)


def colmajor(Mat, lda, ncols, fill):
    """Mat (r x c) into a column-major array (ncols, lda) filled with `fill` elsewhere"""
    out = np.full((ncols, lda), fill)
    out[:Mat.shape[1], :Mat.shape[0]] = Mat.T
    return out


def run_chol_solve(be, tpb, shared, Lcm, lda, winv, n, rhs, label, sL=None, sW=None):
    """rhs (nprob, n) <- (L L')^-1 rhs; Lcm / winv: device tensors or host arrays of nprob problems."""
    nprob = rhs.shape[0]
    r = Slices(be, nprob, n, values=rhs)
    Ld = Lcm if isinstance(Lcm, torch.Tensor) else dev(Lcm, be)
    Wd = winv if isinstance(winv, torch.Tensor) else dev(winv, be)
    rc = seam(be, "chol_solve", tpb, shared, nprob, rows=n, ld=lda, M=Ld, sM=Ld.numel() // nprob if sL is None else sL,
              y=r.t, sy=r.stride, winv=Wd, sW=Wd.numel() // nprob if sW is None else sW)
    assert rc == 0, (label, rc, be.lib.madqp_last_error(be.ctx))
    return r.read(label)


# ---------------------------------------------------------------------------------------------- the batched factorisation
def spd_batch(seed, n, B=4):
    """B SPD matrices G'G / k + I of mixed conditioning (the columns of G scaled by 1, 10, 100, 300: condition numbers from
    ~10 to ~1e6) and one right-hand side each."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 2)
    As = []
    for b in range(B):
        G = rng.standard_normal((k, n)) * (1.0, 10.0, 100.0, 300.0)[b % 4]
        As.append(G.T @ G / k + np.eye(n))
    return np.stack(As), rng.standard_normal((B, n))


def diag_block_restated(Ablk):
    """potf2_inv_body in float64 numpy: the w x w diagonal block (lower triangle of Ablk) in steps of 16 columns -- the
    16 x 16 sub-block by Cholesky, its inverse W_JJ by substitution, the rows below it INSIDE the block as the product
    L_IJ = A_IJ W_JJ' (an explicit inverse here too, not a substitution), the trailing update -- and the inverse of the block's
    factor by the block recurrence W_IJ = -W_II sum_{K=J}^{I-1} L_IK W_KJ.  Returns (L_jj, W)."""
    w = Ablk.shape[0]
    L = np.tril(Ablk).copy()
    sub = [(a, min(w, a + SB)) for a in range(0, w, SB)]
    W = np.zeros((w, w))
    for a, b in sub:
        Ljj = np.linalg.cholesky(L[a:b, a:b])  # raises LinAlgError like the oracle's cho_factor
        L[a:b, a:b] = Ljj
        W[a:b, a:b] = sla.solve_triangular(Ljj, np.eye(b - a), lower=True)
        if b < w:
            L[b:, a:b] = L[b:, a:b] @ W[a:b, a:b].T
            L[b:, b:] -= np.tril(L[b:, a:b] @ L[b:, a:b].T)
    for I, (a, b) in enumerate(sub):
        for c, d in sub[:I]:
            W[a:b, c:d] = -W[a:b, a:b] @ (L[a:b, c:a] @ W[c:a, c:d])
    return np.tril(L), W


class BlockCholRestated:
    """float64 numpy restatement of the device's algorithm (after tools/numerics/blockchol_emul.py): 128-column blocks, left
    looking; the diagonal block and its inverse as potf2_inv_body forms them (diag_block_restated); the panel below a block
    by block substitution with the inverses of the 16 x 16 diagonal sub-blocks (panel_sub16_kernel); the sweeps as products
    with the 128 x 128 inverses."""

    def __init__(self, A):
        n = A.shape[0]
        L = np.tril(A).copy()
        self.W = []
        for j0, j1 in blocks_of(n):
            if j0:
                L[j0:, j0:j1] -= L[j0:, :j0] @ L[j0:j1, :j0].T
            Ljj, Wjj = diag_block_restated(L[j0:j1, j0:j1])
            L[j0:j1, j0:j1] = Ljj
            self.W.append(Wjj)
            if j1 < n:
                Cm, w = L[j1:, j0:j1], j1 - j0
                X = np.zeros_like(Cm)
                for a in range(0, w, SB):
                    b = min(w, a + SB)
                    X[:, a:b] = (Cm[:, a:b] - X[:, :a] @ Ljj[a:b, :a].T) @ Wjj[a:b, a:b].T
                L[j1:, j0:j1] = X
        self.L = np.tril(L)

    def solve(self, b):
        return sweep_formula(self.L, self.W, b, np.float64)


def residual_rows(n):
    """Rows whose residual entries are measured: all of them up to order 200; beyond that the rows on both sides of every
    block boundary, the first and the last, and 16 seeded ones (longdouble products run at ~1e8 flop/s).  Device, restatement
    and LAPACK are measured on the same rows."""
    if n <= 200:
        return np.arange(n)
    edge = [0, n - 1] + [j + d for j in range(NB, n, NB) for d in (-1, 0, 1)]
    rnd = np.random.default_rng(n).choice(n, 16, replace=False)
    return np.unique(np.clip(np.concatenate([edge, rnd]), 0, n - 1))


def factor_residual(A, L):
    """max over the measured rows i and all j <= i of |A - L L'| / (u |L| |L|'): the product in longdouble (the denominator in
    float64: it only scales)"""
    Lt = np.tril(L)
    aL = np.abs(Lt)
    worst = 0.0
    for i in residual_rows(A.shape[0]):
        P = Lt[:i + 1, :i + 1].astype(LD) @ Lt[i, :i + 1].astype(LD)
        q = np.abs(A[i, :i + 1].astype(LD) - P) / (LD(U) * (aL[:i + 1, :i + 1] @ aL[i, :i + 1]).astype(LD))
        worst = max(worst, float(np.max(q)) if np.all(np.isfinite(q)) else np.inf)
    return worst


def factor_residual_f64(A, L):
    """The same figure over EVERY entry of the lower triangle with the product in float64.  Its own rounding adds up to
    (n + 1) units in the worst case and about sqrt(n) in practice -- the same for any factor of the same matrix, so it is
    compared between factors, not read as a residual: an entry of L that is wrong shows as 1e10, wherever it lies."""
    Lt = np.tril(L)
    q = np.abs(A - Lt @ Lt.T) / (U * (np.abs(Lt) @ np.abs(Lt).T))
    low = np.tril(np.ones(A.shape, dtype=bool))
    return float(np.max(q[low])) if np.all(np.isfinite(q[low])) else np.inf


def backward_error(A, x, b):
    """normwise backward error |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) in units of u, in longdouble"""
    Al, xl, bl = A.astype(LD), x.astype(LD), b.astype(LD)
    r = np.max(np.abs(bl - Al @ xl))
    return float(r / (np.max(np.abs(Al).sum(axis=1)) * np.max(np.abs(xl)) + np.max(np.abs(bl))) / LD(U))


def k_storage(As, lda, pad_rows=0.0, upper=np.nan):
    """(B, npad, lda) column-major storage of the lower triangles: strict upper triangle `upper`, rows n .. of the columns
    < n `pad_rows` (a value or a callable shape -> array), columns n .. zero."""
    B, n, _ = As.shape
    ncols = npad_of(n)
    K = np.zeros((B, ncols, lda))
    for b in range(B):
        Kb = K[b]
        Kb[:n, :n] = np.tril(As[b]).T  # [j][i] = A(i, j), i >= j
        jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        Kb[:n, :n][ii < jj] = upper
        Kb[:n, n:] = pad_rows((n, lda - n)) if callable(pad_rows) else pad_rows
    return K


def factor_batched(be, K, lda, n, winv=None, skip=None, lst=None, slots=0, info0=None):
    """madqp_debug_chol_factor_batched on the host storage K (B, npad, lda); returns (rc, K after, winv after, info) and
    the device tensors (Kd, Wd) for a solve behind it."""
    B = K.shape[0]
    nblk = npad_of(n) // NB
    Kd = dev(np.concatenate([K.ravel(), np.zeros(128)]), be)  # (the slack the engine allocates behind its K)
    Wd = dev(np.zeros(B * nblk * WBLK) if winv is None else winv, be)
    info = i32dev(np.full(B, 77, dtype=np.int32) if info0 is None else info0, be)
    sk = i32dev(skip, be) if skip is not None else None
    ls = i32dev(lst if len(lst) else [0], be) if lst is not None else None
    cnt = i32dev([len(lst)], be) if lst is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = be.lib.madqp_debug_chol_factor_batched(be.ctx, Kd.data_ptr(), lda, n, K.shape[1] * lda, Wd.data_ptr(), nblk * WBLK,
                                                info.data_ptr(), B, ptr(sk), slots, ptr(ls), ptr(cnt))
    torch.cuda.synchronize()
    return rc, host(Kd)[:K.size].reshape(K.shape), host(Wd).reshape(B, nblk * WBLK), host(info), (Kd, Wd)


def lower_of(Kb, n):
    """the n x n lower triangular factor held in column-major storage (npad, lda)"""
    return np.tril(Kb[:n, :n].T)
