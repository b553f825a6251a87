"""Dense QP held in HBM and the on-device synthetic instance generator.

    min c0 + q'x + x'Hx/2   s.t.  lcon <= A x <= ucon,  lvar <= x <= uvar

``H`` is a full symmetric (nx, nx) tensor (or None for an LP) and ``A`` an
(m, nx) row-major tensor: the layouts the MFMA kernels consume directly.
The sparse front end takes ``A`` as a :class:`DeviceCSR` and ``H`` dense, as a
1-D tensor (its diagonal) or as a :class:`DeviceSymCSR`.
The synthetic family is the one of BASELINE.md section 3; entries are produced
in place on the device by ``madqp_gen_*`` and are bit-identical to the CPU
generator the tests use.
"""
from __future__ import annotations

import math

import numpy as np
import torch

_MASK = 0xFFFFFFFFFFFFFFFF
STREAM_A, STREAM_H, STREAM_Q = 1, 2, 3


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def stream_key(seed: int, stream: int) -> int:
    """Per-(seed, stream) generator key (host side of ``madqp_gen_normal``)."""
    return _mix64((seed ^ ((stream * 0xD1B54A32D192ED03) & _MASK)) & _MASK)


def csr_plan(I, J, nrows, ncols, kind):
    """``madqp_csr_map_plan_host`` for a 0-based host pattern (duplicates allowed): ``(rows, ptr, col, seg, src)`` as
    numpy int64 arrays -- the CSR structure ``madqp_csr_map_create`` would upload and, per stored entry, the COO positions
    ``src[seg[d]:seg[d + 1]]`` of its sources in ascending order.  Host only: the library is loaded, no device is touched."""
    import ctypes as C

    from . import _lib

    I, J = np.asarray(I, dtype=np.int64).ravel(), np.asarray(J, dtype=np.int64).ravel()
    if len(I) != len(J):
        raise ValueError("I and J of the sparsity pattern differ in length")
    if len(I) and (min(I.min(), J.min()) < 0 or max(I.max(), J.max()) >= 2 ** 31 - 1):
        raise ValueError("index out of range in the sparsity pattern")
    I1, J1 = np.ascontiguousarray(I + 1, dtype=np.int32), np.ascontiguousarray(J + 1, dtype=np.int32)  # 1-based, as MadNLP's
    lib, k = _lib.load_cdll(), _lib.CSR_KINDS.index(kind)
    sizes = (C.c_int64 * 3)()
    head = (len(I1), I1.ctypes.data, J1.ctypes.data, int(nrows), int(ncols), k, sizes)
    if lib.madqp_csr_map_plan_host(*head, None, None, None, None) != 0:
        raise ValueError(f"sparsity pattern refused: an entry outside {nrows} x {ncols}, or kind {kind!r} does not fit")
    rows, stored, sources = sizes
    ptr, col = np.zeros(rows + 1, dtype=np.int64), np.zeros(stored, dtype=np.int64)
    seg, src = np.zeros(stored + 1, dtype=np.int64), np.zeros(sources, dtype=np.int64)
    rc = lib.madqp_csr_map_plan_host(*head, ptr.ctypes.data, col.ctypes.data, seg.ctypes.data, src.ctypes.data)
    assert rc == 0, rc
    return rows, ptr, col, seg, src


def _csr_values(vals, seg, src):
    """The value rule of ``madqp_csr_map_apply`` on the host: per stored entry, its sources added one after the other
    from +0.0 in ascending COO position (``numpy.add.at`` is unbuffered and takes the indices in order)."""
    vals = np.asarray(vals, dtype=np.float64).ravel()
    out = np.zeros(len(seg) - 1)
    np.add.at(out, np.repeat(np.arange(len(seg) - 1), np.diff(seg)), vals[src])
    return out


class DeviceCSR:
    """A sparse Jacobian on the device: CSR of A (``ptr, col, val``; m rows, column indices ascending within
    a row) plus what the transposed products need -- the CSR of A' (``t_ptr, t_col``) and the permutation
    ``t_perm`` with ``val_of_At = val[t_perm]`` -- and ``row`` (row index of every stored entry).  The
    pattern is built once on the host (A is constant for a QP), the reference's ``coo_to_csr``
    (src/utils.jl:148-197) in spirit; values can be rescaled on the device without touching it."""

    def __init__(self, device, m, n, rows, cols, vals):
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        vals = np.asarray(vals, dtype=np.float64)
        order = np.lexsort((cols, rows))  # by row, then column
        rows, cols, vals = rows[order], cols[order], vals[order]
        if len(rows) > 1 and np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])):
            raise ValueError("duplicate entries in the sparse Jacobian")
        t_perm = np.lexsort((rows, cols))  # by column, then row: the order of the entries of A'
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=device)
        count = lambda idx, k: np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=k))])
        self.m, self.n, self.nnz = int(m), int(n), len(vals)
        self.ptr, self.col, self.val = dev(count(rows, m), torch.int64), dev(cols, torch.int64), dev(vals, torch.float64)
        self.row = dev(rows, torch.int64)
        self.t_ptr, self.t_col = dev(count(cols, n), torch.int64), dev(rows[t_perm], torch.int64)
        self.t_perm = dev(t_perm, torch.int64)

    @classmethod
    def from_dense(cls, device, A):
        A = np.asarray(A, dtype=np.float64)
        r, c = np.nonzero(A)
        return cls(device, A.shape[0], A.shape[1], r, c, A[r, c])

    @classmethod
    def from_coo(cls, device, m, n, I, J, vals):
        """From a COO pattern as a model reports it (0-based host arrays, any order, duplicates allowed) and its values:
        duplicates are summed in COO order.  Built on ``madqp_csr_map_plan_host`` -- the plan the device maps
        (``madqp_csr_map_create``, kinds rows and cols) upload -- so the container equals what the maps produce."""
        vals = np.asarray(vals, dtype=np.float64).ravel()
        if len(vals) != len(np.ravel(I)):
            raise ValueError("vals and the sparsity pattern differ in length")
        m, n = int(m), int(n)
        _, ptr, col, seg, src = csr_plan(I, J, m, n, "rows")
        _, t_ptr, t_col, _, _ = csr_plan(I, J, m, n, "cols")
        rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
        t_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(t_ptr))  # column of A of every entry of A'
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=device)
        out = object.__new__(cls)
        out.m, out.n, out.nnz = m, n, len(col)
        out.ptr, out.col, out.row = dev(ptr, torch.int64), dev(col, torch.int64), dev(rows, torch.int64)
        out.val = dev(_csr_values(vals, seg, src), torch.float64)
        out.t_ptr, out.t_col = dev(t_ptr, torch.int64), dev(t_col, torch.int64)
        # entry (r, c) of A' order sits at the position of key r * n + c among the (ascending) keys of A's order
        out.t_perm = dev(np.searchsorted(rows * n + col, t_col * n + t_rows), torch.int64)
        return out

    def scaled(self, row_scale):
        """A copy that shares the pattern, with row i multiplied by ``row_scale[i]``."""
        out = object.__new__(DeviceCSR)
        out.__dict__.update(self.__dict__)
        out.val = (self.val * row_scale[self.row]).contiguous()
        return out

    @property
    def t_val(self):
        return self.val[self.t_perm].contiguous()

    def row_absmax(self):
        out = torch.zeros(self.m, dtype=torch.float64, device=self.val.device)
        return out.scatter_reduce(0, self.row, self.val.abs(), reduce="amax", include_self=True)

    def to_dense(self):
        A = torch.zeros((self.m, self.n), dtype=torch.float64, device=self.val.device)
        A[self.row, self.col] = self.val
        return A


class DeviceSymCSR:
    """A sparse symmetric Hessian on the device, built once on the host from the entries of its LOWER triangle
    (``rows[k] >= cols[k]``: how MadNLP and QuadraticModels hold a Hessian; explicit zeros are kept).  Stored is the FULL
    symmetric pattern in CSR (``ptr, col, val``; n rows, column indices ascending within a row; int64 / float64) plus
    ``row`` (row index of every stored entry): with both triangles one row-wise mat-vec gives ``H x`` in a fixed order
    without atomics, and column j of the lower triangle is row j's entries with ``col >= j`` (``madqp_kkt_set_hcsr``)."""

    def __init__(self, device, n, rows, cols, vals):
        rows, cols = np.asarray(rows, dtype=np.int64).ravel(), np.asarray(cols, dtype=np.int64).ravel()
        vals = np.asarray(vals, dtype=np.float64).ravel()
        n = int(n)
        if not (len(rows) == len(cols) == len(vals)):
            raise ValueError("rows, cols and vals of the sparse Hessian differ in length")
        if len(rows) and (rows.min() < 0 or cols.min() < 0 or rows.max() >= n):
            raise ValueError("index out of range in the sparse Hessian")
        if np.any(cols > rows):
            raise ValueError("entry above the diagonal in the sparse Hessian (pass the lower triangle)")
        order = np.lexsort((cols, rows))
        rows, cols, vals = rows[order], cols[order], vals[order]
        if len(rows) > 1 and np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])):
            raise ValueError("duplicate entries in the sparse Hessian")
        off = rows != cols  # mirrored into the upper triangle
        fr, fc = np.concatenate([rows, cols[off]]), np.concatenate([cols, rows[off]])
        fv = np.concatenate([vals, vals[off]])
        order = np.lexsort((fc, fr))  # by row, then column
        fr, fc, fv = fr[order], fc[order], fv[order]
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=device)
        self.n, self.nnz, self.nnz_lower = n, len(fv), len(vals)  # nnz_lower: the count QuadraticModels reports
        self.ptr = dev(np.concatenate([[0], np.cumsum(np.bincount(fr, minlength=n))]), torch.int64)
        self.col, self.val, self.row = dev(fc, torch.int64), dev(fv, torch.float64), dev(fr, torch.int64)

    @classmethod
    def from_dense(cls, device, H):
        """From a dense symmetric matrix: the non-zeros of ``tril(H)``."""
        L = np.tril(np.asarray(H.detach().cpu().numpy() if torch.is_tensor(H) else H, dtype=np.float64))
        r, c = np.nonzero(L)
        return cls(device, L.shape[0], r, c, L[r, c])

    @classmethod
    def from_coo(cls, device, n, I, J, vals):
        """From a COO pattern as a model reports it (0-based host arrays, any order, duplicates allowed, entries in EITHER
        triangle) and its values: all entries of the pair {i, j} are summed in COO order into both (i, j) and (j, i).  Built
        on ``madqp_csr_map_plan_host`` -- the plan the device map (``madqp_csr_map_create``, kind sym) uploads."""
        vals = np.asarray(vals, dtype=np.float64).ravel()
        if len(vals) != len(np.ravel(I)):
            raise ValueError("vals and the sparsity pattern differ in length")
        n = int(n)
        _, ptr, col, seg, src = csr_plan(I, J, n, n, "sym")
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=device)
        out = object.__new__(cls)
        out.n, out.nnz, out.nnz_lower = n, len(col), int(np.count_nonzero(col <= rows))
        out.ptr, out.col, out.row = dev(ptr, torch.int64), dev(col, torch.int64), dev(rows, torch.int64)
        out.val = dev(_csr_values(vals, seg, src), torch.float64)
        return out

    def to_dense(self):
        H = torch.zeros((self.n, self.n), dtype=torch.float64, device=self.val.device)
        H[self.row, self.col] = self.val
        return H

    def scaled(self, s):
        """A copy that shares the pattern, with every value multiplied by the scalar ``s`` (one IEEE product per entry:
        what ``s * H`` does to a dense H)."""
        out = object.__new__(DeviceSymCSR)
        out.__dict__.update(self.__dict__)
        out.val = (self.val * float(s)).contiguous()
        return out

    def matvec(self, x):
        """``H x`` for the one-off host-side uses (scaling, fixed variables, post-solve): every row summed left to right,
        one row after the other -- a fixed order, no atomics."""
        if self.nnz == 0:
            return torch.zeros(self.n, dtype=torch.float64, device=self.val.device)
        return torch.segment_reduce(self.val * x[self.col], "sum", offsets=self.ptr, initial=0.0)

    def submatrix(self, free):
        """``H[free][:, free]`` as a new container; ``free``: ascending index tensor (or array)."""
        free = np.asarray(free.cpu().numpy() if torch.is_tensor(free) else free, dtype=np.int64)
        new = np.full(self.n, -1, dtype=np.int64)
        new[free] = np.arange(len(free))
        r, c, v = (t.cpu().numpy() for t in (self.row, self.col, self.val))
        keep = (c <= r) & (new[r] >= 0) & (new[c] >= 0)  # the lower triangle, both indices kept
        return DeviceSymCSR(self.val.device, len(free), new[r[keep]], new[c[keep]], v[keep])


class DeviceQP:
    def __init__(self, H, q, A, lvar, uvar, lcon, ucon, x0, c0=0.0, y0=None, name="qp"):
        """``A``: (m, nx) row-major tensor, or a :class:`DeviceCSR` (sparse front end); ``H``: (nx, nx) tensor, None,
        a 1-D tensor (diagonal) or a :class:`DeviceSymCSR`."""
        self.H, self.q, self.A = H, q, A
        self.lvar, self.uvar, self.lcon, self.ucon, self.x0 = lvar, uvar, lcon, ucon, x0
        self.c0 = float(c0)
        self.y0 = torch.zeros_like(lcon) if y0 is None else y0
        self.name = name
        self.nvar, self.ncon = q.numel(), lcon.numel()

    @classmethod
    def from_numpy(cls, device, H, q, A, lvar, uvar, lcon, ucon, x0, c0=0.0, y0=None, name="qp", sparse=False):
        f = lambda a: None if a is None else torch.as_tensor(
            np.ascontiguousarray(a, dtype=np.float64), device=device)
        n = len(q)
        Hn = None if (H is None or not np.any(H)) else f(H)
        A2 = np.asarray(A, dtype=np.float64).reshape(len(lcon), n)
        An = DeviceCSR.from_dense(device, A2) if sparse else f(A2)
        return cls(Hn, f(q), An, f(lvar), f(uvar), f(lcon), f(ucon), f(x0), c0, f(y0), name)

    def eliminate_fixed(self):
        """``MadNLP.MakeParameter`` (the fixed-variable treatment src/utils.jl:81 selects for every KKT system that
        is not condensed): variables with ``lvar == uvar`` leave the problem as parameters.  Returns None when there
        are none, else ``(reduced DeviceQP, free, fixed, xfix, shift)`` with index tensors ``free`` / ``fixed``, the
        fixed values and ``shift = A[:, fixed] xfix`` (the rows of the reduced model are ``A_f x_f`` in
        ``[lcon - shift, ucon - shift]``).  All on the device."""
        mask = self.lvar == self.uvar
        if not bool(mask.any()):
            return None
        fixed, free = torch.nonzero(mask).flatten(), torch.nonzero(~mask).flatten()
        xf = self.lvar[fixed]
        c0 = self.c0 + float(self.q[fixed] @ xf)
        q = self.q[free].clone()
        H = self.H
        if isinstance(H, DeviceSymCSR):
            xfull = torch.zeros(self.nvar, dtype=torch.float64, device=self.q.device)
            xfull[fixed] = xf
            Hx = H.matvec(xfull)  # H[:, fixed] xfix
            c0 += 0.5 * float(Hx[fixed] @ xf)
            q += Hx[free]
            H = H.submatrix(free)
        elif H is not None and H.dim() == 1:
            c0 += 0.5 * float((H[fixed] * xf) @ xf)
            H = H[free].contiguous()
        elif H is not None:
            Hx = H.index_select(1, fixed) @ xf  # H[:, fixed] xfix
            c0 += 0.5 * float(Hx[fixed] @ xf)
            q += Hx[free]
            H = H.index_select(0, free).index_select(1, free).contiguous()
        if isinstance(self.A, DeviceCSR):
            a = self.A
            isfix = mask[a.col]
            shift = torch.zeros(self.ncon, dtype=torch.float64, device=self.q.device)
            shift.index_add_(0, a.row[isfix], a.val[isfix] * self.lvar[a.col[isfix]])
            newcol = torch.cumsum((~mask).to(torch.int64), 0) - 1
            keep = ~isfix
            A = DeviceCSR(self.q.device, self.ncon, free.numel(), a.row[keep].cpu().numpy(),
                          newcol[a.col[keep]].cpu().numpy(), a.val[keep].cpu().numpy())
        else:
            shift = self.A.index_select(1, fixed) @ xf
            A = self.A.index_select(1, free).contiguous()
        red = DeviceQP(H, q, A, self.lvar[free].clone(), self.uvar[free].clone(), self.lcon - shift, self.ucon - shift,
                       self.x0[free].clone(), c0, self.y0, self.name + "-free")
        return red, free, fixed, xf, shift

    @classmethod
    def synthetic(cls, backend, seed: int, n: int, m: int, family: str = "wigner"):
        """0 <= x <= 1, 0 <= Ax <= 1, x0 = 0; A ~ N(0,1); H by family: "wigner" (Wigner + 3 I, O(n^2) to
        generate: the large configs), "dummy" (H = G'G + 100 I with G n x n N(0,1) from the H stream -- R R' + 100 I of
        MadNLPTests.DenseDummyQP, test/runtests.jl:9, with R = G': n_x <= ~10 000, one call of the library's own SYRK),
        "lp" (no Hessian)."""
        dev = backend.device
        A = torch.empty((m, n), dtype=torch.float64, device=dev)
        backend.gen_normal(stream_key(seed, STREAM_A), 0, A)
        q = torch.empty(n, dtype=torch.float64, device=dev)
        backend.gen_normal(stream_key(seed, STREAM_Q), 0, q)
        H = None
        if family == "wigner":
            H = torch.empty((n, n), dtype=torch.float64, device=dev)
            backend.gen_wigner(stream_key(seed, STREAM_H), n, 1.0 / math.sqrt(n), H)
        elif family == "dummy":
            G = torch.empty((n, n), dtype=torch.float64, device=dev)
            backend.gen_normal(stream_key(seed, STREAM_H), 0, G)
            H = torch.zeros((n, n), dtype=torch.float64, device=dev)
            d = torch.full((n,), 100.0, dtype=torch.float64, device=dev)
            # lower triangle of G'G + 100 I (column-major lower = row-major upper of the same symmetric matrix)
            backend.syrk_assemble(n, n, G, n, None, None, n, d, H, n)
            H = torch.triu(H) + torch.triu(H, 1).T
            del G
        elif family != "lp":
            raise ValueError(family)
        z = lambda k, v: torch.full((k,), v, dtype=torch.float64, device=dev)
        return cls(H, q, A, z(n, 0.0), z(n, 1.0), z(m, 0.0), z(m, 1.0), z(n, 0.0),
                   name=f"synthetic-{family}-n{n}-m{m}-s{seed}")
