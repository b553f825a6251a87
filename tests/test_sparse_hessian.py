"""CPU (torch on the CPU device, no library call): the sparse-Hessian container ``DeviceSymCSR`` and the host-side code that
learns it as the third shape of H -- ``DeviceQP.eliminate_fixed``, ``preprocess.to_device(sparse_hessian=True)`` and the
refusals of ``MPCSolver.__init__``.  The kernels behind it are held in tests/test_gpu_sparse_hessian.py."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import madqp_jl_amd as M
from madqp_jl_amd import preprocess as P
from sparse_hessian import PATTERNS, pattern, sparse_hessian, sparse_hessian_qp

CPU = torch.device("cpu")
U = 2.0 ** -53


def dense_of(n, r, c, v):
    H = np.zeros((n, n))
    H[r, c] = v
    H[c, r] = v
    return H


def container_cases():
    rng = np.random.default_rng(2)
    L = np.tril(rng.standard_normal((23, 23)) * (rng.random((23, 23)) < 0.25))
    yield "random", 23, *np.nonzero(L), L[np.nonzero(L)]
    L2 = L.copy()
    L2[7, :] = 0.0
    L2[:, 7] = 0.0  # row 7 of the symmetric pattern is empty
    yield "empty_row", 23, *np.nonzero(L2), L2[np.nonzero(L2)]
    L3 = np.tril(L, -1)
    yield "no_diagonal", 23, *np.nonzero(L3), L3[np.nonzero(L3)]
    z = np.zeros(0, dtype=np.int64)
    yield "nnz0", 9, z, z, np.zeros(0)
    yield "n1", 1, np.array([0]), np.array([0]), np.array([2.5])
    yield "n1_nnz0", 1, z, z, np.zeros(0)


@pytest.mark.parametrize("case", list(container_cases()), ids=lambda c: c[0])
def test_container_from_lower_triangle(case):
    _, n, r, c, v = case
    h = M.DeviceSymCSR(CPU, n, r, c, v)
    D = h.to_dense().numpy()
    want = dense_of(n, r, c, v)
    assert np.array_equal(D, D.T) and np.array_equal(D, want)
    ptr, col, row, val = (t.numpy() for t in (h.ptr, h.col, h.row, h.val))
    assert h.ptr.dtype == h.col.dtype == h.row.dtype == torch.int64 and h.val.dtype == torch.float64
    assert ptr.shape == (n + 1,) and ptr[0] == 0 and ptr[-1] == h.nnz == len(col) == len(val) == len(row)
    assert h.nnz_lower == len(v) and h.nnz == 2 * len(v) - int(np.sum(r == c)) and h.n == n
    for i in range(n):
        seg = col[ptr[i]:ptr[i + 1]]
        assert np.all(np.diff(seg) > 0), "columns ascend within a row"
        assert np.all(row[ptr[i]:ptr[i + 1]] == i)
    # shuffled input: the same container
    perm = np.random.default_rng(0).permutation(len(v))
    h2 = M.DeviceSymCSR(CPU, n, r[perm], c[perm], v[perm])
    assert all(torch.equal(getattr(h, k), getattr(h2, k)) for k in ("ptr", "col", "row", "val"))
    assert np.array_equal(M.DeviceSymCSR.from_dense(CPU, want).to_dense().numpy(), want)


def test_container_keeps_explicit_zeros_and_refuses_bad_input():
    h = M.DeviceSymCSR(CPU, 3, [1, 2, 2], [0, 0, 2], [0.0, 1.5, 0.0])
    assert h.nnz_lower == 3 and h.nnz == 5 and np.array_equal(h.to_dense().numpy(), dense_of(3, [2], [0], [1.5]))
    with pytest.raises(ValueError, match="above the diagonal"):
        M.DeviceSymCSR(CPU, 3, [0, 1], [0, 2], [1.0, 2.0])
    with pytest.raises(ValueError, match="duplicate"):
        M.DeviceSymCSR(CPU, 3, [2, 1, 2], [1, 0, 1], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="out of range"):
        M.DeviceSymCSR(CPU, 3, [3], [0], [1.0])
    # from_dense reads tril only
    A = np.arange(9.0).reshape(3, 3)
    assert np.array_equal(M.DeviceSymCSR.from_dense(CPU, A).to_dense().numpy(), np.tril(A) + np.tril(A, -1).T)


def test_scaled_is_one_product_per_entry():
    H = sparse_hessian(4, 40, 3)
    h = M.DeviceSymCSR.from_dense(CPU, H)
    s = h.scaled(0.37)
    assert s.ptr is h.ptr and s.col is h.col and s.row is h.row  # the pattern is shared
    assert np.array_equal(s.to_dense().numpy().view(np.uint64), (0.37 * torch.as_tensor(H)).numpy().view(np.uint64))
    assert np.array_equal(h.to_dense().numpy(), H)  # (the original is untouched)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", [1, 40, 300])
def test_matvec_against_extended_precision(name, n):
    """(len + 4) u S against numpy.longdouble: len = the row's stored entries, S = |H| |x|."""
    r, c, v = pattern(name, n)
    h = M.DeviceSymCSR(CPU, n, r, c, v)
    x = np.random.default_rng(n).standard_normal(n)
    y = h.matvec(torch.as_tensor(x)).numpy()
    D = dense_of(n, r, c, v).astype(np.longdouble)
    ref = D @ x.astype(np.longdouble)
    S = np.abs(D) @ np.abs(x).astype(np.longdouble)
    length = np.diff(h.ptr.numpy())
    assert y.shape == (n,) and np.all(np.abs(y.astype(np.longdouble) - ref) <= (length + 4) * U * S)


def test_submatrix():
    H = sparse_hessian(8, 31, 3)
    h = M.DeviceSymCSR.from_dense(CPU, H)
    free = torch.as_tensor([0, 1, 4, 5, 6, 11, 12, 20, 29, 30])
    sub = h.submatrix(free)
    f = free.numpy()
    assert isinstance(sub, M.DeviceSymCSR) and sub.n == len(f)
    assert np.array_equal(sub.to_dense().numpy(), H[f][:, f])
    assert h.submatrix(torch.arange(31)).nnz == h.nnz and h.submatrix(torch.as_tensor([], dtype=torch.int64)).nnz == 0


@pytest.mark.parametrize("sparse_A", [True, False])
def test_eliminate_fixed_matches_the_dense_branch(sparse_A):
    qp = sparse_hessian_qp(11, 129, 40, 4, 1, equality_cons=(1,))
    fixed, vals = [5, 64, 128], [0.3, 0.0, 0.9]
    qp.lvar[fixed] = qp.uvar[fixed] = vals
    out = []
    for as_csr in (True, False):
        dq = M.DeviceQP.from_numpy(CPU, None, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, 0.75, sparse=sparse_A)
        dq.H = M.DeviceSymCSR.from_dense(CPU, qp.H) if as_csr else torch.as_tensor(qp.H)
        red, free, fx, xf, shift = dq.eliminate_fixed()
        assert fx.tolist() == fixed and red.nvar == 126
        out.append(red)
    s, d = out
    assert isinstance(s.H, M.DeviceSymCSR) and np.array_equal(s.H.to_dense().numpy(), d.H.numpy())
    assert np.max(np.abs(s.q.numpy() - d.q.numpy())) <= 1e-14 * np.max(np.abs(d.q.numpy()))
    assert abs(s.c0 - d.c0) <= 1e-14 * abs(d.c0) and d.c0 != 0.75
    assert torch.equal(s.lcon, d.lcon) and torch.equal(s.ucon, d.ucon)


def host_qp(H):
    n = H.shape[0]
    A = sp.csr_matrix(np.array([[1.0 if j % 2 == 0 else 0.0 for j in range(n)]]))
    return P.HostQP(0.5, np.arange(n, dtype=float), sp.csr_matrix(H), A, np.zeros(n), np.ones(n), np.zeros(1), np.ones(1))


def test_to_device_keeps_a_sparse_hessian_sparse_on_request():
    stub = types.SimpleNamespace(device="cpu")
    H = sparse_hessian(2, 12, 2)
    q = host_qp(H)
    d = P.to_device(q, stub)  # default keywords: what every existing caller gets
    assert torch.is_tensor(d.H) and d.H.dim() == 2 and np.array_equal(d.H.numpy(), H)
    s = P.to_device(q, stub, sparse_hessian=True)
    assert isinstance(s.H, M.DeviceSymCSR) and np.array_equal(s.H.to_dense().numpy(), q.H.toarray())
    assert s.H.nnz_lower == q.nnzh and isinstance(s.A, M.DeviceCSR)
    # sparse_hessian without the sparse front end: dense, as before
    assert torch.is_tensor(P.to_device(q, stub, sparse=False, sparse_hessian=True).H)
    for kw in ({}, {"sparse_hessian": True}):
        dg = P.to_device(host_qp(np.diag(np.arange(1.0, 13.0))), stub, **kw)
        assert torch.is_tensor(dg.H) and dg.H.dim() == 1 and np.array_equal(dg.H.numpy(), np.arange(1.0, 13.0))
        assert P.to_device(host_qp(np.zeros((12, 12))), stub, **kw).H is None


def test_boundary_control_smoothing_variant():
    base, again, sm = P.boundary_control_qp(6), P.boundary_control_qp(6, smooth=0.0), P.boundary_control_qp(6, smooth=0.5)
    assert (base.H != again.H).nnz == 0 and np.array_equal(base.H.indices, again.H.indices)  # output unchanged without it
    Hd, Hs = base.H.toarray(), sm.H.toarray()
    assert np.array_equal(np.diag(np.diag(Hd)), Hd) and np.array_equal(Hs, Hs.T)
    N, h = 6, 1.0 / 7
    assert np.array_equal(Hs[:N * N, :], Hd[:N * N, :])  # the states are untouched
    u = np.random.default_rng(0).standard_normal(4 * N)
    want = 0.5 * h * sum(np.sum(np.diff(u[k * N:(k + 1) * N]) ** 2) for k in range(4))
    got = u @ (Hs - Hd)[N * N:, N * N:] @ u
    assert abs(got - want) <= 1e-12 * want
    for f in ("c", "lvar", "uvar", "lcon", "ucon"):
        assert np.array_equal(getattr(base, f), getattr(sm, f))
    assert (base.A != sm.A).nnz == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(dense_A=True), "needs the sparse front end"),
    (dict(kkt_system="normal"), "supports only linear programs"),
    (dict(kkt_system="scaled_augmented"), "scaled augmented"),
    (dict(grid=True), "DistributedQP"),
])
def test_solver_refuses_what_a_sparse_hessian_cannot_do(kw, msg):
    """ValueError in the style of the existing refusals, before anything touches a device (never an AttributeError)."""
    kw = dict(kw)
    qp = sparse_hessian_qp(3, 12, 5, 2, 2)
    dq = M.DeviceQP.from_numpy(CPU, None, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, sparse=not kw.pop("dense_A", False))
    dq.H = M.DeviceSymCSR.from_dense(CPU, qp.H)
    if kw.pop("grid", False):
        dq.grid = object()
    with pytest.raises(ValueError, match=msg):
        M.MPCSolver(dq, types.SimpleNamespace(device="cpu"), **kw)


def test_batched_driver_keeps_its_refusal():
    qp = sparse_hessian_qp(3, 12, 5, 2, 2)
    dq = M.DeviceQP.from_numpy(CPU, None, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0)
    dq.H = M.DeviceSymCSR.from_dense(CPU, qp.H)
    with pytest.raises(ValueError, match="the batched driver takes dense H and dense A"):
        M.BatchedMPCSolver([dq], types.SimpleNamespace(device=CPU))


def test_sparse_normal_kkt_system_refuses_with_its_lp_only_message():
    h = M.DeviceSymCSR.from_dense(CPU, sparse_hessian(1, 4, 1))
    with pytest.raises(ValueError, match="supports only linear programs"):
        M.HIPSparseNormalKKTSystem(None, None, 4, [], h, None)
