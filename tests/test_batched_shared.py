"""CPU: ``BatchedMPCSolver(..., shared_matrices=True)`` -- one H and one A for every problem of a batch
(madqp_batch_share_matrices) -- as far as it goes without a device: the constructor's rules, the host set-up against the
stacked form's (bitwise: the library then sees the same numbers, H apart, which it scales itself), the C entry's NULL
handle.  The engine itself is in tests/test_gpu_batched_shared.py, which takes its batches from the builders below."""
import copy
import types

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
from oracle import qp as Q

REG = M.FixedRegularization(1e-8, -1e-8)
MADQP_ERR_ARG = -1


def base_problem(n, m, seed, lp=False):
    """One model.  Every third row of A is 150 x larger (con_scale < 1 there: the one scaling of a shared A is not the
    identity)."""
    qp = Q.synthetic_qp(seed, n, m, "lp" if lp else "wigner")
    if m:
        qp.A[::3] *= 150.0
        qp.ucon[::3] *= 150.0
    return qp


def family(base, B, seed, pattern=None):
    """B problems of one model: q, the variable bounds and the row bounds are each problem's own (seeded).  |q| spans 1.5
    decades, so obj_scale = min(1, 100 / max|q + H x0|) -- the factor of a shared H -- differs from problem to problem
    and is no power of two.  ``pattern(qp, rng)``: gives problems 1.. a finiteness pattern of their own."""
    rng = np.random.default_rng(seed)
    n, m = base.nvar, base.ncon
    out = []
    for b in range(B):
        qp = copy.deepcopy(base)
        qp.q = base.q * 10.0 ** rng.uniform(1.5, 3.0) + 0.05 * rng.standard_normal(n)
        qp.lvar = base.lvar - 0.1 * rng.random(n)
        qp.uvar = base.uvar + 0.1 * rng.random(n)
        qp.lcon = base.lcon - 0.1 * rng.random(m) * np.maximum(1.0, base.ucon)
        qp.ucon = base.ucon + 0.1 * rng.random(m) * np.maximum(1.0, base.ucon)
        if pattern is not None and b > 0:
            qp = pattern(qp, rng)
        out.append(qp)
    return out


def to_device(qp, device):
    return M.DeviceQP.from_numpy(device, qp.H, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0)


def stacked_and_shared(qps, device):
    """The same problems twice: every problem with clones of H and A, and every problem holding ONE H and ONE A."""
    stacked = [to_device(q, device) for q in qps]
    shared = [to_device(q, device) for q in qps]
    for d in shared:
        d.H, d.A = shared[0].H, shared[0].A
    return stacked, shared


class _Stop(Exception):
    pass


def host_setup(dqs, **kw):
    """initialize() on CPU tensors up to the point where the library would be called."""
    kw.setdefault("regularization", REG)
    s = M.BatchedMPCSolver(dqs, types.SimpleNamespace(device=torch.device("cpu")), **kw)

    def stop(_):
        raise _Stop

    s.pre_create_hook = stop
    with pytest.raises(_Stop):
        s.initialize()
    return s


def test_different_storage_is_refused_and_names_the_problem():
    cpu = torch.device("cpu")
    qps = family(base_problem(12, 5, 3), 4, 1)
    _, shared = stacked_and_shared(qps, cpu)
    shared[2].H = shared[0].H.clone()
    with pytest.raises(ValueError, match=r"problem 2 has a H of its own"):
        M.BatchedMPCSolver(shared, types.SimpleNamespace(device=cpu), shared_matrices=True, regularization=REG)
    _, shared = stacked_and_shared(qps, cpu)
    shared[3].A = shared[0].A.clone()
    with pytest.raises(ValueError, match=r"problem 3 has a A of its own"):
        M.BatchedMPCSolver(shared, types.SimpleNamespace(device=cpu), shared_matrices=True, regularization=REG)
    _, shared = stacked_and_shared(qps, cpu)
    shared[1].A = shared[0].A.t().contiguous().t()  # same shape, other strides (and other storage)
    with pytest.raises(ValueError, match=r"problem 1 has a A of its own"):
        M.BatchedMPCSolver(shared, types.SimpleNamespace(device=cpu), shared_matrices=True, regularization=REG)
    # the stacked form does not care
    stacked, _ = stacked_and_shared(qps, cpu)
    assert M.BatchedMPCSolver(stacked, types.SimpleNamespace(device=cpu), regularization=REG).H.shape == (4, 12, 12)


def test_shared_solver_holds_one_matrix_each():
    cpu = torch.device("cpu")
    qps = family(base_problem(12, 5, 3), 4, 1)
    _, shared = stacked_and_shared(qps, cpu)
    s = M.BatchedMPCSolver(shared, types.SimpleNamespace(device=cpu), shared_matrices=True, regularization=REG)
    assert s.H.shape == (1, 12, 12) and s.A.shape == (1, 5, 12)
    assert s.H.data_ptr() == shared[0].H.data_ptr() and s.A.data_ptr() == shared[0].A.data_ptr()
    s = host_setup(shared, shared_matrices=True)
    assert s._H.shape == (1, 12, 12) and s._A.shape == (1, 5, 12)
    assert s._H.data_ptr() == shared[0].H.data_ptr()  # H goes to the library as the caller holds it
    big = 4 * 5 * 12
    assert not any(torch.is_tensor(v) and v.numel() >= big for v in vars(s).values())


def test_lps_with_a_shared_A_are_accepted():
    cpu = torch.device("cpu")
    qps = family(base_problem(10, 4, 5, lp=True), 3, 2)
    _, shared = stacked_and_shared(qps, cpu)
    assert all(d.H is None for d in shared)
    s = host_setup(shared, shared_matrices=True)
    assert s.H is None and s._H is None and s.h_scale is None and s.A.shape == (1, 4, 10)
    s = host_setup(shared, shared_matrices=True, kkt_system="normal", regularization=M.FixedRegularization(1e-8, 0.0))
    assert s._A.shape == (1, 4, 10)


@pytest.mark.parametrize("case", ["qp", "lp", "patterns", "unscaled", "no_rows"])
def test_host_setup_is_bitwise_the_stacked_forms(case):
    cpu = torch.device("cpu")
    kw = {}
    n, m = (14, 0) if case == "no_rows" else (14, 6)
    pattern = None
    if case == "patterns":
        kw["per_problem_patterns"] = True

        def pattern(qp, rng):
            qp.uvar[rng.random(n) < 0.4] = np.inf
            qp.ucon[rng.random(m) < 0.4] = np.inf
            return qp
    if case == "unscaled":
        kw["scaling"] = False
    qps = family(base_problem(n, m, 7, lp=case == "lp"), 5, 4, pattern)
    stacked, shared = stacked_and_shared(qps, cpu)
    a, b = host_setup(stacked, **kw), host_setup(shared, shared_matrices=True, **kw)
    for name in ("obj_scale", "con_scale", "x", "xl", "xu", "y", "_q", "_rhs", "_c0"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert ta.shape == tb.shape and np.array_equal(ta.numpy(), tb.numpy(), equal_nan=True), name
    if case in ("qp", "patterns"):
        assert len(set(a.obj_scale.tolist())) >= 3 and float(a.obj_scale.min()) < 1.0  # the factor of H is not trivial
    if case != "unscaled" and m:
        assert float(a.con_scale.min()) < 1.0
    if case == "lp" or case == "unscaled":
        assert b.h_scale is None
    else:
        assert b.h_scale.data_ptr() == b.obj_scale.data_ptr() or torch.equal(b.h_scale, b.obj_scale)
        assert b.h_scale.is_contiguous() and b.h_scale.shape == (5,)
        # what the library forms on load is what the stacked form stores
        assert torch.equal(a._H, b.h_scale[:, None, None] * b._H)
    # one scaled A, and it is the stacked form's A of every problem
    assert b._A.shape[0] == 1 and all(torch.equal(a._A[k], b._A[0]) for k in range(5))


def test_share_matrices_without_a_handle_is_an_error_code():
    lib = M.load_cdll()
    assert lib.madqp_batch_share_matrices(None, 1, 1, None) == MADQP_ERR_ARG
    assert lib.madqp_batch_share_matrices(None, 0, 0, None) == MADQP_ERR_ARG
