"""GPU: per-problem bound and inequality patterns in the lock-step batched engine (``per_problem_patterns=True``,
madqp_batch_create_patterns).  A batch whose problems have different finite bounds and equality rows agrees with the
CPU oracle problem by problem; every problem of such a batch gives bitwise what a batch of copies of itself gives;
the order of the problems does not matter; the padded tail of the slack part is neither read nor written; a uniform
batch through the new path is bitwise the default path; malformed lists are refused with a return code."""
import ctypes as C

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
from madqp_jl_amd._lib import CBatchData, ptr
from madqp_jl_amd.options import IPMOptions
from madqp_jl_amd.solver import native_options
from oracle import mpc
from oracle import qp as Q

from test_gpu_batched import OREG, REG, _edge_batch, check_against_oracle, close, to_device

pytestmark = pytest.mark.gpu
EDGE_CASES = ["lower_bounds_only", "upper_bounds_only", "mixed", "no_bounds", "default"]


def edge_mix(B_per_case=2, cases=EDGE_CASES):
    """The patterns test_gpu_batched.py runs one per batch, side by side in ONE batch (same base problems)."""
    per = [_edge_batch(c, B_per_case) for c in cases]
    return [per[c][i] for i in range(B_per_case) for c in range(len(cases))]


def random_pattern(qp, rng, lp=False):
    """A pattern of its own: some variables free, lower-only or upper-only, some rows equalities or one-sided.
    LPs keep every variable bounded below and some rows two-sided (a bounded feasible set)."""
    nx, m = len(qp.lvar), len(qp.lcon)
    v = rng.random(nx)
    if lp:
        qp.uvar[v < 0.4] = np.inf
    else:
        qp.lvar[v < 0.15], qp.uvar[v < 0.15] = -np.inf, np.inf
        qp.uvar[(v >= 0.15) & (v < 0.35)] = np.inf
        qp.lvar[(v >= 0.35) & (v < 0.55)] = -np.inf
    r = rng.random(m)
    qp.lcon[r < 0.15] = qp.ucon[r < 0.15] = 0.1
    qp.ucon[(r >= 0.15) & (r < 0.35)] = np.inf
    qp.lcon[(r >= 0.35) & (r < 0.5)] = -np.inf
    return qp


def solve(hip, qps, **kw):
    s = M.BatchedMPCSolver([to_device(q, hip) for q in qps], hip, **kw)
    res = s.solve()
    s.close()
    return res, s.scalars.copy()


def assert_bitwise(r, ref, what):
    assert r["status"] == ref["status"] and r["iter"] == ref["iter"], (what, r["status"], ref["status"], r["iter"], ref["iter"])
    for k in ("solution", "multipliers", "multipliers_L", "multipliers_U"):
        assert np.array_equal(r[k], ref[k]), (what, k)
    assert r["objective"] == ref["objective"] or (r["objective"] != r["objective"] and ref["objective"] != ref["objective"])


def test_mixed_batch_vs_oracle(hip):
    qps = edge_mix()
    res, _ = solve(hip, qps, per_problem_patterns=True, regularization=REG)
    assert len({len(q.lcon) - int(np.sum(q.lcon == q.ucon)) for q in qps}) > 1  # ns_b differs within the batch
    check_against_oracle(qps, res)


def test_mixed_batch_vs_oracle_configs3_shape(hip):
    rng = np.random.default_rng(7)
    qps = [Q.synthetic_qp(20250614 + 3 + i, 512, 256) for i in range(4)]
    qps = [qps[0]] + [random_pattern(q, rng) for q in qps[1:]]
    res, _ = solve(hip, qps, per_problem_patterns=True, regularization=REG)
    check_against_oracle(qps, res)


def test_mixed_equals_batch_of_copies(hip):
    """Problem b inside a mixed batch gives bitwise what a batch of B copies of b gives (default path, same B: the
    same workgroup width): the strides and the other problems' patterns do not enter its arithmetic."""
    qps = edge_mix(1) + [random_pattern(Q.synthetic_qp(31, 40, 15), np.random.default_rng(3))]
    B = len(qps)
    res, scal = solve(hip, qps, per_problem_patterns=True, regularization=REG)
    for b, qp in enumerate(qps):
        one, sc1 = solve(hip, [qp] * B, regularization=REG)
        for k in range(B):
            assert_bitwise(res[b], one[k], (b, k))
            assert np.array_equal(scal[b], sc1[k]), (b, k)


def test_mixed_batch_order_does_not_matter(hip):
    qps = edge_mix()
    res, scal = solve(hip, qps, per_problem_patterns=True, regularization=REG)
    perm = np.random.default_rng(11).permutation(len(qps))
    res2, scal2 = solve(hip, [qps[i] for i in perm], per_problem_patterns=True, regularization=REG)
    for k, i in enumerate(perm):
        assert_bitwise(res2[k], res[i], (k, i))
        assert np.array_equal(scal2[k], scal[i])


def test_padding_is_never_touched(hip):
    qps = edge_mix()
    s = M.BatchedMPCSolver([to_device(q, hip) for q in qps], hip, per_problem_patterns=True, regularization=REG)
    nb = s.nx + s.pat["ns"]
    assert s.n > nb.min()  # there is a tail
    tail = torch.as_tensor(np.arange(s.n)[None, :] >= nb[:, None], device=hip.device)
    nan_bits = 0x7FF8DEADBEEF0123
    names = ("x", "xl", "xu", "zl", "zu")

    def poison(solver):
        for k in names:
            getattr(solver, k).view(torch.int64)[tail] = nan_bits

    s.pre_create_hook = poison
    res = s.solve()
    for k in names:
        bits = getattr(s, k).view(torch.int64)[tail]
        assert bool((bits == nan_bits).all()), k  # nothing wrote the tails
    s.close()
    for r in res:  # nothing read them
        assert r["status"] == M.SOLVE_SUCCEEDED
        for k in ("solution", "multipliers", "multipliers_L", "multipliers_U"):
            assert np.all(np.isfinite(r[k])), k
        assert np.isfinite(r["objective"])
    assert np.all(np.isfinite(s.scalars))
    check_against_oracle(qps, res)


def test_mixed_normal_equations(hip):
    rng = np.random.default_rng(6)
    qps = [Q.synthetic_qp(2100 + i, 40, 16, "lp") for i in range(6)]
    qps = [qps[0]] + [random_pattern(q, rng, lp=True) for q in qps[1:]]
    reg, oreg = M.FixedRegularization(1e-8, 0.0), mpc.FixedRegularization(1e-8, 0.0)
    res, _ = solve(hip, qps, per_problem_patterns=True, kkt_system="normal", regularization=reg)
    for i, (qp, r) in enumerate(zip(qps, res)):
        ref = mpc.solve(qp, kkt_system="normal", regularization=oreg)
        assert r["status"] == ref["status"] == M.SOLVE_SUCCEEDED, (i, r["status"], ref["status"])
        assert r["iter"] == ref["iter"], (i, r["iter"], ref["iter"])
        assert close(r["objective"], ref["objective"], 1e-9)
        assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-7
        assert np.max(np.abs(r["multipliers"] - ref["multipliers"])) <= 1e-6


def test_mixed_gondzio(hip):
    qps = edge_mix(cases=[c for c in EDGE_CASES if c != "no_bounds"])  # (no bound: mu = 0, the oracle's 0 / 0 raises)
    res, _ = solve(hip, qps, per_problem_patterns=True, regularization=REG, max_ncorr=3)
    for i, (qp, r) in enumerate(zip(qps, res)):
        ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG, max_ncorr=3)
        assert r["status"] == ref["status"] == M.SOLVE_SUCCEEDED and r["iter"] == ref["iter"], (i, r["iter"], ref["iter"])
        assert r["n_factorizations"] == ref["n_factorizations"], i
        assert close(r["objective"], ref["objective"], 1e-9), i
        assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-7, i
        assert np.max(np.abs(r["multipliers"] - ref["multipliers"])) <= 1e-6, i


@pytest.mark.parametrize("max_ncorr", [0, 3])
def test_retry_with_a_variable_free_in_one_problem(hip, max_ncorr):
    """The x100 retry of src/linear_solver.jl:6-17 where only the failing problem has the free variable (the batch that
    test_batched_regularization_retry could not build with one pattern): n_factorizations follows the oracle's."""
    qps, free, bad = [], 3, 2
    for i in range(5):
        qp = Q.synthetic_qp(40 + i, 20, 8)
        qp.H = np.diag(np.diag(qp.H))
        if i == bad:
            qp.lvar[free], qp.uvar[free] = -np.inf, np.inf
            qp.A[:, free] = 0.0
            qp.q[free] = 0.0
            qp.H[free, free] = -1e-7
        qps.append(qp)
    res, _ = solve(hip, qps, per_problem_patterns=True, regularization=REG, max_iter=4, max_ncorr=max_ncorr)
    for i, (qp, r) in enumerate(zip(qps, res)):
        ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG, max_iter=4, max_ncorr=max_ncorr)
        assert r["status"] == ref["status"] and r["iter"] == ref["iter"], (i, r["status"], ref["status"], r["iter"], ref["iter"])
        assert r["n_factorizations"] == ref["n_factorizations"], (i, r["n_factorizations"], ref["n_factorizations"])
        t = ref["trace"][-1]
        assert close(r["inf_pr"], t["inf_pr"], 1e-6) and close(r["inf_du"], t["inf_du"], 1e-6), i
        assert close(r["del_w"], t["del_w"], 1e-12), i
        assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-6, i
    assert res[bad]["n_factorizations"] > res[0]["n_factorizations"]


@pytest.mark.parametrize("case,kw", [("mixed", {}), ("default", dict(max_ncorr=2)), ("lp", dict(kkt_system="normal"))])
def test_uniform_batch_through_the_new_path_is_bitwise_the_default(hip, case, kw):
    if case == "lp":
        qps = [Q.synthetic_qp(2100 + i, 40, 16, "lp") for i in range(5)]
        kw = dict(kw, regularization=M.FixedRegularization(1e-8, 0.0))
    else:
        qps = _edge_batch(case, 5)
        kw = dict(kw, regularization=REG)
    res, scal = solve(hip, qps, **kw)
    res2, scal2 = solve(hip, qps, per_problem_patterns=True, **kw)
    for b in range(len(qps)):
        assert_bitwise(res2[b], res[b], b)
    assert np.array_equal(scal, scal2)


def test_malformed_lists_are_refused(hip):
    B, nx, m = 2, 3, 2
    f64 = dict(dtype=torch.float64, device=hip.device)
    keep = [torch.zeros(B * nx * max(nx, m) + 16, **f64) for _ in range(11)]
    data = CBatchData(**{k: ptr(t) for k, t in zip(("H", "A", "q", "rhs", "c0", "x", "xl", "xu", "zl", "zu", "y"), keep)})
    opt = native_options(IPMOptions(regularization=REG))
    lib = hip.lib

    def create(ineq_ptr, ineq, lb_ptr, lb, ub_ptr, ub):
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (ineq_ptr, ineq, lb_ptr, lb, ub_ptr, ub)]
        ps = [a.ctypes.data_as(C.POINTER(C.c_int64)) if a.size else None for a in arrs]
        h = C.c_void_p()
        r = lib.madqp_batch_create_patterns(hip.ctx, B, nx, m, *ps, C.byref(data), C.byref(opt), C.byref(h))
        if r == 0:
            lib.madqp_batch_destroy(h)
        return r, lib.madqp_last_error(hip.ctx)

    ok = ([0, 2, 3], [0, 1, 1], [0, 2, 5], [0, 4, 0, 1, 3], [0, 1, 1], [2])
    assert create(*ok)[0] == 0
    bad = {
        "ptr does not start at 0": ([1, 2, 3], [0, 1, 1], *ok[2:]),
        "ptr decreases": ok[:2] + ([0, 3, 2], [0, 4, 0, 1, 3]) + ok[4:],
        "ns_b > m": ([0, 3, 3], [0, 1, 1], *ok[2:]),
        "ind_ineq not increasing": ([0, 2, 3], [1, 0, 1], *ok[2:]),
        "ind_ineq out of range": ([0, 2, 3], [0, 2, 1], *ok[2:]),
        "ind_lb repeated": ok[:2] + ([0, 2, 5], [0, 0, 0, 1, 3]) + ok[4:],
        "ind_lb beyond n_b": ok[:2] + ([0, 2, 5], [0, 4, 0, 1, 4]) + ok[4:],  # problem 1: n_b = 4
        "ind_ub negative": ok[:4] + ([0, 1, 1], [-1]),
    }
    for what, args in bad.items():
        r, msg = create(*args)
        assert r == -1 and msg, what  # MADQP_ERR_ARG with a message
    # equality rows in the condensed form without delta_d < 0
    opt0 = native_options(IPMOptions())
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in ([0, 1, 2], [0, 1], [0, 0, 0], [], [0, 0, 0], [])]
    ps = [a.ctypes.data_as(C.POINTER(C.c_int64)) if a.size else None for a in arrs]
    h = C.c_void_p()
    assert lib.madqp_batch_create_patterns(hip.ctx, B, nx, m, *ps, C.byref(data), C.byref(opt0), C.byref(h)) == -1
    assert create(*ok)[0] == 0  # the context is still usable
