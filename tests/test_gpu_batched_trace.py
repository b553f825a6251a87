"""GPU: the per-iteration trace of the lock-step batched engine (written on the device by the loop head, csrc/batch_wg.inc:
bq_iter_pre_kernel) and `refine_steps` inside it (wg_solve_system), against the CPU oracle under the rule of tests/parity.py.

Before these two options existed the soak could hold the batched engine to iteration count, objective and solution only
(tests/test_gpu_soak.py: `trace = name != "batched"`); here its traces are held to the per-iteration bar with the one remedy
the project has for small ill-conditioned problems -- a refinement step per solve -- switched on, as the AUTO rule does for
the single-problem drivers.  The bar, SENS_FACTOR and the tie cap are those of the soak.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
from oracle import mpc
from oracle import qp as Q
from parity import assert_parity, ensemble_floor, exceeds_stated_bar, iteration_parity
from test_gpu_soak import soak_cases

pytestmark = pytest.mark.gpu
REG, OREG = M.FixedRegularization(1e-8, -1e-8), mpc.FixedRegularization(1e-8, -1e-8)
RECORD_KEYS = {"k", "obj", "inf_pr", "inf_du", "inf_compl", "mu", "dnorm", "del_w", "alpha_d", "alpha_p", "residual_ratio"}
BITWISE = ("solution", "multipliers", "multipliers_L", "multipliers_U")


def to_device(qp, be):
    return M.DeviceQP.from_numpy(be.device, qp.H, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0)


def solve(hip, dqs, **kw):
    kw.setdefault("regularization", REG)
    s = M.BatchedMPCSolver(dqs, hip, **kw)
    try:
        return s.solve()
    finally:
        s.close()


def first_batch(hip):
    qps = [Q.synthetic_qp(500 + 7 * i + 64, 64, 24, "wigner") for i in range(12)]  # test_batched_vs_oracle, first case
    return qps, [to_device(q, hip) for q in qps]


def same_bits(a, b):
    return a["status"] == b["status"] and a["iter"] == b["iter"] and a["objective"] == b["objective"] and all(
        np.array_equal(a[k], b[k]) for k in BITWISE)


def test_trace_shape_and_bookkeeping(hip):
    qps, dqs = first_batch(hip)
    res = solve(hip, dqs, trace=True)
    assert len({r["iter"] for r in res}) > 1  # the problems stop at different iterations
    for i, (qp, r) in enumerate(zip(qps, res)):
        ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG)
        tr = r["trace"]
        assert r["status"] == M.SOLVE_SUCCEEDED
        assert len(tr) == r["iter"] + 1, (i, len(tr), r["iter"])
        assert [t["k"] for t in tr] == list(range(r["iter"] + 1))
        assert all(set(t) == RECORD_KEYS for t in tr)
        assert tr[0]["dnorm"] == 0.0
        for key in ("inf_pr", "inf_du", "inf_compl", "mu", "del_w"):
            assert tr[-1][key] == r[key], (i, key, tr[-1][key], r[key])
        assert tr[-1]["obj"] == r["objective"]
        assert r["iter"] == ref["iter"]
        assert [t["del_w"] for t in tr] == [t["del_w"] for t in ref["trace"]], i  # 1.0 at the start point, 1e-8 after
        assert tr[0]["del_w"] == 1.0 and all(t["del_w"] == 1e-8 for t in tr[1:])
    head = solve(hip, dqs, trace=3)
    for r, h in zip(res, head):
        assert same_bits(r, h)
        assert h["trace"] == r["trace"][:3]


@pytest.mark.parametrize("kw", [dict(max_ncorr=3), dict(per_problem_patterns=True)], ids=["gondzio", "patterns"])
def test_tracing_changes_nothing(hip, kw):
    _, dqs = first_batch(hip)
    plain = solve(hip, dqs, trace=False, **kw)
    traced = solve(hip, dqs, trace=True, **kw)
    assert all("trace" not in r for r in plain)
    for i, (a, b) in enumerate(zip(plain, traced)):
        assert same_bits(a, b), i
        assert len(b["trace"]) == b["iter"] + 1


@pytest.mark.parametrize("seed0,count,only_lp", [(9000, 200, True), (1000, 150, False)])
def test_trace_follows_the_oracle_with_refinement(hip, seed0, count, only_lp):
    """The soak streams the batched engine already runs, each problem as a batch of one with refine_steps=1, under the rule
    tests/test_gpu_soak.py:run_case applies to the native driver -- per-iteration traces included."""
    ties, cases, beyond_bar = [], 0, 0
    for seed, n, m, lp in soak_cases(seed0, count, only_lp):
        qp = Q.random_qp(seed, n, m, lp)
        ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG)
        r = solve(hip, [to_device(qp, hip)], refine_steps=1, trace=True)[0]
        cases += 1
        what = (seed, n, m, lp, "batched refine_steps=1")
        assert r["status"] == ref["status"], (what, r["status"], ref["status"])
        if ref["status"] != M.SOLVE_SUCCEEDED:
            continue
        if iteration_parity(r, ref, 1e-8, what, lp=lp) == "tie":
            ties.append((what, r["iter"], ref["iter"]))
            dobj = abs(r["objective"] - ref["objective"]) / max(1.0, abs(ref["objective"]))
            assert dobj <= 1e-7, (what, "objective after a tie", dobj)
            continue
        floor = None
        if exceeds_stated_bar(r, ref, trace=True):
            beyond_bar += 1
            floor = ensemble_floor(qp, ref, regularization=OREG)
        assert_parity(r, ref, qp, what, trace=True, floor=floor, regularization=OREG)
    print(f"batched trace soak seed0={seed0}: {cases} solves, {beyond_bar} beyond the stated bar (held to the ensemble "
          f"floor), {len(ties)} threshold ties: {ties}")
    assert all(w[3] for w, _, _ in ties), ("a threshold tie on a QP", ties)
    assert len(ties) <= max(2, cases // 20), ties


def test_refinement_is_the_drivers_refinement(hip):
    qp = Q.random_qp(9030, 204, 51, False)  # test_refinement_inside_solve_is_the_drivers_refinement's problem
    ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG)
    dqs = [to_device(qp, hip) for _ in range(4)]
    out = {steps: solve(hip, dqs, refine_steps=steps, trace=True) for steps in (0, 1, 2)}
    assert all(r["status"] == M.SOLVE_SUCCEEDED for res in out.values() for r in res)
    mean_ratio = {steps: float(np.mean([t["residual_ratio"] for t in res[0]["trace"][1:]])) for steps, res in out.items()}
    print("mean residual_ratio over iterations by refine_steps:", mean_ratio)
    assert not np.array_equal(out[0][0]["solution"], out[1][0]["solution"])  # (a) the option is not ignored
    for steps in (1, 2):  # (b), (d)
        res = out[steps]
        for r in res[1:]:
            assert same_bits(res[0], r) and r["trace"] == res[0]["trace"]
        assert_parity(res[0], ref, qp, f"soak9030 batched refine_steps={steps}", trace=True, regularization=OREG)
    assert mean_ratio[1] < mean_ratio[0], mean_ratio  # (c) a direction, not a tolerance


def test_every_solve_refines(hip):
    """Gondzio's trial solves and the normal equations go through the same wg_solve_system.

    The oracle runs with the same algorithmic options (max_ncorr / kkt_system, regularization) and -- as everywhere in the
    parity tests, e.g. test_gpu_soak.py::test_refinement_inside_solve_is_the_drivers_refinement -- as the LAPACK execution
    the ensemble floor of tests/parity.py is measured from, i.e. without a refinement step of its own: refinement is a way
    to execute the solves, not another algorithm, and `ensemble_floor` handed refine_steps=1 would compare refined
    executions with each other only.  Measured for the record (MI355X, problem 9030, max_ncorr=3): the engine with one step
    is as far from the LAPACK run as the oracle's own refined run is (2.9e-07 ... 5.0e-06 per iteration, floor 7.3e-07 ...
    6.2e-06); against the REFINED oracle it is at 9e-09 in inf_du at iteration 2, where five refined CPU executions
    differ by 1.2e-11 among themselves -- one step from the inverse-image product leaves a residual ratio of ~1e-09, two
    steps ~1e-13 (LAPACK's first solve is already there)."""
    qp = Q.random_qp(9030, 204, 51, False)
    ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG, max_ncorr=3)
    r = solve(hip, [to_device(qp, hip)], max_ncorr=3, refine_steps=1, trace=True)[0]
    assert r["status"] == ref["status"] == M.SOLVE_SUCCEEDED
    assert_parity(r, ref, qp, "soak9030 batched gondzio refine_steps=1", trace=True, regularization=OREG, max_ncorr=3)
    lp = Q.random_qp(9195, 186, 78, True)  # an LP of the first stream (test_seed_9195_condensed_lp)
    reg0, oreg0 = M.FixedRegularization(1e-8, 0.0), mpc.FixedRegularization(1e-8, 0.0)
    ref = mpc.solve(lp, kkt_system="normal", regularization=oreg0)
    r = solve(hip, [to_device(lp, hip)], kkt_system="normal", regularization=reg0, refine_steps=1, trace=True)[0]
    assert r["status"] == ref["status"] == M.SOLVE_SUCCEEDED
    # (the ensemble floor of tests/parity.py is a floor of the condensed form: the normal equations must meet the stated bar)
    assert assert_parity(r, ref, lp, "seed 9195 batched normal refine_steps=1", trace=True, regularization=oreg0) == "bar"


def test_errors(hip):
    _, dqs = first_batch(hip)
    for bad in (0, -2):
        with pytest.raises(ValueError):
            M.BatchedMPCSolver(dqs[:2], hip, regularization=REG, trace=bad)
    with pytest.raises(ValueError):
        M.BatchedMPCSolver(dqs[:2], hip, regularization=REG, refine_steps=-1)
    s = M.BatchedMPCSolver(dqs[:2], hip, regularization=REG)
    s.initialize()
    try:
        assert hip.lib.madqp_batch_set_trace(s._h, 5) == -4  # MADQP_ERR_STATE: after madqp_batch_init
        assert hip.lib.madqp_batch_trace(s._h, None, (C.c_int32 * 2)()) == -4  # no trace was set
        copt = M.solver.native_options(s.opt)
        copt.refine_steps = -1  # the library itself refuses it too
        h = C.c_void_p()
        c0 = torch.zeros(2, dtype=torch.float64, device=hip.device)
        data = M._lib.CBatchData(c0=M._lib.ptr(c0))
        assert hip.lib.madqp_batch_create(hip.ctx, 2, 0, 0, 0, None, 0, None, 0, None, C.byref(data), C.byref(copt),
                                          C.byref(h)) == -1  # MADQP_ERR_ARG
    finally:
        s.close()
    t = M.BatchedMPCSolver(dqs[:2], hip, regularization=REG, trace=2)
    t.initialize()
    try:
        assert hip.lib.madqp_batch_set_trace(t._h, 5) == -4  # twice
    finally:
        t.close()
