"""GPU: one H and one A shared by every problem of a batch (``shared_matrices=True``, madqp_batch_share_matrices).

The acceptance rule is bitwise: the library multiplies each entry of the shared H by the problem's obj_scale as it loads
it -- one IEEE product, the double the stacked form keeps in memory -- and the assembly starts from that product written
into K, so a shared batch must give the stacked batch's results bit for bit, traces included.  Every batch here is one
model (tests/test_batched_shared.py: base_problem) with per-problem q, variable bounds and row bounds (family)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
from madqp_jl_amd._lib import CBatchData, ptr
from madqp_jl_amd.options import IPMOptions
from madqp_jl_amd.solver import native_options
from oracle import mpc
from parity import assert_parity
from test_batched_shared import base_problem, family, stacked_and_shared
from test_gpu_batched_patterns import random_pattern

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG, OREG = M.FixedRegularization(1e-8, -1e-8), mpc.FixedRegularization(1e-8, -1e-8)
REG0, OREG0 = M.FixedRegularization(1e-8, 0.0), mpc.FixedRegularization(1e-8, 0.0)
BITWISE = ("solution", "multipliers", "multipliers_L", "multipliers_U")
MADQP_ERR_ARG, MADQP_ERR_STATE = -1, -4

# name -> (n, m, B, lp, solver options, per-problem pattern): the smallest shapes at which each path can go wrong
CASES = {
    "two_blocks": (130, 40, 6, False, {}, None),          # two 128-blocks, a short second one
    "no_rows": (64, 0, 6, False, {}, None),               # empty product: K = base + diagonal only
    "more_rows": (72, 200, 6, False, {}, None),           # m > nx
    "beyond_symv": (520, 16, 4, False, {}, None),         # nx > 512: the wg_gemv_t form of the H product, no sym scratch
    "lp_condensed": (40, 16, 8, True, {}, None),          # H None, A shared
    "lp_normal": (40, 16, 8, True, dict(kkt_system="normal", regularization=REG0), None),
    "gondzio": (64, 24, 7, False, dict(max_ncorr=3), None),
    "refine": (64, 24, 7, False, dict(refine_steps=1), None),
    "patterns": (64, 24, 7, False, dict(per_problem_patterns=True), random_pattern),
    "unscaled": (64, 24, 7, False, dict(scaling=False), None),  # h_scale NULL
    "different_stops": (64, 24, 12, False, {}, None),
}


def problems(name):
    n, m, B, lp, _, pattern = CASES[name]
    pat = None if pattern is None else (lambda qp, rng: pattern(qp, rng, lp=lp))
    return family(base_problem(n, m, 4000 + n + m, lp), B, 17 + n, pat)


def run(hip, dqs, **kw):
    kw.setdefault("regularization", REG)
    s = M.BatchedMPCSolver(dqs, hip, trace=True, **kw)
    try:
        return s.solve()
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def both(hip, name):
    """(problems, stacked results, shared results) of a case, solved once for every test that looks at it."""
    qps = problems(name)
    stacked, shared = stacked_and_shared(qps, hip.device)
    kw = CASES[name][4]
    return qps, run(hip, stacked, **kw), run(hip, shared, shared_matrices=True, **kw)


def assert_same_bits(a, b, what):
    assert a["status"] == b["status"] and a["iter"] == b["iter"], (what, a["status"], b["status"], a["iter"], b["iter"])
    assert a["n_factorizations"] == b["n_factorizations"], (what, a["n_factorizations"], b["n_factorizations"])
    assert a["objective"] == b["objective"] or (a["objective"] != a["objective"] and b["objective"] != b["objective"]), what
    for k in BITWISE:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert len(a["trace"]) == len(b["trace"]), what
    for ta, tb in zip(a["trace"], b["trace"]):
        assert set(ta) == set(tb)
        for k in ta:
            assert ta[k] == tb[k] or (ta[k] != ta[k] and tb[k] != tb[k]), (what, ta["k"], k, ta[k], tb[k])


# ---------------------------------------------------------------------------------------------- 1: bitwise the stacked form
@pytest.mark.parametrize("name", list(CASES))
def test_shared_is_bitwise_the_stacked_form(hip, name):
    qps, stacked, shared = both(hip, name)
    assert len(stacked) == len(shared) == len(qps)
    for b, (r0, r1) in enumerate(zip(stacked, shared)):
        assert_same_bits(r0, r1, (name, b))
    assert any(r["status"] == M.SOLVE_SUCCEEDED for r in stacked), name  # (the case is a solve, not a common breakdown)
    if name == "different_stops":
        assert len({r["iter"] for r in stacked}) > 1, [r["iter"] for r in stacked]


# ---------------------------------------------------------------------------------------------- 2: the x100 retry
def test_retry_rounds_start_from_the_scaled_H(hip):
    """The construction of test_gpu_batched.py::test_batched_regularization_retry with ONE H: a slightly negative diagonal
    entry on variable 3, which no row and no q touches.  The problem that fails is made to fail through its own bounds --
    variable 3 is free in problem 2 alone (Sigma = 0 there, K[3][3] = -1e-7 + 1e-8 < 0), bounded in the others -- so the
    batch has per-problem patterns.  By the retry rounds K holds what the failed factorisation left: an assembly that did
    not start again from fl(h_scale * H) would not give the stacked form's bits, nor the oracle's count."""
    free, bad = 3, 2
    base = base_problem(20, 8, 40)
    base.H = np.diag(np.diag(base.H))
    base.H[free, free] = -1e-7
    base.A[:, free] = 0.0
    base.q[free] = 0.0
    qps = family(base, 5, 9)
    for i, qp in enumerate(qps):
        qp.q = base.q + 0.05 * np.random.default_rng(90 + i).standard_normal(20)  # (obj_scale = 1: the entry stays -1e-7)
        qp.q[free] = 0.0
        if i == bad:
            qp.lvar[free], qp.uvar[free] = -np.inf, np.inf
    stacked, shared = stacked_and_shared(qps, hip.device)
    kw = dict(per_problem_patterns=True, max_iter=4)
    r0, r1 = run(hip, stacked, **kw), run(hip, shared, shared_matrices=True, **kw)
    for i, (qp, a, b) in enumerate(zip(qps, r0, r1)):
        assert_same_bits(a, b, ("retry", i))
        ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG, max_iter=4)
        assert b["status"] == ref["status"] and b["iter"] == ref["iter"], (i, b["status"], ref["status"], b["iter"], ref["iter"])
        assert b["n_factorizations"] == ref["n_factorizations"], (i, b["n_factorizations"], ref["n_factorizations"])
    assert r1[bad]["n_factorizations"] > r1[0]["n_factorizations"]  # only the bad problem paid for retries


# ---------------------------------------------------------------------------------------------- 3: against the oracle
@pytest.mark.parametrize("name", ["refine", "lp_condensed"])
def test_shared_follows_the_oracle(hip, name):
    qps, _, shared = both(hip, name)
    for b, (qp, r) in enumerate(zip(qps, shared)):
        ref = mpc.solve(qp, kkt_system="condensed", regularization=OREG)
        assert r["status"] == ref["status"] == M.SOLVE_SUCCEEDED, (name, b, r["status"], ref["status"])
        assert_parity(r, ref, qp, (name, b), trace=True, regularization=OREG)


# ---------------------------------------------------------------------------------------------- 5: sharing is real
def test_the_library_reads_the_callers_own_matrices(hip):
    qps = problems("refine")
    _, shared = stacked_and_shared(qps, hip.device)
    H, A = shared[0].H, shared[0].A
    seen = {}

    def look(solver):
        seen["H"], seen["A"] = solver._data.H, solver._data.A
        seen["shapes"] = (tuple(solver._H.shape), tuple(solver._A.shape))

    for scaling in (True, False):
        s = M.BatchedMPCSolver(shared, hip, shared_matrices=True, scaling=scaling, regularization=REG)
        s.pre_create_hook = look
        first = s.solve()
        assert seen["H"] == H.data_ptr()  # H is never scaled on the host
        assert seen["shapes"] == ((1, 64, 64), (1, 24, 64))
        if not scaling:
            assert seen["A"] == A.data_ptr()
        else:
            assert seen["A"] == s._A.data_ptr() and s._A.numel() == A.numel()  # scaled once
        assert s.H.shape[0] == 1 and s.A.shape[0] == 1
        # the ONE H changes under the solver: every problem's result changes
        keep = H.clone()
        H.diagonal().add_(0.5)
        second = s.solve()
        s.close()
        H.copy_(keep)
        for b, (r0, r1) in enumerate(zip(first, second)):
            assert r0["status"] == r1["status"] == M.SOLVE_SUCCEEDED, (scaling, b)
            assert not np.array_equal(r0["solution"], r1["solution"]), (scaling, b)
    # ... and likewise the ONE A (unscaled: the caller's own storage)
    s = M.BatchedMPCSolver(shared, hip, shared_matrices=True, scaling=False, regularization=REG)
    first = s.solve()
    keep = A.clone()
    A.mul_(0.5)
    second = s.solve()
    s.close()
    A.copy_(keep)
    for b, (r0, r1) in enumerate(zip(first, second)):
        assert not np.array_equal(r0["solution"], r1["solution"]), b


# ---------------------------------------------------------------------------------------------- 6: errors
def _handle(hip, lp):
    """A batch of two tiny problems straight at the C ABI; returns (handle, the arrays it borrows)."""
    nx, m, B = 4, 2, 2
    f64 = dict(dtype=torch.float64, device=hip.device)
    keep = dict(H=None if lp else torch.eye(nx, **f64).repeat(B, 1, 1).contiguous(),
                A=torch.ones((B, m, nx), **f64), q=torch.ones((B, nx), **f64), rhs=torch.zeros((B, m), **f64),
                c0=torch.zeros(B, **f64), x=torch.full((B, nx + m), 0.5, **f64), xl=torch.zeros((B, nx + m), **f64),
                xu=torch.full((B, nx + m), 4.0, **f64), zl=torch.zeros((B, nx + m), **f64),
                zu=torch.zeros((B, nx + m), **f64), y=torch.zeros((B, m), **f64),
                ind=torch.arange(nx + m, dtype=torch.int64, device=hip.device), hs=torch.ones(B, **f64))
    data = CBatchData(**{k: ptr(keep[k]) for k in ("H", "A", "q", "rhs", "c0", "x", "xl", "xu", "zl", "zu", "y")})
    opt = native_options(IPMOptions(regularization=REG))
    h = C.c_void_p()
    ineq = (C.c_int64 * m)(*range(m))
    hip._ck(hip.lib.madqp_batch_create(hip.ctx, B, nx, m, m, ineq, nx + m, ptr(keep["ind"]), nx + m, ptr(keep["ind"]),
                                       C.byref(data), C.byref(opt), C.byref(h)))
    return h, keep


def test_share_matrices_errors(hip):
    lib = hip.lib
    h, keep = _handle(hip, lp=False)
    assert lib.madqp_batch_share_matrices(h, 0, 0, ptr(keep["hs"])) == MADQP_ERR_ARG  # h_scale without share_H
    assert lib.madqp_batch_share_matrices(h, 1, 1, ptr(keep["hs"])) == 0
    assert lib.madqp_batch_share_matrices(h, 1, 1, ptr(keep["hs"])) == MADQP_ERR_STATE  # twice
    assert b"madqp_batch_share_matrices" in lib.madqp_last_error(hip.ctx)
    lib.madqp_batch_destroy(h)
    h, keep = _handle(hip, lp=False)
    hip._ck(lib.madqp_batch_init(h, 0.1, 1e-2))
    assert lib.madqp_batch_share_matrices(h, 1, 1, None) == MADQP_ERR_STATE  # after init
    lib.madqp_batch_destroy(h)
    h, keep = _handle(hip, lp=True)
    assert lib.madqp_batch_share_matrices(h, 1, 1, None) == MADQP_ERR_ARG  # share_H without an H
    assert lib.madqp_batch_share_matrices(h, 0, 1, None) == 0  # (the refused call left the handle as it was)
    lib.madqp_batch_destroy(h)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4: both workgroup widths
def test_narrow_programs_in_a_child_process(hip):
    """MADQP_BATCH_WIDE_MAX is read once per process: a child runs one case with the 256-thread programs and compares shared
    against stacked itself (tests/batched_shared_child.py).  A child that ends with a fault or at its time limit ends the
    session: nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "batched_shared_child.py"), "two_blocks"]
    try:
        p = subprocess.run(cmd, env=dict(os.environ, MADQP_BATCH_WIDE_MAX="0"), capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"batched_shared_child.py ran into its time limit: {e}", returncode=3)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        pytest.exit(f"batched_shared_child.py ended with {p.returncode}: {p.stderr[-2000:]}", returncode=3)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    assert "narrow programs: shared == stacked" in p.stdout
