"""GPU: julia/MadQPHIPSparse.jl replayed through the C ABI (tests/julia_replay_sparse.py).

(a) A KKT object fed through the COO -> CSR maps is, bit for bit, the ``HIPSparse*`` object the Python front end builds
    from ``DeviceCSR.from_dense`` / ``DeviceSymCSR.from_dense``: every stored double of K, ``solve!``, ``mul!``, ``jtprod!``.
(b) Whole solves through the replayed glue against the CPU oracle, with the recipe of
    tests/test_gpu_sparse_hessian.py::test_whole_solves_vs_oracle (the bar is measured from two oracle executions).
(c) The ccall targets of the Julia file are the symbols the replay touched."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import julia_replay as JR
import julia_replay_sparse as JS
import madqp_jl_amd as M
import parity
import sparse_hessian as SH
from oracle import mpc
from oracle import qp as Q
from test_gpu_julia_replay import CASES as GLUE_CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = M.FixedRegularization(1e-8, -1e-8)
KKT_FIELDS = ("reg", "pr_diag", "du_diag", "l_diag", "l_lower", "u_diag", "u_lower")


@pytest.fixture(scope="module")
def sbe():
    be = JS.ReplaySparseBackend(0)
    yield be
    be.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(t):
    return t.detach().cpu().numpy().copy()


def whole_matrix(be, handle, order):
    """Every stored double of the first ``order`` columns of the library's K (padding rows included)."""
    p, ld = be.kkt_matrix(handle, order)
    return be.read_doubles(p, ld * order)


def problem(nx, m, form):
    """The sparse-Jacobian family at (nx, m); H: none for the normal equations, else a sparse SPD matrix -- the arrow
    pattern (row 0 of the full pattern holds all 300 entries) at nx = 300.  At nx = 129 row 5 and column 7 of A are empty."""
    qp = Q.sparse_qp(40 + nx, nx, m, 2, "lp")
    if nx == 129:
        qp.A[5, :] = 0.0
        qp.A[:, 7] = 0.0
        assert not qp.A[5].any() and not qp.A[:, 7].any() and qp.A.any()
    H = None
    if form != "normal":
        r, c, v = SH.pattern("arrow" if nx == 300 else "generator", nx)
        H = np.zeros((nx, nx))
        H[r, c] = v
        H = H + np.tril(H, -1).T
    return qp, H


@pytest.mark.parametrize("form", ["condensed", "normal", "augmented"])
@pytest.mark.parametrize("nx,m", [(1, 1), (129, 43), (300, 100)])
def test_maps_feed_the_kkt_object_the_python_front_end_builds(hip, sbe, nx, m, form):
    """``hip`` carries the Python front end, ``sbe`` the replay: two contexts on one stream."""
    be = sbe
    qp, H = problem(nx, m, form)
    dq = M.DeviceQP.from_numpy(hip.device, None, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0, sparse=True)
    if H is not None:
        dq.H = M.DeviceSymCSR.from_dense(hip.device, H)
    kw = dict(regularization=REG) if form == "condensed" else {}
    s = M.MPCSolver(dq, hip, kkt_system=form, **kw)
    s.initialize()
    assert type(s.kkt).__name__.startswith("HIPSparse") and isinstance(s.A, M.DeviceCSR)
    s.kkt.set_refine(-1)  # what the glue asks for (MadIPM's loop calls solve! once)
    st = s.st
    # the scaled model data the Python object holds, as a model would report it: shuffled COO with 9 split entries each
    A = host(s.A.to_dense())
    Hs = None if H is None else host(s.H.to_dense())
    rng = np.random.default_rng(nx + m)
    (jI, jJ, jv), (hI, hJ, hv) = JS.model_patterns(A, Hs, rng, duplicates=9)
    assert len(jv) == min(np.count_nonzero(A), 9) + np.count_nonzero(A)
    kkt = JS.ReplaySparseKKTSystem(be, form, nx, m, s.ind_ineq, host(st.ind_lb), host(st.ind_ub), jI, jJ, hI, hJ)
    kkt.get_jacobian().copy_(torch.as_tensor(jv, device=be.device))
    kkt.compress_jacobian()
    if len(hv):
        kkt.get_hessian().copy_(torch.as_tensor(hv, device=be.device))
        kkt.compress_hessian()
    # nothing of size nx * m or nx * nx: the largest tensor is a callback buffer, a CSR value array or a KKT diagonal
    assert kkt.largest_tensor() <= max(len(jv), len(hv) * 2, st.n, 1)
    assert nx * m <= 1 or kkt.largest_tensor() < min(nx * m, nx * nx)
    # the CSR operands are the Python front end's, bit for bit (the split halves add up exactly)
    assert np.array_equal(bits(host(kkt.a_val)), bits(host(s.A.val)))
    assert np.array_equal(bits(host(kkt.at_val)), bits(host(s.A.t_val)))
    if len(hv):
        assert np.array_equal(bits(host(kkt.h_val)), bits(host(s.H.val)))
    # one state: the diagonals the Python object has after set_aug_diagonal_reg!, copied into the replay's own fields
    kkt.initialize()
    # (del_c = 0 for the normal equations, as every caller of that form has it: its solve! leaves the dual
    # regularization out -- src/KKT/normalkkt.jl:182-205 -- while mul! applies it)
    s.kkt.set_aug_diagonal_reg(1.0, 0.0 if form == "normal" else -1e-8)
    for k in KKT_FIELDS:
        getattr(kkt, k).copy_(getattr(st, k))
    order = {"condensed": nx, "normal": m, "augmented": (nx + 127) // 128 * 128 + m}[form]
    assert kkt.linear_solver.order == order
    s.kkt.build_kkt()
    kkt.build_kkt()
    what = (form, nx, m)
    assert np.array_equal(bits(whole_matrix(be, kkt.handle, order)), bits(whole_matrix(hip, s.kkt._h, order))), what
    s.kkt.linear_solver.factorize()
    kkt.linear_solver.factorize()
    assert kkt.linear_solver.is_factorized() and s.kkt.linear_solver.is_factorized(), what
    assert np.array_equal(bits(whole_matrix(be, kkt.handle, order)), bits(whole_matrix(hip, s.kkt._h, order))), what
    b = torch.as_tensor(rng.standard_normal(st.ntot), device=be.device)
    w_r, w_p = b.clone(), b.clone()
    kkt.solve(w_r)  # solve!
    s.kkt.solve(w_p)
    assert np.all(np.isfinite(host(w_r))) and np.array_equal(bits(host(w_r)), bits(host(w_p))), what
    r_r, r_p = b.clone(), b.clone()
    kkt.mul(r_r, w_r, -1.0, 1.0)  # mul!(w, kkt, d, -1, 1): the residual of solve_system!
    s.kkt.mul(r_p, w_p, -1.0, 1.0)
    assert np.array_equal(bits(host(r_r)), bits(host(r_p))), what
    # ... and it is a solve: a backward error far above rounding, far below a wrong entry
    assert float(r_r.abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()), float(w_r.abs().max())), what
    y = torch.as_tensor(rng.standard_normal(m), device=be.device)
    j_r = torch.full((st.n,), float("nan"), dtype=torch.float64, device=be.device)
    j_p = j_r.clone()
    kkt.jtprod(j_r, y)
    s.kkt.jtprod(j_p, y)
    assert np.all(np.isfinite(host(j_r))) and np.array_equal(bits(host(j_r)), bits(host(j_p))), what
    kkt.close()
    s.close()


def test_normal_form_refuses_a_hessian(sbe):
    one = np.ones(1, dtype=np.int32)
    with pytest.raises(ValueError, match="NormalKKTSystem supports only linear programs"):
        JS.ReplaySparseKKTSystem(sbe, "normal", 1, 1, [0], [0, 1], [0, 1], one, one, one, one)


def to_device(qp, be):
    return M.DeviceQP.from_numpy(be.device, qp.H, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0)


# (name, make, form, oracle kkt_system, regularization or None = the default, max_ncorr, oracle iterations)
WHOLE = [(f"sparse-hessian-{c[0]}-s{c[2]}-n{c[3]}-m{c[4]}",
          functools.partial(SH.sparse_hessian_qp, c[2], c[3], c[4], c[5], c[6], c[7]), c[0], c[1],
          (1e-8, -1e-8) if c[0] == "condensed" else None, 0, c[8]) for c in SH.CASES]
WHOLE += [(c[0], c[1], c[2], c[3], c[4], c[5], it)
          for c, it in zip([c for c in GLUE_CASES if c[2] in ("condensed", "augmented", "normal")],
                           (4, 4, 6, 6, 7, 10, 12, 9, 10))]
assert len(WHOLE) == 14


@functools.lru_cache(maxsize=None)
def oracle_runs(i):
    _, make, _, oform, reg, ncorr, _ = WHOLE[i]
    qp = make()
    kw = dict(max_ncorr=ncorr)
    if reg is not None:
        kw["regularization"] = mpc.FixedRegularization(*reg)
    return qp, mpc.solve(qp, kkt_system=oform, **kw), mpc.solve(qp, kkt_system=oform, refine_steps=1, **kw)


@pytest.mark.parametrize("i", range(len(WHOLE)), ids=[w[0] for w in WHOLE])
def test_madipm_loop_through_the_sparse_glue(sbe, i):
    """MadIPM.solve!(MPCSolver(qp; kkt_system = MadQPHIPSparse.HIPSparse*KKTSystem, linear_solver =
    MadQPHIP.HIPCholeskySolver)) against two executions of the oracle."""
    name, _, form, _, reg, ncorr, iters = WHOLE[i]
    qp, ref, ref2 = oracle_runs(i)
    assert ref["status"] == ref2["status"] == M.SOLVE_SUCCEEDED and ref["iter"] == ref2["iter"] == iters, name
    kw = dict(regularization=M.FixedRegularization(*reg)) if reg is not None else {}
    s = JS.ReplaySparseMPCSolver(to_device(qp, sbe), sbe, kkt_system=form, max_ncorr=ncorr, **kw)
    r = s.solve()
    assert type(s.kkt) is JS.ReplaySparseKKTSystem
    tol = s.opt.tol
    s.close()
    assert r["status"] == ref["status"], name
    assert parity.iteration_parity(r, ref, tol, name, lp=False) == "equal"
    parity.compare_traces_measured(r["trace"], ref["trace"], ref2["trace"], name)
    assert parity.close(r["objective"], ref["objective"], 1e-9), name
    assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-7, name


def test_every_symbol_the_sparse_glue_binds_was_replayed(sbe):
    """The ccall targets of julia/MadQPHIPSparse.jl, minus the create / destroy lifecycle, == the ABI symbols the replay
    touched (after one solve per form with Gondzio corrections, so that set_extra_correction! runs; the QP brings
    compress_hessian! and madqp_kkt_set_hcsr in)."""
    for form, make, reg in (("condensed", lambda: Q.dummy_qp(10, 5), (1e-8, -1e-8)),
                            ("augmented", lambda: Q.dummy_qp(10, 5), (1e-8, 0.0)),
                            ("normal", lambda: Q.simple_lp(), (1e-8, 0.0))):
        s = JS.ReplaySparseMPCSolver(to_device(make(), sbe), sbe, kkt_system=form,
                                     regularization=M.FixedRegularization(*reg), max_ncorr=2)
        assert s.solve()["status"] == M.SOLVE_SUCCEEDED
        s.close()
    src = open(os.path.join(ROOT, "julia", "MadQPHIPSparse.jl")).read()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    bound = set(re.findall(r"(?::|@k )(madqp_[a-z0-9_]+)", code))
    lifecycle = {"madqp_kkt_destroy", "madqp_csr_map_destroy"}  # close() here, finalizers there
    assert lifecycle <= bound
    assert bound - lifecycle == JS.SPARSE_ENTRY_POINTS, (sorted(bound - lifecycle - JS.SPARSE_ENTRY_POINTS),
                                                        sorted(JS.SPARSE_ENTRY_POINTS - bound))
    assert bound <= set(M.EXPORTED_SYMBOLS)
    # none of the new symbols went through the dense replay's recorder (its set is held to julia/MadQPHIP.jl)
    assert not {n for n in JR.GLUE_ENTRY_POINTS if "csr_map" in n or n in ("madqp_kkt_create_sparse", "madqp_kkt_set_hcsr")}
