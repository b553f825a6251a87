"""GPU: the matrix methods of the Julia glue -- ``MadNLP.solve!(::HIPCholeskySolver, X::AbstractMatrix)`` and
``MadNLP.solve!(kkt, W::AbstractMatrix)`` of julia/MadQPHIP.jl, the latter also of julia/MadQPHIPSparse.jl -- replayed
through the C ABI in their order, in the manner of tests/test_gpu_julia_replay.py: Julia cannot run here, so the replay
classes of tests/julia_replay.py / tests/julia_replay_sparse.py are extended by the ccall of each new method, argument for
argument (a Julia matrix is column-major with stride ``size(., 1)``: the torch tensor ``(size(., 2), size(., 1))``).

The calls go through the recorders of those modules (``JR.ccall`` / ``JS.ccall``): the coverage assertions of
tests/test_gpu_julia_replay.py and tests/test_gpu_julia_sparse.py hold the set of symbols the glue binds to the set the
replays touched in the session, and this file, which pytest collects before them, is where the two new symbols are
replayed."""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import julia_replay as JR
import julia_replay_sparse as JS
from oracle import qp as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, MROWS = 150, 40


@pytest.fixture(scope="module")
def rbe():
    be = JR.ReplayBackend(0)
    yield be
    be.close()


def solve_matrix_ls(ccall, ls, X):
    """MadNLP.solve!(s::HIPCholeskySolver, X::AbstractMatrix)"""
    ccall(ls.be, "madqp_chol_solve_many", ls.chol, JR.ptr(X), X.shape[1], X.shape[0])
    return X


def solve_matrix_kkt(ccall, kkt, W):
    """MadNLP.solve!(kkt, W::AbstractMatrix): the KKT's own state view, as solve!(kkt, w)"""
    ccall(kkt.be, "madqp_kkt_solve_many", kkt.handle, JR.C.byref(kkt.cstate), JR.ptr(W), W.shape[1], W.shape[0])
    return W


def prepared(rbe, cls, rng):
    """a condensed KKT object of the glue after compress_*!, initialize! and factorize_wrapper!, and its matrix"""
    qp = Q.synthetic_qp(3, NX, MROWS)
    jI, jJ, jv = JR.coo_pattern(qp.A, rng)
    hI, hJ, hv = JR.coo_pattern(np.tril(qp.H), rng)
    n = NX + MROWS
    kkt = cls(rbe, "condensed", NX, MROWS, np.arange(MROWS), np.arange(n), np.arange(n), jI, jJ, hI, hJ)
    kkt.get_jacobian().copy_(torch.as_tensor(jv, device=rbe.device))
    kkt.compress_jacobian()
    kkt.get_hessian().copy_(torch.as_tensor(hv, device=rbe.device))
    kkt.compress_hessian()
    kkt.initialize()
    sig = rng.uniform(0.5, 2.0, n)
    kkt.pr_diag.copy_(torch.as_tensor(sig, device=rbe.device))
    kkt.du_diag.fill_(-1.0)
    kkt.factorize_wrapper()
    assert kkt.linear_solver.is_factorized() and kkt.linear_solver.order == NX
    theta = sig[NX:] / (1.0 + sig[NX:])
    return kkt, qp.H + np.diag(sig[:NX]) + (qp.A.T * theta) @ qp.A


@pytest.mark.parametrize("glue", ["MadQPHIP", "MadQPHIPSparse"])
def test_matrix_methods_replayed(rbe, glue):
    rng = np.random.default_rng(21)
    cls, ccall = (JR.ReplayKKTSystem, JR.ccall) if glue == "MadQPHIP" else (JS.ReplaySparseKKTSystem, JS.ccall)
    kkt, K = prepared(rbe, cls, rng)
    try:
        ntot = kkt.cstate.n + kkt.cstate.m + kkt.cstate.nlb + kkt.cstate.nub
        for nrhs in (3, 40):  # either side of any cut-over between the two paths of madqp_chol_solve_many
            if glue == "MadQPHIP":  # (the sparse glue uses the same linear solver type: the method is inherited)
                B = rng.standard_normal((nrhs, NX))
                X = torch.as_tensor(B, device=rbe.device).clone()
                assert solve_matrix_ls(ccall, kkt.linear_solver, X) is X
                ref = sla.cho_solve(sla.cho_factor(K, lower=True), B.T).T
                assert np.max(np.abs(X.cpu().numpy() - ref)) <= 1e-11 * np.max(np.abs(ref))
            W0 = rng.standard_normal((nrhs, ntot))
            W = torch.as_tensor(W0, device=rbe.device).clone()
            assert solve_matrix_kkt(ccall, kkt, W) is W
            out = W.cpu().numpy()
            for c in range(nrhs):
                w = torch.as_tensor(W0[c], device=rbe.device).clone()
                kkt.solve(w)  # solve!(kkt, w), the glue's AUTO refinement request in force for both
                ref = w.cpu().numpy()
                assert np.max(np.abs(out[c] - ref)) < 1e-10 * np.max(np.abs(ref)), (nrhs, c)
    finally:
        kkt.close()


@pytest.mark.parametrize("glue,symbols", [("MadQPHIP", ("madqp_chol_solve_many", "madqp_kkt_solve_many")),
                                          ("MadQPHIPSparse", ("madqp_kkt_solve_many",))])
def test_the_glue_passes_the_matrix_as_the_replay_does(glue, symbols):
    src = open(os.path.join(ROOT, "julia", glue + ".jl")).read()
    for sym in symbols:
        call = re.search(r"function MadNLP\.solve!\(\w+::\w+, (\w)::AbstractMatrix\)\s*\n\s*check\([^\n]*ccall\(\(:" + sym
                         + r", libmadqp\), Int32,[^\n]*Int64, Int64\),\s*\n([^\n]*)\)\)", src)
        assert call, sym
        m = call.group(1)
        assert f"dptr({m}), size({m}, 1), size({m}, 2)" in call.group(2)
