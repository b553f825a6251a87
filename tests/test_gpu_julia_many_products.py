"""GPU: the block methods the Julia glue gained with the KKT products on a block of vectors --
``mul!(W::AbstractMatrix, kkt, V::AbstractMatrix, alpha, beta)`` and ``block_products!(kkt, on)`` of julia/MadQPHIP.jl and
julia/MadQPHIPSparse.jl -- replayed through the C ABI argument for argument, in the manner of tests/test_gpu_julia_many.py
(a Julia matrix is column-major with stride ``size(., 1)``: the torch tensor ``(size(., 2), size(., 1))``).  The calls go
through the recorders of tests/julia_replay.py / tests/julia_replay_sparse.py, so the coverage assertions of
tests/test_gpu_julia_replay.py and tests/test_gpu_julia_sparse.py, which pytest collects after this file, see the two new
symbols replayed."""
import os
import re

import numpy as np
import pytest
import torch

import julia_replay as JR
import julia_replay_sparse as JS
from test_gpu_julia_many import NX, MROWS, prepared, solve_matrix_kkt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def rbe():
    be = JR.ReplayBackend(0)
    yield be
    be.close()


def mul_matrix_kkt(ccall, kkt, W, V, alpha=1.0, beta=0.0):
    """mul!(W::AbstractMatrix, kkt, V::AbstractMatrix, alpha, beta)"""
    ccall(kkt.be, "madqp_kkt_mul_many", kkt.handle, JR.C.byref(kkt.cstate), JR.ptr(W), W.shape[1], JR.ptr(V), V.shape[1],
          W.shape[0], alpha, beta)
    return W


def block_products(ccall, kkt, on):
    """block_products!(kkt, on)"""
    ccall(kkt.be, "madqp_kkt_set_block_products", kkt.handle, 1 if on else 0)
    return kkt


@pytest.mark.parametrize("glue", ["MadQPHIP", "MadQPHIPSparse"])
def test_block_methods_replayed(rbe, glue):
    rng = np.random.default_rng(22)
    cls, ccall = (JR.ReplayKKTSystem, JR.ccall) if glue == "MadQPHIP" else (JS.ReplaySparseKKTSystem, JS.ccall)
    kkt, _ = prepared(rbe, cls, rng)
    try:
        ntot = kkt.cstate.n + kkt.cstate.m + kkt.cstate.nlb + kkt.cstate.nub
        t = lambda a: torch.as_tensor(a, device=rbe.device).clone()
        g = (NX + MROWS + 8) * U / (1.0 - (NX + MROWS + 8) * U)
        E, KE = torch.eye(ntot, dtype=torch.float64, device=rbe.device), torch.zeros((ntot, ntot), dtype=torch.float64, device=rbe.device)
        for c in range(ntot):
            kkt.mul(KE[c], E[c], 1.0, 0.0)
        absK = np.abs(KE.cpu().numpy().T)  # the explicit |K| (exact: mul on unit vectors)
        for nrhs in (3, 17):
            W0, V0 = rng.standard_normal((nrhs, ntot + 2)), rng.standard_normal((nrhs, ntot))
            W, V = t(W0), t(V0)
            assert mul_matrix_kkt(ccall, kkt, W, V, -1.0, 1.0) is W
            out = W.cpu().numpy()
            assert np.array_equal(out[:, ntot:], W0[:, ntot:])
            for c in range(nrhs):
                w, v = t(W0[c, :ntot]), t(V0[c])
                kkt.mul(w, v, -1.0, 1.0)  # mul!(w, kkt, v, -1, 1)
                bound = 2 * g * (absK @ np.abs(V0[c]) + np.abs(W0[c, :ntot]))  # tests/test_gpu_many_products.py: both sides gamma_p
                assert (np.abs(out[c, :ntot] - w.cpu().numpy()) <= bound).all(), (nrhs, c)
            # solve!(kkt, W) with block products on, then off again: the columns of solve!(kkt, w), to the tolerance
            # tests/test_gpu_julia_many.py holds the matrix method to
            P = rng.standard_normal((nrhs, ntot))
            for on in (True, False):
                block_products(ccall, kkt, on)
                X = solve_matrix_kkt(ccall, kkt, t(P)).cpu().numpy()
                for c in range(nrhs):
                    ref = kkt.solve(t(P[c])).cpu().numpy()
                    assert np.max(np.abs(X[c] - ref)) < 1e-10 * np.max(np.abs(ref)), (nrhs, on, c)
    finally:
        kkt.close()


@pytest.mark.parametrize("glue,kind", [("MadQPHIP", "HIPKKTSystem"), ("MadQPHIPSparse", "HIPSparseKKTSystem")])
def test_the_glue_passes_the_blocks_as_the_replay_does(glue, kind):
    src = open(os.path.join(ROOT, "julia", glue + ".jl")).read()
    call = re.search(r"function mul!\(W::AbstractMatrix, kkt::" + kind + r", V::AbstractMatrix, alpha = 1\.0, beta = 0\.0\)\s*\n"
                     r"\s*check\(kkt\.ctx, ccall\(\(:madqp_kkt_mul_many, libmadqp\), Int32,\s*\n([^\n]*)\n([^\n]*)\)\)", src)
    assert call, glue
    assert "(Ptr{Cvoid}, Ref{CState}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64)" in call.group(1)
    assert "kkt.handle, kkt.cstate, dptr(W), size(W, 1), dptr(V), size(V, 1), size(W, 2), alpha, beta" in call.group(2)
    sw = re.search(r"function block_products!\(kkt::" + kind + r", on::Bool\)\s*\n\s*check\(kkt\.ctx, ccall\(\(:madqp_kkt_set_block_products, "
                   r"libmadqp\), Int32, \(Ptr\{Cvoid\}, Int32\), kkt\.handle, Int32\(on\)\)\)", src)
    assert sw, glue
