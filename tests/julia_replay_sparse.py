"""Replay of julia/MadQPHIPSparse.jl through the C ABI (test infrastructure; see tests/julia_replay.py for the why).

``ReplaySparseKKTSystem`` has one method per Julia method of ``HIPSparseKKTSystem`` (``!`` dropped), each issuing exactly
the ccall sequence of the glue: the two sparsity patterns become CSR structures on the device once
(``madqp_csr_map_create`` / ``_pattern``: A by rows, A by columns, the full symmetric H), the KKT object borrows them
(``madqp_kkt_create_sparse`` with H = NULL, ``madqp_kkt_set_hcsr``), and ``compress_jacobian!`` / ``compress_hessian!``
are ``madqp_csr_map_apply`` from the nnz-long callback buffers.  No tensor of nx * m or nx * nx elements exists here.

The symbols this replay touches are recorded in ``SPARSE_ENTRY_POINTS`` -- a set of its own: ``JR.GLUE_ENTRY_POINTS`` is
compared with the ccall targets of julia/MadQPHIP.jl (tests/test_gpu_julia_replay.py), which bind none of the new ones, so
no new symbol name ever passes through ``JR.ccall``.  The linear solver is MadQPHIP.jl's (``JR.ReplayCholeskySolver``)."""
import ctypes as C
import os

import numpy as np
import torch

import julia_replay as JR
import madqp_jl_amd as M
from madqp_jl_amd._lib import CSR_KINDS, CState, ptr

SPARSE_ENTRY_POINTS = set()  # every ABI symbol the methods of MadQPHIPSparse.jl (as replayed here) touched


def ccall(be, name, *args):
    """``check(ctx, ccall((name, libmadqp), Int32, ...))`` of the sparse glue."""
    SPARSE_ENTRY_POINTS.add(name)
    rc = getattr(be.lib, name)(*args)
    if rc < 0:
        be._ck(rc)
    if rc > 0:
        raise M.SolveException()
    return rc


class ReplayCSRMap:
    """``csr_map(ctx, I, J, nrows, ncols, kind)`` of the glue: create, then ask for the pattern."""

    def __init__(self, be, I, J, nrows, ncols, kind):
        self.be = be
        h = C.c_void_p()
        ccall(be, "madqp_csr_map_create", be.ctx, len(I), I.ctypes.data_as(C.c_void_p), J.ctypes.data_as(C.c_void_p),
              nrows, ncols, CSR_KINDS.index(kind), C.byref(h))
        rows, stored, p, c = C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p()
        ccall(be, "madqp_csr_map_pattern", h, C.byref(rows), C.byref(stored), C.byref(p), C.byref(c))
        self.handle, self.stored, self.ptr, self.col = h, stored.value, p, c

    def destroy(self):
        self.be.lib.madqp_csr_map_destroy(self.handle)


class ReplaySparseKKTSystem:
    """HIPSparseKKTSystem{..., F} of the glue, F in ("condensed", "augmented", "normal")."""

    MODES = {"condensed": 0, "normal": 1, "augmented": 2}

    def __init__(self, be, form, nx, m, ind_ineq, ind_lb, ind_ub, jac_I, jac_J, hess_I, hess_J):
        """``_create`` of the glue (create_kkt_system): patterns are 1-based int32 host arrays, as MadNLP keeps them."""
        self.be, self.form, self.nx, self.m = be, form, int(nx), int(m)
        dev, f64 = be.device, torch.float64
        self.ns = len(ind_ineq)
        self.n = self.nx + self.ns
        z = lambda k: torch.zeros(max(int(k), 1), dtype=f64, device=dev)[: int(k)]
        nnzj, nnzh = len(jac_I), len(hess_I)
        if form == "normal" and nnzh > 0:
            raise ValueError("The KKT system NormalKKTSystem supports only linear programs.")
        jI, jJ = np.ascontiguousarray(jac_I, dtype=np.int32), np.ascontiguousarray(jac_J, dtype=np.int32)
        hI, hJ = np.ascontiguousarray(hess_I, dtype=np.int32), np.ascontiguousarray(hess_J, dtype=np.int32)
        self.jac_map = ReplayCSRMap(be, jI, jJ, self.m, self.nx, "rows")
        self.jact_map = ReplayCSRMap(be, jI, jJ, self.m, self.nx, "cols")
        self.hess_map = ReplayCSRMap(be, hI, hJ, self.nx, self.nx, "sym") if nnzh else None
        # VT(undef, k): whatever the allocator hands out -- NaN here, so that an entry apply does not write shows
        und = lambda k: torch.full((max(int(k), 1),), float("nan"), dtype=f64, device=dev)[: int(k)]
        self.a_val, self.at_val = und(self.jac_map.stored), und(self.jact_map.stored)
        self.h_val = und(self.hess_map.stored) if nnzh else None
        self.jac, self.hess = z(nnzj), z(nnzh)
        ineq0 = (C.c_int64 * max(self.ns, 1))(*[int(i) for i in ind_ineq])
        h = C.c_void_p()
        ccall(be, "madqp_kkt_create_sparse", be.ctx, self.MODES[form], self.nx, self.m, self.ns, ineq0, None,
              max(self.nx, 1), self.jac_map.ptr, self.jac_map.col, ptr(self.a_val), self.jact_map.ptr, self.jact_map.col,
              ptr(self.at_val), C.byref(h))
        if nnzh:
            ccall(be, "madqp_kkt_set_hcsr", h, self.hess_map.ptr, self.hess_map.col, ptr(self.h_val))
        self.handle = h
        ccall(be, "madqp_kkt_set_refine", h, int(os.environ.get("MADQP_KKT_REFINE", "-1")))
        self.linear_solver = JR.ReplayCholeskySolver(be, h)  # linear_solver(aug_com; opt = opt_linear_solver)
        n, m = self.n, self.m
        self.ind_lb0 = torch.as_tensor(ind_lb, dtype=torch.int64, device=dev).contiguous()
        self.ind_ub0 = torch.as_tensor(ind_ub, dtype=torch.int64, device=dev).contiguous()
        nlb, nub = self.ind_lb0.numel(), self.ind_ub0.numel()
        self.reg, self.pr_diag, self.du_diag = z(n), z(n), z(m)
        self.l_diag, self.u_diag, self.l_lower, self.u_lower = z(nlb), z(nub), z(nlb), z(nub)
        cs = CState()  # the KKT's own view: solver-level pointers stay NULL
        cs.n, cs.m, cs.nlb, cs.nub = n, m, nlb, nub
        cs.ind_lb, cs.ind_ub = ptr(self.ind_lb0), ptr(self.ind_ub0)
        for k in ("reg", "pr_diag", "du_diag", "l_diag", "l_lower", "u_diag", "u_lower"):
            setattr(cs, k, ptr(getattr(self, k)))
        self.cstate = cs
        self.n_factorizations = 0

    def close(self):  # the finalizers of aug_com: the KKT object, and the maps it borrows from
        if self.handle is not None:
            self.be.lib.madqp_kkt_destroy(self.handle)
            for mp in (self.jac_map, self.jact_map, self.hess_map):
                if mp is not None:
                    mp.destroy()
            self.handle = None

    def largest_tensor(self):
        """Elements of the largest tensor this object holds (nothing of nx * m or nx * nx may be among them)."""
        return max(t.numel() for t in vars(self).values() if torch.is_tensor(t))

    def num_variables(self):
        return self.n

    def get_jacobian(self):  # the nnzj buffer the SparseCallback fills
        return self.jac

    def get_hessian(self):
        return self.hess

    def initialize(self):  # MadNLP.initialize!(kkt)
        ccall(self.be, "madqp_kkt_initialize", self.handle, C.byref(self.cstate))

    def set_aug_diagonal_reg(self, del_w, del_c):  # MadIPM.set_aug_diagonal_reg!(kkt, solver): state(solver)
        ccall(self.be, "madqp_kkt_set_aug_diagonal_reg", self.handle, C.byref(self.solver_state.cstruct), del_w, del_c)

    def compress_jacobian(self):  # two applies: the values of A and of A'
        ccall(self.be, "madqp_csr_map_apply", self.jac_map.handle, ptr(self.jac), ptr(self.a_val))
        ccall(self.be, "madqp_csr_map_apply", self.jact_map.handle, ptr(self.jac), ptr(self.at_val))

    def compress_hessian(self):
        if self.hess_map is not None:
            ccall(self.be, "madqp_csr_map_apply", self.hess_map.handle, ptr(self.hess), ptr(self.h_val))

    def jtprod(self, out, y):
        ccall(self.be, "madqp_kkt_jtprod", self.handle, ptr(out), ptr(y))

    def build_kkt(self):
        ccall(self.be, "madqp_kkt_build", self.handle, C.byref(self.cstate))

    def factorize_wrapper(self):  # MadNLP.factorize_wrapper! = build_kkt!(kkt); factorize!(kkt.linear_solver)
        self.build_kkt()
        self.linear_solver.factorize()
        self.n_factorizations += 1

    def solve(self, w):
        ccall(self.be, "madqp_kkt_solve", self.handle, C.byref(self.cstate), ptr(w))
        return w

    def mul(self, w, v, alpha=1.0, beta=0.0):
        ccall(self.be, "madqp_kkt_mul", self.handle, C.byref(self.cstate), ptr(w), ptr(v), alpha, beta)
        return w


class ReplaySparseBackend(JR.ReplayBackend):
    """The per-variable kernels MadQPHIPSparse.jl overrides for its own types: the calls of JR.ReplayBackend, recorded
    here as well."""

    def _bound(name):  # noqa: N805
        def call(self, *a, **k):
            SPARSE_ENTRY_POINTS.add("madqp_" + name)
            return getattr(JR.ReplayBackend, name)(self, *a, **k)
        return call

    for _n in ("set_initial_primal_rhs", "set_initial_dual_rhs", "set_predictive_rhs", "set_correction_rhs",
               "get_correction", "set_extra_correction", "get_complementarity_measure",
               "get_affine_complementarity_measure", "get_alpha_max"):
        locals()[_n] = _bound(_n)
    del _n, _bound


def model_patterns(A, H, rng, duplicates=3):
    """The two patterns as a model reports them (``JR.coo_pattern``): the Jacobian, and the lower triangle of H."""
    jac = JR.coo_pattern(A, rng, duplicates)
    if H is not None:
        hess = JR.coo_pattern(np.tril(H), rng, duplicates)  # MadNLP's Hessians are lower triangular
    else:
        hess = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    return jac, hess


class ReplaySparseMPCSolver(JR.ReplayMPCSolver):
    """MadIPM.MPCSolver with ``kkt_system = MadQPHIPSparse.HIPSparse*KKTSystem, linear_solver = MadQPHIP.HIPCholeskySolver``.
    The model stays dense behind the COO interface, as in the dense replay."""

    def _create_kkt_system(self):
        A = self.A.detach().cpu().numpy()
        H = None if self.H is None else self.H.detach().cpu().numpy()
        (self._jI, self._jJ, jv), (hI, hJ, hv) = model_patterns(A, H, self._rng)
        st = self.st
        kkt = ReplaySparseKKTSystem(self.be, self.opt.kkt_system, self.nx, self.m, self.ind_ineq, st.ind_lb.cpu().numpy(),
                                    st.ind_ub.cpu().numpy(), self._jI, self._jJ, hI, hJ)
        st.adopt(kkt)
        # eval_jac_wrapper! / eval_lag_hess_wrapper! (src/solver.jl:167,170): the callback fills the buffers, then
        # compress_*! moves them into the CSR operands (QP: constant, evaluated once)
        kkt.get_jacobian().copy_(torch.as_tensor(jv, device=self.be.device))
        kkt.compress_jacobian()
        if len(hv):
            kkt.get_hessian().copy_(torch.as_tensor(hv, device=self.be.device))
            kkt.compress_hessian()
        kkt.eval_model = self._eval_model
        return kkt
