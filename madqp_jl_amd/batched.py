"""Lock-step solver for a batch of small, equally shaped QPs (BASELINE configs[3]; csrc/batch.hip).

All problems share (nx, m).  By default they also share the pattern of finite bounds / equality rows; with
``per_problem_patterns=True`` every problem has its own (``pack_patterns``: CSR index lists, the slack part of the
stacked arrays padded to the largest number of slacks, ``madqp_batch_create_patterns``).  The one-off set-up of
``MPCSolver.initialize`` (src/solver.jl:127-159: bounds, interior push, scaling) runs here as
elementwise torch ops over the stacked arrays; from ``madqp_batch_init`` on everything happens in
``libmadqp_hip.so``: a handful of launches per iteration for the whole batch, per-problem scalars on
the device, a finished problem masked out by its status word.  Across GPUs the batch is sharded by
``batch.shard`` (problem b -> rank b mod N, no communication).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import BATCH_SCALARS, BATCH_TRACE, CBatchData, ptr
from .options import IPMOptions
from .solver import _push_interior, get_index_constraints, native_options


def pack_patterns(lvar, uvar, lcon, ucon, fixed_variable_treatment="relax_bound"):
    """Per-problem index lists of a batch (host, numpy; ``lvar``, ``uvar``: [B][nx], ``lcon``, ``ucon``: [B][m]):
    ``get_index_constraints`` of every problem, concatenated in CSR form -- problem b's ind_ineq is
    ``ind_ineq[ineq_ptr[b]:ineq_ptr[b+1]]``, likewise ind_lb / ind_ub (indices into its own n_b = nx + ns_b variables).
    ``gather`` / ``mask`` ([B][ns_max]): slack k of problem b belongs to row ``gather[b, k]`` where ``mask[b, k]``; the
    padding (mask False) points at row 0."""
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (lvar, uvar, lcon, ucon))
    B = lvar.shape[0]
    ics = [get_index_constraints(lvar[b], uvar[b], lcon[b], ucon[b], fixed_variable_treatment) for b in range(B)]
    csr = lambda key: (np.concatenate([[0], np.cumsum([len(ic[key]) for ic in ics])]).astype(np.int64),
                       np.concatenate([np.asarray(ic[key], dtype=np.int64) for ic in ics] + [np.zeros(0, np.int64)]))
    ineq_ptr, ind_ineq = csr("ind_ineq")
    lb_ptr, ind_lb = csr("ind_lb")
    ub_ptr, ind_ub = csr("ind_ub")
    ns = np.diff(ineq_ptr)
    ns_max = int(ns.max()) if B else 0
    mask = np.arange(ns_max)[None, :] < ns[:, None]
    gather = np.zeros((B, ns_max), dtype=np.int64)
    gather[mask] = ind_ineq
    return dict(ineq_ptr=ineq_ptr, ind_ineq=ind_ineq, lb_ptr=lb_ptr, ind_lb=ind_lb, ub_ptr=ub_ptr, ind_ub=ind_ub,
                ns=ns, ns_max=ns_max, gather=gather, mask=mask, any_eq=bool((ns < lcon.shape[1]).any()))


class BatchedMPCSolver:
    """``qps``: list of :class:`DeviceQP` with identical shapes and -- unless ``per_problem_patterns`` -- identical bound
    patterns (which variables have a finite lower / upper bound, which rows are equalities).

    ``trace``: ``True`` records every iteration of every problem on the device (``max_iter + 1`` records per problem), a
    positive ``int`` the first that many, ``False`` (default) none -- the library is then called exactly as without the
    keyword.  ``refine_steps`` (an :class:`IPMOptions` field): steps of iterative refinement in every solve, as in
    :class:`MPCSolver`; ``None`` means 0 here (the AUTO rule is ``MPCSolver``'s).

    ``shared_matrices=True``: the parametric batch -- one model, many right-hand sides.  Every problem's ``A`` (and ``H``,
    unless all are LPs) must be the SAME tensor (equal ``data_ptr()``, shape and strides); ``q``, the bounds and the row
    bounds are per problem.  Nothing of size ``B * nx * nx`` or ``B * m * nx`` is then made: ``A`` is scaled once, ``H`` stays
    as the caller holds it and the library multiplies each entry by the problem's ``obj_scale`` as it reads it
    (``madqp_batch_share_matrices``) -- the very product the stacked form stores, so the results are bitwise the same."""

    def __init__(self, qps, backend, per_problem_patterns=False, trace=False, shared_matrices=False, **opts):
        if not qps:
            raise ValueError("empty batch")
        if trace is not True and trace is not False:
            if isinstance(trace, bool) or not isinstance(trace, (int, np.integer)) or trace < 1:
                raise ValueError("trace: True, False or a positive number of records per problem")
        self._trace = trace if isinstance(trace, bool) else int(trace)
        self.be, self.qps = backend, list(qps)
        self.per_problem = bool(per_problem_patterns)
        self.shared = bool(shared_matrices)
        if any((q.nvar, q.ncon) != (qps[0].nvar, qps[0].ncon) for q in self.qps):
            raise ValueError("all problems of a batch must have the same (nx, m)")
        self.opt = IPMOptions(**opts)
        if self.opt.refine_steps is not None and int(self.opt.refine_steps) < 0:
            raise ValueError("refine_steps must be >= 0 (None: 0 for the batched engine)")
        if self.opt.kkt_system not in ("condensed", "normal") or self.opt.check_residual:
            raise ValueError("the batched driver supports the condensed KKT system and the normal equations, on one GPU")
        if self.opt.kkt_bandwidth is not None:
            raise ValueError("kkt_bandwidth: the batched engine factorises dense matrices (band-limited assembly and "
                             "Cholesky belong to MPCSolver's sparse front end)")
        if self.opt.kkt_storage != "dense":
            raise ValueError("kkt_storage: the batched engine factorises dense matrices (packed band storage belongs to "
                             "MPCSolver's sparse front end)")
        self.normal = self.opt.kkt_system == "normal"
        q0 = self.qps[0]
        self.B, self.nx, self.m = len(self.qps), q0.nvar, q0.ncon
        dev = backend.device
        st = lambda name: torch.stack([getattr(q, name) for q in self.qps]).contiguous()
        self.lvar, self.uvar, self.lcon, self.ucon = st("lvar"), st("uvar"), st("lcon"), st("ucon")
        host = lambda t: t.detach().cpu().numpy()
        fvt = self.opt.fixed_variable_treatment or "relax_bound"
        if self.per_problem:
            self.pat = pack_patterns(host(self.lvar), host(self.uvar), host(self.lcon), host(self.ucon), fvt)
            has_eq = self.pat["any_eq"]
            self.ns = self.pat["ns_max"]
        else:
            self.pat = None
            ic = get_index_constraints(host(self.lvar[0]), host(self.uvar[0]), host(self.lcon[0]), host(self.ucon[0]), fvt)
            same = lambda a: bool((torch.isfinite(a) == torch.isfinite(a[0])).all())
            if not (same(self.lvar) and same(self.uvar) and same(self.lcon) and same(self.ucon)
                    and bool(((self.lcon == self.ucon) == (self.lcon[0] == self.ucon[0])).all())):
                raise ValueError("all problems of a batch must share the pattern of finite bounds and equality rows "
                                 "(per_problem_patterns=True lifts this)")
            self.ind_ineq, self.ind_eq = ic["ind_ineq"], ic["ind_eq"]
            has_eq = len(self.ind_eq) > 0
            self.ns = len(self.ind_ineq)
            self.ind_lb = torch.as_tensor(ic["ind_lb"], dtype=torch.int64, device=dev)
            self.ind_ub = torch.as_tensor(ic["ind_ub"], dtype=torch.int64, device=dev)
            self.nlb, self.nub = self.ind_lb.numel(), self.ind_ub.numel()
        if any(q.H is not None and (not torch.is_tensor(q.H) or q.H.dim() != 2) for q in self.qps) or any(not torch.is_tensor(q.A) for q in self.qps):
            raise ValueError("the batched driver takes dense H and dense A")
        if any((q.H is None) != (q0.H is None) for q in self.qps):
            raise ValueError("all problems of a batch must be QPs or all LPs")
        self.n = self.nx + self.ns  # per_problem_patterns: n_max, the stride of x, xl, xu, zl, zu
        reg = self.opt.regularization
        self._copt = native_options(self.opt)
        self._copt.kkt_form = 1 if self.normal else 0
        if self.normal and q0.H is not None:
            raise ValueError("The KKT system NormalKKTSystem supports only linear programs.")  # normalkkt.jl:45-48
        if not self.normal and has_eq and not (self._copt.regularization != 0 and reg.delta_d < 0.0):
            raise ValueError("the condensed KKT system needs dual regularization delta_d < 0 "
                             "when the problem has equality constraints")
        if self.shared:
            for name in ("A",) if q0.H is None else ("H", "A"):
                t0 = getattr(q0, name)
                for i, q in enumerate(self.qps):
                    t = getattr(q, name)
                    if (t.data_ptr(), t.shape, t.stride()) != (t0.data_ptr(), t0.shape, t0.stride()):
                        raise ValueError(f"shared_matrices: problem {i} has a {name} of its own (every problem must hold "
                                         f"the same tensor: equal data_ptr(), shape and strides)")
            self.H = None if q0.H is None else q0.H.unsqueeze(0)  # [1, ...] views of the caller's tensors
            self.A, self.q = q0.A.unsqueeze(0), st("q")
        else:
            self.H = None if q0.H is None else st("H")
            self.A, self.q = st("A"), st("q")
        self.c0 = torch.as_tensor([q.c0 for q in self.qps], dtype=torch.float64, device=dev)
        self.x0, self.y0 = st("x0"), st("y0")
        self._h = None
        self.status = self.iters = self.scalars = None
        self.pre_create_hook = None  # called with the solver after the torch set-up, before the library sees the arrays

    # ---- src/solver.jl:127-159, vectorised over the batch ----
    def initialize(self):
        opt, be, dev = self.opt, self.be, self.be.device
        B, nx, n, m = self.B, self.nx, self.n, self.m
        f64 = dict(dtype=torch.float64, device=dev)
        one = torch.ones((), **f64)
        x = torch.zeros((B, n), **f64)
        x[:, :nx] = self.x0
        y = self.y0.clone()
        if self.pat is None:
            ineq = torch.as_tensor(self.ind_ineq, dtype=torch.int64, device=dev)
            rows = lambda a, pad: a[:, ineq]
        else:  # slack k of problem b: row gather[b, k]; the padding gets -inf / +inf bounds, scale 1 (and x = 0)
            gather = torch.as_tensor(self.pat["gather"], device=dev)
            mask = torch.as_tensor(self.pat["mask"], device=dev)
            rows = lambda a, pad: torch.where(mask, a.gather(1, gather), torch.full_like(gather, pad, dtype=a.dtype))
        xl = torch.cat([self.lvar, rows(self.lcon, -np.inf)], dim=1)
        xu = torch.cat([self.uvar, rows(self.ucon, np.inf)], dim=1)
        rhs = torch.where(self.lcon == self.ucon, self.lcon, torch.zeros_like(self.lcon))
        tol = opt.bound_relax_factor
        xl = torch.where(torch.isfinite(xl), xl - torch.maximum(one, xl.abs()) * tol, xl)
        xu = torch.where(torch.isfinite(xu), xu + torch.maximum(one, xu.abs()) * tol, xu)
        x = _push_interior(x, xl, xu, opt.bound_push, opt.bound_fac)
        H, A, q = self.H, self.A, self.q
        self.obj_scale = torch.ones(B, **f64)
        self.con_scale = torch.ones((B, m), **f64)
        self.h_scale = None  # shared H: the per-problem factor the library applies as it reads H (None: 1)
        if opt.scaling and (m or nx):  # MadNLP.set_scaling!(..., 100)
            if m and nx:  # (shared A: one row of scales, the same for every problem)
                self.con_scale = torch.minimum(one, 100.0 / A.abs().amax(dim=2)).expand(B, m).contiguous()
            g = q.clone()
            if H is not None and nx:
                step = max(1, (1 << 27) // max(nx * nx, 1))  # bounded temporaries
                Hb = H.expand(B, nx, nx)  # (shared H: a view -- the temporaries below have the stacked form's shape and layout)
                for b0 in range(0, B, step):
                    g[b0:b0 + step] += (Hb[b0:b0 + step] * x[b0:b0 + step, None, :nx]).sum(dim=2)
            gmax = g.abs().amax(dim=1) if nx else torch.zeros(B, **f64)
            self.obj_scale = torch.where(gmax > 0, torch.minimum(one, 100.0 / gmax), one)
            cs = self.con_scale
            y = y / cs
            rhs = rhs * cs
            cs_s = rows(cs, 1.0)
            x[:, nx:] *= cs_s
            xl[:, nx:] *= cs_s
            xu[:, nx:] *= cs_s
            A = (cs[:A.shape[0], :, None] * A).contiguous()  # (shared A: scaled once)
            if self.shared and H is not None:
                self.h_scale = self.obj_scale.contiguous()  # H itself stays unscaled: fl(obj_scale[b] * H[i][j]) on load
            elif H is not None:
                H = (self.obj_scale[:, None, None] * H).contiguous()
            q = self.obj_scale[:, None] * q
        self._H, self._A, self._q = None if H is None else H.contiguous(), A.contiguous(), q.contiguous()
        self._rhs, self._c0 = rhs.contiguous(), (self.obj_scale * self.c0).contiguous()
        self.x, self.xl, self.xu, self.y = x.contiguous(), xl.contiguous(), xu.contiguous(), y.contiguous()
        self.zl, self.zu = torch.zeros((B, n), **f64), torch.zeros((B, n), **f64)
        self.close()
        data = CBatchData(H=ptr(self._H), A=ptr(self._A), q=ptr(self._q), rhs=ptr(self._rhs), c0=ptr(self._c0),
                          x=ptr(self.x), xl=ptr(self.xl), xu=ptr(self.xu), zl=ptr(self.zl), zu=ptr(self.zu),
                          y=ptr(self.y))
        self._data = data
        if self.pre_create_hook is not None:
            self.pre_create_hook(self)
        h = C.c_void_p()
        if self.pat is None:
            ineq_host = (C.c_int64 * max(1, self.ns))(*[int(i) for i in self.ind_ineq])
            be._ck(be.lib.madqp_batch_create(be.ctx, B, nx, m, self.ns, ineq_host, self.nlb, ptr(self.ind_lb),
                                             self.nub, ptr(self.ind_ub), C.byref(data), C.byref(self._copt),
                                             C.byref(h)))
        else:
            arr = {k: np.ascontiguousarray(self.pat[k], dtype=np.int64)
                   for k in ("ineq_ptr", "ind_ineq", "lb_ptr", "ind_lb", "ub_ptr", "ind_ub")}
            p64 = lambda k: arr[k].ctypes.data_as(C.POINTER(C.c_int64)) if arr[k].size else None
            be._ck(be.lib.madqp_batch_create_patterns(be.ctx, B, nx, m, p64("ineq_ptr"), p64("ind_ineq"), p64("lb_ptr"),
                                                      p64("ind_lb"), p64("ub_ptr"), p64("ind_ub"), C.byref(data),
                                                      C.byref(self._copt), C.byref(h)))
        self._h = h
        if self.shared:
            be._ck(be.lib.madqp_batch_share_matrices(h, int(self._H is not None), 1, ptr(self.h_scale)))
        self.trace_capacity = 0
        if self._trace is not False:
            cap = opt.max_iter + 1 if self._trace is True else self._trace
            be._ck(be.lib.madqp_batch_set_trace(h, cap))
            self.trace_capacity = cap
        be._ck(be.lib.madqp_batch_init(h, opt.mu_init, opt.bound_fac))

    def iterate(self, max_steps=None, check_every=1) -> int:
        """Advance every active problem by up to ``max_steps`` iterations; returns how many are still active."""
        n = C.c_int32()
        steps = self.opt.max_iter + 1 if max_steps is None else int(max_steps)
        self.be._ck(self.be.lib.madqp_batch_iterate(self._h, steps, int(check_every), C.byref(n)))
        return n.value

    def fetch(self):
        B = self.B
        status = (C.c_int32 * B)()
        iters = (C.c_int32 * B)()
        scal = (C.c_double * (B * len(BATCH_SCALARS)))()
        self.be._ck(self.be.lib.madqp_batch_results(self._h, status, iters, scal))
        self.status = np.frombuffer(status, dtype=np.int32).copy()
        self.iters = np.frombuffer(iters, dtype=np.int32).copy()
        self.scalars = np.frombuffer(scal, dtype=np.float64).reshape(B, len(BATCH_SCALARS)).copy()
        return self.status, self.iters, self.scalars

    def fetch_trace(self):
        """``(records, count)``: the device's trace buffer, [B][capacity][len(BATCH_TRACE)] (``_lib.BATCH_TRACE`` names the
        columns; ``obj`` still scaled), and how many records of each problem are stored."""
        if not self.trace_capacity:
            raise ValueError("the solver was made without trace=")
        B, cap, L = self.B, self.trace_capacity, len(BATCH_TRACE)
        buf = np.empty((B, cap, L), dtype=np.float64)
        count = np.empty(B, dtype=np.int32)
        self.be._ck(self.be.lib.madqp_batch_trace(self._h, buf.ctypes.data_as(C.POINTER(C.c_double)),
                                                  count.ctypes.data_as(C.POINTER(C.c_int32))))
        return buf, count

    def solve(self, check_every=1):
        """Returns one result dict per problem (same keys as :meth:`MPCSolver.result`; ``trace`` -- one record per
        iteration, the keys of ``MPCSolver.record`` plus ``residual_ratio`` -- when the solver was made with ``trace=``)."""
        self.initialize()
        self.iterate(check_every=check_every)
        return self.results()

    def results(self):
        """One dict per problem.  The unscaling runs on the device over the whole batch and the four arrays come back in
        one copy each; the dicts hold row views (1024 problems: 2 ms instead of 8 for a per-problem numpy loop)."""
        status, iters, scal = self.fetch()
        nx, os_ = self.nx, self.obj_scale[:, None]
        h = lambda t: t.contiguous().cpu().numpy()
        x = h(self.x[:, :nx])
        y = h(self.y * self.con_scale / os_)
        zl, zu = h(self.zl[:, :nx] / os_), h(self.zu[:, :nx] / os_)
        obj = scal[:, BATCH_SCALARS.index("obj")] / h(self.obj_scale)
        col = {k: i for i, k in enumerate(BATCH_SCALARS)}
        c_pr, c_du, c_co, c_mu, c_dw, c_nf = (col[k] for k in ("inf_pr", "inf_du", "inf_compl", "mu", "del_w",
                                                                 "n_factorizations"))
        st, it, nf = status.tolist(), iters.tolist(), scal[:, c_nf].astype(np.int64).tolist()
        out = [dict(status=st[b], iter=it[b], objective=obj[b], solution=x[b], multipliers=y[b],
                    multipliers_L=zl[b], multipliers_U=zu[b], inf_pr=scal[b, c_pr], inf_du=scal[b, c_du],
                    inf_compl=scal[b, c_co], mu=scal[b, c_mu], del_w=scal[b, c_dw], n_factorizations=nf[b])
               for b in range(self.B)]
        if self.trace_capacity:
            buf, count = self.fetch_trace()
            buf[:, :, BATCH_TRACE.index("obj")] /= h(self.obj_scale)[:, None]
            for b, r in enumerate(out):  # (only the stored records become Python objects: the buffer has max_iter + 1 slots)
                r["trace"] = [dict(zip(BATCH_TRACE, rec), k=k) for k, rec in enumerate(buf[b, :count[b]].tolist())]
        return out

    def close(self):
        if self._h is not None:
            self.be.lib.madqp_batch_destroy(self._h)
            self._h = None
