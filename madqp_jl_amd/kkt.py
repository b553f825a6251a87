"""Host-side mirror of the MadNLP plugin surface for the MI355X path.

``HIPCondensedKKTSystem`` plays the role of ``NormalKKTSystem <:
MadNLP.AbstractKKTSystem`` (src/KKT/normalkkt.jl) and ``HIPCholeskySolver`` that
of the ``MadNLP.AbstractLinearSolver`` it owns (``MadNLP.LapackCPUSolver`` in
test/runtests.jl:151).  Method names follow the reference's generic functions
(``build_kkt!`` -> ``build_kkt`` ...); all arithmetic happens in
``libmadqp_hip.so``.  The Julia glue that binds the same C ABI is
``julia/MadQPHIP.jl``.
"""
from __future__ import annotations

import numpy as np

from .backend import State
from .qp import DeviceSymCSR


def pattern_bandwidth(A, H=None, form="condensed") -> int:
    """Half-bandwidth of the matrix the sparse front end factorises, from the patterns alone (host, numpy): the number
    ``madqp_kkt_set_bandwidth`` checks its argument against.  ``A``: :class:`DeviceCSR`; ``H``: None, a 1-D tensor
    (diagonal) or a :class:`DeviceSymCSR`; ``form``: "condensed" (``H + Sigma_x + A' Theta A``: two variables meet where a
    row of A holds both) or "normal" (``A Sigma^-1 A'``: two rows meet where a column of A holds both)."""
    if form not in ("condensed", "normal"):
        raise ValueError(f"a bandwidth is defined for the condensed and the normal form, not {form!r}")
    host = lambda t: t.detach().cpu().numpy()
    ptr, col = (host(A.ptr), host(A.col)) if form == "condensed" else (host(A.t_ptr), host(A.t_col))
    bw = 0
    rows = np.flatnonzero(np.diff(ptr) > 0)  # (column indices ascend within a row)
    if len(rows):
        bw = int(np.max(col[ptr[rows + 1] - 1] - col[ptr[rows]]))
    if isinstance(H, DeviceSymCSR) and H.nnz:
        if form == "normal":
            raise ValueError("The KKT system NormalKKTSystem supports only linear programs "
                             "(or a diagonal Hessian given as a vector).")
        bw = max(bw, int(np.max(np.abs(host(H.col) - host(H.row)))))
    return bw


KKT_STORAGES = ("dense", "packed")


def check_storage(storage, bandwidth, band_form="condensed", H=None):
    """The refusals of ``storage=`` / ``kkt_storage``, before any device call: packed storage is laid out for one
    bandwidth, which the object therefore needs at construction, on the forms that take one."""
    if storage not in KKT_STORAGES:
        raise ValueError(f"storage: one of {KKT_STORAGES}, not {storage!r}")
    if storage == "packed":
        if bandwidth is None:
            raise ValueError("storage='packed' needs a bandwidth at construction: the object never allocates the dense K")
        if band_form is None:
            raise ValueError("storage='packed' is taken by the sparse condensed and normal KKT systems only")
        if H is not None and not isinstance(H, DeviceSymCSR) and H.dim() == 2:
            raise ValueError("storage='packed' needs a sparse (DeviceSymCSR), diagonal or absent Hessian, not a dense one")


GRID_REFUSAL = ("solves with a block of right-hand sides are not available on a grid of GPUs "
                "(madqp_dist_* / madqp_dkkt_* take one vector): loop over solve()")


def check_rhs_block(W, length, device, what="W"):
    """The refusals of a block of right-hand sides, before any device call: a contiguous 2-D float64 tensor on the
    backend's device, one right-hand side per row, rows of at least ``length`` entries.  Returns the number of rows."""
    import torch

    if not isinstance(W, torch.Tensor) or W.dim() != 2:
        raise ValueError(f"{what}: a 2-D tensor (nrhs, >= {length}), one right-hand side per row")
    if W.dtype != torch.float64:
        raise ValueError(f"{what}: float64, not {W.dtype}")
    if W.device != torch.device(device):
        raise ValueError(f"{what}: on {torch.device(device)}, not {W.device}")
    if W.shape[1] < length:
        raise ValueError(f"{what}: rows of at least {length} entries, not {W.shape[1]}")
    if not W.is_contiguous():
        raise ValueError(f"{what}: contiguous (row c = right-hand side c at stride shape[1]), strides {tuple(W.stride())}")
    return W.shape[0]


class HIPCholeskySolver:
    """AbstractLinearSolver contract: ctor keeps the matrix it re-reads at every
    ``factorize`` (src/KKT/normalkkt.jl:99-101); ``solve`` is in place (:196)."""

    def __init__(self, backend, kkt_handle, bandwidth=None):
        """``bandwidth``: half-bandwidth of the matrix (sparse condensed / normal KKT objects only): assembly and
        factorisation are band-limited from here on (``madqp_kkt_set_bandwidth``).  None: the dense schedules."""
        self.be, self._kkt = backend, kkt_handle
        self.info = 0
        self.bandwidth = None
        self.sweep_band_blocks = None  # 128-blocks a block row of the sweeps reads left of the diagonal; None: all (dense)
        if bandwidth is not None:
            backend.kkt_set_bandwidth(kkt_handle, int(bandwidth))
            self.bandwidth = int(bandwidth)
            kb = backend.chol_sweep_info(backend.kkt_chol(kkt_handle)[0])[0]
            self.sweep_band_blocks = kb if kb >= 0 else None

    def introduce(self) -> str:  # MadNLP.introduce, src/solver.jl:360
        if self.bandwidth is not None:
            return f"madqp-hip blocked left-looking fp64 Cholesky, band-limited (bw = {self.bandwidth}; MFMA, gfx950)"
        return "madqp-hip blocked left-looking fp64 Cholesky (MFMA, gfx950)"

    def factorize(self):  # MadNLP.factorize!
        self.info = self.be.kkt_factorize(self._kkt)
        return self

    def is_factorized(self) -> bool:  # MadIPM.is_factorized, src/utils.jl:54-62
        return self.info == 0

    def solve(self, rhs):
        """MadNLP.solve!(linear_solver, rhs), in place.  ``rhs``: a vector of the matrix's order (``madqp_chol_solve``)
        or a contiguous 2-D float64 tensor ``(nrhs, >= order)``, one right-hand side per row -- LAPACK's column-major
        n x nrhs operand -- solved with one factor (``madqp_chol_solve_many``)."""
        if self._kkt is None:
            raise ValueError(GRID_REFUSAL)
        ch, order = self.be.kkt_chol(self._kkt)
        import torch

        if isinstance(rhs, torch.Tensor) and rhs.dim() == 1:
            if rhs.dtype != torch.float64 or rhs.numel() < order or not rhs.is_contiguous():
                raise ValueError(f"rhs: a contiguous float64 vector of at least {order} entries")
            self.be.chol_solve(ch, rhs)
            return rhs
        check_rhs_block(rhs, order, self.be.device, "rhs")
        if rhs.shape[0]:
            self.be.chol_solve_many(ch, rhs, max(rhs.shape[1], 1))
        return rhs

    def is_inertia(self) -> bool:
        return True

    def inertia(self, n):  # (pos, zero, neg) of the SPD condensed matrix
        return (n, 0, 0) if self.info == 0 else (self.info - 1, 0, 1)


class HIPQuasiDefiniteSolver(HIPCholeskySolver):
    """The same blocked factorisation in quasi-definite mode (``madqp_chol_set_signature``): ``L diag(I, -I) L'`` of
    the augmented matrix, inertia (nx, 0, m) when every pivot has the expected sign."""

    def __init__(self, backend, kkt_handle, nx, m):
        super().__init__(backend, kkt_handle)
        self.nx, self.m = nx, m

    def introduce(self) -> str:
        return "madqp-hip blocked left-looking fp64 L diag(I,-I) L' (quasi-definite, MFMA, gfx950)"

    def inertia(self, n=None):
        return (self.nx, 0, self.m) if self.info == 0 else (0, 1, 0)


class HIPCondensedKKTSystem:
    """Dense condensed KKT system ``K = H + Sigma_x + A' Theta A`` on the device.

    Fields that MadIPM reads generically (``reg, pr_diag, du_diag, l_diag, u_diag,
    l_lower, u_lower, ind_lb, ind_ub, linear_solver``; src/kernels.jl:135-144,
    src/solver.jl:16-18) live in the shared :class:`State` and are exposed as
    attributes.
    """

    def __init__(self, backend, st: State, nx, ind_ineq, H, A):
        """``create_kkt_system`` (src/KKT/normalkkt.jl:29-126).  ``H``: (nx, nx) symmetric
        tensor or None (LP); ``A``: (m, nx) row-major tensor; both are borrowed."""
        self._init_problem(backend, st, nx, ind_ineq)
        self.H, self.A = H, A
        if H is not None:
            assert H.is_contiguous() and H.shape == (nx, nx)
        assert A.is_contiguous() and tuple(A.shape) == (self.m, self.nx)
        self._h = backend.kkt_create(self.nx, self.m, self.ind_ineq, H, max(self.nx, 1), A,
                                     max(self.nx, 1))
        self.linear_solver = HIPCholeskySolver(backend, self._h)

    def _init_problem(self, backend, st, nx, ind_ineq):
        """what every constructor starts from: the backend, the shared state and the sizes it fixes"""
        self.be, self.st = backend, st
        self.nx, self.m = int(nx), st.m
        self.ind_ineq = [int(i) for i in ind_ineq]
        self.ns = len(self.ind_ineq)
        assert st.n == self.nx + self.ns
        self.n_factorizations = 0

    def close(self):
        if self._h is not None:
            self.be.kkt_destroy(self._h)
            self._h = None

    # generic field access, as MadIPM does on any AbstractKKTSystem
    reg = property(lambda s: s.st.reg)
    pr_diag = property(lambda s: s.st.pr_diag)
    du_diag = property(lambda s: s.st.du_diag)
    l_diag = property(lambda s: s.st.l_diag)
    u_diag = property(lambda s: s.st.u_diag)
    l_lower = property(lambda s: s.st.l_lower)
    u_lower = property(lambda s: s.st.u_lower)
    ind_lb = property(lambda s: s.st.ind_lb)
    ind_ub = property(lambda s: s.st.ind_ub)

    def num_variables(self):  # src/KKT/normalkkt.jl:128
        return self.st.n

    def is_inertia_correct(self, num_pos, num_zero, num_neg):  # :132-134
        return num_zero == 0 and num_pos == self.nx

    def initialize(self):  # MadNLP.initialize!(kkt), :136-147
        st, be = self.st, self.be
        for t, v in ((st.reg, 1.0), (st.pr_diag, 1.0), (st.du_diag, 0.0), (st.l_lower, 0.0),
                     (st.u_lower, 0.0), (st.l_diag, 1.0), (st.u_diag, 1.0)):
            be.fill(v, t)

    def set_aug_diagonal_reg(self, del_w, del_c):
        """``set_aug_diagonal_reg!(kkt, solver)`` -- dispatched on the KKT type (src/kernels.jl:128-146; the
        ``ScaledSparseKKTSystem`` method of :149-165 is :class:`HIPScaledAugmentedKKTSystem`)."""
        self.be.set_aug_diagonal_reg(self.st, del_w, del_c)

    def jtprod(self, out, y):  # MadNLP.jtprod!, :162-164
        self.be.kkt_jtprod(self._h, out, y)

    def build_kkt(self):  # MadNLP.build_kkt!, :166-180
        self.be.kkt_build(self._h, self.st)

    def factorize_wrapper(self):
        """MadNLP.factorize_wrapper! = build_kkt! then factorize! (src/linear_solver.jl:10)."""
        self.build_kkt()
        self.linear_solver.factorize()
        self.n_factorizations += 1

    def solve(self, w):  # MadNLP.solve!(kkt, w), :182-205
        self.be.kkt_solve(self._h, self.st, w)
        return w

    def solve_many(self, W):
        """MadNLP.solve!(kkt, w) for every row of ``W`` with one factor (``madqp_kkt_solve_many``): ``W`` is a contiguous
        2-D float64 device tensor ``(nrhs, >= n + m + nlb + nub)``, row c an UnreducedKKTVector.values, solved in place.
        Anything else is refused before a device call.  ``set_refine`` is honoured; ``mul_solved`` afterwards is ``mul``."""
        st = self.st
        nrhs = check_rhs_block(W, st.n + st.m + st.nlb + st.nub, self.be.device)
        if nrhs:
            self.be.kkt_solve_many(self._h, st, W)
        return W

    def set_refine(self, steps):
        """Refinement steps ``solve`` runs itself (``madqp_kkt_set_refine``; -1 = the AUTO rule by order).  For hosts whose
        loop calls ``solve!`` once (MadIPM's ``solve_system!``: what the Julia glue asks for); the drivers of this package
        refine in their own ``solve_system`` (option ``refine_steps``) and leave this at 0."""
        self.be.kkt_set_refine(self._h, steps)

    def mul(self, w, v, alpha=1.0, beta=0.0):  # MadNLP.mul!, :207-219
        self.be.kkt_mul(self._h, self.st, w, v, alpha, beta)
        return w

    def mul_many(self, W, V, alpha=1.0, beta=0.0):
        """``mul`` for every pair of rows of ``W`` and ``V`` (``madqp_kkt_mul_many``): both contiguous 2-D float64 device
        tensors ``(nrhs, >= n + m + nlb + nub)`` as :meth:`solve_many` takes them, row c of ``W`` <- alpha K (row c of ``V``) +
        beta (row c of ``W``).  The products with A, A' and H run once on the block.  Anything else is refused before a
        device call."""
        st = self.st
        ntot = st.n + st.m + st.nlb + st.nub
        nrhs = check_rhs_block(W, ntot, self.be.device)
        if check_rhs_block(V, ntot, self.be.device, "V") != nrhs:
            raise ValueError(f"V: {nrhs} rows as W, not {V.shape[0]}")
        if nrhs and W.data_ptr() == V.data_ptr():
            raise ValueError("W and V: two different blocks")
        if nrhs:
            self.be.kkt_mul_many(self._h, st, W, V, alpha, beta)
        return W

    def set_block_products(self, on):
        """``solve_many`` runs the products with A / A' of its stages, and the residuals of its refinement steps, on the
        block of all right-hand sides (``madqp_kkt_set_block_products``) instead of column by column.  Off by default."""
        self.be.kkt_set_block_products(self._h, bool(on))

    def mul_solved(self, w, v, alpha=1.0, beta=0.0):
        """``mul`` for the residual check of solve_system! (src/linear_solver.jl:26-31): ``v`` is what the last
        ``solve`` returned, unmodified -- the condensed solve's own ``A dx`` is taken instead of a second pass over A
        (``madqp_kkt_mul_solved``: bitwise the result of ``mul``)."""
        self.be.kkt_mul(self._h, self.st, w, v, alpha, beta, solved=True)
        return w

    def eval_model(self, q, rhs, c0) -> float:
        """obj / grad! / cons! callbacks of the loop (src/solver.jl:166-169, 338-340)."""
        return self.be.kkt_eval(self._h, self.st, q, rhs, c0)


class HIPNormalKKTSystem(HIPCondensedKKTSystem):
    """The reference's own ``NormalKKTSystem`` (src/KKT/normalkkt.jl) on the device: normal equations
    ``A Sigma^-1 A'`` (m x m), LP only (:45-48); equality rows need no dual regularization.

    ``At``: (nx, m) tensor, row k = variable k contiguous (a Julia ``m x nx`` matrix as is); borrowed.
    """

    def __init__(self, backend, st: State, nx, ind_ineq, H, At):
        if H is not None:
            raise ValueError("The KKT system NormalKKTSystem supports only linear programs.")  # :45-48
        self._init_problem(backend, st, nx, ind_ineq)
        self.H, self.A, self.At = None, None, At
        assert At.is_contiguous() and tuple(At.shape) == (self.nx, self.m)
        self._h = backend.kkt_create_normal(self.nx, self.m, self.ind_ineq, At, max(self.m, 1))
        self.linear_solver = HIPCholeskySolver(backend, self._h)

    def is_inertia_correct(self, num_pos, num_zero, num_neg):  # src/KKT/normalkkt.jl:132-134
        return num_zero == 0 and num_pos == self.m


class HIPAugmentedKKTSystem(HIPCondensedKKTSystem):
    """The K2 form of MadNLP's default ``SparseKKTSystem`` (src/utils.jl:108; the system the reference's tests
    compare everything against, test/runtests.jl:102-115,165-180) with the slack block eliminated, dense on
    the device: ``[H + Sigma_x, A'; A, -D]`` of order ``ceil128(nx) + m``, factorised as ``L diag(I, -I) L'``
    without pivoting (quasi-definite).  Equality rows enter exactly (``D_i = -dc_i``, which may be 0 when the
    equality rows are linearly independent) -- no ``-1/dc`` weights as in the condensed form.

    ``H``: (nx, nx) tensor, a 1-D tensor (diagonal of H) or None; ``A``: (m, nx) row-major tensor; borrowed.
    """

    def __init__(self, backend, st: State, nx, ind_ineq, H, A):
        self._init_problem(backend, st, nx, ind_ineq)
        self.H, self.A = H, A
        diag = H is not None and H.dim() == 1
        if H is not None:
            assert H.is_contiguous() and tuple(H.shape) in ((nx, nx), (nx,))
        assert A.is_contiguous() and tuple(A.shape) == (self.m, self.nx)
        self._h = backend.kkt_create_augmented(self.nx, self.m, self.ind_ineq, None if diag else H,
                                               max(self.nx, 1), A, max(self.nx, 1))
        if diag:
            backend.kkt_set_hdiag(self._h, H)
        self.linear_solver = HIPQuasiDefiniteSolver(backend, self._h, self.nx, self.m)

    def is_inertia_correct(self, num_pos, num_zero, num_neg):  # src/KKT/normalkkt.jl:132-134, K2 inertia
        return num_zero == 0 and num_neg == self.m


class HIPScaledAugmentedKKTSystem(HIPAugmentedKKTSystem):
    """K2.5: MadNLP's ``ScaledSparseKKTSystem`` (``kkt_system=MadNLP.ScaledSparseKKTSystem`` in test/runtests.jl:95-115)
    on the dense quasi-definite path: the augmented matrix scaled symmetrically by ``sqrt((x - xl)(xu - x))`` per variable
    (scripts/cuda_wrapper.jl:90-116), ``l_diag = x - xl``, ``u_diag = xu - x`` positive (src/kernels.jl:149-165).  Same
    iterates as the K2 form; every entry of the matrix stays bounded as the iterates converge."""

    def __init__(self, backend, st: State, nx, ind_ineq, H, A):
        self._init_problem(backend, st, nx, ind_ineq)
        self.H, self.A = H, A
        if H is not None:
            assert H.is_contiguous() and tuple(H.shape) == (nx, nx)
        assert A.is_contiguous() and tuple(A.shape) == (self.m, self.nx)
        self._h = backend.kkt_create_scaled_augmented(self.nx, self.m, self.ind_ineq, H, max(self.nx, 1), A,
                                                      max(self.nx, 1))
        self.linear_solver = HIPQuasiDefiniteSolver(backend, self._h, self.nx, self.m)

    def initialize(self):  # MadNLP.initialize!(kkt): also the scaling factor (library owned) = 1
        self.be.kkt_initialize(self._h, self.st)

    def set_aug_diagonal_reg(self, del_w, del_c):  # src/kernels.jl:149-165
        self.be.kkt_set_aug_diagonal_reg(self._h, self.st, del_w, del_c)


class _SparseMixin:
    """The Jacobian stays sparse (``DeviceCSR``), the factorised matrix stays dense (SURVEY.md 8f rank 1;
    reference: src/utils.jl:148-298, src/KKT/normalkkt.jl:51-101)."""

    def _init_sparse(self, backend, st, nx, ind_ineq, H, csr, mode, bandwidth=None, storage="dense"):
        """``H``: None, a dense (nx, nx) tensor (condensed or augmented mode), a 1-D tensor = diagonal of H (any mode)
        or a :class:`DeviceSymCSR` (condensed or augmented mode; kept alive here, the library borrows its arrays).
        ``bandwidth`` (int or "auto"): :meth:`set_bandwidth` at construction.  ``storage="packed"``: the object never
        allocates the dense K -- the band alone, laid out for that bandwidth (``madqp_kkt_create_sparse_packed``)."""
        check_storage(storage, bandwidth, self._band_form, H)
        self._init_problem(backend, st, nx, ind_ineq)
        assert (csr.m, csr.n) == (self.m, self.nx)
        self.H, self.A, self.csr = H, None, csr
        self._t_val = csr.t_val  # values of A' in CSR order, borrowed by the library
        hcsr = isinstance(H, DeviceSymCSR)
        diag = H is not None and not hcsr and H.dim() == 1
        self.storage = storage
        if storage == "packed":
            self._h = backend.kkt_create_sparse_packed(mode, self.nx, self.m, self.ind_ineq, csr, self._t_val)
        else:
            self._h = backend.kkt_create_sparse(mode, self.nx, self.m, self.ind_ineq, None if diag or hcsr else H,
                                                max(self.nx, 1), csr, self._t_val)
        if hcsr:
            assert H.n == self.nx
            backend.kkt_set_hcsr(self._h, H)
        if diag:
            assert H.is_contiguous() and H.numel() == self.nx
            backend.kkt_set_hdiag(self._h, H)
        self.linear_solver = HIPCholeskySolver(backend, self._h)
        if bandwidth is not None:
            self.set_bandwidth(bandwidth)

    def dense_matrix(self):
        """The lower triangle of the stored K (assembled, or factored after a factorisation) as a dense host array of the
        matrix's order, zeros above the diagonal -- from either storage (packed: ``madqp_band_expand`` over the extent).
        Allocates order^2 doubles on the device: inspection and tests, not the large problems packed storage is for."""
        import torch

        ch, order = self.be.kkt_chol(self._h)
        p, ld = self.be.kkt_matrix(self._h, order)
        if not self.be.kkt_storage(self._h)[0]:
            return np.tril(self.be.read_doubles(p, ld * order).reshape(order, ld)[:, :order].T)
        D = torch.zeros((order, max(order, 1)), dtype=torch.float64, device=self.be.device)
        self.be.band_expand(order, p, ld, min(self.be.chol_band_extent(ch), ld), D, max(order, 1))
        return D.cpu().numpy().T.copy()

    _band_form = None  # "condensed" / "normal" on the classes that take a bandwidth

    def set_bandwidth(self, bw):
        """Band-limited assembly and factorisation from here on.  ``bw``: the half-bandwidth of the KKT matrix (at least
        :func:`pattern_bandwidth`, which the library checks once), or "auto" = that number.  Returns the bandwidth set.
        Cannot be undone on this object; dense Hessians and the augmented forms are refused."""
        if self._band_form is None:
            raise ValueError("a bandwidth is taken by the sparse condensed and normal KKT systems only")
        if self.H is not None and not isinstance(self.H, DeviceSymCSR) and self.H.dim() == 2:
            raise ValueError("a bandwidth needs a sparse (DeviceSymCSR), diagonal or absent Hessian, not a dense one")
        if isinstance(bw, str):
            if bw != "auto":
                raise ValueError(f"bandwidth: an int or 'auto', not {bw!r}")
            bw = pattern_bandwidth(self.csr, self.H, self._band_form)
        self.linear_solver = HIPCholeskySolver(self.be, self._h, bandwidth=int(bw))
        return int(bw)


class HIPSparseCondensedKKTSystem(_SparseMixin, HIPCondensedKKTSystem):
    _band_form = "condensed"

    def __init__(self, backend, st, nx, ind_ineq, H, csr, bandwidth=None, storage="dense"):
        if H is not None and not isinstance(H, DeviceSymCSR) and H.dim() == 2:
            assert H.is_contiguous() and H.shape == (nx, nx)
        self._init_sparse(backend, st, nx, ind_ineq, H, csr, 0, bandwidth, storage)


class HIPSparseNormalKKTSystem(_SparseMixin, HIPNormalKKTSystem):
    """Normal equations A (H + Sigma)^-1 A' with H = 0 (the reference's LP-only NormalKKTSystem) or H diagonal
    (1-D tensor; SURVEY.md 8a-note -- what CONT-type QPs need)."""
    _band_form = "normal"

    def __init__(self, backend, st, nx, ind_ineq, H, csr, bandwidth=None, storage="dense"):
        if H is not None and (isinstance(H, DeviceSymCSR) or H.dim() != 1):
            raise ValueError("The KKT system NormalKKTSystem supports only linear programs "
                             "(or a diagonal Hessian given as a vector).")  # normalkkt.jl:45-48
        self._init_sparse(backend, st, nx, ind_ineq, H, csr, 1, bandwidth, storage)


class HIPSparseAugmentedKKTSystem(_SparseMixin, HIPAugmentedKKTSystem):
    """Augmented system with a sparse Jacobian (``DeviceCSR``) scattered into the dense quasi-definite matrix:
    the exact treatment of equality rows for a QP whose Hessian is dense, diagonal (1-D tensor) or sparse
    (:class:`DeviceSymCSR`)."""

    def __init__(self, backend, st, nx, ind_ineq, H, csr):
        if H is not None and not isinstance(H, DeviceSymCSR) and H.dim() == 2:
            assert H.is_contiguous() and H.shape == (nx, nx)
        self._init_sparse(backend, st, nx, ind_ineq, H, csr, 2)
        self.linear_solver = HIPQuasiDefiniteSolver(backend, self._h, self.nx, self.m)
