# MadQPHIPSparse.jl -- the sparse front end of libmadqp_hip.so behind MadNLP's AbstractKKTSystem surface.
#
# STATUS: UNVERIFIED UNDER JULIA, like MadQPHIP.jl (no Julia toolchain in the authoring or GPU image).  What IS executed:
# every ccall below binds one prototype of include/madqp.h (tests/test_csr_map.py), and tests/julia_replay_sparse.py
# replays -- through ctypes, entry point by entry point, in the order MadIPM issues them -- exactly the call sequence of
# the methods of this file (tests/test_gpu_julia_sparse.py).  A change here needs the same change there.
#
# Why a second file: MadQPHIP.jl hands the library DENSE operands -- nx*m doubles for A, nx*nx for H, cleared and
# refilled by madqp_coo_map_apply -- whatever the sparsity of the model.  Here the operands stay sparse, as in the
# reference (coo_to_csr src/utils.jl:148-197, src/KKT/normalkkt.jl:51-101): the two patterns MadNLP.SparseCallback
# reports become CSR structures on the device once (madqp_csr_map_create: A, A' and the full symmetric H from its one
# triangle, duplicates merged), and after every evaluation compress_jacobian! / compress_hessian! move the nnz callback
# values into the stored values (madqp_csr_map_apply; src/KKT/normalkkt.jl:149-158).  Nothing of size nx*m or nx*nx is
# allocated for an operand; the factorised matrix stays dense (madqp_kkt_create_sparse).
#
# What it provides
#   HIPSparseCondensedKKTSystem / HIPSparseAugmentedKKTSystem / HIPSparseNormalKKTSystem  <: MadNLP.AbstractKKTSystem
#   with the linear solver of MadQPHIP.jl (HIPCholeskySolver) and the same per-variable kernels.
#
# Usage
#   using MadNLP, MadIPM, AMDGPU; include("MadQPHIP.jl"); include("MadQPHIPSparse.jl"); using .MadQPHIP, .MadQPHIPSparse
#   solver = MadIPM.MPCSolver(qp_on_rocarrays; kkt_system = MadQPHIPSparse.HIPSparseCondensedKKTSystem,
#                             linear_solver = MadQPHIP.HIPCholeskySolver,
#                             regularization = MadIPM.FixedRegularization(1e-8, -1e-8))
#   MadIPM.solve!(solver)
module MadQPHIPSparse

import MadNLP
import MadIPM
using LinearAlgebra
import LinearAlgebra: mul!
import ..MadQPHIP: Context, check, CState, dptr, NULLF, libmadqp, HIPDenseKKTMatrix, HIPCholeskySolver, state, @k

const CSR_ROWS = Int32(0)   # MADQP_CSR_ROWS: CSR of the matrix
const CSR_COLS = Int32(1)   # MADQP_CSR_COLS: CSR of its transpose
const CSR_SYM = Int32(2)    # MADQP_CSR_SYM:  full symmetric pattern from entries of either triangle

# One madqp_csr_map: the handle, the number of stored entries and the two DEVICE arrays of the structure.  The arrays
# belong to the map; the KKT object borrows them (include/madqp.h: no call on the KKT object after the map is destroyed).
struct CSRMap
    handle::Ptr{Cvoid}
    stored::Int
    ptr::Ptr{Int64}
    col::Ptr{Int64}
end
const NO_MAP = CSRMap(C_NULL, 0, Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL))

function csr_map(ctx::Context, I::Vector{Int32}, J::Vector{Int32}, nrows, ncols, kind::Int32)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ctx, ccall((:madqp_csr_map_create, libmadqp), Int32,
                     (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int32}, Int64, Int64, Int32, Ref{Ptr{Cvoid}}),
                     ctx.ptr, length(I), I, J, nrows, ncols, kind, ref))
    rows, stored = Ref{Int64}(0), Ref{Int64}(0)
    p, c = Ref{Ptr{Int64}}(C_NULL), Ref{Ptr{Int64}}(C_NULL)
    check(ctx, ccall((:madqp_csr_map_pattern, libmadqp), Int32,
                     (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Ptr{Int64}}, Ref{Ptr{Int64}}), ref[], rows, stored, p, c))
    return CSRMap(ref[], Int(stored[]), p[], c[])
end
destroy(mp::CSRMap) = mp.handle == C_NULL || ccall((:madqp_csr_map_destroy, libmadqp), Int32, (Ptr{Cvoid},), mp.handle)

# F = :condensed  K = H + Sigma_x + A' Theta A               (madqp_kkt_create_sparse, mode 0)
#     :normal     A Sigma^-1 A', LP only                      (mode 1; the reference's NormalKKTSystem)
#     :augmented  [H + Sigma_x, A'; A, -D], L diag(I,-I) L'    (mode 2; MadNLP's default K2 form)
struct HIPSparseKKTSystem{T, VT, MT, QN, VI, LS, F} <: MadNLP.AbstractKKTSystem{T, VT, MT, QN}
    aug_com::HIPDenseKKTMatrix{T}     # the matrix object the linear solver keeps (K and its factor live in the library)
    handle::Ptr{Cvoid}
    ctx::Context
    a_val::VT             # stored values of A in CSR order   (jac_map.stored)
    at_val::VT            # stored values of A' in CSR order  (jact_map.stored)
    h_val::VT             # stored values of the full symmetric H in CSR order (hess_map.stored)
    jac::VT               # nnzj callback buffer (get_jacobian), COO order of the model's pattern
    hess::VT              # nnzh callback buffer (get_hessian)
    jac_map::CSRMap       # jac -> a_val
    jact_map::CSRMap      # jac -> at_val
    hess_map::CSRMap      # hess -> h_val (NO_MAP for an LP)
    # fields MadIPM reads generically (src/kernels.jl:135-144, src/solver.jl:16-18)
    reg::VT; pr_diag::VT; du_diag::VT
    l_diag::VT; u_diag::VT; l_lower::VT; u_lower::VT
    linear_solver::LS
    ind_ineq::VI; ind_lb::VI; ind_ub::VI      # 1-based, as MadNLP keeps them
    ind_lb0::VI; ind_ub0::VI                  # 0-based device copies handed to the library
    cstate::Base.RefValue{CState}             # view with the KKT's own fields only (build_kkt!, solve!, mul!)
    n::Int; m::Int; nx::Int
end
const HIPSparseCondensedKKTSystem = HIPSparseKKTSystem{T, VT, MT, QN, VI, LS, :condensed} where {T, VT, MT, QN, VI, LS}
const HIPSparseAugmentedKKTSystem = HIPSparseKKTSystem{T, VT, MT, QN, VI, LS, :augmented} where {T, VT, MT, QN, VI, LS}
const HIPSparseNormalKKTSystem = HIPSparseKKTSystem{T, VT, MT, QN, VI, LS, :normal} where {T, VT, MT, QN, VI, LS}
form(::HIPSparseKKTSystem{T, VT, MT, QN, VI, LS, F}) where {T, VT, MT, QN, VI, LS, F} = F

function _create(F::Symbol, cb::MadNLP.SparseCallback{T, VT}, ind_cons, linear_solver::Type, opt_linear_solver) where {T, VT}
    nx, m = cb.nvar, cb.ncon
    ind_ineq = ind_cons.ind_ineq
    ns = length(ind_ineq)
    n = nx + ns
    nlb, nub = length(ind_cons.ind_lb), length(ind_cons.ind_ub)
    if F == :normal && cb.nnzh > 0                                    # src/KKT/normalkkt.jl:45-48
        error("The KKT system NormalKKTSystem supports only linear programs.")
    end
    ctx = Context()
    # sparsity patterns of the callbacks (src/KKT/normalkkt.jl:51-53)
    jI = MadNLP.create_array(cb, Int32, cb.nnzj); jJ = MadNLP.create_array(cb, Int32, cb.nnzj)
    MadNLP._jac_sparsity_wrapper!(cb, jI, jJ)
    hI = MadNLP.create_array(cb, Int32, cb.nnzh); hJ = MadNLP.create_array(cb, Int32, cb.nnzh)
    cb.nnzh > 0 && MadNLP._hess_sparsity_wrapper!(cb, hI, hJ)
    jIh, jJh = Vector{Int32}(Array(jI)), Vector{Int32}(Array(jJ))
    maps = CSRMap[]
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    local jac_map, jact_map, hess_map, a_val, at_val, h_val
    mk(k) = VT(undef, k)
    try
        # pattern -> CSR structure, once (coo_to_csr, src/utils.jl:148-197; src/KKT/normalkkt.jl:84-91): A by rows, A' by
        # rows (= A by columns), and both triangles of H from the one MadNLP reports
        jac_map = csr_map(ctx, jIh, jJh, m, nx, CSR_ROWS); push!(maps, jac_map)
        jact_map = csr_map(ctx, jIh, jJh, m, nx, CSR_COLS); push!(maps, jact_map)
        hess_map = NO_MAP
        if cb.nnzh > 0
            hess_map = csr_map(ctx, Vector{Int32}(Array(hI)), Vector{Int32}(Array(hJ)), nx, nx, CSR_SYM)
            push!(maps, hess_map)
        end
        a_val, at_val, h_val = mk(jac_map.stored), mk(jact_map.stored), mk(hess_map.stored)
        ineq0 = Int64.(Array(ind_ineq)) .- 1
        mode = F == :condensed ? Int32(0) : (F == :normal ? Int32(1) : Int32(2))
        check(ctx, ccall((:madqp_kkt_create_sparse, libmadqp), Int32,
                         (Ptr{Cvoid}, Int32, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Int64,
                          Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                         ctx.ptr, mode, nx, m, ns, ineq0, NULLF, max(nx, 1),
                         jac_map.ptr, jac_map.col, dptr(a_val), jact_map.ptr, jact_map.col, dptr(at_val), ref))
        if cb.nnzh > 0      # the symmetry madqp_kkt_set_hcsr asks for is the SYM map's: (i, j) and (j, i) share their sources
            check(ctx, ccall((:madqp_kkt_set_hcsr, libmadqp), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                             ref[], hess_map.ptr, hess_map.col, dptr(h_val)))
        end
        # the AUTO refinement request of MadQPHIP.jl (MadIPM's solve_system! calls solve! once; DESIGN.md section 4.2)
        check(ctx, ccall((:madqp_kkt_set_refine, libmadqp), Int32, (Ptr{Cvoid}, Int32), ref[],
                         parse(Int32, get(ENV, "MADQP_KKT_REFINE", "-1"))))
    catch
        ref[] != C_NULL && ccall((:madqp_kkt_destroy, libmadqp), Int32, (Ptr{Cvoid},), ref[])
        foreach(destroy, maps)
        rethrow()
    end
    order = F == :augmented ? (cld(nx, 128) * 128 + m) : (F == :normal ? m : nx)
    aug_com = HIPDenseKKTMatrix{T}(ref[], ctx, order, Ptr{Cvoid}[])   # its finalizer destroys the KKT object
    # The maps live exactly as long as the matrix object that the KKT system AND the linear solver hold: nothing can call
    # into the KKT object once this runs (madqp_kkt_destroy, the other finalizer, reads no borrowed array).
    finalizer(_ -> foreach(destroy, maps), aug_com)
    ls = linear_solver(aug_com; opt = opt_linear_solver)             # src/KKT/normalkkt.jl:99-101
    reg, pr_diag, du_diag = mk(n), mk(n), mk(m)
    l_diag, u_diag, l_lower, u_lower = mk(nlb), mk(nub), mk(nlb), mk(nub)
    ind_lb0, ind_ub0 = ind_cons.ind_lb .- 1, ind_cons.ind_ub .- 1
    cs = CState(n, m, nlb, nub, dptr(ind_lb0), dptr(ind_ub0),
                NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF, NULLF,
                dptr(reg), dptr(pr_diag), dptr(du_diag), dptr(l_diag), dptr(l_lower), dptr(u_diag), dptr(u_lower))
    VI = typeof(ind_cons.ind_lb)
    MT = typeof(reshape(mk(0), 0, 0))
    return HIPSparseKKTSystem{T, VT, MT, MadNLP.ExactHessian{T, VT}, VI, typeof(ls), F}(
        aug_com, ref[], ctx, a_val, at_val, h_val, mk(cb.nnzj), mk(cb.nnzh), jac_map, jact_map, hess_map,
        reg, pr_diag, du_diag, l_diag, u_diag, l_lower, u_lower, ls,
        ind_ineq, ind_cons.ind_lb, ind_cons.ind_ub, ind_lb0, ind_ub0, Ref(cs), n, m, nx)
end

for (TY, F) in ((:HIPSparseCondensedKKTSystem, :condensed), (:HIPSparseAugmentedKKTSystem, :augmented),
                (:HIPSparseNormalKKTSystem, :normal))
    @eval function MadNLP.create_kkt_system(
        ::Type{$TY}, cb::MadNLP.SparseCallback{T, VT}, ind_cons, linear_solver::Type;
        opt_linear_solver = MadNLP.default_options(linear_solver),
        hessian_approximation = MadNLP.ExactHessian, qn_options = MadNLP.QuasiNewtonOptions(),
    ) where {T, VT}
        return _create($(QuoteNode(F)), cb, ind_cons, linear_solver, opt_linear_solver)
    end
end

MadNLP.num_variables(kkt::HIPSparseKKTSystem) = kkt.n                 # src/KKT/normalkkt.jl:128
MadNLP.get_jacobian(kkt::HIPSparseKKTSystem) = kkt.jac                # :129 -- the nnzj buffer SparseCallback fills
MadNLP.get_hessian(kkt::HIPSparseKKTSystem) = kkt.hess                # :130
function MadNLP.is_inertia_correct(kkt::HIPSparseKKTSystem, num_pos, num_zero, num_neg)   # :132-134
    form(kkt) == :augmented && return (num_zero == 0) && (num_neg == kkt.m)
    return (num_zero == 0) && (num_pos == kkt.aug_com.order)
end

function MadNLP.initialize!(kkt::HIPSparseKKTSystem{T}) where {T}      # src/KKT/normalkkt.jl:136-147
    check(kkt.ctx, ccall((:madqp_kkt_initialize, libmadqp), Int32, (Ptr{Cvoid}, Ref{CState}), kkt.handle, kkt.cstate))
    return
end

# src/KKT/normalkkt.jl:149-158: callback values (COO order) -> nzval of the CSR operands, A and A' (the reference keeps
# A' only; the library multiplies with both).  The slack columns (-1) are implicit in the library (ind_ineq).
function MadNLP.compress_jacobian!(kkt::HIPSparseKKTSystem)
    check(kkt.ctx, ccall((:madqp_csr_map_apply, libmadqp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                         kkt.jac_map.handle, dptr(kkt.jac), dptr(kkt.a_val)))
    check(kkt.ctx, ccall((:madqp_csr_map_apply, libmadqp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                         kkt.jact_map.handle, dptr(kkt.jac), dptr(kkt.at_val)))
    return
end
function MadNLP.compress_hessian!(kkt::HIPSparseKKTSystem)
    kkt.hess_map.handle == C_NULL && return
    check(kkt.ctx, ccall((:madqp_csr_map_apply, libmadqp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                         kkt.hess_map.handle, dptr(kkt.hess), dptr(kkt.h_val)))
    return
end

function MadNLP.jtprod!(y::AbstractVector, kkt::HIPSparseKKTSystem, x::AbstractVector)   # :162-164
    check(kkt.ctx, ccall((:madqp_kkt_jtprod, libmadqp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                         kkt.handle, dptr(y), dptr(x)))
    return y
end

function MadNLP.build_kkt!(kkt::HIPSparseKKTSystem)                  # src/KKT/normalkkt.jl:166-180
    check(kkt.ctx, ccall((:madqp_kkt_build, libmadqp), Int32, (Ptr{Cvoid}, Ref{CState}), kkt.handle, kkt.cstate))
    return
end

function MadNLP.solve!(kkt::HIPSparseKKTSystem, w::MadNLP.AbstractKKTVector)   # :182-205
    check(kkt.ctx, ccall((:madqp_kkt_solve, libmadqp), Int32, (Ptr{Cvoid}, Ref{CState}, Ptr{Float64}),
                         kkt.handle, kkt.cstate, dptr(MadNLP.full(w))))
    return w
end

# a block of right-hand sides, as MadQPHIP's method for its KKT type (the linear solver's matrix method is inherited:
# this type uses MadQPHIP.HIPCholeskySolver): column c of W is the `full` of an UnreducedKKTVector
function MadNLP.solve!(kkt::HIPSparseKKTSystem, W::AbstractMatrix)
    check(kkt.ctx, ccall((:madqp_kkt_solve_many, libmadqp), Int32, (Ptr{Cvoid}, Ref{CState}, Ptr{Float64}, Int64, Int64),
                         kkt.handle, kkt.cstate, dptr(W), size(W, 1), size(W, 2)))
    return W
end

function mul!(w::MadNLP.AbstractKKTVector{T}, kkt::HIPSparseKKTSystem, v::MadNLP.AbstractKKTVector,
              alpha = one(T), beta = zero(T)) where {T}           # :207-219
    check(kkt.ctx, ccall((:madqp_kkt_mul, libmadqp), Int32,
                         (Ptr{Cvoid}, Ref{CState}, Ptr{Float64}, Ptr{Float64}, Float64, Float64),
                         kkt.handle, kkt.cstate, dptr(MadNLP.full(w)), dptr(MadNLP.full(v)), alpha, beta))
    return w
end

# the block forms of MadQPHIP.jl for this KKT type: W[:, c] <- alpha K V[:, c] + beta W[:, c] (madqp_kkt_mul_many: with
# sparse A and H bitwise the column loop over mul!), and the switch of solve!(kkt, ::AbstractMatrix) to block products
function mul!(W::AbstractMatrix, kkt::HIPSparseKKTSystem, V::AbstractMatrix, alpha = 1.0, beta = 0.0)
    check(kkt.ctx, ccall((:madqp_kkt_mul_many, libmadqp), Int32,
                         (Ptr{Cvoid}, Ref{CState}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Float64, Float64),
                         kkt.handle, kkt.cstate, dptr(W), size(W, 1), dptr(V), size(V, 1), size(W, 2), alpha, beta))
    return W
end

function block_products!(kkt::HIPSparseKKTSystem, on::Bool)
    check(kkt.ctx, ccall((:madqp_kkt_set_block_products, libmadqp), Int32, (Ptr{Cvoid}, Int32), kkt.handle, Int32(on)))
    return kkt
end

# --------------------------------------------------------------------------- src/kernels.jl on the device
# The overrides of MadQPHIP.jl dispatch on its own KKT types; these are the same calls for the sparse types (`state` and
# the macro `@k` are MadQPHIP's: the full state view of one solver, and check(ccall(name, ctx, state, args...))).
const HIPSparseSolver = MadIPM.MPCSolver{T, VT, VI, K} where {T, VT, VI, K <: HIPSparseKKTSystem}

function MadIPM.set_aug_diagonal_reg!(kkt::HIPSparseKKTSystem{T}, solver::MadNLP.AbstractMadNLPSolver{T}) where {T}   # kernels.jl:128-146
    check(kkt.ctx, ccall((:madqp_kkt_set_aug_diagonal_reg, libmadqp), Int32, (Ptr{Cvoid}, Ref{CState}, Float64, Float64),
                         kkt.handle, state(solver), solver.del_w, solver.del_c))
    return
end
MadIPM.set_initial_primal_rhs!(solver::HIPSparseSolver) = @k madqp_set_initial_primal_rhs ()
MadIPM.set_initial_dual_rhs!(solver::HIPSparseSolver) = @k madqp_set_initial_dual_rhs ()
MadIPM.set_predictive_rhs!(solver::MadNLP.AbstractMadNLPSolver, ::HIPSparseKKTSystem) = @k madqp_set_predictive_rhs ()
MadIPM.set_correction_rhs!(solver::MadNLP.AbstractMadNLPSolver, ::HIPSparseKKTSystem, mu::Float64,
                           clb::AbstractVector{Float64}, cub::AbstractVector{Float64}, ilb, iub) =
    @k madqp_set_correction_rhs (Float64,) mu
MadIPM.get_correction!(solver::HIPSparseSolver, clb, cub) = @k madqp_get_correction ()
MadIPM.set_extra_correction!(solver::HIPSparseSolver, clb, cub, ap, ad, bmin, bmax, mu) =
    @k madqp_set_extra_correction (Float64, Float64, Float64, Float64, Float64) ap ad bmin bmax mu

function MadIPM.get_complementarity_measure(solver::HIPSparseSolver)            # kernels.jl:171-190
    out = Ref{Float64}(0.0)
    @k madqp_get_complementarity_measure (Ref{Float64},) out
    return out[]
end
function MadIPM.get_affine_complementarity_measure(solver::HIPSparseSolver, ap, ad)   # kernels.jl:192-224
    out = Ref{Float64}(0.0)
    @k madqp_get_affine_complementarity_measure (Float64, Float64, Ref{Float64}) ap ad out
    return out[]
end
function MadIPM.get_fraction_to_boundary_step(solver::HIPSparseSolver, tau)      # kernels.jl:290-305
    a = zeros(Float64, 4); ib = zeros(Int64, 4)
    @k madqp_get_alpha_max (Float64, Ptr{Float64}, Ptr{Int64}) tau a ib
    return min(a[1], a[2]), min(a[3], a[4])
end

end # module
