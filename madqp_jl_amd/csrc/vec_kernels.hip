// Fused per-variable kernels of the predictor-corrector loop (src/kernels.jl, src/solver.jl) and
// the MadNLP vector helpers they call.  All are HBM-bound streaming passes; every reduction is a
// wave-shuffle + LDS block reduction into per-block partials followed by a fixed-order final
// pass (deterministic), the scalars land in the context's device result block and are copied to
// the host with one synchronisation.
//
// Arithmetic is written in the reference's evaluation order and the library is compiled with
// -ffp-contract=off, so elementwise results are bit-identical to the numpy oracle; max / min /
// arg-min reductions are order independent, sums are compared to a tolerance.
#include "grid_kernels.h"

namespace {
#include "vec_kernels.inc"

int32_t finalize(madqp_ctx* ctx, int nblocks, int nv, const int* ops, int slot0 = 0) {
    FinalOps f;
    f.nv = nv;
    for (int i = 0; i < nv; ++i) f.op[i] = (int8_t)ops[i];
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(TPB), 0, ctx->stream, ctx->d_part, nblocks, f,
                       ctx->d_res + slot0);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

int32_t check_state(madqp_ctx* ctx, const madqp_state* st) {
    ARG_TRY(ctx, ctx != nullptr);
    ARG_TRY(ctx, st != nullptr);
    ARG_TRY(ctx, st->n >= 0 && st->m >= 0 && st->nlb >= 0 && st->nub >= 0);
    ARG_TRY(ctx, st->nlb == 0 || st->ind_lb);
    ARG_TRY(ctx, st->nub == 0 || st->ind_ub);
    return MADQP_OK;
}
}  // namespace

#define CHECK_STATE()                         \
    do {                                      \
        if (!ctx) return MADQP_ERR_ARG;       \
        int32_t r_ = check_state(ctx, st);    \
        if (r_) return r_;                    \
    } while (0)

static inline int64_t max4(int64_t a, int64_t b, int64_t c, int64_t d) {
    return std::max(std::max(a, b), std::max(c, d));
}

extern "C" int32_t madqp_set_aug_diagonal_reg(madqp_ctx* ctx, const madqp_state* st, double del_w,
                                              double del_c) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(aug_diag_fill_kernel, std::max(st->n, st->m), *st, del_w, del_c);
    if (st->nlb) LAUNCH(aug_diag_lb_kernel, st->nlb, *st);
    if (st->nub) LAUNCH(aug_diag_ub_kernel, st->nub, *st);
    return MADQP_OK;
}

static int32_t rhs_launch(madqp_ctx* ctx, const madqp_state* st, int mode, double mu, const double* mu_dev = nullptr) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(rhs_kernel, max4(st->n, st->m, st->nlb, st->nub), *st, mode, mu, mu_dev);
    return MADQP_OK;
}
// set_correction_rhs! with mu taken from device memory (mpc.hip, body_fused)
int32_t madqp_set_correction_rhs_dev(madqp_ctx* ctx, const madqp_state* st, const double* mu_dev) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, mu_dev != nullptr);
    return rhs_launch(ctx, st, 1, 0.0, mu_dev);
}
extern "C" int32_t madqp_set_initial_primal_rhs(madqp_ctx* ctx, const madqp_state* st) {
    return rhs_launch(ctx, st, 2, 0.0);
}
extern "C" int32_t madqp_set_initial_dual_rhs(madqp_ctx* ctx, const madqp_state* st) {
    return rhs_launch(ctx, st, 3, 0.0);
}
extern "C" int32_t madqp_set_predictive_rhs(madqp_ctx* ctx, const madqp_state* st) {
    return rhs_launch(ctx, st, 0, 0.0);
}
extern "C" int32_t madqp_set_correction_rhs(madqp_ctx* ctx, const madqp_state* st, double mu) {
    return rhs_launch(ctx, st, 1, mu);
}

extern "C" int32_t madqp_get_correction(madqp_ctx* ctx, const madqp_state* st) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(correction_kernel, std::max(st->nlb, st->nub), *st);
    return MADQP_OK;
}

// mu_dev != nullptr: mu is read there and the kernel forms beta_min * mu, beta_max * mu; a8 != nullptr: the step lengths
// are mpc_steps(a8), read on the device
int32_t madqp_set_extra_correction_dev(madqp_ctx* ctx, const madqp_state* st, double alpha_p, double alpha_d,
                                       double beta_min, double beta_max, const double* mu_dev, const double* a8) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(extra_correction_kernel, std::max(st->nlb, st->nub), *st, alpha_p, alpha_d, beta_min, beta_max, mu_dev, a8);
    return MADQP_OK;
}
extern "C" int32_t madqp_set_extra_correction(madqp_ctx* ctx, const madqp_state* st, double alpha_p,
                                              double alpha_d, double beta_min, double beta_max,
                                              double mu) {
    return madqp_set_extra_correction_dev(ctx, st, alpha_p, alpha_d, beta_min * mu, beta_max * mu, nullptr, nullptr);
}

// ---- scalars of the iteration that never visit the host (mpc.hip, body_fused) -------------------------------------------
// One thread and one rule of mpc_rules.inc each, between the fields of the result block that file names.
#define ONE_THREAD if (threadIdx.x || blockIdx.x) return
__global__ void mpc_trial_alpha_kernel(double* __restrict__ res) {
    ONE_THREAD;
    mpc_trial_alpha_block(res + MPC_SL_GZ_ALPHA, res + MPC_SL_TRIAL_ALPHA);
}
__global__ void mpc_mu_kernel(double* __restrict__ res, double nb, double mu_min, int step_rule, double step_param) {
    ONE_THREAD;
    mpc_barrier_block(res + MPC_SL_COMPL, nb, mu_min, step_rule, step_param, res + MPC_SL_BARRIER);
}
__global__ void mpc_muc_kernel(double* __restrict__ res, int compl_slot, double nb) {
    ONE_THREAD;
    res[MPC_SL_MUC] = mpc_muc(mpc_compl_mean(res + compl_slot, nb), res[MPC_SL_MUCURR]);
}
__global__ void mpc_decide_kernel(double* res, MpcDecideOpt opt) {
    ONE_THREAD;
    mpc_decide(res, opt, res + MPC_SL_DECISION);
}
#define LAUNCH_ONE_THREAD(kern, ...)                                                              \
    do {                                                                                          \
        if (!ctx) return MADQP_ERR_ARG;                                                           \
        ProfScope ps(ctx, MADQP_PROF_VEC);                                                        \
        hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, ctx->stream, ctx->d_res, ##__VA_ARGS__);   \
        LAUNCH_CHECK(ctx);                                                                        \
        return MADQP_OK;                                                                          \
    } while (0)
int32_t madqp_q_mpc_trial_alpha(madqp_ctx* ctx) { LAUNCH_ONE_THREAD(mpc_trial_alpha_kernel); }
int32_t madqp_q_mpc_mu(madqp_ctx* ctx, int64_t nb, double mu_min, int step_rule, double step_param) {
    LAUNCH_ONE_THREAD(mpc_mu_kernel, (double)nb, mu_min, step_rule, step_param);
}
int32_t madqp_q_mpc_muc(madqp_ctx* ctx, int compl_slot, int64_t nb) {
    ARG_TRY(ctx, compl_slot >= 0 && compl_slot + MPC_W_COMPL <= MADQP_FAULT_SLOT);
    LAUNCH_ONE_THREAD(mpc_muc_kernel, compl_slot, (double)nb);
}
int32_t madqp_q_mpc_decide(madqp_ctx* ctx, const MpcDecideOpt& opt) { LAUNCH_ONE_THREAD(mpc_decide_kernel, opt); }
// dst = src where *flag != 0 (the dropped Gondzio trial's direction goes back, src/solver.jl:232)
__global__ __launch_bounds__(TPB) void copy_if_kernel(int64_t len, const double* __restrict__ src, double* __restrict__ dst,
                                                      const double* __restrict__ flag) {
    if (*flag == 0.0) return;
    GRID_STRIDE(i, len) dst[i] = src[i];
}
int32_t madqp_copy_if_dev(madqp_ctx* ctx, int64_t len, const double* src, double* dst, const double* flag_dev) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, len >= 0 && (len == 0 || (src && dst)) && flag_dev);
    if (len == 0) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(copy_if_kernel, len, len, src, dst, flag_dev);
    return MADQP_OK;
}

// Queued forms (madqp_q_*): the reduction lands in the device result block at slot0 and stays there; the caller
// reads several of them back with ONE madqp_read_results (mpc.hip).  The extern "C" entry points below are the
// queued form at slot 0 followed by the read-back.
int32_t madqp_q_compl(madqp_ctx* ctx, const madqp_state* st, int affine, double ap, double ad, const double* a8,
                      int slot0) {
    CHECK_STATE();
    if (st->nlb + st->nub == 0) {  // src/kernels.jl:173-174
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_res + slot0, 0, 2 * sizeof(double), ctx->stream));
        return MADQP_OK;
    }
    const int64_t L = std::max(st->nlb, st->nub);
    const int nb = grid_for(L);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    hipLaunchKernelGGL(compl_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, *st, affine, ap, ad, a8, ctx->d_part);
    LAUNCH_CHECK(ctx);
    const int ops[2] = {OP_SUM, OP_SUM};
    return finalize(ctx, nb, 2, ops, slot0);
}

static int32_t compl_launch(madqp_ctx* ctx, const madqp_state* st, int affine, double ap, double ad,
                            double* mu_host) {
    CHECK_STATE();
    ARG_TRY(ctx, mu_host != nullptr);
    if (st->nlb + st->nub == 0) {  // src/kernels.jl:173-174
        *mu_host = 0.0;
        return MADQP_OK;
    }
    int32_t r = madqp_q_compl(ctx, st, affine, ap, ad, nullptr, 0);
    if (r) return r;
    double out[2];
    r = madqp_read_results(ctx, 2, out);
    if (r) return r;
    *mu_host = mpc_compl_mean(out, (double)(st->nlb + st->nub));
    return MADQP_OK;
}
extern "C" int32_t madqp_get_complementarity_measure(madqp_ctx* ctx, const madqp_state* st,
                                                     double* mu_host) {
    return compl_launch(ctx, st, 0, 0.0, 0.0, mu_host);
}
extern "C" int32_t madqp_get_affine_complementarity_measure(madqp_ctx* ctx, const madqp_state* st,
                                                            double alpha_p, double alpha_d,
                                                            double* mu_host) {
    return compl_launch(ctx, st, 1, alpha_p, alpha_d, mu_host);
}

namespace {
__global__ void alpha_none_kernel(double* __restrict__ res) {  // no bounds: alpha = 1, nothing blocks
    if (threadIdx.x < 4) {
        res[2 * threadIdx.x] = 1.0;
        res[2 * threadIdx.x + 1] = -1.0;
    }
}
}  // namespace
int32_t madqp_q_alpha_max(madqp_ctx* ctx, const madqp_state* st, double tau, int slot0) {
    return madqp_q_alpha_max_dev(ctx, st, tau, nullptr, slot0);
}
// tau_dev != nullptr: tau is read from device memory
int32_t madqp_q_alpha_max_dev(madqp_ctx* ctx, const madqp_state* st, double tau, const double* tau_dev, int slot0) {
    CHECK_STATE();
    const int64_t L = std::max(st->nlb, st->nub);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (L == 0) {
        hipLaunchKernelGGL(alpha_none_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->d_res + slot0);
        LAUNCH_CHECK(ctx);
        return MADQP_OK;
    }
    const int nb = grid_for(L);
    hipLaunchKernelGGL(alpha_max_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, *st, tau, ctx->d_part, tau_dev);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(alpha_max_final_kernel, dim3(1), dim3(TPB), 0, ctx->stream, ctx->d_part, nb,
                       ctx->d_res + slot0);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

extern "C" int32_t madqp_get_alpha_max(madqp_ctx* ctx, const madqp_state* st, double tau,
                                       double* alpha_host, int64_t* iblock_host) {
    CHECK_STATE();
    ARG_TRY(ctx, alpha_host && iblock_host);
    const int64_t L = std::max(st->nlb, st->nub);
    if (L == 0) {
        for (int q = 0; q < 4; ++q) {
            alpha_host[q] = 1.0;
            iblock_host[q] = -1;
        }
        return MADQP_OK;
    }
    int32_t r = madqp_q_alpha_max(ctx, st, tau, 0);
    if (r) return r;
    double out[8];
    r = madqp_read_results(ctx, 8, out);
    if (r) return r;
    for (int q = 0; q < 4; ++q) {
        alpha_host[q] = out[2 * q];
        iblock_host[q] = (int64_t)out[2 * q + 1];
    }
    return MADQP_OK;
}

int32_t madqp_update_iterates_dev(madqp_ctx* ctx, const madqp_state* st, double alpha_p, double alpha_d,
                                  const double* dec_dev) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(update_iterates_kernel, max4(st->n, st->m, st->nlb, st->nub), *st, alpha_p, alpha_d, dec_dev);
    return MADQP_OK;
}
extern "C" int32_t madqp_update_iterates(madqp_ctx* ctx, const madqp_state* st, double alpha_p,
                                         double alpha_d) {
    return madqp_update_iterates_dev(ctx, st, alpha_p, alpha_d, nullptr);
}
// 4 slots: |c|, dual, complementarity lower / upper (madqp_inf_from_block combines the last two)
int32_t madqp_q_inf(madqp_ctx* ctx, const madqp_state* st, int slot0) {
    CHECK_STATE();
    const int64_t L = max4(st->n, st->m, st->nlb, st->nub);
    if (L == 0) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_res + slot0, 0, 4 * sizeof(double), ctx->stream));
        return MADQP_OK;
    }
    const int nb = grid_for(L);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    hipLaunchKernelGGL(inf_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, *st, ctx->d_part);
    LAUNCH_CHECK(ctx);
    const int ops[4] = {OP_MAX, OP_MAX, OP_MAX, OP_MAX};
    return finalize(ctx, nb, 4, ops, slot0);
}
void madqp_inf_from_block(const double* out, double* out3) {
    out3[0] = out[0];
    out3[1] = out[1];
    out3[2] = mpc_nanmax(out[2], out[3]);
}

extern "C" int32_t madqp_get_inf(madqp_ctx* ctx, const madqp_state* st, double* out_host) {
    CHECK_STATE();
    ARG_TRY(ctx, out_host != nullptr);
    const int64_t L = max4(st->n, st->m, st->nlb, st->nub);
    if (L == 0) {
        out_host[0] = out_host[1] = out_host[2] = 0.0;
        return MADQP_OK;
    }
    int32_t r = madqp_q_inf(ctx, st, 0);
    if (r) return r;
    double out[4];
    r = madqp_read_results(ctx, 4, out);
    if (r) return r;
    madqp_inf_from_block(out, out_host);
    return MADQP_OK;
}

int32_t madqp_adjust_boundary_dev(madqp_ctx* ctx, const madqp_state* st, double mu, const double* dec_dev,
                                  const double* mu_dev) {
    CHECK_STATE();
    const double c1 = mu_dev ? MPC_EPS : mpc_adjust_c1(mu);  // (the kernel multiplies by *mu_dev)
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (std::max(st->nlb, st->nub) > 0)
        LAUNCH(adjust_boundary_kernel, std::max(st->nlb, st->nub), *st, c1, MPC_ADJUST_C2, dec_dev, mu_dev);
    return MADQP_OK;
}
extern "C" int32_t madqp_adjust_boundary(madqp_ctx* ctx, const madqp_state* st, double mu) {
    return madqp_adjust_boundary_dev(ctx, st, mu, nullptr, nullptr);
}

extern "C" int32_t madqp_reduce_rhs(madqp_ctx* ctx, const madqp_state* st, double* w) {
    CHECK_STATE();
    ARG_TRY(ctx, w != nullptr);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (st->nlb)
        LAUNCH(reduce_rhs_kernel, st->nlb, st->nlb, st->ind_lb, w, w + st->n + st->m, st->l_diag);
    if (st->nub)
        LAUNCH(reduce_rhs_kernel, st->nub, st->nub, st->ind_ub, w, w + st->n + st->m + st->nlb,
               st->u_diag);
    return MADQP_OK;
}

extern "C" int32_t madqp_finish_aug_solve(madqp_ctx* ctx, const madqp_state* st, double* w) {
    CHECK_STATE();
    ARG_TRY(ctx, w != nullptr);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (std::max(st->nlb, st->nub) > 0)
        LAUNCH(finish_aug_solve_kernel, std::max(st->nlb, st->nub), *st, w);
    return MADQP_OK;
}

extern "C" int32_t madqp_kktmul(madqp_ctx* ctx, const madqp_state* st, double* w, const double* v,
                                double alpha, double beta) {
    CHECK_STATE();
    ARG_TRY(ctx, w && v);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (std::max(st->n, st->m) > 0)
        LAUNCH(kktmul_diag_kernel, std::max(st->n, st->m), *st, w, v, alpha);
    if (st->nlb) LAUNCH(kktmul_lb_kernel, st->nlb, *st, w, v, alpha, beta);
    if (st->nub) LAUNCH(kktmul_ub_kernel, st->nub, *st, w, v, alpha, beta);
    return MADQP_OK;
}

int32_t madqp_q_norm_inf3(madqp_ctx* ctx, int64_t len, const double* a, const double* b, const double* c,
                          int slot0) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, len >= 0);
    if (len == 0) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_res + slot0, 0, 3 * sizeof(double), ctx->stream));
        return MADQP_OK;
    }
    const int nb = grid_for(len);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    hipLaunchKernelGGL(norm_inf3_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, len, a, b, c, ctx->d_part);
    LAUNCH_CHECK(ctx);
    const int ops[3] = {OP_MAX, OP_MAX, OP_MAX};
    return finalize(ctx, nb, 3, ops, slot0);
}

extern "C" int32_t madqp_norm_inf3(madqp_ctx* ctx, int64_t len, const double* a, const double* b,
                                   const double* c, double* out_host) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, len >= 0 && out_host);
    if (len == 0) {
        out_host[0] = out_host[1] = out_host[2] = 0.0;
        return MADQP_OK;
    }
    int32_t r = madqp_q_norm_inf3(ctx, len, a, b, c, 0);
    if (r) return r;
    return madqp_read_results(ctx, 3, out_host);
}

extern "C" int32_t madqp_norm_inf(madqp_ctx* ctx, int64_t len, const double* a, double* out_host) {
    double o[3];
    int32_t r = madqp_norm_inf3(ctx, len, a, nullptr, nullptr, o);
    if (r) return r;
    *out_host = o[0];
    return MADQP_OK;
}

extern "C" int32_t madqp_axpy(madqp_ctx* ctx, int64_t len, double alpha, const double* x, double* y) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, len >= 0 && (len == 0 || (x && y)));
    if (len == 0) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(axpy_kernel, len, len, alpha, x, y);
    return MADQP_OK;
}

extern "C" int32_t madqp_copy(madqp_ctx* ctx, int64_t len, const double* src, double* dst) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, len >= 0 && (len == 0 || (src && dst)));
    if (len == 0) return MADQP_OK;
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, len * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return MADQP_OK;
}

extern "C" int32_t madqp_fill(madqp_ctx* ctx, int64_t len, double value, double* dst) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, len >= 0 && (len == 0 || dst));
    if (len == 0) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(fill_kernel, len, len, value, dst);
    return MADQP_OK;
}

// ------------------------------------------------------------ starting point
extern "C" int32_t madqp_sp_init_duals(madqp_ctx* ctx, const madqp_state* st) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (st->n) LAUNCH(sp_init_duals_kernel, st->n, *st);
    return MADQP_OK;
}

extern "C" int32_t madqp_sp_mins(madqp_ctx* ctx, const madqp_state* st, double* out_host) {
    CHECK_STATE();
    ARG_TRY(ctx, out_host != nullptr);
    const int64_t L = std::max(st->nlb, st->nub);
    if (L == 0) {
        for (int q = 0; q < 4; ++q) out_host[q] = 0.0;
        return MADQP_OK;
    }
    const int nb = grid_for(L);
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        hipLaunchKernelGGL(sp_mins_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, *st, ctx->d_part);
        LAUNCH_CHECK(ctx);
        const int ops[4] = {OP_MIN, OP_MIN, OP_MIN, OP_MIN};
        int32_t r = finalize(ctx, nb, 4, ops);
        if (r) return r;
    }
    return madqp_read_results(ctx, 4, out_host);
}

extern "C" int32_t madqp_sp_shift(madqp_ctx* ctx, const madqp_state* st, double dx, double dz) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (st->nlb) LAUNCH(sp_shift_kernel, st->nlb, st->nlb, st->ind_lb, st->x, dx);
    if (st->nub) LAUNCH(sp_shift_kernel, st->nub, st->nub, st->ind_ub, st->x, -dx);
    if (st->nlb) LAUNCH(sp_shift_kernel, st->nlb, st->nlb, st->ind_lb, st->zl, dz);
    if (st->nub) LAUNCH(sp_shift_kernel, st->nub, st->nub, st->ind_ub, st->zu, dz);
    return MADQP_OK;
}

extern "C" int32_t madqp_sp_sums(madqp_ctx* ctx, const madqp_state* st, double* out_host) {
    CHECK_STATE();
    ARG_TRY(ctx, out_host != nullptr);
    const int64_t L = std::max(st->nlb, st->nub);
    if (L == 0) {
        for (int q = 0; q < 8; ++q) out_host[q] = 0.0;
        return MADQP_OK;
    }
    const int nb = grid_for(L);
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        hipLaunchKernelGGL(sp_sums_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, *st, ctx->d_part);
        LAUNCH_CHECK(ctx);
        const int ops[8] = {OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM};
        int32_t r = finalize(ctx, nb, 8, ops);
        if (r) return r;
    }
    return madqp_read_results(ctx, 8, out_host);
}

extern "C" int32_t madqp_sp_project(madqp_ctx* ctx, const madqp_state* st, double kappa) {
    CHECK_STATE();
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (st->n) LAUNCH(sp_project_kernel, st->n, *st, kappa);
    return MADQP_OK;
}

extern "C" int32_t madqp_sp_check(madqp_ctx* ctx, const madqp_state* st, int32_t* ok_host) {
    CHECK_STATE();
    ARG_TRY(ctx, ok_host != nullptr);
    const int64_t L = std::max(st->nlb, st->nub);
    if (L == 0) {
        *ok_host = 1;
        return MADQP_OK;
    }
    const int nb = grid_for(L);
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        hipLaunchKernelGGL(sp_check_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, *st, ctx->d_part);
        LAUNCH_CHECK(ctx);
        const int ops[1] = {OP_MAX};
        int32_t r = finalize(ctx, nb, 1, ops);
        if (r) return r;
    }
    double bad = 0.0;
    int32_t r = madqp_read_results(ctx, 1, &bad);
    if (r) return r;
    *ok_host = (bad == 0.0) ? 1 : 0;
    return MADQP_OK;
}
