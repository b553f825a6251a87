// Native host driver of one Mehrotra predictor-corrector iteration (src/solver.jl:259-343).
//
// The same control flow as madqp_jl_amd/solver.py (MPCSolver.iteration_head / iteration_body), in
// C++ above the kernels of this library: one foreign call per iteration instead of ~60, so the host
// overhead of an interpreted driver disappears (it matters for small problems and for batches,
// where each host thread drives its own context).
//
// Read-backs.  The sequential form (body_sequential: every reduction returns its scalar at once) makes about
// ten per iteration, thirteen to sixteen with Gondzio corrections.  The fused form (body_fused; AdaptiveStep /
// ConservativeStep) queues the reductions of a phase in the context's result block and fetches the block TWICE per
// iteration, plus once per tried Gondzio correction beyond the first:
//   (b) behind the corrector: factorisation info; residual norms of both solve_system! calls, the predictor's step-length
//       minima and the complementarity sums, from which a one-thread kernel (mpc_mu_kernel) has formed sigma, mu and
//       the step rule's tau ON THE DEVICE -- the corrector's right-hand side and step-length kernels read them there --
//       then the corrector's step-length minima and |dx|  -> SolveException test BEFORE the iterates move; likewise
//       a Gondzio trial's mu_c (mpc_muc_kernel) and, for the FIRST trial, its step lengths min(alpha + delta, 1)
//       (mpc_trial_alpha_kernel): that trial is queued behind the corrector and decided from the same block; a
//       further trial costs the one read-back that decides whether it is kept;
//   (c) behind the update: objective sums and the residual norms of the NEXT termination test (madqp_mpc_head then
//       finds them cached).
// A blocking read-back is a 28 us round trip, and the launches behind it start from an empty queue -- 3.7 us each from
// the host against 1.6 us when they are already queued (tools/launch_probe.cpp) -- ~0.1 ms at n_x = 5 000 each, plus
// the driver's way around the loop behind (c).  Round 5: neither fetch leaves the queue empty any more.  The decisions
// of (b) are ALSO taken by a one-thread kernel (mpc_decide_kernel: the host's arithmetic on the same words), phase
// (c) is queued behind it as kernels that do nothing unless that kernel said "go on" (update_iterates / adjust_boundary
// are the two with side effects; the evaluations behind them recompute what they would have anyway), the block is
// copied to the host behind the decision AND behind (c), and the host waits for the two events: for (b) while (c)
// runs, and for (c) after it has queued the NEXT iteration's set_aug_diagonal_reg! and build_kkt! (their inputs are
// final once (c) has run, the regularisation is host arithmetic; K is rebuilt from scratch every pass, so a loop that
// ends here has lost one assembly).  The host replays every decision from the block and fails loudly if the device's
// differ; where the device said "the host takes over" (failed factorisation or verdict, a second Gondzio trial) the
// iterates have not moved and the round-4 flow continues from the same block.  MADQP_MPC_AHEAD=0: the round-4 form.
// Same kernels, same arithmetic (mpc_rules.inc: each scalar rule is ONE host+device function, which the batched engine
// calls too, the block's fields are named there once), same order on the stream: the iterates are bitwise those of the
// sequential form (tests/test_gpu_solver.py).
// A failed first factorisation (the x100 retries of src/linear_solver.jl:6-17) sends the rest of that iteration down it.
#include <cmath>
#include <cstdlib>

#include "common.h"

struct madqp_mpc {
    madqp_kkt* kkt;
    madqp_ctx* ctx;
    madqp_state st;
    double *w1, *w2;
    const double *q, *rhs;
    double c0, norm_b, norm_c;
    madqp_mpc_options opt;
    // mutable solver scalars (src/structure.jl:60-75)
    double mu, del_w, del_c, alpha_p, alpha_d, obj, inf_pr, inf_du, inf_compl, dnorm, residual_ratio;
    double reg_delta_p, reg_delta_d;  // AdaptiveRegularization state (src/kernels.jl:410-417)
    int64_t k, n_factorizations;
    int32_t last_info;
    bool fused;        // body_fused eligible (options) and not switched off (MADQP_MPC_FUSED=0)
    bool head_cached;  // nrm_cached = the residual norms of the current iterate, read with the last body's block (c)
    double nrm_cached[3];
    int64_t n_readbacks;  // blocking scalar read-backs issued by head/body (reported for DESIGN's count)
    // body_fused, queued ahead of its read-backs (see the head of this file)
    bool ahead;            // MADQP_MPC_AHEAD != 0
    double *h_early, *h_final;  // pinned copies of the result block
    hipEvent_t ev_early, ev_final;
    bool moved;            // a pass has completed since the scalars were set: f, c are those of the current x
    bool prebuilt;         // the NEXT iteration's diagonal and K are already queued, with these regularisations:
    double pre_del_w, pre_del_c;
    int64_t n_prebuilt, n_prebuilt_used;
};

madqp_ctx* madqp_kkt_ctx(madqp_kkt* kkt);  // kkt.hip

namespace {
#define TRY(expr)               \
    do {                        \
        int32_t r_ = (expr);    \
        if (r_) return r_;      \
    } while (0)

int64_t ntot(const madqp_state& s) { return s.n + s.m + s.nlb + s.nub; }

// src/kernels.jl:386-417
MpcReg next_regularization(const madqp_mpc* s) {
    const madqp_mpc_options& o = s->opt;
    return mpc_update_regularization(o.regularization, o.delta_p, o.delta_d, o.delta_min, s->reg_delta_p, s->reg_delta_d);
}
void update_regularization(madqp_mpc* s) {
    const MpcReg r = next_regularization(s);
    s->del_w = r.del_w;
    s->del_c = r.del_c;
    s->reg_delta_p = r.run_p;
    s->reg_delta_d = r.run_d;
}

// src/linear_solver.jl:6-17
int32_t factorize_regularized_system(madqp_mpc* s, int first_trial = 0) {
    for (int trial = first_trial; trial < MPC_FACTOR_TRIALS; ++trial) {
        TRY(madqp_kkt_set_aug_diagonal_reg(s->kkt, &s->st, s->del_w, s->del_c));  // dispatched on the KKT type
        TRY(madqp_kkt_build(s->kkt, &s->st));
        TRY(madqp_kkt_factorize(s->kkt, &s->last_info));
        s->n_factorizations += 1;
        if (s->last_info == 0) break;
        s->del_w = mpc_retry(s->del_w);
        s->del_c = mpc_retry(s->del_c);
    }
    return MADQP_OK;
}

// solve_system! up to its reduction: d = K^-1 p, w1 = p - K d, the three norms into the result block at slot0
int32_t solve_system_queue(madqp_mpc* s, int slot0) {
    const int64_t len = ntot(s->st);
    TRY(madqp_kkt_solve_from(s->kkt, &s->st, s->st.p, s->st.d, s->w1));   // d = K^-1 p, w1 = p
    TRY(madqp_kkt_mul_solved(s->kkt, &s->st, s->w1, s->st.d, -1.0, 1.0));  // d: the solve's result, untouched
    for (int32_t it = 0; it < s->opt.refine_steps; ++it) {  // extension (off by default): d += K^-1 (p - K d)
        TRY(madqp_kkt_solve(s->kkt, &s->st, s->w1));
        TRY(madqp_axpy(s->ctx, len, 1.0, s->w1, s->st.d));
        TRY(madqp_copy(s->ctx, len, s->st.p, s->w1));
        TRY(madqp_kkt_mul(s->kkt, &s->st, s->w1, s->st.d, -1.0, 1.0));
    }
    return madqp_q_norm_inf3(s->ctx, len, s->w1, s->st.p, s->st.d, slot0);
}
int32_t residual_verdict(madqp_mpc* s, const double* nrm) {  // src/linear_solver.jl:36-43
    s->residual_ratio = mpc_residual_ratio(nrm);
    if (mpc_solve_failed(s->residual_ratio, s->opt.check_residual, s->opt.tol_linear_solve))
        return MADQP_NUM_NAN;  // MadNLP.SolveException
    return MADQP_OK;
}
// src/linear_solver.jl:19-45
int32_t solve_system(madqp_mpc* s) {
    TRY(solve_system_queue(s, 0));
    double nrm[MPC_W_NRM];
    TRY(madqp_read_results(s->ctx, MPC_W_NRM, nrm));
    return residual_verdict(s, nrm);
}

// src/kernels.jl:290-305
int32_t fraction_to_boundary(madqp_mpc* s, double tau, double* ap, double* ad, double* a4 = nullptr,
                             int64_t* i4 = nullptr) {
    double a[4];
    int64_t ib[4];
    if (!a4) a4 = a, i4 = ib;
    TRY(madqp_get_alpha_max(s->ctx, &s->st, tau, a4, i4));
    *ap = mpc_min(a4[0], a4[1]);
    *ad = mpc_min(a4[2], a4[3]);
    return MADQP_OK;
}

int32_t read1(madqp_mpc* s, const double* dptr, double* out) {
    return madqp_memcpy_d2h(s->ctx, out, dptr, sizeof(double));
}
int32_t read_idx(madqp_mpc* s, const int64_t* dptr, int64_t* out) {
    return madqp_memcpy_d2h(s->ctx, out, dptr, sizeof(int64_t));
}

// update_step!(::MehrotraAdaptiveStep), src/kernels.jl:325-374 (scalar reads at the blocking indices)
int32_t mehrotra_adaptive_step(madqp_mpc* s) {
    const madqp_state& st = s->st;
    double a[4], max_ap, max_ad, mean, row[2][MPC_ROW_LEN] = {};
    int64_t ib[4];
    TRY(fraction_to_boundary(s, 1.0, &max_ap, &max_ad, a, ib));
    TRY(madqp_get_affine_complementarity_measure(s->ctx, &s->st, max_ap, max_ad, &mean));
    for (int dual = 0; dual < 2; ++dual) {
        const int k = mpc_blocking(a, dual);
        if (k < 0) continue;
        const bool ub = k & 1;
        const int64_t i = ib[k];
        int64_t j;
        TRY(read_idx(s, (ub ? st.ind_ub : st.ind_lb) + i, &j));
        double* r = row[dual];
        TRY(read1(s, st.x + j, r + MPC_ROW_X));
        TRY(read1(s, (ub ? st.xu : st.xl) + j, r + MPC_ROW_BOUND));
        TRY(read1(s, (ub ? st.zu : st.zl) + j, r + MPC_ROW_Z));
        TRY(read1(s, st.d + j, r + MPC_ROW_DX));
        TRY(read1(s, st.d + st.n + st.m + (ub ? st.nlb : 0) + i, r + MPC_ROW_DZ));
    }
    const MpcSteps alpha = mpc_mehrotra_step(a, row[0], row[1], mean, s->opt.step_param);
    s->alpha_p = alpha.p;
    s->alpha_d = alpha.d;
    return MADQP_OK;
}

// src/solver.jl:200-251
int32_t gondzio(madqp_mpc* s, double mu_curr) {
    const int64_t len = ntot(s->st);
    MpcSteps alpha;
    TRY(fraction_to_boundary(s, MPC_GZ_TAU, &alpha.p, &alpha.d));
    for (int c = 0; c < s->opt.max_ncorr; ++c) {
        const MpcSteps ta = mpc_trial_alpha(alpha);
        double ga;
        TRY(madqp_get_affine_complementarity_measure(s->ctx, &s->st, ta.p, ta.d, &ga));
        const double mu = mpc_muc(ga, mu_curr);
        TRY(madqp_set_extra_correction(s->ctx, &s->st, ta.p, ta.d, MPC_GZ_BMIN, MPC_GZ_BMAX, mu));
        TRY(madqp_set_correction_rhs(s->ctx, &s->st, mu));
        TRY(madqp_copy(s->ctx, len, s->st.d, s->w2));
        TRY(solve_system(s));
        MpcSteps ha;
        TRY(fraction_to_boundary(s, MPC_GZ_TAU, &ha.p, &ha.d));
        if (mpc_trial_dropped(ha, alpha)) {
            TRY(madqp_copy(s->ctx, len, s->w2, s->st.d));
            break;
        }
        alpha = ha;
    }
    return MADQP_OK;
}

void fill_info(const madqp_mpc* s, madqp_mpc_info* i) {
    if (!i) return;
    i->k = s->k;
    i->obj = s->obj;
    i->inf_pr = s->inf_pr;
    i->inf_du = s->inf_du;
    i->inf_compl = s->inf_compl;
    i->mu = s->mu;
    i->dnorm = s->dnorm;
    i->del_w = s->del_w;
    i->del_c = s->del_c;
    i->alpha_p = s->alpha_p;
    i->alpha_d = s->alpha_d;
    i->residual_ratio = s->residual_ratio;
    i->n_factorizations = s->n_factorizations;
    i->factor_info = s->last_info;
}
}  // namespace

extern "C" int32_t madqp_mpc_create(madqp_kkt* kkt, const madqp_state* st, double* w1, double* w2,
                                    const double* q, const double* rhs, double c0, double norm_b,
                                    double norm_c, const madqp_mpc_options* opt, madqp_mpc** out) {
    if (!kkt || !out) return MADQP_ERR_ARG;
    madqp_ctx* ctx = madqp_kkt_ctx(kkt);
    ARG_TRY(ctx, st && opt && (ntot(*st) == 0 || (w1 && w2)));
    ARG_TRY(ctx, opt->step_rule >= 0 && opt->step_rule <= 2 && opt->regularization >= 0 &&
                     opt->regularization <= 2 && opt->max_ncorr >= 0);
    madqp_mpc* s = new (std::nothrow) madqp_mpc();
    if (!s) return madqp_fail(ctx, MADQP_ERR_ALLOC, "host allocation failed");
    memset(s, 0, sizeof(*s));
    s->kkt = kkt;
    s->ctx = ctx;
    s->st = *st;
    s->w1 = w1;
    s->w2 = w2;
    s->q = q;
    s->rhs = rhs;
    s->c0 = c0;
    s->norm_b = norm_b;
    s->norm_c = norm_c;
    s->opt = *opt;
    s->reg_delta_p = opt->delta_p;
    s->reg_delta_d = opt->delta_d;
    const char* env = getenv("MADQP_MPC_FUSED");  // 0: the sequential form (A/B tests)
    s->fused = !(env && env[0] == '0') && opt->step_rule != 2;
    env = getenv("MADQP_MPC_AHEAD");  // 0: body_fused waits for its read-backs with nothing queued behind them (A/B tests)
    s->ahead = s->fused && !(env && env[0] == '0');
    if (s->ahead) {
        hipError_t e = hipHostMalloc((void**)&s->h_early, 2 * MADQP_RESULT_SLOTS * sizeof(double), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_early, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_final, hipEventDisableTiming);
        if (e != hipSuccess) {
            madqp_mpc_destroy(s);
            return madqp_fail(ctx, MADQP_ERR_HIP, "madqp_mpc_create: %s", hipGetErrorString(e));
        }
        s->h_final = s->h_early + MADQP_RESULT_SLOTS;
    }
    *out = s;
    return MADQP_OK;
}

extern "C" int32_t madqp_mpc_destroy(madqp_mpc* s) {
    if (s) {
        if (s->ev_early) (void)hipEventDestroy(s->ev_early);
        if (s->ev_final) (void)hipEventDestroy(s->ev_final);
        if (s->h_early) (void)hipHostFree(s->h_early);
    }
    delete s;
    return MADQP_OK;
}

extern "C" int32_t madqp_mpc_set_scalars(madqp_mpc* s, double mu, double del_w, double del_c, double obj,
                                         int64_t k) {
    if (!s) return MADQP_ERR_ARG;
    s->mu = mu;
    s->del_w = del_w;
    s->del_c = del_c;
    s->obj = obj;
    s->k = k;
    s->head_cached = false;
    s->prebuilt = false;
    s->moved = false;
    return MADQP_OK;
}

// src/solver.jl:259-283: residuals and the termination test.
// status_host: MPC_ST_ACTIVE = continue, MPC_ST_SOLVED = SOLVE_SUCCEEDED, MPC_ST_MAXITER = MAXIMUM_ITERATIONS_EXCEEDED
extern "C" int32_t madqp_mpc_head(madqp_mpc* s, madqp_mpc_info* info_host, int32_t* status_host) {
    if (!s || !status_host) return MADQP_ERR_ARG;
    double nrm[3];
    if (s->head_cached) {  // read with the last body's block (c): same iterate, same kernels
        for (int q = 0; q < 3; ++q) nrm[q] = s->nrm_cached[q];
    } else {
        TRY(madqp_kkt_jtprod(s->kkt, s->st.jacl, s->st.y));
        TRY(madqp_get_inf(s->ctx, &s->st, nrm));
        s->n_readbacks += 1;
    }
    const MpcHead h = mpc_head(nrm, s->norm_b, s->norm_c, s->opt.tol, s->k, s->opt.max_iter);
    s->inf_pr = h.inf_pr;
    s->inf_du = h.inf_du;
    s->inf_compl = h.inf_compl;
    fill_info(s, info_host);
    *status_host = h.status;
    return MADQP_OK;
}

namespace {
// src/solver.jl:294-343 behind a successful factorisation, every reduction read back at once
int32_t body_after_factorization(madqp_mpc* s, madqp_mpc_info* info_host) {
    madqp_ctx* ctx = s->ctx;
    TRY(madqp_set_predictive_rhs(ctx, &s->st)); // :294
    TRY(solve_system(s));
    double a_aff_p, a_aff_d, mu_affine, mu_curr;
    TRY(fraction_to_boundary(s, 1.0, &a_aff_p, &a_aff_d));  // :295
    TRY(madqp_get_affine_complementarity_measure(ctx, &s->st, a_aff_p, a_aff_d, &mu_affine));  // :296
    TRY(madqp_get_correction(ctx, &s->st));     // :297
    // update_barrier!(Mehrotra), src/kernels.jl:226-236 (field-order quirk: "any bound")
    TRY(madqp_get_complementarity_measure(ctx, &s->st, &mu_curr));
    const MpcBarrier bar = mpc_barrier(mu_affine, mu_curr, (double)(s->st.nlb + s->st.nub), s->opt.mu_min, s->opt.step_rule,
                                       s->opt.step_param);
    s->mu = bar.mu;
    TRY(madqp_set_correction_rhs(ctx, &s->st, s->mu));  // :307
    TRY(solve_system(s));
    if (s->opt.max_ncorr > 0) TRY(gondzio(s, mu_curr));  // :316-324
    // update_step!, src/kernels.jl:307-374
    if (s->opt.step_rule == 2) {
        TRY(mehrotra_adaptive_step(s));
    } else {
        TRY(fraction_to_boundary(s, bar.tau, &s->alpha_p, &s->alpha_d));
    }
    TRY(madqp_norm_inf(ctx, s->st.n, s->st.d, &s->dnorm));             // print_iter, src/structure.jl:190
    TRY(madqp_update_iterates(ctx, &s->st, s->alpha_p, s->alpha_d));   // :332-335
    TRY(madqp_kkt_eval(s->kkt, &s->st, s->q, s->rhs, s->c0, &s->obj)); // :338-340
    TRY(madqp_adjust_boundary(ctx, &s->st, s->mu));                    // :342
    s->k += 1;
    fill_info(s, info_host);
    return MADQP_OK;
}

int32_t body_sequential(madqp_mpc* s, madqp_mpc_info* info_host) {
    update_regularization(s);                   // :288
    TRY(factorize_regularized_system(s));       // :289
    return body_after_factorization(s, info_host);
}

// One Gondzio trial, queued (src/solver.jl:216-230): mu_c formed on the device from the trial's affine sums, the
// direction before it saved in w2, and behind the solve the trial block at `base` (MpcTrialBlock).  The trial's step
// lengths min(alpha + delta, 1) are read on the device from ta_dev (TRIAL_ALPHA: the first trial) or, with nullptr, are ta.
int32_t queue_gondzio_trial(madqp_mpc* s, const double* ta_dev, MpcSteps ta, int compl_slot, int base) {
    madqp_ctx* ctx = s->ctx;
    const double* res = ctx->d_res;
    TRY(madqp_q_compl(ctx, &s->st, 1, ta.p, ta.d, ta_dev, compl_slot));
    TRY(madqp_q_mpc_muc(ctx, compl_slot, s->st.nlb + s->st.nub));
    TRY(madqp_set_extra_correction_dev(ctx, &s->st, ta.p, ta.d, MPC_GZ_BMIN, MPC_GZ_BMAX, res + MPC_SL_MUC, ta_dev));
    TRY(madqp_set_correction_rhs_dev(ctx, &s->st, res + MPC_SL_MUC));
    TRY(madqp_copy(ctx, ntot(s->st), s->st.d, s->w2));
    TRY(solve_system_queue(s, base + MPC_TRIAL.nrm));
    TRY(madqp_q_alpha_max(ctx, &s->st, MPC_GZ_TAU, base + MPC_TRIAL.alpha_gz));
    TRY(madqp_q_alpha_max_dev(ctx, &s->st, 0.0, res + MPC_SL_TAU, base + MPC_TRIAL.alpha_tau));
    return madqp_q_norm_inf3(ctx, s->st.n, s->st.d, nullptr, nullptr, base + MPC_TRIAL.dnorm);  // print_iter, src/structure.jl:190
}

// Phase (c), queued: the update of the iterates, the model at the new point and the residual norms of the next
// termination test into PHASE_C.  dec: the DECISION words in device memory -- the two kernels with side effects do nothing
// unless they say "go on" and take their scalars from the block, and a dropped trial's direction comes back first -- or
// nullptr: the host has decided (s->alpha_p, s->alpha_d, s->mu).
int32_t queue_phase_c(madqp_mpc* s, const double* dec) {
    madqp_ctx* ctx = s->ctx;
    if (dec && s->opt.max_ncorr > 0) TRY(madqp_copy_if_dev(ctx, ntot(s->st), s->w2, s->st.d, dec + MPC_DEC_RESTORE));
    TRY(madqp_update_iterates_dev(ctx, &s->st, s->alpha_p, s->alpha_d, dec));                        // :332-335
    TRY(madqp_q_kkt_eval(s->kkt, &s->st, s->q, s->rhs, MPC_SL_OBJ_LIN));                              // :338-340
    TRY(madqp_adjust_boundary_dev(ctx, &s->st, s->mu, dec, dec ? ctx->d_res + MPC_SL_MU : nullptr));  // :342
    TRY(madqp_kkt_jtprod(s->kkt, s->st.jacl, s->st.y));                                               // :259-283 of the next pass
    TRY(madqp_q_inf(ctx, &s->st, MPC_SL_INF));
    if (s->ahead) TRY(madqp_results_post(ctx, s->h_final, s->ev_final));
    return MADQP_OK;
}

// The same iteration with two blocking read-backs (see the head of this file).
int32_t body_fused(madqp_mpc* s, madqp_mpc_info* info_host) {
    madqp_ctx* ctx = s->ctx;
    const double* res = ctx->d_res;
    const bool gz = s->opt.max_ncorr > 0;
    update_regularization(s);  // :288
    // (a) factorisation and predictor
    const bool have_k = s->prebuilt && s->pre_del_w == s->del_w && s->pre_del_c == s->del_c;  // queued by the last pass
    s->prebuilt = false;
    if (have_k) {
        s->n_prebuilt_used += 1;
    } else {
        TRY(madqp_kkt_set_aug_diagonal_reg(s->kkt, &s->st, s->del_w, s->del_c));
        TRY(madqp_kkt_build(s->kkt, &s->st));
    }
    TRY(madqp_q_kkt_factorize(s->kkt, MPC_SL_INFO));
    s->n_factorizations += 1;
    TRY(madqp_set_predictive_rhs(ctx, &s->st));                                                   // :294
    TRY(solve_system_queue(s, MPC_SL_PRED_NRM));
    TRY(madqp_q_alpha_max(ctx, &s->st, 1.0, MPC_SL_PRED_ALPHA));                                  // :295
    TRY(madqp_q_compl(ctx, &s->st, 1, 0.0, 0.0, res + MPC_SL_PRED_ALPHA, MPC_SL_COMPL));          // :296, step lengths from the block
    TRY(madqp_get_correction(ctx, &s->st));                                                       // :297
    TRY(madqp_q_compl(ctx, &s->st, 0, 0.0, 0.0, nullptr, MPC_SL_COMPL + MPC_W_COMPL));
    // update_barrier! on the device, into BARRIER: the corrector is queued behind the predictor without a read-back
    TRY(madqp_q_mpc_mu(ctx, s->st.nlb + s->st.nub, s->opt.mu_min, s->opt.step_rule, s->opt.step_param));
    // (b) corrector.  The step rule's minima and |dx| are queued behind every direction that may turn out to be the
    // final one, so that the Gondzio loop below ends without a read-back of its own.
    TRY(madqp_set_correction_rhs_dev(ctx, &s->st, res + MPC_SL_MU));  // :307
    TRY(solve_system_queue(s, MPC_SL_CORR_NRM));
    TRY(madqp_q_alpha_max_dev(ctx, &s->st, 0.0, res + MPC_SL_TAU, MPC_SL_CORR_ALPHA));
    TRY(madqp_q_norm_inf3(ctx, s->st.n, s->st.d, nullptr, nullptr, MPC_SL_CORR_DNORM));  // print_iter, src/structure.jl:190
    // gondzio(), first trial: queued behind the corrector, its step lengths and its mu_c formed on the device from the
    // block -- the read-back that follows serves the corrector AND the trial
    if (gz) {
        TRY(madqp_q_alpha_max(ctx, &s->st, MPC_GZ_TAU, MPC_SL_GZ_ALPHA));
        TRY(madqp_q_mpc_trial_alpha(ctx));
        TRY(queue_gondzio_trial(s, res + MPC_SL_TRIAL_ALPHA, MpcSteps{0.0, 0.0}, MPC_SL_TRIAL_COMPL, MPC_SL_TRIAL));
    }
    // Queued ahead: the decisions of the read-back below on the device too (DECISION) and phase (c) behind them; the
    // block travels to the host behind the decision (the host waits for THAT copy while the update runs) and behind (c).
    // (Not in the first pass behind the start point: f and c are then the values initialize! left, from BEFORE the start
    // point moved x -- src/solver.jl:100-146 -- and an evaluation queued ahead would refresh them even where the host
    // takes over and the reference's loop goes on with the stale ones.)
    double rb[MADQP_RESULT_SLOTS];
    const bool spec = s->ahead && s->moved;
    if (spec) {
        const MpcDecideOpt opt{gz ? 1 : 0, s->opt.max_ncorr, s->opt.check_residual ? 1 : 0, s->opt.tol_linear_solve};
        TRY(madqp_q_mpc_decide(ctx, opt));
        TRY(madqp_results_post(ctx, s->h_early, s->ev_early));
        TRY(queue_phase_c(s, res + MPC_SL_DECISION));
        TRY(madqp_results_wait(ctx, s->h_early, s->ev_early, MPC_READ_DECISION, rb));
    } else {
        TRY(madqp_read_results(ctx, gz ? MPC_READ_FIRST_TRIAL : MPC_READ_CORRECTOR, rb));
    }
    s->n_readbacks += 1;
    // The host's replay of (b) from the block, with the rules the device used
    const double* dec = rb + MPC_SL_DECISION;
    const bool went = spec && dec[MPC_DEC_GO] != 0.0;  // the device has gone on: the host's decisions must be the same
    auto differ = [&]() {
        return madqp_fail(ctx, MADQP_ERR_HIP, "body_fused: the device's decisions behind the corrector are not the host's");
    };
    auto verdict = [&](const double* nrm) {  // of a solve_system! call; a failed one cannot be behind a "go on"
        const int32_t v = residual_verdict(s, nrm);
        return (v && went) ? differ() : v;
    };
    s->last_info = (int32_t)rb[MPC_SL_INFO];
    if (s->last_info != 0) {  // src/linear_solver.jl:6-17: what was queued behind the failed factorisation is void
        if (went) return differ();
        s->del_w = mpc_retry(s->del_w);
        s->del_c = mpc_retry(s->del_c);
        TRY(factorize_regularized_system(s, 1));
        return body_after_factorization(s, info_host);
    }
    TRY(verdict(rb + MPC_SL_PRED_NRM));  // the predictor's solve
    s->mu = rb[MPC_SL_MU];
    TRY(verdict(rb + MPC_SL_CORR_NRM));  // the corrector's
    auto take_step = [&](const double* a8, const double* dnorm) {  // update_step! from the block of the direction that stays
        const MpcSteps a = mpc_steps(a8);
        s->alpha_p = a.p;
        s->alpha_d = a.d;
        s->dnorm = *dnorm;
    };
    take_step(rb + MPC_SL_CORR_ALPHA, rb + MPC_SL_CORR_DNORM);
    if (gz) {  // the first trial is in the block; a further one (while the last was kept) costs a read-back of its own
        MpcSteps g = mpc_steps(rb + MPC_SL_GZ_ALPHA);
        const double* tb = rb + MPC_SL_TRIAL;
        double tr[MPC_READ_LATER_TRIAL];
        for (int c = 0; c < s->opt.max_ncorr; ++c) {
            if (c > 0) {
                if (went) return differ();
                TRY(queue_gondzio_trial(s, nullptr, mpc_trial_alpha(g), MPC_SL_LATER_COMPL, MPC_SL_LATER_TRIAL));
                TRY(madqp_read_results(ctx, MPC_READ_LATER_TRIAL, tr));
                s->n_readbacks += 1;
                tb = tr + MPC_SL_LATER_TRIAL;
            }
            TRY(verdict(tb + MPC_TRIAL.nrm));
            const MpcSteps h = mpc_steps(tb + MPC_TRIAL.alpha_gz);
            if (mpc_trial_dropped(h, g)) {
                if (went) {
                    if (dec[MPC_DEC_RESTORE] == 0.0) return differ();  // (the device has put the direction back itself)
                } else {
                    TRY(madqp_copy(ctx, ntot(s->st), s->w2, s->st.d));  // the direction before it, whose step is already known
                }
                break;
            }
            if (went && c == 0 && dec[MPC_DEC_RESTORE] != 0.0) return differ();
            g = h;
            take_step(tb + MPC_TRIAL.alpha_tau, tb + MPC_TRIAL.dnorm);
        }
    }
    if (went && (dec[MPC_DEC_ALPHA_P] != s->alpha_p || dec[MPC_DEC_ALPHA_D] != s->alpha_d)) return differ();
    // (c) update, objective, and the residuals the next termination test needs
    if (!went) TRY(queue_phase_c(s, nullptr));
    if (s->ahead) {
        // Queue the NEXT iteration's diagonal and assembly before waiting for the norms (see the head of this file) -- not
        // when this pass is the last one allowed, nor when the iterate it started from was already within 100 x the
        // tolerance: the loop then usually ends behind this pass or the next, and the assembly would be for nobody
        if (mpc_queue_next_assembly({s->inf_pr, s->inf_du, s->inf_compl, MPC_ST_ACTIVE}, s->opt.tol, s->k, s->opt.max_iter)) {
            const MpcReg nx = next_regularization(s);  // the regularisation of the next pass; the scalars stay
            TRY(madqp_kkt_set_aug_diagonal_reg(s->kkt, &s->st, nx.del_w, nx.del_c));
            TRY(madqp_kkt_build(s->kkt, &s->st));
            s->prebuilt = true;
            s->pre_del_w = nx.del_w;
            s->pre_del_c = nx.del_c;
            s->n_prebuilt += 1;
        }
        TRY(madqp_results_wait(ctx, s->h_final, s->ev_final, MPC_READ_FINAL, rb));
    } else {
        TRY(madqp_read_results(ctx, MPC_READ_FINAL, rb));
    }
    s->moved = true;
    s->k += 1;
    s->n_readbacks += 1;
    s->obj = mpc_objective(s->c0, rb[MPC_SL_OBJ_LIN], rb[MPC_SL_OBJ_QUAD]);
    madqp_inf_from_block(rb + MPC_SL_INF, s->nrm_cached);
    s->head_cached = true;
    fill_info(s, info_host);
    return MADQP_OK;
}
}  // namespace

// src/solver.jl:288-343: one predictor-corrector step.  Returns MADQP_NUM_NAN for the
// SolveException of src/linear_solver.jl:41-43.
extern "C" int32_t madqp_mpc_body(madqp_mpc* s, madqp_mpc_info* info_host) {
    if (!s) return MADQP_ERR_ARG;
    s->head_cached = false;
    if (!s->fused) return body_sequential(s, info_host);
    const int32_t r = body_fused(s, info_host);
    if (r) s->prebuilt = false;
    return r;
}

extern "C" int32_t madqp_mpc_readbacks(const madqp_mpc* s, int64_t* count) {
    if (!s || !count) return MADQP_ERR_ARG;
    *count = s->n_readbacks;
    return MADQP_OK;
}

extern "C" int32_t madqp_mpc_ahead_stats(const madqp_mpc* s, int64_t* queued, int64_t* used) {
    if (!s || !queued || !used) return MADQP_ERR_ARG;
    *queued = s->n_prebuilt;
    *used = s->n_prebuilt_used;
    return MADQP_OK;
}
