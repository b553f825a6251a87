// What the two native drivers of an interior-point iteration share, each written once: the host driver of one problem
// (mpc.hip, with the one-thread kernels of vec_kernels.hip) and the workgroup programs of the batched engine
// (batch_wg.inc, batch.hip).  Two parts: where every scalar of a fused iteration lies in the context's result block, and
// the scalar rules of the iteration, the start point included (src/kernels.jl, src/solver.jl, src/linear_solver.jl).
// Plain C++17, no HIP call and no context: host and device call the same functions, tests/csrc compiles them for the CPU
// and tests/test_mpc_rules.py holds them to oracle/mpc.py without a GPU.  Needs MADQP_FAULT_SLOT (common.h).
//
// Bits.  min and max are explicit comparisons in the operand order of std::min / std::max (what solver.py, oracle/mpc.py
// and the reference do with a NaN too); a driver that calls a rule therefore takes that order, not fmin / fmax's.  The
// library and the test build compile with -ffp-contract=off, so an expression gives the same bits inside a function as
// written out at its call site, on the host and on the device.
#pragma once
#ifdef __HIPCC__
#define MPC_HOST_DEVICE __host__ __device__
#else
#define MPC_HOST_DEVICE
#endif

// ---- layout -----------------------------------------------------------------------------------------------------------
// slots the queued reductions write (common.h, madqp_q_*)
enum { MPC_W_NRM = 3, MPC_W_ALPHA = 8, MPC_W_COMPL = 2, MPC_W_INF = 4, MPC_W_EVAL = 2, MPC_W_INFO = 1 };

// What one Gondzio trial leaves behind, as offsets from its base: solve_system!'s norms, the step-length minima at
// Gondzio's tau (keep or drop) and at the step rule's tau (the step, should this direction be the last), |dx|
struct MpcTrialBlock { int nrm, alpha_gz, alpha_tau, dnorm, width; };
constexpr MpcTrialBlock MPC_TRIAL{0, MPC_W_NRM, MPC_W_NRM + MPC_W_ALPHA, MPC_W_NRM + 2 * MPC_W_ALPHA,
                                  2 * MPC_W_NRM + 2 * MPC_W_ALPHA};

// name, first slot, width -- in ascending order (checked below)
#define MPC_FIELDS(X)                                                                                                 \
    X(PRED_NRM, 0, MPC_W_NRM)           /* predictor: norms of its solve_system! */                                   \
    X(PRED_ALPHA, 3, MPC_W_ALPHA)       /*   step-length minima at tau = 1 */                                         \
    X(COMPL, 11, 2 * MPC_W_COMPL)       /*   complementarity sums: affine, then current */                            \
    X(INFO, 15, MPC_W_INFO)             /* factorisation info */                                                      \
    X(BARRIER, 32, 3)                   /* update_barrier! on the device: mu, the step rule's tau, mu_curr */         \
    X(CORR_NRM, 35, MPC_W_NRM)          /* corrector: norms */                                                        \
    X(CORR_ALPHA, 38, MPC_W_ALPHA)      /*   step-length minima at the rule's tau */                                  \
    X(CORR_DNORM, 46, MPC_W_NRM)        /*   |dx| (first word) */                                                     \
    X(GZ_ALPHA, 49, MPC_W_ALPHA)        /* Gondzio: the corrector's minima at Gondzio's tau */                        \
    X(MUC, 58, 1)                       /*   mu_c of the trial being queued */                                        \
    X(TRIAL_ALPHA, 64, MPC_W_ALPHA)     /*   the first trial's min(alpha + delta, 1), in the 8-slot pattern */        \
    X(TRIAL_COMPL, 72, MPC_W_COMPL)     /*   its affine sums */                                                       \
    X(TRIAL, 74, MPC_TRIAL.width)       /*   its trial block */                                                       \
    X(DECISION, 100, 4)                 /* mpc_decide: go, alpha_p, alpha_d, restore */                               \
    X(PHASE_C, 106, MPC_W_EVAL + MPC_W_INF) /* behind the update: objective sums, the next termination test's norms */

#define MPC_X_ENUM(name, first, width) MPC_SL_##name = (first), MPC_N_##name = (width),
enum {
    MPC_FIELDS(MPC_X_ENUM)
    MPC_SL_MU = MPC_SL_BARRIER, MPC_SL_TAU, MPC_SL_MUCURR,
    MPC_DEC_GO = 0, MPC_DEC_ALPHA_P, MPC_DEC_ALPHA_D, MPC_DEC_RESTORE,  // offsets in DECISION
    MPC_SL_OBJ_LIN = MPC_SL_PHASE_C, MPC_SL_OBJ_QUAD, MPC_SL_INF = MPC_SL_OBJ_LIN + MPC_W_EVAL,  // obj = c0 + lin + quad / 2
    // a further trial is queued when the host has read the block: its sums and its trial block reuse the predictor's slots
    MPC_SL_LATER_COMPL = MPC_SL_PRED_NRM, MPC_SL_LATER_TRIAL = MPC_SL_PRED_NRM
};
#undef MPC_X_ENUM

struct MpcField { const char* name; int first, width; };
#define MPC_X_ROW(name, first, width) {#name, (first), (width)},
constexpr MpcField MPC_LAYOUT[] = {MPC_FIELDS(MPC_X_ROW)};
#undef MPC_X_ROW
constexpr int MPC_NFIELDS = sizeof(MPC_LAYOUT) / sizeof(MPC_LAYOUT[0]);
constexpr bool mpc_layout_ok() {
    int end = 0;
    for (int i = 0; i < MPC_NFIELDS; ++i) {
        if (MPC_LAYOUT[i].width <= 0 || MPC_LAYOUT[i].first < end) return false;
        end = MPC_LAYOUT[i].first + MPC_LAYOUT[i].width;
    }
    return end <= MADQP_FAULT_SLOT;
}
static_assert(mpc_layout_ok(), "result-block fields overlap or reach the fault word");
// a further trial must leave alone what is still read on the device when it runs: mu_curr, tau, mu_c
static_assert(MPC_SL_LATER_TRIAL + MPC_TRIAL.width <= MPC_SL_BARRIER, "a later Gondzio trial overwrites the barrier block");

// Words the host reads from each copy of the block (the `count` of madqp_read_results / madqp_results_wait)
constexpr int MPC_READ_CORRECTOR = MPC_SL_CORR_DNORM + MPC_N_CORR_DNORM; // behind the corrector, no Gondzio trial
constexpr int MPC_READ_FIRST_TRIAL = MPC_SL_TRIAL + MPC_N_TRIAL;      // ... with the first trial queued behind it
constexpr int MPC_READ_DECISION = MPC_SL_DECISION + MPC_N_DECISION;   // ... and the device's decisions
constexpr int MPC_READ_LATER_TRIAL = MPC_SL_LATER_TRIAL + MPC_TRIAL.width;
constexpr int MPC_READ_FINAL = MPC_SL_PHASE_C + MPC_N_PHASE_C;

// ---- rules ------------------------------------------------------------------------------------------------------------
MPC_HOST_DEVICE inline double mpc_min(double a, double b) { return (b < a) ? b : a; }  // std::min(a, b)
MPC_HOST_DEVICE inline double mpc_max(double a, double b) { return (a < b) ? b : a; }  // std::max(a, b)
// solve_system!'s verdict (src/linear_solver.jl:36-43) from the norms |p - K d|, |p|: true = MadNLP.SolveException
MPC_HOST_DEVICE inline double mpc_residual_ratio(const double* nrm) { return nrm[0] / mpc_max(1.0, nrm[1]); }
MPC_HOST_DEVICE inline bool mpc_solve_failed(double ratio, int check_residual, double tol_linear_solve) {
    return ratio != ratio || (check_residual && ratio > tol_linear_solve);
}
// get_fraction_to_boundary_step (src/kernels.jl:290-305) from the 8-slot block (value, index) of {xl, xu, zl, zu}
struct MpcSteps { double p, d; };
MPC_HOST_DEVICE inline MpcSteps mpc_steps(const double* a8) { return {mpc_min(a8[0], a8[2]), mpc_min(a8[4], a8[6])}; }
// get_complementarity_measure from its two sums (src/kernels.jl:173-174: 0 without bounds)
MPC_HOST_DEVICE inline double mpc_compl_mean(const double* sums2, double nb) {
    return nb > 0.0 ? (sums2[0] + sums2[1]) / nb : 0.0;
}

// update_barrier!(Mehrotra) (src/kernels.jl:226-236; sigma = (mu_aff / mu_curr)^3 as t*t*t, Julia's literal power) and
// the tau of update_step! for ConservativeStep (0) and AdaptiveStep (1) (src/kernels.jl:307-323)
struct MpcBarrier { double mu, tau, mu_curr; };
MPC_HOST_DEVICE inline double mpc_step_tau(double mu, int step_rule, double step_param) {
    return step_rule == 0 ? step_param : mpc_max(1.0 - mu, step_param);
}
MPC_HOST_DEVICE inline MpcBarrier mpc_barrier(double mu_affine, double mu_curr, double nb, double mu_min, int step_rule,
                                              double step_param) {
    double sigma = 1.0;
    if (nb > 0.0) {
        const double t = mu_affine / mu_curr;
        sigma = mpc_min(mpc_max(t * t * t, 1e-6), 10.0);
    }
    const double mu = mpc_max(mu_min, sigma * mu_curr);
    return {mu, mpc_step_tau(mu, step_rule, step_param), mu_curr};
}
// ... from the COMPL sums into the BARRIER words
MPC_HOST_DEVICE inline void mpc_barrier_block(const double* sums4, double nb, double mu_min, int step_rule,
                                              double step_param, double* out3) {
    const MpcBarrier b = mpc_barrier(mpc_compl_mean(sums4, nb), mpc_compl_mean(sums4 + MPC_W_COMPL, nb), nb, mu_min,
                                     step_rule, step_param);
    out3[0] = b.mu;
    out3[1] = b.tau;
    out3[2] = b.mu_curr;
}

// gondzio_correction_direction! (src/solver.jl:200-251)
constexpr double MPC_GZ_DELTA = 0.1, MPC_GZ_BMIN = 0.1, MPC_GZ_BMAX = 10.0, MPC_GZ_TAU = 0.995, MPC_GZ_KEEP = 1.005;
MPC_HOST_DEVICE inline MpcSteps mpc_trial_alpha(MpcSteps a) {
    return {mpc_min(a.p + MPC_GZ_DELTA, 1.0), mpc_min(a.d + MPC_GZ_DELTA, 1.0)};
}
// ... from a step-length block into the pattern the step-length readers take (mpc_steps of out8 gives them back)
MPC_HOST_DEVICE inline void mpc_trial_alpha_block(const double* a8, double* out8) {
    const MpcSteps t = mpc_trial_alpha(mpc_steps(a8));
    out8[0] = out8[2] = t.p;
    out8[4] = out8[6] = t.d;
}
MPC_HOST_DEVICE inline double mpc_muc(double ga, double mu_curr) { return (ga / mu_curr) * (ga / mu_curr) * ga; }
// the trial's direction is dropped (and the one before it comes back) unless both step lengths grew by 0.5 %
MPC_HOST_DEVICE inline bool mpc_trial_dropped(MpcSteps trial, MpcSteps before) {
    return trial.p < MPC_GZ_KEEP * before.p || trial.d < MPC_GZ_KEEP * before.d;
}

// The decisions body_fused takes from its read-back behind the corrector, for the device to take them too (the update of
// the iterates is queued behind them without waiting for that read-back): both verdicts, the step lengths and, with
// Gondzio corrections, whether the first trial is kept.  out4 (DECISION): go = 1: the iteration goes on as queued (0: the
// host takes over -- failed factorisation, failed verdict, or a further trial to run); alpha_p, alpha_d; restore = 1:
// the trial's direction is dropped, the one saved before it comes back.  blk and out4 may be the same block.
struct MpcDecideOpt { int gondzio, max_ncorr, check_residual; double tol_linear_solve; };
MPC_HOST_DEVICE inline void mpc_decide(const double* blk, const MpcDecideOpt& o, double* out4) {
    auto failed = [&](const double* nrm) {
        return mpc_solve_failed(mpc_residual_ratio(nrm), o.check_residual, o.tol_linear_solve);
    };
    bool go = blk[MPC_SL_INFO] == 0.0 && !failed(blk + MPC_SL_PRED_NRM) && !failed(blk + MPC_SL_CORR_NRM);
    MpcSteps a = mpc_steps(blk + MPC_SL_CORR_ALPHA);
    bool restore = false;
    if (o.gondzio) {
        const double* tb = blk + MPC_SL_TRIAL;
        go = go && !failed(tb + MPC_TRIAL.nrm);
        if (mpc_trial_dropped(mpc_steps(tb + MPC_TRIAL.alpha_gz), mpc_steps(blk + MPC_SL_GZ_ALPHA))) {
            restore = go;
        } else {
            a = mpc_steps(tb + MPC_TRIAL.alpha_tau);
            if (o.max_ncorr > 1) go = false;  // the next trial is the host's to queue
        }
    }
    out4[MPC_DEC_GO] = go ? 1.0 : 0.0;
    out4[MPC_DEC_ALPHA_P] = a.p;
    out4[MPC_DEC_ALPHA_D] = a.d;
    out4[MPC_DEC_RESTORE] = restore ? 1.0 : 0.0;
}

// ---- rules of both drivers: loop head, regularisation, step, model --------------------------------------------------
// Status words of the loop (MadNLP's, as madqp_mpc_head's status_host and madqp_batch_results report them)
enum { MPC_ST_ACTIVE = 0, MPC_ST_SOLVED = 1, MPC_ST_MAXITER = 6, MPC_ST_STEP_ERROR = -3, MPC_ST_INTERNAL = -1 };

// get_optimality_gap from the two maxima the reduction kernels leave (vec_kernels.inc: a NaN on either side stays)
MPC_HOST_DEVICE inline double mpc_nanmax(double a, double b) { return (a != a) ? a : ((b != b) ? b : mpc_max(a, b)); }
MPC_HOST_DEVICE inline double mpc_max3(double a, double b, double c) { return mpc_max(mpc_max(a, b), c); }  // max(a, b, c)
// src/solver.jl:264-283 from |c|, the dual residual and the optimality gap: scaled infeasibilities, termination test
struct MpcHead { double inf_pr, inf_du, inf_compl; int status; };
MPC_HOST_DEVICE inline MpcHead mpc_head(const double* nrm3, double norm_b, double norm_c, double tol, long long k,
                                        long long max_iter) {
    MpcHead h{nrm3[0] / mpc_max(1.0, norm_b), nrm3[1] / mpc_max(1.0, norm_c), nrm3[2] / mpc_max(1.0, norm_c), MPC_ST_ACTIVE};
    if (mpc_max3(h.inf_pr, h.inf_du, h.inf_compl) <= tol)
        h.status = MPC_ST_SOLVED;
    else if (k >= max_iter)
        h.status = MPC_ST_MAXITER;
    return h;
}
// mpc.hip only: the next pass's assembly is queued ahead unless this pass is the last one allowed or the iterate it
// started from was already within 100 x the tolerance (the loop then usually ends behind this pass or the next)
MPC_HOST_DEVICE inline bool mpc_queue_next_assembly(const MpcHead& h, double tol, long long k, long long max_iter) {
    return k + 1 < max_iter && !(mpc_max3(h.inf_pr, h.inf_du, h.inf_compl) <= 100.0 * tol);
}

// init_regularization! and update_regularization! (src/kernels.jl:380-417).  mode: 0 No-, 1 Fixed-, 2 AdaptiveRegularization;
// delta_p, delta_d: the options'; run_p, run_d: AdaptiveRegularization's running pair (the others hand it through)
struct MpcReg { double del_w, del_c, run_p, run_d; };
MPC_HOST_DEVICE inline MpcReg mpc_init_regularization(int mode, double delta_p, double delta_d) {
    return {1.0, mode == 0 ? 0.0 : delta_d, delta_p, delta_d};
}
MPC_HOST_DEVICE inline MpcReg mpc_update_regularization(int mode, double delta_p, double delta_d, double delta_min,
                                                        double run_p, double run_d) {
    if (mode == 0) return {0.0, 0.0, run_p, run_d};
    if (mode == 1) return {delta_p, delta_d, run_p, run_d};
    run_p = mpc_max(run_p / 10.0, delta_min);
    run_d = mpc_min(run_d / 10.0, -delta_min);
    return {run_p, run_d, run_p, run_d};
}
// factorize_regularized_system! (src/linear_solver.jl:6-17): MPC_FACTOR_TRIALS factorisations at the most, del_w and
// del_c times MPC_RETRY_FACTOR behind each failed one
constexpr int MPC_FACTOR_TRIALS = 3;
constexpr double MPC_RETRY_FACTOR = 100.0;
MPC_HOST_DEVICE inline double mpc_retry(double del) { return del * MPC_RETRY_FACTOR; }

// update_step!(::MehrotraAdaptiveStep) (src/kernels.jl:325-374) behind get_alpha_max_primal / _dual at tau = 1.
// a4: the minima of {xl, xu, zl, zu}.  mpc_blocking: which of them stops the primal (dual = 0) or the dual step -- 0 / 1 or
// 2 / 3, odd = an upper bound -- or -1 where the step is free; the caller reads {x, bound, z, dx, dz} at that one's
// blocking index into row_p / row_d (not read where the step is free).  mean: the affine complementarity at the two minima.
MPC_HOST_DEVICE inline int mpc_blocking(const double* a4, int dual) {
    const double* a = a4 + 2 * dual;
    return mpc_min(a[0], a[1]) < 1.0 ? 2 * dual + (a[0] <= a[1] ? 0 : 1) : -1;
}
enum { MPC_ROW_X = 0, MPC_ROW_BOUND, MPC_ROW_Z, MPC_ROW_DX, MPC_ROW_DZ, MPC_ROW_LEN };
MPC_HOST_DEVICE inline MpcSteps mpc_mehrotra_step(const double* a4, const double* row_p, const double* row_d, double mean,
                                                  double gamma_f) {
    const double gamma_a = 1.0 / (1.0 - gamma_f);
    const double mu_full = mean / gamma_a;
    const double max_ap = mpc_min(a4[0], a4[1]), max_ad = mpc_min(a4[2], a4[3]);
    const int kp = mpc_blocking(a4, 0), kd = mpc_blocking(a4, 1);
    MpcSteps alpha{1.0, 1.0};
    if (kp >= 0) {
        const double* r = row_p;
        const double tmp = mu_full / (r[MPC_ROW_Z] + max_ad * r[MPC_ROW_DZ]);
        alpha.p = (kp & 1) ? (r[MPC_ROW_BOUND] - r[MPC_ROW_X] - tmp) / r[MPC_ROW_DX]
                           : (r[MPC_ROW_X] - r[MPC_ROW_BOUND] - tmp) / (-r[MPC_ROW_DX]);
    }
    if (kd >= 0) {
        const double* r = row_d;
        const double tmp = (kd & 1) ? mu_full / (r[MPC_ROW_BOUND] - r[MPC_ROW_X] - max_ap * r[MPC_ROW_DX])
                                    : mu_full / (r[MPC_ROW_X] + max_ap * r[MPC_ROW_DX] - r[MPC_ROW_BOUND]);
        alpha.d = -(r[MPC_ROW_Z] - tmp) / r[MPC_ROW_DZ];
    }
    return {mpc_max(alpha.p, gamma_f * max_ap), mpc_max(alpha.d, gamma_f * max_ad)};
}

// the objective from the sums of eval_grad_kernel: c0 + q'x + x'Hx / 2
MPC_HOST_DEVICE inline double mpc_objective(double c0, double lin, double quad) { return c0 + lin + 0.5 * quad; }
// MadNLP.adjust_boundary! (src/solver.jl:342): a bound nearer than eps * mu moves out by eps^(3/4) max(1, |x|)
constexpr double MPC_EPS = 2.220446049250313e-16, MPC_ADJUST_C2 = 1.8189894035458565e-12;
MPC_HOST_DEVICE inline double mpc_adjust_c1(double mu) { return MPC_EPS * mu; }

// ---- the start point (init_starting_point!, src/solver.jl:68-99; the batched engine is the one native caller) ------------
// mn4: the minima (0 at the most) of x - xl, xu - x, zl, zu over their bounds.  The first shift: x by delta_x, z by 1 + delta_s
struct MpcShift { double x, z; };
MPC_HOST_DEVICE inline MpcShift mpc_start_shift(const double* mn4) {
    const double delta_x = mpc_max3(0.0, -1.5 * mn4[0], -1.5 * mn4[1]);
    const double delta_s = mpc_max3(0.0, -1.5 * mn4[2], -1.5 * mn4[3]);
    return {delta_x, 1.0 + delta_s};
}
// sm8: x'zl, xl'zl, xu'zu, x'zu, then the sums of zl, zu, x - xl, xu - x, behind that shift.  The second one (0 / 0 = NaN
// without a bound, as in the reference: nothing is shifted by it then)
MPC_HOST_DEVICE inline MpcShift mpc_start_shift2(const double* sm8, bool has_lb, bool has_ub) {
    double mu = 0.0;
    if (has_lb) mu += sm8[0] - sm8[1];
    if (has_ub) mu += sm8[2] - sm8[3];
    return {mu / (2 * (sm8[4] + sm8[5])), mu / (2 * (sm8[6] + sm8[7]))};
}
