// The fused iteration of mpc.hip in its two fixed parts, each written once: where every scalar of an iteration lies in
// the context's result block, and the scalar rules of the iteration (src/kernels.jl, src/solver.jl,
// src/linear_solver.jl).  Plain C++17, no HIP call and no context: the host driver (mpc.hip) and the one-thread kernels
// (vec_kernels.hip) call the same functions, tests/csrc compiles them for the CPU and tests/test_mpc_rules.py holds them
// to oracle/mpc.py without a GPU.  Needs MADQP_FAULT_SLOT (common.h).
//
// Bits.  min and max are explicit comparisons in the operand order of std::min / std::max (what solver.py, oracle/mpc.py
// and the reference do with a NaN too), and no expression has a multiply feeding an add, so a host and a device compiler
// cannot contract them differently.
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
MPC_HOST_DEVICE inline MpcBarrier mpc_barrier(double mu_affine, double mu_curr, double nb, double mu_min, int step_rule,
                                              double step_param) {
    double sigma = 1.0;
    if (nb > 0.0) {
        const double t = mu_affine / mu_curr;
        sigma = mpc_min(mpc_max(t * t * t, 1e-6), 10.0);
    }
    const double mu = mpc_max(mu_min, sigma * mu_curr);
    return {mu, step_rule == 0 ? step_param : mpc_max(1.0 - mu, step_param), mu_curr};
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
