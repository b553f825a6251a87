// Test infrastructure: the result-block layout and the scalar rules of the fused iteration
// (madqp_jl_amd/csrc/mpc_rules.inc) behind C entry points, so that tests/test_mpc_rules.py can hold them without a GPU.
#define MADQP_RESULT_SLOTS 128  // common.h's, which needs the HIP runtime (the test compares the two)
#define MADQP_FAULT_SLOT (MADQP_RESULT_SLOTS - 1)
#include "../../madqp_jl_amd/csrc/mpc_rules.inc"

extern "C" int mpc_fault_slot_c() { return MADQP_FAULT_SLOT; }

// Row i of the layout: the fields, then the parts of the trial block at the first trial's base ("TRIAL.*") and at the
// later trials' ("LATER.*"), then the later trials' sums.  Returns the number of rows.
extern "C" int mpc_layout_c(int i, const char** name, int* first, int* width) {
    static const MpcField parts[] = {{"nrm", MPC_TRIAL.nrm, MPC_W_NRM},
                                     {"alpha_gz", MPC_TRIAL.alpha_gz, MPC_W_ALPHA},
                                     {"alpha_tau", MPC_TRIAL.alpha_tau, MPC_W_ALPHA},
                                     {"dnorm", MPC_TRIAL.dnorm, MPC_TRIAL.width - MPC_TRIAL.dnorm}};
    static const char* names[2][4] = {{"TRIAL.nrm", "TRIAL.alpha_gz", "TRIAL.alpha_tau", "TRIAL.dnorm"},
                                      {"LATER.nrm", "LATER.alpha_gz", "LATER.alpha_tau", "LATER.dnorm"}};
    const int total = MPC_NFIELDS + 9;
    if (i < 0 || i >= total) return total;
    MpcField f;
    if (i < MPC_NFIELDS) {
        f = MPC_LAYOUT[i];
    } else if (i < MPC_NFIELDS + 8) {
        const int t = (i - MPC_NFIELDS) / 4, q = (i - MPC_NFIELDS) % 4;
        f = {names[t][q], (t ? MPC_SL_LATER_TRIAL : MPC_SL_TRIAL) + parts[q].first, parts[q].width};
    } else {
        f = {"LATER_COMPL", MPC_SL_LATER_COMPL, MPC_W_COMPL};
    }
    *name = f.name, *first = f.first, *width = f.width;
    return total;
}

// out[5]: words read behind the corrector, with the first trial, with the decisions, for a later trial, behind (c)
extern "C" void mpc_read_counts_c(int* out) {
    const int c[5] = {MPC_READ_CORRECTOR, MPC_READ_FIRST_TRIAL, MPC_READ_DECISION, MPC_READ_LATER_TRIAL, MPC_READ_FINAL};
    for (int i = 0; i < 5; ++i) out[i] = c[i];
}

extern "C" int mpc_verdict_c(const double* nrm, int check_residual, double tol, double* ratio) {
    *ratio = mpc_residual_ratio(nrm);
    return mpc_solve_failed(*ratio, check_residual, tol) ? 1 : 0;
}
extern "C" void mpc_steps_c(const double* a8, double* out2) {
    const MpcSteps a = mpc_steps(a8);
    out2[0] = a.p, out2[1] = a.d;
}
extern "C" void mpc_barrier_block_c(const double* sums4, double nb, double mu_min, int step_rule, double step_param,
                                    double* out3) {
    mpc_barrier_block(sums4, nb, mu_min, step_rule, step_param, out3);
}
extern "C" void mpc_trial_alpha_block_c(const double* a8, double* out8) { mpc_trial_alpha_block(a8, out8); }
extern "C" double mpc_muc_c(const double* sums2, double nb, double mu_curr) {
    return mpc_muc(mpc_compl_mean(sums2, nb), mu_curr);
}
extern "C" int mpc_trial_dropped_c(const double* trial2, const double* before2) {
    return mpc_trial_dropped({trial2[0], trial2[1]}, {before2[0], before2[1]}) ? 1 : 0;
}
extern "C" void mpc_decide_c(const double* blk, int gondzio, int max_ncorr, int check_residual, double tol, double* out4) {
    mpc_decide(blk, MpcDecideOpt{gondzio, max_ncorr, check_residual, tol}, out4);
}

// ---- the rules the batched engine calls too ---------------------------------------------------------------------------------
extern "C" void mpc_status_codes_c(int* out5) {
    const int c[5] = {MPC_ST_ACTIVE, MPC_ST_SOLVED, MPC_ST_MAXITER, MPC_ST_STEP_ERROR, MPC_ST_INTERNAL};
    for (int i = 0; i < 5; ++i) out5[i] = c[i];
}
extern "C" double mpc_nanmax_c(double a, double b) { return mpc_nanmax(a, b); }
// out3: the scaled infeasibilities; returns the status
extern "C" int mpc_head_c(const double* nrm3, double norm_b, double norm_c, double tol, long long k, long long max_iter,
                          double* out3) {
    const MpcHead h = mpc_head(nrm3, norm_b, norm_c, tol, k, max_iter);
    out3[0] = h.inf_pr, out3[1] = h.inf_du, out3[2] = h.inf_compl;
    return h.status;
}
extern "C" int mpc_queue_next_assembly_c(const double* inf3, double tol, long long k, long long max_iter) {
    return mpc_queue_next_assembly({inf3[0], inf3[1], inf3[2], MPC_ST_ACTIVE}, tol, k, max_iter) ? 1 : 0;
}
static void put_reg(const MpcReg& r, double* out4) { out4[0] = r.del_w, out4[1] = r.del_c, out4[2] = r.run_p, out4[3] = r.run_d; }
extern "C" void mpc_init_regularization_c(int mode, double delta_p, double delta_d, double* out4) {
    put_reg(mpc_init_regularization(mode, delta_p, delta_d), out4);
}
extern "C" void mpc_update_regularization_c(int mode, double delta_p, double delta_d, double delta_min, double run_p,
                                            double run_d, double* out4) {
    put_reg(mpc_update_regularization(mode, delta_p, delta_d, delta_min, run_p, run_d), out4);
}
// factorize_regularized_system! as the drivers loop it, the first `failures` factorisations failing: del2 = (del_w, del_c) in
// and out; returns the number of factorisations
extern "C" int mpc_factorize_trials_c(int failures, double* del2) {
    int n = 0;
    for (int trial = 0; trial < MPC_FACTOR_TRIALS; ++trial) {
        n += 1;
        if (trial >= failures) break;
        del2[0] = mpc_retry(del2[0]);
        del2[1] = mpc_retry(del2[1]);
    }
    return n;
}
extern "C" int mpc_blocking_c(const double* a4, int dual) { return mpc_blocking(a4, dual); }
extern "C" void mpc_mehrotra_step_c(const double* a4, const double* row_p, const double* row_d, double mean, double gamma_f,
                                    double* out2) {
    const MpcSteps a = mpc_mehrotra_step(a4, row_p, row_d, mean, gamma_f);
    out2[0] = a.p, out2[1] = a.d;
}
extern "C" double mpc_objective_c(double c0, double lin, double quad) { return mpc_objective(c0, lin, quad); }
extern "C" void mpc_adjust_c(double mu, double* out2) { out2[0] = mpc_adjust_c1(mu), out2[1] = MPC_ADJUST_C2; }
extern "C" void mpc_start_shifts_c(const double* mn4, const double* sm8, int has_lb, int has_ub, double* out4) {
    const MpcShift a = mpc_start_shift(mn4), b = mpc_start_shift2(sm8, has_lb != 0, has_ub != 0);
    out4[0] = a.x, out4[1] = a.z, out4[2] = b.x, out4[3] = b.z;
}
