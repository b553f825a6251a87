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
