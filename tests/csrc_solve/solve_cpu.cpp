// Test infrastructure: madqp_jl_amd/csrc/solve_plan.inc behind C entry points, so that tests/test_solve_plan.py can check
// and execute the plan of madqp_chol_solve_many in numpy without a GPU.
#include "../../madqp_jl_amd/csrc/solve_plan.inc"

// Plans (n, npos, sweep_kb, nrhs) and writes up to max_rows rows (kind, sweep, blk, row0, rows, k0, k1, bytes) to out --
// bytes: what the operation moves of the factor on a handle with (has_upper != 0) or without U = L'; *nrows = operations in
// all; count = (launches, bytes) of one call.
extern "C" void solve_plan_rows(int64_t n, int64_t npos, int64_t sweep_kb, int64_t nrhs, int64_t has_upper, int64_t* out,
                                int64_t max_rows, int64_t* nrows, int64_t* count) {
    std::vector<SolveOp> ops;
    solve_plan(n, npos, sweep_kb, nrhs, ops);
    *nrows = (int64_t)ops.size();
    for (int64_t i = 0; i < *nrows && i < max_rows; ++i) {
        const SolveOp& o = ops[i];
        int64_t* row = out + 8 * i;
        row[0] = o.kind, row[1] = o.sweep, row[2] = o.blk, row[3] = o.row0, row[4] = o.rows, row[5] = o.k0, row[6] = o.k1;
        row[7] = solve_op_bytes(o, has_upper != 0);
    }
    const SolveCount c = solve_plan_count(ops, has_upper != 0);
    count[0] = c.launches, count[1] = c.bytes;
}
// count = (launches, bytes) of nrhs one-vector solves
extern "C" void solve_looped_count_c(int64_t n, int64_t npos, int64_t sweep_kb, int64_t nrhs, int64_t has_upper, int64_t* count) {
    const SolveCount c = solve_looped_count(n, npos, sweep_kb, nrhs, has_upper != 0);
    count[0] = c.launches, count[1] = c.bytes;
}
extern "C" int64_t solve_plan_workspace_c(int64_t n, int64_t nrhs, int64_t has_upper) {
    return solve_plan_workspace(n, nrhs, has_upper != 0);
}
