// Test infrastructure: madqp_jl_amd/csrc/band_plan.inc behind C entry points -- the schedule of the left-looking
// factorisations (chol_plan.inc, which it includes), the job lists of the sweeps under a band with the decode of a job
// that the kernels compile, and the layout of packed band storage -- so that the tests (tests/band_cases.py) can check and
// execute them in numpy without a GPU.
#include "../../madqp_jl_amd/csrc/band_plan.inc"

static void plan_rows(const std::vector<CholOp>& ops, int64_t* out, int64_t max_rows, int64_t* nrows) {
    *nrows = (int64_t)ops.size();
    for (int64_t i = 0; i < *nrows && i < max_rows; ++i) {
        const CholOp& o = ops[i];
        int64_t* row = out + 7 * i;
        row[0] = o.kind, row[1] = o.row0, row[2] = o.rows, row[3] = o.k0, row[4] = o.kend, row[5] = o.width, row[6] = o.sign;
    }
}
// Plans (n, bw, npos) on `slots` workgroups (force_wt > 0: the outer panel width in blocks wherever the band limits it) and
// writes up to max_rows rows (kind, row0, rows, k0, kend, width, sign) to out; *nrows = operations in all; returns the extent.
extern "C" int64_t band_plan_rows(int64_t n, int64_t bw, int64_t npos, int64_t slots, int64_t force_wt, int64_t* out,
                                  int64_t max_rows, int64_t* nrows) {
    std::vector<CholOp> ops;
    const int64_t extent = chol_plan(n, bw, npos, slots, ops, 6, 20, force_wt);
    plan_rows(ops, out, max_rows, nrows);
    return extent;
}
// the bare halving of the columns [j0, j0 + w) of an order-n matrix (chol_plan_range), rows as above
extern "C" void chol_range_rows(int64_t n, int64_t j0, int64_t w, int64_t* out, int64_t max_rows, int64_t* nrows) {
    std::vector<CholOp> ops;
    chol_plan_range(n, j0, w, ops);
    plan_rows(ops, out, max_rows, nrows);
}
// the outer panel where no band limits it (plan_outer_width with the default MADQP_CHOL_WMIN / WMAX)
extern "C" int64_t band_dense_outer_width(int64_t rows, int64_t has_update, int64_t slots) {
    return plan_outer_width(rows, has_update != 0, slots, 6, 20);
}

extern "C" int64_t band_sweep_blocks_c(int64_t bw) { return band_sweep_blocks(bw); }
extern "C" int64_t band_sweep_reach_c(int64_t n, int64_t kb) { return band_sweep_reach(n, kb); }
// The job list of (nblk, kb, chunk) -- kb < 0: the dense list -- into out (up to max_jobs entries, r | c << 20);
// *njobs = jobs in all; returns maxc, the stride of the partial-sum slots.
extern "C" int64_t band_sweep_jobs_c(int64_t nblk, int64_t kb, int64_t chunk, int32_t* out, int64_t max_jobs, int64_t* njobs) {
    std::vector<int32_t> jobs;
    const int64_t maxc = band_sweep_jobs(nblk, kb, chunk, jobs);
    *njobs = (int64_t)jobs.size();
    for (int64_t i = 0; i < *njobs && i < max_jobs; ++i) out[i] = jobs[i];
    return maxc;
}
// what the kernels make of job (r, c) of a list: out = (j0, j1, owner, clo)
extern "C" void band_sweep_range_c(int32_t r, int32_t c, int32_t chunk, int32_t kb, int32_t* out) {
    const BandSweepRange g = band_sweep_range(r, c, chunk, kb, true);
    out[0] = g.j0, out[1] = g.j1, out[2] = g.owner, out[3] = g.clo;
}

// out[0] = leading dimension, out[1] = doubles of storage; returns 0 when ld_in is refused.  pad < 0: the library's default.
extern "C" int64_t band_packed_layout_c(int64_t n, int64_t extent, int64_t ld_in, int64_t pad, int64_t* out) {
    return band_packed_layout(n, extent, ld_in, out, pad < 0 ? BAND_PACKED_PAD : pad) ? 1 : 0;
}
extern "C" int64_t band_packed_default_pad_c() { return BAND_PACKED_PAD; }
