// Test infrastructure: the schedule of the band-limited factorisation (madqp_jl_amd/csrc/band_plan.inc) behind a C entry
// point, so that tests/test_band_plan.py can execute it in numpy and check its ranges without a GPU.
#include "../../madqp_jl_amd/csrc/band_plan.inc"

// Plans (n, bw) on `slots` workgroups (force_wt > 0: the outer panel width in blocks wherever the band limits it) and
// writes up to max_rows rows (kind, row0, rows, k0, kend, width) to out; *nrows = operations in all; returns the extent.
extern "C" int64_t band_plan_rows(int64_t n, int64_t bw, int64_t slots, int64_t force_wt, int64_t* out, int64_t max_rows,
                                  int64_t* nrows) {
    std::vector<BandOp> ops;
    const int64_t extent = band_plan(n, bw, slots, ops, 6, 20, force_wt);
    *nrows = (int64_t)ops.size();
    for (int64_t i = 0; i < *nrows && i < max_rows; ++i) {
        const BandOp& o = ops[i];
        int64_t* row = out + 6 * i;
        row[0] = o.kind, row[1] = o.row0, row[2] = o.rows, row[3] = o.k0, row[4] = o.kend, row[5] = o.width;
    }
    return extent;
}
// the dense schedule's outer panel (chol.hip: outer_panel_width with the default MADQP_CHOL_WMIN / WMAX)
extern "C" int64_t band_dense_outer_width(int64_t rows, int64_t has_update, int64_t slots) {
    return plan_outer_width(rows, has_update != 0, slots, 6, 20);
}
