// Test infrastructure: the job lists of the triangular sweeps under a band (madqp_jl_amd/csrc/band_plan.inc) behind C
// entry points, so that tests/test_band_sweep_plan.py can check them and execute the sweeps along them without a GPU.
#include "../../madqp_jl_amd/csrc/band_plan.inc"

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
// the extent of the factorisation's plan, which the sweeps' reach must not exceed
extern "C" int64_t band_plan_extent_c(int64_t n, int64_t bw, int64_t slots) {
    std::vector<BandOp> ops;
    return band_plan(n, bw, slots, ops);
}
