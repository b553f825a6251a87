// Test infrastructure: walks the sweep job lists of madqp_jl_amd/csrc/band_plan.inc over the shapes
// tests/test_band_sweep_plan.py uses, through the band_sweep_range the kernels of chol.hip read them with, and checks
// every tile range, every wait and every partial-sum slot -- a stand-alone program, built with
// -fsanitize=address,undefined by the Makefile here and run once by the test; it is never loaded into Python.
#include <cstdio>

#include "../../madqp_jl_amd/csrc/band_plan.inc"

static int check(int64_t n, int64_t bw, int64_t chunk) {
    const int64_t nblk = std::max<int64_t>(1, (n + BAND_NB - 1) / BAND_NB), kb = band_sweep_blocks(bw);
    std::vector<int32_t> jobs, dense;
    const int64_t maxc = band_sweep_jobs(nblk, kb, chunk, jobs);
    band_sweep_jobs(nblk, -1, chunk, dense);
    int bad = 0;
    std::vector<int32_t> seen((size_t)(nblk * nblk), 0);  // tile (r, j) -> jobs that read it
    std::vector<int64_t> ticket((size_t)(nblk * maxc), -1);  // slot (r, c) -> ticket of the job that fills it
    std::vector<int32_t> owned((size_t)nblk, 0);
    int64_t prev = -1;
    for (size_t t = 0; t < jobs.size(); ++t) {
        const int64_t r = jobs[t] & 0xFFFFF, c = jobs[t] >> 20;
        if (r >= nblk || c >= maxc) {
            ++bad;
            continue;
        }
        const int64_t key = r * maxc + c;
        if (key <= prev) ++bad;  // ascending in (r, c)
        prev = key;
        const BandSweepRange g = band_sweep_range((int)r, (int)c, (int)chunk, (int)kb, true);  // what the kernels read
        if (g.j0 > g.j1) ++bad;
        for (int64_t j = g.j0; j < g.j1; ++j) {
            ++seen[(size_t)(r * nblk + j)];
            if (!owned[(size_t)j]) ++bad;  // the solution block j comes from an earlier ticket
        }
        ticket[(size_t)key] = (int64_t)t;
        if (g.owner) {  // waits for the chunks clo .. c - 1
            for (int64_t cc = g.clo; cc < c; ++cc)
                if (ticket[(size_t)(r * maxc + cc)] < 0) ++bad;
            ++owned[(size_t)r];
        }
    }
    for (int64_t r = 0; r < nblk; ++r) {
        if (owned[(size_t)r] != 1) ++bad;
        for (int64_t j = 0; j < nblk; ++j)
            if (seen[(size_t)(r * nblk + j)] != ((j >= band_sweep_lo(r, kb) && j < r) ? 1 : 0)) ++bad;
    }
    std::vector<BandOp> ops;
    const int64_t extent = band_plan(n, bw, 512, ops);
    if (band_sweep_reach(n, kb) > extent) ++bad;
    if (kb >= nblk - 1 && jobs != dense) ++bad;
    std::printf("n=%lld bw=%lld chunk=%lld jobs=%zu of %zu reach=%lld extent=%lld %s\n", (long long)n, (long long)bw,
                (long long)chunk, jobs.size(), dense.size(), (long long)band_sweep_reach(n, kb), (long long)extent,
                bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    const int64_t ns[] = {1, 128, 129, 500, 1537, 2100, 9000};
    const int64_t chunks[] = {1, 2, 3, 5, 64};
    for (int64_t n : ns) {
        const int64_t bws[] = {0, 1, 127, 128, 129, 300, 640, n - 1};
        for (int64_t bw : bws)
            for (int64_t chunk : chunks)
                if (bw < n) bad += check(n, bw, chunk);
    }
    bad += check(90000, 600, 64);
    bad += check(22500, 300, 64);
    return bad ? 1 : 0;
}
