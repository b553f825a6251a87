// Test infrastructure: walks the plans of madqp_jl_amd/csrc/band_plan.inc over the shapes tests/test_band_plan.py uses and
// checks every range against the matrix -- a stand-alone program, built with -fsanitize=address,undefined by the Makefile
// here and run once by the test; it is never loaded into Python.
#include <cstdio>

#include "../../madqp_jl_amd/csrc/band_plan.inc"

static int check(int64_t n, int64_t bw, int64_t slots) {
    std::vector<BandOp> ops;
    const int64_t extent = band_plan(n, bw, slots, ops);
    int bad = 0;
    int64_t done = 0;  // columns factored so far
    for (const BandOp& o : ops) {
        if (o.row0 < 0 || o.rows < 0 || o.row0 + o.rows > n || o.width < 1) ++bad;
        if (o.kind == BAND_UPDATE) {
            if (!(o.k0 < o.kend && o.k0 % BAND_NB == 0 && o.kend == o.row0 && o.kend <= done)) ++bad;
            if (o.row0 + o.width > n || o.rows < o.width) ++bad;
            if (o.row0 + o.rows - 1 - o.k0 > extent) ++bad;
        } else {
            if (o.width > BAND_NB || o.row0 != done || o.row0 + o.width + o.rows > n) ++bad;
            if (o.width + o.rows - 1 > extent) ++bad;
            done += o.width;
        }
    }
    if (done != n || extent > n - 1 || extent < std::min(bw, n - 1)) ++bad;
    std::printf("n=%lld bw=%lld ops=%zu extent=%lld %s\n", (long long)n, (long long)bw, ops.size(), (long long)extent,
                bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    const int64_t ns[] = {1, 128, 129, 500, 1537, 2100};
    for (int64_t n : ns) {
        const int64_t bws[] = {0, 1, 127, 128, 129, 300, 640, n - 1};
        for (int64_t bw : bws)
            if (bw < n) bad += check(n, bw, 512);
    }
    bad += check(90000, 600, 512);
    bad += check(22500, 300, 512);
    bad += check(90000, 89999, 512);
    return bad ? 1 : 0;
}
