// Test infrastructure: walks the plans of madqp_jl_amd/csrc/chol_plan.inc over the shapes tests/test_band_plan.py uses --
// band, signature and bare range -- and checks every range against the matrix: a stand-alone program, built with
// -fsanitize=address,undefined by the Makefile here and run once by the test; it is never loaded into Python.
#include <cstdio>

#include "../../madqp_jl_amd/csrc/band_plan.inc"

// The operations against a matrix of order n whose columns [done, end) they factor (npos: where the negative block
// starts); extent < 0: none reported (a bare range).
static int walk(const std::vector<CholOp>& ops, int64_t n, int64_t npos, int64_t done, int64_t end, int64_t extent) {
    int bad = 0;
    const int64_t first = done;
    int64_t plus_at = -1;  // row0 of the last + update
    for (const CholOp& o : ops) {
        if (o.row0 < 0 || o.rows < 0 || o.row0 + o.rows > n || o.width < 1) ++bad;
        if (o.kind == CHOL_UPDATE) {
            // the k-range lies inside the factored columns (a bare range: the ones it factored itself)
            if (!(first <= o.k0 && o.k0 < o.kend && o.k0 % BAND_NB == 0 && o.kend <= o.row0 && o.kend <= done)) ++bad;
            if (o.row0 + o.width > n || o.rows < o.width) ++bad;
            if (extent >= 0 && o.row0 + o.rows - 1 - o.k0 > extent) ++bad;
            if (o.sign == +1) {  // at most one per panel, on panels at or beyond npos only, the columns [0, npos)
                if (o.row0 < npos || o.row0 == plus_at || o.k0 != 0 || o.kend != npos) ++bad;
                plus_at = o.row0;
            } else if (o.sign != -1 || o.kend != o.row0 || (o.row0 >= npos && o.k0 < npos)) {
                ++bad;
            }
        } else {
            if (o.width > BAND_NB || o.row0 != done || o.row0 + o.width + o.rows > n) ++bad;  // blocks in column order
            if (extent >= 0 && o.width + o.rows - 1 > extent) ++bad;
            done += o.width;
        }
    }
    return bad + (done != end);
}

static int check(int64_t n, int64_t bw, int64_t npos, int64_t slots) {
    std::vector<CholOp> ops;
    const int64_t extent = chol_plan(n, bw, npos, slots, ops);
    int bad = walk(ops, n, npos, 0, n, extent);
    if (extent > n - 1 || extent < std::min(bw, n - 1)) ++bad;
    std::printf("n=%lld bw=%lld npos=%lld ops=%zu extent=%lld %s\n", (long long)n, (long long)bw, (long long)npos, ops.size(),
                (long long)extent, bad ? "BAD" : "ok");
    return bad;
}

static int check_range(int64_t n, int64_t j0, int64_t w) {
    std::vector<CholOp> ops;
    chol_plan_range(n, j0, w, ops);
    const int bad = walk(ops, n, n, j0, j0 + w, -1);
    std::printf("n=%lld range=[%lld, %lld) ops=%zu %s\n", (long long)n, (long long)j0, (long long)(j0 + w), ops.size(),
                bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    const int64_t ns[] = {1, 128, 129, 500, 1537, 2100};
    for (int64_t n : ns) {
        const int64_t bws[] = {0, 1, 127, 128, 129, 300, 640, n - 1};
        for (int64_t bw : bws)
            if (bw < n) bad += check(n, bw, n, 512);
    }
    bad += check(90000, 600, 90000, 512);
    bad += check(22500, 300, 22500, 512);
    bad += check(90000, 89999, 90000, 512);
    const int64_t sig[][2] = {{0, 300},    {128, 50},    {256, 300},   {768, 800},  {1024, 129},
                              {1152, 1300}, {128, 2561}, {1280, 2900}, {2304, 1500}};  // (npos, nneg)
    for (const auto& s : sig) bad += check(s[0] + s[1], s[0] + s[1] - 1, s[0], 512);
    const int64_t rng[][3] = {{1, 0, 1},       {128, 0, 128},    {129, 0, 129},      {640, 0, 640},
                              {1000, 0, 1000}, {900, 256, 644}, {2100, 1024, 1076}};  // (n, j0, w)
    for (const auto& r : rng) bad += check_range(r[0], r[1], r[2]);
    return bad ? 1 : 0;
}
