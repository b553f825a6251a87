// Test infrastructure: walks the plans of madqp_jl_amd/csrc/solve_plan.inc over the shapes tests/test_solve_plan.py and
// tests/test_gpu_solve_many.py use and checks every range against the matrix and the band -- a stand-alone program, built
// with -fsanitize=address,undefined by the Makefile here and run once by the test; it is never loaded into Python.
#include <cstdio>

#include "../../madqp_jl_amd/csrc/solve_plan.inc"

static int check(int64_t n, int64_t npos, int64_t kb, int64_t nrhs) {
    std::vector<SolveOp> ops;
    solve_plan(n, npos, kb, nrhs, ops);
    const int64_t nblk = (n + SOLVE_NB - 1) / SOLVE_NB;
    const int64_t reach = kb < 0 ? n - 1 : std::min(n - 1, kb * SOLVE_NB + SOLVE_NB - 1);
    std::vector<int> solved(2 * (size_t)nblk, 0);
    int bad = 0, negates = 0;
    int64_t bytes = 0;
    for (const SolveOp& o : ops) {
        bytes += solve_op_bytes(o, false);
        if (o.kind == SOLVE_NEGATE) {
            ++negates;
            if (o.row0 != npos || o.row0 + o.rows != n) ++bad;
            for (int64_t j = 0; j < nblk; ++j)
                if (!solved[(size_t)j] || solved[(size_t)(nblk + j)]) ++bad;  // between the sweeps
            continue;
        }
        if (o.blk < 0 || o.blk >= nblk || o.k0 != o.blk * SOLVE_NB || o.k1 != std::min(n, o.k0 + SOLVE_NB) || o.rows < 1) ++bad;
        if (o.row0 < 0 || o.row0 + o.rows > n) ++bad;
        int& mine = solved[(size_t)(o.sweep * nblk + o.blk)];
        if (o.kind == SOLVE_DIAG) {
            if (mine || o.row0 != o.k0 || o.rows != o.k1 - o.k0) ++bad;
            mine = 1;
        } else {
            if (!mine) ++bad;  // the block's solution is applied after its diagonal step ...
            for (int64_t j = o.row0 / SOLVE_NB; j <= (o.row0 + o.rows - 1) / SOLVE_NB; ++j)
                if (solved[(size_t)(o.sweep * nblk + j)]) ++bad;  // ... to blocks whose own step is still to come
            // the entries of L read: rows row0.. x columns k0..k1 (forward), rows k0..k1 x columns row0.. (backward)
            const int64_t far = o.sweep == 0 ? o.row0 + o.rows - 1 - o.k0 : o.k1 - 1 - o.row0;
            if (far > reach) ++bad;
            if (o.sweep == 0 ? o.row0 != o.k1 : o.row0 + o.rows != o.k0) ++bad;
            if (o.sweep == 1 && (o.rows % SOLVE_NB || o.row0 % SOLVE_NB)) ++bad;  // whole tiles: the strip and U are read as such
        }
    }
    for (int v : solved)
        if (!v) ++bad;
    if (negates != (npos < n ? 1 : 0)) ++bad;
    const SolveCount c = solve_plan_count(ops, false), cu = solve_plan_count(ops, true);
    if (c.bytes != bytes || cu.bytes > c.bytes || cu.launches > c.launches || c.launches < (int64_t)ops.size() + 2) ++bad;
    std::printf("n=%lld npos=%lld kb=%lld nrhs=%lld ops=%zu launches=%lld bytes=%lld %s\n", (long long)n, (long long)npos,
                (long long)kb, (long long)nrhs, ops.size(), (long long)c.launches, (long long)c.bytes, bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    const int64_t ns[] = {1, 17, 128, 129, 300, 640, 1100, 1537};
    const int64_t rs[] = {1, 2, 15, 16, 17, 33, 130};
    for (int64_t n : ns)
        for (int64_t r : rs) {
            bad += check(n, n, -1, r);
            for (int64_t kb = 0; kb <= 3; ++kb) bad += check(n, n, kb, r);
        }
    bad += check(129, 128, -1, 17);
    bad += check(300, 128, -1, 17);
    bad += check(556, 256, -1, 17);
    bad += check(50000, 50000, -1, 64);
    bad += check(90000, 90000, 3, 64);
    std::vector<SolveOp> none;
    solve_plan(0, 0, -1, 5, none);
    bad += none.empty() ? 0 : 1;
    solve_plan(5, 5, -1, 0, none);
    bad += none.empty() ? 0 : 1;
    return bad ? 1 : 0;
}
