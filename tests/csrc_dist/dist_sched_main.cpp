// TEST INFRASTRUCTURE -- a stand-alone program, never loaded into Python (tests/test_dist2d.py runs it once).
//
// The grid schedule of madqp_jl_amd/csrc/dist_core.inc in its CPU form (tests/csrc/dist_cpu.cpp), walked by ONE rank with
// every collective forced (force_comm = 1) under the address and undefined-behaviour sanitizers: the stored-operand
// staircases over several levels, operands_exchange with its tile gathers, band_collect with the send-to-self and the
// group sweeps all run in one process, no launcher involved.  The collectives are in-process: bcast / reduce / allreduce
// of one rank leave the buffer as it is, send appends the bytes to a queue, recv pops the front and fails on a length
// mismatch.  dist_cpu.cpp's dop_gemm touches the padded read extents, so a wrong extent is an out-of-bounds read here.
#include "../csrc/dist_cpu.cpp"

#include <deque>
#include <string>

namespace {
std::deque<std::vector<char>> g_wire;
int32_t w_bcast(void*, void*, int64_t, int32_t, int32_t) { return 0; }
int32_t w_reduce(void*, double*, int64_t, int32_t, int32_t) { return 0; }
int32_t w_allreduce(void*, double*, int64_t, int32_t) { return 0; }
int32_t w_send(void*, const void* buf, int64_t bytes, int32_t) {
    g_wire.emplace_back((const char*)buf, (const char*)buf + bytes);
    return 0;
}
int32_t w_recv(void*, void* buf, int64_t bytes, int32_t) {
    if (g_wire.empty() || (int64_t)g_wire.front().size() != bytes) return 1;
    memcpy(buf, g_wire.front().data(), (size_t)bytes);
    g_wire.pop_front();
    return 0;
}

uint64_t g_seed = 20250614;
double uniform_half() {  // uniform in +-0.5
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_seed >> 11) / 9007199254740992.0 - 0.5;
}

// group = 0: MADQP_DIST_GROUP unset; bad_col >= 0: that diagonal entry is made negative and info must name it
bool run_case(int64_t n, int64_t nb, int group, int32_t force_comm, int64_t bad_col) {
    if (group)
        setenv("MADQP_DIST_GROUP", std::to_string(group).c_str(), 1);
    else
        unsetenv("MADQP_DIST_GROUP");
    const madqp_comm_ops ops{nullptr, w_bcast, w_reduce, w_allreduce, w_send, w_recv};
    Dev dev;
    madqp_dist* d = nullptr;
    int32_t r = distcore::create(&dev, 0, 1, 1, 1, n, nb, &ops, force_comm, &d);
    if (!r) r = distcore::allocate(d);
    if (r) {
        printf("(%lld, %lld, %d): create failed: %d %s\n", (long long)n, (long long)nb, group, r, d ? d->err : "");
        distcore::destroy(d);
        return false;
    }
    int64_t mem[8];
    madqp_distcpu_memory(d, mem);
    // symmetric, diagonally dominant: diagonal n, off-diagonal uniform in +-0.5; the lower triangle goes into the handle
    std::vector<double> A((size_t)(n * n)), b((size_t)n), x;
    for (int64_t j = 0; j < n; ++j) {
        A[(size_t)(j + j * n)] = (j == bad_col) ? -(double)n : (double)n;
        for (int64_t i = j + 1; i < n; ++i) A[(size_t)(i + j * n)] = A[(size_t)(j + i * n)] = uniform_half();
    }
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j; i < n; ++i) d->K[i + j * d->ld] = A[(size_t)(i + j * n)];
    double bmax = 0.0, res = 0.0;
    for (double& v : b) bmax = std::max(bmax, std::fabs(v = uniform_half()));
    x = b;
    int32_t info = -1;
    r = madqp_distcpu_factor(d, &info);
    bool ok = (r == 0) && info == (int32_t)(bad_col + 1);
    if (ok && bad_col < 0) {
        ok = madqp_distcpu_solve(d, x.data()) == 0;
        for (int64_t i = 0; i < n; ++i) {
            double s = -b[(size_t)i];
            for (int64_t j = 0; j < n; ++j) s += A[(size_t)(i + j * n)] * x[(size_t)j];
            res = std::max(res, std::fabs(s));
        }
        res /= bmax;
        ok = ok && res <= 1e-12;  // the bar tests/test_dist2d.py applies to factor_err
    }
    ok = ok && g_wire.empty();
    printf("(%lld, %lld, %d) force_comm %d: rc %d info %d residual %.3e queue %zu memory8 %lld %lld %lld %lld %lld %lld %lld %lld%s\n",
           (long long)n, (long long)nb, group, force_comm, r, info, res, g_wire.size(), (long long)mem[0], (long long)mem[1],
           (long long)mem[2], (long long)mem[3], (long long)mem[4], (long long)mem[5], (long long)mem[6], (long long)mem[7],
           ok ? "" : "  FAILED");
    g_wire.clear();
    distcore::destroy(d);
    return ok;
}
}  // namespace

int main() {
    bool ok = run_case(700, 128, 2, 1, -1);      // six tiles, three levels, a partial last tile, three groups
    ok = run_case(900, 256, 0, 1, -1) && ok;     // two 128-blocks per tile, one group
    ok = run_case(130, 128, 1, 1, -1) && ok;     // a 2-column last tile
    ok = run_case(600, 128, 2, 0, -1) && ok;     // nothing forced: the in-place path and dop_solve_local
    ok = run_case(700, 128, 2, 1, 437) && ok;    // a negative diagonal entry: info is that column, 1-based
    printf(ok ? "dist schedule ok\n" : "dist schedule FAILED\n");
    return ok ? 0 : 1;
}
