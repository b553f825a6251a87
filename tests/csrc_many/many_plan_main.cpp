// Test infrastructure: madqp_jl_amd/csrc/many_plan.inc -- the launch decode of the dense product on a block of vectors --
// compiled for the CPU.  Built twice by the Makefile here: as tests/_build/libmadqp_manyplan.so, whose C entry points hand
// the plan, the jobs, the staging and lane tables and the index functions to tests/test_many_plan.py (which replays the
// kernel in numpy), and as the stand-alone program tests/_build/many_plan_check under the address and undefined-behaviour
// sanitizers, which walks every job of the tested shapes against the operand bounds.  No sanitizer is ever loaded into Python.
#include <cstdio>
#include <vector>

#include "../../madqp_jl_amd/csrc/many_plan.inc"

extern "C" {
// out[10]: trans, ylen, klen, nrhs, row_tiles, col_groups, ksplit, kchunk, workgroups, partial_doubles
void many_plan_c(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, int64_t* out) {
    const ManyPlan p = many_plan(trans, rows, cols, nrhs);
    const int64_t v[10] = {p.trans, p.ylen, p.klen, p.nrhs, p.row_tiles, p.col_groups, p.ksplit, p.kchunk, p.workgroups,
                           p.partial_doubles};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}
// out: workgroups x 7 (row0, rows, col0, cols, k0, k1, split)
void many_jobs_c(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, int64_t* out) {
    const ManyPlan p = many_plan(trans, rows, cols, nrhs);
    for (int64_t wg = 0; wg < p.workgroups; ++wg) {
        const ManyJob j = many_job(p, wg);
        const int64_t v[7] = {j.row0, j.rows, j.col0, j.cols, j.k0, j.k1, j.split};
        for (int i = 0; i < 7; ++i) out[7 * wg + i] = v[i];
    }
}
// consts[6]: TR, TC, TK, A loads, X loads, MFMA steps per k step.  a_slot[trans][t][e][2], x_slot[t][e][2]: (local row or
// column, local k); lane_rc[64]; lane_k[step][64]; acc_col[64][4]
void many_tables_c(int64_t* consts, int32_t* a_slot, int32_t* x_slot, int32_t* lane_rc, int32_t* lane_k, int32_t* acc_col) {
    const int64_t c[6] = {MANY_TR, MANY_TC, MANY_TK, MANY_A_LOADS, MANY_X_LOADS, MANY_TK / 4};
    for (int i = 0; i < 6; ++i) consts[i] = c[i];
    for (int tr = 0; tr < 2; ++tr)
        for (int t = 0; t < 256; ++t)
            for (int e = 0; e < MANY_A_LOADS; ++e) {
                const ManySlot s = many_a_slot(tr, t, e);
                int32_t* o = a_slot + (((tr * 256 + t) * MANY_A_LOADS) + e) * 2;
                o[0] = s.r, o[1] = s.k;
            }
    for (int t = 0; t < 256; ++t)
        for (int e = 0; e < MANY_X_LOADS; ++e) {
            const ManySlot s = many_x_slot(t, e);
            int32_t* o = x_slot + ((t * MANY_X_LOADS) + e) * 2;
            o[0] = s.r, o[1] = s.k;
        }
    for (int l = 0; l < 64; ++l) {
        lane_rc[l] = many_lane_rc(l);
        for (int s = 0; s < MANY_TK / 4; ++s) lane_k[s * 64 + l] = many_lane_k(s, l);
        for (int g = 0; g < 4; ++g) acc_col[l * 4 + g] = many_acc_col(l, g);
    }
}
// the index functions on arrays of count entries
void many_a_index_c(int32_t trans, int64_t count, const int64_t* y, const int64_t* k, int64_t lda, int64_t* out) {
    for (int64_t i = 0; i < count; ++i) out[i] = many_a_index(trans, y[i], k[i], lda);
}
void many_x_index_c(int64_t count, const int64_t* k, const int64_t* c, int64_t ldx, int64_t* out) {
    for (int64_t i = 0; i < count; ++i) out[i] = many_x_index(k[i], c[i], ldx);
}
void many_y_index_c(int64_t count, const int64_t* y, const int64_t* c, int64_t ldy, int64_t* out) {
    for (int64_t i = 0; i < count; ++i) out[i] = many_y_index(y[i], c[i], ldy);
}
void many_partial_index_c(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, int64_t count, const int64_t* split,
                          const int64_t* y, const int64_t* c, int64_t* out) {
    const ManyPlan p = many_plan(trans, rows, cols, nrhs);
    for (int64_t i = 0; i < count; ++i) out[i] = many_partial_index(p, split[i], y[i], c[i]);
}
}

// every job of one shape against the bounds: the outputs and columns tile their ranges exactly once per k range, the k ranges
// tile [0, klen) in whole MANY_TK steps, every unmasked staging load and every store lands inside its operand, every tile
// slot is written by exactly one (thread, load)
static int check(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs) {
    const ManyPlan p = many_plan(trans, rows, cols, nrhs);
    const int64_t lda = cols + 3, ldx = p.klen + 2, ldy = p.ylen + 5;
    int bad = 0;
    if (p.workgroups != p.row_tiles * p.col_groups * p.ksplit || p.kchunk % MANY_TK || p.ksplit < 1 ||
        (p.ksplit - 1) * p.kchunk >= p.klen || p.ksplit * p.kchunk < p.klen)
        ++bad;
    if (p.partial_doubles != (p.ksplit > 1 ? p.ksplit * nrhs * p.ylen : 0)) ++bad;
    std::vector<int> owned((size_t)(p.ksplit * p.ylen * nrhs), 0);
    for (int64_t wg = 0; wg < p.workgroups; ++wg) {
        const ManyJob j = many_job(p, wg);
        if (j.rows < 1 || j.rows > MANY_TR || j.cols < 1 || j.cols > MANY_TC || j.row0 + j.rows > p.ylen || j.col0 + j.cols > nrhs ||
            j.k0 >= j.k1 || j.k1 > p.klen || j.k0 != j.split * p.kchunk || j.split >= p.ksplit)
            ++bad;
        for (int64_t kb = j.k0; kb < j.k1; kb += MANY_TK) {
            std::vector<int> sa((size_t)(MANY_TR * MANY_TK), 0), sx((size_t)(MANY_TC * MANY_TK), 0);
            for (int t = 0; t < 256; ++t) {
                for (int e = 0; e < MANY_A_LOADS; ++e) {
                    const ManySlot s = many_a_slot(trans, t, e);
                    if (s.r < 0 || s.r >= MANY_TR || s.k < 0 || s.k >= MANY_TK) { ++bad; continue; }
                    ++sa[(size_t)(s.r * MANY_TK + s.k)];
                    if (s.r < j.rows && kb + s.k < j.k1) {
                        const int64_t i = many_a_index(trans, j.row0 + s.r, kb + s.k, lda);
                        if (i < 0 || i / lda >= rows || i % lda >= cols) ++bad;
                    }
                }
                for (int e = 0; e < MANY_X_LOADS; ++e) {
                    const ManySlot s = many_x_slot(t, e);
                    if (s.r < 0 || s.r >= MANY_TC || s.k < 0 || s.k >= MANY_TK) { ++bad; continue; }
                    ++sx[(size_t)(s.r * MANY_TK + s.k)];
                    if (s.r < j.cols && kb + s.k < j.k1) {
                        const int64_t i = many_x_index(kb + s.k, j.col0 + s.r, ldx);
                        if (i < 0 || i / ldx >= nrhs || i % ldx >= p.klen) ++bad;
                    }
                }
            }
            for (int v : sa) bad += v != 1;
            for (int v : sx) bad += v != 1;
        }
        for (int64_t y = j.row0; y < j.row0 + j.rows; ++y)
            for (int64_t c = j.col0; c < j.col0 + j.cols; ++c) {
                const int64_t iy = many_y_index(y, c, ldy), ip = many_partial_index(p, j.split, y, c);
                if (iy / ldy >= nrhs || iy % ldy >= p.ylen) ++bad;
                if (ip < 0 || ip >= p.ksplit * nrhs * p.ylen) { ++bad; continue; }
                ++owned[(size_t)ip];
            }
    }
    for (int v : owned) bad += v != 1;
    if (bad) std::printf("trans=%d rows=%lld cols=%lld nrhs=%lld BAD (%d)\n", trans, (long long)rows, (long long)cols, (long long)nrhs, bad);
    return bad;
}

int main() {
    const int64_t rs[] = {1, 15, 16, 17, 127, 128, 129, 200}, cs[] = {1, 3, 4, 5, 63, 64, 65, 130};
    const int64_t ns[] = {1, 2, 15, 16, 17, 33, 128, 130};
    int bad = 0, cases = 0;
    for (int32_t trans = 0; trans < 2; ++trans) {
        for (int64_t r : rs)
            for (int64_t c : cs)
                for (int64_t n : ns) bad += check(trans, r, c, n), ++cases;
        bad += check(trans, 2000, 5000, 64), ++cases;  // the shape of the mid-size configuration
        bad += check(trans, 5000, 5000, 130), ++cases;
        const ManyPlan none = many_plan(trans, 0, 5, 3), none2 = many_plan(trans, 5, 5, 0);
        bad += none.workgroups != 0 || none2.workgroups != 0;
    }
    std::printf("%d shapes, %s\n", cases, bad ? "BAD" : "ok");
    return bad ? 1 : 0;
}
