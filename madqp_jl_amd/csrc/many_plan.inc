// Host-and-device plan of the dense product on a block of vectors (gemv_many.hip: madqp_gemv_many):
//   Y[:, c] = alpha op(A) X[:, c] + beta Y[:, c],  c < nrhs,   A: rows x cols, row r at A + r*lda,
//   trans = 0: op(A) = A  (contraction along the contiguous index of A),  trans = 1: op(A) = A' (along its slow index).
// Plain C++17 -- no HIP, no context, no environment -- so that tests/csrc_many compiles it for the CPU and
// tests/test_many_plan.py replays it in numpy without a GPU (the arrangement of gemm_plan.inc / solve_plan.inc).  The
// kernel reads the SAME functions: which workgroup owns which outputs, over which k range, and where every operand sits.
//
// A workgroup owns MANY_TR outputs (rows of Y) x one group of at most MANY_TC columns x one k range, and walks its k range
// in steps of MANY_TK through LDS.  A is therefore read ceil(nrhs / MANY_TC) times per call, whatever nrhs.  With one k range
// (ksplit == 1) the workgroup writes Y itself; with several, range s leaves its sums at many_partial_index(.., s, ..)
// and a second kernel adds the ranges s = 0, 1, .. in that order (one ordered chain per output: deterministic, no atomics).
#include <algorithm>
#include <cstdint>

#ifndef MANY_HD
#if defined(__HIPCC__)
#define MANY_HD __host__ __device__ inline
#else
#define MANY_HD inline
#endif
#endif

constexpr int64_t MANY_TR = 64;   // outputs per workgroup: 4 waves x one 16-row MFMA tile
constexpr int64_t MANY_TC = 128;  // columns per group: 8 MFMA tiles of 16
constexpr int64_t MANY_TK = 32;   // k step staged through LDS: 8 MFMA steps of 4
constexpr int64_t MANY_KMIN = 128;       // shortest k range worth a workgroup of its own
constexpr int64_t MANY_KSPLIT_MAX = 64;  // most k ranges (the reduce kernel walks them serially)
constexpr int64_t MANY_WG_TARGET = 512;  // workgroups wanted before the k ranges stop splitting (two per CU)

struct ManyPlan {
    int32_t trans;
    int64_t ylen, klen, nrhs;  // outputs per column, contraction length, columns
    int64_t row_tiles, col_groups, ksplit, kchunk;  // kchunk: a multiple of MANY_TK
    int64_t workgroups;                             // row_tiles * col_groups * ksplit
    int64_t partial_doubles;                        // ksplit > 1: ksplit * nrhs * ylen, else 0
};

struct ManyJob {
    int64_t row0, rows;  // outputs [row0, row0 + rows)
    int64_t col0, cols;  // columns [col0, col0 + cols)
    int64_t k0, k1;      // contraction range [k0, k1)
    int64_t split;       // which k range
};

// rows / cols: the shape of A.  Nothing to launch (workgroups == 0) when an output dimension is empty; klen == 0 is the
// caller's (Y <- beta Y needs no product).
MANY_HD ManyPlan many_plan(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs) {
    ManyPlan p{};
    p.trans = trans;
    p.ylen = trans ? cols : rows;
    p.klen = trans ? rows : cols;
    p.nrhs = nrhs;
    if (p.ylen <= 0 || p.klen <= 0 || nrhs <= 0) return p;
    p.row_tiles = (p.ylen + MANY_TR - 1) / MANY_TR;
    p.col_groups = (nrhs + MANY_TC - 1) / MANY_TC;
    const int64_t tiles = p.row_tiles * p.col_groups;
    int64_t want = (MANY_WG_TARGET + tiles - 1) / tiles;
    const int64_t most = (p.klen + MANY_KMIN - 1) / MANY_KMIN;
    if (want > most) want = most;
    if (want > MANY_KSPLIT_MAX) want = MANY_KSPLIT_MAX;
    if (want < 1) want = 1;
    p.kchunk = ((p.klen + want - 1) / want + MANY_TK - 1) / MANY_TK * MANY_TK;
    p.ksplit = (p.klen + p.kchunk - 1) / p.kchunk;
    p.workgroups = tiles * p.ksplit;
    p.partial_doubles = p.ksplit > 1 ? p.ksplit * nrhs * p.ylen : 0;
    return p;
}

// workgroup wg of the launch: row tile fastest, then column group, then k range
MANY_HD ManyJob many_job(const ManyPlan& p, int64_t wg) {
    ManyJob j{};
    const int64_t rt = wg % p.row_tiles, rest = wg / p.row_tiles;
    const int64_t cg = rest % p.col_groups;
    j.split = rest / p.col_groups;
    j.row0 = rt * MANY_TR;
    j.rows = p.ylen - j.row0 < MANY_TR ? p.ylen - j.row0 : MANY_TR;
    j.col0 = cg * MANY_TC;
    j.cols = p.nrhs - j.col0 < MANY_TC ? p.nrhs - j.col0 : MANY_TC;
    j.k0 = j.split * p.kchunk;
    j.k1 = j.k0 + p.kchunk < p.klen ? j.k0 + p.kchunk : p.klen;
    return j;
}

// where the operands of output y, contraction index k, column c sit
MANY_HD int64_t many_a_index(int32_t trans, int64_t y, int64_t k, int64_t lda) { return trans ? k * lda + y : y * lda + k; }
MANY_HD int64_t many_x_index(int64_t k, int64_t c, int64_t ldx) { return k + c * ldx; }
MANY_HD int64_t many_y_index(int64_t y, int64_t c, int64_t ldy) { return y + c * ldy; }
MANY_HD int64_t many_partial_index(const ManyPlan& p, int64_t split, int64_t y, int64_t c) {
    return (split * p.nrhs + c) * p.ylen + y;
}

// The staging of one k step, as data: thread t of the 256 loads element e = 0 .. of its operand tile.
//   A tile (MANY_TR outputs x MANY_TK k), 8 per thread: the contiguous index of A runs over the lanes, so a wave reads
//   whole 256-byte (trans = 0: 32 k of one row) or 512-byte (trans = 1: 64 outputs of one k) runs.
//   X tile (MANY_TC columns x MANY_TK k), 16 per thread: 32 consecutive k of one column per half wave.
// (local output / column, local k) of the e-th load of thread t:
struct ManySlot {
    int32_t r, k;
};
MANY_HD ManySlot many_a_slot(int32_t trans, int32_t t, int32_t e) {
    return trans ? ManySlot{t & 63, (t >> 6) + 4 * e} : ManySlot{(t >> 5) + 8 * e, t & 31};
}
MANY_HD ManySlot many_x_slot(int32_t t, int32_t e) { return ManySlot{(t >> 5) + 8 * e, t & 31}; }
constexpr int32_t MANY_A_LOADS = 8, MANY_X_LOADS = 16;
// The MFMA step s (4 k) of a wave's 16 outputs x 16 columns: lane l feeds output / column (l & 15) at k = 4 s + (l >> 4) to
// both operands (v_mfma_f64_16x16x4_f64: one f64 per lane per operand), and holds in register g the sum of
// column 4 g + (l >> 4), output (l & 15) -- the columns ride the MFMA's row index so that a register's 16 lanes store 16
// consecutive outputs of one column.
MANY_HD int32_t many_lane_rc(int32_t lane) { return lane & 15; }
MANY_HD int32_t many_lane_k(int32_t step, int32_t lane) { return 4 * step + (lane >> 4); }
MANY_HD int32_t many_acc_col(int32_t lane, int32_t reg) { return 4 * reg + (lane >> 4); }
