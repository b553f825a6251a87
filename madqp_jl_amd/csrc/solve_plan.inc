// Host-side plan of a blocked solve with many right-hand sides (chol.hip: madqp_chol_solve_many): the operations of the two
// sweeps of a block substitution over the 128-column blocks of the factor, in the order they are launched.
// Plain C++17 -- no HIP, no context, no environment -- so that tests/csrc_solve compiles it for the CPU and
// tests/test_solve_plan.py executes it in numpy without a GPU (the arrangement of band_plan.inc / gemm_plan.inc).
//
// The right-hand sides are held transposed, T = B' (nrhs x n, right-hand-side index fastest), so that both sweeps are
// right-looking products of the form X Y' that madqp_gemm_tn runs:
//   forward,  block j = columns [k0, k1):   T[:, k0:k1] <- T[:, k0:k1] L_jj^-T                      SOLVE_DIAG
//                                           T[:, row0:row0+rows] -= T[:, k0:k1] L[row0.., k0:k1]'   SOLVE_UPDATE (row0 = k1)
//   between the sweeps, a signature npos < n:  T[:, npos:n] <- -T[:, npos:n]                         SOLVE_NEGATE
//   backward, block j from the last one:    T[:, k0:k1] <- T[:, k0:k1] L_jj^-1                      SOLVE_DIAG
//                                           T[:, row0:row0+rows] -= T[:, k0:k1] L[k0:k1, row0..]    SOLVE_UPDATE (row0 + rows = k0)
// Every block of L is read once per sweep, whatever nrhs.  Under a band of kb blocks (band_plan.inc: band_sweep_blocks;
// negative: none) an update reaches the kb blocks next to block j only, so the largest i - j read is min(n - 1, 128 kb + 127)
// -- the contract of the band sweeps, which packed storage relies on.
// The backward update needs its block row of L with the contraction index slow.  A handle that keeps U = L' (the mid-size
// schedule) has it; the others transpose the block row into a strip of the workspace first: one more launch per block and
// the block row written once and read once more -- counted in solve_plan_count.
#include <algorithm>
#include <cstdint>
#include <vector>

constexpr int64_t SOLVE_NB = 128;  // the factor's blocks (NB of chol.hip)

enum SolveOpKind { SOLVE_DIAG = 0, SOLVE_UPDATE = 1, SOLVE_NEGATE = 2 };

struct SolveOp {
    int32_t kind;   // SolveOpKind
    int32_t sweep;  // 0: forward, 1: backward (SOLVE_NEGATE: 0)
    int64_t blk;    // the block solved / whose solution is applied (SOLVE_NEGATE: -1)
    int64_t row0, rows;  // the entries of every right-hand side written: SOLVE_DIAG [k0, k1), SOLVE_NEGATE [npos, n)
    int64_t k0, k1;      // the columns of block blk (SOLVE_NEGATE: 0, 0)
};

// The operations of one call for a factor of order n with signature npos (n: positive definite) under a band of sweep_kb
// blocks (negative: none).  nrhs does not change the list -- every operation covers all right-hand sides -- only the
// counts below; nrhs <= 0 or n <= 0: nothing to do.
static inline void solve_plan(int64_t n, int64_t npos, int64_t sweep_kb, int64_t nrhs, std::vector<SolveOp>& ops) {
    ops.clear();
    if (n <= 0 || nrhs <= 0) return;
    const int64_t nblk = (n + SOLVE_NB - 1) / SOLVE_NB;
    const int64_t reach = sweep_kb < 0 ? n : sweep_kb * SOLVE_NB;
    for (int64_t j = 0; j < nblk; ++j) {
        const int64_t k0 = j * SOLVE_NB, k1 = std::min(n, k0 + SOLVE_NB);
        ops.push_back(SolveOp{SOLVE_DIAG, 0, j, k0, k1 - k0, k0, k1});
        const int64_t rows = std::min(n, k1 + reach) - k1;
        if (rows > 0) ops.push_back(SolveOp{SOLVE_UPDATE, 0, j, k1, rows, k0, k1});
    }
    if (npos < n) ops.push_back(SolveOp{SOLVE_NEGATE, 0, -1, std::max<int64_t>(npos, 0), n - std::max<int64_t>(npos, 0), 0, 0});
    for (int64_t j = nblk - 1; j >= 0; --j) {
        const int64_t k0 = j * SOLVE_NB, k1 = std::min(n, k0 + SOLVE_NB);
        ops.push_back(SolveOp{SOLVE_DIAG, 1, j, k0, k1 - k0, k0, k1});
        const int64_t row0 = std::max<int64_t>(0, k0 - reach);
        if (k0 > row0) ops.push_back(SolveOp{SOLVE_UPDATE, 1, j, row0, k0 - row0, k0, k1});
    }
}

// what one operation reads of the factor (bytes; has_upper = false: a backward update also writes and re-reads its strip)
static inline int64_t solve_op_bytes(const SolveOp& o, bool has_upper) {
    const int64_t w = o.k1 - o.k0;
    if (o.kind == SOLVE_DIAG) return 8 * (w * (w + 1) / 2);
    if (o.kind == SOLVE_UPDATE) return 8 * o.rows * w * ((o.sweep == 1 && !has_upper) ? 3 : 1);
    return 0;
}
// launches of one operation (SOLVE_UPDATE: K = 128 is below every K-split threshold of gemm_plan.inc: one launch)
static inline int64_t solve_op_launches(const SolveOp& o, bool has_upper) {
    return (o.kind == SOLVE_UPDATE && o.sweep == 1 && !has_upper) ? 2 : 1;
}

struct SolveCount {
    int64_t launches;  // of one call: the operations and the two transposes of the caller's block
    int64_t bytes;     // of the factor (and of the strips that stand for it) moved by one call
};
static inline SolveCount solve_plan_count(const std::vector<SolveOp>& ops, bool has_upper) {
    SolveCount c{ops.empty() ? 0 : 2, 0};
    for (const SolveOp& o : ops) c.launches += solve_op_launches(o, has_upper), c.bytes += solve_op_bytes(o, has_upper);
    return c;
}
// the same for nrhs one-vector solves (madqp_chol_solve): every sweep streams the factor's lower triangle inside the band;
// stream operations of one solve: three with U (fill, two sweeps), else three fills, two sweeps and the negation
static inline SolveCount solve_looped_count(int64_t n, int64_t npos, int64_t sweep_kb, int64_t nrhs, bool has_upper) {
    std::vector<SolveOp> ops;
    solve_plan(n, npos, sweep_kb, 1, ops);
    SolveCount c{0, 0};
    for (const SolveOp& o : ops) c.bytes += solve_op_bytes(o, true);
    c.bytes *= std::max<int64_t>(nrhs, 0);
    c.launches = n > 0 ? std::max<int64_t>(nrhs, 0) * (has_upper ? 3 : 5 + (npos < n ? 1 : 0)) : 0;
    return c;
}
// doubles of workspace: T (nrhs padded to whole 128s, n padded to whole blocks) and, without U, the strip of one block row
static inline int64_t solve_plan_ldt(int64_t nrhs) { return (std::max<int64_t>(nrhs, 1) + SOLVE_NB - 1) / SOLVE_NB * SOLVE_NB; }
static inline int64_t solve_plan_workspace(int64_t n, int64_t nrhs, bool has_upper) {
    const int64_t np = (std::max<int64_t>(n, 1) + SOLVE_NB - 1) / SOLVE_NB * SOLVE_NB;
    return solve_plan_ldt(nrhs) * np + (has_upper ? 0 : np * SOLVE_NB);
}
