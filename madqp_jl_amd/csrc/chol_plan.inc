// The schedule of every left-looking factorisation of chol.hip as a list of operations (run_ops there executes it): plain
// C++17, host only, shared with the CPU test build tests/csrc_band, which executes it in numpy and walks it under the
// sanitizers.  The matrix is dense, column-major, of order n with half-bandwidth bw (A[i,j] = 0 for i - j > bw; n - 1: no
// band): a factor without pivoting stays inside the band, so every product and panel solve is cut down to the rows and the
// k-range the band can reach.  npos < n (no band): the matrix is [P, .; B, Q] and stands for the quasi-definite
// [P, B'; B, -Q] = L diag(I_npos, -I) L' with L = [L11, 0; W, L22], W = B L11^-T, L22 L22' = Q + W W' (stable unpivoted).
#include <algorithm>
#include <cassert>
#include <cstdint>
#include <vector>

constexpr int64_t BAND_NB = 128;    // block width (chol.hip: NB)
constexpr int64_t BAND_NBO = 1024;  // outer panel without an update (chol.hip: NBO)

// UPDATE: C[row0:row0+rows, row0:row0+width] += sign L[row0:row0+rows, k0:kend] L[row0:row0+width, k0:kend]', lower part only.
// BLOCK:  factor the diagonal block of width w <= 128 at jb, then solve the `rows` rows below it (whole tiles, or up to n).
enum { CHOL_UPDATE = 0, CHOL_BLOCK = 1 };
struct CholOp {
    int32_t kind;
    int64_t row0, rows, k0, kend, width;  // BLOCK: row0 = jb, width = w, k0 = kend = 0
    int32_t sign = -1;                    // of an UPDATE's product; +1: columns of the positive block onto the negative one
};

static int64_t band_up(int64_t v) { return (v + BAND_NB - 1) / BAND_NB * BAND_NB; }
static int64_t band_down(int64_t v) { return v < 0 ? 0 : v / BAND_NB * BAND_NB; }

// Width (multiple of 128) of the next outer panel over `rows` remaining rows: the wide update runs (rows/128) x (W/128)
// tiles of equal cost on `slots` resident workgroups, W fills the last round of tiles best (tail quantisation is the main
// loss of a left-looking factorisation; 8 fixed tile columns leave the last round 5-50 % full).
static int64_t plan_outer_width(int64_t rows, bool has_update, int64_t slots, int64_t wt_min, int64_t wt_max) {
    const int64_t mt = (rows + BAND_NB - 1) / BAND_NB;
    if (!has_update || mt <= 6) return BAND_NBO;
    int64_t best = BAND_NBO / BAND_NB;
    double best_eff = -1.0;
    for (int64_t wt = wt_min; wt <= wt_max && wt <= mt; ++wt) {
        const int64_t tiles = mt * wt - wt * (wt - 1) / 2;
        const int64_t rounds = (tiles + slots - 1) / slots;
        const double eff = (double)tiles / (double)(rounds * slots);
        if (eff > best_eff + 1e-9 || (eff > best_eff - 0.01 && wt > best && eff > 0.97)) {
            best_eff = std::max(eff, best_eff);
            best = wt;
        }
    }
    return best * BAND_NB;
}

// Outer panel under a band.  Where the band does not limit the remaining rows the rule above holds.  Where it does, a
// round of tiles is never full and that rule has nothing to optimise: the panel is as wide as the band in whole blocks,
// within [wt_min, wt_max] blocks -- a wider panel makes the outer update run tiles with i - j > bw (products of stored
// zeros), a narrower one adds dependent launches.  force_wt > 0 fixes the width in blocks (measurements).
static int64_t band_outer_width(int64_t rows, int64_t bw, bool has_update, int64_t slots, int64_t wt_min, int64_t wt_max,
                                int64_t force_wt) {
    const int64_t mt = (rows + BAND_NB - 1) / BAND_NB, mb = bw / BAND_NB + 1;
    if (mb >= mt) return plan_outer_width(rows, has_update, slots, wt_min, wt_max);
    if (force_wt > 0) return force_wt * BAND_NB;
    return std::max(wt_min, std::min(mb, wt_max)) * BAND_NB;
}

static void band_plan_block(int64_t n, int64_t bw, int64_t jb, int64_t w, std::vector<CholOp>& ops) {
    // the rows below the block that the band reaches from its columns: i <= jb + w - 1 + bw
    ops.push_back({CHOL_BLOCK, jb, std::min(band_up(bw), n - jb - w), 0, 0, w});
}
// an update of the columns [row0, row0 + width) with the columns [lo, hi) to their left, band-limited; nothing when the
// range is empty or the band reaches none of them
static void band_plan_update(int64_t n, int64_t bw, int64_t lo, int64_t hi, int64_t row0, int64_t width, int32_t sign,
                             std::vector<CholOp>& ops) {
    const int64_t k0 = std::max(lo, band_down(row0 - bw));
    if (k0 >= hi) return;
    ops.push_back({CHOL_UPDATE, row0, std::min(band_up(width + bw), n - row0), k0, hi, width, sign});
}
// Recursive halving of the columns [j0, j0 + w), which already carry the updates of all columns < j0: factor the first
// half (whole blocks, the larger half first), apply it to the second half with ONE wide product (N = K = w/2), recurse.
// Compared with a flat loop over 128-column blocks (N = 128, K up to w - 128) this moves the in-panel flops into
// well-filled launches; only the leaves are narrow.
static void band_plan_range(int64_t n, int64_t bw, int64_t j0, int64_t w, std::vector<CholOp>& ops) {
    if (w <= BAND_NB) return band_plan_block(n, bw, j0, w, ops);
    const int64_t h = ((w + BAND_NB - 1) / BAND_NB + 1) / 2 * BAND_NB;
    band_plan_range(n, bw, j0, h, ops);
    band_plan_update(n, bw, j0, j0 + h, j0 + h, w - h, -1, ops);
    band_plan_range(n, bw, j0 + h, w - h, ops);
}

// The bare halving of the columns [j0, j0 + w) of a dense matrix of order n, no outer panels: the batched factorisation
// (j0 = 0, w = n) and the panel pieces of the distributed one.
static void chol_plan_range(int64_t n, int64_t j0, int64_t w, std::vector<CholOp>& ops) {
    ops.clear();
    band_plan_range(n, n - 1, j0, w, ops);
}

// The ordered operations of the factorisation of an order-n matrix with half-bandwidth bw (0 <= bw < n) and signature npos
// (n: positive definite; a multiple of 128 below n, without a band only) on `slots` resident GEMM workgroups; returns the
// extent: the largest i - j of any entry an operation reads or writes (n - 1 at bw = n - 1).  An outer panel never straddles
// npos; one of the positive block receives the columns to its left, one of the negative block +[0, npos), then -[npos, J0).
// Rows are counted up to n; a padded leading dimension lets the kernels read (never write) whole tiles beyond n.
static int64_t chol_plan(int64_t n, int64_t bw, int64_t npos, int64_t slots, std::vector<CholOp>& ops, int64_t wt_min = 6,
                         int64_t wt_max = 20, int64_t force_wt = 0) {
    assert(npos == n || bw == n - 1);
    ops.clear();
    int64_t W = 0;
    for (int64_t J0 = 0; J0 < n; J0 += W) {
        W = std::min<int64_t>(band_outer_width(n - J0, bw, J0 > 0, slots, wt_min, wt_max, force_wt), n - J0);
        if (J0 < npos && J0 + W > npos) W = npos - J0;
        if (J0 < npos) {
            band_plan_update(n, bw, 0, J0, J0, W, -1, ops);
        } else {
            band_plan_update(n, bw, 0, npos, J0, W, +1, ops);
            band_plan_update(n, bw, npos, J0, J0, W, -1, ops);
        }
        band_plan_range(n, bw, J0, W, ops);
    }
    int64_t extent = 0;
    for (const CholOp& o : ops)
        extent = std::max(extent, o.kind == CHOL_UPDATE ? o.row0 + o.rows - 1 - o.k0 : o.width + o.rows - 1);
    return extent;
}
