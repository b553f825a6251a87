// Schedule of the band-limited left-looking factorisation (see chol.hip, "band driver") and, at the end, the job lists of
// the triangular sweeps under a band with band_sweep_range, the one place that says which tiles a sweep job reads: plain
// C++17, shared by chol.hip (host code and both sweep kernels) and the CPU test build tests/csrc_band (one library, three
// sanitized check programs).  The matrix is dense, column-major and of order n with half-bandwidth bw (A[i,j] = 0 for i - j > bw); a factor without pivoting stays inside the band, so every product and
// every panel solve of the dense schedule is cut down to the rows and the k-range the band can reach.
#include <algorithm>
#include <cstdint>
#include <vector>

constexpr int64_t BAND_NB = 128;    // block width (chol.hip: NB)
constexpr int64_t BAND_NBO = 1024;  // outer panel of the dense schedule without an update (chol.hip: NBO)

// UPDATE: C[row0:row0+rows, row0:row0+width] -= L[row0:row0+rows, k0:kend] L[row0:row0+width, k0:kend]', lower part only.
// BLOCK:  factor the diagonal block of width w <= 128 at jb, then solve the `rows` rows below it.
enum { BAND_UPDATE = 0, BAND_BLOCK = 1 };
struct BandOp {
    int32_t kind;
    int64_t row0, rows, k0, kend, width;  // BLOCK: row0 = jb, width = w, k0 = kend = 0
};

static int64_t band_up(int64_t v) { return (v + BAND_NB - 1) / BAND_NB * BAND_NB; }
static int64_t band_down(int64_t v) { return v < 0 ? 0 : v / BAND_NB * BAND_NB; }

// Width (multiple of 128) of the dense schedule's next outer panel over `rows` remaining rows: the wide update runs
// (rows/128) x (W/128) tiles of equal cost on `slots` resident workgroups, W fills the last round of tiles best.
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

// Outer panel of the band schedule.  Where the band does not limit the remaining rows the dense rule holds (so the plan at
// bw = n - 1 IS the dense schedule).  Where it does, a round of tiles is never full and the dense rule has nothing to
// optimise: the panel is as wide as the band in whole blocks, within [wt_min, wt_max] blocks -- a wider panel makes the
// outer update run tiles with i - j > bw (products of stored zeros), a narrower one adds dependent launches.  force_wt > 0
// fixes the width in blocks (measurements).
static int64_t band_outer_width(int64_t rows, int64_t bw, bool has_update, int64_t slots, int64_t wt_min, int64_t wt_max,
                                int64_t force_wt) {
    const int64_t mt = (rows + BAND_NB - 1) / BAND_NB, mb = bw / BAND_NB + 1;
    if (mb >= mt) return plan_outer_width(rows, has_update, slots, wt_min, wt_max);
    if (force_wt > 0) return force_wt * BAND_NB;
    return std::max(wt_min, std::min(mb, wt_max)) * BAND_NB;
}

static void band_plan_block(int64_t n, int64_t bw, int64_t jb, int64_t w, std::vector<BandOp>& ops) {
    // the rows below the block that the band reaches from its columns: i <= jb + w - 1 + bw
    ops.push_back({BAND_BLOCK, jb, std::min(band_up(bw), n - jb - w), 0, 0, w});
}
// an update of the columns [row0, row0 + width) with the columns [lo, row0) to their left, band-limited; nothing when the
// band reaches none of them
static void band_plan_update(int64_t n, int64_t bw, int64_t lo, int64_t row0, int64_t width, std::vector<BandOp>& ops) {
    const int64_t k0 = std::max(lo, band_down(row0 - bw));
    if (k0 >= row0) return;
    ops.push_back({BAND_UPDATE, row0, std::min(band_up(width + bw), n - row0), k0, row0, width});
}
// the recursive halving of chol.hip's factor_range
static void band_plan_range(int64_t n, int64_t bw, int64_t j0, int64_t w, std::vector<BandOp>& ops) {
    if (w <= BAND_NB) return band_plan_block(n, bw, j0, w, ops);
    const int64_t h = ((w + BAND_NB - 1) / BAND_NB + 1) / 2 * BAND_NB;
    band_plan_range(n, bw, j0, h, ops);
    band_plan_update(n, bw, j0, j0 + h, w - h, ops);
    band_plan_range(n, bw, j0 + h, w - h, ops);
}

// The ordered operations of the factorisation of an order-n matrix with half-bandwidth bw (0 <= bw < n) on `slots` resident
// GEMM workgroups; returns the extent: the largest i - j of any entry an operation reads or writes (n - 1 at bw = n - 1).
// Rows are counted up to n; a padded leading dimension lets the kernels read (never write) whole tiles beyond n.
static int64_t band_plan(int64_t n, int64_t bw, int64_t slots, std::vector<BandOp>& ops, int64_t wt_min = 6,
                         int64_t wt_max = 20, int64_t force_wt = 0) {
    ops.clear();
    int64_t W = 0;
    for (int64_t J0 = 0; J0 < n; J0 += W) {
        W = std::min<int64_t>(band_outer_width(n - J0, bw, J0 > 0, slots, wt_min, wt_max, force_wt), n - J0);
        band_plan_update(n, bw, 0, J0, W, ops);
        band_plan_range(n, bw, J0, W, ops);
    }
    int64_t extent = 0;
    for (const BandOp& o : ops)
        extent = std::max(extent, o.kind == BAND_UPDATE ? o.row0 + o.rows - 1 - o.k0 : o.width + o.rows - 1);
    return extent;
}

// ---- packed band storage (madqp_chol_set_packed, madqp_chol_packed_layout) --------------------------------------------------
// Entry (i, j) of the lower triangle at P[i + j ld] with ld >= extent: LAPACK's lower band storage AB[(i - j) + j LDAB],
// LDAB = ld + 1, seen as a column-major matrix of leading dimension LDAB - 1 (what dpbtrf does to run dense kernels on band
// storage), so every kernel of the band path runs on it with lda = ld.  Two entries with 0 <= i - j <= extent never share
// an address ((j' - j)(ld + 1) - extent >= 1 for j' > j); an entry above the diagonal aliases the tail of earlier columns,
// one with i - j > ld the head of later ones -- neither is written by the band path, and what a whole-tile read finds there
// is masked or discarded.  Such reads go up to the padded order in rows AND columns, (npad - 1)(ld + 1) at most, and
// never below (0, 0): npad (ld + 1) doubles hold them all, + 128 of slack for 16-byte loads at the edge as the dense K has.
static int64_t band_packed_size(int64_t n, int64_t ld) { return band_up(std::max<int64_t>(n, 1)) * (ld + 1) + 128; }
// The library's own leading dimension: even (16-byte loads of whole columns), at least extent + 1 (so that the entry
// right above a diagonal entry, which the diagonal and sweep-image kernels load and drop, is no entry of the band), in
// whole 16s.  pad: further doubles (measurements).  Columns a large power of two apart (extent = 2 047 -> ld = 2 048) were
// expected to map badly onto the memory channels; measured at order 90 000 they do not -- pad 0 / 16 / 48 give 63.0 /
// 63.4 / 63.1 ms per factorisation and 10.08 / 10.16 / 10.23 ms per pair of sweeps (DESIGN.md 3.4b) -- so the default adds none.
constexpr int64_t BAND_PACKED_PAD = 0;
static int64_t band_packed_ld(int64_t extent, int64_t pad = BAND_PACKED_PAD) { return (extent + 1 + 15) / 16 * 16 + pad; }
// out[0] = the leading dimension (ld_in, or the library's choice for ld_in <= 0), out[1] = doubles of storage; false: ld_in
// is below the extent
static bool band_packed_layout(int64_t n, int64_t extent, int64_t ld_in, int64_t* out, int64_t pad = BAND_PACKED_PAD) {
    const int64_t ld = ld_in > 0 ? ld_in : band_packed_ld(extent, pad);
    if (ld < std::max<int64_t>(extent, 1)) return false;
    out[0] = ld;
    out[1] = band_packed_size(n, ld);
    return true;
}

// ---- the triangular sweeps under a band (chol.hip, trsv_*_sweep_kernel) --------------------------------------------------
// Block row r of the factor has nonzero tiles (r, j) for r - kb <= j < r only, kb = band_up(bw) / 128: a tile further left
// holds entries with i - j >= (kb + 1) 128 - 127 > bw alone.  The sweeps read those tiles and the diagonal blocks, so the
// largest i - j they touch is min(n - 1, kb 128 + 127) -- never above the extent of band_plan, whose first BLOCK op alone
// reaches min(band_up(bw) + 127, n - 1) for n >= 128.  The backward sweep is the same in chain coordinates (position rr
// is block nblk - 1 - rr, its tiles are counted from the last block row).
static int64_t band_sweep_blocks(int64_t bw) { return band_up(bw) / BAND_NB; }
// the first tile of block row r by the sentence above: what the CPU checks hold band_sweep_range (below) to, not used by it
static int64_t band_sweep_lo(int64_t r, int64_t kb) { return kb < 0 ? 0 : std::max<int64_t>(0, r - kb); }
static int64_t band_sweep_reach(int64_t n, int64_t kb) { return std::min(n - 1, kb * BAND_NB + BAND_NB - 1); }

// What job (r, c) of a sweep reads -- both sweep kernels and every CPU check call this: the tiles [j0, j1) of block row r
// (the backward sweep: of position r of the chain), whether the job owns the row (it holds the tile next to the diagonal
// block, solves the block and publishes it), and clo, the first chunk whose partial sums the owner adds.  split: the row
// is cut into chunks of `chunk` tiles along a job list; without one, job r is the whole row (c = 0).  Under a band of kb
// blocks (negative: none) the tiles before r - kb hold nothing of the factor: they are not read, and the chunks before
// the one that holds tile r - kb are no jobs and publish nothing.
#ifdef __HIPCC__
#define BAND_HOST_DEVICE __host__ __device__
#else
#define BAND_HOST_DEVICE
#endif
struct BandSweepRange {
    int j0, j1, clo;
    bool owner;
};
BAND_HOST_DEVICE static inline BandSweepRange band_sweep_range(int r, int c, int chunk, int kb, bool split) {
    int j0 = 0, j1 = r, clo = 0;
    if (split) {
        j0 = c * chunk;
        j1 = (j0 + chunk < r) ? j0 + chunk : r;
    }
    if (kb >= 0 && r > kb) {
        const int lo = r - kb;
        j0 = j0 > lo ? j0 : lo;
        if (split) clo = lo / chunk;
    }
    return {j0, j1, clo, j1 == r};
}

// The job list of one sweep over nblk < 2^20 block rows (ticket -> r | c << 20, ordered by (r, c)): the chunks of row r
// from the owner's first one (band_sweep_range) on; the last chunk owns the row and is a job even where the row has no
// tile (r = 0, kb = 0).  kb < 0 or kb >= nblk - 1: every chunk, the dense list.  Returns the most chunks any row has (the
// stride of the partial-sum slots).
static int64_t band_sweep_jobs(int64_t nblk, int64_t kb, int64_t chunk, std::vector<int32_t>& jobs) {
    jobs.clear();
    for (int64_t r = 0; r < nblk; ++r) {
        const int64_t nc = std::max<int64_t>(1, (r + chunk - 1) / chunk);
        const int64_t clo = band_sweep_range((int)r, 0, (int)chunk, (int)kb, true).clo;
        for (int64_t c = std::min(clo, nc - 1); c < nc; ++c) jobs.push_back((int32_t)(r | (c << 20)));
    }
    return std::max<int64_t>(1, (nblk - 1 + chunk - 1) / chunk);
}
