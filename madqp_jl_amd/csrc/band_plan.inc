// The band-limited Cholesky beyond its schedule (chol_plan.inc): packed band storage and the job lists of the sweeps under a
// band with band_sweep_range, the one place that says which tiles a sweep job reads.  Plain C++17, shared by chol.hip (host
// code and both sweep kernels) and the CPU test build tests/csrc_band (one library, three sanitized check programs).
#include "chol_plan.inc"

// The plan under a band, in the band's own names: positive definite (a band admits no signature), so every update subtracts.
using BandOp = CholOp;
enum { BAND_UPDATE = CHOL_UPDATE, BAND_BLOCK = CHOL_BLOCK };
static int64_t band_plan(int64_t n, int64_t bw, int64_t slots, std::vector<BandOp>& ops, int64_t wt_min = 6, int64_t wt_max = 20, int64_t force_wt = 0) {
    return chol_plan(n, bw, n, slots, ops, wt_min, wt_max, force_wt);
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
// largest i - j they touch is min(n - 1, kb 128 + 127) -- never above the extent of chol_plan, whose first BLOCK op alone
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
