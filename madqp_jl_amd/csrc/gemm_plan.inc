// Host-side decisions of the fp64 MFMA product (gemm_f64.hip: madqp_gemm_tn): the tile table and the launch plan.
// Plain C++17 -- no HIP, no context, no environment -- so that tests/csrc/gemm_plan_cpu.cpp compiles it for the CPU and
// tests/test_gemm_plan.py holds every threshold below from both sides without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

constexpr int64_t GEMM_TILE = 128;   // edge of an output tile (BM = BN of gemm_core.inc)
constexpr int64_t GEMM_KSTEP = 16;   // K consumed per stage (BK): chunks of K are multiples of it

// The MADQP_GEMM_* environment switches with their defaults (gemm_f64.hip fills them once, at the first use)
struct GemmModes {
    int splitk = 1;       // MADQP_GEMM_SPLITK: 0 = no launch is cut in K
    int tailsplit = 1;    // MADQP_GEMM_TAILSPLIT: 0 = the last round of a few-round launch runs whole
    int seg_rounds = 64;  // MADQP_GEMM_SEG_ROUNDS: rounds of resident workgroups per launch segment; <= 0: one segment
    int xcd = 1;          // MADQP_GEMM_XCD: workgroup ids remapped to XCD-contiguous chunks of the table
    int batch_xcd = 1;    // MADQP_GEMM_BATCH_XCD: batches of a multiple of 8 problems dealt to the XCDs whole
    int64_t patch_m = 8, patch_n = 8;  // MADQP_GEMM_PATCH_M / _N: tiles per patch of the table
};

enum GemmMask { GEMM_MASK_NONE = 0, GEMM_MASK_COLS = 1, GEMM_MASK_ROW0 = 2 };

// The active tiles of an M x N product, packed (tile row << 16) | tile column, in launch order.
// mask: GEMM_MASK_COLS -- nmask / 2 column ranges [mask[2r], mask[2r+1]), only tile columns inside one are active;
//       GEMM_MASK_ROW0 -- per tile column the first active tile row.
// Edge tiles (partial last tile row / column) run the slower register-staged loop: they go FIRST so that they overlap
// with the bulk instead of forming the tail of the launch.  The rest follows in patches of PM x PN tiles, column inside
// patch: the 64 tiles resident on an XCD share 8 X panels and 8 Y panels.
static inline std::vector<int32_t> gemm_tile_table(int64_t M, int64_t N, bool lower_only, int64_t diag_off, GemmMask kind,
                                            const int64_t* mask, int64_t nmask, int64_t PM, int64_t PN) {
    const int64_t tiles_m = (M + GEMM_TILE - 1) / GEMM_TILE, tiles_n = (N + GEMM_TILE - 1) / GEMM_TILE;
    std::vector<char> col_on;
    if (kind == GEMM_MASK_COLS) {
        col_on.assign((size_t)tiles_n, 0);
        for (int64_t r = 0; r + 1 < nmask; r += 2)
            for (int64_t t = mask[r] / GEMM_TILE; t < (mask[r + 1] + GEMM_TILE - 1) / GEMM_TILE; ++t) col_on[(size_t)t] = 1;
    }
    const bool m_edge = (M % GEMM_TILE) != 0, n_edge = (N % GEMM_TILE) != 0;
    // diag_off in tile units must be exact for the tile-skip test
    auto active = [&](int64_t tm, int64_t tn) {
        if (kind == GEMM_MASK_COLS && !col_on[(size_t)tn]) return false;
        if (kind == GEMM_MASK_ROW0 && tm < mask[tn]) return false;
        return !(lower_only && (tm * GEMM_TILE + GEMM_TILE - 1 + diag_off < tn * GEMM_TILE));
    };
    auto is_edge = [&](int64_t tm, int64_t tn) { return (m_edge && tm == tiles_m - 1) || (n_edge && tn == tiles_n - 1); };
    std::vector<int32_t> tab;
    tab.reserve((size_t)tiles_m * tiles_n);
    if (m_edge)
        for (int64_t tn = 0; tn < tiles_n; ++tn)
            if (active(tiles_m - 1, tn)) tab.push_back((int32_t)(((tiles_m - 1) << 16) | tn));
    if (n_edge)
        for (int64_t tm = 0; tm < tiles_m - (m_edge ? 1 : 0); ++tm)
            if (active(tm, tiles_n - 1)) tab.push_back((int32_t)((tm << 16) | (tiles_n - 1)));
    for (int64_t pm = 0; pm < tiles_m; pm += PM)
        for (int64_t pn = 0; pn < tiles_n; pn += PN)
            for (int64_t tn = pn; tn < pn + PN && tn < tiles_n; ++tn)
                for (int64_t tm = pm; tm < pm + PM && tm < tiles_m; ++tm)
                    if (active(tm, tn) && !is_edge(tm, tn)) tab.push_back((int32_t)((tm << 16) | tn));
    return tab;
}

// Cost model of a launch cut in K (microseconds, measured): 0.216 per unit of K and 10 per piece of a tile, 0.05 per
// partial tile of the pass that sums them.  `tiles` tiles in S pieces each on `slots` resident workgroups take
//   rounds(S) x (time of a piece of K/S) + pass over the S x tiles partial tiles
// (an extra term for the drain of the last round was tried: 0.5 .. 2 tile times cost 0 .. 5 ms).
constexpr double GEMM_US_PER_K = 0.216, GEMM_US_PER_PIECE = 10.0, GEMM_US_PER_PARTIAL = 0.05;
static inline double gemm_piece_cost(int64_t K, int64_t S) { return GEMM_US_PER_K * (double)K / (double)S + GEMM_US_PER_PIECE; }
static inline double gemm_split_cost(int64_t tiles, int64_t K, int64_t S, int64_t slots) {
    const double rounds = std::ceil((double)tiles * (double)S / (double)slots);
    return rounds * gemm_piece_cost(K, S) + GEMM_US_PER_PARTIAL * (double)S * (double)tiles;
}
// the S in 2 .. max_S, with chunks of at least min_chunk, that costs least and less than `bound` (ties: `<` on doubles,
// the smaller S); 0: none
static inline int64_t gemm_best_split(int64_t tiles, int64_t K, int64_t slots, int64_t max_S, int64_t min_chunk, double bound) {
    int64_t S = 0;
    for (int64_t s = 2; s <= max_S && K / s >= min_chunk; ++s)
        if (gemm_split_cost(tiles, K, s, slots) < bound) bound = gemm_split_cost(tiles, K, s, slots), S = s;
    return S;
}
// K in S chunks: the chunk length, a multiple of the stage; ceil(K / chunk) <= S chunks are launched
static inline int64_t gemm_kchunk(int64_t K, int64_t S) { return ((K + S - 1) / S + GEMM_KSTEP - 1) / GEMM_KSTEP * GEMM_KSTEP; }
static inline int64_t gemm_nchunks(int64_t K, int64_t chunk) { return (K + chunk - 1) / chunk; }

enum GemmBatchForm { GEMM_SINGLE = 0, GEMM_BATCH = 1, GEMM_BATCH_LIST = 2 };

// What one call launches.  Either one persistent launch (persistent > 0) or `segments` launches of the plain kernel
// over the first `whole` tiles of the table, grid.y = gy (ksplit > 1: every tile in ksplit chunks of kchunk, then the
// reduction), then -- tail_tiles > 0 -- the remaining tiles in tail_split chunks of tail_chunk and their reduction.
struct GemmPlan {
    int32_t ntiles, whole;  // active tiles; of them launched whole (or all of them cut alike): ntiles - tail_tiles
    int32_t ksplit;         // > 1: chunks of K of every tile
    int64_t kchunk;         // their length; K when ksplit == 1
    int64_t seg;            // tiles per segment (see gemm_segment)
    int32_t segments;       // launches over the `whole` tiles; 0 for a persistent launch
    int32_t tail_tiles, tail_split;
    int64_t tail_chunk;
    int64_t persistent;     // workgroups of the persistent launch
    int32_t batch_xcd;
    uint32_t gy;            // grid.y of the plain launches: chunks of K, problems or slots of a batch
    size_t work_bytes;      // workspace of the partial tiles of a split launch (whole or tail; never both)
};

// tiles of the segment that starts at tile `off`: a remainder shorter than a quarter of a segment joins it
static inline int64_t gemm_segment(const GemmPlan& p, int64_t off) {
    const int64_t cnt = std::min<int64_t>(p.seg, p.whole - off);
    return p.whole - off - cnt < p.seg / 4 ? p.whole - off : cnt;
}

static inline GemmPlan gemm_plan(int64_t ntiles, int64_t K, int64_t slots, int64_t cap_slots, GemmBatchForm form, int64_t B,
                          const GemmModes& m) {
    GemmPlan p{};
    p.ntiles = (int32_t)ntiles, p.ksplit = 1, p.kchunk = K;
    p.gy = (unsigned)std::max<int64_t>(1, form == GEMM_SINGLE ? 1 : B);
    p.batch_xcd = (m.batch_xcd && form == GEMM_BATCH && B >= 8 && B % 8 == 0) ? 1 : 0;
    const bool may_split = m.splitk && form == GEMM_SINGLE;
    // Split-K.  A launch with far fewer tiles than resident workgroups leaves most of the chip idle while each tile
    // walks all of K alone (5k-20k matrices, the last panels of a large one): up to 16 chunks of >= 256, one workgroup
    // per (tile, chunk), partials summed in chunk order by a second small kernel -- same result on every run.
    // A launch of a few rounds of LONG tiles (the wide updates of the lazy distributed schedule, whose tile-column width
    // is the grid's tile and cannot be tuned to fill the rounds as chol.hip tunes its panels: 560 tiles of K = 38 000
    // take two rounds of 11 ms, the second one a tenth full, and whoever shares a CU with a finished workgroup runs on
    // alone) is cut into the S chunks that minimise the cost model -- more, shorter rounds.  With short tiles
    // (n_x = 5 000: K = 2 000) the model and the measurement agree that it does not pay; those launches are left alone.
    int64_t S = 0;
    if (may_split && ntiles * 2 > slots && ntiles < 8 * slots && K >= 4096)
        S = gemm_best_split(ntiles, K, slots, 16, 2048, gemm_split_cost(ntiles, K, 1, slots) * 0.97);
    else if (may_split && ntiles * 2 <= slots && K >= 512)
        S = std::min<int64_t>(std::min<int64_t>(slots / ntiles, K / 256), 16);
    if (S >= 2 && gemm_nchunks(K, gemm_kchunk(K, S)) >= 2) {
        p.kchunk = gemm_kchunk(K, S);
        p.ksplit = (int32_t)gemm_nchunks(K, p.kchunk);
        p.gy = (unsigned)p.ksplit;
    }
    // Tail split: a launch of one to three rounds whose LAST round is partly empty -- the assembly of a mid-size matrix:
    // 820 tiles on 512 slots are 1.6 rounds that take the time of 2 -- runs its whole rounds as they are and cuts only
    // the tiles of the last round into S chunks of K (more, shorter pieces that fill the chip), summed in chunk order
    // like every split launch.  S from the cost model, applied to the tiles of the last round; the round as it is costs
    // one whole piece, and the split is worth it only with a clear gain.
    if (may_split && m.tailsplit && p.ksplit == 1 && K >= 1024 && cap_slots == 0 && ntiles > slots && ntiles < 4 * slots) {
        const int64_t tl = ntiles % slots;  // (slots > 0 here)
        const bool part = tl > 0 && 10 * tl < 8 * slots;
        if (const int64_t tail_S = part ? gemm_best_split(tl, K, slots, 8, 256, gemm_piece_cost(K, 1) * 0.93) : 0) {
            p.tail_tiles = (int32_t)tl;
            p.tail_chunk = gemm_kchunk(K, tail_S);
            p.tail_split = (int32_t)gemm_nchunks(K, p.tail_chunk);
        }
    }
    p.whole = p.ntiles - p.tail_tiles;
    const int64_t partials = p.ksplit > 1 ? p.ksplit * ntiles : (int64_t)p.tail_split * p.tail_tiles;
    p.work_bytes = (size_t)partials * GEMM_TILE * GEMM_TILE * sizeof(double);
    // capped launch (cap_slots > 0, set by dist.hip around a bulk trailing update): a persistent grid that leaves
    // workgroup slots free for the kernels of other streams
    const int64_t capped = cap_slots > 0 ? std::max<int64_t>(8, (slots - cap_slots) / 8 * 8) : 0;
    p.persistent = capped && p.ksplit == 1 && form == GEMM_SINGLE && p.whole > capped ? capped : 0;
    if (p.persistent) return p;
    // Long launches are cut into segments of 64 rounds of resident workgroups.  Equal-cost tiles that start together
    // sweep K in lockstep and share their operand panels through the XCD's L2; over many rounds that lockstep diffuses
    // away (measured at n = 50000, K = 20480: 0.93-1.3 TB fetched by one assembly launch, 0.75 TB when re-synchronised
    // every 64 rounds, floor 0.68 TB).  The last round of a segment finishes almost simultaneously: +0.25 % time.
    // A launch cut in K is one segment: its partial tiles are indexed by the launch's own tile count.
    p.seg = m.seg_rounds > 0 && p.ksplit == 1 ? (int64_t)m.seg_rounds * slots : ntiles;
    for (int64_t off = 0; off < p.whole; off += gemm_segment(p, off)) p.segments += 1;
    return p;
}
