// Test infrastructure: walks the plan of the band factorisation and the job lists of the band sweeps
// (madqp_jl_amd/csrc/band_plan.inc) over a packed buffer of exactly the size the layout reports -- every store the kernels
// make must land on the slot of its own band entry, every whole-tile read (rows and columns up to the padded order)
// inside the buffer -- a stand-alone program, built with -fsanitize=address,undefined by the Makefile here and run once by
// tests/test_band_packed.py; it is never loaded into Python.
#include <cmath>
#include <cstdio>

#include "../../madqp_jl_amd/csrc/band_plan.inc"

static int check(int64_t n, int64_t bw, int64_t ld_in, int64_t slots) {
    std::vector<BandOp> ops;
    const int64_t extent = band_plan(n, bw, slots, ops);
    int64_t lay[2] = {0, 0};
    if (!band_packed_layout(n, extent, ld_in, lay)) return 1;
    const int64_t ld = lay[0], size = lay[1], npad = band_up(n);
    int bad = 0;
    if (ld_in <= 0 && (ld % 2 != 0 || ld < extent + 1)) ++bad;
    if (size != npad * (ld + 1) + 128) ++bad;
    // the owner of every slot: the band entry (i, j), 0 <= i - j <= extent, stored there (as i - j + 1), or 0
    std::vector<double> P((size_t)size, std::nan(""));  // exactly `size` doubles: a read past it is the sanitizer's
    std::vector<int32_t> owner((size_t)size, 0);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j; i < n && i - j <= extent; ++i) {
            const int64_t a = i + j * ld;
            if (owner[a]) ++bad;  // two band entries at one address
            owner[a] = (int32_t)(i - j + 1);
            P[a] = 0.0;
        }
    double sink = 0.0;
    auto read_tile = [&](int64_t i0, int64_t rows, int64_t j0, int64_t cols) {  // a whole-tile read: masked or discarded
        for (int64_t j = j0; j < j0 + cols; ++j)
            for (int64_t i = i0; i < i0 + rows; ++i) sink += std::isnan(P[i + j * ld]) ? 0.0 : 1.0;
    };
    auto store = [&](int64_t i, int64_t j) {
        const int64_t a = i + j * ld;
        if (i < j || i >= n || i - j > extent || owner[a] != (int32_t)(i - j + 1)) ++bad;
        P[a] = 1.0;
    };
    for (const BandOp& o : ops) {
        if (o.kind == BAND_UPDATE) {
            // operands X (rows x K) and Y (width x K) in whole 128-row tiles, the addend C likewise; stores: the lower part
            read_tile(o.row0, band_up(o.rows), o.k0, o.kend - o.k0);
            read_tile(o.row0, std::min(npad - o.row0, band_up(o.width)), o.k0, o.kend - o.k0);
            read_tile(o.row0, o.rows, o.row0, o.width);
            for (int64_t gj = 0; gj < o.width; ++gj)
                for (int64_t gi = gj; gi < o.rows; ++gi) store(o.row0 + gi, o.row0 + gj);
        } else {
            // the diagonal kernel (lower triangle in, lower triangle out), the sweep-image kernel (the whole block in),
            // the panel solve (rows in whole tiles in, `rows` rows out)
            read_tile(o.row0, o.width, o.row0, o.width);
            for (int64_t c = 0; c < o.width; ++c)
                for (int64_t r = c; r < o.width; ++r) store(o.row0 + r, o.row0 + c);
            read_tile(o.row0 + o.width, band_up(o.rows), o.row0, o.width);
            for (int64_t c = 0; c < o.width; ++c)
                for (int64_t r = 0; r < o.rows; ++r) store(o.row0 + o.width + r, o.row0 + c);
        }
    }
    // the sweeps: block row r reads the tiles next to its diagonal block that band_sweep_range gives the kernels (one job
    // per row here), whole, up to the padded order
    const int64_t nblk = npad / BAND_NB, kb = band_sweep_blocks(bw);
    for (int64_t r = 0; r < nblk; ++r) {
        const BandSweepRange g = band_sweep_range((int)r, 0, 1, (int)kb, false);
        for (int64_t j = g.j0; j < g.j1; ++j)
            read_tile(r * BAND_NB, BAND_NB, j * BAND_NB, BAND_NB);  // forward: L[r, j]; backward reads the same tile as L[j', r']
    }
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j; i < n && i - j <= extent; ++i)
            if (std::isnan(P[i + j * ld])) ++bad;
    for (int64_t a = 0; a < size; ++a)
        if (!owner[a] && !std::isnan(P[a])) ++bad;  // a store outside the band
    std::printf("n=%lld bw=%lld ld=%lld extent=%lld doubles=%lld %s (%g)\n", (long long)n, (long long)bw, (long long)ld,
                (long long)extent, (long long)size, bad ? "BAD" : "ok", sink);
    return bad;
}

// the large shapes: no buffer, the highest address of a whole-tile read against the reported size
static int check_size(int64_t n, int64_t bw, int64_t slots) {
    std::vector<BandOp> ops;
    const int64_t extent = band_plan(n, bw, slots, ops);
    int64_t lay[2] = {0, 0};
    if (!band_packed_layout(n, extent, 0, lay)) return 1;
    const int64_t ld = lay[0], npad = band_up(n);
    const int64_t top = (npad - 1) + (npad - 1) * ld;  // row and column up to the padded order
    const int bad = (top + 2 > lay[1]) || ld < extent + 1 || ld % 2;  // (+ 2: a 16-byte load at the last address)
    std::printf("n=%lld bw=%lld ld=%lld extent=%lld doubles=%lld %s\n", (long long)n, (long long)bw, (long long)ld,
                (long long)extent, (long long)lay[1], bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    const int64_t ns[] = {129, 500, 1537, 2100};
    for (int64_t n : ns) {
        const int64_t bws[] = {0, 1, 127, 128, 129, 300, 640, n - 1};
        for (int64_t bw : bws) {
            if (bw >= n) continue;
            std::vector<BandOp> ops;
            const int64_t extent = band_plan(n, bw, 512, ops);
            const int64_t lds[] = {extent, extent + 1, 0, extent + 37};
            for (int64_t ld : lds) bad += check(n, bw, ld, 512);
        }
    }
    bad += check_size(90000, 600, 512);
    bad += check_size(202500, 900, 512);
    int64_t lay[2];
    if (band_packed_layout(2100, 767, 766, lay)) ++bad;  // below the extent: refused
    return bad ? 1 : 0;
}
