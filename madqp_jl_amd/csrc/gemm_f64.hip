// fp64 MFMA GEMM core for gfx950:  C[i,j] = alpha * sum_k X[i,k] Y[j,k] + beta * Cin[i,j] (+ dvec on the diagonal)
//
// One kernel serves the three dense contractions of the hot path:
//   * condensed-KKT assembly  K = H + Sigma_x + A' Theta A          (madqp_syrk_assemble)
//   * left-looking Cholesky panel update  C -= L[:, :k] L[J, :k]'   (chol.hip)
//   * panel times inverse diagonal block  L[:, J] = C[:, J] W'      (chol.hip)
//
// Both operands are "k-major": for a fixed k the M (resp. N) entries are contiguous in memory.
// That is the natural layout of column-major L (column k contiguous) and of row-major A
// (row k contiguous), so every tile row is one coalesced 1 KiB wave load and both LDS images
// are [k][index] with the index fastest.
//
// Tiling: 128 x 128 output tile per 256-thread workgroup (4 waves = 2 x 2, one per SIMD), each wave
// owns 64 x 64 = 4 x 4 v_mfma_f64_16x16x4_f64 accumulators (128 VGPRs).  K is consumed in
// stages of 16, LDS double buffered, one barrier per stage.  Interior tiles stage with LDS-DMA
// (global_load_lds_dwordx4: one wave instruction = one 1 KiB tile row, no VGPR round trip, no
// ds_write); edge tiles stage through registers with bounds checks and zero fill.  Per stage a
// wave issues 64 MFMAs and 32 ds_read_b64.  On gfx950 the fp64 MFMA shares the SIMD's issue with
// every other vector instruction (measured: each v_fma between two MFMAs costs ~9 cycles of
// matrix pipe, tools/mfma_probe.hip), so the loop is written to keep VALU work out of it.
// LDS row stride 144 doubles (= 16 mod 32) makes the two k-rows of a 32-lane ds_read_b64 group
// hit disjoint banks.
//
// MFMA operand roles (v_mfma_f64_16x16x4_f64: D[r][c] = sum_k A[r][k] B[k][c]; lane l feeds
// A[l&15][l>>4] and B[l>>4][l&15]; lane l holds D[(l>>4) + 4v][l&15], v = 0..3):
//   A-operand <- Y fragment (r = column index j of C),  B-operand <- X fragment (c = row index i)
// so the 16 lanes l&15 of an accumulator register walk 16 consecutive rows i of column-major C
// and each store instruction writes four 128-byte segments.
//
// Tile order: the host builds a table of the active tiles (all, or the lower triangle) in
// 8 x 8-tile patches; workgroup ids are remapped so that each XCD (ids equal mod 8 share an
// XCD and its L2) walks one contiguous chunk of the table: the 64 tiles resident on an XCD
// share 8 X panels and 8 Y panels.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

#include "common.h"
#include "gemm_plan.inc"

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

namespace {
#include "gemm_core.inc"
static_assert(BM == GEMM_TILE && BN == GEMM_TILE && BK == GEMM_KSTEP, "gemm_plan.inc plans for the tiles of gemm_core.inc");

struct KArgs {
    GemmArgs g;
    const int32_t* table;
    int32_t ntiles;
    int32_t fast_ok;  // pointers / leading dimensions allow 16-byte loads
    int32_t xcd_remap;
    int32_t batch_xcd;  // batch: problems dealt to XCDs whole (see gemm_tn_f64_kernel)
    GemmBatch batch;  // B <= 1: single problem
    // split-K (launches with fewer tiles than resident workgroups): blockIdx.y = split, each split
    // covers kchunk of K and stores its raw 128 x 128 partial into work[(split * ntiles + t)]
    int32_t ksplit;
    int64_t kchunk;
    double* work;
#ifdef MADQP_STAMPS
    unsigned long long* stamps;  // diagnostic build only (tools/gemm_probe): per-workgroup clocks
#endif
};

// wave-uniform operand offsets of a split-K chunk / of problem blockIdx.y of a batch; false: nothing to do
__device__ __forceinline__ bool gemm_select(const KArgs& ka, GemmArgs& g, int64_t b_batch = -1) {
    if (ka.ksplit > 1) {
        const int64_t k0 = (int64_t)blockIdx.y * ka.kchunk;
        g.X += k0 * g.ldx;
        g.Y += k0 * g.ldy;
        g.K = (g.K - k0 < ka.kchunk) ? (g.K - k0) : ka.kchunk;
    } else if (ka.batch.B > 1 || ka.batch.skip) {  // wave-uniform pointer offsets of problem blockIdx.y
        // (a batch of ONE with a skip list is still a batch: round 3 ignored the list then, and the masked retry rounds of
        // the batched engine re-assembled K over the factor of a problem that had not failed -- unnoticed while the sweeps
        // read only the inverse images and the re-computed panels, fatal once the panel solve reads L_kk itself)
        const int64_t b = b_batch >= 0 ? b_batch : (int64_t)blockIdx.y;
        if (ka.batch.skip && ka.batch.skip[b] != 0) return false;
        g.X += b * ka.batch.sX;
        g.Y += b * ka.batch.sY;
        g.C += b * ka.batch.sC;
        if (g.Cin) g.Cin += b * ka.batch.sCin;
        if (g.dvec) g.dvec += b * ka.batch.sD;
    }
    return true;
}

// one 128 x 128 output tile (entry t of the tile table) by the calling workgroup
__device__ __forceinline__ void gemm_tile(const KArgs& ka, const GemmArgs& g, int t, int bid, double* lds) {
    const int tid = threadIdx.x;
    const int32_t packed = ka.table[t];
    const int64_t i0 = (int64_t)(packed >> 16) * BM;
    const int64_t j0 = (int64_t)(packed & 0xFFFF) * BN;

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform, lives in an SGPR
    const int wi = wave & 1, wj = wave >> 1;
#ifdef MADQP_STAMPS
    const unsigned long long st_t0 = __builtin_amdgcn_s_memtime();
    const unsigned long long st_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    double4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};

    const bool interior = ka.fast_ok && (i0 + BM <= (g.Mread ? g.Mread : g.M)) &&
                          (j0 + BN <= (g.Nread ? g.Nread : g.N)) && (g.K % BK == 0);
    if (interior)
        mainloop_dma(g, i0, j0, lds, wi, wj, lane, wave, acc);
    else
        mainloop_staged(g, i0, j0, lds, tid, wi, wj, lane, acc);

#ifdef MADQP_STAMPS
    if (ka.stamps && tid == 0) {
        ka.stamps[2 * (size_t)bid] = __builtin_amdgcn_s_memtime() - st_t0;
        ka.stamps[2 * (size_t)bid + 1] = __builtin_amdgcn_s_memrealtime() - st_r0;
    }
#endif
    const int lo = lane & 15, hi = lane >> 4;
    if (ka.ksplit > 1) {  // raw partial tile, column-major 128 x 128; the epilogue runs in splitk_reduce_kernel
        double* W = ka.work + ((int64_t)blockIdx.y * ka.ntiles + t) * (BM * BN);
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    W[(wj * 64 + tj * 16 + hi + 4 * v) * BM + wi * 64 + ti * 16 + lo] = acc[ti][tj][v];
        return;
    }
    // out = alpha*acc + beta*Cin (+ dvec on the diagonal).  The addend is fetched 16 elements at a time from clamped
    // (always valid) addresses BEFORE the guarded stores: as one guarded read-modify-write per element the compiler
    // emits load, s_waitcnt vmcnt(0), store -- 64 dependent round trips, 40-45 us per tile, which is what held the
    // K = 128 .. 1024 update launches of the factorisation at 15-59 TFLOP/s.  Same arithmetic, same results.
    const bool has_cin = (g.Cin != nullptr);
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int64_t gi = i0 + wi * 64 + ti * 16 + lo;
        double cin[4][4];
        if (has_cin) {
            const int64_t gic = gi < g.M ? gi : g.M - 1;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int64_t gj = j0 + wj * 64 + tj * 16 + hi + 4 * v;
                    cin[tj][v] = g.Cin[gic + (gj < g.N ? gj : g.N - 1) * g.ldcin];
                }
        }
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t gj = j0 + wj * 64 + tj * 16 + hi + 4 * v;
                if (gi < g.M && gj < g.N && (!g.lower_only || gi + g.diag_off >= gj)) {
                    double val = g.alpha * acc[ti][tj][v];
                    if (has_cin) val += g.beta * cin[tj][v];
                    g.C[gi + gj * g.ldc] = val;
                }
            }
        }
    }
    // + dvec where global row == global column: a second pass over the (at most 128) diagonal elements of the tile,
    // after the stores above are visible to the workgroup -- val + dvec[j] either way
    if (g.dvec) {
        __syncthreads();
        if (tid < BN) {
            const int64_t gj = j0 + tid, gi = gj - g.diag_off;
            if (gj < g.N && gi >= i0 && gi < i0 + BM && gi < g.M) g.C[gi + gj * g.ldc] += g.dvec[gj];
        }
    }
}

__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_f64_kernel(KArgs ka) {
    __shared__ __attribute__((aligned(16))) double lds[4 * TILE_DOUBLES];
    if (ka.batch.list) {  // compacted batch (GemmBatch::list): the problems of this slot, one after the other
        const int cnt = __builtin_amdgcn_readfirstlane(*ka.batch.count);
        const int bid = blockIdx.x, T = ka.ntiles;
        const int xcd = bid & 7, q = T >> 3, r = T & 7;
        const int t = ka.xcd_remap ? (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3) : bid;
        for (int pb = blockIdx.y; pb < cnt; pb += gridDim.y) {
            const int64_t b = ka.batch.list[pb];
            GemmArgs g = ka.g;
            g.X += b * ka.batch.sX;
            g.Y += b * ka.batch.sY;
            g.C += b * ka.batch.sC;
            if (g.Cin) g.Cin += b * ka.batch.sCin;
            if (g.dvec) g.dvec += b * ka.batch.sD;
            gemm_tile(ka, g, t, bid, lds);
            __syncthreads();  // the LDS image is reused
        }
        return;
    }
    GemmArgs g = ka.g;
    if (ka.batch_xcd) {
        // A batch of small problems (grid = tiles x problems, dispatched tile index first): in launch order the ~10 tiles
        // of ONE problem land on eight different XCDs and each fetches its two operand blocks from HBM -- 5 MB per
        // problem where the operand is 1 MB.  Re-deal: XCD x (workgroups equal mod 8) takes problems x, x + 8, ..
        // whole, their tiles on workgroups that start together, so an operand block is fetched once per XCD.
        const int T = ka.ntiles;
        const int lin = (int)blockIdx.y * T + (int)blockIdx.x, slot = lin >> 3;
        const int64_t b = (int64_t)(slot / T) * 8 + (lin & 7);
        if (!gemm_select(ka, g, b)) return;
        gemm_tile(ka, g, slot % T, (int)blockIdx.x, lds);
        return;
    }
    if (!gemm_select(ka, g)) return;
    // Tile selection: the table is cut into 8 contiguous chunks, one per XCD (workgroup ids equal
    // mod 8 share an XCD under the observed round-robin dispatch; claiming tiles by the real
    // HW_REG_XCC_ID gave the same traffic and time, so the static map is kept).  Speed only: any
    // placement computes the same result.
    const int bid = blockIdx.x, T = ka.ntiles;
    const int xcd = bid & 7, q = T >> 3, r = T & 7;
    const int t = ka.xcd_remap ? (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3) : bid;
    gemm_tile(ka, g, t, bid, lds);
}

// The same tiles by a FIXED number of workgroups (gridDim.x, a multiple of 8, fewer than the chip holds): each draws
// tiles of its XCD's chunk of the table from that XCD's ticket counter until the chunk is used up.  Which workgroup
// computes a tile does not enter the result.  The eight counters are zeroed on the stream before the launch.
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_f64_persistent_kernel(KArgs ka, unsigned long long* tickets) {
    __shared__ __attribute__((aligned(16))) double lds[4 * TILE_DOUBLES];
    __shared__ int next_tile;
    const GemmArgs g = ka.g;
    const int bid = blockIdx.x, T = ka.ntiles;
    const int xcd = bid & 7, q = T >> 3, r = T & 7;
    const int chunk0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int chunk = q + (xcd < r ? 1 : 0);
    for (;;) {
        if (threadIdx.x == 0) {
            const unsigned long long tix = atomicAdd(tickets + xcd, 1ull);
            next_tile = tix < (unsigned long long)chunk ? chunk0 + (int)tix : -1;
        }
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(next_tile);
        if (t < 0) break;
        gemm_tile(ka, g, t, bid, lds);
        __syncthreads();  // the LDS image and next_tile are reused
    }
}

// C tile = epilogue(sum over the splits, in split order) -- deterministic two-pass split-K
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs g, const int32_t* __restrict__ table,
                                                            int32_t ntiles, int32_t ksplit,
                                                            const double* __restrict__ work) {
    const int t = blockIdx.x;
    const int32_t packed = table[t];
    const int64_t i0 = (int64_t)(packed >> 16) * BM, j0 = (int64_t)(packed & 0xFFFF) * BN;
    const int li = threadIdx.x & (BM - 1);
    const int64_t gi = i0 + li;
    // eight columns per pass with all their loads issued before the first store, every load unconditional (clamped
    // addresses; the partial tiles are whole): a load under a condition is followed by its own s_waitcnt -- one
    // dependent round trip per element made this kernel 60-80 us for a hundred tiles
    constexpr int U = 8;
    const bool has_cin = (g.Cin != nullptr), has_dvec = (g.dvec != nullptr);
    const int64_t gic = gi < g.M ? gi : g.M - 1;
    for (int lj0 = threadIdx.x >> 7; lj0 < BN; lj0 += 2 * U) {  // lj0 + 2u <= 127
        double sum[U], cin[U], dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t gj = j0 + lj0 + 2 * u, gjc = gj < g.N ? gj : g.N - 1;
            sum[u] = 0.0;
            cin[u] = has_cin ? g.Cin[gic + gjc * g.ldcin] : 0.0;
            dv[u] = has_dvec ? g.dvec[gjc] : 0.0;
        }
        for (int sp = 0; sp < ksplit; ++sp) {  // split order: the same result on every run
            const double* w = work + ((int64_t)sp * ntiles + t) * (BM * BN) + li;
#pragma unroll
            for (int u = 0; u < U; ++u) sum[u] += w[(lj0 + 2 * u) * BM];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t gj = j0 + lj0 + 2 * u;
            if (!(gi < g.M && gj < g.N) || (g.lower_only && gi + g.diag_off < gj)) continue;
            double val = g.alpha * sum[u];
            if (has_cin) val += g.beta * cin[u];
            if (has_dvec && gi + g.diag_off == gj) val += dv[u];
            g.C[gi + gj * g.ldc] = val;
        }
    }
}

// Identity of a tile table: what gemm_tile_table builds it from.  An unmasked product has an empty mask, which allocates
// nothing; a masked one (the distributed driver: hundreds of masks per context) copies its mask once per call.
struct TableKey {
    int64_t tm, tn, flags, doff;  // tile counts; lower_only | partial last tile row << 1 | column << 2; diag_off if lower
    GemmMask kind;
    std::vector<int64_t> mask;  // the column ranges / per-column first rows
    bool operator<(const TableKey& o) const {
        return std::tie(tm, tn, flags, doff, kind, mask) < std::tie(o.tm, o.tn, o.flags, o.doff, o.kind, o.mask);
    }
};
struct TableVal {
    int32_t* d;
    int32_t n;
};
// per-context cache of tile tables.  A context is used by one host thread at a time, different
// contexts may live on different threads (batch sharding): the outer map is guarded by a mutex,
// the inner map belongs to its context's thread (std::map nodes are address stable).
std::mutex& table_mutex() {
    static std::mutex m;
    return m;
}
std::map<madqp_ctx*, std::map<TableKey, TableVal>>& table_cache() {
    static std::map<madqp_ctx*, std::map<TableKey, TableVal>> c;
    return c;
}
std::map<TableKey, TableVal>& tables_of(madqp_ctx* ctx) {
    std::lock_guard<std::mutex> lock(table_mutex());
    return table_cache()[ctx];
}

const GemmModes& gemm_modes() {  // the environment switches, read once, at the first use
    static const GemmModes modes = [] {
        auto num = [](const char* name, int64_t dflt) { return getenv(name) ? (int64_t)atoi(getenv(name)) : dflt; };
        GemmModes m;
        m.splitk = (int)num("MADQP_GEMM_SPLITK", m.splitk);
        m.tailsplit = (int)num("MADQP_GEMM_TAILSPLIT", m.tailsplit);
        m.seg_rounds = (int)num("MADQP_GEMM_SEG_ROUNDS", m.seg_rounds);
        m.xcd = (int)num("MADQP_GEMM_XCD", m.xcd);
        m.batch_xcd = (int)num("MADQP_GEMM_BATCH_XCD", m.batch_xcd);
        m.patch_m = num("MADQP_GEMM_PATCH_M", m.patch_m);  // (tuning knobs for experiments)
        m.patch_n = num("MADQP_GEMM_PATCH_N", m.patch_n);
        return m;
    }();
    return modes;
}

// The n tiles at `table` cut into S chunks of K, one workgroup per (tile, chunk), raw partial tiles to the workspace;
// splitk_reduce_kernel sums them in chunk order and applies the epilogue: same result on every run.
int32_t launch_split(madqp_ctx* ctx, KArgs ka, const int32_t* table, int32_t n, int32_t S, int64_t chunk) {
    ka.table = table, ka.ntiles = n, ka.ksplit = S, ka.kchunk = chunk, ka.work = ctx->d_work;
    hipLaunchKernelGGL(gemm_tn_f64_kernel, dim3(n, (unsigned)S), dim3(NTHREADS), 0, ctx->stream, ka);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, ka.g, table, n, S, ka.work);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}
}  // namespace

void madqp_gemm_release_tables(madqp_ctx* ctx) {
    std::map<TableKey, TableVal> mine;
    {
        std::lock_guard<std::mutex> lock(table_mutex());
        auto& all = table_cache();
        auto it = all.find(ctx);
        if (it == all.end()) return;
        mine.swap(it->second);
        all.erase(it);
    }
    for (auto& kv : mine) (void)hipFree(kv.second.d);
}

// Validates, fetches the tile table, asks gemm_plan (gemm_plan.inc) what to launch and launches it.
int32_t madqp_gemm_tn(madqp_ctx* ctx, const GemmArgs& a, int prof_cls, const int64_t* cols, int64_t ncols,
                      const GemmBatch* batch, madqp_debug_gemm_info* info) {
    if (info) {  // (test seam only, madqp_debug_gemm_tn: what this call launched; filled from the plan at the end)
        *info = madqp_debug_gemm_info{};
        info->gemm_slots = ctx ? ctx->gemm_slots : 0;
    }
    ARG_TRY(ctx, a.M >= 0 && a.N >= 0 && a.K >= 0 && a.X && a.Y && a.C);
    if (a.M == 0 || a.N == 0) return MADQP_OK;
    const int64_t tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
    ARG_TRY(ctx, tiles_m < 65536 && tiles_n < 32768);
    const GemmModes& md = gemm_modes();
    TableKey key{tiles_m, tiles_n, (a.lower_only ? 1 : 0) | ((a.M % BM) != 0 ? 2 : 0) | ((a.N % BN) != 0 ? 4 : 0),
                 a.lower_only ? a.diag_off : 0, GEMM_MASK_NONE, {}};
    if (cols) {
        for (int64_t r = 0; r < 2 * ncols; ++r)
            ARG_TRY(ctx, cols[r] >= 0 && cols[r] <= a.N && (cols[r] % BN == 0 || cols[r] == a.N));
        key.kind = GEMM_MASK_COLS;
        key.mask.assign(cols, cols + 2 * ncols);
    }
    if (a.tile_row0) {  // per-column first active tile row
        ARG_TRY(ctx, !cols && !a.lower_only);
        key.kind = GEMM_MASK_ROW0;
        key.mask.assign(a.tile_row0, a.tile_row0 + tiles_n);
    }
    auto& cache = tables_of(ctx);
    auto it = cache.find(key);
    if (it == cache.end()) {
        const std::vector<int32_t> tab = gemm_tile_table(a.M, a.N, a.lower_only != 0, a.diag_off, key.kind, key.mask.data(),
                                                         (int64_t)key.mask.size(), md.patch_m, md.patch_n);
        TableVal v{nullptr, (int32_t)tab.size()};
        if (!tab.empty()) {
            HIP_TRY(ctx, hipMalloc(&v.d, tab.size() * sizeof(int32_t)));
            HIP_TRY(ctx, hipMemcpyAsync(v.d, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        it = cache.emplace(std::move(key), v).first;
    }
    if (it->second.n == 0) return MADQP_OK;
    const int32_t* table = it->second.d;
    const GemmPlan p = gemm_plan(it->second.n, a.K, ctx->gemm_slots, ctx->gemm_cap_slots,
                                 !batch ? GEMM_SINGLE : batch->list ? GEMM_BATCH_LIST : GEMM_BATCH, batch ? batch->B : 1, md);
    ARG_TRY(ctx, p.gy <= 65535);
    if (int32_t r = madqp_work_reserve(ctx, p.work_bytes)) return r;  // (nothing for a launch of whole tiles)
    auto al16 = [](const void* ptr) { return ((uintptr_t)ptr & 15) == 0; };
    const int32_t fast_ok = al16(a.X) && al16(a.Y) && (a.ldx % 2 == 0) && (a.ldy % 2 == 0);
    KArgs ka{a, table, p.ntiles, fast_ok, md.xcd, p.batch_xcd, batch ? *batch : GemmBatch{1, 0, 0, 0, 0, 0, nullptr},
             1, a.K, nullptr};  // (whole tiles; launch_split sets the three split fields)
#ifdef MADQP_STAMPS
    extern unsigned long long* madqp_stamp_buffer;
    ka.stamps = madqp_stamp_buffer;
#endif
    ProfScope ps(ctx, prof_cls);
    if (p.persistent) {
        if (!ctx->d_tickets) HIP_TRY(ctx, hipMalloc(&ctx->d_tickets, 8 * sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_tickets, 0, 8 * sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(gemm_tn_f64_persistent_kernel, dim3((unsigned)p.persistent), dim3(NTHREADS), 0, ctx->stream, ka,
                           ctx->d_tickets);
        LAUNCH_CHECK(ctx);
    } else if (p.ksplit > 1) {
        if (int32_t r = launch_split(ctx, ka, table, p.whole, p.ksplit, p.kchunk)) return r;
    } else {
        for (int64_t off = 0; off < p.whole; off += ka.ntiles) {
            ka.table = table + off;
            ka.ntiles = (int32_t)gemm_segment(p, off);
            hipLaunchKernelGGL(gemm_tn_f64_kernel, dim3(ka.ntiles, p.gy), dim3(NTHREADS), 0, ctx->stream, ka);
            LAUNCH_CHECK(ctx);
        }
    }
    if (p.tail_tiles)  // the tiles of the last round, K-split
        if (int32_t r = launch_split(ctx, ka, table + p.whole, p.tail_tiles, p.tail_split, p.tail_chunk)) return r;
    if (info)
        *info = madqp_debug_gemm_info{p.ntiles, p.ksplit, p.tail_tiles ? p.tail_chunk : p.kchunk, p.tail_tiles, p.tail_split,
                                      p.segments, p.persistent, fast_ok, p.batch_xcd, ctx->gemm_slots};
    return MADQP_OK;
}

namespace {
// S[k, :] = sqrt(w[k]) * B[k, :], zero padded to npad columns and kpad rows: one streaming pass
// (16 n kdim bytes).  The assembly then is the plain product S'S with BOTH operands read from this
// library-owned, 128-aligned image: no per-k scaling inside the MFMA loop (every VALU instruction
// there costs matrix-pipe cycles), a single operand stream, and no partial tiles.
__global__ __launch_bounds__(256) void scale_rows_kernel(int64_t n, int64_t npad, int64_t kdim,
                                                         const double* __restrict__ B, int64_t ldb,
                                                         const double* __restrict__ w,
                                                         double* __restrict__ out, int vec) {
    const int64_t k = blockIdx.y;
    double* dst = out + k * npad;
    if (k >= kdim) {  // zero rows up to a multiple of 16
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npad; i += (int64_t)gridDim.x * 256)
            dst[i] = 0.0;
        return;
    }
    const double wk = sqrt(w[k]);
    const double* src = B + k * ldb;
    if (vec) {
        const int64_t pairs = npad >> 1, full = n >> 1;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * 256) {
            double2_t v = {0.0, 0.0};
            if (p < full) {
                v = *reinterpret_cast<const double2_t*>(src + 2 * p);
                v.x *= wk;
                v.y *= wk;
            } else if (2 * p < n) {
                v.x = src[2 * p] * wk;
            }
            *reinterpret_cast<double2_t*>(dst + 2 * p) = v;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npad; i += (int64_t)gridDim.x * 256)
            dst[i] = (i < n) ? src[i] * wk : 0.0;
    }
}
}  // namespace

// Lower triangle of C = base + diag(dvec) + B' diag(w) B (declared in common.h: kkt.hip assembles through it).
int32_t madqp_syrk_assemble_impl(madqp_ctx* ctx, int64_t n, int64_t kdim, const double* B, int64_t ldb, const double* w,
                                 const double* base, int64_t ldbase, const double* dvec, double* C, int64_t ldc) {
    ARG_TRY(ctx, n >= 0 && kdim >= 0 && C && ldc >= n && (kdim == 0 || (B && ldb >= n)));
    ARG_TRY(ctx, !base || ldbase >= n);
    const double* X = B ? B : C;  // K == 0: never dereferenced
    int64_t ldx = ldb, K = kdim, npad = 0;
    if (w && kdim > 0 && n > 0) {
        npad = (n + BM - 1) / BM * BM;
        const int64_t kpad = (kdim + BK - 1) / BK * BK;
        const size_t bytes = (size_t)kpad * npad * sizeof(double);
        if (bytes > ctx->scaled_bytes) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->d_scaled) HIP_TRY(ctx, hipFree(ctx->d_scaled));
            ctx->d_scaled = nullptr;
            ctx->scaled_bytes = 0;
            hipError_t e = hipMalloc(&ctx->d_scaled, bytes);
            if (e != hipSuccess)
                return madqp_fail(ctx, MADQP_ERR_ALLOC, "scaled operand hipMalloc(%zu): %s", bytes,
                                  hipGetErrorString(e));
            ctx->scaled_bytes = bytes;
        }
        const int vec = ((((uintptr_t)B) & 15) == 0) && (ldb % 2 == 0);
        {
            ProfScope ps(ctx, MADQP_PROF_VEC);
            const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((npad / 2 + 255) / 256, 64));
            hipLaunchKernelGGL(scale_rows_kernel, dim3(gx, (unsigned)kpad), dim3(256), 0, ctx->stream, n,
                               npad, kdim, B, ldb, w, ctx->d_scaled, vec);
            LAUNCH_CHECK(ctx);
        }
        X = ctx->d_scaled;
        ldx = npad;
        K = kpad;
    }
    GemmArgs g{};
    g.X = X;
    g.ldx = ldx;
    g.Y = X;
    g.ldy = ldx;
    g.K = K;
    if (npad) g.Mread = g.Nread = npad;
    g.C = C;
    g.ldc = ldc;
    g.Cin = base;
    g.ldcin = ldbase;
    g.dvec = dvec;
    g.alpha = 1.0;
    g.beta = 1.0;
    g.M = n;
    g.N = n;
    g.diag_off = 0;
    g.lower_only = 1;
    return madqp_gemm_tn(ctx, g, MADQP_PROF_SYRK);
}

extern "C" int32_t madqp_syrk_assemble(madqp_ctx* ctx, int64_t n, int64_t kdim, const double* B,
                                       int64_t ldb, const double* w, const double* base,
                                       int64_t ldbase, const double* dvec, double* C,
                                       int64_t ldc) {
    ARG_TRY(ctx, ctx != nullptr);
    return madqp_syrk_assemble_impl(ctx, n, kdim, B, ldb, w, base, ldbase, dvec, C, ldc);
}

// Test seam: one call of madqp_gemm_tn with every argument in the caller's hands, and a report of the launch form the
// dispatcher chose (tests/test_gpu_gemm_paths.py).  Not part of the solver's interface.
extern "C" int32_t madqp_debug_gemm_tn(madqp_ctx* ctx, const madqp_debug_gemm* d, madqp_debug_gemm_info* info) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, d != nullptr && d->cap_slots >= 0 && d->ncols >= 0 && d->B >= 0);
    GemmArgs g{};
    g.X = d->X;
    g.ldx = d->ldx;
    g.Y = d->Y;
    g.ldy = d->ldy;
    g.C = d->C;
    g.ldc = d->ldc;
    g.Cin = d->Cin;
    g.ldcin = d->ldcin;
    g.dvec = d->dvec;
    g.alpha = d->alpha;
    g.beta = d->beta;
    g.M = d->M;
    g.N = d->N;
    g.K = d->K;
    g.Mread = d->Mread;
    g.Nread = d->Nread;
    g.diag_off = d->diag_off;
    g.lower_only = d->lower_only ? 1 : 0;
    g.tile_row0 = d->tile_row0_host;
    const GemmBatch bt{d->B, d->sX, d->sY, d->sC, d->sCin, d->sD, d->skip, d->list, d->count};
    const int64_t cap0 = ctx->gemm_cap_slots;
    ctx->gemm_cap_slots = d->cap_slots;
    const int32_t r = madqp_gemm_tn(ctx, g, MADQP_PROF_POTRF_GEMM, d->cols_host, d->cols_host ? d->ncols : 0,
                                    d->B > 0 ? &bt : nullptr, info);
    ctx->gemm_cap_slots = cap0;
    return r;
}

// ------------------------------------------------------------------ hardware probe
namespace {
__global__ __launch_bounds__(256) void mfma_f64_probe_kernel(int iters, double* sink) {
    double4_t acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = double4_t{0.0, 0.0, 0.0, 0.0};
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    // inline asm pins the accumulators in VGPRs: with the builtin the compiler parks them in AGPRs and the
    // loop measures its accvgpr copies (47 instead of 77.7 TFLOP/s; tools/mfma_probe.hip)
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b));
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) sink[0] = s;  // keep the chain alive
}
}  // namespace

extern "C" int32_t madqp_probe_mfma_f64(madqp_ctx* ctx, int32_t iters, double* tflops_host) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, iters > 0 && tflops_host);
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int blocks = prop.multiProcessorCount * 2;  // two 256-thread workgroups per CU
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    hipLaunchKernelGGL(mfma_f64_probe_kernel, dim3(blocks), dim3(256), 0, ctx->stream, 64, ctx->d_res);
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    hipLaunchKernelGGL(mfma_f64_probe_kernel, dim3(blocks), dim3(256), 0, ctx->stream, iters, ctx->d_res);
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    const double flops = (double)blocks * 4.0 * (double)iters * 8.0 * 2048.0;
    *tflops_host = flops / (ms * 1e-3) * 1e-12;
    return MADQP_OK;
}
