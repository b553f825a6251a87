// Internal helpers shared by the translation units of libmadqp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/madqp.h"

#define MADQP_RESULT_SLOTS 128
// last slot of the result block: device-side fault word (non-zero: a triangular sweep's hand-off timed out);
// it rides along with every synchronising scalar read-back (madqp_read_results) and turns into MADQP_ERR_HIP
#define MADQP_FAULT_SLOT (MADQP_RESULT_SLOTS - 1)
#include "mpc_rules.inc"  // where the fused iteration keeps what in the block (MPC_SL_*, MPC_W_*), and its scalar rules

struct ProfEvent {
    hipEvent_t a, b;
    int cls;
};

struct madqp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t gemm_slots = 512;  // resident GEMM workgroups: 2 per CU
    // > 0: GEMM launches with more tiles than (gemm_slots - gemm_cap_slots) run as ONE persistent launch of that many
    // workgroups drawing tiles from per-XCD ticket counters, leaving gemm_cap_slots workgroup slots of the chip free
    // for kernels on other streams (dist.hip: the collectives beside a trailing update).  0: one workgroup per tile.
    int64_t gemm_cap_slots = 0;
    unsigned long long* d_tickets = nullptr;  // 8 counters, zeroed on the stream before every capped launch
    char err[512] = {0};
    // scalar results: device block + pinned host mirror
    double* d_res = nullptr;
    double* h_res = nullptr;
    // reduction partials (MADQP_MAX_BLOCKS x MADQP_RESULT_SLOTS doubles)
    double* d_part = nullptr;
    // generic workspace for deterministic two-pass gemv
    double* d_work = nullptr;
    size_t work_bytes = 0;
    // scaled copy of the assembly operand (Theta A), grow-only
    double* d_scaled = nullptr;
    size_t scaled_bytes = 0;
    // profiling
    uint32_t prof = 0;  // bit mask of enabled MADQP_PROF_* classes
    std::vector<ProfEvent> pending;
    std::vector<hipEvent_t> pool;
    double prof_ms[MADQP_PROF_COUNT] = {0};
    int64_t prof_n[MADQP_PROF_COUNT] = {0};
};

static inline int32_t madqp_fail(madqp_ctx* ctx, int32_t code, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return madqp_fail((ctx), MADQP_ERR_HIP, "%s failed: %s (%s:%d)", #expr,          \
                              hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

#define ARG_TRY(ctx, cond)                                                                   \
    do {                                                                                     \
        if (!(cond))                                                                         \
            return madqp_fail((ctx), MADQP_ERR_ARG, "bad argument: %s (%s:%d)", #cond,       \
                              __FILE__, __LINE__);                                           \
    } while (0)

#define LAUNCH_CHECK(ctx) HIP_TRY(ctx, hipGetLastError())

// ctx.hip
int32_t madqp_work_reserve(madqp_ctx* ctx, size_t bytes);
void madqp_prof_begin(madqp_ctx* ctx, int cls);
void madqp_prof_end(madqp_ctx* ctx);
int32_t madqp_read_results(madqp_ctx* ctx, int count, double* out_host);
// queued reductions (vec_kernels.hip, kkt.hip, chol.hip): results stay in ctx->d_res at the given slot until one
// madqp_read_results fetches the block (slots 0 .. MADQP_FAULT_SLOT-1)
int32_t madqp_q_compl(madqp_ctx* ctx, const madqp_state* st, int affine, double ap, double ad, const double* a8,
                      int slot0);                                                               // MPC_W_COMPL slots: sums
int32_t madqp_q_alpha_max(madqp_ctx* ctx, const madqp_state* st, double tau, int slot0);        // MPC_W_ALPHA slots
// the same with a scalar that stays in device memory (mpc.hip, body_fused: no read-back between predictor and corrector)
int32_t madqp_q_alpha_max_dev(madqp_ctx* ctx, const madqp_state* st, double tau, const double* tau_dev, int slot0);
int32_t madqp_set_correction_rhs_dev(madqp_ctx* ctx, const madqp_state* st, const double* mu_dev);
// (vec_kernels.hip: with mu_dev, beta_min and beta_max are multiplied by *mu_dev on the device; a8 as madqp_q_compl's)
int32_t madqp_set_extra_correction_dev(madqp_ctx* ctx, const madqp_state* st, double alpha_p, double alpha_d, double beta_min,
                                       double beta_max, const double* mu_dev, const double* a8 = nullptr);
// One-thread kernels on the block, each a rule of mpc_rules.inc between the fields it names there:
// GZ_ALPHA -> TRIAL_ALPHA; COMPL -> BARRIER; the two sums at compl_slot and mu_curr -> MUC; the block -> DECISION
int32_t madqp_q_mpc_trial_alpha(madqp_ctx* ctx);
int32_t madqp_q_mpc_mu(madqp_ctx* ctx, int64_t nb, double mu_min, int step_rule, double step_param);
int32_t madqp_q_mpc_muc(madqp_ctx* ctx, int compl_slot, int64_t nb);
int32_t madqp_q_mpc_decide(madqp_ctx* ctx, const MpcDecideOpt& opt);
int32_t madqp_copy_if_dev(madqp_ctx* ctx, int64_t len, const double* src, double* dst, const double* flag_dev);
// madqp_update_iterates / madqp_adjust_boundary gated by the DECISION words in device memory (nullptr: the extern "C"
// forms); with them the step lengths are the decided ones, and mu is read from *mu_dev
int32_t madqp_update_iterates_dev(madqp_ctx* ctx, const madqp_state* st, double alpha_p, double alpha_d,
                                  const double* dec_dev);
int32_t madqp_adjust_boundary_dev(madqp_ctx* ctx, const madqp_state* st, double mu, const double* dec_dev,
                                  const double* mu_dev);
// the result block on its way to a pinned host copy, marked by an event: the host waits for the event, not for the stream
int32_t madqp_results_post(madqp_ctx* ctx, double* h_dst, hipEvent_t ev);
int32_t madqp_results_wait(madqp_ctx* ctx, const double* h_src, hipEvent_t ev, int count, double* out_host);
int32_t madqp_q_inf(madqp_ctx* ctx, const madqp_state* st, int slot0);                          // MPC_W_INF slots
void madqp_inf_from_block(const double* out4, double* out3);
int32_t madqp_q_norm_inf3(madqp_ctx* ctx, int64_t len, const double* a, const double* b, const double* c,
                          int slot0);                                                           // MPC_W_NRM slots
int32_t madqp_q_kkt_eval(madqp_kkt* k, const madqp_state* st, const double* q, const double* rhs, int slot0);  // MPC_W_EVAL
int32_t madqp_q_kkt_factorize(madqp_kkt* k, int slot0);                                         // MPC_W_INFO slot: info
// w = K^-1 p, optionally pcopy = p (kkt.hip: the condensed mode runs its per-variable passes fused)
int32_t madqp_kkt_solve_from(madqp_kkt* k, const madqp_state* st, const double* p, double* w, double* pcopy);
int32_t madqp_chol_factor_q(madqp_chol* s, double* A, int64_t lda, double* d_slot);  // info -> *d_slot, no read-back

struct ProfScope {
    madqp_ctx* c;
    bool on;
    ProfScope(madqp_ctx* ctx, int cls) : c(ctx), on((ctx->prof >> cls) & 1u) {
        if (on) madqp_prof_begin(c, cls);
    }
    ~ProfScope() {
        if (on) madqp_prof_end(c);
    }
};
// one timer scope for a whole call: the scopes of the launches inside are switched off while this lives
struct ProfMute {
    madqp_ctx* c;
    uint32_t saved;
    explicit ProfMute(madqp_ctx* ctx) : c(ctx), saved(ctx->prof) { c->prof = 0; }
    ~ProfMute() { c->prof = saved; }
};

// gemm_f64.hip
struct GemmArgs {
    const double* X;  // X[i + k*ldx], i in [0,M)
    int64_t ldx;
    const double* Y;  // Y[j + k*ldy], j in [0,N)
    int64_t ldy;
    double* C;        // out C[i + j*ldc]
    int64_t ldc;
    const double* Cin;  // optional addend, same indexing with ldcin (may alias C).  When given, the kernel computes
                        // alpha*acc + beta*Cin as written: beta = 0 does NOT ignore a NaN / Inf in Cin as BLAS would
                        // (pass nullptr for "no addend")
    int64_t ldcin;
    const double* dvec;  // optional: added where (i + diag_off == j), indexed by j
    double alpha, beta;  // out = alpha*acc + beta*Cin (+ dvec)
    int64_t M, N, K;
    int64_t Mread, Nread;  // rows of X / Y that may be READ (>= M, N; 0 = M, N): operands padded to a
                           // multiple of 128 let edge tiles take the fast path, stores stay masked to M, N
    int64_t diag_off;  // global_row(i) - global_col(j) = i - j + diag_off
    int lower_only;    // 1: write only elements with i + diag_off >= j; skip tiles above
    const int64_t* tile_row0;  // optional HOST array, one entry per 128-column tile of C: the first 128-row tile that is
                               // computed in that tile column (block-cyclic local matrices: "global tile row >= global
                               // tile column" is a per-column suffix, not an affine rule); whole tiles are written
};
// cols: optional host list of ncols column ranges [cols[2r], cols[2r+1]) (multiples of 128 relative to
// C) -- only output tiles whose columns fall in one of them are computed (multi-GPU path: the block
// columns a rank owns, in ONE launch)
// batch: optional -- the same product for B problems laid out at fixed strides (doubles) from the
// pointers of `a` (grid.y = problem); problems with skip[b] != 0 are left untouched
struct GemmBatch {
    int64_t B;
    int64_t sX, sY, sC, sCin, sD;
    const int32_t* skip;
    // compacted form (the masked x100-retry rounds of the batched engine): the launch has B "slots" in grid.y and slot y
    // works off the problems list[y], list[y + B], .. < *count -- with nothing to retry (the usual case) every workgroup
    // of the launch leaves after one load instead of B problems' worth of workgroups reading their skip word
    const int32_t* list = nullptr;
    const int32_t* count = nullptr;
};
// info: optional report of the launch form chosen (the test seam madqp_debug_gemm_tn; nullptr everywhere else)
int32_t madqp_gemm_tn(madqp_ctx* ctx, const GemmArgs& a, int prof_cls, const int64_t* cols = nullptr,
                      int64_t ncols = 0, const GemmBatch* batch = nullptr, madqp_debug_gemm_info* info = nullptr);

void madqp_gemm_release_tables(madqp_ctx* ctx);

// chol.hip: recursive blocked factorisation of B equally sized matrices (see there)
int32_t madqp_chol_factor_batched(madqp_ctx* ctx, double* A, int64_t lda, int64_t n, int64_t sA, double* winv,
                                  int64_t sW, int32_t* info, int64_t B, const int32_t* skip, int64_t slots = 0,
                                  const int32_t* list = nullptr, const int32_t* count = nullptr);

// gemv.hip (internal entry with explicit class)
int32_t madqp_gemv_impl(madqp_ctx* ctx, int32_t trans, int64_t rows, int64_t cols, double alpha,
                        const double* A, int64_t lda, const double* x, double beta, double* y,
                        int prof_cls);
// gemv_many.hip: the same product on nrhs columns (X + c ldx -> Y + c ldy), A read once per MADQP_GEMV_MANY_GROUP columns.
// work: at least madqp_gemv_many_workspace(..) doubles for the partial sums of the k ranges, or nullptr = the context's
constexpr int64_t MADQP_GEMV_MANY_GROUP = 128;  // MANY_TC of many_plan.inc
int64_t madqp_gemv_many_workspace(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs);
int32_t madqp_gemv_many_impl(madqp_ctx* ctx, int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, double alpha,
                             const double* A, int64_t lda, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy,
                             double* work, int prof_cls);

// y(n) = alpha H x + beta y for a symmetric H (row r at H + r*ldh) from its LOWER triangle only: half the bytes of the
// general product (gemv.hip)
bool madqp_symv_lower_reads_triangle(int64_t n, const double* H, int64_t ldh);
int32_t madqp_symv_lower(madqp_ctx* ctx, int64_t n, double alpha, const double* H, int64_t ldh, const double* x,
                         double beta, double* y, int prof_cls);
// only the entries H[r*ldh + c] with c >= r are read, at every size (H 16-byte aligned, ldh even)
int32_t madqp_symv_upper(madqp_ctx* ctx, int64_t n, double alpha, const double* H, int64_t ldh, const double* x,
                         double beta, double* y, int prof_cls);

// sparse.hip: a CSR matrix in device memory (int64 indices, column indices ascending within a row), borrowed
struct Csr {
    const int64_t* ptr = nullptr;
    const int64_t* col = nullptr;
    const double* val = nullptr;
};
int32_t madqp_spmv_csr(madqp_ctx* ctx, int64_t rows, const Csr& a, double alpha, const double* x, double beta, double* y,
                       int prof_cls);
// the same on nrhs columns, bitwise the column loop; the CSR arrays are read once per MADQP_SPMM_GROUP columns
constexpr int MADQP_SPMM_GROUP = 32;
int32_t madqp_spmm_csr(madqp_ctx* ctx, int64_t rows, const Csr& a, double alpha, const double* X, int64_t ldx, double beta,
                       double* Y, int64_t ldy, int64_t nrhs, int prof_cls);
// C = base + diag(dvec) + V diag(w) V' (lower triangle) from the rows of V (v) and the rows of V' (vt); the base dense
// (base, ldbase), a symmetric matrix with both triangles in CSR (b), or none
int32_t madqp_sparse_gram(madqp_ctx* ctx, int64_t n, const Csr& v, const Csr& vt, const double* w, const double* base,
                          int64_t ldbase, const double* dvec, const Csr& b, double* C, int64_t ldc);
// the band form (madqp_kkt_set_bandwidth): column j over the rows j .. min(n-1, j+extent), zeros beyond j+bw; sparse or no base
int32_t madqp_sparse_gram_band(madqp_ctx* ctx, int64_t n, const Csr& v, const Csr& vt, const double* w, const double* dvec,
                               const Csr& b, double* C, int64_t ldc, int64_t bw, int64_t extent);

// gemm_f64.hip: lower triangle of C = base + diag(dvec) + B' diag(w) B (madqp_syrk_assemble without its ctx check)
int32_t madqp_syrk_assemble_impl(madqp_ctx* ctx, int64_t n, int64_t kdim, const double* B, int64_t ldb, const double* w,
                                 const double* base, int64_t ldbase, const double* dvec, double* C, int64_t ldc);

// The device buffers an object owns (madqp_kkt, madqp_dkkt, madqp_batch, madqp_chol): every allocation is recorded and freed by
// release() or the destructor.  `who` is the caller's name for the message of a failure.
struct DevOwner {
    madqp_ctx* ctx = nullptr;
    std::vector<void*> owned;
    DevOwner() = default;
    explicit DevOwner(madqp_ctx* c) : ctx(c) {}
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    ~DevOwner() { release(); }
    // max(count, 1) elements, optionally zeroed on the stream
    template <class T>
    int32_t alloc(T** p, int64_t count, const char* who, bool zero = false) {
        *p = nullptr;
        const size_t bytes = (size_t)(count > 1 ? count : 1) * sizeof(T);
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            return madqp_fail(ctx, MADQP_ERR_ALLOC, "%s: hipMalloc(%zu): %s", who, bytes, hipGetErrorString(e));
        }
        owned.push_back(*p);
        if (zero && (e = hipMemsetAsync(*p, 0, bytes, ctx->stream)) != hipSuccess)
            return madqp_fail(ctx, MADQP_ERR_HIP, "%s: hipMemset: %s", who, hipGetErrorString(e));
        return MADQP_OK;
    }
    // A grow-only buffer of *have elements (contents are not kept).  Kernels in flight may still read the old buffer, so
    // the stream is synchronised before it is freed.  After a failure the buffer is gone: *p == nullptr, *have == 0.
    template <class T>
    int32_t grow(T** p, int64_t* have, int64_t want, const char* who) {
        if (*p && want <= *have) return MADQP_OK;
        if (*p) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)free_one(p);
        }
        *have = 0;
        const int32_t r = alloc(p, want, who);
        if (!r) *have = want;
        return r;
    }
    // the buffers of another owner become this one's
    void take(DevOwner& o) {
        owned.insert(owned.end(), o.owned.begin(), o.owned.end());
        o.owned.clear();
    }
    // frees the buffers recorded at position `from` and later (0: all of them)
    void release(size_t from = 0) {
        while (owned.size() > from) {
            (void)hipFree(owned.back());
            owned.pop_back();
        }
    }
    // frees one buffer now (the caller knows that nothing on the stream still uses it); *p == nullptr afterwards
    template <class T>
    hipError_t free_one(T** p) {
        for (size_t i = 0; i < owned.size(); ++i)
            if (owned[i] == *p) {
                owned.erase(owned.begin() + (std::ptrdiff_t)i);
                break;
            }
        const hipError_t e = *p ? hipFree(*p) : hipSuccess;
        *p = nullptr;
        return e;
    }
};

// chol.hip: the panel solve of one 128-column block, X (rows x 128) <- X L^-T by block substitution (see there); w < 128 only
// with rows <= 0 (a short block is the last of its matrix or tile).  (The products with the 128 x 128 inverse of rounds
// 1-3 were removed; their A/B numbers: DESIGN.md 4.1 and 5.2.)
struct CholTarget;
int32_t madqp_chol_panel_solve(madqp_ctx* ctx, double* X, int64_t ldx, int64_t rows, int64_t rows_read, const double* L,
                               int64_t ldl, const double* Wcm, int64_t w, const CholTarget* batch = nullptr);
// chol.hip: one triangular sweep over an order-w tile whose factor and inverse diagonal blocks are given (dist.hip):
// trans = 0: v <- L^-1 v, trans = 1: v <- L^-T v.  tmp: w doubles, ctl: 4 ints of device scratch.
int32_t madqp_trsv_tile(madqp_ctx* ctx, int32_t trans, const double* L, int64_t ld, const double* winv, double* v,
                        int64_t w, double* tmp, int32_t* ctl);

// chol.hip, for the grid path (dist.hip), which knows the handle by these alone: its order, and the packed image
// (panel_image.h) of the DIAGONAL part of a factored panel -- buf = [info, 0 | inverse blocks of the panel |
// L(j0:j0+w, j0:j0+w), leading dimension w].  j0 = 0, w = n: what madqp_chol_panel_pack writes.
int64_t madqp_chol_order(const madqp_chol* s);
int32_t madqp_chol_pack_diag(madqp_chol* s, int64_t j0, int64_t w, double* buf);
