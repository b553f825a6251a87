// Batches of small, equally shaped QPs (BASELINE configs[3], SURVEY.md 8e "persistent kernel or per-QP
// convergence mask"): B problems advance in lock step, a handful of launches per iteration for the
// whole batch instead of ~60 launches (and ~12 host round trips) per problem.
//
//   * dense MFMA work is batched: ONE launch of the GEMM core assembles K_b = H_b + Sigma_b + A_b' Theta_b A_b
//     for all b (grid.y = problem), the recursive Cholesky runs as ~10 launches for all b
//     (madqp_chol_factor_batched: diagonal kernel with grid = B, TRSM / update GEMMs with grid.y = B);
//   * everything else of an iteration -- residuals, termination test, right-hand sides, the
//     condensed solves with their triangular sweeps, the residual check of solve_system!, step
//     lengths, centering, iterate update, model callbacks -- is ONE workgroup per problem running the
//     kernel bodies of vec_kernels.inc / kkt_kernels.inc back to back (compiled here as device
//     functions with a workgroup-stride loop): the per-problem scalars (mu, alpha, norms) never leave
//     the chip, and a problem that has converged (or failed) is masked out by its status word;
//   * the host only reads the status words (one small copy per call of madqp_batch_iterate).
//
// Same arithmetic as the single-problem path (src/solver.jl:127-182, 254-345 in the same order);
// sums are accumulated in a different order, so results agree to rounding, not bitwise.  All step
// rules, Gondzio's corrections and the x100 regularization retry of src/linear_solver.jl:6-17 (two extra, masked
// assembly + Cholesky rounds per iteration that only the problems whose factorisation failed take part in) are in,
// and so is the reference's own formulation: normal equations A Sigma^-1 A' of order m (opt.kkt_form = 1, LP only).
// The problems share (nx, m); which bounds are finite and which rows are inequalities may differ from problem to problem
// (madqp_batch_create_patterns): the MFMA work does not depend on it, the workgroup programs take problem b's counts and
// list offsets from its row of the pattern table (BQ::pat), its [B][n] arrays at stride nx + max ns_b.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "kkt_form.inc"

typedef double double2_t __attribute__((ext_vector_type(2)));

namespace {
constexpr int NB = 128;
constexpr int64_t WBLK = 2 * NB * NB;


enum {
    S_MU = 0, S_ALPHA_P, S_ALPHA_D, S_OBJ, S_INF_PR, S_INF_DU, S_INF_COMPL, S_DNORM, S_NORM_B, S_NORM_C,
    S_DEL_W, S_DEL_C, S_RATIO, S_REG_P, S_REG_D, S_NFACT, S_COUNT
};
static_assert(S_COUNT == MADQP_BATCH_SCALARS, "scalar block layout is part of the ABI");
// one record of the per-iteration trace (madqp_batch_set_trace)
enum { T_OBJ = 0, T_INF_PR, T_INF_DU, T_INF_COMPL, T_MU, T_DNORM, T_DEL_W, T_ALPHA_P, T_ALPHA_D, T_RATIO, T_COUNT };
static_assert(T_COUNT == MADQP_BATCH_TRACE_LEN, "trace record layout is part of the ABI");

// Per-problem pattern (PAT_LEN int64 per problem, bq.pat): problem b has its own number of slacks ns_b (n_b = nx + ns_b),
// of finite lower / upper bounds, and offsets into the index lists and into the arrays of length nlb / nub.  A batch made by
// madqp_batch_create has one list of each kind that every problem points at (list offsets 0, storage offsets b * nlb);
// madqp_batch_create_patterns concatenates the problems' own lists (list offset == storage offset).
enum { P_NS = 0, P_NLB, P_NUB, P_INEQ, P_LB, P_UB, P_LBS, P_UBS, P_SLOT, PAT_LEN };

struct BQ {  // device view of the batch (by value in the kernel arguments); problem b at offset b * length
    // nst = nx + max_b ns_b: stride of the [B][n] arrays; ntst = max_b (n_b + m + nlb_b + nub_b): stride of d, p, w1, w2
    int64_t B, nx, m, nst, ntst, ldk, npad, kpad, nblk;
    int64_t dim;     // order of the factorised matrix: nx (condensed) or m (normal equations)
    int32_t normal;  // 1: the reference's NormalKKTSystem (src/KKT/normalkkt.jl), LP only
    const int64_t* pat;  // [B][PAT_LEN]
    const int64_t *ind_lb, *ind_ub, *ind_ineq, *slot;  // slot: m entries per problem at pat[P_SLOT], -1 on equality rows
    const double *H, *A, *q, *rhs, *c0;
    double *x, *xl, *xu, *zl, *zu, *y;
    double *f, *c, *jacl, *reg, *pr_diag, *du_diag, *d, *p, *w1, *w2;
    double *l_diag, *l_lower, *u_diag, *u_lower, *corr_lb, *corr_ub;
    double *theta, *t, *u, *K, *S, *winv, *tmp, *tn;
    double* sym;      // scratch of the symmetric H products (batch_wg.inc: wg_symv_lower), nullptr: full-matrix passes
    int64_t sym_len;  // doubles per problem
    // incremental model evaluation (round 5, MADQP_BATCH_INCR): H x of the current iterate and the two products the LAST
    // solve's residual check formed -- H dx and A' dy, unscaled -- per problem (nx each); nullptr: every iteration
    // evaluates H x, A x and A' y with passes of their own.  incr_ok[b]: the products belong to the step just taken.
    double *hx, *raw_h, *raw_at;
    double* at;  // A' dy of the LAST condensed solve, formed in the pass that formed A dx (batch_wg.inc: wg_gemv_n_then_t); nx each
    int32_t* incr_ok;
    double* scal;
    int32_t *status, *iters, *info, *retry_skip;
    int32_t *retry_list, *retry_count;  // the problems of the current x100-retry round, compacted (bq_retry_kernel appends)
    // per-iteration trace (madqp_batch_set_trace; nullptr: none): [B][trace_cap][T_COUNT], written by bq_iter_pre_kernel;
    // trace_count[b]: records of problem b that are stored
    double* trace;
    int32_t* trace_count;
    int64_t trace_cap;
    madqp_mpc_options opt;
    double mu_init, bound_fac;
    // madqp_batch_share_matrices: doubles from problem b's H / A to problem b + 1's (0: ONE matrix read by every problem,
    // else nx * nx / m * nx) and the per-problem factor of a shared H (nullptr: 1).  Read by the shared instantiations of the
    // workgroup programs only (prob_of<true>); the others keep the natural strides as constants of their own.
    int64_t sH, sA;
    const double* h_scale;
};

// the pattern words are uniform across the workgroup: scalar loads, read once at the top of a program
__device__ __forceinline__ madqp_state state_of(const BQ& q, int64_t b) {
    const int64_t* pt = q.pat + b * PAT_LEN;
    const int64_t nlb = pt[P_NLB], nub = pt[P_NUB], lbs = pt[P_LBS], ubs = pt[P_UBS];
    madqp_state s;
    s.n = q.nx + pt[P_NS];
    s.m = q.m;
    s.nlb = nlb;
    s.nub = nub;
    s.ind_lb = q.ind_lb + pt[P_LB];
    s.ind_ub = q.ind_ub + pt[P_UB];
    s.x = q.x + b * q.nst;
    s.xl = q.xl + b * q.nst;
    s.xu = q.xu + b * q.nst;
    s.zl = q.zl + b * q.nst;
    s.zu = q.zu + b * q.nst;
    s.f = q.f + b * q.nst;
    s.y = q.y + b * q.m;
    s.c = q.c + b * q.m;
    s.jacl = q.jacl + b * q.nst;
    s.d = q.d + b * q.ntst;
    s.p = q.p + b * q.ntst;
    s.correction_lb = q.corr_lb + lbs;
    s.correction_ub = q.corr_ub + ubs;
    s.reg = q.reg + b * q.nst;
    s.pr_diag = q.pr_diag + b * q.nst;
    s.du_diag = q.du_diag + b * q.m;
    s.l_diag = q.l_diag + lbs;
    s.l_lower = q.l_lower + lbs;
    s.u_diag = q.u_diag + ubs;
    s.u_lower = q.u_lower + ubs;
    return s;
}

// per-problem pointers that are not part of madqp_state
struct Prob {
    const double *H, *A, *qv, *rhs;
    double *theta, *t, *u, *K, *S, *winv, *tmp, *tn, *w1, *scal, *sym;
    double *hx, *raw_h, *raw_at, *at;
    double c0;
    double hs;  // shared instantiations: problem b reads fl(hs * H[i][j]) wherever it reads H (batch_wg.inc: wg_hmul)
    int64_t ns, ntot;  // slacks of this problem; length of its [x | y | zl | zu] (the used part of d, p, w1, w2)
    const int64_t *ind_ineq, *slot;
};
template <bool SHARED>
__device__ __forceinline__ Prob prob_of(const BQ& q, int64_t b) {
    const int64_t* pt = q.pat + b * PAT_LEN;
    Prob p;
    p.ns = pt[P_NS];
    p.ntot = q.nx + p.ns + q.m + pt[P_NLB] + pt[P_NUB];
    p.ind_ineq = q.ind_ineq + pt[P_INEQ];
    p.slot = q.slot + pt[P_SLOT];
    if constexpr (SHARED) {
        p.H = q.H ? q.H + b * q.sH : nullptr;
        p.A = q.A + b * q.sA;
        p.hs = q.h_scale ? q.h_scale[b] : 1.0;
    } else {
        p.H = q.H ? q.H + b * q.nx * q.nx : nullptr;
        p.A = q.A + b * q.m * q.nx;
        p.hs = 1.0;
    }
    p.qv = q.q + b * q.nx;
    p.rhs = q.rhs + b * q.m;
    p.theta = q.theta + b * q.m;
    p.t = q.t + b * q.m;
    p.u = q.u + b * q.m;
    p.K = q.K + b * q.ldk * q.ldk;
    p.S = q.S + b * q.kpad * q.npad;
    p.winv = q.winv + b * q.nblk * WBLK;
    p.tmp = q.tmp + b * q.npad;
    p.tn = q.tn ? q.tn + b * q.nst : nullptr;
    p.sym = q.sym ? q.sym + b * q.sym_len : nullptr;
    p.hx = q.hx ? q.hx + b * q.nx : nullptr;
    p.raw_h = q.hx ? q.raw_h + b * q.nx : nullptr;
    p.raw_at = q.hx ? q.raw_at + b * q.nx : nullptr;
    p.at = q.at ? q.at + b * q.nx : nullptr;
    p.w1 = q.w1 + b * q.ntst;
    p.scal = q.scal + b * S_COUNT;
    p.c0 = q.c0[b];
    return p;
}

// The workgroup programs are compiled twice (batch_wg.inc): 256 threads per problem for large batches
// (many problems per CU, HBM bound) and 512 threads per problem for small ones (1024 would spill), where the time of a
// lock-step iteration is the serial time of ONE problem's vector work.
// -- and each width once more for batches that share H / A (madqp_batch_share_matrices; WG_SHARED 1: strides and the factor
// of H from BQ): the programs of a batch that shares nothing are compiled from the very text they always were.
#define WG_SHARED 0
#define TPB 256
#define WGNS wg256
#ifdef MADQP_BATCH_STAMPS
__device__ unsigned long long madqp_batch_stamps[32];  // [31] = last stamp; slot 0 = everything not listed
#endif
#include "batch_wg.inc"
#undef TPB
#undef WGNS
#define TPB 512
#define WGNS wg512
#include "batch_wg.inc"
#undef TPB
#undef WGNS
#undef WG_SHARED
#define WG_SHARED 1
#define TPB 256
#define WGNS wg256s
#include "batch_wg.inc"
#undef TPB
#undef WGNS
#define TPB 512
#define WGNS wg512s
#include "batch_wg.inc"
#undef TPB
#undef WGNS
#undef WG_SHARED

__global__ void bq_count_active_kernel(const int32_t* __restrict__ status, int64_t B, int32_t* out) {
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < B; i += blockDim.x) cnt += (status[i] == MPC_ST_ACTIVE);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (threadIdx.x == 0) *out = cnt;
}

// Shared H: the addend of the assembly, fl(h_scale[b] * H), into the lower triangle of problem b's K (the entries the GEMM
// reads where it writes: flat index i + j * nx of H for i >= j, as the stacked form's Cin), so that the assembly accumulates in
// place.  Same masks as the GEMM launch behind it: skip[b] != 0 leaves problem b alone; list / count: slot blockIdx.y works
// off list[y], list[y + slots], .. < *count.  grid.x: blocks of PW_COLS columns.
constexpr int PW_COLS = 16;
__global__ __launch_bounds__(256) void bq_prewrite_h_kernel(const double* __restrict__ H, const double* __restrict__ h_scale,
                                                            int64_t nx, double* __restrict__ K, int64_t ldk, int64_t B,
                                                            const int32_t* __restrict__ skip,
                                                            const int32_t* __restrict__ list,
                                                            const int32_t* __restrict__ count) {
    const int64_t j0 = (int64_t)blockIdx.x * PW_COLS;
    const int64_t j1 = (j0 + PW_COLS < nx) ? j0 + PW_COLS : nx;
    const int64_t first = list ? (int64_t)blockIdx.y : 0, last = list ? (int64_t)*count : 1, step = list ? (int64_t)gridDim.y : 1;
    for (int64_t pb = first; pb < last; pb += step) {
        const int64_t b = list ? (int64_t)list[pb] : (int64_t)blockIdx.y;
        if (b < 0 || b >= B) continue;
        if (!list && skip && skip[b] != 0) continue;
        const double hs = h_scale ? h_scale[b] : 1.0;
        double* Kb = K + b * ldk * ldk;
        for (int64_t j = j0; j < j1; ++j)
            for (int64_t i = j + threadIdx.x; i < nx; i += 256) Kb[i + j * ldk] = hs * H[i + j * nx];
    }
}
}  // namespace

struct madqp_batch {
    madqp_ctx* ctx;
    BQ q;
    DevOwner mem;  // every device buffer of the batch
    int32_t* d_active;
    // one lock-step iteration (13 launches + 2 masked retry rounds) captured once as a hipGraph and replayed on an internal stream
    hipStream_t sG = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipEvent_t evIn = nullptr, evOut = nullptr;
    int graph_state = 0;  // 0 not tried, 1 ready, -1 unavailable
    bool wide;  // 512 threads per problem (small batches)
    bool started = false;  // madqp_batch_init has run: BQ has gone into kernels (and soon into the graph) by value
    bool shared = false;    // madqp_batch_share_matrices has been called: the shared instantiations of the programs run
    bool shared_H = false;  // ... with ONE H: factor_all writes fl(h_scale[b] * H) into K before every assembly
};

namespace {
// build_kkt! + factorize! for every active problem: one assembly launch, ~2 nx/128 launches of Cholesky
// retry == true: the masked x100-retry rounds -- the launches have RETRY_SLOTS problem slots in place of B problems and
// work off the compacted list bq_retry_kernel has just written (usually empty: every workgroup leaves after one load;
// round 3 launched B problems' worth of workgroups that each read a skip word: 1.8 % of the batch's time)
constexpr int64_t RETRY_SLOTS = 8;
int32_t factor_all(madqp_batch* b, const int32_t* skip, bool retry = false) {
    madqp_ctx* ctx = b->ctx;
    const BQ& q = b->q;
    if (q.dim == 0) return hipMemsetAsync(q.info, 0, q.B * sizeof(int32_t), ctx->stream) == hipSuccess
                               ? MADQP_OK
                               : MADQP_ERR_HIP;
    GemmArgs g{};
    g.X = q.S;
    g.ldx = q.npad;
    g.Y = q.S;
    g.ldy = q.npad;
    g.K = q.kpad;
    g.Mread = g.Nread = q.npad;
    g.C = q.K;
    g.ldc = q.ldk;
    g.Cin = q.normal ? nullptr : q.H;
    g.ldcin = q.nx;
    int64_t sCin = q.nx * q.nx;
    g.dvec = q.normal ? q.theta : q.pr_diag;  // normal equations: Sigma_s^-1 on the inequality rows
    g.alpha = 1.0;
    g.beta = 1.0;
    g.M = q.dim;
    g.N = q.dim;
    g.lower_only = 1;
    if ((q.normal ? q.nx : q.m) == 0) {  // empty product: K = base + diagonal through a K = 0 product
        g.K = 0;
        g.X = g.Y = q.K;
        g.Mread = g.Nread = 0;
    }
    static const bool compact = !(getenv("MADQP_BATCH_RETRY_COMPACT") && atoi(getenv("MADQP_BATCH_RETRY_COMPACT")) == 0);
    const bool lst = retry && compact;
    if (b->shared_H && g.Cin) {
        // ONE H for the batch: K_b <- fl(h_scale[b] * H) first (the double the stacked form keeps in memory), then the assembly
        // adds to it in place as the updates of the factorisation do -- the GEMM, its sums and beta = 1 are the stacked form's.
        // Before EVERY assembly: by the x100-retry rounds K holds what the failed factorisation left.
        ProfScope ps(ctx, MADQP_PROF_SYRK);
        hipLaunchKernelGGL(bq_prewrite_h_kernel, dim3((unsigned)((q.nx + PW_COLS - 1) / PW_COLS), (unsigned)(lst ? RETRY_SLOTS : q.B)),
                           dim3(256), 0, ctx->stream, q.H, q.h_scale, q.nx, q.K, q.ldk, q.B, lst ? nullptr : skip,
                           lst ? q.retry_list : nullptr, lst ? q.retry_count : nullptr);
        LAUNCH_CHECK(ctx);
        g.Cin = q.K;
        g.ldcin = q.ldk;
        sCin = q.ldk * q.ldk;
    }
    GemmBatch bt{lst ? RETRY_SLOTS : q.B, q.kpad * q.npad, q.kpad * q.npad, q.ldk * q.ldk, sCin, q.normal ? q.m : q.nst,
                 lst ? nullptr : skip, lst ? q.retry_list : nullptr, lst ? q.retry_count : nullptr};
    int32_t r = madqp_gemm_tn(ctx, g, MADQP_PROF_SYRK, nullptr, 0, &bt);
    if (r) return r;
    return madqp_chol_factor_batched(ctx, q.K, q.ldk, q.dim, q.ldk * q.ldk, q.winv, q.nblk * WBLK, q.info, q.B, skip,
                                     RETRY_SLOTS, lst ? q.retry_list : nullptr, lst ? q.retry_count : nullptr);
}
}  // namespace

extern "C" int32_t madqp_batch_destroy(madqp_batch* b) {
    if (!b) return MADQP_OK;
    (void)hipStreamSynchronize(b->ctx->stream);
    if (b->sG) (void)hipStreamSynchronize(b->sG);
    if (b->exec) (void)hipGraphExecDestroy(b->exec);
    if (b->graph) (void)hipGraphDestroy(b->graph);
    if (b->evIn) (void)hipEventDestroy(b->evIn);
    if (b->evOut) (void)hipEventDestroy(b->evOut);
    if (b->sG) (void)hipStreamDestroy(b->sG);
    delete b;  // (its owner frees the buffers)
    return MADQP_OK;
}

namespace {
// What the two creation entry points hand to create_batch: the per-problem pattern table, the slack lists and slack maps
// on the host, the bound lists on the device (borrowed, or copied by the caller into arrays the batch owns).
struct PatternHost {
    std::vector<int64_t> pat;       // [B][PAT_LEN]
    std::vector<int64_t> ineq;      // every problem's ind_ineq, at pat[P_INEQ]
    std::vector<int64_t> slot;      // m entries per distinct pattern, at pat[P_SLOT]
    int64_t ns_max = 0, ntot_max = 0, nlb_total = 0, nub_total = 0;
    bool any_eq = false;  // some problem has an equality row
};

// slot map of one problem's ind_ineq (strictly increasing rows in [0, m)): row -> slack index or -1
bool append_slots(const int64_t* ineq, int64_t ns, int64_t m, std::vector<int64_t>& slot) {
    const size_t base = slot.size();
    slot.resize(base + (size_t)m);
    return kkt_slot_map(ineq, ns, m, slot.data() + base);
}

int32_t create_batch(madqp_ctx* ctx, int64_t B, int64_t nx, int64_t m, PatternHost& ph, const int64_t* ind_lb,
                     const int64_t* ind_ub, DevOwner& lists, const madqp_batch_data* data,
                     const madqp_mpc_options* opt, madqp_batch** out) {
    const int32_t normal = opt->kkt_form;
    // the condensed form needs delta_d < 0 on equality rows (conventions)
    if (!normal && ph.any_eq && !(opt->regularization != 0 && opt->delta_d < 0.0)) {
        return madqp_fail(ctx, MADQP_ERR_ARG, "bad argument: the condensed form needs delta_d < 0 on equality rows");
    }
    *out = nullptr;
    madqp_batch* b = new (std::nothrow) madqp_batch();
    if (!b) return madqp_fail(ctx, MADQP_ERR_ALLOC, "host allocation failed");
    b->ctx = b->mem.ctx = ctx;
    b->mem.take(lists);
    // measured at (512, 256): 512 threads per problem are faster up to B = 512 and equal at 1024
    static const int wide_max = getenv("MADQP_BATCH_WIDE_MAX") ? atoi(getenv("MADQP_BATCH_WIDE_MAX")) : 1024;
    b->wide = B <= wide_max;
    BQ& q = b->q;
    memset(&q, 0, sizeof(q));
    q.B = B;
    q.nx = nx;
    q.m = m;
    q.nst = nx + ph.ns_max;
    q.ntst = ph.ntot_max;
    q.normal = normal;
    q.dim = normal ? m : nx;
    q.npad = std::max<int64_t>(128, (q.dim + 127) / 128 * 128);
    q.ldk = q.npad;
    q.kpad = std::max<int64_t>(16, ((normal ? nx : m) + 15) / 16 * 16);
    q.nblk = q.npad / 128;
    q.ind_lb = ind_lb;
    q.ind_ub = ind_ub;
    q.H = data->H;
    q.A = data->A;
    q.q = data->q;
    q.rhs = data->rhs;
    q.c0 = data->c0;
    q.x = data->x;
    q.xl = data->xl;
    q.xu = data->xu;
    q.zl = data->zl;
    q.zu = data->zu;
    q.y = data->y;
    q.opt = *opt;
    q.sH = nx * nx;
    q.sA = m * nx;
    const int64_t nst = q.nst, ntst = q.ntst, nlbt = ph.nlb_total, nubt = ph.nub_total;
    int32_t r = MADQP_OK;
    int64_t *d_pat = nullptr, *d_ineq = nullptr, *d_slot = nullptr;
#define BALLOC(ptr, count, ...)                                   \
    if (r == MADQP_OK) r = b->mem.alloc(&(ptr), (count), "madqp_batch_create", ##__VA_ARGS__)
    BALLOC(d_pat, B * PAT_LEN);
    BALLOC(d_ineq, (int64_t)ph.ineq.size());
    BALLOC(d_slot, (int64_t)ph.slot.size());
    BALLOC(q.f, B * nst);
    BALLOC(q.c, B * m);
    BALLOC(q.jacl, B * nst);
    BALLOC(q.reg, B * nst);
    BALLOC(q.pr_diag, B * nst);
    BALLOC(q.du_diag, B * m);
    BALLOC(q.d, B * ntst);
    BALLOC(q.p, B * ntst);
    BALLOC(q.w1, B * ntst);
    BALLOC(q.w2, opt->max_ncorr > 0 ? B * ntst : 1);
    BALLOC(q.l_diag, nlbt);
    BALLOC(q.l_lower, nlbt);
    BALLOC(q.u_diag, nubt);
    BALLOC(q.u_lower, nubt);
    BALLOC(q.corr_lb, nlbt);
    BALLOC(q.corr_ub, nubt);
    BALLOC(q.theta, B * m);
    BALLOC(q.t, B * m);
    BALLOC(q.u, B * m);
    BALLOC(q.K, B * q.ldk * q.ldk + 128, true);
    BALLOC(q.S, B * q.kpad * q.npad);
    BALLOC(q.winv, B * q.nblk * WBLK, true);  // potf2_inv_kernel writes the lower parts only
    BALLOC(q.tmp, B * q.npad);
    if (normal) BALLOC(q.tn, B * nst);
    {  // H products from the lower triangle (MADQP_BATCH_SYMV=0: full-matrix passes)
        static const bool symv = !(getenv("MADQP_BATCH_SYMV") && atoi(getenv("MADQP_BATCH_SYMV")) == 0);
        q.sym_len = (512 / 64 + 1) * 512;  // SYM_DOUBLES of the widest workgroup program
        if (symv && data->H && nx > 0 && nx <= 512) BALLOC(q.sym, B * q.sym_len);
    }
    {   // incremental model evaluation: condensed form without Gondzio corrections (a rejected trial would leave the
        // products of a direction that was not taken)
        static const bool incr = !(getenv("MADQP_BATCH_INCR") && atoi(getenv("MADQP_BATCH_INCR")) == 0);
        if (incr && !normal && opt->max_ncorr == 0 && nx > 0) {
            BALLOC(q.hx, B * nx, true);
            BALLOC(q.raw_h, B * nx, true);
            BALLOC(q.raw_at, B * nx, true);
        }
        BALLOC(q.incr_ok, B, true);
        // A dx and A' dy of a condensed solve in ONE pass over A (the workgroup programs are HBM bound; the residual check
        // of solve_system! then has no pass of its own over A): needs a row of A in a wave's registers, nx <= 512
        static const bool nt = !(getenv("MADQP_BATCH_NT") && atoi(getenv("MADQP_BATCH_NT")) == 0);
        if (nt && !normal && nx > 0 && nx <= 512 && m > 0) BALLOC(q.at, B * nx, true);
    }
    BALLOC(q.scal, B * S_COUNT, true);
    BALLOC(q.status, B, true);
    BALLOC(q.iters, B, true);
    BALLOC(q.info, B, true);
    BALLOC(q.retry_skip, B, true);
    BALLOC(q.retry_list, B, true);
    BALLOC(q.retry_count, 4, true);
    BALLOC(b->d_active, 1, true);
#undef BALLOC
    auto up = [&](int64_t* dst, const std::vector<int64_t>& src, const char* what) {
        if (r == MADQP_OK && !src.empty() &&
            hipMemcpy(dst, src.data(), src.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess)
            r = madqp_fail(ctx, MADQP_ERR_HIP, "copy of %s failed", what);
    };
    up(d_pat, ph.pat, "the pattern table");
    up(d_ineq, ph.ineq, "ind_ineq");
    up(d_slot, ph.slot, "the slack map");
    if (r != MADQP_OK) {
        madqp_batch_destroy(b);
        return r;
    }
    q.pat = d_pat;
    q.ind_ineq = d_ineq;
    q.slot = d_slot;
    *out = b;
    return MADQP_OK;
}

int32_t check_common(madqp_ctx* ctx, int64_t B, int64_t nx, int64_t m, const madqp_batch_data* data,
                     const madqp_mpc_options* opt, madqp_batch** out) {
    ARG_TRY(ctx, out && data && opt && B >= 1 && B <= 65535 && nx >= 0 && m >= 0);
    ARG_TRY(ctx, (nx == 0 || (data->q && data->x && data->xl && data->xu && data->zl && data->zu)) &&
                     (m == 0 || (data->A && data->rhs && data->y)) && data->c0);
    ARG_TRY(ctx, opt->step_rule >= 0 && opt->step_rule <= 2 && opt->max_ncorr >= 0 && opt->regularization >= 0 &&
                     opt->regularization <= 2);
    ARG_TRY(ctx, opt->kkt_form == 0 || opt->kkt_form == 1);
    ARG_TRY(ctx, opt->refine_steps >= 0);  // (the AUTO value -1 belongs to madqp_kkt_set_refine)
    ARG_TRY(ctx, !opt->kkt_form || !data->H);  // NormalKKTSystem supports only linear programs (src/KKT/normalkkt.jl:45-48)
    return MADQP_OK;
}
}  // namespace

extern "C" int32_t madqp_batch_create(madqp_ctx* ctx, int64_t B, int64_t nx, int64_t m, int64_t ns,
                                      const int64_t* ind_ineq_host, int64_t nlb, const int64_t* ind_lb,
                                      int64_t nub, const int64_t* ind_ub, const madqp_batch_data* data,
                                      const madqp_mpc_options* opt, madqp_batch** out) {
    if (!ctx) return MADQP_ERR_ARG;
    if (int32_t r = check_common(ctx, B, nx, m, data, opt, out)) return r;
    ARG_TRY(ctx, ns >= 0 && ns <= m);
    ARG_TRY(ctx, nlb >= 0 && nub >= 0 && (nlb == 0 || ind_lb) && (nub == 0 || ind_ub) && (ns == 0 || ind_ineq_host));
    // one pattern: every problem points at the same lists and slack map, its nlb / nub arrays at b * nlb / b * nub
    PatternHost ph;
    if (!append_slots(ind_ineq_host, ns, m, ph.slot))
        return madqp_fail(ctx, MADQP_ERR_ARG, "ind_ineq must be strictly increasing row indices");
    ph.ineq.assign(ind_ineq_host, ind_ineq_host + ns);
    ph.pat.resize((size_t)(B * PAT_LEN));
    for (int64_t bb = 0; bb < B; ++bb) {
        int64_t* pt = ph.pat.data() + bb * PAT_LEN;
        pt[P_NS] = ns;
        pt[P_NLB] = nlb;
        pt[P_NUB] = nub;
        pt[P_INEQ] = pt[P_LB] = pt[P_UB] = pt[P_SLOT] = 0;
        pt[P_LBS] = bb * nlb;
        pt[P_UBS] = bb * nub;
    }
    ph.ns_max = ns;
    ph.ntot_max = nx + ns + m + nlb + nub;
    ph.nlb_total = B * nlb;
    ph.nub_total = B * nub;
    ph.any_eq = ns < m;
    DevOwner none(ctx);
    return create_batch(ctx, B, nx, m, ph, ind_lb, ind_ub, none, data, opt, out);
}

extern "C" int32_t madqp_batch_create_patterns(madqp_ctx* ctx, int64_t B, int64_t nx, int64_t m, const int64_t* ineq_ptr,
                                               const int64_t* ind_ineq_host, const int64_t* lb_ptr,
                                               const int64_t* ind_lb_host, const int64_t* ub_ptr,
                                               const int64_t* ind_ub_host, const madqp_batch_data* data,
                                               const madqp_mpc_options* opt, madqp_batch** out) {
    if (!ctx) return MADQP_ERR_ARG;
    if (int32_t r = check_common(ctx, B, nx, m, data, opt, out)) return r;
    ARG_TRY(ctx, ineq_ptr && lb_ptr && ub_ptr);
    auto csr_ok = [&](const int64_t* ptr, const int64_t* list) {
        if (ptr[0] != 0) return false;
        for (int64_t bb = 0; bb < B; ++bb)
            if (ptr[bb + 1] < ptr[bb]) return false;
        return ptr[B] == 0 || list != nullptr;
    };
    if (!csr_ok(ineq_ptr, ind_ineq_host) || !csr_ok(lb_ptr, ind_lb_host) || !csr_ok(ub_ptr, ind_ub_host))
        return madqp_fail(ctx, MADQP_ERR_ARG, "madqp_batch_create_patterns: a *_ptr array must start at 0 and not decrease"
                                              " (and a non-empty list needs its array)");
    PatternHost ph;
    ph.pat.resize((size_t)(B * PAT_LEN));
    ph.nlb_total = lb_ptr[B];
    ph.nub_total = ub_ptr[B];
    for (int64_t bb = 0; bb < B; ++bb) {
        const int64_t ns = ineq_ptr[bb + 1] - ineq_ptr[bb], nlb = lb_ptr[bb + 1] - lb_ptr[bb],
                      nub = ub_ptr[bb + 1] - ub_ptr[bb], n = nx + ns;
        if (ns > m)
            return madqp_fail(ctx, MADQP_ERR_ARG, "madqp_batch_create_patterns: problem %lld has %lld slacks > m = %lld",
                              (long long)bb, (long long)ns, (long long)m);
        if (!append_slots(ind_ineq_host + ineq_ptr[bb], ns, m, ph.slot))
            return madqp_fail(ctx, MADQP_ERR_ARG,
                              "madqp_batch_create_patterns: ind_ineq of problem %lld must be strictly increasing in [0, m)",
                              (long long)bb);
        auto inc = [&](const int64_t* l, int64_t len) {
            for (int64_t k = 0; k < len; ++k)
                if (!(l[k] >= 0 && l[k] < n && (k == 0 || l[k - 1] < l[k]))) return false;
            return true;
        };
        if (!inc(ind_lb_host + lb_ptr[bb], nlb) || !inc(ind_ub_host + ub_ptr[bb], nub))
            return madqp_fail(ctx, MADQP_ERR_ARG,
                              "madqp_batch_create_patterns: ind_lb / ind_ub of problem %lld must be strictly increasing "
                              "in [0, n_b)", (long long)bb);
        int64_t* pt = ph.pat.data() + bb * PAT_LEN;
        pt[P_NS] = ns;
        pt[P_NLB] = nlb;
        pt[P_NUB] = nub;
        pt[P_INEQ] = ineq_ptr[bb];
        pt[P_LB] = pt[P_LBS] = lb_ptr[bb];
        pt[P_UB] = pt[P_UBS] = ub_ptr[bb];
        pt[P_SLOT] = bb * m;
        ph.ns_max = std::max(ph.ns_max, ns);
        ph.ntot_max = std::max(ph.ntot_max, n + m + nlb + nub);
        ph.any_eq = ph.any_eq || ns < m;
    }
    if (ineq_ptr[B]) ph.ineq.assign(ind_ineq_host, ind_ineq_host + ineq_ptr[B]);
    // the bound lists: copied into arrays the batch owns
    DevOwner lists(ctx);  // (freed here unless create_batch takes them)
    int64_t* d_lists[2] = {nullptr, nullptr};
    const int64_t* hl[2] = {ind_lb_host, ind_ub_host};
    const int64_t len[2] = {lb_ptr[B], ub_ptr[B]};
    for (int k = 0; k < 2; ++k) {
        if (int32_t r = lists.alloc(&d_lists[k], len[k], "madqp_batch_create_patterns: bound lists")) return r;
        if (len[k]) HIP_TRY(ctx, hipMemcpy(d_lists[k], hl[k], len[k] * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return create_batch(ctx, B, nx, m, ph, d_lists[0], d_lists[1], lists, data, opt, out);
}

// one workgroup program for the whole batch: 512 or 256 threads per problem, from namespace W / N
#define WG_LAUNCH(b, W, N, ...)                                                                                   \
    do {                                                                                                          \
        if ((b)->wide)                                                                                            \
            hipLaunchKernelGGL((W::__VA_ARGS__), dim3((unsigned)(b)->q.B), dim3(512), 0, (b)->ctx->stream, (b)->q); \
        else                                                                                                      \
            hipLaunchKernelGGL((N::__VA_ARGS__), dim3((unsigned)(b)->q.B), dim3(256), 0, (b)->ctx->stream, (b)->q); \
    } while (0)

// src/solver.jl:162-179 for every problem (the caller has done :127-159: bounds, interior push, scaling)
extern "C" int32_t madqp_batch_init(madqp_batch* b, double mu_init, double bound_fac) {
    if (!b) return MADQP_ERR_ARG;
    madqp_ctx* ctx = b->ctx;
    b->started = true;
    b->q.mu_init = mu_init;
    b->q.bound_fac = bound_fac;
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (b->shared)
            WG_LAUNCH(b, wg512s, wg256s, bq_init_pre_kernel);
        else
            WG_LAUNCH(b, wg512, wg256, bq_init_pre_kernel);
        LAUNCH_CHECK(ctx);
    }
    int32_t r = factor_all(b, b->q.status);
    if (r) return r;
    ProfScope ps(ctx, MADQP_PROF_VEC);
    const bool rf = b->q.opt.refine_steps > 0;  // refinement is a template parameter, like GONDZIO below
    if (b->shared && rf)
        WG_LAUNCH(b, wg512s, wg256s, bq_init_post_kernel<true>);
    else if (b->shared)
        WG_LAUNCH(b, wg512s, wg256s, bq_init_post_kernel<false>);
    else if (rf)
        WG_LAUNCH(b, wg512, wg256, bq_init_post_kernel<true>);
    else
        WG_LAUNCH(b, wg512, wg256, bq_init_post_kernel<false>);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// one lock-step iteration on ctx->stream: loop head + operands, assembly + Cholesky, the rest
static int32_t launch_iteration(madqp_batch* b) {
    madqp_ctx* ctx = b->ctx;
    const BQ& q = b->q;
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (b->shared)
            WG_LAUNCH(b, wg512s, wg256s, bq_iter_pre_kernel);
        else
            WG_LAUNCH(b, wg512, wg256, bq_iter_pre_kernel);
        LAUNCH_CHECK(ctx);
    }
    int32_t r = factor_all(b, q.status);
    if (r) return r;
    for (int trial = 1; trial < MPC_FACTOR_TRIALS; ++trial) {  // src/linear_solver.jl:7
        HIP_TRY(ctx, hipMemsetAsync(q.retry_count, 0, sizeof(int32_t), ctx->stream));
        {
            ProfScope ps(ctx, MADQP_PROF_VEC);
            if (b->shared)
                WG_LAUNCH(b, wg512s, wg256s, bq_retry_kernel);
            else
                WG_LAUNCH(b, wg512, wg256, bq_retry_kernel);
            LAUNCH_CHECK(ctx);
        }
        if ((r = factor_all(b, q.retry_skip, true))) return r;
    }
    ProfScope ps(ctx, MADQP_PROF_VEC);
    const bool gz = q.opt.max_ncorr > 0, rf = q.opt.refine_steps > 0;
#define POST(G, R)                                                      \
    do {                                                                \
        if (b->shared)                                                  \
            WG_LAUNCH(b, wg512s, wg256s, bq_iter_post_kernel<G, R>);    \
        else                                                            \
            WG_LAUNCH(b, wg512, wg256, bq_iter_post_kernel<G, R>);      \
    } while (0)
    if (gz && rf) POST(true, true);
    else if (gz) POST(true, false);
    else if (rf) POST(false, true);
    else POST(false, false);
#undef POST
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// Captures launch_iteration into a graph (MADQP_BATCH_GRAPH=0: off).  The launches are identical from one
// iteration to the next (problems drop out through their status words, not through the grid), the tile
// tables they need exist since madqp_batch_init, and nothing in between touches the host.
static bool graph_ready(madqp_batch* b) {
    static const int enabled = getenv("MADQP_BATCH_GRAPH") ? atoi(getenv("MADQP_BATCH_GRAPH")) : 1;
    madqp_ctx* ctx = b->ctx;
    if (!enabled || ctx->prof != 0 || b->graph_state < 0) return false;  // profiling events are not capturable
    if (b->graph_state == 1) return true;
    b->graph_state = -1;
    if (hipStreamCreateWithFlags(&b->sG, hipStreamNonBlocking) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&b->evIn, hipEventDisableTiming) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&b->evOut, hipEventDisableTiming) != hipSuccess) return false;
    (void)hipStreamSynchronize(ctx->stream);
    hipStream_t saved = ctx->stream;
    ctx->stream = b->sG;
    bool ok = hipStreamBeginCapture(b->sG, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        const int32_t r = launch_iteration(b);
        const hipError_t e = hipStreamEndCapture(b->sG, &b->graph);
        ok = (r == MADQP_OK) && (e == hipSuccess) && b->graph;
    }
    ctx->stream = saved;
    if (ok) ok = hipGraphInstantiate(&b->exec, b->graph, nullptr, nullptr, 0) == hipSuccess;
    (void)hipGetLastError();  // a failed capture must not poison later launch checks
    if (getenv("MADQP_BATCH_GRAPH_VERBOSE")) fprintf(stderr, "madqp batch graph: %s\n", ok ? "captured" : "capture failed, direct launches");
    if (!ok) return false;
    b->graph_state = 1;
    return true;
}

// Up to max_steps lock-step iterations of mpc! (src/solver.jl:254-345); stops as soon as no problem
// is active (checked every `check_every` steps with one 4-byte read-back).  n_active_host: problems
// still active on return.
extern "C" int32_t madqp_batch_iterate(madqp_batch* b, int32_t max_steps, int32_t check_every,
                                       int32_t* n_active_host) {
    if (!b) return MADQP_ERR_ARG;
    madqp_ctx* ctx = b->ctx;
    ARG_TRY(ctx, max_steps >= 0 && check_every >= 1 && n_active_host);
    const BQ& q = b->q;
    const bool graph = max_steps > 0 && graph_ready(b);
    hipStream_t st = graph ? b->sG : ctx->stream;
    if (graph) {
        HIP_TRY(ctx, hipEventRecord(b->evIn, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(b->sG, b->evIn, 0));
    }
    auto count_active = [&](int32_t* active) -> int32_t {
        hipLaunchKernelGGL(bq_count_active_kernel, dim3(1), dim3(64), 0, st, q.status, q.B, b->d_active);
        LAUNCH_CHECK(ctx);
        HIP_TRY(ctx, hipMemcpyAsync(active, b->d_active, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return MADQP_OK;
    };
    int32_t active = -1, r = MADQP_OK;
    for (int32_t it = 0; it < max_steps && !r; ++it) {
        if (graph) {
            if (hipGraphLaunch(b->exec, b->sG) != hipSuccess) r = madqp_fail(ctx, MADQP_ERR_HIP, "hipGraphLaunch failed");
        } else {
            r = launch_iteration(b);
        }
        if (!r && ((it + 1) % check_every == 0 || it + 1 == max_steps)) {
            r = count_active(&active);
            if (!r && active == 0) break;
        }
    }
    if (!r && active < 0) r = count_active(&active);
    if (graph) {  // later work on the context's stream is ordered after the replays
        (void)hipEventRecord(b->evOut, b->sG);
        (void)hipStreamWaitEvent(ctx->stream, b->evOut, 0);
    }
    if (r) return r;
    *n_active_host = active;
    return MADQP_OK;
}

// status (0 active, 1 SOLVE_SUCCEEDED, 6 MAXIMUM_ITERATIONS_EXCEEDED, -3 ERROR_IN_STEP_COMPUTATION,
// -1 INTERNAL_ERROR), iteration count and the MADQP_BATCH_SCALARS scalars of every problem
extern "C" int32_t madqp_batch_results(madqp_batch* b, int32_t* status_host, int32_t* iters_host,
                                       double* scal_host) {
    if (!b) return MADQP_ERR_ARG;
    madqp_ctx* ctx = b->ctx;
    const BQ& q = b->q;
    if (status_host)
        HIP_TRY(ctx, hipMemcpyAsync(status_host, q.status, q.B * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (iters_host)
        HIP_TRY(ctx, hipMemcpyAsync(iters_host, q.iters, q.B * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (scal_host)
        HIP_TRY(ctx, hipMemcpyAsync(scal_host, q.scal, q.B * S_COUNT * sizeof(double), hipMemcpyDeviceToHost,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MADQP_OK;
}

// Per-iteration trace (include/madqp.h): the pointer goes into the kernels inside BQ, by value, and the first
// madqp_batch_iterate captures the launches into a graph -- so it has to be set before anything is launched.
extern "C" int32_t madqp_batch_set_trace(madqp_batch* b, int64_t capacity) {
    if (!b) return MADQP_ERR_ARG;
    madqp_ctx* ctx = b->ctx;
    ARG_TRY(ctx, capacity >= 1);
    if (b->started || b->q.trace)
        return madqp_fail(ctx, MADQP_ERR_STATE, "madqp_batch_set_trace: once, and before madqp_batch_init");
    BQ& q = b->q;
    double* tr = nullptr;
    int32_t* cnt = nullptr;
    const size_t before = b->mem.owned.size();
    int32_t r = b->mem.alloc(&tr, q.B * capacity * T_COUNT, "madqp_batch_set_trace", true);
    if (r == MADQP_OK) r = b->mem.alloc(&cnt, q.B, "madqp_batch_set_trace", true);
    if (r != MADQP_OK) {  // the handle stays usable, without a trace
        b->mem.release(before);
        (void)hipGetLastError();
        return r;
    }
    q.trace = tr;
    q.trace_count = cnt;
    q.trace_cap = capacity;
    return MADQP_OK;
}

// One H / one A for the whole batch (include/madqp.h).  Like the trace: strides and h_scale go into the kernels inside BQ, by
// value, and into the captured graph -- once, and before madqp_batch_init.
extern "C" int32_t madqp_batch_share_matrices(madqp_batch* b, int32_t share_H, int32_t share_A, const double* h_scale) {
    if (!b) return MADQP_ERR_ARG;
    madqp_ctx* ctx = b->ctx;
    if (b->started || b->shared)
        return madqp_fail(ctx, MADQP_ERR_STATE, "madqp_batch_share_matrices: once, and before madqp_batch_init");
    BQ& q = b->q;
    if (share_H && !q.H) return madqp_fail(ctx, MADQP_ERR_ARG, "madqp_batch_share_matrices: share_H on a batch without H");
    if (h_scale && !share_H) return madqp_fail(ctx, MADQP_ERR_ARG, "madqp_batch_share_matrices: h_scale needs share_H");
    b->shared = true;
    b->shared_H = share_H != 0;
    if (share_H) q.sH = 0;
    if (share_A) q.sA = 0;
    q.h_scale = h_scale;
    return MADQP_OK;
}

extern "C" int32_t madqp_batch_trace(madqp_batch* b, double* trace_host, int32_t* count_host) {
    if (!b) return MADQP_ERR_ARG;
    madqp_ctx* ctx = b->ctx;
    const BQ& q = b->q;
    if (!q.trace) return madqp_fail(ctx, MADQP_ERR_STATE, "madqp_batch_trace: no trace was set (madqp_batch_set_trace)");
    if (trace_host)
        HIP_TRY(ctx, hipMemcpyAsync(trace_host, q.trace, (size_t)(q.B * q.trace_cap * T_COUNT) * sizeof(double),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (count_host)
        HIP_TRY(ctx, hipMemcpyAsync(count_host, q.trace_count, q.B * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MADQP_OK;
}

// Test seams (include/madqp.h; tests/test_gpu_batched_ops.py).  Not part of the solver's interface.
// madqp_debug_batch_op: one dense helper of the workgroup programs, or the pre-write of a shared H exactly as factor_all
// launches it.  Whatever could make a helper read or write outside its operands is refused before anything is launched.
extern "C" int32_t madqp_debug_batch_op(madqp_ctx* ctx, const madqp_debug_batch_op_args* d) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, d != nullptr);
    ARG_TRY(ctx, d->op >= 0 && d->op < MADQP_DEBUG_OP_COUNT && (d->tpb == 256 || d->tpb == 512) && (d->shared == 0 || d->shared == 1));
    ARG_TRY(ctx, d->nprob >= 1 && d->nprob <= 65535 && d->rows >= 0 && d->cols >= 0);
    ARG_TRY(ctx, d->M && d->y && d->sM >= 0 && d->sx >= 0 && d->sy >= 0 && d->sraw >= 0 && d->st >= 0 && d->sat >= 0 &&
                     d->sW >= 0 && d->ssym >= 0);
    if (d->op == MADQP_DEBUG_OP_PREWRITE_H) {
        const bool lst = d->list != nullptr;
        ARG_TRY(ctx, d->rows >= 1 && d->ld >= d->rows && (!lst || (d->count && d->slots >= 1 && d->slots <= 65535)));
        ProfScope ps(ctx, MADQP_PROF_SYRK);
        hipLaunchKernelGGL(bq_prewrite_h_kernel, dim3((unsigned)((d->rows + PW_COLS - 1) / PW_COLS), (unsigned)(lst ? d->slots : d->nprob)),
                           dim3(256), 0, ctx->stream, d->M, d->h_scale, d->rows, d->y, d->ld, d->nprob, lst ? nullptr : d->skip,
                           lst ? d->list : nullptr, lst ? d->count : nullptr);
        LAUNCH_CHECK(ctx);
        return MADQP_OK;
    }
    double* tmp = nullptr;
    int64_t stmp = 0;
    // an empty matrix is a case of the engine only as rows == 0 (wg_kkt_mul at m = 0); cols == 0 would divide by zero in wg_gemv_t
    switch ((int)d->op) {
        case MADQP_DEBUG_OP_GEMV_N:
        case MADQP_DEBUG_OP_GEMV_T:
            ARG_TRY(ctx, d->x && d->cols >= 1);
            break;
        case MADQP_DEBUG_OP_GEMV_N_THEN_T:  // a row of M in a wave's registers: 8 chunks of 64 columns; tot = cols <= LDS_DOUBLES
            ARG_TRY(ctx, d->x && d->cols >= 1 && d->cols <= 512 && d->theta && d->t && d->at);
            break;
        case MADQP_DEBUG_OP_SYMV_LOWER:  // SYM_MAX; the loads are clamped to row / column n - 1
            ARG_TRY(ctx, d->x && d->rows >= 1 && d->rows <= 512 && d->sym);
            break;
        case MADQP_DEBUG_OP_CHOL_SOLVE:
            ARG_TRY(ctx, d->rows >= 1 && d->ld >= d->rows && d->winv);
            stmp = (d->rows + NB - 1) / NB * NB;
            HIP_TRY(ctx, hipMalloc(&tmp, (size_t)(d->nprob * stmp) * sizeof(double)));
            break;
        default:
            break;
    }
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        const dim3 grid((unsigned)d->nprob);
        if (d->tpb == 512 && d->shared)
            hipLaunchKernelGGL(wg512s::bq_debug_op_kernel, grid, dim3(512), 0, ctx->stream, *d, tmp, stmp);
        else if (d->tpb == 512)
            hipLaunchKernelGGL(wg512::bq_debug_op_kernel, grid, dim3(512), 0, ctx->stream, *d, tmp, stmp);
        else if (d->shared)
            hipLaunchKernelGGL(wg256s::bq_debug_op_kernel, grid, dim3(256), 0, ctx->stream, *d, tmp, stmp);
        else
            hipLaunchKernelGGL(wg256::bq_debug_op_kernel, grid, dim3(256), 0, ctx->stream, *d, tmp, stmp);
    }
    const hipError_t le = hipGetLastError();
    hipError_t se = hipSuccess;
    if (tmp) {  // the work vector is this call's own: wait, then give it back
        se = hipStreamSynchronize(ctx->stream);
        (void)hipFree(tmp);
    }
    if (le != hipSuccess) return madqp_fail(ctx, MADQP_ERR_HIP, "madqp_debug_batch_op: launch: %s", hipGetErrorString(le));
    if (se != hipSuccess) return madqp_fail(ctx, MADQP_ERR_HIP, "madqp_debug_batch_op: %s", hipGetErrorString(se));
    return MADQP_OK;
}

extern "C" int32_t madqp_debug_chol_factor_batched(madqp_ctx* ctx, double* A, int64_t lda, int64_t n, int64_t sA, double* winv,
                                                   int64_t sW, int32_t* info, int64_t B, const int32_t* skip, int64_t slots,
                                                   const int32_t* list, const int32_t* count) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, n >= 0 && sA >= 0 && sW >= 0 && B <= 65535 && slots <= 65535);
    return madqp_chol_factor_batched(ctx, A, lda, n, sA, winv, sW, info, B, skip, slots, list, count);
}

#ifdef MADQP_BATCH_STAMPS
extern "C" int32_t madqp_batch_read_stamps(unsigned long long* out32, int32_t reset) {
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(madqp_batch_stamps), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(madqp_batch_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
