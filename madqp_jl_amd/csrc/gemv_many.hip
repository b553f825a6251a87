// Dense product on a block of vectors:  Y[:, c] = alpha op(A) X[:, c] + beta Y[:, c],  c < nrhs  (madqp_gemv_many).
//
// The many-column forms of the products gemv.hip runs one vector at a time: A x / A' y / H x of a many-column KKT solve or
// residual streamed A once per COLUMN; here A is read once per group of MANY_TC = 128 columns.  One kernel serves both
// orientations of A: a workgroup stages a tile of A (64 outputs x 32 k) and a tile of X (up to 128 columns x 32 k) in LDS
// with loads that run along the contiguous index of each operand, and its four waves multiply them with
// v_mfma_f64_16x16x4_f64 (16 outputs x 16 columns x 4 k per instruction).  The decode -- which workgroup owns what, where
// every operand sits, which lane feeds which k -- is many_plan.inc, which tests/test_many_plan.py replays on the CPU.
// Edge tiles mask their loads (zeros enter the product) and their stores: nothing outside rows x cols of A or outside the
// stated lengths of the columns of X and Y is touched.  Several k ranges leave partial sums that a second kernel adds in
// range order: every output is one ordered chain, no atomics.
#include "common.h"
#include "many_plan.inc"

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {
constexpr int LDS_LD = (int)MANY_TK + 1;  // both staging loops write along one index of the tile: no bank conflicts

// y <- alpha s + beta y with madqp_gemv's rule: beta == 0 assigns (y is not read, a NaN there does not survive)
__device__ __forceinline__ void many_store(double* __restrict__ y, double alpha, double s, double beta) {
    *y = (beta == 0.0) ? alpha * s : alpha * s + beta * *y;
}

template <bool TRANS>
__global__ __launch_bounds__(256) void gemv_many_kernel(ManyPlan p, double alpha, const double* __restrict__ A, int64_t lda,
                                                        const double* __restrict__ X, int64_t ldx, double beta,
                                                        double* __restrict__ Y, int64_t ldy, double* __restrict__ partial) {
    __shared__ double As[MANY_TR][LDS_LD];
    __shared__ double Xs[MANY_TC][LDS_LD];
    const ManyJob j = many_job(p, blockIdx.x);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int nct = (int)((j.cols + 15) / 16);  // MFMA column tiles of this group
    double4_t acc[MANY_TC / 16];
#pragma unroll
    for (int jt = 0; jt < MANY_TC / 16; ++jt) acc[jt] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int64_t kb = j.k0; kb < j.k1; kb += MANY_TK) {
#pragma unroll
        for (int e = 0; e < MANY_A_LOADS; ++e) {
            const ManySlot s = many_a_slot(TRANS ? 1 : 0, t, e);
            const int64_t k = kb + s.k;
            As[s.r][s.k] = (s.r < j.rows && k < j.k1) ? A[many_a_index(TRANS ? 1 : 0, j.row0 + s.r, k, lda)] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < MANY_X_LOADS; ++e) {
            const ManySlot s = many_x_slot(t, e);
            const int64_t k = kb + s.k;
            if (s.r < 16 * nct) Xs[s.r][s.k] = (s.r < j.cols && k < j.k1) ? X[many_x_index(k, j.col0 + s.r, ldx)] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < MANY_TK / 4; ++s) {
            const int kk = many_lane_k(s, lane);
            const double a = As[16 * w + many_lane_rc(lane)][kk];
#pragma unroll
            for (int jt = 0; jt < MANY_TC / 16; ++jt)
                if (jt < nct)  // (the columns are the MFMA's row operand: many_acc_col)
                    acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[16 * jt + many_lane_rc(lane)][kk], a, acc[jt], 0, 0, 0);
        }
        __syncthreads();
    }
    const int64_t yl = 16 * w + many_lane_rc(lane);
    if (yl >= j.rows) return;
#pragma unroll
    for (int jt = 0; jt < MANY_TC / 16; ++jt) {
        if (jt >= nct) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t c = 16 * jt + many_acc_col(lane, g);
            if (c >= j.cols) continue;
            if (p.ksplit == 1)
                many_store(Y + many_y_index(j.row0 + yl, j.col0 + c, ldy), alpha, acc[jt][g], beta);
            else
                partial[many_partial_index(p, j.split, j.row0 + yl, j.col0 + c)] = acc[jt][g];
        }
    }
}

// the k ranges of one output, added in range order
__global__ __launch_bounds__(256) void gemv_many_reduce_kernel(ManyPlan p, double alpha, const double* __restrict__ partial,
                                                               double beta, double* __restrict__ Y, int64_t ldy) {
    const int64_t y = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (y >= p.ylen) return;
    for (int64_t c = blockIdx.y; c < p.nrhs; c += gridDim.y) {
        double tot = 0.0;
        for (int64_t s = 0; s < p.ksplit; ++s) tot += partial[many_partial_index(p, s, y, c)];
        many_store(Y + many_y_index(y, c, ldy), alpha, tot, beta);
    }
}

// no contraction at all: Y <- beta Y
__global__ __launch_bounds__(256) void gemv_many_scale_kernel(int64_t ylen, int64_t nrhs, double beta, double* __restrict__ Y,
                                                              int64_t ldy) {
    const int64_t y = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (y >= ylen) return;
    for (int64_t c = blockIdx.y; c < nrhs; c += gridDim.y) many_store(Y + many_y_index(y, c, ldy), 0.0, 0.0, beta);
}
}  // namespace

int64_t madqp_gemv_many_workspace(int32_t trans, int64_t rows, int64_t cols, int64_t nrhs) {
    return many_plan(trans, rows, cols, nrhs).partial_doubles;
}

int32_t madqp_gemv_many_impl(madqp_ctx* ctx, int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, double alpha,
                             const double* A, int64_t lda, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy,
                             double* work, int prof_cls) {
    ARG_TRY(ctx, ctx != nullptr);
    ARG_TRY(ctx, rows >= 0 && cols >= 0 && nrhs >= 0 && (trans == 0 || trans == 1));
    const int64_t ylen = trans ? cols : rows, klen = trans ? rows : cols;
    if (ylen == 0 || nrhs == 0) return MADQP_OK;
    ARG_TRY(ctx, Y != nullptr && ldy >= ylen);
    const dim3 vgrid((unsigned)((ylen + 255) / 256), (unsigned)std::min<int64_t>(nrhs, 1024));
    if (klen == 0) {
        ProfScope ps(ctx, prof_cls);
        hipLaunchKernelGGL(gemv_many_scale_kernel, vgrid, dim3(256), 0, ctx->stream, ylen, nrhs, beta, Y, ldy);
        LAUNCH_CHECK(ctx);
        return MADQP_OK;
    }
    ARG_TRY(ctx, A && X && lda >= cols && ldx >= klen);
    const ManyPlan p = many_plan(trans, rows, cols, nrhs);
    if (p.ksplit > 1 && !work) {
        if (int32_t r = madqp_work_reserve(ctx, (size_t)p.partial_doubles * sizeof(double))) return r;
        work = ctx->d_work;
    }
    ProfScope ps(ctx, prof_cls);
    const dim3 grid((unsigned)p.workgroups);
    if (trans)
        hipLaunchKernelGGL(gemv_many_kernel<true>, grid, dim3(256), 0, ctx->stream, p, alpha, A, lda, X, ldx, beta, Y, ldy, work);
    else
        hipLaunchKernelGGL(gemv_many_kernel<false>, grid, dim3(256), 0, ctx->stream, p, alpha, A, lda, X, ldx, beta, Y, ldy, work);
    LAUNCH_CHECK(ctx);
    if (p.ksplit > 1) {
        hipLaunchKernelGGL(gemv_many_reduce_kernel, vgrid, dim3(256), 0, ctx->stream, p, alpha, work, beta, Y, ldy);
        LAUNCH_CHECK(ctx);
    }
    return MADQP_OK;
}

extern "C" int32_t madqp_gemv_many(madqp_ctx* ctx, int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, double alpha,
                                   const double* A, int64_t lda, const double* X, int64_t ldx, double beta, double* Y,
                                   int64_t ldy) {
    if (!ctx) return MADQP_ERR_ARG;
    return madqp_gemv_many_impl(ctx, trans, rows, cols, nrhs, alpha, A, lda, X, ldx, beta, Y, ldy, nullptr, MADQP_PROF_GEMV);
}
