// Sparse-A front end: the Jacobian arrives in CSR (the reference keeps it sparse:
// coo_to_csr, src/utils.jl:148-197; NormalKKTSystem constructor, src/KKT/normalkkt.jl:51-101) but the
// matrix that is factorised stays the DENSE condensed / normal matrix of this library, so the MFMA
// Cholesky and the triangular sweeps are unchanged.  Two pieces:
//   * y = alpha M x + beta y for a CSR matrix (products with A use the CSR of A, products with A' the
//     CSR of A' = the CSC of A, built once by the host: no atomics, fixed summation order);
//   * the weighted Gram matrix  C = base + diag(dvec) + V diag(w) V'  (lower triangle, dense, column
//     major) of the sparse rows of V -- assemble_normal_system! (src/utils.jl:266-298) with V = A,
//     w = 1/Sigma for the normal equations, and V = A', w = Theta for the condensed form.  One
//     workgroup per column of C (see sparse_gram_kernel): deterministic, no atomics.  The base may itself be
//     sparse (a symmetric H, both triangles in CSR: madqp_kkt_set_hcsr), so that nothing of size n^2 is read.
#include <algorithm>

#include "common.h"

namespace {
__global__ __launch_bounds__(256) void spmv_csr_kernel(int64_t rows, const int64_t* __restrict__ rowptr,
                                                       const int64_t* __restrict__ col,
                                                       const double* __restrict__ val, double alpha,
                                                       const double* __restrict__ x, double beta,
                                                       double* __restrict__ y) {
    // a quarter wave (16 lanes) per row: short rows dominate in LP / QP Jacobians
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    double acc = 0.0;
    if (r < rows) {
        const int64_t e = rowptr[r + 1];
        for (int64_t p = rowptr[r] + sub; p < e; p += 16) acc += val[p] * x[col[p]];
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_down(acc, off, 16);
    if (r < rows && sub == 0) y[r] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * y[r];
}

// The same product on a block of vectors, Y[:, c] = alpha M X[:, c] + beta Y[:, c]: the quarter wave of a row keeps CG
// columns' sums at once, so the row pointers, indices and values are read once per group of CG columns (blockIdx.y)
// instead of once per column.  Every (row, column) sum is spmv_csr_kernel's: the same entries per lane in the same order,
// the same multiply and add, the same shuffle reduction and the same last line -- bitwise the column loop over it.
template <int CG>
__global__ __launch_bounds__(256) void spmm_csr_kernel(int64_t rows, const int64_t* __restrict__ rowptr,
                                                       const int64_t* __restrict__ col, const double* __restrict__ val,
                                                       double alpha, const double* __restrict__ X, int64_t ldx, double beta,
                                                       double* __restrict__ Y, int64_t ldy, int64_t nrhs) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    const int64_t c0 = (int64_t)blockIdx.y * CG;
    const int nc = (int)(nrhs - c0 < CG ? nrhs - c0 : CG);
    double acc[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) acc[c] = 0.0;
    if (r < rows) {
        const int64_t e = rowptr[r + 1];
        for (int64_t p = rowptr[r] + sub; p < e; p += 16) {
            const double v = val[p];
            const double* __restrict__ x = X + col[p] + c0 * ldx;
#pragma unroll
            for (int c = 0; c < CG; ++c)
                if (c < nc) acc[c] += v * x[c * ldx];
        }
    }
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        double a = acc[c];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) a += __shfl_down(a, off, 16);
        if (c < nc && r < rows && sub == 0) {
            double* y = Y + r + (c0 + c) * ldy;
            *y = (beta == 0.0) ? alpha * a : alpha * a + beta * *y;
        }
    }
}

// Column j of the lower triangle of C = base + diag(dvec) + V diag(w) V' is owned by one workgroup:
//   C[j:n, j] <- base[j:n, j] (+ dvec[j] on the diagonal), one contiguous, coalesced run of the column-major
//   matrix; then for every stored entry (j, k) of row j of V, in ascending k, the column k of V (= row k of V',
//   entries (i, V[i,k]), i ascending) is scattered:  C[i, j] += w[k] V[j,k] V[i,k]  for i >= j.
// The entries of one column are distinct rows, so a pass has no write conflicts; the passes are separated
// by a barrier and ordered: every entry of C is a sum in a fixed order -- no atomics.  Work = nnz(V) x
// (average column length) multiply-adds plus one write of the triangle (n^2/2 x 8 B); the merge of two index
// lists per ENTRY of C, the obvious alternative, costs n^2/2 list merges and is 300 x slower at n = 90 000.
__global__ __launch_bounds__(256) void sparse_gram_kernel(int64_t n, const int64_t* __restrict__ rowptr,
                                                          const int64_t* __restrict__ col,
                                                          const double* __restrict__ val,
                                                          const int64_t* __restrict__ t_ptr,
                                                          const int64_t* __restrict__ t_col,
                                                          const double* __restrict__ t_val,
                                                          const double* __restrict__ w,
                                                          const double* __restrict__ base, int64_t ldbase,
                                                          const double* __restrict__ dvec,
                                                          const int64_t* __restrict__ b_ptr,
                                                          const int64_t* __restrict__ b_col,
                                                          const double* __restrict__ b_val,
                                                          double* __restrict__ C, int64_t ldc) {
    const int64_t j = blockIdx.x;
    double* Cj = C + j * ldc;
    if (b_ptr) {
        // sparse symmetric base (row j = column j; column indices ascending, no duplicates): zeros over the run, then the
        // stored entries with i = col >= j are ASSIGNED -- h (+ dvec[j] on the diagonal), the operations of the dense
        // base below on the same operands, so the bits are those of the dense form of the same matrix
        for (int64_t i = j + threadIdx.x; i < n; i += 256) Cj[i] = (dvec && i == j) ? dvec[j] : 0.0;
        __syncthreads();
        const int64_t e = b_ptr[j + 1];
        for (int64_t p = b_ptr[j] + threadIdx.x; p < e; p += 256) {
            const int64_t i = b_col[p];
            if (i >= j && i < n) Cj[i] = (dvec && i == j) ? b_val[p] + dvec[j] : b_val[p];
        }
    } else {
        const double* Bj = base ? base + j * ldbase : nullptr;
        for (int64_t i = j + threadIdx.x; i < n; i += 256) {
            double v = Bj ? Bj[i] : 0.0;
            if (dvec && i == j) v += dvec[j];
            Cj[i] = v;
        }
    }
    __syncthreads();
    for (int64_t p = rowptr[j]; p < rowptr[j + 1]; ++p) {
        const int64_t k = col[p];
        const double f = w[k] * val[p];
        const int64_t e = t_ptr[k + 1];
        for (int64_t q = t_ptr[k] + threadIdx.x; q < e; q += 256) {
            const int64_t i = t_col[q];
            if (i >= j) Cj[i] += f * t_val[q];
        }
        __syncthreads();
    }
}

// Band form of sparse_gram_kernel for a matrix with half-bandwidth bw whose factorisation reaches `extent` below the
// diagonal (madqp_chol_band_extent): column j is written over the rows j .. min(n-1, j+extent) only.  The base, diagonal
// and scatter passes are those above on the same operands in the same order, so inside the band every entry has the bits of
// the dense form; the rows j+bw+1 .. j+extent receive zeros -- every build, because a factorisation that ran on a NaN or
// an overflow leaves NaN there and nothing else would overwrite them.  The base is sparse or absent (no dense H in this form).  A
// pattern entry outside the band (the caller checked the pattern once; never expected) is dropped, not written out of range.
__global__ __launch_bounds__(256) void sparse_gram_band_kernel(int64_t n, const int64_t* __restrict__ rowptr,
                                                               const int64_t* __restrict__ col,
                                                               const double* __restrict__ val,
                                                               const int64_t* __restrict__ t_ptr,
                                                               const int64_t* __restrict__ t_col,
                                                               const double* __restrict__ t_val,
                                                               const double* __restrict__ w,
                                                               const double* __restrict__ dvec,
                                                               const int64_t* __restrict__ b_ptr,
                                                               const int64_t* __restrict__ b_col,
                                                               const double* __restrict__ b_val,
                                                               double* __restrict__ C, int64_t ldc, int64_t bw,
                                                               int64_t extent) {
    const int64_t j = blockIdx.x;
    double* Cj = C + j * ldc;
    const int64_t end = (j + extent < n - 1 ? j + extent : n - 1) + 1;  // one past the last row written
    const int64_t band_end = (j + bw < n - 1 ? j + bw : n - 1) + 1;     // one past the last row of the band
    // (no base: the dense form adds dvec[j] to 0.0; sparse base: it assigns dvec[j])
    for (int64_t i = j + threadIdx.x; i < end; i += 256) Cj[i] = (dvec && i == j) ? (b_ptr ? dvec[j] : 0.0 + dvec[j]) : 0.0;
    if (b_ptr) {
        __syncthreads();
        const int64_t e = b_ptr[j + 1];
        for (int64_t p = b_ptr[j] + threadIdx.x; p < e; p += 256) {
            const int64_t i = b_col[p];
            if (i >= j && i < band_end) Cj[i] = (dvec && i == j) ? b_val[p] + dvec[j] : b_val[p];
        }
    }
    __syncthreads();
    for (int64_t p = rowptr[j]; p < rowptr[j + 1]; ++p) {
        const int64_t k = col[p];
        const double f = w[k] * val[p];
        const int64_t e = t_ptr[k + 1];
        for (int64_t q = t_ptr[k] + threadIdx.x; q < e; q += 256) {
            const int64_t i = t_col[q];
            if (i >= j && i < band_end) Cj[i] += f * t_val[q];
        }
        __syncthreads();
    }
}
}  // namespace

// The host wrappers unpack the CSR views: the kernels keep their parameter lists.
int32_t madqp_sparse_gram_band(madqp_ctx* ctx, int64_t n, const Csr& v, const Csr& vt, const double* w, const double* dvec,
                               const Csr& b, double* C, int64_t ldc, int64_t bw, int64_t extent) {
    if (n == 0) return MADQP_OK;
    // (ldc >= n: dense storage; packed band storage has ldc >= extent alone -- the kernel writes the rows j .. j + extent of column j)
    ARG_TRY(ctx, v.ptr && vt.ptr && w && C && ldc >= std::max<int64_t>(extent, 1) && bw >= 0 && bw <= extent && extent < n);
    ProfScope ps(ctx, MADQP_PROF_SYRK);
    hipLaunchKernelGGL(sparse_gram_band_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, n, v.ptr, v.col, v.val, vt.ptr,
                       vt.col, vt.val, w, dvec, b.ptr, b.col, b.val, C, ldc, bw, extent);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

int32_t madqp_spmv_csr(madqp_ctx* ctx, int64_t rows, const Csr& a, double alpha, const double* x, double beta, double* y,
                       int prof_cls) {
    if (rows == 0) return MADQP_OK;
    ARG_TRY(ctx, a.ptr && x && y);
    ProfScope ps(ctx, prof_cls);
    const unsigned grid = (unsigned)((rows * 16 + 255) / 256);
    hipLaunchKernelGGL(spmv_csr_kernel, dim3(grid), dim3(256), 0, ctx->stream, rows, a.ptr, a.col, a.val, alpha, x, beta, y);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// Y[:, c] = alpha M X[:, c] + beta Y[:, c], c < nrhs (column c of X at X + c ldx, of Y at Y + c ldy): bitwise the loop over
// madqp_spmv_csr, the CSR arrays read ceil(nrhs / MADQP_SPMM_GROUP) times
int32_t madqp_spmm_csr(madqp_ctx* ctx, int64_t rows, const Csr& a, double alpha, const double* X, int64_t ldx, double beta,
                       double* Y, int64_t ldy, int64_t nrhs, int prof_cls) {
    if (rows == 0 || nrhs == 0) return MADQP_OK;
    ARG_TRY(ctx, a.ptr && X && Y && nrhs > 0);
    ProfScope ps(ctx, prof_cls);
    const unsigned gx = (unsigned)((rows * 16 + 255) / 256);
    if (nrhs <= 8)  // fewer sums to carry: the same arithmetic
        hipLaunchKernelGGL(spmm_csr_kernel<8>, dim3(gx, 1), dim3(256), 0, ctx->stream, rows, a.ptr, a.col, a.val, alpha, X, ldx,
                           beta, Y, ldy, nrhs);
    else
        hipLaunchKernelGGL(spmm_csr_kernel<MADQP_SPMM_GROUP>, dim3(gx, (unsigned)((nrhs + MADQP_SPMM_GROUP - 1) / MADQP_SPMM_GROUP)),
                           dim3(256), 0, ctx->stream, rows, a.ptr, a.col, a.val, alpha, X, ldx, beta, Y, ldy, nrhs);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

int32_t madqp_sparse_gram(madqp_ctx* ctx, int64_t n, const Csr& v, const Csr& vt, const double* w, const double* base,
                          int64_t ldbase, const double* dvec, const Csr& b, double* C, int64_t ldc) {
    if (n == 0) return MADQP_OK;
    ARG_TRY(ctx, v.ptr && vt.ptr && w && C && ldc >= n && (!base || ldbase >= n) && !(base && b.ptr));
    ProfScope ps(ctx, MADQP_PROF_SYRK);
    hipLaunchKernelGGL(sparse_gram_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, n, v.ptr, v.col, v.val, vt.ptr,
                       vt.col, vt.val, w, base, ldbase, dvec, b.ptr, b.col, b.val, C, ldc);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}
