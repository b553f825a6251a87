// HIPCondensedKKTSystem: dense condensed KKT  K = H + Sigma_x + A' Theta A  (SURVEY.md 8a-note).
//
// The MI355X counterpart of NormalKKTSystem (src/KKT/normalkkt.jl): same plugin methods
// (build_kkt!, solve!, mul!, jtprod!), same sign conventions, but the slack block is eliminated
// so that the system stays n_x x n_x and positive definite for a QP with dense Hessian:
//   inequality row i with slack k:  Theta_i = S_k / (1 - dc_i S_k),  S_k = pr_diag[nx + k]
//   equality   row i             :  Theta_i = -1 / dc_i              (requires dc_i < 0)
//   rhs_x = r1_x + A' Theta (r2 + r1_s / S),   K dx = rhs_x,
//   dy = Theta (A dx - r2 - r1_s / S),          ds = (r1_s + dy) / S
//
// The same object also provides the reference's own formulation (mode NORMAL): the normal
// equations  S = A_full Sigma^-1 A_full' = A Sigma_x^-1 A' + diag(Sigma_s^-1)  (m x m) of
// src/KKT/normalkkt.jl:166-205, LP only as there (:45-48), dual regularization not added to the
// matrix.  It needs A' with row k (a variable) contiguous, which is again the
// k-major layout the GEMM core consumes; equality rows need no regularization in this form.
//
// Mode AUGMENTED is the K2 form of MadNLP's default SparseKKTSystem (src/utils.jl:108) with only the slack block
// eliminated:  [H + Sigma_x, A'; A, -D],  D_i = 1/S_k - dc_i (inequality row) or -dc_i (equality row), order
// nx + m.  It is quasi-definite, so L diag(I, -I) L' without pivoting is stable (madqp_chol_set_signature), and
// equality rows need no dual regularization when A_eq has full row rank:
//   [H + Sigma_x, A'; A, -D] [dx; dy] = [r1_x; r2 + r1_s / S],   ds = (r1_s + dy) / S
//
// Mode AUGMENTED with `scaled` set is K2.5, MadNLP's ScaledSparseKKTSystem as MadIPM drives it (src/kernels.jl:149-165;
// test/runtests.jl:95-115): l_diag = x - xl > 0, u_diag = xu - x > 0 (signs flipped against K2), a_j = l_diag or 1,
// b_j = u_diag or 1,  scaling_j = sqrt(a_j b_j),  pr_diag_j = zl_j b_j + zu_j a_j + dw a_j b_j = scaling^2 (dw + Sigma).
// The matrix is the symmetric scaling of K2 entry by entry as scripts/cuda_wrapper.jl:90-116 does it for the COO
// values -- pr_diag as it stands, Hessian entries times scaling_i scaling_j, Jacobian entries times scaling_j, du_diag
// as it stands -- with the slack block eliminated as in the unscaled case (1/S_k becomes scaling_k^2 / pr_diag_k):
// every entry stays bounded as the iterates converge.
#include "grid_kernels.h"
#include "kkt_form.inc"  // KKT_CONDENSED / KKT_NORMAL / KKT_AUGMENTED, the slot map, the orders, the bandwidth of a pattern

struct madqp_kkt {
    madqp_ctx* ctx = nullptr;
    int mode = KKT_CONDENSED;
    int64_t nx = 0, m = 0, ns = 0;
    const double* H = nullptr;
    int64_t ldh = 0;
    const double* A = nullptr;  // m x nx, row k = constraint k contiguous (condensed mode)
    int64_t lda = 0;
    const double* At = nullptr;  // nx x m, row k = variable k contiguous (normal mode)
    int64_t ldat = 0;
    Csr a, at;  // sparse front end (either mode): CSR of A (m rows) and CSR of A' (nx rows); A == At == nullptr then
    const double* hdiag = nullptr;  // diagonal Hessian (nx), instead of the dense H; borrowed
    // sparse Hessian instead of the dense H (sparse front end, condensed or augmented): the full symmetric pattern in
    // CSR, nx rows, column indices ascending within a row; borrowed (madqp_kkt_set_hcsr)
    Csr h;
    DevOwner mem;          // every device buffer below
    double* sg = nullptr;  // Sigma + [hdiag; 0] (n); the solves divide by it
    double *dn = nullptr, *tn = nullptr;  // normal mode: 1/Sigma (n) and an n-vector of scratch
    int64_t* d_ind_ineq = nullptr;        // ns
    int64_t* d_slot = nullptr;            // m: slack slot of a row, -1 for an equality row
    double* K = nullptr;
    int64_t ldk = 0;
    double *theta = nullptr, *t = nullptr, *u = nullptr;  // m
    const double* u_is_A_of = nullptr;  // condensed mode: u = A x for the primal part of this vector (the last solve's), or nullptr
    int64_t np = 0;         // augmented mode: nx rounded up to a multiple of 128 = row of the first constraint
    double* b = nullptr;    // augmented mode: right-hand side of order np + m
    int scaled = 0;         // augmented mode: K2.5 (see the header comment)
    double *sfac = nullptr, *sb = nullptr;  // K2.5: scaling factor (n) and a scratch n-vector
    madqp_chol* chol = nullptr;
    // refinement steps madqp_kkt_solve runs itself (madqp_kkt_set_refine; 0 = none, the default) and their two work vectors,
    // one grow-only buffer
    int32_t refine = 0;
    double* rf = nullptr;
    int64_t rf_cap = 0;
    // madqp_kkt_solve_many: the work vectors t, u, tn, b of its columns, one grow-only buffer (kkt_many_work)
    double* many = nullptr;
    int64_t many_cap = 0;
    // products on a block of vectors (apply_A_many / apply_At_many / apply_H_many): the partial sums of the dense kernel's k
    // ranges (mw) and the A V block of madqp_kkt_mul_many (mu), grow-only; block: madqp_kkt_set_block_products
    double *mw = nullptr, *mu = nullptr;
    int64_t mw_cap = 0, mu_cap = 0;
    bool block = false;
    // fused per-variable passes of the condensed mode (solve_pre_kernel / solve_post_kernel / resid_tail_kernel below):
    // where each variable sits in the two bound lists (-1: not there), built when the lists are first seen (grow-only
    // buffers, allocated with rs at the first fused pass), and the reduced right-hand side of the slacks kept between the
    // two passes around the sweeps
    int32_t *pos_lb = nullptr, *pos_ub = nullptr;
    int64_t pos_lb_cap = 0, pos_ub_cap = 0;
    bool pos_ok = false;  // the maps are those of the keys below
    const int64_t *pos_key_lb = nullptr, *pos_key_ub = nullptr;
    int64_t pos_nlb = 0, pos_nub = 0, pos_n = 0;
    double* rs = nullptr;  // ns
    bool fuse = true;      // MADQP_KKT_FUSE != 0
    // band-limited assembly and factorisation (madqp_kkt_set_bandwidth): half-bandwidth of K (-1: none) and the rows below
    // the diagonal the factorisation reaches (madqp_chol_band_extent), which every build rewrites
    int64_t bw = -1, band_extent = 0;
    // packed band storage (madqp_kkt_create_sparse_packed): no K until madqp_kkt_set_bandwidth allocates the band alone --
    // entry (i, j) at K[i + j ldk], ldk >= band_extent (band_plan.inc); k_doubles: what K holds, either form
    bool packed = false;
    int64_t k_doubles = 0;
};

namespace {
#include "kkt_kernels.inc"

// ---- fused per-variable passes of the condensed mode ---------------------------------------------------------------------
// An iteration at n_x = 5 000 spent ~0.5 ms in ~100 launches of 2 us kernels that follow each other at the 4.7 us interval of
// dependent dispatches.  Three runs of them -- in front of the sweeps, behind them, and the tail of the residual
// p - K d -- touch each entry independently EXCEPT for the scatters of the bound lists into the variables
// (reduce_rhs!, _kktmul!), which is why they were separate launches in list order.  With the inverse of the lists
// (pos_lb / pos_ub: the place of a variable in each list) every variable gathers its two terms itself, in the order
// the scatters applied them -- the same operations on the same operands, so the results are bitwise those of the
// separate kernels (tests/test_gpu_solver.py compares the two forms; MADQP_KKT_FUSE=0 selects the separate ones).
__global__ __launch_bounds__(TPB) void pos_fill_kernel(int64_t n, int32_t* __restrict__ a, int32_t* __restrict__ b) {
    GRID_STRIDE(i, n) a[i] = b[i] = -1;
}
__global__ __launch_bounds__(TPB) void pos_scatter_kernel(int64_t cnt, const int64_t* __restrict__ ind, int32_t* __restrict__ pos) {
    GRID_STRIDE(i, cnt) pos[ind[i]] = (int32_t)i;
}
// reduce_rhs! for one variable (src/kernels.jl:150-161 order: lower list, then upper list)
__device__ __forceinline__ double reduced_rhs(const madqp_state& s, const double* __restrict__ p, int64_t j,
                                              const int32_t* __restrict__ pos_lb, const int32_t* __restrict__ pos_ub) {
    double v = p[j];
    const int32_t pl = pos_lb[j], pu = pos_ub[j];
    if (pl >= 0) v -= p[s.n + s.m + pl] / s.l_diag[pl];
    if (pu >= 0) v -= p[s.n + s.m + s.nlb + pu] / s.u_diag[pu];
    return v;
}
// w <- p with reduce_rhs! applied, t / u of condense_kernel, rs <- the reduced right-hand side of the slacks
__global__ __launch_bounds__(TPB) void solve_pre_kernel(madqp_state s, const double* __restrict__ p, double* __restrict__ w,
                                                        const int32_t* __restrict__ pos_lb, const int32_t* __restrict__ pos_ub,
                                                        int64_t nx, const int64_t* __restrict__ slot,
                                                        const double* __restrict__ theta, double* __restrict__ t,
                                                        double* __restrict__ u, double* __restrict__ rs) {
    int64_t L = s.n > s.m ? s.n : s.m;
    if (s.nlb > L) L = s.nlb;
    if (s.nub > L) L = s.nub;
    GRID_STRIDE(i, L) {
        if (i < s.n) {
            const double v = reduced_rhs(s, p, i, pos_lb, pos_ub);
            w[i] = v;
            if (i >= nx) rs[i - nx] = v;
        }
        if (i < s.m) {
            const int64_t k = slot[i];
            double ti = p[s.n + i];
            if (k >= 0) ti += reduced_rhs(s, p, nx + k, pos_lb, pos_ub) / s.pr_diag[nx + k];
            t[i] = ti;
            u[i] = theta[i] * ti;
            w[s.n + i] = p[s.n + i];
        }
        if (i < s.nlb) w[s.n + s.m + i] = p[s.n + s.m + i];
        if (i < s.nub) w[s.n + s.m + s.nlb + i] = p[s.n + s.m + s.nlb + i];
    }
}
// decondense_kernel + finish_aug_solve_kernel (u holds A dx, w[0 .. nx) the solved dx), optionally pcopy <- p
__global__ __launch_bounds__(TPB) void solve_post_kernel(madqp_state s, double* __restrict__ w, int64_t nx,
                                                         const int64_t* __restrict__ slot, const int64_t* __restrict__ ind_ineq,
                                                         const double* __restrict__ theta, const double* __restrict__ t,
                                                         const double* __restrict__ u, const double* __restrict__ rs,
                                                         const double* __restrict__ p, double* __restrict__ pcopy) {
    int64_t L = s.n > s.m ? s.n : s.m;
    if (s.nlb > L) L = s.nlb;
    if (s.nub > L) L = s.nub;
    double* wzl = w + s.n + s.m;
    double* wzu = wzl + s.nlb;
    auto dx_of = [&](int64_t j) {  // the entry of dx the separate kernels would read at j
        if (j < nx) return w[j];
        const int64_t k = j - nx, r = ind_ineq[k];
        const double dy = theta[r] * (u[r] - t[r]);
        return (rs[k] + dy) / s.pr_diag[nx + k];
    };
    GRID_STRIDE(i, L) {
        if (i < s.m) {
            const int64_t k = slot[i];
            const double dy = theta[i] * (u[i] - t[i]);
            w[s.n + i] = dy;
            if (k >= 0) w[nx + k] = (rs[k] + dy) / s.pr_diag[nx + k];
        }
        if (i < s.nlb) wzl[i] = (-wzl[i] + s.l_lower[i] * dx_of(s.ind_lb[i])) / s.l_diag[i];
        if (i < s.nub) wzu[i] = (wzu[i] - s.u_lower[i] * dx_of(s.ind_ub[i])) / s.u_diag[i];
        if (pcopy) {
            if (i < s.n) pcopy[i] = p[i];
            if (i < s.m) pcopy[s.n + i] = p[s.n + i];
            if (i < s.nlb) pcopy[s.n + s.m + i] = p[s.n + s.m + i];
            if (i < s.nub) pcopy[s.n + s.m + s.nlb + i] = p[s.n + s.m + s.nlb + i];
        }
    }
}
// the tail of w = alpha K v + beta w behind the matrix products: jt_slack_kernel, mul_rows_kernel and the three passes of
// _kktmul! (vec_kernels.inc) in one
__global__ __launch_bounds__(TPB) void resid_tail_kernel(madqp_state s, double* __restrict__ w, const double* __restrict__ v,
                                                         double alpha, double beta, int64_t nx,
                                                         const int64_t* __restrict__ slot, const int64_t* __restrict__ ind_ineq,
                                                         const double* __restrict__ u, const int32_t* __restrict__ pos_lb,
                                                         const int32_t* __restrict__ pos_ub) {
    int64_t L = s.n > s.m ? s.n : s.m;
    if (s.nlb > L) L = s.nlb;
    if (s.nub > L) L = s.nub;
    double* wzl = w + s.n + s.m;
    double* wzu = wzl + s.nlb;
    const double* vzl = v + s.n + s.m;
    const double* vzu = vzl + s.nlb;
    GRID_STRIDE(i, L) {
        if (i < s.n) {
            double wi = w[i];
            if (i >= nx) {  // jt_slack_kernel
                const double val = alpha * (-v[s.n + ind_ineq[i - nx]]);
                wi = (beta == 0.0) ? val : val + beta * wi;
            }
            wi += alpha * s.reg[i] * v[i];  // kktmul_diag_kernel
            const int32_t pl = pos_lb[i], pu = pos_ub[i];
            if (pl >= 0) wi -= alpha * vzl[pl];  // kktmul_lb_kernel
            if (pu >= 0) wi += alpha * vzu[pu];  // kktmul_ub_kernel
            w[i] = wi;
        }
        if (i < s.m) {
            const int64_t k = slot[i];
            double a = u[i];  // mul_rows_kernel
            if (k >= 0) a -= v[nx + k];
            double wy = (beta == 0.0) ? alpha * a : alpha * a + beta * w[s.n + i];
            wy += alpha * s.du_diag[i] * v[s.n + i];
            w[s.n + i] = wy;
        }
        if (i < s.nlb) {
            const int64_t j = s.ind_lb[i];
            wzl[i] = beta * wzl[i] + alpha * (v[j] * s.l_lower[i] - vzl[i] * s.l_diag[i]);
        }
        if (i < s.nub) {
            const int64_t j = s.ind_ub[i];
            wzu[i] = beta * wzu[i] + alpha * (v[j] * s.u_lower[i] + vzu[i] * s.u_diag[i]);
        }
    }
}

// Lower triangle of the augmented matrix, one 64 x 64 tile per workgroup (blockIdx.x = tile row, .y = tile column):
//   rows/cols [0, nx): H + diag(dx);  [nx, np): identity (padding up to a block boundary);
//   rows np + r, cols [0, nx): A[r, :] (A is row-major: transposed through LDS);  rows/cols np + r: diag(dd).
__global__ __launch_bounds__(256) void aug_fill_kernel(int64_t nx, int64_t np, int64_t m, const double* __restrict__ H,
                                                       int64_t ldh, const double* __restrict__ hdiag,
                                                       const double* __restrict__ dx, const double* __restrict__ A,
                                                       int64_t lda, const double* __restrict__ dd,
                                                       const double* __restrict__ sf,  // K2.5 scaling or nullptr
                                                       double* __restrict__ K, int64_t ldk) {
    const int64_t ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int64_t i0 = ti * 64, j0 = tj * 64, N = np + m;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    __shared__ double tile[64][65];
    if (i0 >= np && j0 < np && !A) {  // sparse Jacobian: zero here, aug_scatter_kernel adds the entries
        const int64_t i = i0 + tx;
        if (i < N)
            for (int c = ty; c < 64; c += 4) K[i + (j0 + c) * ldk] = 0.0;
        return;
    }
    if (i0 >= np && j0 < np) {  // constraint rows x variable columns
        const int64_t r0 = i0 - np;
        for (int rr = ty; rr < 64; rr += 4) {
            const int64_t r = r0 + rr, j = j0 + tx;
            tile[rr][tx] = (r < m && j < nx) ? (sf ? A[r * lda + j] * sf[j] : A[r * lda + j]) : 0.0;
        }
        __syncthreads();
        const int64_t i = i0 + tx;
        if (i < N)
            for (int c = ty; c < 64; c += 4) K[i + (j0 + c) * ldk] = tile[tx][c];
        return;
    }
    const int64_t i = i0 + tx;
    if (i >= N) return;
    for (int c = ty; c < 64; c += 4) {
        const int64_t j = j0 + c;
        if (j > i) continue;
        double v = 0.0;
        if (i < nx) {
            if (H) v = sf ? H[i + j * ldh] * sf[i] * sf[j] : H[i + j * ldh];
            if (i == j) v += dx[i] + (hdiag ? (sf ? hdiag[i] * sf[i] * sf[i] : hdiag[i]) : 0.0);
        } else if (i == j) {
            v = (i < np) ? 1.0 : dd[i - np];
        }
        K[i + j * ldk] = v;
    }
}

// sparse Jacobian (CSR of A): K[np + r, col] = val, 16 lanes per row
__global__ __launch_bounds__(256) void aug_scatter_kernel(int64_t m, int64_t np, const int64_t* __restrict__ ptr,
                                                          const int64_t* __restrict__ col,
                                                          const double* __restrict__ val,
                                                          const double* __restrict__ sf, double* __restrict__ K,
                                                          int64_t ldk) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (r >= m) return;
    for (int64_t e = ptr[r] + (threadIdx.x & 15); e < ptr[r + 1]; e += 16)
        K[(np + r) + col[e] * ldk] = sf ? val[e] * sf[col[e]] : val[e];
}

// sparse Hessian (full symmetric pattern in CSR) behind aug_fill_kernel run with H == nullptr, which has left dx on the
// diagonal and zeros below it: K[i, j] = h for the stored entries with i > j, K[i, i] = h + dx[i] -- the values the
// dense-H fill writes.  16 lanes per row; only rows and columns < nx are touched.
__global__ __launch_bounds__(256) void aug_scatter_h_kernel(int64_t nx, const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ col,
                                                            const double* __restrict__ val,
                                                            const double* __restrict__ dx, double* __restrict__ K,
                                                            int64_t ldk) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (i >= nx) return;
    for (int64_t e = ptr[i] + (threadIdx.x & 15); e < ptr[i + 1]; e += 16) {
        const int64_t j = col[e];
        if (j >= 0 && j <= i) K[i + j * ldk] = (j == i) ? val[e] + dx[i] : val[e];
    }
}

// ---- K2.5 (scaled augmented system): set_aug_diagonal_reg!(::ScaledSparseKKTSystem) (src/kernels.jl:149-165) with
// MadNLP._set_aug_diagonal! folded in, and the sign-flipped reduce_rhs! / finish_aug_solve! / _kktmul! rows
__global__ __launch_bounds__(TPB) void k25_fill_kernel(madqp_state s, double del_w, double del_c, double* a, double* b) {
    const int64_t L = s.n > s.m ? s.n : s.m;
    GRID_STRIDE(i, L) {
        if (i < s.n) {
            s.reg[i] = del_w;
            a[i] = 1.0;
            b[i] = 1.0;
        }
        if (i < s.m) s.du_diag[i] = del_c;
    }
}
__global__ __launch_bounds__(TPB) void k25_bounds_kernel(madqp_state s, double* a, double* b) {
    const int64_t L = s.nlb > s.nub ? s.nlb : s.nub;
    GRID_STRIDE(i, L) {
        if (i < s.nlb) {
            const int64_t j = s.ind_lb[i];
            const double ld = s.x[j] - s.xl[j];  // (X - Xl), src/kernels.jl:157
            s.l_diag[i] = ld;
            s.l_lower[i] = s.zl[j];
            a[j] = ld;
        }
        if (i < s.nub) {
            const int64_t j = s.ind_ub[i];
            const double ud = s.xu[j] - s.x[j];  // (Xu - X), :158
            s.u_diag[i] = ud;
            s.u_lower[i] = s.zu[j];
            b[j] = ud;
        }
    }
}
__global__ __launch_bounds__(TPB) void k25_final_kernel(madqp_state s, double del_w, double* a, const double* b) {
    GRID_STRIDE(j, s.n) {
        const double aj = a[j], bj = b[j];
        s.pr_diag[j] = s.zl[j] * bj + s.zu[j] * aj + del_w * (aj * bj);
        a[j] = sqrt(aj * bj);  // a becomes the scaling factor
    }
}
__global__ __launch_bounds__(TPB) void k25_reduce_kernel(madqp_state s, double* w) {
    const double* wzl = w + s.n + s.m;
    const double* wzu = wzl + s.nlb;
    // the two lists may name the same variable: two passes in one launch would race, so lb here, ub below
    GRID_STRIDE(i, s.nlb) w[s.ind_lb[i]] += wzl[i] / s.l_diag[i];
    (void)wzu;
}
__global__ __launch_bounds__(TPB) void k25_reduce_ub_kernel(madqp_state s, double* w) {
    const double* wzu = w + s.n + s.m + s.nlb;
    GRID_STRIDE(i, s.nub) w[s.ind_ub[i]] += wzu[i] / s.u_diag[i];
}
__global__ __launch_bounds__(TPB) void k25_finish_kernel(madqp_state s, double* w) {
    const double* wx = w;
    double* wzl = w + s.n + s.m;
    double* wzu = wzl + s.nlb;
    const int64_t L = s.nlb > s.nub ? s.nlb : s.nub;
    GRID_STRIDE(i, L) {
        if (i < s.nlb) wzl[i] = (wzl[i] - s.l_lower[i] * wx[s.ind_lb[i]]) / s.l_diag[i];
        if (i < s.nub) wzu[i] = (s.u_lower[i] * wx[s.ind_ub[i]] - wzu[i]) / s.u_diag[i];
    }
}
__global__ __launch_bounds__(TPB) void k25_kktmul_diag_kernel(madqp_state s, double* w, const double* v, double alpha) {
    const int64_t L = s.n > s.m ? s.n : s.m;
    GRID_STRIDE(i, L) {
        if (i < s.n) w[i] += alpha * s.reg[i] * v[i];
        if (i < s.m) w[s.n + i] += alpha * s.du_diag[i] * v[s.n + i];
    }
}
__global__ __launch_bounds__(TPB) void k25_kktmul_lb_kernel(madqp_state s, double* w, const double* v, double alpha,
                                                            double beta) {
    double* wzl = w + s.n + s.m;
    const double* vzl = v + s.n + s.m;
    GRID_STRIDE(i, s.nlb) {
        const int64_t j = s.ind_lb[i];
        w[j] -= alpha * vzl[i];
        wzl[i] = beta * wzl[i] + alpha * (v[j] * s.l_lower[i] + vzl[i] * s.l_diag[i]);
    }
}
__global__ __launch_bounds__(TPB) void k25_kktmul_ub_kernel(madqp_state s, double* w, const double* v, double alpha,
                                                            double beta) {
    double* wzu = w + s.n + s.m + s.nlb;
    const double* vzu = v + s.n + s.m + s.nlb;
    GRID_STRIDE(i, s.nub) {
        const int64_t j = s.ind_ub[i];
        w[j] += alpha * vzu[i];
        wzu[i] = beta * wzu[i] + alpha * (v[j] * s.u_lower[i] - vzu[i] * s.u_diag[i]);
    }
}
__global__ __launch_bounds__(TPB) void k25_ones_kernel(int64_t n, double* a) {
    GRID_STRIDE(i, n) a[i] = 1.0;
}
}  // namespace

// y(m) = alpha A x(nx) + beta y   /   y(nx) = alpha A' x(m) + beta y, from whichever layout is held
static int32_t apply_A(madqp_kkt* k, double alpha, const double* x, double beta, double* y) {
    if (k->a.ptr) return madqp_spmv_csr(k->ctx, k->m, k->a, alpha, x, beta, y, MADQP_PROF_GEMV);
    if (k->A) return madqp_gemv_impl(k->ctx, 0, k->m, k->nx, alpha, k->A, k->lda, x, beta, y, MADQP_PROF_GEMV);
    return madqp_gemv_impl(k->ctx, 1, k->nx, k->m, alpha, k->At, k->ldat, x, beta, y, MADQP_PROF_GEMV);
}
static int32_t apply_At(madqp_kkt* k, double alpha, const double* x, double beta, double* y) {
    if (k->a.ptr) return madqp_spmv_csr(k->ctx, k->nx, k->at, alpha, x, beta, y, MADQP_PROF_GEMV);
    if (k->A) return madqp_gemv_impl(k->ctx, 1, k->m, k->nx, alpha, k->A, k->lda, x, beta, y, MADQP_PROF_GEMV);
    return madqp_gemv_impl(k->ctx, 0, k->nx, k->m, alpha, k->At, k->ldat, x, beta, y, MADQP_PROF_GEMV);
}
// y(nx) = alpha H x(nx) + beta y for the Hessian the object holds (at most one kind), beta 0 or 1; nothing without one
static bool kkt_has_H(const madqp_kkt* k) { return (k->H || k->hdiag || k->h.ptr) && k->nx; }
static int32_t apply_H(madqp_kkt* k, double alpha, const double* x, double beta, double* y) {
    madqp_ctx* ctx = k->ctx;
    if (!kkt_has_H(k)) return MADQP_OK;
    ARG_TRY(ctx, beta == 0.0 || beta == 1.0);
    if (k->H)  // H is symmetric: its lower triangle is enough (gemv.hip: madqp_symv_lower)
        return madqp_symv_lower(ctx, k->nx, alpha, k->H, k->ldh, x, beta, y, MADQP_PROF_GEMV);
    if (k->h.ptr)  // both triangles are stored: one row-wise mat-vec, fixed order
        return madqp_spmv_csr(ctx, k->nx, k->h, alpha, x, beta, y, MADQP_PROF_GEMV);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    LAUNCH(hdiag_mul_kernel, k->nx, k->nx, alpha, k->hdiag, x, beta, y);
    return MADQP_OK;
}

// The three operators on a block of nrhs vectors (column c of X at X + c ldx, of Y at Y + c ldy), dispatched as above.  The
// CSR forms are bitwise the column loop over the one-vector operator (madqp_spmm_csr), and so is the diagonal H; the dense
// forms read the matrix once per MADQP_GEMV_MANY_GROUP columns (madqp_gemv_many_impl; the dense H is full symmetric storage
// and goes through the same kernel).  The partial sums of the dense kernel live in k->mem and grow at the first call that
// needs more.
static int32_t dense_many(madqp_kkt* k, int32_t trans, int64_t rows, int64_t cols, int64_t nrhs, double alpha, const double* A,
                          int64_t lda, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy) {
    const int64_t need = madqp_gemv_many_workspace(trans, rows, cols, nrhs);
    if (need)
        if (int32_t r = k->mem.grow(&k->mw, &k->mw_cap, need, "block products: partial sums")) return r;
    return madqp_gemv_many_impl(k->ctx, trans, rows, cols, nrhs, alpha, A, lda, X, ldx, beta, Y, ldy, k->mw, MADQP_PROF_GEMV);
}
static int32_t apply_A_many(madqp_kkt* k, double alpha, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy,
                            int64_t nrhs) {
    if (k->a.ptr) return madqp_spmm_csr(k->ctx, k->m, k->a, alpha, X, ldx, beta, Y, ldy, nrhs, MADQP_PROF_GEMV);
    if (k->A) return dense_many(k, 0, k->m, k->nx, nrhs, alpha, k->A, k->lda, X, ldx, beta, Y, ldy);
    return dense_many(k, 1, k->nx, k->m, nrhs, alpha, k->At, k->ldat, X, ldx, beta, Y, ldy);
}
static int32_t apply_At_many(madqp_kkt* k, double alpha, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy,
                             int64_t nrhs) {
    if (k->a.ptr) return madqp_spmm_csr(k->ctx, k->nx, k->at, alpha, X, ldx, beta, Y, ldy, nrhs, MADQP_PROF_GEMV);
    if (k->A) return dense_many(k, 1, k->m, k->nx, nrhs, alpha, k->A, k->lda, X, ldx, beta, Y, ldy);
    return dense_many(k, 0, k->nx, k->m, nrhs, alpha, k->At, k->ldat, X, ldx, beta, Y, ldy);
}
static int32_t apply_H_many(madqp_kkt* k, double alpha, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy,
                            int64_t nrhs) {
    madqp_ctx* ctx = k->ctx;
    if (!kkt_has_H(k)) return MADQP_OK;
    ARG_TRY(ctx, beta == 0.0 || beta == 1.0);
    if (k->H) return dense_many(k, 0, k->nx, k->nx, nrhs, alpha, k->H, k->ldh, X, ldx, beta, Y, ldy);
    if (k->h.ptr) return madqp_spmm_csr(ctx, k->nx, k->h, alpha, X, ldx, beta, Y, ldy, nrhs, MADQP_PROF_GEMV);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    for (int64_t c = 0; c < nrhs; ++c) LAUNCH(hdiag_mul_kernel, k->nx, k->nx, alpha, k->hdiag, X + c * ldx, beta, Y + c * ldy);
    return MADQP_OK;
}
// passes over the arrays of A (or A') / of H that ONE product on nrhs columns makes: per column, or per group of the block form
static int64_t kkt_passes(int64_t nrhs, bool block, bool csr) {
    if (!block || nrhs < 2) return nrhs;
    const int64_t g = csr ? MADQP_SPMM_GROUP : MADQP_GEMV_MANY_GROUP;
    return (nrhs + g - 1) / g;
}

extern "C" int32_t madqp_kkt_destroy(madqp_kkt* k) {
    if (!k) return MADQP_OK;
    (void)hipStreamSynchronize(k->ctx->stream);
    if (k->chol) madqp_chol_destroy(k->chol);
    delete k;  // (its owner frees the buffers)
    return MADQP_OK;
}

// Every creation function ends here.  a / at: the borrowed CSR of A and A' of the sparse front end (A == At == nullptr
// then); packed: no K until madqp_kkt_set_bandwidth knows the band's extent.  On failure *out stays nullptr.
static int32_t kkt_create_common(madqp_ctx* ctx, int mode, int64_t nx, int64_t m, int64_t ns,
                                 const int64_t* ind_ineq_host, const double* H, int64_t ldh,
                                 const double* A, int64_t lda, const double* At, int64_t ldat,
                                 const Csr& a, const Csr& at, bool packed, madqp_kkt** out) {
    ARG_TRY(ctx, out && nx >= 0 && m >= 0 && ns >= 0 && ns <= m);
    ARG_TRY(ctx, ns == 0 || ind_ineq_host);
    *out = nullptr;
    std::vector<int64_t> slot((size_t)std::max<int64_t>(m, 1));
    ARG_TRY(ctx, kkt_slot_map(ind_ineq_host, ns, m, slot.data()));
    madqp_kkt* k = new (std::nothrow) madqp_kkt();
    if (!k) return madqp_fail(ctx, MADQP_ERR_ALLOC, "host allocation failed");
    k->ctx = k->mem.ctx = ctx;
    k->mode = mode;
    k->nx = nx;
    k->m = m;
    k->ns = ns;
    {
        const char* e_fuse = getenv("MADQP_KKT_FUSE");  // 0: the separate per-variable kernels (A/B tests)
        k->fuse = !(e_fuse && e_fuse[0] == '0');
    }
    k->H = H;
    k->ldh = ldh;
    k->A = A;
    k->lda = lda;
    k->At = At;
    k->ldat = ldat;
    k->a = a;
    k->at = at;
    const KktOrders o = kkt_orders(mode, nx, m);
    k->np = o.np;
    k->packed = packed;
    const int64_t n = nx + ns;
    const char* who = "madqp_kkt_create";
    int32_t r = MADQP_OK;
    if (!packed) {  // (packed: the band alone, once its extent is known)
        k->ldk = o.ldk;
        k->k_doubles = o.k_doubles;
        r = k->mem.alloc(&k->K, o.k_doubles, who, /*zero=*/true);
    }
    if (!r) r = k->mem.alloc(&k->d_ind_ineq, ns, who);
    if (!r) r = k->mem.alloc(&k->d_slot, m, who);
    if (!r) r = k->mem.alloc(&k->theta, m, who);
    if (!r) r = k->mem.alloc(&k->t, m, who);
    if (!r) r = k->mem.alloc(&k->u, m, who);
    if (!r && mode == KKT_NORMAL) r = k->mem.alloc(&k->dn, n, who);
    if (!r && mode == KKT_NORMAL) r = k->mem.alloc(&k->tn, n, who);
    if (!r && mode == KKT_AUGMENTED) r = k->mem.alloc(&k->b, o.stored_order, who);
    hipError_t e = hipSuccess;
    if (!r && ns) e = hipMemcpy(k->d_ind_ineq, ind_ineq_host, ns * sizeof(int64_t), hipMemcpyHostToDevice);
    if (!r && e == hipSuccess && m) e = hipMemcpy(k->d_slot, slot.data(), m * sizeof(int64_t), hipMemcpyHostToDevice);
    if (!r && e != hipSuccess)
        r = madqp_fail(ctx, MADQP_ERR_ALLOC, "madqp_kkt_create(nx=%lld, m=%lld): %s", (long long)nx, (long long)m,
                       hipGetErrorString(e));
    if (!r) r = madqp_chol_create(ctx, o.stored_order, &k->chol);
    if (!r && mode == KKT_AUGMENTED) r = madqp_chol_set_signature(k->chol, k->np);
    if (r) {
        madqp_kkt_destroy(k);
        return r;
    }
    *out = k;
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_create(madqp_ctx* ctx, int64_t nx, int64_t m, int64_t ns,
                                    const int64_t* ind_ineq_host, const double* H, int64_t ldh,
                                    const double* A, int64_t lda, madqp_kkt** out) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, !H || ldh >= nx);
    ARG_TRY(ctx, m == 0 || nx == 0 || (A && lda >= nx));
    return kkt_create_common(ctx, KKT_CONDENSED, nx, m, ns, ind_ineq_host, H, ldh, A, lda, nullptr, 0, {}, {}, false, out);
}

// Sparse front end: A as CSR (a_*: m rows, column indices < nx, ascending within a row) and A' as CSR
// (at_*: nx rows, indices < m), both device, int64, borrowed.  mode 0: condensed K = H + Sigma_x + A' Theta A
// (H dense, NULL, diagonal through madqp_kkt_set_hdiag or CSR through madqp_kkt_set_hcsr), mode 1: the reference's
// normal equations A Sigma^-1 A' (LP only, or H diagonal), mode 2: the augmented system [H + Sigma_x, A'; A, -D] (H as in
// mode 0).  (The modes of the interface are the KKT_* values.)
extern "C" int32_t madqp_kkt_create_sparse(madqp_ctx* ctx, int32_t mode, int64_t nx, int64_t m, int64_t ns,
                                           const int64_t* ind_ineq_host, const double* H, int64_t ldh,
                                           const int64_t* a_ptr, const int64_t* a_col, const double* a_val,
                                           const int64_t* at_ptr, const int64_t* at_col, const double* at_val,
                                           madqp_kkt** out) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, (mode >= 0 && mode <= 2) && a_ptr && at_ptr && (!H || ldh >= nx) && !(mode == 1 && H));
    return kkt_create_common(ctx, mode, nx, m, ns, ind_ineq_host, H, ldh, nullptr, 0, nullptr, 0, {a_ptr, a_col, a_val},
                             {at_ptr, at_col, at_val}, /*packed=*/false, out);
}

// The same object on PACKED band storage: no dense H (NULL, diagonal or CSR as above), mode 0 or 1, and no K at all until
// madqp_kkt_set_bandwidth -- which such an object needs before anything is built, factorised or solved (MADQP_ERR_STATE
// until then) -- allocates the band: npad (ld + 1) + 128 doubles instead of the ldk x ldk of the dense storage.
extern "C" int32_t madqp_kkt_create_sparse_packed(madqp_ctx* ctx, int32_t mode, int64_t nx, int64_t m, int64_t ns,
                                                  const int64_t* ind_ineq_host, const int64_t* a_ptr, const int64_t* a_col,
                                                  const double* a_val, const int64_t* at_ptr, const int64_t* at_col,
                                                  const double* at_val, madqp_kkt** out) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, (mode == 0 || mode == 1) && a_ptr && at_ptr);
    return kkt_create_common(ctx, mode, nx, m, ns, ind_ineq_host, nullptr, 0, nullptr, 0, nullptr, 0, {a_ptr, a_col, a_val},
                             {at_ptr, at_col, at_val}, /*packed=*/true, out);
}
// a packed object has no storage before its bandwidth is set
static int32_t kkt_storage_ready(madqp_kkt* k, const char* what) {
    if (k->packed && !k->K)
        return madqp_fail(k->ctx, MADQP_ERR_STATE, "%s: a packed KKT object has no storage before madqp_kkt_set_bandwidth", what);
    return MADQP_OK;
}

// Diagonal Hessian H = diag(hdiag) (nx entries, device, borrowed) for a KKT object created without a dense
// H: the condensed matrix becomes diag(hdiag) + Sigma_x + A' Theta A, the normal equations A (H + Sigma)^-1 A'
// ("the alternative of row 6 applies verbatim with Sigma -> H + Sigma") -- the reference's
// NormalKKTSystem is LP only (src/KKT/normalkkt.jl:45-48); this is the diagonal-H extension CONT-type QPs need.
extern "C" int32_t madqp_kkt_set_hdiag(madqp_kkt* k, const double* hdiag) {
    if (!k) return MADQP_ERR_ARG;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, hdiag && !k->H && !k->h.ptr);
    ARG_TRY(ctx, k->bw < 0);  // the bandwidth was checked against the Hessian the object held
    if (!k->sg)
        if (int32_t r = k->mem.alloc(&k->sg, k->nx + k->ns, "madqp_kkt_set_hdiag")) return r;
    k->hdiag = hdiag;
    return MADQP_OK;
}

// Sparse Hessian for the sparse front end: the FULL symmetric pattern of H in CSR (nx rows, column indices ascending
// within a row, no duplicates; device, borrowed) for an object created by madqp_kkt_create_sparse without a dense H, in
// the condensed or the augmented form.  Both triangles are stored so that H x is one row-wise mat-vec in a fixed order
// (no atomics) and column j of the lower triangle is row j's entries with col >= j.  One 8-byte read-back of h_ptr[nx].
extern "C" int32_t madqp_kkt_set_hcsr(madqp_kkt* k, const int64_t* h_ptr, const int64_t* h_col, const double* h_val) {
    if (!k) return MADQP_ERR_ARG;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, h_ptr && !k->H && !k->hdiag);
    ARG_TRY(ctx, k->a.ptr && k->mode != KKT_NORMAL && !k->scaled);
    ARG_TRY(ctx, k->bw < 0);  // the bandwidth was checked against the Hessian the object held
    int64_t nnz = 0;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(&nnz, h_ptr + k->nx, sizeof(int64_t), hipMemcpyDeviceToHost));
    ARG_TRY(ctx, nnz >= 0 && (nnz == 0 || (h_col && h_val)));
    k->h = {h_ptr, h_col, h_val};
    return MADQP_OK;
}

// The two positive definite forms are one weighted Gram matrix  K = base + diag(dvec) + V diag(w) V'  of order `order`
// with inner dimension `inner`, roles swapped:
//   condensed  V = A' (rows = variables),   w = Theta over the constraints,   dvec = Sigma_x (+ hdiag),  base = H
//   normal     V = A  (rows = constraints), w = 1/Sigma over the variables,   dvec = Sigma_s^-1 on the inequality rows
// v / vt: the rows of V and of V' of the sparse front end; dense: the operand of the dense one, row k of V' contiguous.
struct KktGram {
    int64_t order = 0, inner = 0;
    Csr v, vt;
    const double* dense = nullptr;
    int64_t ld = 0;
    const double *w = nullptr, *dvec = nullptr;
    const double* base = nullptr;  // dense base, or
    int64_t ldbase = 0;
    Csr hbase;  // symmetric CSR base, or none
};
// st == nullptr: the pattern alone (madqp_kkt_set_bandwidth)
static KktGram kkt_gram(const madqp_kkt* k, const madqp_state* st) {
    KktGram g;
    if (k->mode == KKT_NORMAL) {
        g.order = k->m;
        g.inner = k->nx;
        g.v = k->a;
        g.vt = k->at;
        g.dense = k->At;
        g.ld = k->ldat;
        g.w = k->dn;
        g.dvec = k->theta;
    } else {
        g.order = k->nx;
        g.inner = k->m;
        g.v = k->at;
        g.vt = k->a;
        g.dense = k->A;
        g.ld = k->lda;
        g.w = k->theta;
        g.dvec = k->hdiag ? k->sg : st ? st->pr_diag : nullptr;  // diagonal of H + Sigma_x
        g.base = k->H;
        g.ldbase = k->ldh;
        g.hbase = k->h;
    }
    return g;
}

// Band-limited assembly and factorisation (see include/madqp.h).  The pattern's bandwidth is read off the structures the
// object holds, once, on the host (kkt_form.inc): the rows of V' of the Gram description, and the CSR of H.
static int32_t csr_download(madqp_ctx* ctx, int64_t rows, const int64_t* d_ptr, const int64_t* d_col,
                            std::vector<int64_t>& ptr, std::vector<int64_t>& col) {
    ptr.assign((size_t)rows + 1, 0);
    HIP_TRY(ctx, hipMemcpy(ptr.data(), d_ptr, (size_t)(rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    ARG_TRY(ctx, ptr[0] == 0 && ptr[rows] >= 0);
    col.assign((size_t)ptr[rows], 0);
    if (ptr[rows]) HIP_TRY(ctx, hipMemcpy(col.data(), d_col, (size_t)ptr[rows] * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MADQP_OK;
}
extern "C" int32_t madqp_kkt_set_bandwidth(madqp_kkt* k, int64_t bw) {
    if (!k) return MADQP_ERR_ARG;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, k->a.ptr && !k->H && (k->mode == KKT_CONDENSED || k->mode == KKT_NORMAL) && !k->scaled);
    ARG_TRY(ctx, bw >= 0 && bw < kkt_orders(k->mode, k->nx, k->m).rule_order);
    if (k->packed && k->K)
        return madqp_fail(ctx, MADQP_ERR_STATE, "madqp_kkt_set_bandwidth: the packed storage of this object is laid out already");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const KktGram g = kkt_gram(k, nullptr);
    std::vector<int64_t> ptr, col;
    int32_t r = csr_download(ctx, g.inner, g.vt.ptr, g.vt.col, ptr, col);
    if (r) return r;
    int64_t pattern = kkt_pattern_halfbandwidth(g.inner, ptr.data(), col.data());
    if (g.hbase.ptr) {
        if ((r = csr_download(ctx, g.order, g.hbase.ptr, g.hbase.col, ptr, col))) return r;
        pattern = std::max(pattern, kkt_csr_halfbandwidth(g.order, ptr.data(), col.data()));
    }
    if (bw < pattern)
        return madqp_fail(ctx, MADQP_ERR_ARG, "madqp_kkt_set_bandwidth(%lld): the pattern's half-bandwidth is %lld",
                          (long long)bw, (long long)pattern);
    if ((r = madqp_chol_set_bandwidth(k->chol, bw))) return r;
    int64_t extent = 0;
    if ((r = madqp_chol_band_extent(k->chol, &extent))) return r;
    if (k->packed) {  // the band alone, zeroed once: every build rewrites the rows j .. j + extent of every column
        int64_t lay[2] = {0, 0};
        double* band = nullptr;
        const size_t before = k->mem.owned.size();
        r = madqp_chol_packed_layout(k->chol, 0, lay);
        if (!r) r = madqp_chol_set_packed(k->chol, 1);
        if (!r) r = k->mem.alloc(&band, lay[1], "madqp_kkt_set_bandwidth: packed storage", /*zero=*/true);
        if (r) {  // nothing is committed: the object has no storage and takes another madqp_kkt_set_bandwidth
            k->mem.release(before);
            (void)madqp_chol_set_bandwidth(k->chol, -1);
            return r;
        }
        k->K = band;
        k->ldk = lay[0];
        k->k_doubles = lay[1];
    } else {
        // K once: from now on nothing writes beyond the extent.  No reader of these zeros is left -- the sweeps of a solve stay
        // inside the extent too (chol.hip, band form; MADQP_SWEEP_BAND=0 alone still streams the whole lower triangle)
        HIP_TRY(ctx, hipMemsetAsync(k->K, 0, (size_t)k->k_doubles * sizeof(double), ctx->stream));
    }
    k->bw = bw;
    k->band_extent = extent;
    return MADQP_OK;
}

// Augmented (K2) system [H + Sigma_x, A'; A, -D] of order ceil128(nx) + m; same operands as madqp_kkt_create.
// H may be NULL (LP, or a diagonal Hessian through madqp_kkt_set_hdiag).
extern "C" int32_t madqp_kkt_create_augmented(madqp_ctx* ctx, int64_t nx, int64_t m, int64_t ns,
                                              const int64_t* ind_ineq_host, const double* H, int64_t ldh,
                                              const double* A, int64_t lda, madqp_kkt** out) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, !H || ldh >= nx);
    ARG_TRY(ctx, m == 0 || nx == 0 || (A && lda >= nx));
    return kkt_create_common(ctx, KKT_AUGMENTED, nx, m, ns, ind_ineq_host, H, ldh, A, lda, nullptr, 0, {}, {}, false, out);
}

// K2.5: the augmented system symmetrically scaled (MadNLP's ScaledSparseKKTSystem; see the header comment).
extern "C" int32_t madqp_kkt_create_scaled_augmented(madqp_ctx* ctx, int64_t nx, int64_t m, int64_t ns,
                                                     const int64_t* ind_ineq_host, const double* H, int64_t ldh,
                                                     const double* A, int64_t lda, madqp_kkt** out) {
    int32_t r = madqp_kkt_create_augmented(ctx, nx, m, ns, ind_ineq_host, H, ldh, A, lda, out);
    if (r) return r;
    madqp_kkt* k = *out;
    const int64_t n = nx + ns;
    r = k->mem.alloc(&k->sfac, n, "madqp_kkt_create_scaled_augmented");
    if (!r) r = k->mem.alloc(&k->sb, n, "madqp_kkt_create_scaled_augmented");
    if (r) {
        madqp_kkt_destroy(k);
        *out = nullptr;
        return r;
    }
    k->scaled = 1;
    if (n) LAUNCH(k25_ones_kernel, n, n, k->sfac);
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_create_normal(madqp_ctx* ctx, int64_t nx, int64_t m, int64_t ns,
                                           const int64_t* ind_ineq_host, const double* At,
                                           int64_t ldat, madqp_kkt** out) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, m == 0 || nx == 0 || (At && ldat >= m));
    return kkt_create_common(ctx, KKT_NORMAL, nx, m, ns, ind_ineq_host, nullptr, 0, nullptr, 0, At, ldat, {}, {}, false, out);
}

static int32_t check_kkt_state(madqp_kkt* k, const madqp_state* st) {
    if (!k) return MADQP_ERR_ARG;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, st != nullptr);
    ARG_TRY(ctx, st->n == k->nx + k->ns && st->m == k->m);
    return MADQP_OK;
}

// [H + Sigma_x, A'; A, -D], lower triangle, identity over the padding rows nx .. np
static int32_t kkt_build_augmented(madqp_kkt* k, const madqp_state* st) {
    madqp_ctx* ctx = k->ctx;
    const int64_t N = k->np + k->m;
    if (N == 0) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_SYRK);
    const double* sf = k->scaled ? k->sfac : nullptr;
    if (k->m) LAUNCH(aug_diag_kernel, k->m, k->m, k->nx, k->d_slot, st->pr_diag, st->du_diag, sf, k->theta);
    const unsigned tiles = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(aug_fill_kernel, dim3(tiles, tiles), dim3(256), 0, ctx->stream, k->nx, k->np, k->m, k->H,
                       k->ldh, k->hdiag, st->pr_diag, k->A, k->lda, k->theta, sf, k->K, k->ldk);
    LAUNCH_CHECK(ctx);
    if (k->a.ptr && k->m) {
        hipLaunchKernelGGL(aug_scatter_kernel, dim3((unsigned)((k->m * 16 + 255) / 256)), dim3(256), 0, ctx->stream,
                           k->m, k->np, k->a.ptr, k->a.col, k->a.val, sf, k->K, k->ldk);
        LAUNCH_CHECK(ctx);
    }
    if (k->h.ptr && k->nx) {
        hipLaunchKernelGGL(aug_scatter_h_kernel, dim3((unsigned)((k->nx * 16 + 255) / 256)), dim3(256), 0, ctx->stream,
                           k->nx, k->h.ptr, k->h.col, k->h.val, st->pr_diag, k->K, k->ldk);
        LAUNCH_CHECK(ctx);
    }
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_build(madqp_kkt* k, const madqp_state* st) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    if ((r = kkt_storage_ready(k, "madqp_kkt_build"))) return r;
    madqp_ctx* ctx = k->ctx;
    if (k->mode == KKT_AUGMENTED) return kkt_build_augmented(k, st);
    {  // the vectors of the Gram description (kkt_gram)
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (k->mode == KKT_NORMAL) {
            // S = A diag(D_x) A' + diag(D_s on inequality rows),  D = 1/Sigma; du_diag is NOT added
            // (src/KKT/normalkkt.jl:166-180, src/utils.jl:266-298)
            if (k->hdiag && st->n) LAUNCH(sigma_h_kernel, st->n, st->n, k->nx, st->pr_diag, k->hdiag, k->sg);
            if (st->n) LAUNCH(recip_kernel, st->n, st->n, k->hdiag ? k->sg : st->pr_diag, k->dn);
            if (k->m) LAUNCH(slack_diag_kernel, k->m, k->m, k->nx, k->d_slot, k->dn, k->theta);
        } else {
            if (k->m) LAUNCH(theta_kernel, k->m, k->m, k->nx, k->d_slot, st->pr_diag, st->du_diag, k->theta);
            if (k->hdiag && st->n) LAUNCH(sigma_h_kernel, st->n, st->n, k->nx, st->pr_diag, k->hdiag, k->sg);
        }
    }
    const KktGram g = kkt_gram(k, st);
    if (k->a.ptr && k->bw >= 0)
        return madqp_sparse_gram_band(ctx, g.order, g.v, g.vt, g.w, g.dvec, g.hbase, k->K, k->ldk, k->bw, k->band_extent);
    if (k->a.ptr) return madqp_sparse_gram(ctx, g.order, g.v, g.vt, g.w, g.base, g.ldbase, g.dvec, g.hbase, k->K, k->ldk);
    return madqp_syrk_assemble_impl(ctx, g.order, g.inner, g.dense, g.ld, g.w, g.base, g.ldbase, g.dvec, k->K, k->ldk);
}

// set_aug_diagonal_reg!(kkt, solver), dispatched on the KKT type as the reference does (src/kernels.jl:128 for every
// AbstractKKTSystem, :149 for ScaledSparseKKTSystem)
extern "C" int32_t madqp_kkt_set_aug_diagonal_reg(madqp_kkt* k, const madqp_state* st, double del_w, double del_c) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    madqp_ctx* ctx = k->ctx;
    if (!k->scaled) return madqp_set_aug_diagonal_reg(ctx, st, del_w, del_c);
    ARG_TRY(ctx, st->x && st->xl && st->xu && st->zl && st->zu);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (std::max(st->n, st->m) > 0) LAUNCH(k25_fill_kernel, std::max(st->n, st->m), *st, del_w, del_c, k->sfac, k->sb);
    if (std::max(st->nlb, st->nub) > 0) LAUNCH(k25_bounds_kernel, std::max(st->nlb, st->nub), *st, k->sfac, k->sb);
    if (st->n) LAUNCH(k25_final_kernel, st->n, *st, del_w, k->sfac, k->sb);
    return MADQP_OK;
}

// MadNLP.initialize!(kkt) (src/KKT/normalkkt.jl:136-147): reg = pr_diag = 1, du_diag = 0, l_lower = u_lower = 0,
// l_diag = u_diag = 1 -- and, for K2.5, scaling factor 1
extern "C" int32_t madqp_kkt_initialize(madqp_kkt* k, const madqp_state* st) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    madqp_ctx* ctx = k->ctx;
    if ((r = madqp_fill(ctx, st->n, 1.0, st->reg)) || (r = madqp_fill(ctx, st->n, 1.0, st->pr_diag)) ||
        (r = madqp_fill(ctx, st->m, 0.0, st->du_diag)) || (r = madqp_fill(ctx, st->nlb, 0.0, st->l_lower)) ||
        (r = madqp_fill(ctx, st->nub, 0.0, st->u_lower)) || (r = madqp_fill(ctx, st->nlb, 1.0, st->l_diag)) ||
        (r = madqp_fill(ctx, st->nub, 1.0, st->u_diag)))
        return r;
    if (k->scaled && st->n) LAUNCH(k25_ones_kernel, st->n, st->n, k->sfac);
    return MADQP_OK;
}

// the Cholesky handle and the order it was created with (kkt_form.inc: stored_order)
extern "C" int32_t madqp_kkt_chol(madqp_kkt* k, madqp_chol** chol, int64_t* order) {
    if (!k || !chol) return MADQP_ERR_ARG;
    *chol = k->chol;
    if (order) *order = kkt_orders(k->mode, k->nx, k->m).stored_order;
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_factorize(madqp_kkt* k, int32_t* info_host) {
    if (!k) return MADQP_ERR_ARG;
    if (int32_t r = kkt_storage_ready(k, "madqp_kkt_factorize")) return r;
    return madqp_chol_factor(k->chol, k->K, k->ldk, info_host);
}
// queued form: the factorisation is enqueued, its info lands in the result block and comes back with the caller's next
// madqp_read_results
int32_t madqp_q_kkt_factorize(madqp_kkt* k, int slot0) {
    if (!k) return MADQP_ERR_ARG;
    if (int32_t r = kkt_storage_ready(k, "madqp_kkt_factorize")) return r;
    return madqp_chol_factor_q(k->chol, k->K, k->ldk, k->ctx->d_res + slot0);
}

static int32_t kkt_solve_once(madqp_kkt* k, const madqp_state* st, double* w);

// The fused passes serve the condensed mode with dense or sparse A, unscaled; the lists of st must be the ones the
// inverse maps were made from (same pointers and lengths: the state layout is fixed while a KKT object lives,
// include/madqp.h) -- they are made again when that changes.
static bool kkt_fusable(const madqp_kkt* k) { return k->fuse && k->mode == KKT_CONDENSED && !k->scaled && k->m > 0; }
static int32_t ensure_pos(madqp_kkt* k, const madqp_state* st) {
    madqp_ctx* ctx = k->ctx;
    if (k->pos_ok && k->pos_key_lb == st->ind_lb && k->pos_key_ub == st->ind_ub && k->pos_nlb == st->nlb &&
        k->pos_nub == st->nub && k->pos_n == st->n)
        return MADQP_OK;
    k->pos_ok = false;
    const char* who = "inverse bound lists";
    int32_t r = k->mem.grow(&k->pos_lb, &k->pos_lb_cap, st->n, who);
    if (!r) r = k->mem.grow(&k->pos_ub, &k->pos_ub_cap, st->n, who);
    if (!r && !k->rs) r = k->mem.alloc(&k->rs, k->ns, who);
    if (r) return r;
    ARG_TRY(ctx, st->n < (int64_t)1 << 31 && st->nlb < (int64_t)1 << 31 && st->nub < (int64_t)1 << 31);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (st->n) LAUNCH(pos_fill_kernel, st->n, st->n, k->pos_lb, k->pos_ub);
    if (st->nlb) LAUNCH(pos_scatter_kernel, st->nlb, st->nlb, st->ind_lb, k->pos_lb);
    if (st->nub) LAUNCH(pos_scatter_kernel, st->nub, st->nub, st->ind_ub, k->pos_ub);
    k->pos_ok = true;
    k->pos_key_lb = st->ind_lb;
    k->pos_key_ub = st->ind_ub;
    k->pos_nlb = st->nlb;
    k->pos_nub = st->nub;
    k->pos_n = st->n;
    return MADQP_OK;
}

// w = K^-1 p (p untouched; w a different vector), optionally pcopy = p on the way: solve_system!'s copy, solve! and the
// copy in front of its residual (src/linear_solver.jl:19-35) -- in the condensed mode with the per-variable passes fused
int32_t madqp_kkt_solve_from(madqp_kkt* k, const madqp_state* st, const double* p, double* w, double* pcopy) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    if ((r = kkt_storage_ready(k, "madqp_kkt_solve"))) return r;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, p && w && p != w);
    const int64_t len = st->n + st->m + st->nlb + st->nub;
    if (!kkt_fusable(k) || k->refine > 0) {
        if ((r = madqp_copy(ctx, len, p, w))) return r;
        if ((r = madqp_kkt_solve(k, st, w))) return r;
        return pcopy ? madqp_copy(ctx, len, p, pcopy) : MADQP_OK;
    }
    if ((r = ensure_pos(k, st))) return r;
    k->u_is_A_of = nullptr;
    const int64_t L = std::max(std::max(st->n, st->m), std::max(st->nlb, st->nub));
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(solve_pre_kernel, L, *st, p, w, k->pos_lb, k->pos_ub, k->nx, k->d_slot, k->theta, k->t, k->u, k->rs);
    }
    if ((r = apply_At(k, 1.0, k->u, 1.0, w))) return r;  // rhs_x = r1_x + A' (theta t)
    if ((r = madqp_chol_solve(k->chol, w))) return r;
    if ((r = apply_A(k, 1.0, w, 0.0, k->u))) return r;
    {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(solve_post_kernel, L, *st, w, k->nx, k->d_slot, k->d_ind_ineq, k->theta, k->t, k->u, k->rs, p, pcopy);
    }
    k->u_is_A_of = w;  // dx is final since the sweeps: u = A dx (madqp_kkt_mul_solved)
    return MADQP_OK;
}

// Steps of iterative refinement INSIDE solve!: w = K^-1 p, then w += K^-1 (p - K w) -- for hosts whose loop is not ours.
// MadIPM's solve_system! (src/linear_solver.jl:19-45) calls solve!(kkt, d) once and only LOOKS at the residual; the device
// factorisation multiplies with explicit inverses of 16 x 16 sub-blocks where LAPACK substitutes scalar by scalar, which on
// small ill-conditioned problems shows in the per-iteration traces and which one step removes.  The
// Julia glue asks for the AUTO rule (steps = -1: one step while the system has order <= 1024, none above -- rule_order of
// kkt_form.inc, nx + m for the augmented form whatever its padding: the rule madqp_jl_amd/options.py applies in the drivers
// of this repository, which refine in their own solve_system with the residual they form anyway and leave this at 0).
// Arithmetic: operation for operation the drivers' (bitwise equal results).
extern "C" int32_t madqp_kkt_set_refine(madqp_kkt* k, int32_t steps) {
    if (!k) return MADQP_ERR_ARG;
    ARG_TRY(k->ctx, steps >= -1 && steps <= 8);
    if (steps < 0) {
        static const int64_t auto_max = getenv("MADQP_REFINE_AUTO_MAX") ? atoll(getenv("MADQP_REFINE_AUTO_MAX")) : 1024;
        steps = kkt_orders(k->mode, k->nx, k->m).rule_order <= auto_max ? 1 : 0;
    }
    k->refine = steps;
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_solve(madqp_kkt* k, const madqp_state* st, double* w) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    if ((r = kkt_storage_ready(k, "madqp_kkt_solve"))) return r;
    ARG_TRY(k->ctx, w != nullptr);
    if (k->refine <= 0) return kkt_solve_once(k, st, w);
    madqp_ctx* ctx = k->ctx;
    const int64_t len = st->n + st->m + st->nlb + st->nub;
    const int64_t stride = (len + 31) / 32 * 32;  // both vectors 256-byte aligned, as two allocations were
    if ((r = k->mem.grow(&k->rf, &k->rf_cap, 2 * stride, "madqp_kkt_solve: work vectors of the refinement steps"))) return r;
    double *rf_p = k->rf, *rf_r = k->rf + stride;
    if ((r = madqp_copy(ctx, len, w, rf_p))) return r;  // p
    if ((r = kkt_solve_once(k, st, w))) return r;       // w = K^-1 p
    for (int32_t it = 0; it < k->refine; ++it) {
        if ((r = madqp_copy(ctx, len, rf_p, rf_r))) return r;
        if ((r = madqp_kkt_mul(k, st, rf_r, w, -1.0, 1.0))) return r;  // r = p - K w
        if ((r = kkt_solve_once(k, st, rf_r))) return r;
        if ((r = madqp_axpy(ctx, len, 1.0, rf_r, w))) return r;  // w += K^-1 r
    }
    k->u_is_A_of = nullptr;  // (u belongs to the last correction, not to w)
    return MADQP_OK;
}

// The work vectors of one right-hand side: the object's own (madqp_kkt_solve), or one column of each of the blocks that
// madqp_kkt_solve_many grows (kkt_many_work)
struct KktWork {
    double *t, *u;  // m
    double* tn;     // normal mode: n
    double* b;      // augmented mode: the stored order
};
static KktWork kkt_own_work(const madqp_kkt* k) { return KktWork{k->t, k->u, k->tn, k->b}; }
// what the factor solves for the right-hand side w: dy in place (normal), the vector b (augmented), dx in place (condensed)
static double* kkt_factor_rhs(const madqp_kkt* k, const madqp_state* st, double* w, const KktWork& wk) {
    return k->mode == KKT_NORMAL ? w + st->n : k->mode == KKT_AUGMENTED ? wk.b : w;
}

// The middle of a solve, two functions per form around the factor solve: on entry of `before` w holds the reduced
// right-hand side [r1; r2; ..], on return of `after` dx (with ds) in wx and dy in wy.  Each is three pieces in order -- the
// vector passes in front of the form's product with A or A' (part KKT_HEAD), the product (KKT_PRODUCT), the vector passes
// behind it (KKT_TAIL) -- so that a many-column solve can run the product of all columns as one block between them
// (kkt_stage_product / kkt_solve_many_once).  A one-vector solve asks for all three.
enum { KKT_HEAD = 1, KKT_PRODUCT = 2, KKT_TAIL = 4, KKT_ALL = 7 };
// the product of a stage: y <- op x + beta y on the vectors of one column (op: 0 none, 1 A, 2 A')
struct KktProduct {
    int op;
    const double* x;
    double beta;
    double* y;
};
static int32_t kkt_run_product(madqp_kkt* k, const KktProduct& p) {
    return p.op == 1 ? apply_A(k, 1.0, p.x, p.beta, p.y) : p.op == 2 ? apply_At(k, 1.0, p.x, p.beta, p.y) : MADQP_OK;
}
static KktProduct kkt_before_product(const madqp_kkt* k, const madqp_state* st, double* w, const KktWork& wk) {
    if (k->mode == KKT_NORMAL) return KktProduct{1, wk.tn, 0.0, wk.u};                   // A r1
    if (k->mode == KKT_CONDENSED && k->m) return KktProduct{2, wk.u, 1.0, w};              // rhs_x = r1_x + A' (theta t)
    return KktProduct{0, nullptr, 0.0, nullptr};
}
static KktProduct kkt_after_product(const madqp_kkt* k, const madqp_state* st, double* w, const KktWork& wk) {
    if (k->mode == KKT_NORMAL) return KktProduct{2, w + st->n, 0.0, wk.tn};               // A' dy
    if (k->mode == KKT_CONDENSED && k->m) return KktProduct{1, w, 0.0, wk.u};              // A dx
    return KktProduct{0, nullptr, 0.0, nullptr};
}
static int32_t kkt_normal_before(madqp_kkt* k, const madqp_state* st, double* wx, double* wy, const KktWork& wk, int parts) {  // src/KKT/normalkkt.jl:185-201
    int32_t r = 0;
    madqp_ctx* ctx = k->ctx;
    const double* sig = k->hdiag ? k->sg : st->pr_diag;  // H + Sigma
    if (parts & KKT_HEAD) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (st->n) LAUNCH(div_kernel, st->n, st->n, wx, sig, wk.tn);  // r1 = (H + Sigma)^-1 wx
    }
    if ((parts & KKT_PRODUCT) && (r = kkt_run_product(k, kkt_before_product(k, st, wx, wk)))) return r;
    if ((parts & KKT_TAIL) && k->m) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(normal_rhs_kernel, k->m, k->m, k->d_slot, wk.u, wk.tn + k->nx, wy, wy);  // A r1 - r2
    }
    return MADQP_OK;  // the factor: wy = dy
}
static int32_t kkt_normal_after(madqp_kkt* k, const madqp_state* st, double* wx, double* wy, const KktWork& wk, int parts) {
    int32_t r = 0;
    madqp_ctx* ctx = k->ctx;
    const double* sig = k->hdiag ? k->sg : st->pr_diag;
    if ((parts & KKT_PRODUCT) && (r = kkt_run_product(k, kkt_after_product(k, st, wx, wk)))) return r;
    if (!(parts & KKT_TAIL)) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_VEC);
    if (k->ns) LAUNCH(jt_slack_kernel, k->ns, k->ns, k->d_ind_ineq, wy, wk.tn + k->nx, 1.0, 0.0);
    if (st->n) LAUNCH(normal_back_kernel, st->n, st->n, wk.tn, sig, wx);
    return MADQP_OK;
}
static int32_t kkt_augmented_before(madqp_kkt* k, const madqp_state* st, double* wx, double* wy, const KktWork& wk) {
    madqp_ctx* ctx = k->ctx;
    const int64_t N = k->np + k->m;
    const double* sf = k->scaled ? k->sfac : nullptr;
    if (N) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(aug_rhs_kernel, N, k->nx, k->np, k->m, k->d_slot, st->pr_diag, sf, wx, wy, wk.b);
    }
    return MADQP_OK;  // the factor: b
}
static int32_t kkt_augmented_after(madqp_kkt* k, const madqp_state* st, double* wx, double* wy, const KktWork& wk) {
    madqp_ctx* ctx = k->ctx;
    const double* sf = k->scaled ? k->sfac : nullptr;
    if (k->nx + k->m) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(aug_back_kernel, k->nx + k->m, k->nx, k->np, k->m, k->d_slot, st->pr_diag, sf, wk.b, wx, wy);
    }
    return MADQP_OK;
}
static int32_t kkt_condensed_before(madqp_kkt* k, const madqp_state* st, double* wx, double* wy, const KktWork& wk, int parts) {
    madqp_ctx* ctx = k->ctx;
    if (k->m) {
        if (parts & KKT_HEAD) {
            ProfScope ps(ctx, MADQP_PROF_VEC);
            LAUNCH(condense_kernel, k->m, k->m, k->nx, k->d_slot, st->pr_diag, k->theta, wx, wy, wk.t, wk.u);
        }
        if (parts & KKT_PRODUCT)
            if (int32_t r = kkt_run_product(k, kkt_before_product(k, st, wx, wk))) return r;
    }
    return MADQP_OK;  // the factor: wx = dx
}
static int32_t kkt_condensed_after(madqp_kkt* k, const madqp_state* st, double* wx, double* wy, const KktWork& wk, int parts) {
    madqp_ctx* ctx = k->ctx;
    if (k->m) {
        if (parts & KKT_PRODUCT)
            if (int32_t r = kkt_run_product(k, kkt_after_product(k, st, wx, wk))) return r;
        if (!(parts & KKT_TAIL)) return MADQP_OK;
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(decondense_kernel, k->m, k->m, k->nx, k->d_slot, st->pr_diag, k->theta, wk.t, wk.u, wx, wy);
    }
    return MADQP_OK;
}

// The three stages of a solve.  Before the factor solve: reduce_rhs! and the first half of the form's middle -- the K2.5
// object with its sign-flipped first and last step.  parts: see KKT_HEAD above (reduce_rhs! belongs to the head,
// finish_aug_solve! to the tail; the augmented forms have no product: their middle is head and tail at once).
static int32_t kkt_solve_before(madqp_kkt* k, const madqp_state* st, double* w, const KktWork& wk, int parts = KKT_ALL) {
    int32_t r = 0;
    madqp_ctx* ctx = k->ctx;
    if ((parts & KKT_HEAD) && k->scaled) {  // r1 = p_x + p_zl / l_diag + p_zu / u_diag (signs of src/kernels.jl:157-158)
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (st->nlb) LAUNCH(k25_reduce_kernel, st->nlb, *st, w);
        if (st->nub) LAUNCH(k25_reduce_ub_kernel, st->nub, *st, w);
    } else if ((parts & KKT_HEAD) && (r = madqp_reduce_rhs(ctx, st, w))) {
        return r;
    }
    return k->mode == KKT_NORMAL      ? kkt_normal_before(k, st, w, w + st->n, wk, parts)
           : k->mode == KKT_AUGMENTED ? ((parts & KKT_HEAD) ? kkt_augmented_before(k, st, w, w + st->n, wk) : MADQP_OK)
                                      : kkt_condensed_before(k, st, w, w + st->n, wk, parts);
}
// after it: the second half of the middle and finish_aug_solve!
static int32_t kkt_solve_after(madqp_kkt* k, const madqp_state* st, double* w, const KktWork& wk, int parts = KKT_ALL) {
    madqp_ctx* ctx = k->ctx;
    const int32_t r = k->mode == KKT_NORMAL      ? kkt_normal_after(k, st, w, w + st->n, wk, parts)
                      : k->mode == KKT_AUGMENTED ? ((parts & KKT_TAIL) ? kkt_augmented_after(k, st, w, w + st->n, wk) : MADQP_OK)
                                                 : kkt_condensed_after(k, st, w, w + st->n, wk, parts);
    if (r || !(parts & KKT_TAIL)) return r;
    if (k->scaled) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (std::max(st->nlb, st->nub) > 0) LAUNCH(k25_finish_kernel, std::max(st->nlb, st->nub), *st, w);
        return MADQP_OK;
    }
    return madqp_finish_aug_solve(ctx, st, w);
}

static int32_t kkt_solve_once(madqp_kkt* k, const madqp_state* st, double* w) {
    int32_t r = 0;
    k->u_is_A_of = nullptr;
    const KktWork wk = kkt_own_work(k);
    if ((r = kkt_solve_before(k, st, w, wk))) return r;
    if ((r = madqp_chol_solve(k->chol, kkt_factor_rhs(k, st, w, wk)))) return r;
    if ((r = kkt_solve_after(k, st, w, wk))) return r;
    if (!k->scaled && k->mode == KKT_CONDENSED && k->m) k->u_is_A_of = w;  // dx is final since the sweeps: u = A dx (madqp_kkt_mul_solved)
    return MADQP_OK;
}

// ---- many right-hand sides (madqp_kkt_solve_many) ------------------------------------------------------------------------
// The same three stages with the middle one shared: stage 1 for every column, ONE madqp_chol_solve_many on the column-major
// matrix that the columns' factor right-hand sides form where they stand (dy / dx inside W with leading dimension ldw; the
// augmented form's b vectors in a block of their own), stage 3 for every column.  The per-column passes are the kernels of
// the one-vector solve launched on offset pointers.  The products with A / A' are mat-vecs per column too, unless
// madqp_kkt_set_block_products is on: then the product of each stage runs once on the block of all columns
// (apply_A_many / apply_At_many) between the heads and the tails of the columns' stage.
// column c of the work blocks: [t | u | tn | b], each a block of nrhs columns at a stride of whole 256 bytes
static int64_t kkt_pad32(int64_t v) { return (v + 31) / 32 * 32; }
// the stride of the augmented form's b block: the order of the factorised matrix (kkt_form.inc), padded
static int64_t kkt_many_sb(const madqp_kkt* k) {
    return k->mode == KKT_AUGMENTED ? kkt_pad32(kkt_orders(k->mode, k->nx, k->m).stored_order) : 0;
}
static KktWork kkt_many_work(const madqp_kkt* k, const madqp_state* st, int64_t nrhs, int64_t c) {
    const int64_t sm = kkt_pad32(k->m), sn = k->mode == KKT_NORMAL ? kkt_pad32(st->n) : 0;
    const int64_t sb = kkt_many_sb(k);
    double* t = k->many;
    double* u = t + nrhs * sm;
    double* tn = u + nrhs * sm;
    double* b = tn + nrhs * sn;
    return KktWork{t + c * sm, u + c * sm, tn + c * sn, b + c * sb};
}
static int32_t kkt_solve_many_once(madqp_kkt* k, const madqp_state* st, double* W, int64_t ldw, int64_t nrhs) {
    int32_t r = 0;
    const int64_t per = 2 * kkt_pad32(k->m) + (k->mode == KKT_NORMAL ? kkt_pad32(st->n) : 0) + kkt_many_sb(k);
    if ((r = k->mem.grow(&k->many, &k->many_cap, nrhs * per, "madqp_kkt_solve_many: work vectors of the columns"))) return r;
    k->u_is_A_of = nullptr;
    // a stage of every column: whole per column, or heads, ONE product on the block, tails (the operands of the columns'
    // products sit at one stride each: ldw inside W, the strides of the work blocks)
    const KktWork w0 = kkt_many_work(k, st, nrhs, 0), w1 = kkt_many_work(k, st, nrhs, 1);
    auto stage = [&](bool before) -> int32_t {
        auto run = [&](int64_t c, int parts) {
            return before ? kkt_solve_before(k, st, W + c * ldw, kkt_many_work(k, st, nrhs, c), parts)
                          : kkt_solve_after(k, st, W + c * ldw, kkt_many_work(k, st, nrhs, c), parts);
        };
        const KktProduct p0 = before ? kkt_before_product(k, st, W, w0) : kkt_after_product(k, st, W, w0);
        const KktProduct p1 = before ? kkt_before_product(k, st, W + ldw, w1) : kkt_after_product(k, st, W + ldw, w1);
        int32_t rr = 0;
        if (!k->block || !p0.op) {
            for (int64_t c = 0; c < nrhs; ++c)
                if ((rr = run(c, KKT_ALL))) return rr;
            return MADQP_OK;
        }
        for (int64_t c = 0; c < nrhs; ++c)
            if ((rr = run(c, KKT_HEAD))) return rr;
        const int64_t ldx = p1.x - p0.x, ldy = p1.y - p0.y;
        if ((rr = p0.op == 1 ? apply_A_many(k, 1.0, p0.x, ldx, p0.beta, p0.y, ldy, nrhs)
                             : apply_At_many(k, 1.0, p0.x, ldx, p0.beta, p0.y, ldy, nrhs)))
            return rr;
        for (int64_t c = 0; c < nrhs; ++c)
            if ((rr = run(c, KKT_TAIL))) return rr;
        return MADQP_OK;
    };
    if ((r = stage(true))) return r;
    const int64_t ldb = k->mode == KKT_AUGMENTED ? kkt_many_sb(k) : ldw;
    if ((r = madqp_chol_solve_many(k->chol, kkt_factor_rhs(k, st, W, w0), ldb, nrhs))) return r;
    return stage(false);
}

extern "C" int32_t madqp_kkt_solve_many(madqp_kkt* k, const madqp_state* st, double* W, int64_t ldw, int64_t nrhs) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    if ((r = kkt_storage_ready(k, "madqp_kkt_solve_many"))) return r;
    madqp_ctx* ctx = k->ctx;
    const int64_t len = st->n + st->m + st->nlb + st->nub;
    ARG_TRY(ctx, nrhs >= 0 && (W != nullptr || nrhs == 0) && ldw >= len);
    if (nrhs == 0) return MADQP_OK;
    if (nrhs == 1) return madqp_kkt_solve(k, st, W);
    if (k->refine <= 0) return kkt_solve_many_once(k, st, W, ldw, nrhs);
    // refinement as in madqp_kkt_solve, the residuals per column, the corrections through one solve of the residual block
    const int64_t stride = kkt_pad32(len);
    if ((r = k->mem.grow(&k->rf, &k->rf_cap, 2 * nrhs * stride, "madqp_kkt_solve_many: work vectors of the refinement steps"))) return r;
    double *rf_p = k->rf, *rf_r = k->rf + nrhs * stride;
    for (int64_t c = 0; c < nrhs; ++c)
        if ((r = madqp_copy(ctx, len, W + c * ldw, rf_p + c * stride))) return r;  // p
    if ((r = kkt_solve_many_once(k, st, W, ldw, nrhs))) return r;                  // w = K^-1 p
    for (int32_t it = 0; it < k->refine; ++it) {
        for (int64_t c = 0; c < nrhs; ++c) {
            if ((r = madqp_copy(ctx, len, rf_p + c * stride, rf_r + c * stride))) return r;
            if (!k->block && (r = madqp_kkt_mul(k, st, rf_r + c * stride, W + c * ldw, -1.0, 1.0))) return r;  // r = p - K w
        }
        if (k->block && (r = madqp_kkt_mul_many(k, st, rf_r, stride, W, ldw, nrhs, -1.0, 1.0))) return r;  // R = P - K W
        if ((r = kkt_solve_many_once(k, st, rf_r, stride, nrhs))) return r;
        for (int64_t c = 0; c < nrhs; ++c)
            if ((r = madqp_axpy(ctx, len, 1.0, rf_r + c * stride, W + c * ldw))) return r;  // w += K^-1 r
    }
    k->u_is_A_of = nullptr;
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_jtprod(madqp_kkt* k, double* out, const double* y) {
    if (!k) return MADQP_ERR_ARG;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, (out || k->nx + k->ns == 0) && (y || k->m == 0));  // no constraints: y is empty
    int32_t r;
    if ((r = apply_At(k, 1.0, y, 0.0, out))) return r;
    if (k->ns) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(jt_slack_kernel, k->ns, k->ns, k->d_ind_ineq, y, out + k->nx, 1.0, 0.0);
    }
    return MADQP_OK;
}

static int32_t kkt_mul_impl(madqp_kkt* k, const madqp_state* st, double* w, const double* v, double alpha, double beta,
                            bool v_is_last_solution);
static int32_t kkt_mul_tail(madqp_kkt* k, const madqp_state* st, double* w, const double* v, double alpha, double beta,
                            const double* u);
extern "C" int32_t madqp_kkt_mul(madqp_kkt* k, const madqp_state* st, double* w, const double* v,
                                 double alpha, double beta) {
    return kkt_mul_impl(k, st, w, v, alpha, beta, false);
}
extern "C" int32_t madqp_kkt_mul_solved(madqp_kkt* k, const madqp_state* st, double* w, const double* v,
                                        double alpha, double beta) {
    return kkt_mul_impl(k, st, w, v, alpha, beta, true);
}
static int32_t kkt_mul_impl(madqp_kkt* k, const madqp_state* st, double* w, const double* v, double alpha, double beta,
                            bool v_is_last_solution) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, w && v);
    const int64_t n = st->n;
    const bool have_Av = v_is_last_solution && k->m && k->u_is_A_of == v;  // the solve's own A dx, same kernel and operands
    k->u_is_A_of = nullptr;
    // wx = alpha A_full' vy + beta wx  (+ alpha H vx)
    if ((r = apply_At(k, alpha, v + n, beta, w))) return r;
    if ((r = apply_H(k, alpha, v, 1.0, w))) return r;
    if (k->m && !have_Av && (r = apply_A(k, 1.0, v, 0.0, k->u))) return r;
    return kkt_mul_tail(k, st, w, v, alpha, beta, k->u);
}
// The per-variable passes of w = alpha K v + beta w behind the three matrix products: w[0 .. nx) holds
// alpha (A' vy + H vx) + beta wx, u = A vx.
static int32_t kkt_mul_tail(madqp_kkt* k, const madqp_state* st, double* w, const double* v, double alpha, double beta,
                            const double* u) {
    int32_t r = 0;
    madqp_ctx* ctx = k->ctx;
    const int64_t nx = k->nx, n = st->n;
    if (kkt_fusable(k)) {  // the five per-variable passes that follow, in one (resid_tail_kernel)
        if ((r = ensure_pos(k, st))) return r;
        const int64_t L = std::max(std::max(st->n, st->m), std::max(st->nlb, st->nub));
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(resid_tail_kernel, L, *st, w, v, alpha, beta, nx, k->d_slot, k->d_ind_ineq, u, k->pos_lb, k->pos_ub);
        return MADQP_OK;
    }
    if (k->ns) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(jt_slack_kernel, k->ns, k->ns, k->d_ind_ineq, v + n, w + nx, alpha, beta);
    }
    // wy = alpha A_full vx + beta wy
    if (k->m) {
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(mul_rows_kernel, k->m, k->m, k->d_slot, u, v + nx, w + n, alpha, beta);
    }
    if (k->scaled) {  // mul!(w, ::ScaledSparseKKTSystem, v): zl dx + l_diag dzl, zu dx - u_diag dzu
        ProfScope ps(ctx, MADQP_PROF_VEC);
        if (std::max(st->n, st->m) > 0) LAUNCH(k25_kktmul_diag_kernel, std::max(st->n, st->m), *st, w, v, alpha);
        if (st->nlb) LAUNCH(k25_kktmul_lb_kernel, st->nlb, *st, w, v, alpha, beta);
        if (st->nub) LAUNCH(k25_kktmul_ub_kernel, st->nub, *st, w, v, alpha, beta);
        return MADQP_OK;
    }
    return madqp_kktmul(ctx, st, w, v, alpha, beta);
}

// mul! for nrhs pairs of columns: the three matrix products once on the block (apply_*_many), the per-variable tail per
// column on offset pointers.  The A V block is the object's (k->mu, a column per 256-byte stride).
extern "C" int32_t madqp_kkt_mul_many(madqp_kkt* k, const madqp_state* st, double* W, int64_t ldw, const double* V, int64_t ldv,
                                      int64_t nrhs, double alpha, double beta) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    madqp_ctx* ctx = k->ctx;
    const int64_t len = st->n + st->m + st->nlb + st->nub, n = st->n;
    ARG_TRY(ctx, nrhs >= 0 && ldw >= len && ldv >= len);
    if (nrhs == 0) return MADQP_OK;
    ARG_TRY(ctx, W && V && W != V);
    if (nrhs == 1) return madqp_kkt_mul(k, st, W, V, alpha, beta);
    const int64_t sm = kkt_pad32(k->m);
    if ((r = k->mem.grow(&k->mu, &k->mu_cap, nrhs * sm, "madqp_kkt_mul_many: the A V block"))) return r;
    k->u_is_A_of = nullptr;
    if ((r = apply_At_many(k, alpha, V + n, ldv, beta, W, ldw, nrhs))) return r;
    if ((r = apply_H_many(k, alpha, V, ldv, 1.0, W, ldw, nrhs))) return r;
    if (k->m && (r = apply_A_many(k, 1.0, V, ldv, 0.0, k->mu, sm, nrhs))) return r;
    for (int64_t c = 0; c < nrhs; ++c)
        if ((r = kkt_mul_tail(k, st, W + c * ldw, V + c * ldv, alpha, beta, k->mu + c * sm))) return r;
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_set_block_products(madqp_kkt* k, int32_t on) {
    if (!k) return MADQP_ERR_ARG;
    ARG_TRY(k->ctx, on == 0 || on == 1);
    k->block = on != 0;
    return MADQP_OK;
}

// what madqp_kkt_solve_many of nrhs columns would run as (include/madqp.h)
extern "C" int32_t madqp_kkt_many_info(madqp_kkt* k, int64_t nrhs, int64_t* out_host) {
    if (!k) return MADQP_ERR_ARG;
    ARG_TRY(k->ctx, out_host && nrhs >= 0);
    const bool block = k->block && nrhs >= 2;
    const int64_t stage_products = (k->mode == KKT_NORMAL || (k->mode == KKT_CONDENSED && k->m)) ? 2 : 0;  // one per stage
    const int64_t mul_products = 1 + (k->m ? 1 : 0);                                                        // A' and A of a residual
    const int64_t steps = std::max<int32_t>(k->refine, 0);
    out_host[0] = block ? 1 : 0;
    out_host[1] = (stage_products + steps * mul_products) * kkt_passes(nrhs, block, k->a.ptr != nullptr);
    out_host[2] = !kkt_has_H(k) ? 0 : steps * (k->hdiag ? nrhs : kkt_passes(nrhs, block, k->h.ptr != nullptr));
    out_host[3] = k->many_cap + k->rf_cap + k->mw_cap + k->mu_cap;
    return MADQP_OK;
}

// objective pieces into 2 slots (q'x and x'Hx; obj = c0 + s0 + s1/2), gradient and constraint values into st
int32_t madqp_q_kkt_eval(madqp_kkt* k, const madqp_state* st, const double* q, const double* rhs, int slot0) {
    int32_t r = check_kkt_state(k, st);
    if (r) return r;
    madqp_ctx* ctx = k->ctx;
    ARG_TRY(ctx, (k->nx == 0 || q) && (k->m == 0 || rhs));
    const int64_t nx = k->nx, n = st->n;
    if ((r = apply_H(k, 1.0, st->x, 0.0, st->f))) return r;
    if (n) {
        const int nb = grid_for(n);
        {
            ProfScope ps(ctx, MADQP_PROF_VEC);
            hipLaunchKernelGGL(eval_grad_kernel, dim3(nb), dim3(TPB), 0, ctx->stream, n, nx, kkt_has_H(k) ? 1 : 0, q, st->x,
                               st->f, ctx->d_part);
            LAUNCH_CHECK(ctx);
            hipLaunchKernelGGL(sum2_final_kernel, dim3(1), dim3(TPB), 0, ctx->stream, ctx->d_part, nb,
                               ctx->d_res + slot0);
            LAUNCH_CHECK(ctx);
        }
    } else {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_res + slot0, 0, 2 * sizeof(double), ctx->stream));
    }
    if (k->m) {
        if ((r = apply_A(k, 1.0, st->x, 0.0, st->c))) return r;
        ProfScope ps(ctx, MADQP_PROF_VEC);
        LAUNCH(eval_cons_kernel, k->m, k->m, k->d_slot, st->x + nx, rhs, st->c);
    }
    return MADQP_OK;
}

extern "C" int32_t madqp_kkt_eval(madqp_kkt* k, const madqp_state* st, const double* q,
                                  const double* rhs, double c0, double* obj_host) {
    if (!k) return MADQP_ERR_ARG;
    ARG_TRY(k->ctx, obj_host != nullptr);
    int32_t r = madqp_q_kkt_eval(k, st, q, rhs, 0);
    if (r) return r;
    double sums[2] = {0.0, 0.0};
    if ((r = madqp_read_results(k->ctx, 2, sums))) return r;
    *obj_host = mpc_objective(c0, sums[0], sums[1]);
    return MADQP_OK;
}

madqp_ctx* madqp_kkt_ctx(madqp_kkt* kkt) { return kkt->ctx; }

extern "C" int32_t madqp_kkt_matrix(madqp_kkt* k, double** K, int64_t* ld) {
    if (!k || !K || !ld) return MADQP_ERR_ARG;
    if (int32_t r = kkt_storage_ready(k, "madqp_kkt_matrix")) return r;
    *K = k->K;
    *ld = k->ldk;
    return MADQP_OK;
}

// [0] packed 0 / 1, [1] the leading dimension of K (0: a packed object whose bandwidth is not set), [2] doubles allocated
extern "C" int32_t madqp_kkt_storage(madqp_kkt* k, int64_t* out_host) {
    if (!k || !out_host) return MADQP_ERR_ARG;
    out_host[0] = k->packed ? 1 : 0;
    out_host[1] = k->ldk;
    out_host[2] = k->K ? k->k_doubles : 0;
    return MADQP_OK;
}

// Packed band storage -> the lower triangle of a dense column-major matrix, for hosts that want to look at K: entry (i, j),
// i >= j, becomes P[i + j ld] where i - j <= reach and 0 beyond; the upper triangle of D is left alone.  One thread per
// row of a column (coalesced along the column), columns in a grid-stride loop.
namespace {
__global__ __launch_bounds__(256) void band_expand_kernel(int64_t n, const double* __restrict__ P, int64_t ld, int64_t reach,
                                                          double* __restrict__ D, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int64_t j = blockIdx.y; j <= i; j += gridDim.y) D[i + j * ldd] = (i - j <= reach) ? P[i + j * ld] : 0.0;
}
}  // namespace
extern "C" int32_t madqp_band_expand(madqp_ctx* ctx, int64_t n, const double* P, int64_t ld, int64_t reach, double* D,
                                     int64_t ldd) {
    if (!ctx) return MADQP_ERR_ARG;
    ARG_TRY(ctx, n >= 0 && reach >= 0 && ld >= 1 && reach <= ld && (n == 0 || (P && D && ldd >= n)));
    if (n == 0) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_VEC);
    hipLaunchKernelGGL(band_expand_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(n, 4096)), dim3(256), 0,
                       ctx->stream, n, P, ld, reach, D, ldd);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}
