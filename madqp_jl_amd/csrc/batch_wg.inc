// Workgroup programs of batch.hip for TPB threads per problem (included once per TPB and WG_SHARED; needs TPB, WGNS, WG_SHARED).
// WG_SHARED 1: the programs of a batch that shares H / A (madqp_batch_share_matrices) -- prob_of takes the strides from BQ,
// and every entry of H is multiplied by the problem's factor as it is loaded (MS below).  WG_SHARED 0: none of that.
namespace WGNS {
namespace wg {
#define MQ_KERNEL __device__ __forceinline__ void
#define MQ_BLOCK 0
#define GRID_STRIDE(i, len) for (int64_t i = threadIdx.x; i < (len); i += TPB)
#include "vec_kernels.inc"
#include "kkt_kernels.inc"
#undef MQ_KERNEL
#undef MQ_BLOCK
#undef GRID_STRIDE
}  // namespace wg

constexpr int LDS_DOUBLES = 2 * NB + TPB;  // vs | xs | partial sums of the block products / column sums

#ifndef WG_SYNC
#define WG_SYNC() __syncthreads()
#endif
#ifndef BSTAMP
#ifdef MADQP_BATCH_STAMPS  // diagnostic build only: phase times of problem 0 (10 ns ticks), tools/batch_stamps.py
#define BSTAMP(slot)                                                             \
    do {                                                                         \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                               \
            const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();      \
            madqp_batch_stamps[slot] += t_ - madqp_batch_stamps[31];             \
            madqp_batch_stamps[31] = t_;                                         \
        }                                                                        \
    } while (0)
#else
#define BSTAMP(slot)
#endif
#endif

// ---- workgroup-level dense helpers (one problem: matrices of a few MB, vectors of a few KB) ----
// y(rows) = alpha * M x + beta * y,  M row-major rows x cols (row k contiguous): a wave per row
__device__ __forceinline__ void wg_gemv_n(int64_t rows, int64_t cols, double alpha, const double* __restrict__ M,
                          const double* __restrict__ x, double beta, double* __restrict__ y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // R rows x JU column chunks per wave pass: R * JU independent loads in flight per lane before the first
    // fma (the matrices live in HBM: one dependent load per step made this product latency bound, 4x slower
    // than wg_gemv_t on the same data -- tools/batch_stamps.py).  Accumulation order per row is still j ascending.
    constexpr int NW = TPB / 64, R = 4, JU = 4;
    for (int64_t k0 = (int64_t)wave * R; k0 < rows; k0 += NW * R) {
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        for (int64_t j0 = lane; j0 < cols; j0 += 64 * JU) {
            double mv[R][JU], xv[JU];
#pragma unroll
            for (int u = 0; u < JU; ++u) {
                const int64_t j = j0 + 64 * u;
                xv[u] = (j < cols) ? x[j] : 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) mv[r][u] = (j < cols && k0 + r < rows) ? M[(k0 + r) * cols + j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < JU; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (j0 + 64 * u < cols && k0 + r < rows) acc[r] += mv[r][u] * xv[u];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double a = acc[r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
            if (lane == 0 && k0 + r < rows) y[k0 + r] = (beta == 0.0) ? alpha * a : alpha * a + beta * y[k0 + r];
        }
    }
}
// u(rows) = M x as wg_gemv_n forms it (alpha = 1, beta = 0: the same sums in the same order), then -- from the SAME
// registers -- at(cols) = M' dy with dy_i = theta_i (u_i - t_i), the value decondense_kernel gives dy: the condensed solve's
// A dx and the A' dy of the residual check behind it in ONE pass over A (1 of the ~5 MB a solve_system! reads at
// (512, 256)).  A wave keeps its R rows in registers (cols <= 64 CH); the waves' column sums meet in LDS in wave order.
// tot: cols doubles of LDS.
template <int CH>
__device__ __forceinline__ void wg_gemv_n_then_t(int64_t rows, int64_t cols, const double* __restrict__ M,
                                                 const double* __restrict__ x, const double* __restrict__ theta,
                                                 const double* __restrict__ t, double* __restrict__ u,
                                                 double* __restrict__ at, double* tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = TPB / 64;  // a row per step and wave, the next two rows already on their way (the rows come from HBM:
    // a step that waits for its own loads runs at one memory latency per step) -- and no more registers than that: the
    // program must stay under 128 so that two workgroups share a compute unit
    double col[CH], xv[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        col[c] = 0.0;
        xv[c] = (lane + 64 * c < cols) ? x[lane + 64 * c] : 0.0;
    }
    double cur[CH], n1[CH], n2[CH];
    auto fetch = [&](int64_t k, double (&dst)[CH]) {
#pragma unroll
        for (int c = 0; c < CH; ++c) dst[c] = (lane + 64 * c < cols && k < rows) ? M[k * cols + lane + 64 * c] : 0.0;
    };
    fetch(wave, cur);
    fetch(wave + NW, n1);
    for (int64_t k = wave; k < rows; k += NW) {
        fetch(k + 2 * NW, n2);  // (beyond the last row: zeros, no loads)
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (lane + 64 * c < cols) a += cur[c] * xv[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
        a = __shfl(a, 0, 64);
        if (lane == 0) u[k] = a;
        const double dy = theta[k] * (a - t[k]);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            col[c] += cur[c] * dy;
            cur[c] = n1[c];
            n1[c] = n2[c];
        }
    }
    for (int64_t j = threadIdx.x; j < cols; j += TPB) tot[j] = 0.0;
    WG_SYNC();
    for (int w = 0; w < NW; ++w) {
        if (wave == w) {
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (lane + 64 * c < cols) tot[lane + 64 * c] += col[c];
        }
        WG_SYNC();
    }
    for (int64_t j = threadIdx.x; j < cols; j += TPB) at[j] = tot[j];
    WG_SYNC();
}
// out(cols) = alpha * M' v + beta * out,  M row-major rows x cols: a thread per column; when the workgroup
// is wider than the matrix, G thread groups split the rows and their partial sums meet in LDS (scr: TPB doubles)
// raw (optional): the unscaled product M' v itself (what the incremental model evaluation keeps of the residual check)
// MS: the matrix is ms * M, each entry rounded as it is loaded (a shared H under the problem's own scale)
template <bool MS = false>
__device__ __forceinline__ void wg_gemv_t(int64_t rows, int64_t cols, double alpha, const double* __restrict__ M,
                          const double* __restrict__ v, double beta, double* __restrict__ out, double* scr,
                          double* __restrict__ raw = nullptr, double ms = 1.0) {
    auto ld = [&](int64_t idx) { return MS ? ms * M[idx] : M[idx]; };
    const int64_t cpad = (cols + 63) / 64 * 64;
    const int G = (cpad < TPB) ? (int)(TPB / cpad) : 1;
    if (G == 1) {
        for (int64_t j = threadIdx.x; j < cols; j += TPB) {
            double a[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) a[r] = 0.0;
            int64_t k = 0;
            for (; k + 16 <= rows; k += 16) {  // 16 independent loads in flight per thread, 8 accumulation chains as before
                double mv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) mv[r] = ld((k + r) * cols + j);
#pragma unroll
                for (int r = 0; r < 8; ++r) a[r] += mv[r] * v[k + r];
#pragma unroll
                for (int r = 0; r < 8; ++r) a[r] += mv[8 + r] * v[k + 8 + r];
            }
            for (; k + 8 <= rows; k += 8) {
#pragma unroll
                for (int r = 0; r < 8; ++r) a[r] += ld((k + r) * cols + j) * v[k + r];
            }
            for (; k < rows; ++k) a[0] += ld(k * cols + j) * v[k];
            const double acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
            out[j] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * out[j];
            if (raw) raw[j] = acc;
        }
        return;
    }
    const int64_t j = threadIdx.x % cpad;
    const int g = (int)(threadIdx.x / cpad);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (g < G && j < cols) {
        int64_t k = g;
        for (; k + 3 * G < rows; k += 4 * G) {
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] += ld((k + r * G) * cols + j) * v[k + r * G];
        }
        for (; k < rows; k += G) a[0] += ld(k * cols + j) * v[k];
    }
    WG_SYNC();
    if (g < G) scr[g * cpad + j] = (a[0] + a[1]) + (a[2] + a[3]);
    WG_SYNC();
    if (threadIdx.x < cols) {
        double acc = scr[threadIdx.x];
        for (int q = 1; q < G; ++q) acc += scr[q * cpad + threadIdx.x];
        out[threadIdx.x] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * out[threadIdx.x];
        if (raw) raw[threadIdx.x] = acc;
    }
    WG_SYNC();
}
// y(n) = alpha * H x + beta * y for a SYMMETRIC H (row-major n x n, n <= SYM_MAX) from its lower triangle alone: half
// the bytes of wg_gemv_t on the full matrix (the three H passes were 6 of the 29 MB a problem-iteration moves at
// (512, 256), and the workgroup programs are HBM bound).  A wave per group of R rows: entry H[k][j], j <= k, feeds the
// row sum of k (wave reduction) and, for j < k, the column sum of j, which every lane keeps for its own columns
// (lane + 64 u) over all rows of its wave; the waves' column sums meet in `sym` (global scratch of this problem:
// SYM_DOUBLES; the workgroup reads back what it wrote itself) and are added in wave order: nothing depends on timing.
constexpr int SYM_CH = 8, SYM_MAX = 64 * SYM_CH;
constexpr int SYM_DOUBLES = (TPB / 64 + 1) * SYM_MAX;
static_assert(SYM_MAX == 512 && SYM_DOUBLES <= (512 / 64 + 1) * 512, "batch.hip sizes the scratch for nx <= 512, 8 waves");

// MS: the matrix is hs * H, each entry rounded as it is loaded
template <bool MS = false>
__device__ __forceinline__ void wg_symv_lower(int64_t n, double alpha, const double* __restrict__ H,
                                              const double* __restrict__ x, double beta, double* __restrict__ y,
                                              double* __restrict__ sym, double* __restrict__ raw = nullptr, double hs = 1.0) {
    constexpr int NW = TPB / 64, R = 4, UP = 2;  // R x UP loads in flight per lane (registers: the kernel keeps 4 waves per SIMD)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double col[SYM_CH];
#pragma unroll
    for (int u = 0; u < SYM_CH; ++u) col[u] = 0.0;
    double* rows = sym + NW * SYM_MAX;
    for (int64_t k0 = (int64_t)wave * R; k0 < n; k0 += NW * R) {
        double row[R], xk[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            row[r] = 0.0;
            xk[r] = (k0 + r < n) ? x[k0 + r] : 0.0;
        }
        const int64_t klast = (k0 + R - 1 < n) ? k0 + R - 1 : n - 1;
        const int umax = (int)(klast >> 6);  // wave-uniform: last 64-column chunk the group touches
        int ln = lane;
        asm volatile("" : "+v"(ln));  // per-iteration copy: keeps the 8 chunks' addresses and predicates out of loop-invariant registers
        const double* Hr[R];  // (rows and columns clamped into the triangle: every load is valid, none is branched around)
#pragma unroll
        for (int r = 0; r < R; ++r) Hr[r] = H + ((k0 + r < n) ? k0 + r : n - 1) * n;
#pragma unroll
        for (int u0 = 0; u0 < SYM_CH; u0 += UP) {
            if (u0 <= umax) {
                double hv[UP][R], xj[UP];
#pragma unroll
                for (int uu = 0; uu < UP; ++uu) {
                    const int j = ln + 64 * (u0 + uu);
                    xj[uu] = x[(j < n) ? j : (int)n - 1];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int kr = (int)((k0 + r < n) ? k0 + r : n - 1);
                        hv[uu][r] = Hr[r][(j < kr) ? j : kr];
                        if constexpr (MS) hv[uu][r] *= hs;
                    }
                }
#pragma unroll
                for (int uu = 0; uu < UP; ++uu) {
                    const int j = ln + 64 * (u0 + uu);
                    if (j >= n) xj[uu] = 0.0;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (!(k0 + r < n && j <= k0 + r)) hv[uu][r] = 0.0;
                }
#pragma unroll
                for (int uu = 0; uu < UP; ++uu) {
                    const int j = ln + 64 * (u0 + uu);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        row[r] += hv[uu][r] * xj[uu];
                        col[u0 + uu] += (j == k0 + r) ? 0.0 : hv[uu][r] * xk[r];
                    }
                }
            }
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double a = row[r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
            if (lane == 0 && k0 + r < n) rows[k0 + r] = a;
        }
    }
#pragma unroll
    for (int u = 0; u < SYM_CH; ++u) sym[wave * SYM_MAX + 64 * u + lane] = col[u];
    WG_SYNC();
    for (int64_t j = threadIdx.x; j < n; j += TPB) {
        double acc = rows[j];
        for (int w = 0; w < NW; ++w) acc += sym[w * SYM_MAX + j];
        y[j] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * y[j];
        if (raw) raw[j] = acc;
    }
    WG_SYNC();
}
// y(nx) = alpha * H x + beta * y with whichever form applies
__device__ __forceinline__ void wg_hmul(const BQ& q, const Prob& pb, double alpha, const double* x, double beta, double* y,
                                        double* scr, double* raw = nullptr) {
    if (pb.sym)
        wg_symv_lower<WG_SHARED != 0>(q.nx, alpha, pb.H, x, beta, y, pb.sym, raw, pb.hs);
    else
        wg_gemv_t<WG_SHARED != 0>(q.nx, q.nx, alpha, pb.H, x, beta, y, scr, raw, pb.hs);
}
// xs(128, LDS) = img * vs,  img: 128 x 128, fast index = output (the Wcm / Wrm images of chol.hip);
// part: TPB doubles
// LOWER: the image is lower triangular (entry (i, c) = 0 for i < c: the forward image), else upper triangular (the backward
// image): the zero half is not fetched -- a 128-byte line of 16 rows that lies wholly in it is never requested, 44 % of
// the image (the images were 40 % of what the sweeps of a 512 x 512 problem read).  Adding the zeros changed no sum.
template <bool LOWER>
__device__ __forceinline__ void wg_block_matvec(const double* __restrict__ img, const double* vs, double* part, double* xs) {
    constexpr int H = TPB / NB, CW = NB / H;  // H column groups of CW columns
    const int i = threadIdx.x & (NB - 1), h = threadIdx.x >> 7;
    double acc = 0.0;
#pragma unroll 8
    for (int c = h * CW; c < h * CW + CW; ++c) {
        const double v = (LOWER ? i >= c : i <= c) ? img[i + c * NB] : 0.0;
        acc += v * vs[c];
    }
    part[h * NB + i] = acc;
    WG_SYNC();
    if (threadIdx.x < NB) {
        double sum = part[i];
#pragma unroll
        for (int q = 1; q < H; ++q) sum += part[q * NB + i];
        xs[i] = sum;
    }
    WG_SYNC();
}
// rhs(n) <- (L L')^-1 rhs with the inverse diagonal blocks of potf2_inv_kernel; tmp: n doubles
__device__ __forceinline__ void wg_chol_solve(const double* __restrict__ L, int64_t lda, const double* __restrict__ winv,
                              int64_t n, double* rhs, double* tmp, double* lds /* LDS_DOUBLES */) {
    double *vs = lds, *xs = lds + NB, *part = lds + 2 * NB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // forward: L y = b (b updated in place below the block, y collected in tmp)
    for (int64_t jb = 0; jb < n; jb += NB) {
        const int w = (int)((n - jb < NB) ? (n - jb) : NB);
        if (threadIdx.x < NB) vs[threadIdx.x] = (threadIdx.x < w) ? rhs[jb + threadIdx.x] : 0.0;
        WG_SYNC();
        wg_block_matvec<true>(winv + (jb / NB) * WBLK, vs, part, xs);
        if (threadIdx.x < w) tmp[jb + threadIdx.x] = xs[threadIdx.x];
        for (int64_t row = jb + w + threadIdx.x; row < n; row += TPB) {
            const double* Lp = L + row + jb * lda;
            double acc = 0.0;
            int c = 0;
            for (; c + 8 <= w; c += 8) {  // 8 loads in flight, accumulated in column order as before
                double lv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) lv[u] = Lp[(int64_t)(c + u) * lda];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += lv[u] * xs[c + u];
            }
            for (; c < w; ++c) acc += Lp[(int64_t)c * lda] * xs[c];
            rhs[row] -= acc;
        }
        WG_SYNC();
    }
    // backward: L' x = y (y = tmp updated in place left of the block, x written to rhs)
    const int64_t last = ((n - 1) / NB) * NB;
    for (int64_t jb = last; jb >= 0; jb -= NB) {
        const int w = (int)((n - jb < NB) ? (n - jb) : NB);
        if (threadIdx.x < NB) vs[threadIdx.x] = (threadIdx.x < w) ? tmp[jb + threadIdx.x] : 0.0;
        WG_SYNC();
        wg_block_matvec<false>(winv + (jb / NB) * WBLK + NB * NB, vs, part, xs);
        if (threadIdx.x < w) rhs[jb + threadIdx.x] = xs[threadIdx.x];
        // a wave per column left of the block, 8 columns per step (16 loads in flight per lane)
        constexpr int CU = 8;
        for (int64_t c0 = wave; c0 < jb; c0 += CU * (TPB / 64)) {
            double lv[CU][2], acc[CU];
            int ln = lane;
            asm volatile("" : "+v"(ln));
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const int64_t c = c0 + (int64_t)u * (TPB / 64);
                const double* Lp = L + jb + c * lda;
                lv[u][0] = (c < jb && ln < w) ? Lp[ln] : 0.0;
                lv[u][1] = (c < jb && ln + 64 < w) ? Lp[ln + 64] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                acc[u] = 0.0;
                if (lane < w) acc[u] += lv[u][0] * xs[lane];
                if (lane + 64 < w) acc[u] += lv[u][1] * xs[lane + 64];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) acc[u] += __shfl_down(acc[u], off, 64);
                const int64_t c = c0 + (int64_t)u * (TPB / 64);
                if (lane == 0 && c < jb) tmp[c] -= acc[u];
            }
        }
        WG_SYNC();
    }
}

__device__ __forceinline__ void wg_copy(int64_t len, const double* __restrict__ src, double* __restrict__ dst) {
    for (int64_t i = threadIdx.x; i < len; i += TPB) dst[i] = src[i];
}

// MadNLP.jtprod!(out, kkt, y): out = [A' y ; -y[ind_ineq]]   (src/KKT/normalkkt.jl:162-164)
__device__ __forceinline__ void wg_jtprod(const BQ& q, const Prob& pb, const double* y, double* out, double* scr) {
    wg_gemv_t(q.m, q.nx, 1.0, pb.A, y, 0.0, out, scr);
    wg::jt_slack_kernel(pb.ns, pb.ind_ineq, y, out + q.nx, 1.0, 0.0);
    WG_SYNC();
}

// MadNLP.solve!(kkt, w), condensed form (kkt.hip: madqp_kkt_solve)
// NT: the program may form A' dy beside A dx (wg_gemv_n_then_t: registers the Gondzio and start-point programs do not have)
template <bool NT = false>
__device__ __forceinline__ void wg_kkt_solve(const BQ& q, const madqp_state& s, const Prob& pb, double* w, double* lds) {
    double* wx = w;
    double* wy = w + s.n;
    if (s.nlb) wg::reduce_rhs_kernel(s.nlb, s.ind_lb, w, w + s.n + s.m, s.l_diag);
    WG_SYNC();
    if (s.nub) wg::reduce_rhs_kernel(s.nub, s.ind_ub, w, w + s.n + s.m + s.nlb, s.u_diag);
    WG_SYNC();
    BSTAMP(1);
    if (q.normal) {  // src/KKT/normalkkt.jl:185-201 verbatim: the reference's own NormalKKTSystem (LP)
        wg::div_kernel(s.n, wx, s.pr_diag, pb.tn);  // r1 = Sigma^-1 wx
        WG_SYNC();
        if (q.m) {
            wg_gemv_n(q.m, q.nx, 1.0, pb.A, pb.tn, 0.0, pb.u);
            WG_SYNC();
            wg::normal_rhs_kernel(q.m, pb.slot, pb.u, pb.tn + q.nx, wy, wy);  // A_full r1 - r2
            WG_SYNC();
            wg_chol_solve(pb.K, q.ldk, pb.winv, q.m, wy, pb.tmp, lds);  // dy
            wg_gemv_t(q.m, q.nx, 1.0, pb.A, wy, 0.0, pb.tn, lds + 2 * NB);  // A_full' dy
            if (pb.ns) wg::jt_slack_kernel(pb.ns, pb.ind_ineq, wy, pb.tn + q.nx, 1.0, 0.0);
            WG_SYNC();
        } else {
            for (int64_t i = threadIdx.x; i < s.n; i += TPB) pb.tn[i] = 0.0;
            WG_SYNC();
        }
        wg::normal_back_kernel(s.n, pb.tn, s.pr_diag, wx);  // Sigma^-1 (r1 - A' dy)
        WG_SYNC();
        if (s.nlb || s.nub) wg::finish_aug_solve_kernel(s, w);
        WG_SYNC();
        return;
    }
    if (q.m) {
        wg::condense_kernel(q.m, q.nx, pb.slot, s.pr_diag, pb.theta, wx, wy, pb.t, pb.u);
        WG_SYNC();
        wg_gemv_t(q.m, q.nx, 1.0, pb.A, pb.u, 1.0, wx, lds + 2 * NB);
        WG_SYNC();
    }
    BSTAMP(2);
    wg_chol_solve(pb.K, q.ldk, pb.winv, q.nx, wx, pb.tmp, lds);
    BSTAMP(3);
    if (q.m) {
        if (NT && pb.at)
            wg_gemv_n_then_t<8>(q.m, q.nx, pb.A, wx, pb.theta, pb.t, pb.u, pb.at, lds);  // (+ A' dy for the residual check)
        else
            wg_gemv_n(q.m, q.nx, 1.0, pb.A, wx, 0.0, pb.u);
        WG_SYNC();
        BSTAMP(4);
        wg::decondense_kernel(q.m, q.nx, pb.slot, s.pr_diag, pb.theta, pb.t, pb.u, wx, wy);
        WG_SYNC();
    }
    if (s.nlb || s.nub) wg::finish_aug_solve_kernel(s, w);
    WG_SYNC();
    BSTAMP(5);
}

// MadNLP.mul!(w, kkt, v, alpha, beta) (kkt.hip: madqp_kkt_mul + madqp_kktmul)
// have_Av: pb.u already holds A v_x -- the condensed solve that produced v ended with exactly this product
// (wg_solve_system; madqp_kkt_mul_solved on the single-problem path)
// keep: also leave A' v_y and H v_x themselves in pb.raw_at / pb.raw_h (incremental model evaluation)
__device__ __forceinline__ void wg_kkt_mul(const BQ& q, const madqp_state& s, const Prob& pb, double* w, const double* v,
                           double alpha, double beta, double* scr, bool have_Av = false, bool keep = false,
                           bool have_At = false) {
    const int64_t nx = q.nx, n = s.n;
    BSTAMP(0);
    if (have_At) {  // v is the solve's own result: A' v_y was formed beside A v_x (wg_gemv_n_then_t)
        for (int64_t j = threadIdx.x; j < nx; j += TPB) {
            const double acc = pb.at[j];
            w[j] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * w[j];
            if (keep) pb.raw_at[j] = acc;
        }
    } else {
        wg_gemv_t(q.m, nx, alpha, pb.A, v + n, beta, w, scr, keep ? pb.raw_at : nullptr);
    }
    WG_SYNC();
    BSTAMP(6);
    if (pb.H && nx) {
        wg_hmul(q, pb, alpha, v, 1.0, w, scr, keep ? pb.raw_h : nullptr);
        WG_SYNC();
    }
    BSTAMP(7);
    if (pb.ns) wg::jt_slack_kernel(pb.ns, pb.ind_ineq, v + n, w + nx, alpha, beta);
    if (q.m) {
        if (!have_Av) wg_gemv_n(q.m, nx, 1.0, pb.A, v, 0.0, pb.u);
        WG_SYNC();
        BSTAMP(8);
        wg::mul_rows_kernel(q.m, pb.slot, pb.u, v + nx, w + n, alpha, beta);
    }
    WG_SYNC();
    wg::kktmul_diag_kernel(s, w, v, alpha);
    WG_SYNC();
    if (s.nlb) wg::kktmul_lb_kernel(s, w, v, alpha, beta);
    WG_SYNC();
    if (s.nub) wg::kktmul_ub_kernel(s, w, v, alpha, beta);
    WG_SYNC();
    BSTAMP(9);
}

// solve_system! (src/linear_solver.jl:19-45); returns false for MadNLP.SolveException
// REFINE: q.opt.refine_steps (> 0) steps of d += K^-1 (p - K d) with the residual just formed, operation for operation
// MPCSolver.solve_system (solver.py).  A template parameter like GONDZIO: the instantiations without it are the parent's
// programs.  What is kept "of the LAST solve's d" (pb.u = A dx, pb.raw_h = H dx, pb.raw_at = A' dy: wg_eval_model_incr and
// the head of the next iteration consume them) then comes from the mul! of the LAST step, whose operand is the refined d:
// that mul! forms all its products itself (have_Av = have_At = false -- pb.u and pb.at hold products of the correction's
// solve by then), and the earlier ones keep nothing.
template <bool NT = false, bool REFINE = false>
__device__ __forceinline__ bool wg_solve_system(const BQ& q, const madqp_state& s, const Prob& pb, double* lds, double* red,
                                                bool keep = false) {
    wg_copy(pb.ntot, s.p, s.d);
    WG_SYNC();
    wg_kkt_solve<NT>(q, s, pb, s.d, lds);
    wg_copy(pb.ntot, s.p, pb.w1);
    WG_SYNC();
    wg_kkt_mul(q, s, pb, pb.w1, s.d, -1.0, 1.0, lds + 2 * NB, /*have_Av=*/!q.normal && q.m > 0, !REFINE && keep && pb.hx,
               /*have_At=*/NT && pb.at && !q.normal && q.m > 0);
    if constexpr (REFINE) {
        for (int step = 0; step < q.opt.refine_steps; ++step) {
            wg_kkt_solve<false>(q, s, pb, pb.w1, lds);
            wg::axpy_kernel(pb.ntot, 1.0, pb.w1, s.d);
            WG_SYNC();
            wg_copy(pb.ntot, s.p, pb.w1);
            WG_SYNC();
            wg_kkt_mul(q, s, pb, pb.w1, s.d, -1.0, 1.0, lds + 2 * NB, /*have_Av=*/false,
                       keep && pb.hx && step + 1 == q.opt.refine_steps, /*have_At=*/false);
        }
    }
    wg::norm_inf3_kernel(pb.ntot, pb.w1, s.p, s.d, red);
    WG_SYNC();
    const double ratio = mpc_residual_ratio(red);
    WG_SYNC();
    if (threadIdx.x == 0) pb.scal[S_RATIO] = ratio;
    return !mpc_solve_failed(ratio, q.opt.check_residual, q.opt.tol_linear_solve);
}

// callbacks obj / grad! / cons! (kkt.hip: madqp_kkt_eval)
__device__ __forceinline__ double wg_eval_model(const BQ& q, const madqp_state& s, const Prob& pb, double* red, double* scr) {
    BSTAMP(0);
    if (pb.H && q.nx) wg_hmul(q, pb, 1.0, s.x, 0.0, s.f, scr, pb.hx);  // (H x itself is kept for the incremental form)
    WG_SYNC();
    BSTAMP(10);
    wg::eval_grad_kernel(s.n, q.nx, (pb.H && q.nx) ? 1 : 0, pb.qv, s.x, s.f, red);
    WG_SYNC();
    const double obj = mpc_objective(pb.c0, red[0], red[1]);
    WG_SYNC();
    if (q.m) {
        wg_gemv_n(q.m, q.nx, 1.0, pb.A, s.x, 0.0, s.c);
        WG_SYNC();
        wg::eval_cons_kernel(q.m, pb.slot, s.x + q.nx, pb.rhs, s.c);
        WG_SYNC();
    }
    BSTAMP(11);
    return obj;
}

// The same callbacks after a step x += alpha_p dx, from the products the step's last solve_system! left behind instead of
// three more passes over H and A (the workgroup programs are HBM bound: 3 of the 13.4 MB a problem-iteration moves at
// (512, 256)):  H x += alpha_p (H dx)  [the residual check's mul! formed H dx],  c += alpha_p (A dx - ds)  [the condensed
// solve ended with A dx in pb.u], and -- in the next iteration's head -- A' y += alpha_d (A' dy).  Sums and objective as in
// wg_eval_model.  The residuals then carry the rounding of k updates instead of one product: ~k eps of their terms,
// seven orders below the termination tolerance; MADQP_BATCH_INCR=0 evaluates from scratch every iteration.
__device__ __forceinline__ double wg_eval_model_incr(const BQ& q, const madqp_state& s, const Prob& pb, double alpha_p,
                                                     double* red) {
    const bool has_h = pb.H && q.nx;
    if (has_h) {
        for (int64_t j = threadIdx.x; j < q.nx; j += TPB) {
            const double h = pb.hx[j] + alpha_p * pb.raw_h[j];
            pb.hx[j] = h;
            s.f[j] = h;
        }
    }
    WG_SYNC();
    wg::eval_grad_kernel(s.n, q.nx, has_h ? 1 : 0, pb.qv, s.x, s.f, red);
    WG_SYNC();
    const double obj = mpc_objective(pb.c0, red[0], red[1]);
    WG_SYNC();
    for (int64_t i = threadIdx.x; i < q.m; i += TPB) {
        const int64_t k = pb.slot[i];
        const double ds = k >= 0 ? s.d[q.nx + k] : 0.0;
        s.c[i] += alpha_p * (pb.u[i] - ds);
    }
    WG_SYNC();
    return obj;
}

__device__ __forceinline__ double wg_compl(const madqp_state& s, int affine, double ap, double ad, double* red) {
    if (s.nlb + s.nub == 0) return 0.0;
    wg::compl_kernel(s, affine, ap, ad, nullptr, red);
    WG_SYNC();
    const double v = mpc_compl_mean(red, (double)(s.nlb + s.nub));
    WG_SYNC();
    return v;
}

// the four (value, blocking index) pairs of get_alpha_max_primal / _dual (src/kernels.jl:242-288)
__device__ __forceinline__ void wg_alpha_max(const madqp_state& s, double tau, double* red, double (&a)[4], int64_t (&ib)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = 1.0;
        ib[k] = -1;
    }
    if (s.nlb + s.nub == 0) return;
    wg::alpha_max_kernel(s, tau, red, nullptr);
    WG_SYNC();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (red[2 * k] < 1.0) {  // init = (1.0, 0): alpha <= 1, "nothing blocks" otherwise
            a[k] = red[2 * k];
            ib[k] = (int64_t)red[2 * k + 1];
        }
    WG_SYNC();
}
// get_fraction_to_boundary_step (src/kernels.jl:290-305)
__device__ __forceinline__ MpcSteps wg_fraction_to_boundary(const madqp_state& s, double tau, double* red) {
    double a[4];
    int64_t ib[4];
    wg_alpha_max(s, tau, red, a, ib);
    return {mpc_min(a[0], a[1]), mpc_min(a[2], a[3])};
}

// update_step!(::MehrotraAdaptiveStep) (src/kernels.jl:325-374): element reads at the blocking indices
__device__ __forceinline__ MpcSteps wg_mehrotra_adaptive_step(const madqp_state& s, double gamma_f, double* red) {
    double a[4], row[2][MPC_ROW_LEN] = {};
    int64_t ib[4];
    wg_alpha_max(s, 1.0, red, a, ib);
    const double mean = wg_compl(s, 1, mpc_min(a[0], a[1]), mpc_min(a[2], a[3]), red);
#pragma unroll
    for (int dual = 0; dual < 2; ++dual) {
        const int k = mpc_blocking(a, dual);
        if (k < 0) continue;
        const bool ub = k & 1;
        const int64_t i = ib[k], j = (ub ? s.ind_ub : s.ind_lb)[i];
        double* r = row[dual];
        r[MPC_ROW_X] = s.x[j];
        r[MPC_ROW_BOUND] = (ub ? s.xu : s.xl)[j];
        r[MPC_ROW_Z] = (ub ? s.zu : s.zl)[j];
        r[MPC_ROW_DX] = s.d[j];
        r[MPC_ROW_DZ] = s.d[s.n + s.m + (ub ? s.nlb : 0) + i];
    }
    return mpc_mehrotra_step(a, row[0], row[1], mean, gamma_f);
}

// gondzio_correction_direction! (src/solver.jl:200-251); false for MadNLP.SolveException
template <bool REFINE>
__device__ __forceinline__ bool wg_gondzio(const BQ& q, int64_t b, const madqp_state& s, const Prob& pb,
                                                    double mu_curr, double* lds, double* red) {
    double* w2 = q.w2 + b * q.ntst;
    MpcSteps alpha = wg_fraction_to_boundary(s, MPC_GZ_TAU, red);
    for (int c = 0; c < q.opt.max_ncorr; ++c) {
        const MpcSteps ta = mpc_trial_alpha(alpha);
        const double mu_g = mpc_muc(wg_compl(s, 1, ta.p, ta.d, red), mu_curr);
        wg::extra_correction_kernel(s, ta.p, ta.d, MPC_GZ_BMIN * mu_g, MPC_GZ_BMAX * mu_g, nullptr, nullptr);
        WG_SYNC();
        wg::rhs_kernel(s, 1, mu_g, nullptr);
        wg_copy(pb.ntot, s.d, w2);
        WG_SYNC();
        if (!wg_solve_system<false, REFINE>(q, s, pb, lds, red)) return false;
        const MpcSteps ha = wg_fraction_to_boundary(s, MPC_GZ_TAU, red);
        if (mpc_trial_dropped(ha, alpha)) {
            wg_copy(pb.ntot, w2, s.d);
            WG_SYNC();
            break;
        }
        alpha = ha;
    }
    return true;
}

// Theta and the scaled operand S = sqrt(Theta) A (zero padded to kpad x npad) of build_kkt!
__device__ __forceinline__ void wg_build_operands(const BQ& q, const madqp_state& s, const Prob& pb) {
    if (q.normal) {
        // normal equations A Sigma_x^-1 A' + diag(Sigma_s^-1 on inequality rows) (src/KKT/normalkkt.jl:166-180): the
        // GEMM operand is S[k, i] = sqrt(1/Sigma_k) A[i, k] (variable k major, kpad x npad), theta = the diagonal part
        wg::recip_kernel(s.n, s.pr_diag, pb.tn);
        WG_SYNC();
        if (q.m) wg::slack_diag_kernel(q.m, q.nx, pb.slot, pb.tn, pb.theta);
        for (int64_t k = threadIdx.x; k < q.kpad; k += TPB) {  // a thread per variable: reads coalesced over k
            const double sk = (k < q.nx) ? sqrt(pb.tn[k]) : 0.0;
            for (int64_t i = 0; i < q.npad; ++i)
                pb.S[k * q.npad + i] = (k < q.nx && i < q.m) ? sk * pb.A[i * q.nx + k] : 0.0;
        }
        return;
    }
    if (q.m) wg::theta_kernel(q.m, q.nx, pb.slot, s.pr_diag, s.du_diag, pb.theta);
    WG_SYNC();
    for (int64_t i = threadIdx.x; i < q.npad; i += TPB) {  // a thread per column, 8 rows in flight
        for (int64_t k0 = 0; k0 < q.kpad; k0 += 8) {
            double v[8], wk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t k = k0 + u;
                const bool on = k < q.m && i < q.nx;
                wk[u] = on ? pb.theta[k] : 0.0;
                v[u] = on ? pb.A[k * q.nx + i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < q.kpad) pb.S[(k0 + u) * q.npad + i] = (k0 + u < q.m && i < q.nx) ? v[u] * sqrt(wk[u]) : 0.0;
        }
    }
}

__device__ __forceinline__ void wg_fill(int64_t len, double v, double* dst) {
    for (int64_t i = threadIdx.x; i < len; i += TPB) dst[i] = v;
}

// ---- start: src/solver.jl:162-174 and the first half of init_starting_point! (:6-21) ----------
__global__ __launch_bounds__(TPB) void bq_init_pre_kernel(BQ q) {
    __shared__ double red[32];
    __shared__ double lds[LDS_DOUBLES];
    const int64_t b = blockIdx.x;
    const madqp_state s = state_of(q, b);
    const Prob pb = prob_of<WG_SHARED != 0>(q, b);
    if (threadIdx.x == 0) {
        q.status[b] = MPC_ST_ACTIVE;
        q.iters[b] = 0;
        if (q.trace) q.trace_count[b] = 0;
    }
    // MadNLP.initialize!(kkt) (src/KKT/normalkkt.jl:136-147)
    wg_fill(s.n, 1.0, s.reg);
    wg_fill(s.nlb, 0.0, s.l_lower);
    wg_fill(s.nub, 0.0, s.u_lower);
    wg_fill(s.nlb, 1.0, s.l_diag);
    wg_fill(s.nub, 1.0, s.u_diag);
    wg_fill(s.n, 0.0, s.jacl);
    WG_SYNC();
    // init_regularization! (src/kernels.jl:380-384)
    const MpcReg reg = mpc_init_regularization(q.opt.regularization, q.opt.delta_p, q.opt.delta_d);
    const double obj = wg_eval_model(q, s, pb, red, lds + 2 * NB);  // :166-169
    wg::norm_inf3_kernel(s.m, pb.rhs, nullptr, nullptr, red);
    WG_SYNC();
    const double norm_b = red[0];
    WG_SYNC();
    wg::norm_inf3_kernel(s.n, s.f, nullptr, nullptr, red);
    WG_SYNC();
    const double norm_c = red[0];
    WG_SYNC();
    // init_starting_point! :16-18
    wg_fill(s.n, reg.del_w, s.reg);
    wg_fill(s.n, reg.del_w, s.pr_diag);
    wg_fill(s.m, reg.del_c, s.du_diag);
    WG_SYNC();
    wg_build_operands(q, s, pb);
    if (threadIdx.x == 0) {
        double* sc = pb.scal;
        sc[S_MU] = q.mu_init;
        sc[S_ALPHA_P] = sc[S_ALPHA_D] = 0.0;
        sc[S_OBJ] = obj;
        sc[S_INF_PR] = sc[S_INF_DU] = sc[S_INF_COMPL] = sc[S_DNORM] = 0.0;
        sc[S_NORM_B] = norm_b;
        sc[S_NORM_C] = norm_c;
        sc[S_DEL_W] = reg.del_w;
        sc[S_DEL_C] = reg.del_c;
        sc[S_RATIO] = 0.0;
        sc[S_REG_P] = reg.run_p;
        sc[S_REG_D] = reg.run_d;
        sc[S_NFACT] = 1.0;  // the start-point factorisation (src/solver.jl:21)
    }
}

// ---- second half of init_starting_point! (src/solver.jl:25-123) ---------------------------------
template <bool REFINE>
__global__ __launch_bounds__(TPB) void bq_init_post_kernel(BQ q) {
    __shared__ double red[32];
    __shared__ double lds[LDS_DOUBLES];
    const int64_t b = blockIdx.x;
    const madqp_state s = state_of(q, b);
    const Prob pb = prob_of<WG_SHARED != 0>(q, b);
    int status = MPC_ST_ACTIVE;
    if (q.info[b] != 0) status = MPC_ST_INTERNAL;  // the start matrix (Sigma = 1) must be positive definite
    if (status == MPC_ST_ACTIVE) {
        wg::rhs_kernel(s, 2, 0.0, nullptr);  // set_initial_primal_rhs! :25
        WG_SYNC();
        if (!wg_solve_system<false, REFINE>(q, s, pb, lds, red)) status = MPC_ST_STEP_ERROR;
    }
    if (status == MPC_ST_ACTIVE) {
        wg::axpy_kernel(s.n, 1.0, s.d, s.x);  // :28
        WG_SYNC();
        wg::rhs_kernel(s, 3, 0.0, nullptr);  // set_initial_dual_rhs! :31
        WG_SYNC();
        if (!wg_solve_system<false, REFINE>(q, s, pb, lds, red)) status = MPC_ST_STEP_ERROR;
    }
    if (status == MPC_ST_ACTIVE) {
        wg_copy(s.m, s.d + s.n, s.y);  // :33
        WG_SYNC();
        wg_jtprod(q, pb, s.y, s.jacl, lds + 2 * NB);  // :37
        wg::axpy_kernel(s.n, 1.0, s.f, s.jacl);  // :39
        WG_SYNC();
        wg::sp_init_duals_kernel(s);  // :41-66
        WG_SYNC();
        double mn[4] = {0.0, 0.0, 0.0, 0.0};
        if (s.nlb || s.nub) {
            wg::sp_mins_kernel(s, red);  // :68-78
            WG_SYNC();
            for (int k = 0; k < 4; ++k) mn[k] = red[k];
            WG_SYNC();
        }
        auto shift = [&](MpcShift by) {  // :80-83 (madqp_sp_shift: four ordered passes)
            if (s.nlb) wg::sp_shift_kernel(s.nlb, s.ind_lb, s.x, by.x);
            WG_SYNC();
            if (s.nub) wg::sp_shift_kernel(s.nub, s.ind_ub, s.x, -by.x);
            WG_SYNC();
            if (s.nlb) wg::sp_shift_kernel(s.nlb, s.ind_lb, s.zl, by.z);
            if (s.nub) wg::sp_shift_kernel(s.nub, s.ind_ub, s.zu, by.z);
            WG_SYNC();
        };
        shift(mpc_start_shift(mn));
        double sm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s.nlb || s.nub) {
            wg::sp_sums_kernel(s, red);  // :85-94
            WG_SYNC();
            for (int k = 0; k < 8; ++k) sm[k] = red[k];
            WG_SYNC();
        }
        shift(mpc_start_shift2(sm, s.nlb > 0, s.nub > 0));  // :96-99
        wg::sp_project_kernel(s, q.bound_fac);  // :101-118
        WG_SYNC();
        if (s.nlb || s.nub) {
            wg::sp_check_kernel(s, red);  // :120-123
            WG_SYNC();
            if (red[0] != 0.0) status = MPC_ST_INTERNAL;
            WG_SYNC();
        }
    }
    if (threadIdx.x == 0) q.status[b] = status;
}

// ---- loop head + build_kkt! operands: src/solver.jl:259-289 -----------------------------------
__global__ __launch_bounds__(TPB) void bq_iter_pre_kernel(BQ q) {
    __shared__ double red[32];
    __shared__ double lds[LDS_DOUBLES];
    const int64_t b = blockIdx.x;
    if (q.status[b] != MPC_ST_ACTIVE) return;
    const madqp_state s = state_of(q, b);
    const Prob pb = prob_of<WG_SHARED != 0>(q, b);
    double* sc = pb.scal;
    BSTAMP(12);  // since the end of the previous kernel of this problem: launch gap (post -> pre)
    if (q.incr_ok[b] & 1) {  // A' y of the new y = y + alpha_d dy from the product the last residual check formed
        const double ad = sc[S_ALPHA_D];
        for (int64_t j = threadIdx.x; j < q.nx; j += TPB) s.jacl[j] += ad * pb.raw_at[j];
        wg::jt_slack_kernel(pb.ns, pb.ind_ineq, s.y, s.jacl + q.nx, 1.0, 0.0);
        WG_SYNC();
    } else {
        wg_jtprod(q, pb, s.y, s.jacl, lds + 2 * NB);  // :259
    }
    BSTAMP(13);
    wg::inf_kernel(s, red);
    WG_SYNC();
    const double nrm[3] = {red[0], red[1], mpc_nanmax(red[2], red[3])};
    WG_SYNC();
    const MpcHead h = mpc_head(nrm, sc[S_NORM_B], sc[S_NORM_C], q.opt.tol, q.iters[b], q.opt.max_iter);  // :264-283
    const int status = h.status;
    // update_regularization! (src/kernels.jl:386-417)
    const MpcReg reg = mpc_update_regularization(q.opt.regularization, q.opt.delta_p, q.opt.delta_d, q.opt.delta_min,
                                                 sc[S_REG_P], sc[S_REG_D]);
    WG_SYNC();
    if (threadIdx.x == 0) {
        // the reference's print_iter line (src/structure.jl:178-195; MPCSolver.record): record number iters[b], before
        // update_regularization! replaces del_w below -- also in the pass that ends the problem
        const int64_t k = q.iters[b];
        if (q.trace && k < q.trace_cap) {
            double* tr = q.trace + (b * q.trace_cap + k) * T_COUNT;
            tr[T_OBJ] = sc[S_OBJ];
            tr[T_INF_PR] = h.inf_pr;
            tr[T_INF_DU] = h.inf_du;
            tr[T_INF_COMPL] = h.inf_compl;
            tr[T_MU] = sc[S_MU];
            tr[T_DNORM] = (k == 0) ? 0.0 : sc[S_DNORM];
            tr[T_DEL_W] = sc[S_DEL_W];
            tr[T_ALPHA_P] = sc[S_ALPHA_P];
            tr[T_ALPHA_D] = sc[S_ALPHA_D];
            tr[T_RATIO] = sc[S_RATIO];
            q.trace_count[b] = (int32_t)(k + 1);
        }
        sc[S_INF_PR] = h.inf_pr;
        sc[S_INF_DU] = h.inf_du;
        sc[S_INF_COMPL] = h.inf_compl;
        q.status[b] = status;
        if (status == MPC_ST_ACTIVE) {
            sc[S_DEL_W] = reg.del_w;
            sc[S_DEL_C] = reg.del_c;
            sc[S_REG_P] = reg.run_p;
            sc[S_REG_D] = reg.run_d;
            sc[S_NFACT] += 1.0;
        }
    }
    if (status != MPC_ST_ACTIVE) return;
    // set_aug_diagonal_reg! (src/kernels.jl:128-146)
    wg::aug_diag_fill_kernel(s, reg.del_w, reg.del_c);
    WG_SYNC();
    if (s.nlb) wg::aug_diag_lb_kernel(s);
    WG_SYNC();
    if (s.nub) wg::aug_diag_ub_kernel(s);
    WG_SYNC();
    BSTAMP(16);
    wg_build_operands(q, s, pb);
    BSTAMP(17);
}

// ---- factorize_regularized_system! (src/linear_solver.jl:6-17), trials 2 and 3: a problem whose factorisation
// failed (info != 0) multiplies del_w, del_c by 100, rebuilds Sigma / Theta / the scaled operand and takes part in
// the next (masked) assembly + Cholesky launches; every other problem sits the round out (retry_skip = 1)
__global__ __launch_bounds__(TPB) void bq_retry_kernel(BQ q) {
    const int64_t b = blockIdx.x;
    const bool retry = (q.status[b] == MPC_ST_ACTIVE) && (q.info[b] != 0);
    if (threadIdx.x == 0) {
        q.retry_skip[b] = retry ? 0 : 1;
        if (retry) q.retry_list[atomicAdd(q.retry_count, 1)] = (int32_t)b;  // (the order of the list does not enter any result)
    }
    if (!retry) return;
    const madqp_state s = state_of(q, b);
    const Prob pb = prob_of<WG_SHARED != 0>(q, b);
    double* sc = pb.scal;
    const double del_w = mpc_retry(sc[S_DEL_W]), del_c = mpc_retry(sc[S_DEL_C]);  // :14-15
    WG_SYNC();
    if (threadIdx.x == 0) {
        sc[S_DEL_W] = del_w;
        sc[S_DEL_C] = del_c;
        sc[S_NFACT] += 1.0;
    }
    wg::aug_diag_fill_kernel(s, del_w, del_c);  // set_aug_diagonal_reg! again (:9)
    WG_SYNC();
    if (s.nlb) wg::aug_diag_lb_kernel(s);
    WG_SYNC();
    if (s.nub) wg::aug_diag_ub_kernel(s);
    WG_SYNC();
    wg_build_operands(q, s, pb);
}

// ---- the rest of the iteration after factorize!: src/solver.jl:294-343 ------------------------
// GONDZIO is a template parameter: the correction loop costs the common max_ncorr = 0 instantiation
// 130 VGPRs and 864 B of scratch per lane if it is merely branched around.
// REFINE likewise (wg_solve_system): at refine_steps == 0 the programs are the ones without it.
template <bool GONDZIO, bool REFINE>
__global__ __launch_bounds__(TPB) void bq_iter_post_kernel(BQ q) {
    __shared__ double red[32];
    __shared__ double lds[LDS_DOUBLES];
    const int64_t b = blockIdx.x;
    if (q.status[b] != MPC_ST_ACTIVE) return;
    const madqp_state s = state_of(q, b);
    const Prob pb = prob_of<WG_SHARED != 0>(q, b);
    double* sc = pb.scal;
    int status = MPC_ST_ACTIVE;
    if (q.info[b] != 0) status = MPC_ST_STEP_ERROR;  // still not factorized after the three trials of src/linear_solver.jl:7
    double mu = sc[S_MU], alpha_p = 0.0, alpha_d = 0.0, dnorm = 0.0, obj = sc[S_OBJ];
    BSTAMP(14);  // since the end of the pre kernel: assembly + factorisation of the whole batch
    if (status == MPC_ST_ACTIVE) {
        wg::rhs_kernel(s, 0, 0.0, nullptr);  // set_predictive_rhs! :294
        WG_SYNC();
        if (!wg_solve_system<!GONDZIO, REFINE>(q, s, pb, lds, red)) status = MPC_ST_STEP_ERROR;
    }
    if (status == MPC_ST_ACTIVE) {
        const MpcSteps a_aff = wg_fraction_to_boundary(s, 1.0, red);      // :295
        const double mu_affine = wg_compl(s, 1, a_aff.p, a_aff.d, red);   // :296
        wg::correction_kernel(s);                                         // :297
        WG_SYNC();
        const double mu_curr = wg_compl(s, 0, 0.0, 0.0, red);  // update_barrier! src/kernels.jl:226-236
        mu = mpc_barrier(mu_affine, mu_curr, (double)(s.nlb + s.nub), q.opt.mu_min, q.opt.step_rule, q.opt.step_param).mu;
        wg::rhs_kernel(s, 1, mu, nullptr);  // set_correction_rhs! :307
        WG_SYNC();
        if (!wg_solve_system<!GONDZIO, REFINE>(q, s, pb, lds, red, /*keep=*/!GONDZIO)) status = MPC_ST_STEP_ERROR;
        // gondzio_correction_direction! (src/solver.jl:200-251)
        if constexpr (GONDZIO) {
            if (status == MPC_ST_ACTIVE && q.opt.max_ncorr > 0 && !wg_gondzio<REFINE>(q, b, s, pb, mu_curr, lds, red))
                status = MPC_ST_STEP_ERROR;
        }
    }
    if (status == MPC_ST_ACTIVE) {
        // update_step! (src/kernels.jl:307-374)
        const MpcSteps alpha = (q.opt.step_rule == 2)
                                   ? wg_mehrotra_adaptive_step(s, q.opt.step_param, red)
                                   : wg_fraction_to_boundary(s, mpc_step_tau(mu, q.opt.step_rule, q.opt.step_param), red);
        alpha_p = alpha.p;
        alpha_d = alpha.d;
        wg::norm_inf3_kernel(s.n, s.d, nullptr, nullptr, red);  // print_iter, src/structure.jl:190
        WG_SYNC();
        dnorm = red[0];
        WG_SYNC();
        wg::update_iterates_kernel(s, alpha_p, alpha_d, nullptr);  // :332-335
        WG_SYNC();
        // (the start point moves x AFTER initialize! evaluated the model, src/solver.jl:166-170 then :6-125: through the first
        // iteration f and c belong to the old point -- the reference's own loop has it so -- and an update of them would
        // carry that on; the first evaluation in the loop is therefore a full one, bit 1 of incr_ok says it has happened)
        if (!GONDZIO && pb.hx && (q.incr_ok[b] & 2))
            obj = wg_eval_model_incr(q, s, pb, alpha_p, red);  // :338-340 from the last solve's products
        else
            obj = wg_eval_model(q, s, pb, red, lds + 2 * NB);  // :338-340
        if (s.nlb || s.nub) wg::adjust_boundary_kernel(s, mpc_adjust_c1(mu), MPC_ADJUST_C2, nullptr, nullptr);  // :342
        WG_SYNC();
    }
    BSTAMP(15);
    if (threadIdx.x == 0) {
        q.status[b] = status;
        q.incr_ok[b] = (!GONDZIO && pb.hx && status == MPC_ST_ACTIVE) ? 3 : 0;  // bit 0: raw_at / raw_h belong to this step; bit 1: f, c, H x are this x's
        if (status == MPC_ST_ACTIVE) {
            sc[S_MU] = mu;
            sc[S_ALPHA_P] = alpha_p;
            sc[S_ALPHA_D] = alpha_d;
            sc[S_DNORM] = dnorm;
            sc[S_OBJ] = obj;
            q.iters[b] += 1;
        }
    }
}

// ---- test seam (madqp_debug_batch_op, tests/test_gpu_batched_ops.py): ONE of the dense helpers above on caller-made
// operands, workgroup b on the slices at b * stride, with the scratch areas the programs above hand them (tot = the whole
// LDS area, scr = lds + 2 NB).  No program of the engine calls it.  tmp: the work vector of wg_chol_solve.
__global__ __launch_bounds__(TPB) void bq_debug_op_kernel(madqp_debug_batch_op_args a, double* tmp, int64_t stmp) {
    __shared__ double lds[LDS_DOUBLES];
    const int64_t b = blockIdx.x;
    const double* M = a.M + b * a.sM;
    const double* x = a.x + b * a.sx;
    double* y = a.y + b * a.sy;
    double* raw = a.raw ? a.raw + b * a.sraw : nullptr;
    switch ((int)a.op) {
        case MADQP_DEBUG_OP_GEMV_N:
            wg_gemv_n(a.rows, a.cols, a.alpha, M, x, a.beta, y);
            break;
        case MADQP_DEBUG_OP_GEMV_N_THEN_T:
            wg_gemv_n_then_t<8>(a.rows, a.cols, M, x, a.theta + b * a.st, a.t + b * a.st, y, a.at + b * a.sat, lds);
            break;
        case MADQP_DEBUG_OP_GEMV_T:
            wg_gemv_t<WG_SHARED != 0>(a.rows, a.cols, a.alpha, M, x, a.beta, y, lds + 2 * NB, raw, a.ms);
            break;
        case MADQP_DEBUG_OP_SYMV_LOWER:
            wg_symv_lower<WG_SHARED != 0>(a.rows, a.alpha, M, x, a.beta, y, a.sym + b * a.ssym, raw, a.ms);
            break;
        case MADQP_DEBUG_OP_CHOL_SOLVE:
            wg_chol_solve(M, a.ld, a.winv + b * a.sW, a.rows, y, tmp + b * stmp, lds);
            break;
        default:
            break;
    }
}

}  // namespace WGNS
