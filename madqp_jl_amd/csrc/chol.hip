// Blocked fp64 Cholesky (lower, column-major, in place) and the triangular solves.
//
// Replaces the AbstractLinearSolver used behind NormalKKTSystem (MadNLP.LapackCPUSolver -> LAPACK
// dpotrf/dpotrs; reference call sites src/KKT/normalkkt.jl:99-101,196, src/linear_solver.jl:10-11).
//
// Factorisation, two levels of left-looking blocking so that >96 % of the flops run in wide GEMMs:
//   for each outer panel J (768..2560 columns, chosen to fill the last round of workgroups)
//     C[J0:n, J]  -= L[J0:n, 0:J0] * L[J, 0:J0]'            gemm core, N = |J|,  K = J0   (MFMA)
//     inside J, recursively: factor the first half, update the second half with it
//       C[h:n, h:w] -= L[h:n, 0:h] * L[h:w, 0:h]'           gemm core, N = K = w/2        (MFMA)
//     down to 128-column blocks jb:
//       L_jj = chol(C_jj) and the inverses of its 16 x 16 diagonal sub-blocks      one workgroup, block resident in LDS
//       L[jb+128:n, jb] = C[jb+128:n, jb] * L_jj^-T          block substitution over 16-column sub-blocks (MFMA)
// Matrices up to n = 13 312 take a right-looking schedule instead (chol_mid_step_kernel below): two launches per
// 128-column block, the diagonal block factored inside the launch that updates trailing tiles -- which tiles, with
// which panels, a plan made once per handle decides (mid_plan.inc: updates are applied when there is room, two
// panels at a time, no later than due).
// Two sweep images per diagonal block are kept (2 x n x 128 doubles: the 16 x 16 inverses on the diagonal, the
// sub-blocks off it normalised with them) and turn the diagonal solves of the two triangular sweeps into eight
// substitution steps on one wave; each sweep is ONE launch of
// ticket-ordered workgroups handing the solved blocks on through a sentinel-tagged vector, HBM bound
// (4 n^2 bytes); block rows longer than 64 tiles are streamed by several workgroups (SweepPlan).  Which tiles a sweep
// job reads is decided in one place, band_sweep_range of band_plan.inc, which both sweep kernels and the CPU checks call.
// Host side: ONE left-looking schedule as a list of operations (chol_plan.inc) and ONE executor of it (run_ops: panel_update /
// factor_block) on a CholTarget -- one matrix (madqp_chol_factor), a batch of small matrices at fixed strides (madqp_chol_factor_batched)
// or a panel of the multi-GPU loop (madqp_chol_factor_panel, ...); ONE panel solve of a 128-column block (madqp_chol_panel_solve), shared with the
// mid-size schedule (factor_mid) and dist.hip; the environment is read in one place (CholModes).
// The handle (struct madqp_chol, below): ONE owner of its device buffers (DevOwner: destroy is a synchronise and a delete,
// the paths that must leave the handle usable release what they allocated), ONE way to take a matrix (adopt_matrix) and to
// forget its factor (forget_factor: the solves refuse while there is no matrix -- the handle keeps no record of whether a
// factorisation succeeded), ONE description of a solve's sweeps (Sweeps) and ONE launcher of their three kernel forms
// (launch_sweep) on ONE scratch buffer, for both paths of madqp_chol_solve and for madqp_trsv_tile.
#include <algorithm>
#include <cstdlib>

#include <vector>

#include "common.h"
#include "panel_image.h"
#include "band_plan.inc"
#include "mid_plan.inc"
#include "solve_plan.inc"

typedef double double2_t __attribute__((ext_vector_type(2)));

namespace {
constexpr int NB = 128;    // diagonal block
constexpr int NBO = 1024;  // outer panel
static_assert(SOLVE_NB == NB, "solve_plan.inc plans in this file's blocks");
// madqp_chol_solve_many takes the blocked path from this many right-hand sides on (madqp_chol_set_solve_many_min changes it
// per handle).  Measured (tools/bench_solve_many.py -> profiles/solve_many.json, "min_nrhs"): the smallest of 2, 4, .., 128 from
// which on the blocked median beats the looped one by more than the spread at n = 5 000, 12 800, 50 000 and on the packed band
// of order 90 000 alike.  The blocked path costs the same up to 128 columns -- its launches, not its bytes, are its time -- and
// a one-vector solve a sixteenth to a twentieth of that, so the two cross between 16 and 32 in every case.
constexpr int64_t SOLVE_MANY_MIN_DEFAULT = 32;
#ifndef P2_LDS_LD
#define P2_LDS_LD (NB + 1)
#endif
constexpr int LDS_LD = P2_LDS_LD;
static_assert(IMG_NB == NB, "panel_image.h describes this file's blocks");
constexpr int64_t WBLK = IMG_WBLK;  // doubles per block in chol->winv: [Wcm | Wrm], the form they travel in (panel_image.h)

typedef double double4_t __attribute__((ext_vector_type(4)));
#include "gemm_core.inc"
constexpr int SB = 16;             // sub-block of the diagonal kernel (one MFMA tile)
constexpr int NSB = NB / SB;       // 8 sub-block columns
constexpr int WD_LD = SB + 1;      // row stride of the inverse diagonal sub-blocks

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// 1/sqrt(a) for a normal, positive pivot: hardware estimate (v_rsq_f64: 2^-24.2 measured) + two coupled
// Goldschmidt steps in fma form -- eight instructions, six deep, instead of the sqrt-and-divide sequence behind rsqrt().
// Max error 1.90 ulp over 4 M arguments (tools/scratch/rsq_probe.hip).  (One third-order step, y (1 + e + 3/2 e^2)
// with e = (1 - a y^2) / 2, is six instructions, four deep, 1.24 ulp -- and 0.05 us per 16 pivots, which is not worth
// moving every last bit of every factor for: the distributed path's hardest parity case then sits at 19 x instead of
// under 16 x the distance between two CPU runs.)
__device__ __forceinline__ double fast_rsqrt(double a) {
    const double y = __builtin_amdgcn_rsq(a);
    double g = a * y, h = 0.5 * y;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    r = __builtin_fma(-h, g, 0.5);
    h = __builtin_fma(h, r, h);
    return h + h;
}

// the 16 x 16 sub-block at (b, b) of S, both triangles from the stored lower one, in the accumulator layout
__device__ __forceinline__ double4_t diag16_load(const double* __restrict__ S, int b, int lane) {
    const int lo = lane & 15, hi = lane >> 4;
    double4_t A;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int row = hi + 4 * v;
        A[v] = (row >= lo) ? S[(b + lo) * LDS_LD + b + row] : S[(b + row) * LDS_LD + b + lo];
    }
    return A;
}
// One wave: Cholesky of the 16 x 16 sub-block at (b, b) of S and the inverse of its factor, in four RANK-4 steps on the
// MFMA unit.  The (symmetric) sub-block and W live in the accumulator layout of v_mfma_f64_16x16x4_f64 (lane l,
// register v: row (l>>4) + 4v, column l&15), so the four rows 4p .. 4p+3 of the block are ONE register (A[p]: lane
// group hi holds row 4p + hi) -- and one register per lane group is exactly what a k-slot of the instruction takes: the
// four scaled rows of a 4-row group are the A- and the B-operand of D -= sum_j l_j l_j' as they stand, ONE dependent
// MFMA per four pivots.  (Round 1 kept a row per lane and broadcast with 2 x 135 v_readlane: 5.0 us per sub-block;
// rounds 1-2 ran 16 rank-1 MFMA steps, 3.08 us: every pivot paid the round trip through a dependent MFMA; this form
// 2.84 us -- what remains is 16 x (read-lane -> rsqrt chain -> scale -> read-lane -> fma) on the vector ALU, ~175 ns
// each, tools/potf2_probe.)  The 4 x 4 elimination inside the group runs
// on the vector ALU, on all 64 lanes redundantly: the four rows (and the four rows of W) are first replicated to every
// lane group (one cross-lane read each), after which a pivot needs two read-lanes, the rsqrt chain and one fma per
// later row.  Every update is one fused multiply-add, in the order of the pivots; W = L^-1 follows from the same steps
// applied to the identity (W[k,:] *= 1/l_kk, W[i,:] -= l_ik W[k,:], i > k).  Writes L (lower) back to S and W to
// Wd[r*WD_LD + c] (zero above the diagonal).
// A: the symmetric sub-block in the accumulator layout (diag16_load, or the accumulators of the update that completed it)
__device__ __forceinline__ void diag16_factor_invert(double4_t A, double* __restrict__ S, int b, double* __restrict__ Wd,
                                                        int32_t* __restrict__ info, int32_t col0, int lane) {
    const int lo = lane & 15, hi = lane >> 4;
    double4_t W;
#pragma unroll
    for (int v = 0; v < 4; ++v) W[v] = (hi + 4 * v == lo) ? 1.0 : 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int k0 = 4 * p;
        double R[4], V[4], l[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // rows k0 + j of A and of W, in every lane group
            R[j] = __shfl(A[p], lo + 16 * j, 64);
            V[j] = __shfl(W[p], lo + 16 * j, 64);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j;
            double akk = readlane_f64(R[j], k);
            if (__builtin_expect(!(akk > 0.0), 0)) {  // not positive definite (or NaN): record the first column, go on with a unit pivot
                if (lane == 0) atomicCAS(info, 0, col0 + b + k + 1);
                akk = 1.0;
                R[j] = (lo == k) ? 1.0 : R[j];
            }
            const double rd = fast_rsqrt(akk);
            // row k scaled: column k of it is a_kk / sqrt(a_kk) = l_kk itself (the row holds a_kk there), exact zeros above
            // the diagonal.  (The pivot steps are bound by the number of vector instructions one wave issues in order,
            // ~48 per pivot, not by the latency of any of them: every select and masked store here is time on the chain.)
            const double lk = (lo >= k) ? R[j] * rd : 0.0;
            l[j] = lk;
            w[j] = V[j] * rd;  // row k of W, scaled
#pragma unroll
            for (int j2 = j + 1; j2 < 4; ++j2) {  // the later rows of the group: A[i,:] -= l_ik l_k', W[i,:] -= l_ik w_k
                const double s = readlane_f64(lk, k0 + j2);
                R[j2] = __builtin_fma(-s, lk, R[j2]);
                V[j2] = __builtin_fma(-s, w[j], V[j2]);
            }
        }
        const double lsel = (hi == 0) ? l[0] : (hi == 1) ? l[1] : (hi == 2) ? l[2] : l[3];
        const double wsel = (hi == 0) ? w[0] : (hi == 1) ? w[1] : (hi == 2) ? w[2] : w[3];
        if (lo >= k0 + hi) S[(b + k0 + hi) * LDS_LD + b + lo] = lsel;  // rows k0 .. k0+3 of L, one lane group each
        A = __builtin_amdgcn_mfma_f64_16x16x4f64(-lsel, lsel, A, 0, 0, 0);
        const double aw = (lo >= k0 + 4) ? lsel : 0.0;  // rows below the group; its own rows were done above
        W = __builtin_amdgcn_mfma_f64_16x16x4f64(-aw, wsel, W, 0, 0, 0);
        W[p] = wsel;  // rows k0 .. k0+3 of W are final
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) Wd[(hi + 4 * v) * WD_LD + lo] = W[v];
}
// Cholesky of one nb x nb (nb <= 128) diagonal block, resident in LDS, and the inverse of its
// factor -- blocked by 16 so that everything off the 16 x 16 diagonal sub-blocks is
// v_mfma_f64_16x16x4_f64 work with operands read straight from the LDS image:
//   for J = 0..7:  wave 0: L_JJ, W_JJ = L_JJ^-1 (registers + v_readlane)
//                  all waves: L_IJ = A_IJ W_JJ'  (I > J),   A_IK -= L_IJ L_KJ'  (I >= K > J)
//   then W = L^-1 block column by block column (columns are independent -> one per wave, no
//   barrier):  W_IJ = -W_II * sum_{K=J}^{I-1} L_IK W_KJ.  The f64 accumulator layout
//   (row = (lane>>4) + 4v) is exactly the B-operand layout (k = 4s + (lane>>4)), so the inner
//   sum feeds the second product without leaving the registers.
// W_IJ (I > J) is parked in the unused upper triangle at S[R*LDS_LD + C] (R > C global indices).
// info: the first failing column (1-based, LAPACK dpotrf convention) is recorded once; the block
// is then completed with a unit pivot so that the launch always terminates.
// Outputs: L_jj in place; Wcm[r + c*NB] = W(r,c) (column-major) and Wrm[c + r*NB] = W(r,c)
// (row-major), both zero padded to 128 x 128.
#ifdef MADQP_POTF2_STAMPS
__device__ unsigned long long madqp_potf2_stamps[64];  // diagnostic build only (tools/potf2_probe.cpp)
#define P2_STAMP(i)                                                                    \
    do {                                                                               \
        if (threadIdx.x == 0) madqp_potf2_stamps[i] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define P2_STAMP(i)
#endif
struct Potf2Batch {  // problem blockIdx.x: pointer strides (doubles / ints); skip[b] != 0: leave untouched
    int64_t sA, sW, sInfo;
    const int32_t* skip;
    const int32_t* list = nullptr;   // compacted form (GemmBatch::list): slot blockIdx.x works off list[x], list[x + grid], ..
    const int32_t* count = nullptr;
};
#ifndef P2_QUIET_WAVE
#define P2_QUIET_WAVE 4
#endif
constexpr int P2_QUIET = P2_QUIET_WAVE;  // -1: every helper wave works in the trailing phase
// 512 threads: wave 0 runs the chain of 16 x 16 diagonal factorisations, waves 1..7 everything else
constexpr int P2_S_DOUBLES = NB * LDS_LD;         // S[c*LDS_LD + r] = element (r, c)
constexpr int P2_WD_DOUBLES = NSB * SB * WD_LD;   // inverse diagonal sub-blocks
// The helper waves' tile products of step J, NHE waves sharing them round-robin: waves[J][hr] = up to eight entries of
// 8 bits, 0xFF ends the list; bit 6: 0 = trailing tile (K = bits 5..3, I = bits 2..0), 1 = inverse tile (I, J').
// Drawn at compile time: enumerating the 34 tiles of a step in every wave (loop, modulo, three branches per tile) cost
// more instruction issue and fetch than the products themselves -- the phase got SLOWER with more helper waves.
// MODE 0: trailing tiles and inverse tiles (factor + invert in one kernel); 1: trailing tiles only (factor)
template <int NHE, int MODE>
struct P2Lists {
    static_assert(NHE >= 5, "at most 34 tiles per step: seven entries and the end mark per wave");
    unsigned long long waves[NB / 16][NHE];
    constexpr P2Lists() : waves{} {
        constexpr int N = NB / 16;
        for (int J = 0; J < N; ++J) {
            int cnt[NHE] = {};
            for (int h = 0; h < NHE; ++h) waves[J][h] = ~0ull;
            int c = 0;
            auto put = [&](int e) {
                const int h = c % NHE;
                waves[J][h] = (waves[J][h] & ~(0xFFull << (8 * cnt[h]))) | ((unsigned long long)e << (8 * cnt[h]));
                ++cnt[h];
                ++c;
            };
            for (int K = J + 1; K < N; ++K)
                for (int I = K; I < N; ++I)
                    if (!(K == J + 1 && I == J + 1)) put(K * 8 + I);
            if (MODE != 1)
                for (int I = J + 1; I < N; ++I)
                    for (int Jp = 0; Jp <= J; ++Jp) put(64 + I * 8 + Jp);
        }
    }
};
template <int NHE, int MODE>
__device__ __constant__ const P2Lists<NHE, MODE> p2_lists{};

// LDS reads of a 16 x 16 tile product issued TOGETHER (inline asm: left to itself the compiler puts every operand pair
// next to the MFMA that consumes it -- read, wait, MFMA, four times in a row, five LDS round trips per tile product:
// 0.76 us per product on a helper wave where the four dependent MFMAs take 0.11).
template <int OFF>
__device__ __forceinline__ double p2_read(unsigned addr) {
    double d;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
    return d;
}
template <int STRIDE>
__device__ __forceinline__ void p2_read4(unsigned addr, double (&v)[4]) {
    v[0] = p2_read<0>(addr);
    v[1] = p2_read<STRIDE>(addr);
    v[2] = p2_read<2 * STRIDE>(addr);
    v[3] = p2_read<3 * STRIDE>(addr);
}
__device__ __forceinline__ void p2_wait(double (&a)[4], double (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
                 :
                 : "memory");
}
__device__ __forceinline__ void p2_wait(double (&a)[4], double (&b)[4], double (&c)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                   "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3])
                 :
                 : "memory");
}
__device__ __forceinline__ unsigned p2_lds(const double* p) { return (unsigned)(uintptr_t)(lds_ptr_t)p; }
// the whole workgroup (NT threads: 512, or 1024 in probe builds) calls this; S and Wd are its LDS work areas
// MODE (round 4): 0 = factor and invert (the batched engine, whose workgroup sweeps multiply with the full inverses);
// 1 = factor only -- L_jj and the inverses of its eight 16 x 16 diagonal sub-blocks, which is all the panel solve
// (panel_sub16_kernel) needs: the serial spine of a factorisation then carries neither the inverse's tile products nor the
// stores of two 128 x 128 images; the off-diagonal parts of the sweep images follow in ONE launch per factorisation, off
// the chain (sweep_image_kernel).
template <int NT, int MODE = 0>
__device__ __forceinline__ void potf2_inv_body(double* __restrict__ A, int64_t lda, int nb,
                                               double* __restrict__ Wcm, double* __restrict__ Wrm,
                                               int32_t* __restrict__ info, int32_t col0,
                                               double* __restrict__ S, double* __restrict__ Wd,
                                               bool tile_in_lds = false) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    P2_STAMP(0);
    if (!tile_in_lds) {  // lower triangle -> LDS: row r = tid & 127, columns (tid >> 7) + CG*i; all loads of a thread in flight at
        // once (one HBM / L2 latency; the kernel runs alone on its CU, registers are free)
        constexpr int CG = NT / NB;
        const int r = tid & (NB - 1), c0 = tid >> 7;
        double v[NB / CG];
#pragma unroll
        for (int i = 0; i < NB / CG; ++i) {
            const int c = c0 + CG * i;
            double x = 0.0;
            if (r < nb && c < nb) {
                if (r >= c) x = A[r + (int64_t)c * lda];
            } else if (r == c) {
                x = 1.0;  // identity padding keeps the padded block positive definite
            }
            v[i] = x;
        }
#pragma unroll
        for (int i = 0; i < NB / CG; ++i) S[(c0 + CG * i) * LDS_LD + r] = v[i];
    }
    __syncthreads();
    P2_STAMP(1);
    // one 16 x 16 trailing tile (K, I) of step J: A_IK -= L_IJ L_KJ'
    auto trailing_tile = [&](int J, int K, int I) {
        const int b = J * SB;
        double* cp = S + (SB * K + lo) * LDS_LD + SB * I + hi;
        double c[4], av[4], bv[4];
        p2_read4<4 * 8>(p2_lds(cp), c);
        p2_read4<4 * LDS_LD * 8>(p2_lds(S + (b + hi) * LDS_LD + SB * I + lo), av);  // L_IJ[lo][k]
        p2_read4<4 * LDS_LD * 8>(p2_lds(S + (b + hi) * LDS_LD + SB * K + lo), bv);  // L_KJ[lo][k]
        p2_wait(c, av, bv);
        double4_t acc = {c[0], c[1], c[2], c[3]};
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[q], bv[q], acc, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) cp[4 * v] = acc[v];
    };
    // W = L^-1 is built inside the same eight steps by the helper waves (wave 0's 16-step chain is the critical
    // path of a step): T_IJ' = sum_{K=J'}^{I-1} L_IK W_KJ' accumulates in the unused upper triangle (W(r, c) lives
    // at S[r*LDS_LD + c], r > c) -- step J adds L_IJ W_JJ' for every I > J, J' <= J -- and row I is finished as
    // W_IJ' = -W_II T_IJ' at the start of step I, once step I-1 has produced W_II.  The f64 accumulator layout
    // (row = (lane>>4) + 4v) is the B-operand layout (k = 4s + (lane>>4)), so T feeds the second product from
    // registers.  (As a separate phase after the factorisation this cost 8.4 us of the block's 58.)
    auto t_update = [&](int J, int I, int Jp) {  // T_IJ' += L_IJ W_JJ'
        double* tp = S + (SB * I + hi) * LDS_LD + SB * Jp + lo;
        double c[4], av[4], bv[4];
        p2_read4<4 * LDS_LD * 8>(p2_lds(tp), c);
        p2_read4<4 * LDS_LD * 8>(p2_lds(S + (SB * J + hi) * LDS_LD + SB * I + lo), av);  // L_IJ[lo][k]
        if (Jp == J)
            p2_read4<4 * WD_LD * 8>(p2_lds(Wd + (J * SB + hi) * WD_LD + lo), bv);  // W_JJ[k][lo]
        else
            p2_read4<4 * LDS_LD * 8>(p2_lds(S + (SB * J + hi) * LDS_LD + SB * Jp + lo), bv);  // W_JJ'[k][lo]
        p2_wait(c, av, bv);
        double4_t T = {c[0], c[1], c[2], c[3]};
#pragma unroll
        for (int q = 0; q < 4; ++q) T = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], T, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) tp[4 * v * LDS_LD] = T[v];
    };
    auto w_finish = [&](int I, int Jp) {  // W_IJ' = -W_II T_IJ'
        double4_t T, R = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int v = 0; v < 4; ++v) T[v] = S[(SB * I + hi + 4 * v) * LDS_LD + SB * Jp + lo];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double av = Wd[(I * SB + lo) * WD_LD + 4 * s + hi];  // W_II[lo][4s+hi]
            R = __builtin_amdgcn_mfma_f64_16x16x4f64(av, T[s], R, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) S[(SB * I + hi + 4 * v) * LDS_LD + SB * Jp + lo] = -R[v];
    };
    constexpr int NWV = NT / 64, NH = NWV - 1;  // waves; helper waves 1..NH
    if (wave == 0) diag16_factor_invert(diag16_load(S, 0, lane), S, 0, Wd, info, col0, lane);
    __syncthreads();
    P2_STAMP(2);
    for (int J = 0; J < NSB; ++J) {
        const int b = J * SB;
        double* WdJ = Wd + J * SB * WD_LD;
        // panel L_IJ = A_IJ * W_JJ' (I > J) and the rows W_JJ' (J' < J) of the inverse: 7 tile products
        for (int o = wave; o < NSB - 1; o += NWV) {
            if (o < J) {
                if (MODE != 1) w_finish(J, o);
                continue;
            }
            const int I = o + 1;
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double av = S[(b + 4 * s + hi) * LDS_LD + SB * I + lo];  // A_IJ[lo][4s+hi]
                const double bv = WdJ[lo * WD_LD + 4 * s + hi];                // W_JJ[lo][4s+hi]
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) S[(b + lo) * LDS_LD + SB * I + hi + 4 * v] = acc[v];
        }
        __syncthreads();
        P2_STAMP(3 + 3 * J);
        // trailing update with look-ahead: wave 0 updates the next diagonal tile and factors it at once
        // (the 16-step chain of diag16_factor_invert is the critical path) while the helper waves update the
        // other tiles of this step and the T tiles of the inverse
        if (J + 1 < NSB) {
            if (wave == 0) {
                trailing_tile(J, J + 1, J + 1);
                // (keeping this update in registers as the input of the pivot chain, instead of the round trip through
                // S, changed nothing: 2.12-2.20 us per step either way)
                diag16_factor_invert(diag16_load(S, b + SB, lane), S, b + SB, WdJ + SB * WD_LD, info, col0, lane);
            } else if (P2_QUIET < 0 || (wave & 3) != 0) {
                // (waves 4, 8, .. share their SIMD with wave 0 and sit this phase out: the fp64 MFMAs of a helper
                // there hold up every vector instruction of the pivot chain)
                constexpr int NHE = (P2_QUIET < 0) ? NH : NH - (NWV - 1) / 4;
                const int hr = __builtin_amdgcn_readfirstlane((P2_QUIET >= 0) ? wave - 1 - (wave >> 2) : wave - 1);  // 0 .. NHE-1
                unsigned long long lst = p2_lists<NHE, MODE>.waves[J][hr];  // this wave's tiles of the step (P2Lists)
                while ((lst & 0xFF) != 0xFF) {
                    const int e = (int)(lst & 0xFF);
                    lst = (lst >> 8) | (0xFFull << 56);
                    if (e & 64)
                        t_update(J, (e >> 3) & 7, e & 7);
                    else
                        trailing_tile(J, (e >> 3) & 7, e & 7);
                }
                // the 16 columns of L that step J completed go to global memory now, beside wave 0's pivot chain
                // (round 4: as one pass after the last step the store of the factor was 1.5 us at the END of the chain)
                for (int c = b + hr; c < b + SB && c < nb; c += NHE) {
                    const double* sc = S + c * LDS_LD;
                    double* gc = A + (int64_t)c * lda;
                    if (lane >= c && lane < nb) gc[lane] = sc[lane];
                    if (lane + 64 >= c && lane + 64 < nb) gc[lane + 64] = sc[lane + 64];
                }
            }
        }
        __syncthreads();
        P2_STAMP(4 + 3 * J);
    }
    // the last 16 columns of the factor -> global (the others went out step by step)
    {
        const int r = (NSB - 1) * SB + (tid & 15), c = (NSB - 1) * SB + (tid >> 4);
        if (tid < SB * SB && c <= r && r < nb) A[r + (int64_t)c * lda] = S[c * LDS_LD + r];
    }
    P2_STAMP(26);
    P2_STAMP(27);
    // only the lower triangles are written: the images are zero filled once when they are allocated
    if (MODE == 1) {  // the eight 16 x 16 diagonal inverses, at their places in both images
        for (int e = tid; e < NSB * SB * SB; e += NT) {
            const int J = e >> 8, rr = (e >> 4) & 15, cc = e & 15;
            const int gr = SB * J + rr, gc = SB * J + cc;
            if (cc <= rr && gr < nb) {
                const double wv = Wd[(J * SB + rr) * WD_LD + cc];
                Wcm[gc * NB + gr] = wv;
                Wrm[gr * NB + gc] = wv;
            }
        }
    } else {
        constexpr int CG = NT / NB;
        const int i = tid & (NB - 1), j0 = tid >> 7;
        auto W_at = [&](int r, int c) {
            return (r / SB == c / SB) ? Wd[r * WD_LD + c % SB] : S[r * LDS_LD + c];
        };
        if (i < nb) {
#pragma unroll 8
            for (int q = 0; q < NB / CG; ++q) {
                const int j = j0 + CG * q;
                if (j <= i) Wcm[j * NB + i] = W_at(i, j);            // column-major: r = i (fast), c = j
                if (j >= i && j < nb) Wrm[j * NB + i] = W_at(j, i);  // row-major:    c = i (fast), r = j
            }
        }
    }
    P2_STAMP(28);
}

#ifndef P2_KTHREADS
#define P2_KTHREADS 512  // (1024: loads and stores of the block 2.7 us faster, the steps the same; no gain in the applications)
#endif
template <int MODE>
__global__ __launch_bounds__(P2_KTHREADS) void potf2_inv_kernel(double* __restrict__ A, int64_t lda, int nb,
                                                        double* __restrict__ Wcm,
                                                        double* __restrict__ Wrm,
                                                        int32_t* __restrict__ info, int32_t col0,
                                                        Potf2Batch bt) {
    __shared__ double S[P2_S_DOUBLES];
    __shared__ double Wd[P2_WD_DOUBLES];
    if (bt.list) {
        const int cnt = *bt.count;
        for (int pb = blockIdx.x; pb < cnt; pb += gridDim.x) {
            const int64_t b = bt.list[pb];
            potf2_inv_body<P2_KTHREADS, MODE>(A + b * bt.sA, lda, nb, Wcm + b * bt.sW, Wrm + b * bt.sW, info + b * bt.sInfo, col0, S, Wd);
            __syncthreads();
        }
        return;
    }
    if (gridDim.x > 1 || bt.skip) {
        const int64_t b = blockIdx.x;
        if (bt.skip && bt.skip[b] != 0) return;
        A += b * bt.sA;
        Wcm += b * bt.sW;
        Wrm += b * bt.sW;
        info += b * bt.sInfo;
    }
    potf2_inv_body<P2_KTHREADS, MODE>(A, lda, nb, Wcm, Wrm, info, col0, S, Wd);
}

// The off-diagonal 16 x 16 sub-blocks of both sweep images of the diagonal blocks j0/128 .. of a factored matrix, one
// workgroup per block, ONE launch per factorisation (see "the diagonal step of a sweep" below): image 1 (column-major)
// gets Lt_IJ = L_IJ W_JJ at (16 I.., 16 J..), image 2 gets Lh_IJ = W_II L_IJ transposed, i.e. at [(16 I + k) NB + 16 J + c]
// -- what the factor-only diagonal kernels (MODE 1) leave out of the serial spine; the diagonals (W_JJ, left by those
// kernels) stay.
__global__ __launch_bounds__(256) void sweep_image_kernel(const double* __restrict__ A, int64_t lda, int64_t n, int64_t j0,
                                                          double* __restrict__ winv) {
    __shared__ double S[P2_S_DOUBLES];   // S[c*LDS_LD + r] = L(r, c), zero beyond the order of a short block
    __shared__ double Wd[P2_WD_DOUBLES]; // W_JJ[r][c] at (J*SB + r)*WD_LD + c
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const int64_t jb = j0 + (int64_t)blockIdx.x * NB;
    const int nb = (int)((n - jb < NB) ? (n - jb) : NB);
    double* Wcm = winv + (jb / NB) * WBLK;
    double* Wrm = Wcm + NB * NB;
    const double* Ab = A + jb + jb * lda;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e & (NB - 1), c = e >> 7;
        const int rr = r < nb ? r : nb - 1, cc = c < nb ? c : nb - 1;  // (unconditional loads from addresses that exist)
        const double v = Ab[rr + (int64_t)cc * lda];
        S[c * LDS_LD + r] = (r < nb && c <= r) ? v : 0.0;
    }
    for (int e = tid; e < NSB * SB * SB; e += 256) {
        const int J = e >> 8, rr = (e >> 4) & 15, cc = e & 15;
        const double v = Wcm[(SB * J + cc) * NB + SB * J + rr];
        Wd[(J * SB + rr) * WD_LD + cc] = (cc <= rr) ? v : 0.0;
    }
    __syncthreads();
    for (int p = wave; p < NSB * (NSB - 1) / 2; p += 4) {
        int I = 1, q = p;  // pair p -> (I, J), I > J
        while (q >= I) {
            q -= I;
            ++I;
        }
        const int J = q;
        double4_t P = {0.0, 0.0, 0.0, 0.0}, Q = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int k = 4 * s4 + hi;
            // P = L_IJ W_JJ: A[m = lo][k] = L_IJ[lo][k], B[k][n = lo] = W_JJ[k][lo]
            const double pa = S[(SB * J + k) * LDS_LD + SB * I + lo];
            const double pb = Wd[(J * SB + k) * WD_LD + lo];
            P = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, pb, P, 0, 0, 0);
            // Q = W_II L_IJ: A[m = lo][k] = W_II[lo][k], B[k][n = lo] = L_IJ[k][lo]
            const double qa = Wd[(I * SB + lo) * WD_LD + k];
            const double qb = S[(SB * J + lo) * LDS_LD + SB * I + k];
            Q = __builtin_amdgcn_mfma_f64_16x16x4f64(qa, qb, Q, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {  // D[m = hi + 4v][n = lo]
            Wcm[(SB * J + lo) * NB + SB * I + hi + 4 * v] = P[v];
            Wrm[(SB * I + hi + 4 * v) * NB + SB * J + lo] = Q[v];
        }
    }
}

// ---- triangular sweeps, one launch each ---------------------------------------------------------
// A sweep over the 128-row blocks is a chain: block r needs the solutions of all blocks before it.
// Instead of one launch per block (391 launches per sweep at n = 50 000, each with its own ramp and
// tail) ONE launch runs a workgroup per block; workgroup r streams its own tiles L[r, j] (forward) /
// L[j, r] (backward) as the x_j appear and then solves its diagonal block by unit block substitution on the block's
// sweep image (see "the diagonal step of a sweep" below).
//   * order: a workgroup draws its block index from a ticket counter, so it only ever waits for
//     blocks drawn earlier, which are resident or finished -- the grid always drains, whatever the
//     dispatch order and however many workgroups fit on the chip;
//   * hand-off: x_j is published as 128 naturally aligned 8-byte write-through (sc1) stores into a
//     vector pre-filled with a NaN sentinel; consumers poll the values themselves with sc1 loads
//     (data = tag: no flag, no fence; MI355X_MICROARCH.md "handoff-1to1", ~1 us per hop);
//   * streaming: 16 waves x (2 rows per lane) x (4 columns per wave) = half a tile per stage, two
//     stages in flight in registers while the wave waits for the next x_j; the block's sweep image
//     sits in LDS from the start, so the critical path per block is
//     poll -> 8 fma -> cross-wave sum -> eight substitution steps on one wave -> publish.
// Summation order is fixed by the thread mapping: results do not depend on timing.
constexpr unsigned long long SWEEP_SENTINEL = 0x7FF8A5A57FF8A5A5ull;  // a NaN no arithmetic produces
constexpr int SWEEP_SPIN_LIMIT = 1 << 22;

__device__ __forceinline__ unsigned long long ld_sc1_u64(const double* p) {
    return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1_f64(double* p, double v) {
    unsigned long long u = __double_as_longlong(v);
    if (v != v) u = 0x7FF8000000000000ull;  // never publish the sentinel pattern
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave 0: wait until the 128 entries of block j of `x` have been published, copy them to LDS
// (entries at or beyond n are zero).  Returns with the error flag set if the producer never shows up.
__device__ __forceinline__ void sweep_poll_block(const double* __restrict__ x, int64_t j, int64_t n,
                                                 double* __restrict__ dst, double* __restrict__ err,
                                                 int lane) {
    const int64_t i0 = j * NB + 2 * lane;
    unsigned long long u0 = 0, u1 = 0;
    int spins = 0;
    bool wait0 = i0 < n, wait1 = i0 + 1 < n;
    while (wait0 || wait1) {
        if (wait0) {
            u0 = ld_sc1_u64(x + i0);
            wait0 = (u0 == SWEEP_SENTINEL);
        }
        if (wait1) {
            u1 = ld_sc1_u64(x + i0 + 1);
            wait1 = (u1 == SWEEP_SENTINEL);
        }
        if ((wait0 || wait1) && ++spins > SWEEP_SPIN_LIMIT) {
            *err = 1.0;  // the context's fault word: read back with the next scalar result (madqp_read_results)
            u0 = u1 = 0x7FF8000000000000ull;
            break;
        }
    }
    dst[2 * lane] = (i0 < n) ? __longlong_as_double(u0) : 0.0;
    dst[2 * lane + 1] = (i0 + 1 < n) ? __longlong_as_double(u1) : 0.0;
}

// A long block row is streamed by several workgroups (madqp_chol_create builds the job list): job (r, c) takes the
// tiles c*chunk .. min(r, (c+1)*chunk) - 1 of block r (counted from the far end of the dependency chain); the job
// holding the tile next to the diagonal owns the block, the others publish their 128 partial sums to
// part[(r*maxc + c)*128 ..] the way solution blocks are published.  jobs == nullptr: one job per block.
// Under a band of kb blocks (the kernels' last argument; negative: none) block r has the kb tiles next to its diagonal
// block only: a job starts no earlier than the first of them, the chunks before it are no jobs (band_sweep_jobs) and the
// owner adds the partial sums from that chunk on -- band_sweep_range (band_plan.inc) is the arithmetic, for the kernels and
// the CPU checks alike.  The protocol -- tickets, sentinel, spin limit, order -- is the same.
struct SweepPlan {
    const int32_t* jobs;  // ticket -> r | c << 20, ordered by (r, c): a job waits only for earlier tickets
    double* part;
    int32_t chunk, maxc;
};

// one published value (sentinel until its producer has stored it)
__device__ __forceinline__ double sweep_poll_one(const double* p, double* __restrict__ err) {
    unsigned long long u = ld_sc1_u64(p);
    int spins = 0;
    while (u == SWEEP_SENTINEL) {
        if (++spins > SWEEP_SPIN_LIMIT) {
            *err = 1.0;
            return __longlong_as_double(0x7FF8000000000000ull);
        }
        u = ld_sc1_u64(p);
    }
    return __longlong_as_double(u);
}

// The partial sums of a block's other jobs for the lane's two entries, added in job order.  Up to four jobs' words are
// requested at once: one after the other, each an L2 round trip of ~1 us, they were half of a hop at n = 50 000 (six
// jobs per block row: 6.2 us per hop where n = 5 000, one job per row, takes 3.2).  cfirst: the row's first job (0 unless
// a band cuts the row short: the chunks before it are no jobs and publish nothing).
__device__ __forceinline__ void sweep_far2(const double* __restrict__ pp, int cfirst, int c, int lane,
                                           double* __restrict__ err, double& f0, double& f1) {
    f0 = f1 = 0.0;
    for (int c0 = cfirst; c0 < c; c0 += 4) {
        unsigned long long u[4][2];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < c) {
                u[k][0] = ld_sc1_u64(pp + (int64_t)(c0 + k) * NB + lane);
                u[k][1] = ld_sc1_u64(pp + (int64_t)(c0 + k) * NB + 64 + lane);
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < c) {
                const double a = (u[k][0] == SWEEP_SENTINEL) ? sweep_poll_one(pp + (int64_t)(c0 + k) * NB + lane, err)
                                                             : __longlong_as_double(u[k][0]);
                const double b = (u[k][1] == SWEEP_SENTINEL) ? sweep_poll_one(pp + (int64_t)(c0 + k) * NB + 64 + lane, err)
                                                             : __longlong_as_double(u[k][1]);
                f0 += a;
                f1 += b;
            }
    }
}

// half a 128 x 128 column-major tile: rows 2*lane, 2*lane+1 and the 4 columns of this wave
__device__ __forceinline__ void sweep_load_half(const double* __restrict__ base, int64_t ld, bool ok0,
                                                bool ok1, bool vec, double2_t (&dst)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double* p = base + (int64_t)q * ld;
        if (vec && ok1) {
            dst[q] = *reinterpret_cast<const double2_t*>(p);
        } else {
            dst[q].x = ok0 ? p[0] : 0.0;
            dst[q].y = ok1 ? p[1] : 0.0;
        }
    }
}

// ---- the diagonal step of a sweep by UNIT BLOCK SUBSTITUTION over the 16 x 16 sub-blocks (round 5) -----------------------
// A product with a stored 128 x 128 inverse (the form of rounds 1-4, removed; its numbers: DESIGN.md 4.2) leaves a
// residual of cond(L_rr) eps where substitution leaves eps, and the interior-point iterates see the residual: on
// ill-conditioned problems the per-iteration traces sat up to 80 x the CPU noise floor from LAPACK's
// (profiles/r04_parity_ratios_default.json; tools/numerics/blockchol_emul.py: it is the product with ANY stored
// 128-inverse, while block substitution over 16 x 16 sub-blocks is statistically as good as dtrsv).  The sweeps
// therefore substitute: with W_JJ = (L_rr)_JJ^-1 (16 x 16, left on the images' diagonals by the factor-only
// diagonal kernel) and the off-diagonal sub-blocks normalised ONCE per factorisation (sweep_image_kernel),
//     forward   Lt_IJ = L_IJ W_JJ :   u_I = v_I - sum_{J<I} Lt_IJ u_J,    z_I = W_II u_I
//     backward  Lh_IJ = W_II L_IJ :   w_J = v_J - sum_{I>J} Lh_IJ' w_I,   x_J = W_JJ' w_J
// (the same error bound as z_I = W_II (v_I - sum L_IJ z_J): the 16 x 16 inverses enter once per term either way), so
// that ONE broadcast of the 16 values u_J serves both the rows of sub-block J (-> z_J) and every row below (-> update):
// eight steps of 32 read-lanes + 32 fused multiply-adds on ONE wave, no barrier, no LDS round trip on the chain.
// (Plain block substitution on un-normalised images needs a second broadcast per step; measured and removed.)
// The image of a block sits in LDS packed by columns: forward column c (sub-block J) holds rows 16 J .. 127, backward
// column q (sub-block I) rows 0 .. 16 I + 15; a lane reads consecutive rows of one column: conflict free.
constexpr int XIMG_DOUBLES = 16 * (8 * NB - 16 * 28);                                               // 9 216
__host__ __device__ constexpr int ximg_f_col(int J) { return 16 * (NB * J - 8 * J * (J - 1)); }      // first column of sub-block J
__host__ __device__ constexpr int ximg_b_col(int I) { return NB * I * (I + 1); }
static_assert(ximg_f_col(8) == XIMG_DOUBLES && ximg_b_col(8) == XIMG_DOUBLES, "packed image size");

// the column-major 128 x 128 image G (global) -> packed LDS image; all 1024 threads, 16 loads each in flight at once
// (load and store are separate calls so that the first tile loads of the sweep can be issued between them)
__device__ __forceinline__ void ximg_load(const double* __restrict__ G, int tid, double (&v)[16]) {
    const int r = tid & (NB - 1), cg = tid >> 7;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = G[(cg + 8 * i) * NB + r];
}
template <bool BWD>
__device__ __forceinline__ void ximg_store(const double (&v)[16], double* __restrict__ X, int tid) {
    const int r = tid & (NB - 1), cg = tid >> 7;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int B = i >> 1, ck = cg + 8 * (i & 1);  // sub-block and column inside it
        if (!BWD) {
            if (r >= 16 * B) X[ximg_f_col(B) + ck * (NB - 16 * B) + r - 16 * B] = v[i];
        } else {
            if (r < 16 * (B + 1)) X[ximg_b_col(B) + ck * 16 * (B + 1) + r] = v[i];
        }
    }
}

// Eight of the 16 values of sub-block g (lanes 16 g + 8 h .. + 7 of `src`) to every lane, as scalar operands: 16 read-lanes.
// (Through LDS instead -- one store of all 64 lanes, four 16-byte reads of one address each -- measured the same time
// per hop and costs registers: dropped.)
__device__ __forceinline__ void sweep_bcast8(double src, int g, int h, double (&b)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = readlane_f64(src, 16 * g + 8 * h + k);
}
// t0 = sum_k x0[k] b[k], t1 = sum_k x1[k] b[k] over the 16 columns of one sub-block (two partial sums each, fixed order);
// column k of the packed image at X + k * len (+ 64 for the second row of the lane); HAS0 / HAS1: which of the lane's two
// rows take part (compile time)
template <bool HAS0, bool HAS1>
__device__ __forceinline__ void sweep_dot16(const double* __restrict__ X, int len, double src, int g, int lane,
                                            double& t0, double& t1) {
    double t0a = 0.0, t0b = 0.0, t1a = 0.0, t1b = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double b[8], x0[8], x1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (HAS0) x0[k] = X[(8 * h + k) * len + lane];
            if (HAS1) x1[k] = X[(8 * h + k) * len + 64 + lane];
        }
        sweep_bcast8(src, g, h, b);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            if (HAS0) {
                t0a = __builtin_fma(x0[k], b[k], t0a);
                t0b = __builtin_fma(x0[k + 1], b[k + 1], t0b);
            }
            if (HAS1) {
                t1a = __builtin_fma(x1[k], b[k], t1a);
                t1b = __builtin_fma(x1[k + 1], b[k + 1], t1b);
            }
        }
    }
    t0 = t0a + t0b;
    t1 = t1a + t1b;
}
// wave 0: the 128 values of the diagonal step; lane l holds rows l (u0) and 64 + l (u1) on entry (v) and on return (z)
__device__ __forceinline__ double2_t sweep_diag_fwd(const double* __restrict__ X, int lane, double u0, double u1) {
    // (inlined, behind a compiler barrier: as a call the callee saves 48 registers to scratch on the chain; without the
    // barrier the image reads drift up into the streaming loop and its registers spill)
    asm volatile("" ::: "memory");
    const int I0 = lane >> 4;  // sub-block of row `lane`; row 64 + lane sits in sub-block 4 + I0
#pragma unroll
    for (int J = 0; J < 8; ++J) {
        const int len = NB - 16 * J;
        const double* Xj = X + ximg_f_col(J) - 16 * J;  // (lanes above sub-block J read a neighbour's entries: discarded)
        const double src = (J < 4) ? u0 : u1;
        double t0 = 0.0, t1 = 0.0;
        if (J < 4)
            sweep_dot16<true, true>(Xj, len, src, J & 3, lane, t0, t1);
        else
            sweep_dot16<false, true>(Xj, len, src, J & 3, lane, t0, t1);
        if (J < 4) {
            u0 = (I0 == J) ? t0 : (I0 > J) ? u0 - t0 : u0;
            u1 = u1 - t1;
        } else {
            u1 = (4 + I0 == J) ? t1 : (4 + I0 > J) ? u1 - t1 : u1;
        }
    }
    return double2_t{u0, u1};
}
__device__ __forceinline__ double2_t sweep_diag_bwd(const double* __restrict__ X, int lane, double u0, double u1) {
    // (inlined, behind a compiler barrier: as a call the callee saves 48 registers to scratch on the chain; without the
    // barrier the image reads drift up into the streaming loop and its registers spill)
    asm volatile("" ::: "memory");
    const int J0 = lane >> 4;  // sub-block of entry `lane`; entry 64 + lane: 4 + J0
#pragma unroll
    for (int I = 7; I >= 0; --I) {
        const int len = 16 * (I + 1);
        const double* Xi = X + ximg_b_col(I);  // (entries beyond sub-block I read a neighbour's column: discarded)
        const double src = (I < 4) ? u0 : u1;
        double t0 = 0.0, t1 = 0.0;
        if (I >= 4)
            sweep_dot16<true, true>(Xi, len, src, I & 3, lane, t0, t1);
        else
            sweep_dot16<true, false>(Xi, len, src, I & 3, lane, t0, t1);
        if (I >= 4) {
            u1 = (4 + J0 == I) ? t1 : (4 + J0 < I) ? u1 - t1 : u1;
            u0 = u0 - t0;
        } else {
            u0 = (J0 == I) ? t0 : (J0 < I) ? u0 - t0 : u0;
        }
    }
    return double2_t{u0, u1};
}

__global__ __launch_bounds__(256) void negate_kernel(double* __restrict__ v, int64_t len) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) v[i] = -v[i];
}

// REV: the same sweep on U = L' from the far end -- the backward substitution x = L^-T y as sums over the
// ROWS of U's blocks: block r of the chain is block nblk-1-r of the matrix, its sources lie to the right of the diagonal,
// the diagonal step is the backward one on the block's second image.  The mid-size factorisation leaves U in a buffer of
// its own (lower_to_upper_kernel); two accumulators per thread where the transposed product on L (trsv_bwd_sweep_kernel)
// needs sixteen and a column reduction through LDS per block: 3.3 us per hop instead of 4.3.  out: optional second copy
// of the solution (plain stores; the polled copy y may then be scratch memory).
template <bool REV = false>
__global__ __launch_bounds__(1024) void trsv_fwd_sweep_kernel(const double* __restrict__ L, int64_t lda,
                                                              const double* __restrict__ winv,
                                                              const double* __restrict__ b,
                                                              double* __restrict__ y, int64_t n,
                                                              int32_t* __restrict__ ctl, double* __restrict__ fault,
                                                              int vec, SweepPlan plan, double* __restrict__ out, int kb) {
    __shared__ double xs[2][NB];
    __shared__ double red[16][NB];
    __shared__ double ximg[XIMG_DOUBLES];
    __shared__ int s_r;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_r = atomicAdd(&ctl[REV ? 2 : 1], 1);
    __syncthreads();
    int r = s_r, c = 0;
    if (plan.jobs) {
        const int32_t job = plan.jobs[r];
        r = job & 0xFFFFF;
        c = job >> 20;
    }
    const BandSweepRange range = band_sweep_range(r, c, plan.chunk, kb, plan.jobs != nullptr);  // (band_plan.inc)
    const int j0 = range.j0, j1 = range.j1, clo = range.clo;
    const bool owner = range.owner;
    const int rl = r;  // the block's place in the chain (partial sums are filed under it)
    const int nblk = (int)((n + NB - 1) / NB);
    if (REV) r = nblk - 1 - r;  // from here on r is the block of the matrix
    const int64_t row0 = (int64_t)r * NB;
    const int w = (int)((n - row0 < NB) ? (n - row0) : NB);
    const bool ok0 = row0 + 2 * lane < n, ok1 = row0 + 2 * lane + 1 < n;
    // this block's image (16 x 16 inverses on the diagonal, normalised sub-blocks off it; REV: the second of its pair) packed into LDS
    double xv[16];
    if (owner) ximg_load(winv + (int64_t)r * WBLK + (REV ? NB * NB : 0), tid, xv);
    double a0 = 0.0, a1 = 0.0;
    const double* Lr = L + row0 + 2 * lane + (int64_t)(wave * 4) * lda;  // this thread's corner of tile (r, 0)
    auto col = [&](int j) { return (int64_t)(REV ? nblk - 1 - j : j) * NB * lda; };  // tile column of source j of the chain
    double2_t A[4], B[4];
    if (j1 > j0) sweep_load_half(Lr + col(j0), lda, ok0, ok1, vec, A);
    if (owner) ximg_store<REV>(xv, ximg, tid);  // (visible to wave 0 after any later barrier)
    // the right-hand side of this block, fetched NOW: read behind the last barrier it is an L2 round trip on every hop
    double b0 = 0.0, b1 = 0.0;
    if (owner) {
        b0 = lane < w ? b[row0 + lane] : 0.0;
        b1 = 64 + lane < w ? b[row0 + 64 + lane] : 0.0;
    }
    for (int j = j0; j < j1; ++j) {
        const double* Tj = Lr + col(j);
        sweep_load_half(Tj + 64 * lda, lda, ok0, ok1, vec, B);
        if (wave == 0) sweep_poll_block(y, REV ? nblk - 1 - j : j, n, xs[j & 1], fault, lane);
        __syncthreads();
        const double* xj = xs[j & 1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xv = xj[wave * 4 + q];
            a0 = __builtin_fma(A[q].x, xv, a0);
            a1 = __builtin_fma(A[q].y, xv, a1);
        }
        if (j + 1 < j1) sweep_load_half(Lr + col(j + 1), lda, ok0, ok1, vec, A);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xv = xj[64 + wave * 4 + q];
            a0 = __builtin_fma(B[q].x, xv, a0);
            a1 = __builtin_fma(B[q].y, xv, a1);
        }
    }
    red[wave][2 * lane] = a0;
    red[wave][2 * lane + 1] = a1;
    __syncthreads();
    if (!owner) {
        if (tid < NB) {
            double sum = red[0][tid];
#pragma unroll
            for (int q = 1; q < 16; ++q) sum += red[q][tid];
            st_sc1_f64(plan.part + ((int64_t)rl * plan.maxc + c) * NB + tid, sum);
        }
        return;
    }
    if (wave != 0) return;  // (the image was complete before the first barrier of this workgroup)
    // wave 0 alone from here: the sums over the 16 waves for its two rows (the same order as above), no second barrier
    double s0 = red[0][lane], s1 = red[0][64 + lane];
#pragma unroll
    for (int q = 1; q < 16; ++q) {
        s0 += red[q][lane];
        s1 += red[q][64 + lane];
    }
    double far0, far1;  // the partial sums of this block's other jobs, in column order
    sweep_far2(plan.part + (int64_t)rl * plan.maxc * NB, clo, c, lane, fault, far0, far1);
    const double u0 = lane < w ? b0 - (far0 + s0) : 0.0, u1 = 64 + lane < w ? b1 - (far1 + s1) : 0.0;
    const double2_t z = REV ? sweep_diag_bwd(ximg, lane, u0, u1) : sweep_diag_fwd(ximg, lane, u0, u1);
    if (lane < w) st_sc1_f64(y + row0 + lane, z.x);
    if (64 + lane < w) st_sc1_f64(y + row0 + 64 + lane, z.y);
    if (out) {
        if (lane < w) out[row0 + lane] = z.x;
        if (64 + lane < w) out[row0 + 64 + lane] = z.y;
    }
}

// U = L' for the tiles strictly below the diagonal blocks (64 x 64 pieces through LDS; rows of L at or beyond n give zeros:
// the sweep on U multiplies those columns with zeros and must not meet a NaN there)
__global__ __launch_bounds__(256) void lower_to_upper_kernel(const double* __restrict__ A, int64_t lda, int64_t n,
                                                            double* __restrict__ U, int64_t ldu) {
    const int i = blockIdx.x, j = blockIdx.y;  // 64-blocks: source rows i, source columns j
    if ((i >> 1) <= (j >> 1)) return;
    __shared__ double tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r = (int64_t)i * 64 + tx;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int c = ty + 4 * q;
        tile[c][tx] = r < n ? A[r + ((int64_t)j * 64 + c) * lda] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int rr = ty + 4 * q;  // source row inside the piece = destination column
        U[(int64_t)j * 64 + tx + ((int64_t)i * 64 + rr) * ldu] = tile[tx][rr];
    }
}
// the scratch vectors of a solve <- sentinel, the sweeps' ticket counters <- 0: one launch per solve instead of three fills
__global__ __launch_bounds__(256) void sweep_prep_kernel(unsigned long long* __restrict__ v, int64_t len, int32_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x < 3) ctl[1 + threadIdx.x] = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) v[i] = SWEEP_SENTINEL;
}

__global__ __launch_bounds__(1024) void trsv_bwd_sweep_kernel(const double* __restrict__ L, int64_t lda,
                                                              const double* __restrict__ winv,
                                                              const double* __restrict__ y,
                                                              double* __restrict__ x, int64_t n,
                                                              int32_t* __restrict__ ctl, double* __restrict__ fault,
                                                              int vec, SweepPlan plan, int kb) {
    __shared__ double xs[2][NB];
    __shared__ double vs[NB];
    __shared__ double colred[NB][65];  // column-sum staging, padded against bank conflicts
    __shared__ double ximg[XIMG_DOUBLES];
    __shared__ int s_r;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (int)((n + NB - 1) / NB);
    if (tid == 0) s_r = atomicAdd(&ctl[2], 1);
    __syncthreads();
    // block nblk-1-rr has rr tiles below its diagonal block; the job takes tiles k0 .. k1-1 counted from the last row
    int rr = s_r, c = 0;
    if (plan.jobs) {
        const int32_t job = plan.jobs[rr];
        rr = job & 0xFFFFF;
        c = job >> 20;
    }
    const BandSweepRange range = band_sweep_range(rr, c, plan.chunk, kb, plan.jobs != nullptr);  // in chain coordinates
    const int k0 = range.j0, k1 = range.j1, clo = range.clo;
    const bool owner = range.owner;
    const int r = nblk - 1 - rr;
    const int64_t col0 = (int64_t)r * NB;
    const int w = (int)((n - col0 < NB) ? (n - col0) : NB);
    // this block's backward image (the second one of its pair) packed into LDS
    double xv[16];
    if (owner) ximg_load(winv + (int64_t)r * WBLK + NB * NB, tid, xv);
    // this thread's columns: col0 + h*64 + wave*4 + q; rows 2*lane, 2*lane+1 of the row block j
    double acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[h][q] = 0.0;
    const double* Lc = L + 2 * lane + (col0 + wave * 4) * lda;  // + row block offset
    double2_t A[4], B[4];
    const int jhi = nblk - 1 - k0, jlo = nblk - 1 - k1;  // row blocks jhi, jhi-1, .., jlo+1
    auto rows_ok = [&](int j, bool& o0, bool& o1) {
        const int64_t i0 = (int64_t)j * NB + 2 * lane;
        o0 = i0 < n;
        o1 = i0 + 1 < n;
    };
    // (the columns of block r all exist whenever it has tiles: only the last block can be short)
    if (jhi > jlo) {
        bool o0, o1;
        rows_ok(jhi, o0, o1);
        sweep_load_half(Lc + (int64_t)jhi * NB, lda, o0, o1, vec, A);
    }
    if (owner) ximg_store<true>(xv, ximg, tid);
    double y0 = 0.0, y1 = 0.0;  // this block of the right-hand side, fetched now (see the forward kernel)
    if (owner) {
        y0 = lane < w ? y[col0 + lane] : 0.0;
        y1 = 64 + lane < w ? y[col0 + 64 + lane] : 0.0;
    }
    for (int j = jhi; j > jlo; --j) {
        bool o0, o1;
        rows_ok(j, o0, o1);
        const double* Tj = Lc + (int64_t)j * NB;
        sweep_load_half(Tj + 64 * lda, lda, o0, o1, vec, B);
        if (wave == 0) sweep_poll_block(x, j, n, xs[j & 1], fault, lane);
        __syncthreads();
        const double x0 = xs[j & 1][2 * lane], x1 = xs[j & 1][2 * lane + 1];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[0][q] = __builtin_fma(A[q].y, x1, __builtin_fma(A[q].x, x0, acc[0][q]));
        if (j - 1 > jlo) {
            bool p0, p1;
            rows_ok(j - 1, p0, p1);
            sweep_load_half(Tj - NB, lda, p0, p1, vec, A);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[1][q] = __builtin_fma(B[q].y, x1, __builtin_fma(B[q].x, x0, acc[1][q]));
    }
    // column sums over the 64 lanes, then v = y_r - sums.  Through LDS (a 64-lane shuffle butterfly per column put
    // 48 dependent cross-lane operations on the hand-off chain: the backward hop was 6.1 us against 2.6 us forward):
    // every thread parks its 8 partial sums, then 8 threads per column add 8 lanes each and finish with three
    // steps inside their group of 8 lanes.  Fixed order: the same result on every run.
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) colred[h * 64 + wave * 4 + q][lane] = acc[h][q];
    __syncthreads();
    {
        const int cl = tid >> 3, part = tid & 7;
        double t = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += colred[cl][part * 8 + u];
        t += __shfl_down(t, 4, 8);
        t += __shfl_down(t, 2, 8);
        t += __shfl_down(t, 1, 8);
        if (part == 0) vs[cl] = t;
    }
    __syncthreads();
    if (!owner) {
        if (tid < NB) st_sc1_f64(plan.part + ((int64_t)rr * plan.maxc + c) * NB + tid, vs[tid]);
        return;
    }
    if (wave != 0) return;  // wave 0 alone from here, no further barrier
    double far0, far1;
    sweep_far2(plan.part + (int64_t)rr * plan.maxc * NB, clo, c, lane, fault, far0, far1);
    const double u0 = lane < w ? y0 - (far0 + vs[lane]) : 0.0, u1 = 64 + lane < w ? y1 - (far1 + vs[64 + lane]) : 0.0;
    const double2_t z = sweep_diag_bwd(ximg, lane, u0, u1);
    if (lane < w) st_sc1_f64(x + col0 + lane, z.x);
    if (64 + lane < w) st_sc1_f64(x + col0 + 64 + lane, z.y);
}

// ---- panel solve for ONE 128-column block by BLOCK SUBSTITUTION: L[rows, blk] = C[rows, blk] L_kk^-T --------------------
// Multiplying the panel by the explicit inverse of the 128 x 128 diagonal block (rounds 1-3, removed) costs
// cond(L_kk) in the backward error of the factorisation where LAPACK's dtrsm substitutes (tools/numerics/
// blockchol_emul.py: on condensed LPs the device's distance from LAPACK has a tail of tens of times the distance between
// two CPU executions, and neither a correctly rounded inverse nor a Newton-Schulz step removes it -- it is the product
// with ANY stored 128-inverse).  Here the solve runs over the eight 16-column sub-blocks, and only the inverses of the
// 16 x 16 DIAGONAL sub-blocks are multiplied with (statistically indistinguishable from scalar substitution in the same
// emulation).  With Z = X' (128 x rows):
//     Z_J = W_JJ (C'_J - sum_{I<J} L_JI Z_I),      W_JJ = (L_kk)_JJ^-1 = the diagonal 16 x 16 block of the stored inverse
// on the MFMA unit, entirely in registers: D[m][n] += A[m][k] B[k][n] with m = row inside sub-block J, n = one of 16
// matrix rows, k = index inside sub-block I; the accumulator layout (lane l, register v: m = (l>>4) + 4v, n = l&15) IS the
// B-operand layout of k-step v, so a finished Z_I feeds the updates of the later sub-blocks as it stands.  A-operands
// (tiles of L_kk, W_JJ) come straight from L2, two steps ahead.  The same 144 MFMAs per 16 rows as the inverse product
// with its zero half skipped.  A wave owns 16 rows; in place is safe (it reads only the rows it writes, all up front).
struct PanelBatch {  // problem blockIdx.y: pointer strides (doubles); skip[b] != 0: leave untouched
    int64_t sC, sL, sW;
    const int32_t* skip;
    const int32_t* list = nullptr;   // compacted form (GemmBatch::list)
    const int32_t* count = nullptr;
};
template <int J>
__device__ __forceinline__ void ps16_load(const double* __restrict__ Lq, int64_t ldl, const double* __restrict__ Wq,
                                          double (&aw)[4], double (&al)[7][4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) aw[s] = -Wq[16 * J + (16 * J + 4 * s) * NB];  // -W_JJ: Z_J = (-W_JJ) u_J with u = -(C' - ..)
#pragma unroll
    for (int d = 0; d < 7; ++d)
        if (J + 1 + d < 8) {
#pragma unroll
            for (int s = 0; s < 4; ++s) al[d][s] = Lq[16 * (J + 1 + d) + (int64_t)(16 * J + 4 * s) * ldl];
        }
}
template <int J>
__device__ __forceinline__ void ps16_step(double4_t (&z)[8], const double (&aw)[4], const double (&al)[7][4]) {
    double4_t t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) t = __builtin_amdgcn_mfma_f64_16x16x4f64(aw[s], z[J][s], t, 0, 0, 0);
    z[J] = t;  // Z_J
#pragma unroll
    for (int d = 0; d < 7; ++d)
        if (J + 1 + d < 8) {
#pragma unroll
            for (int s = 0; s < 4; ++s)  // u_J2 += L_{J2,J} Z_J
                z[J + 1 + d] = __builtin_amdgcn_mfma_f64_16x16x4f64(al[d][s], t[s], z[J + 1 + d], 0, 0, 0);
        }
}
__device__ __forceinline__ void panel_sub16_body(double* __restrict__ C, int64_t ld, const double* __restrict__ Lkk,
                                                 int64_t ldl, const double* __restrict__ Wcm, int64_t rows, int64_t rows_read) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lo = lane & 15, hi = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * 64 + wave * 16;
    if (i0 >= rows) return;  // (no barrier in this kernel)
    const int64_t gi = i0 + lo;
    const int64_t gir = gi < rows_read ? gi : rows_read - 1;  // rows that may be read: up to the padded order when it exists
    double* Cp = C + gir + (int64_t)hi * ld;
    const double* Lq = Lkk + lo + (int64_t)hi * ldl;
    const double* Wq = Wcm + lo + hi * NB;
    double aw[3][4], al[3][7][4];
    ps16_load<0>(Lq, ldl, Wq, aw[0], al[0]);
    ps16_load<1>(Lq, ldl, Wq, aw[1], al[1]);
    double4_t z[8];  // u_J = -(C'_J - ..) until step J, Z_J afterwards: element (16J + hi + 4v, row gi)
#pragma unroll
    for (int J = 0; J < 8; ++J)
#pragma unroll
        for (int v = 0; v < 4; ++v) z[J][v] = -Cp[(int64_t)(16 * J + 4 * v) * ld];
    ps16_load<2>(Lq, ldl, Wq, aw[2], al[2]);
    ps16_step<0>(z, aw[0], al[0]);
    ps16_load<3>(Lq, ldl, Wq, aw[0], al[0]);
    ps16_step<1>(z, aw[1], al[1]);
    ps16_load<4>(Lq, ldl, Wq, aw[1], al[1]);
    ps16_step<2>(z, aw[2], al[2]);
    ps16_load<5>(Lq, ldl, Wq, aw[2], al[2]);
    ps16_step<3>(z, aw[0], al[0]);
    ps16_load<6>(Lq, ldl, Wq, aw[0], al[0]);
    ps16_step<4>(z, aw[1], al[1]);
    ps16_load<7>(Lq, ldl, Wq, aw[1], al[1]);
    ps16_step<5>(z, aw[2], al[2]);
    ps16_step<6>(z, aw[0], al[0]);
    ps16_step<7>(z, aw[1], al[1]);
    if (gi < rows) {
        double* Co = C + gi + (int64_t)hi * ld;
#pragma unroll
        for (int J = 0; J < 8; ++J)
#pragma unroll
            for (int v = 0; v < 4; ++v) Co[(int64_t)(16 * J + 4 * v) * ld] = z[J][v];
    }
}

__global__ __launch_bounds__(256) void panel_sub16_kernel(double* __restrict__ C, int64_t ld, const double* __restrict__ Lkk,
                                                          int64_t ldl, const double* __restrict__ Wcm, int64_t rows,
                                                          int64_t rows_read, PanelBatch bt) {
    if (bt.list) {  // compacted batch: the problems of slot blockIdx.y, one after the other (no barrier in the body)
        const int cnt = *bt.count;
        for (int pb = blockIdx.y; pb < cnt; pb += gridDim.y) {
            const int64_t b = bt.list[pb];
            panel_sub16_body(C + b * bt.sC, ld, Lkk + b * bt.sL, ldl, Wcm + b * bt.sW, rows, rows_read);
        }
        return;
    }
    if (gridDim.y > 1 || bt.skip) {
        const int64_t b = blockIdx.y;
        if (bt.skip && bt.skip[b] != 0) return;
        C += b * bt.sC;
        Lkk += b * bt.sL;
        Wcm += b * bt.sW;
    }
    panel_sub16_body(C, ld, Lkk, ldl, Wcm, rows, rows_read);
}

// ---- mid-size factorisation: right-looking, two launches per 128-column block ---------------------------------
// Below n ~ 10 000 the left-looking schedule above is a chain of short dependent launches (per block: update with
// split-K, its reduction, the diagonal kernel, panel times inverse -- 120 us, of which the matrix pipes are busy a
// fraction).  Here step k is
//   chol_mid_step_kernel  trailing tiles (i, j), k <= j <= i, receive pending updates C_ij -= L_i,p L_j,p' -- which tiles,
//                         with which panels p < k, the plan of the handle decides (see "which trailing columns a block
//                         step visits" further down; K = 128 per panel, no split-K; a tile accumulates its panels in the
//                         order 0, 1, .., so the factor has the same bits under every plan) --, and workgroup 0 gives the
//                         diagonal tile (k, k) its last panel (mid_diag_syrk) and factors it without leaving the CU;
//   panel solve           L_ik = C_ik L_kk^-T (madqp_chol_panel_solve).
// Workgroups have 512 threads and the diagonal kernel's LDS (one per CU).  (The schedules of rounds 3-4 that this one
// replaced -- every panel in every step, two panels every second step, the diagonal tile through the GEMM loop -- were
// removed; their numbers: DESIGN.md 5.2.)
struct MidArgs {
    double* A;
    int64_t lda, n;
    int32_t nblk, k;
    const uint32_t* plan;  // the units of this step (mid_plan_build, mid_plan.inc)
    double* winv;
    int32_t* info;
};
#ifdef MADQP_MID_STAMPS
__device__ unsigned long long madqp_mid_stamps[64][24];  // diagnostic build only (tools/mid_probe.cpp)
#define MID_STAMP(slot)                                                                                              \
    do {                                                                                                             \
        if (threadIdx.x == 0 && blockIdx.x <= 2)                                                                     \
            madqp_mid_stamps[a.k & 63][8 * blockIdx.x + (slot)] = __builtin_amdgcn_s_memrealtime();                  \
    } while (0)
#else
#define MID_STAMP(slot)
#endif
constexpr int MID_THREADS = 512;

// ---- the diagonal workgroup's own update (round 4): S <- C_kk - R R' with R = L[block row k, panel k-1] ------------------
// Through the GEMM main loop (one 128 x 128 tile on four waves, K = 128 in eight stages with ONE stage of prefetch) this
// took 18-22 us of the ~56 us chain of a block step (tools/mid_probe): a single workgroup has nobody to hide the latency of
// its eight dependent stage loads behind, and it computes all 64 sub-tiles where potf2 reads 36.  Here the whole operand
// (128 KB: both operands of a SYRK are the same block row) is fetched at once -- every load of the workgroup in flight
// together, one latency -- into a k-major LDS image, all eight waves take the 36 lower 16 x 16 sub-tiles (a row pair
// I, 7-I per two waves: nine tiles sharing their fragments), and the result goes straight to the LDS image of potf2.
// D'[m][n] = sum_k R(16 J + m, k) R(16 I + n, k): A-operand <- fragment of block row J, B-operand <- block row I, so lane l holds
// element (row 16 I + (l & 15), column 16 J + (l >> 4) + 4 v): rows are the fast index of every global and LDS access.
constexpr int XS_LD = 144;  // k-row stride of the operand image (= 16 mod 32: the two k-rows of a half-wave read hit disjoint banks)
static_assert(NB * XS_LD <= P2_S_DOUBLES + P2_WD_DOUBLES, "the operand image fits the diagonal kernel's LDS");
#ifdef MADQP_MID_STAMPS
#define DS_STAMP(slot)                                                                                   \
    do {                                                                                                 \
        if (threadIdx.x == 0) madqp_mid_stamps[kstep & 63][(slot)] = __builtin_amdgcn_s_memrealtime();   \
    } while (0)
#else
#define DS_STAMP(slot)
#endif
__device__ __forceinline__ void mid_diag_syrk(const double* __restrict__ Ckk, const double* __restrict__ R, int64_t lda, int nb,
                                              double* __restrict__ smem, int kstep) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 15, hi = lane >> 4;
    // this wave's tiles: row pair (p, 7 - p) has 9 lower tiles, waves 2p / 2p + 1 take the first 5 / last 4 of them
    const int p = wave >> 1, first = (wave & 1) ? 5 : 0, cnt = (wave & 1) ? 4 : 5;
    int tI[5], tJ[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        int q = first + (u < cnt ? u : cnt - 1);  // (a short list repeats its last tile; not stored twice)
        // tiles of the pair in order: (p, 0..p), then (7-p, 0..7-p)
        tI[u] = (q <= p) ? p : 7 - p;
        tJ[u] = (q <= p) ? q : q - (p + 1);
    }
    // 1. the operand: 16 x 16-byte loads per thread, all in flight; pair index e = tid + 512 q: column c = e / 64, rows 2 (e % 64)
    double2_t rv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = tid + MID_THREADS * q, c = e >> 6, i = 2 * (e & 63);
        rv[q] = *reinterpret_cast<const double2_t*>(R + i + (int64_t)c * lda);
    }
    // 2. the tile itself, negated (the products are added, the result is negated back): element (r = 16 I + lo, c = 16 J + hi + 4 v)
    double4_t acc[5];
#pragma unroll
    for (int u = 0; u < 5; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            int c = 16 * tJ[u] + hi + 4 * v;
            c = c < nb ? c : nb - 1;  // (columns beyond the order need not exist in the caller's buffer: any value will do)
            acc[u][v] = -Ckk[(16 * tI[u] + lo) + (int64_t)c * lda];
        }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = tid + MID_THREADS * q, c = e >> 6, i = 2 * (e & 63);
        *reinterpret_cast<double2_t*>(smem + c * XS_LD + i) = rv[q];
    }
    __syncthreads();
    DS_STAMP(4);
    const double* xa[5];
    const double* xb[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        xa[u] = smem + hi * XS_LD + 16 * tJ[u] + lo;  // A[m = lo][k = hi + 4 s] = R(16 J + lo, 4 s + hi)
        xb[u] = smem + hi * XS_LD + 16 * tI[u] + lo;  // B[k = hi + 4 s][n = lo] = R(16 I + lo, 4 s + hi)
    }
#pragma unroll 2
    for (int s4 = 0; s4 < 32; ++s4) {
#pragma unroll
        for (int u = 0; u < 5; ++u)
            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u][4 * s4 * XS_LD], xb[u][4 * s4 * XS_LD], acc[u], 0, 0, 0);
    }
    DS_STAMP(5);
    __syncthreads();  // every wave has read its fragments: the image becomes potf2's S[c * LDS_LD + r]
    DS_STAMP(6);
    // 3. lower tiles -> S (upper triangle of the diagonal sub-tiles zero, identity beyond the order of a short last block);
    //    the strictly upper sub-tiles, which nobody computes, the factor-only diagonal kernel never touches
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        if (u >= cnt) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = 16 * tI[u] + lo, c = 16 * tJ[u] + hi + 4 * v;
            double x = -acc[u][v];
            if (r >= nb || c >= nb) x = (r == c) ? 1.0 : 0.0;
            smem[c * LDS_LD + r] = (r >= c) ? x : 0.0;
        }
    }
    __syncthreads();
}

// Workgroup 0: the diagonal tile (k, k).  Workgroup 1 + u: unit u of this step's list (mid_plan_build) -- one trailing tile
// (row, column) and the panels it receives in one product, on waves 0-3 like one workgroup of gemm_tn_f64_kernel; the
// other four waves keep its barriers company.  (Measured and dropped: two units per workgroup in the steps of more than
// one round of tiles -- 6.15 against 5.77 ms per factorisation at n = 8 000.)
__global__ __launch_bounds__(MID_THREADS) void chol_mid_step_kernel(MidArgs a) {
    __shared__ __attribute__((aligned(16))) double smem[P2_S_DOUBLES + P2_WD_DOUBLES];
    static_assert(P2_S_DOUBLES + P2_WD_DOUBLES >= 4 * TILE_DOUBLES, "the GEMM stages fit the diagonal kernel's LDS");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k;
    MID_STAMP(0);
    if (blockIdx.x == 0) {
        // C_kk - R R' -> the LDS image S[c*LDS_LD + r] (lower triangle, identity padding) -> factor
        const int64_t i0 = (int64_t)k * NB;
        const int nb = (int)((a.n - i0 < NB) ? (a.n - i0) : NB);
        double* Akk = a.A + i0 + i0 * a.lda;
        if (k > 0) mid_diag_syrk(Akk, a.A + i0 + (int64_t)(k - 1) * NB * a.lda, a.lda, nb, smem, k);
        MID_STAMP(1);
        MID_STAMP(2);
        double* Wcm = a.winv + (int64_t)k * WBLK;
        potf2_inv_body<MID_THREADS, 1>(Akk, a.lda, nb, Wcm, Wcm + NB * NB, a.info, (int32_t)i0, smem, smem + P2_S_DOUBLES,
                                       /*tile_in_lds=*/k > 0);
        MID_STAMP(3);
        return;
    }
    // (a step has units only once there are panels: k > 0)
    const uint32_t e = a.plan[(int)blockIdx.x - 1];
    // wave-uniform: the LDS-DMA rows are addressed from scalar registers
    const int bi = __builtin_amdgcn_readfirstlane((int)(e & 255u));
    const int bj = __builtin_amdgcn_readfirstlane((int)((e >> 8) & 255u));
    const int pan0 = __builtin_amdgcn_readfirstlane((int)((e >> 16) & 255u));
    const int kpan = __builtin_amdgcn_readfirstlane((int)(e >> 24));
    const int64_t i0 = (int64_t)bi * NB, j0 = (int64_t)bj * NB;
    if (wave >= 4) {
        const int nbar = kpan * (NB / BK) + 1;
        for (int b = 0; b < nbar; ++b) __builtin_amdgcn_s_barrier();
        return;
    }
    const int wi = wave & 1, wj = wave >> 1;
    const int lo = lane & 15, hi = lane >> 4;
    GemmArgs g{};
    g.X = a.A + (int64_t)pan0 * NB * a.lda;  // kpan panels from pan0 on: their columns are contiguous
    g.Y = g.X;
    g.ldx = g.ldy = a.lda;
    g.M = g.N = a.n;
    g.Mread = g.Nread = (int64_t)a.nblk * NB;
    g.K = kpan * NB;
    // the accumulators start at -C_ij (loads in flight while the first stage is staged; rows up to the padded
    // order exist, what lies beyond n or above the diagonal is never stored) and come back negated
    double4_t acc[4][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                int64_t gj = j0 + wj * 64 + tj * 16 + hi + 4 * v;
                gj = (gj < a.n) ? gj : a.n - 1;  // columns beyond n: any value will do, no branch
                acc[ti][tj][v] = -a.A[i0 + wi * 64 + ti * 16 + lo + gj * a.lda];
            }
    mainloop_dma(g, i0, j0, smem, wi, wj, lane, wave, acc);
    MID_STAMP(1);
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int64_t gi = i0 + wi * 64 + ti * 16 + lo;
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t gj = j0 + wj * 64 + tj * 16 + hi + 4 * v;
                if (gi < a.n && gj < a.n && gi >= gj) a.A[gi + gj * a.lda] = -acc[ti][tj][v];
            }
        }
    }
    MID_STAMP(7);
}

}  // namespace

// ---- the parameters and fallback switches of this file, read from the environment in ONE place ----
struct CholModes {
    bool sweep_upper;  // MADQP_SWEEP_UPPER (1): backward sweep of a mid-size factor on U = L'
    int32_t sweep_chunk;      // MADQP_SWEEP_CHUNK (64): tiles of a block row per sweep job
    bool sweep_band;          // MADQP_SWEEP_BAND (1): under a bandwidth the sweeps stay inside the band; 0: whole block rows
    int64_t mid_max;          // MADQP_CHOL_MID_MAX (13312): largest order of the mid-size schedule
    int mid_cap;              // MADQP_CHOL_MID_CAP (0 = from the CU count; experiments)
    int64_t wt_min, wt_max;   // MADQP_CHOL_WMIN / WMAX (6, 20): outer panel width in blocks
    int64_t band_w;           // MADQP_CHOL_BAND_W (0 = the rule of chol_plan.inc): outer panel in blocks where a band limits it
};
static CholModes chol_modes_from_env() {
    auto num = [](const char* name, int64_t dflt) { return getenv(name) ? atoll(getenv(name)) : dflt; };
    auto on = [&](const char* name) { return num(name, 1) != 0; };
    CholModes m{};
    m.sweep_upper = on("MADQP_SWEEP_UPPER");
    m.sweep_chunk = (int32_t)std::max<int64_t>(1, num("MADQP_SWEEP_CHUNK", 64));
    m.sweep_band = on("MADQP_SWEEP_BAND");
    m.mid_max = num("MADQP_CHOL_MID_MAX", 13312);
    m.mid_cap = (int)num("MADQP_CHOL_MID_CAP", 0);
    m.wt_min = num("MADQP_CHOL_WMIN", 6);
    m.wt_max = num("MADQP_CHOL_WMAX", 20);
    m.band_w = std::max<int64_t>(0, num("MADQP_CHOL_BAND_W", 0));
    return m;
}
static const CholModes& chol_modes() {  // filled once, at the first use
    static const CholModes m = chol_modes_from_env();
    return m;
}

// ---- the handle --------------------------------------------------------------------------------------------------------
// The band state of a Cholesky handle (madqp_chol_set_bandwidth, madqp_chol_set_packed; band_plan.inc), cleared
// (chol.hip: band_clear) and committed as one
struct madqp_chol_band {
    int64_t bw = -1;      // half-bandwidth (-1: none, the dense schedules and sweeps)
    int64_t extent = 0;   // of the plan: the largest i - j the factorisation touches; n - 1 without a band
    bool packed = false;  // packed band storage: the lda of a factorisation is the packed leading dimension (>= extent)
    // the sweeps under the band (MADQP_SWEEP_BAND): blocks a block row reads left of its diagonal block (-1: the dense
    // sweeps), and the band's own job list where the dense sweeps have one
    int64_t sweep_kb = -1;
    int32_t* d_jobs = nullptr;
    int32_t njobs = 0;
};
// The plan of the mid-size schedule (chol.hip: mid_plan_build): which trailing tiles each block step updates, with which
// panels; built at the first factorisation that asks for it
struct MidPlan {
    int32_t state = 0;                  // 0 not built, 1 in use, -1 no plan (the left-looking schedule runs)
    std::vector<int32_t> count, first;  // per step: its number of units, and where they start in d_units
    uint32_t* d_units = nullptr;        // the packed units of all steps (mid_plan.inc)
};

struct madqp_chol {
    madqp_ctx* ctx = nullptr;
    int64_t n = 0;
    DevOwner mem;            // every device buffer below is this owner's
    double* winv = nullptr;  // ceil(n/128) blocks of 128x128 (col-major, ld 128): inverse diagonal blocks
    // The scratch of a solve, one buffer: [x | y | partial-sum slots of the forward sweep | of the backward sweep].  A solve
    // on L fills and uses the tmp_len doubles from y on (y: its intermediate vector); a solve with U = L' the utmp_len
    // doubles from x on (x: the polled copy of its solution), filled by one kernel.  sweep_x == nullptr: the buffer starts
    // at y, no solve of this handle runs on U (one block, or more than 160).
    double* sweep_x = nullptr;
    double* sweep_y = nullptr;
    int64_t tmp_len = 0, utmp_len = 0;
    int32_t* d_jobs = nullptr;  // sweep job list (chol.hip SweepPlan), nullptr when every block row is one job
    int32_t sweep_chunk = 0, sweep_maxc = 0, sweep_njobs = 0;
    bool sweep_band = false;  // MADQP_SWEEP_BAND of this handle: under a bandwidth the sweeps stay inside the band
    madqp_chol_band band;
    // the left-looking plan for the current (bandwidth, npos) (chol_plan.inc; chol.hip: handle_plan); empty: not built, or none needed yet
    std::vector<CholOp> plan;
    int32_t* d_info = nullptr;  // [0] info, [1..2] sweep tickets
    // the last matrix handed to a factorisation (borrowed; chol.hip: adopt_matrix) -- nullptr: none, or forgotten
    // (forget_factor), and the solves refuse with MADQP_ERR_STATE.  Whether that factorisation succeeded is the caller's
    // knowledge, not the handle's.
    double* A = nullptr;
    int64_t lda = 0;
    int64_t npos = 0;  // quasi-definite mode (madqp_chol_set_signature): A = L diag(I_npos, -I) L'; npos == n: Cholesky
    MidPlan mid;
    // the backward sweep on U = L' (chol.hip, trsv_fwd_sweep_kernel<true>): U of the last mid-size factorisation (order
    // npad, allocated at the first one)
    double* upper = nullptr;
    int64_t upper_ld = 0;
    bool upper_ok = false;  // the last factorisation left U
    // madqp_chol_solve_many: the transposed block of right-hand sides and, without U, the strip of one block row of L'
    // (solve_plan.inc: solve_plan_workspace), grown at the first call that needs more; from many_min right-hand sides on
    // the call takes the blocked path
    double* many_ws = nullptr;
    int64_t many_ws_len = 0;
    int64_t many_min = 0;  // (madqp_chol_create: the measured default)
};

// back to "no band"; frees the band's job list, which nothing on the stream may still read
static hipError_t band_clear(madqp_chol* s) {
    const hipError_t e = s->mem.free_one(&s->band.d_jobs);
    s->band = madqp_chol_band{};
    s->band.extent = s->n - 1;
    return e;
}
// What every factor entry point does with its matrix: lda has to cover the storage form (the order, or the extent of packed
// band storage), and what an earlier factorisation left beside the matrix (U) is void
static int32_t adopt_matrix(madqp_chol* s, double* A, int64_t lda) {
    ARG_TRY(s->ctx, A && lda >= (s->band.packed ? std::max<int64_t>(s->band.extent, 1) : s->n));
    s->A = A;
    s->lda = lda;
    s->upper_ok = false;
    return MADQP_OK;
}
// what is stored is no factor for the handle's new settings: the solves refuse until the next factorisation
static void forget_factor(madqp_chol* s) {
    s->A = nullptr;
    s->upper_ok = false;
}

extern "C" int32_t madqp_chol_create(madqp_ctx* ctx, int64_t n, madqp_chol** out) {
    ARG_TRY(ctx, ctx && out && n >= 0);
    *out = nullptr;
    madqp_chol* s = new (std::nothrow) madqp_chol();
    if (!s) return madqp_fail(ctx, MADQP_ERR_ALLOC, "host allocation failed");
    s->ctx = s->mem.ctx = ctx;
    s->n = s->npos = n;
    s->band.extent = n - 1;
    s->many_min = SOLVE_MANY_MIN_DEFAULT;
    const int64_t nblk = std::max<int64_t>(1, (n + NB - 1) / NB);
    // sweeps: block rows longer than `chunk` tiles are streamed by several workgroups (SweepPlan)
    const CholModes md = chol_modes_from_env();  // (read per handle: the tests build job lists with several chunks)
    s->sweep_chunk = md.sweep_chunk;
    s->sweep_band = md.sweep_band;
    std::vector<int32_t> jobs;
    if (nblk - 1 > s->sweep_chunk && nblk < (1 << 20)) {
        s->sweep_maxc = (int32_t)band_sweep_jobs(nblk, -1, s->sweep_chunk, jobs);
        s->sweep_njobs = (int32_t)jobs.size();
    }
    s->tmp_len = nblk * NB + 2 * nblk * (int64_t)s->sweep_maxc * NB;
    s->utmp_len = nblk * NB + s->tmp_len;
    const bool with_x = nblk > 1 && nblk <= 160;  // (the orders a mid-size factorisation may leave U for)
    const char* who = "madqp_chol_create";
    auto hip_ok = [&](hipError_t e) {
        return e == hipSuccess ? MADQP_OK : madqp_fail(ctx, MADQP_ERR_ALLOC, "madqp_chol_create(%lld): %s", (long long)n, hipGetErrorString(e));
    };
    int32_t r = s->mem.alloc(&s->winv, nblk * WBLK, who);
    // the kernel writes lower parts only.  A blocking fill: it is complete when this call returns, whatever stream uses winv next
    if (!r) r = hip_ok(hipMemset(s->winv, 0, nblk * WBLK * sizeof(double)));
    double* scratch = nullptr;
    if (!r) r = s->mem.alloc(&scratch, with_x ? s->utmp_len : s->tmp_len, who);
    s->sweep_x = with_x ? scratch : nullptr;
    s->sweep_y = with_x && scratch ? scratch + nblk * NB : scratch;
    if (!r && !jobs.empty()) {
        r = s->mem.alloc(&s->d_jobs, (int64_t)jobs.size(), who);
        if (!r) r = hip_ok(hipMemcpy(s->d_jobs, jobs.data(), jobs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (!r) r = s->mem.alloc(&s->d_info, 8, who);
    if (r) {
        madqp_chol_destroy(s);
        return r;
    }
    *out = s;
    return MADQP_OK;
}

// The left-looking plan (chol_plan.inc) of handle s at half-bandwidth bw (-1: none) and its signature; returns the extent.
static int64_t handle_plan(const madqp_chol* s, int64_t bw, std::vector<CholOp>& ops) {
    return chol_plan(s->n, bw < 0 ? s->n - 1 : bw, s->npos, s->ctx->gemm_slots, ops, chol_modes().wt_min, chol_modes().wt_max, chol_modes().band_w);
}

// Quasi-definite mode: the matrix handed to madqp_chol_factor is [P, .; B, Q] (lower triangle, P of order npos
// and Q positive definite) and stands for [P, B'; B, -Q]; factor computes L with [P, B'; B, -Q] = L diag(I_npos, -I) L',
// solve applies the inverse of that matrix.  npos a multiple of 128 (or n, which restores plain Cholesky).
extern "C" int32_t madqp_chol_set_signature(madqp_chol* s, int64_t npos) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, npos >= 0 && npos <= s->n && (npos % NB == 0 || npos == s->n));
    ARG_TRY(s->ctx, s->band.bw < 0 || npos == s->n);  // the band schedule factors positive definite matrices only
    s->npos = npos;
    s->plan.clear();  // (built again at the next left-looking factorisation)
    return MADQP_OK;
}

extern "C" int32_t madqp_chol_destroy(madqp_chol* s) {
    if (!s) return MADQP_OK;
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;  // (its owner frees the device buffers)
    return MADQP_OK;
}

// ---- band driver -------------------------------------------------------------------------------------------------------
// A matrix with half-bandwidth bw (A[i,j] = 0 for i - j > bw) has a factor inside the same band, so the left-looking
// schedule below runs its products, diagonal kernels and panel solves on band-limited ranges only: the plan of
// chol_plan.inc, built here once per bandwidth.  The storage stays dense (or packed, below).  The sweeps of madqp_chol_solve stay inside the
// band as well (MADQP_SWEEP_BAND, default 1): block row r streams the band_sweep_blocks(bw) tiles next to its diagonal
// block, along a job list of its own where the dense sweeps have one.  bw = -1 clears the bandwidth (the dense schedules
// and sweeps, launch for launch as without this call).
extern "C" int32_t madqp_chol_set_bandwidth(madqp_chol* s, int64_t bw) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    ARG_TRY(ctx, bw == -1 || (bw >= 0 && bw < s->n && s->npos == s->n));
    // the form of the sweeps changes with this call and what is stored may be the factor of another schedule: a solve
    // needs a new factorisation first (without a matrix madqp_chol_solve refuses with MADQP_ERR_STATE)
    forget_factor(s);
    // (the extent changes with the bandwidth and packed storage is laid out for one extent: madqp_chol_set_packed again)
    if (s->band.d_jobs) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (a solve on the stream may still read the list)
    HIP_TRY(ctx, band_clear(s));
    s->plan.clear();  // (without a band: built at the next left-looking factorisation)
    if (bw < 0) return MADQP_OK;
    // the new state in a local: the handle takes it once the plan and the job list both stand, and keeps "no band" otherwise
    madqp_chol_band b;
    b.bw = bw;
    b.extent = handle_plan(s, bw, s->plan);
    if (s->sweep_band) {
        b.sweep_kb = band_sweep_blocks(bw);
        if (s->d_jobs) {
            std::vector<int32_t> jobs;
            band_sweep_jobs((s->n + NB - 1) / NB, b.sweep_kb, s->sweep_chunk, jobs);
            const size_t before = s->mem.owned.size();
            int32_t r = s->mem.alloc(&b.d_jobs, (int64_t)jobs.size(), "madqp_chol_set_bandwidth");
            const hipError_t e = r ? hipSuccess : hipMemcpy(b.d_jobs, jobs.data(), jobs.size() * sizeof(int32_t), hipMemcpyHostToDevice);
            if (e != hipSuccess) r = madqp_fail(ctx, MADQP_ERR_ALLOC, "madqp_chol_set_bandwidth: %s", hipGetErrorString(e));
            if (r) {
                s->mem.release(before);
                s->plan.clear();
                return r;
            }
            b.njobs = (int32_t)jobs.size();
        }
    }
    s->band = b;
    return MADQP_OK;
}

// What the sweeps of madqp_chol_solve run as: [0] the blocks a block row reads left of its diagonal block (-1: all of them,
// the dense sweeps), [1] workgroups per sweep, [2] tiles per job (MADQP_SWEEP_CHUNK).
extern "C" int32_t madqp_chol_sweep_info(madqp_chol* s, int64_t* out_host) {
    if (!s || !out_host) return MADQP_ERR_ARG;
    const bool band = s->band.sweep_kb >= 0;
    const int64_t nblk = std::max<int64_t>(1, (s->n + NB - 1) / NB);
    out_host[0] = band ? s->band.sweep_kb : -1;
    out_host[1] = !s->d_jobs ? nblk : band ? s->band.njobs : s->sweep_njobs;
    out_host[2] = s->sweep_chunk;
    return MADQP_OK;
}

extern "C" int32_t madqp_chol_band_extent(madqp_chol* s, int64_t* extent_host) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, extent_host != nullptr);
    *extent_host = s->band.extent;  // (n - 1 without a band)
    return MADQP_OK;
}

// Packed band storage (band_plan.inc, "packed band storage"; include/madqp.h).  The kernels and launches of the band path
// stay: only the leading dimension changes, and what `lda` has to cover.  The band sweeps are a condition -- the dense
// sweeps stream the whole lower triangle.
static int64_t packed_ld_pad() {  // MADQP_BAND_LD_PAD: doubles added to ceil16(extent + 1) (measurements)
    const char* e = getenv("MADQP_BAND_LD_PAD");
    return e ? std::max<int64_t>(0, atoll(e)) / 2 * 2 : BAND_PACKED_PAD;
}
extern "C" int32_t madqp_chol_packed_layout(madqp_chol* s, int64_t ld_in, int64_t* out_host) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, out_host != nullptr && s->band.bw >= 0);
    if (!band_packed_layout(s->n, s->band.extent, ld_in, out_host, packed_ld_pad()))
        return madqp_fail(s->ctx, MADQP_ERR_ARG, "madqp_chol_packed_layout: ld = %lld is below the extent %lld", (long long)ld_in,
                          (long long)s->band.extent);
    return MADQP_OK;
}
extern "C" int32_t madqp_chol_set_packed(madqp_chol* s, int32_t on) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, !on || (s->band.bw >= 0 && s->band.sweep_kb >= 0 && s->npos == s->n));
    if (s->band.packed != (on != 0)) forget_factor(s);  // what is stored was factored in the other layout
    s->band.packed = on != 0;
    return MADQP_OK;
}

static_assert(BAND_NB == NB && BAND_NBO == NBO, "chol_plan.inc plans in this file's blocks");

// What a factorisation works on: one matrix, or B equally sized ones at fixed strides (the batch part; every launch
// then covers all problems, grid.y / grid.x = problem, and leaves those with skip[b] != 0 alone).
struct CholTarget {
    madqp_ctx* ctx;
    double* A;
    int64_t lda, n;
    double* winv;   // n/128 blocks of WBLK doubles (per problem)
    int32_t* info;  // one int (per problem)
    // false: B = 1 and no batch part -- launches take no GemmBatch and the default Potf2Batch / PanelBatch, and the diagonal
    // kernel only factors (potf2_inv_kernel<1>); true: it factors and inverts (<0>: what the batched sweeps multiply with)
    bool batched = false;
    int64_t B = 1, sA = 0, sW = 0;  // problems (list: slots) and their strides in A and winv (doubles)
    const int32_t* skip = nullptr;
    const int32_t* list = nullptr;  // compacted form (GemmBatch::list)
    const int32_t* count = nullptr;
    bool packed = false;  // packed band storage: lda >= the band's extent, rows up to the padded order exist (band_packed_size)
    int64_t npad() const { return (n + NB - 1) / NB * NB; }
    // rows up to the padded order may be read when the leading dimension covers them (the KKT
    // object allocates K that way) or the storage is packed: no partial tiles, stores stay masked
    bool padded() const { return packed || lda >= npad(); }
};
// a product of the factorisation on target t: operand Y and addend Cin of problem b at strides sY, sCin (X, C: t.sA)
static int32_t target_gemm(const CholTarget& t, const GemmArgs& g, int cls, int64_t sY, int64_t sCin) {
    if (!t.batched) return madqp_gemm_tn(t.ctx, g, cls);
    const GemmBatch bt{t.B, t.sA, sY, t.sA, sCin, 0, t.skip, t.list, t.count};
    return madqp_gemm_tn(t.ctx, g, cls, nullptr, 0, &bt);
}

static int32_t panel_update(const CholTarget& t, const CholOp& o) {  // an UPDATE of the plan (chol_plan.inc)
    GemmArgs g{};
    g.X = t.A + o.row0 + o.k0 * t.lda;
    g.ldx = t.lda;
    g.Y = g.X;
    g.ldy = t.lda;
    g.C = t.A + o.row0 + o.row0 * t.lda;
    g.ldc = t.lda;
    g.Cin = g.C;
    g.ldcin = t.lda;
    g.alpha = (double)o.sign;
    g.beta = 1.0;
    g.M = o.rows;
    g.N = o.width;
    g.K = o.kend - o.k0;
    if (t.padded()) {
        g.Mread = (o.rows + NB - 1) / NB * NB;
        g.Nread = std::min<int64_t>(t.npad() - o.row0, (o.width + NB - 1) / NB * NB);
    }
    g.diag_off = 0;
    g.lower_only = 1;
    return target_gemm(t, g, MADQP_PROF_POTRF_GEMM, t.sA, t.sA);
}

// what the factor-only diagonal kernels leave out of the serial spine, for all blocks j0/128 .. in ONE launch: the
// off-diagonal parts of the sweep images
static int32_t sweep_images(madqp_chol* s, double* A, int64_t lda, int64_t j0, int64_t w) {
    if (w <= 0) return MADQP_OK;
    madqp_ctx* ctx = s->ctx;
    ProfScope ps(ctx, MADQP_PROF_POTRF_DIAG);
    hipLaunchKernelGGL(sweep_image_kernel, dim3((unsigned)((w + NB - 1) / NB)), dim3(256), 0, ctx->stream, A, lda, s->n, j0, s->winv);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// the forward sweep's kernel, named ahead of factor_block: the compiler emits the instances of kernel templates in the order of
// their first use, and the code object keeps the order it has always had (launch_sweep below is the one user)
static const auto sweep_fwd_kernel = trsv_fwd_sweep_kernel<false>;

// The panel solve of ONE 128-column block: X (rows x 128, leading dimension ldx; rows_read >= rows of them exist in memory)
// <- X L^-T for the factored diagonal block L (ldl), by block substitution with the 16 x 16 diagonal inverses that the
// diagonal kernel left in the image Wcm (panel_sub16_kernel).  A short block (w < 128) is the last of its matrix or tile in
// every caller and has no rows below it.
// batch: a batched target, for its batch part (the same solve for its B problems); nullptr: one matrix.
int32_t madqp_chol_panel_solve(madqp_ctx* ctx, double* X, int64_t ldx, int64_t rows, int64_t rows_read, const double* L,
                               int64_t ldl, const double* Wcm, int64_t w, const CholTarget* batch) {
    if (rows <= 0) return MADQP_OK;
    ARG_TRY(ctx, w == NB);
    ARG_TRY(ctx, rows_read >= rows && (!batch || (batch->B >= 1 && batch->B <= 65535)));
    ProfScope ps(ctx, MADQP_PROF_POTRF_TRSM);
    const PanelBatch bt = batch ? PanelBatch{batch->sA, batch->sA, batch->sW, batch->skip, batch->list, batch->count}
                                : PanelBatch{0, 0, 0, nullptr};
    hipLaunchKernelGGL(panel_sub16_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)(batch ? batch->B : 1)), dim3(256), 0,
                       ctx->stream, X, ldx, L, ldl, Wcm, rows, rows_read, bt);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// A BLOCK of the plan: one 128-column block whose entries already carry every update from the columns to its left --
// factor the diagonal block (a batched target: and invert it), then L[below, jb] = C[below, jb] L_jj^-T for o.rows rows.
static int32_t factor_block(const CholTarget& t, const CholOp& o) {
    madqp_ctx* ctx = t.ctx;
    const int64_t jb = o.row0, w = o.width, rows = o.rows;
    double* Ajj = t.A + jb + jb * t.lda;
    double* Wcm = t.winv + (jb / NB) * WBLK;
    {
        ProfScope ps(ctx, MADQP_PROF_POTRF_DIAG);
        const Potf2Batch bt = t.batched ? Potf2Batch{t.sA, t.sW, 1, t.skip, t.list, t.count} : Potf2Batch{0, 0, 0, nullptr};
        const auto diag_kernel = t.batched ? potf2_inv_kernel<0> : potf2_inv_kernel<1>;
        hipLaunchKernelGGL(diag_kernel, dim3((unsigned)t.B), dim3(P2_KTHREADS), 0, ctx->stream, Ajj, t.lda, (int)w, Wcm,
                           Wcm + NB * NB, t.info, (int32_t)jb, bt);
        LAUNCH_CHECK(ctx);
    }
    return madqp_chol_panel_solve(ctx, Ajj + w, t.lda, rows, t.padded() ? (rows + NB - 1) / NB * NB : rows, Ajj, t.lda, Wcm, w,
                                  t.batched ? &t : nullptr);
}

// The executor of every left-looking schedule: the operations of a plan (chol_plan.inc) in their order.
static int32_t run_ops(const CholTarget& t, const std::vector<CholOp>& ops) {
    for (const CholOp& o : ops) {
        const int32_t r = o.kind == CHOL_UPDATE ? panel_update(t, o) : factor_block(t, o);
        if (r) return r;
    }
    return MADQP_OK;
}
// the one matrix of a handle as a target
static CholTarget chol_target(madqp_chol* s, double* A, int64_t lda) {
    CholTarget t{s->ctx, A, lda, s->n, s->winv, s->d_info};
    t.packed = s->band.packed;
    return t;
}

// ---- mid-size schedule: which trailing columns a block step visits (round 4) ---------------------------------------
// The right-looking schedule rewrote the whole trailing matrix in every step; its first steps were bound by that (two
// rounds of tiles per step at n = 5 000) while the later ones wait for the chain diagonal tile -> panel -> diagonal tile
// with most CUs idle.  The update of column j with panel p is due only at step j, so the work can be moved: tile column
// j carries upto[j] (panels 0 .. upto[j]-1 applied); step k VISITS a column by applying up to MID_Q of its pending panels
// to all its tiles in one product (K = 128 q, one tile per workgroup, a column at most once per step).  Every step
// visits column k (completing it: its panel is solved next) and column k+1 (so that the next diagonal tile lacks panel
// k alone, the diagonal workgroup's own SYRK), then the columns with the least slack -- steps until the column is due
// minus the visits it still needs -- while the step's budget of `rounds` x `cap` tiles lasts; a column whose slack is
// used up is visited whatever the budget.  `rounds` is the smallest count for which no visit ever needs more than
// MID_Q panels: 1 up to n = 5 120 on 256 CUs (every step then fits the shadow of the chain: 40 steps of ~47 us at
// n = 5 000 instead of 8 of them at ~90 us), 2-4 up to 10 240, 5-6 up to 13 312.  The plan depends on (number of blocks, cap) only.
// builds and uploads the plan of s (once; nothing is queued); false: no plan (the caller takes the left-looking driver)
static bool mid_plan_build(madqp_chol* s, int nblk, int cap) {
    MidPlan& mp = s->mid;
    if (mp.state) return mp.state > 0;
    mp.state = -1;
    if (nblk > 255 || cap < 1) return false;
    std::vector<std::vector<MidVisit>> steps;
    std::vector<int32_t> units;
    bool ok = false;
    for (int rounds = 1; rounds <= 64 && !ok; ++rounds) ok = mid_plan_steps(nblk, rounds * cap, steps, units, cap);
    if (!ok) return false;
    std::vector<uint32_t> w;
    std::vector<int32_t> count((size_t)nblk), first((size_t)nblk);
    for (int k = 0; k < nblk; ++k) {
        first[k] = (int32_t)w.size();
        mid_plan_units(nblk, k, steps[k], w);
        count[k] = (int32_t)w.size() - first[k];
        if (count[k] != units[k]) return false;
    }
    if (w.empty()) w.push_back(0);
    // a failure leaves the handle without a plan AND without its pieces (the left-looking driver runs next: no sticky HIP
    // error may reach its first launch check)
    const size_t before = s->mem.owned.size();
    uint32_t* d_units = nullptr;
    // (synchronous, pageable source: the copy has left `w` when the call returns; once per handle)
    if (s->mem.alloc(&d_units, (int64_t)w.size(), "madqp_chol_factor: mid-size plan") ||
        hipMemcpy(d_units, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        s->mem.release(before);
        return false;
    }
    mp.count.swap(count);
    mp.first.swap(first);
    mp.d_units = d_units;
    mp.state = 1;
    return true;
}

// The mid-size schedule (chol_mid_step_kernel): right-looking, two launches per 128-column block, then the sweep images and
// U = L'.  n > 128, s->npos == n, lda >= the padded order and even, A 16-byte aligned, the plan built (chol_factor_enqueue checks).
static int32_t factor_mid(madqp_chol* s, double* A, int64_t lda) {
    madqp_ctx* ctx = s->ctx;
    const int64_t n = s->n;
    const int64_t npad_m = (n + NB - 1) / NB * NB;
    const int32_t nblk = (int32_t)(npad_m / NB);
    // one timer scope for the whole factorisation (80 short launches: a scope each costs 0.7 ms per factorisation
    // at n = 5 000); the scopes of the launches inside are switched off meanwhile
    ProfScope ps_all(ctx, MADQP_PROF_POTRF_GEMM);
    ProfMute mute(ctx);
    for (int32_t k = 0; k < nblk; ++k) {
        hipLaunchKernelGGL(chol_mid_step_kernel, dim3((unsigned)(1 + s->mid.count[k])), dim3(MID_THREADS), 0, ctx->stream,
                           MidArgs{A, lda, n, nblk, k, s->mid.d_units + s->mid.first[k], s->winv, s->d_info});
        LAUNCH_CHECK(ctx);
        // L[below, jb] = C[below, jb] L_kk^-T
        const int64_t jb = (int64_t)k * NB;
        const int32_t r = madqp_chol_panel_solve(ctx, A + (jb + NB) + jb * lda, lda, n - jb - NB, npad_m - jb - NB,
                                                 A + jb + jb * lda, lda, s->winv + (int64_t)k * WBLK, NB);
        if (r) return r;
    }
    const int32_t ri = sweep_images(s, A, lda, 0, n);  // of all blocks, one launch
    if (ri) return ri;
    // U = L' for the backward sweep (trsv_fwd_sweep_kernel<true>): one pass over the factor, 37 us at n = 5 000
    if (chol_modes().sweep_upper && s->sweep_x) {
        if (!s->upper) {  // (allocated at the first mid-size factorisation)
            const size_t before = s->mem.owned.size();
            if (s->mem.alloc(&s->upper, npad_m * npad_m, "madqp_chol_factor: U = L'")) {
                s->mem.release(before);
                return MADQP_OK;  // (no room for the copy, and no sticky HIP error: the backward sweep on L serves)
            }
            s->upper_ld = npad_m;
        }
        hipLaunchKernelGGL(lower_to_upper_kernel, dim3(2 * nblk, 2 * nblk), dim3(256), 0, ctx->stream, A, lda, n, s->upper,
                           s->upper_ld);
        LAUNCH_CHECK(ctx);
        s->upper_ok = true;
    }
    return MADQP_OK;
}

// Everything of a factorisation except reading its info back: the launches are on the stream, info sits in s->d_info.
static int32_t chol_factor_enqueue(madqp_chol* s, double* A, int64_t lda) {
    madqp_ctx* ctx = s->ctx;
    const int64_t n = s->n;
    HIP_TRY(ctx, hipMemsetAsync(s->d_info, 0, sizeof(int32_t), ctx->stream));
    // mid-size matrices: right-looking, two launches per 128-column block (chol_mid_step_kernel)
    // (measured on bench.py, m = 0.4 n, ms per iteration against the left-looking schedule: 3.34 / 3.90 at n = 3 000,
    // 6.37 / 7.51 at 5 000, 13.7 / 15.1 at 8 000, 22.7 / 23.2 at 10 000, 34.4 / 33.0 at 12 000 -- every step rewrites
    // the whole trailing matrix, which the left-looking schedule does not)
    // (round 5, with the backward sweep on U = L' behind this path -- ms per iteration, this path / left-looking: 19.1 / 21.0 at
    // n = 10 000, 23.7 / 25.4 at 11 000, 29.2 / 30.5 at 12 000, 35.5 / 36.4 at 13 000, 42.8 / 42.6 at 14 000, 60.8 / 58.1 at 16 000)
    // (the plan is built before anything of the schedule is queued; without one -- no memory for it, MADQP_CHOL_MID_MAX beyond
    // 255 blocks, fewer than 4 GEMM slots -- the left-looking schedule below serves every order, as it does under a bandwidth)
    const CholModes& md = chol_modes();
    if (s->band.bw < 0 && n <= md.mid_max && n > NB && s->npos == n && lda >= (n + NB - 1) / NB * NB && lda % 2 == 0 && (((uintptr_t)A) & 15) == 0 &&
        mid_plan_build(s, (int)((n + NB - 1) / NB), md.mid_cap > 0 ? md.mid_cap : ctx->gemm_slots / 2 - 1))
        return factor_mid(s, A, lda);
    // left-looking: the handle's plan for its (bandwidth, signature), built here unless it stands (host only)
    if (s->plan.empty()) handle_plan(s, s->band.bw, s->plan);
    const int32_t r = run_ops(chol_target(s, A, lda), s->plan);
    if (r) return r;
    return sweep_images(s, A, lda, 0, n);
}

extern "C" int32_t madqp_chol_factor(madqp_chol* s, double* A, int64_t lda, int32_t* info_host) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    ARG_TRY(ctx, info_host != nullptr);
    int32_t r = adopt_matrix(s, A, lda);
    if (r) return r;
    *info_host = 0;
    if (s->n == 0) return MADQP_OK;
    if ((r = chol_factor_enqueue(s, A, lda))) return r;
    int32_t info = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&info, s->d_info, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *info_host = info;
    return MADQP_OK;
}

namespace {
__global__ void info_to_slot_kernel(const int32_t* __restrict__ info, double* __restrict__ slot) {
    *slot = (double)*info;
}
}  // namespace
// Queued form (mpc.hip): no read-back here; info goes to *d_slot (a word of the context's result block) and comes
// back with the caller's next madqp_read_results.  The handle does not learn it: solves enqueued behind a failed
// factorisation run, and produce values the caller discards.
int32_t madqp_chol_factor_q(madqp_chol* s, double* A, int64_t lda, double* d_slot) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    ARG_TRY(ctx, d_slot != nullptr);
    int32_t r = adopt_matrix(s, A, lda);
    if (r) return r;
    if (s->n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_slot, 0, sizeof(double), ctx->stream));
        return MADQP_OK;
    }
    if ((r = chol_factor_enqueue(s, A, lda))) return r;
    hipLaunchKernelGGL(info_to_slot_kernel, dim3(1), dim3(1), 0, ctx->stream, s->d_info, d_slot);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// ---------------------------------------------------------------------------------------------
// The halving of the whole matrix (chol_plan_range) for a batch of B equally sized matrices at fixed strides (small
// QPs, batch.hip): every launch covers all problems (grid.y / grid.x = problem), problems with
// skip[b] != 0 are left alone.  winv: B x nblk x WBLK, info: B ints.
// internal (batch.hip): asynchronous; info[b] = 0 or the first failing column of problem b (1-based)
int32_t madqp_chol_factor_batched(madqp_ctx* ctx, double* A, int64_t lda, int64_t n, int64_t sA, double* winv,
                                  int64_t sW, int32_t* info, int64_t B, const int32_t* skip, int64_t slots,
                                  const int32_t* list, const int32_t* count) {
    ARG_TRY(ctx, A && winv && info && lda >= n && B >= 1 && (!list || (count && slots >= 1)));
    if (n == 0) return MADQP_OK;
    HIP_TRY(ctx, hipMemsetAsync(info, 0, (size_t)B * sizeof(int32_t), ctx->stream));
    // (the diagonal kernel factors and inverts: the images are what the batched sweeps multiply with)
    const CholTarget t{ctx, A, lda, n, winv, info, true, list ? slots : B, sA, sW, list ? nullptr : skip, list, count};
    std::vector<CholOp> ops;
    chol_plan_range(n, 0, n, ops);
    return run_ops(t, ops);
}

// ---------------------------------------------------------------------------------------------
// Pieces of the factorisation for the multi-GPU path: the diagonal tile of a step of the 2-D block-cyclic
// Cholesky (dist.hip: dop_potrf_tile) is an order-nb matrix the distributed object owns -- factor_begin adopts it,
// factor_panel runs the blocked factorisation on it, pack_image lays out [info | inverse diagonal blocks | L] for the
// broadcast (madqp_chol_pack_diag: the diagonal part, what dist.hip takes; madqp_chol_panel_pack: every row below too).
// All asynchronous on the context's stream.
namespace {
__global__ void info_store_kernel(const int32_t* __restrict__ info, double* __restrict__ hdr) {
    hdr[0] = (double)*info;
    hdr[1] = 0.0;
}
bool panel_ok(const madqp_chol* s, int64_t j0, int64_t w) {
    return s->A && j0 >= 0 && w > 0 && j0 % NB == 0 && j0 + w <= s->n && (w % NB == 0 || j0 + w == s->n);
}
}  // namespace

extern "C" int32_t madqp_chol_factor_begin(madqp_chol* s, double* A, int64_t lda) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    ARG_TRY(ctx, s->npos == s->n);  // the panel pieces factor positive definite matrices only
    ARG_TRY(ctx, s->band.bw < 0);        // ... and know no band
    if (const int32_t r = adopt_matrix(s, A, lda)) return r;
    HIP_TRY(ctx, hipMemsetAsync(s->d_info, 0, sizeof(int32_t), ctx->stream));
    return MADQP_OK;
}

extern "C" int32_t madqp_chol_factor_panel(madqp_chol* s, int64_t j0, int64_t w) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, panel_ok(s, j0, w) && s->band.bw < 0);
    std::vector<CholOp> ops;
    chol_plan_range(s->n, j0, w, ops);
    const int32_t r = run_ops(chol_target(s, s->A, s->lda), ops);
    return r ? r : sweep_images(s, s->A, s->lda, j0, w);  // (the caller packs / reads the images of this panel next)
}

// buf = [info, 0 | inverse diagonal blocks of the panel | L[j0:j0+rows, j0+c] for c = 0..w-1] (panel_image.h)
static int32_t pack_image(madqp_chol* s, int64_t j0, int64_t w, int64_t rows, double* buf) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    ARG_TRY(ctx, panel_ok(s, j0, w) && buf);
    ProfScope ps(ctx, MADQP_PROF_VEC);
    hipLaunchKernelGGL(info_store_kernel, dim3(1), dim3(1), 0, ctx->stream, s->d_info, buf);
    LAUNCH_CHECK(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(buf + IMG_HDR, s->winv + (j0 / NB) * WBLK, img_blocks(w) * sizeof(double),
                                hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(buf + img_L(w), rows * sizeof(double), s->A + j0 + j0 * s->lda, s->lda * sizeof(double),
                                  rows * sizeof(double), (size_t)w, hipMemcpyDeviceToDevice, ctx->stream));
    return MADQP_OK;
}
extern "C" int32_t madqp_chol_panel_pack(madqp_chol* s, int64_t j0, int64_t w, double* buf) {
    return pack_image(s, j0, w, s ? s->n - j0 : 0, buf);  // every row from the panel's first down
}
int32_t madqp_chol_pack_diag(madqp_chol* s, int64_t j0, int64_t w, double* buf) { return pack_image(s, j0, w, w, buf); }
int64_t madqp_chol_order(const madqp_chol* s) { return s ? s->n : -1; }

// ---- the sweeps of one solve, described once: madqp_chol_solve (both of its paths) and madqp_trsv_tile build this and launch
// through launch_sweep ----
struct Sweeps {
    hipStream_t stream;
    unsigned grid;  // workgroups per sweep: the jobs of the list, one per block row without a list
    const double* winv;
    int64_t n;
    int32_t* ctl;       // the sweeps' ticket counters: ctl[1] forward, ctl[2] backward
    double* fault;      // the context's fault word
    int vec;            // the factor may be read in 16-byte pieces
    int kb;             // the band of the sweeps in blocks (band_plan.inc), -1 for whole block rows
    SweepPlan fwd, bwd;  // the job list (dense or band) with the partial-sum slots of either direction
};
// jobs: the list (of njobs) and the slots of the forward sweep; the backward sweep's follow them
static Sweeps solve_sweeps(madqp_ctx* ctx, int64_t n, const double* L, int64_t ld, const double* winv, int32_t* ctl, const SweepPlan& jobs,
                           int32_t njobs, int kb) {
    const int64_t nblk = (n + NB - 1) / NB;
    Sweeps w{ctx->stream, jobs.jobs ? (unsigned)njobs : (unsigned)nblk, winv, n, ctl, ctx->d_res + MADQP_FAULT_SLOT,
             ((((uintptr_t)L) & 15) == 0) && (ld % 2 == 0), kb, jobs, jobs};
    if (jobs.part) w.bwd.part = jobs.part + nblk * jobs.maxc * NB;
    return w;
}
// The three forms of a sweep on the matrix M (ld): v <- L^-1 v on L, v <- L^-T v on L, and v <- L^-T v as the forward
// kernel on U = L' from the far end (out2: the plain copy of the solution)
enum SweepForm { SWEEP_FWD, SWEEP_BWD, SWEEP_REV };
static void launch_sweep(const Sweeps& w, SweepForm form, const double* M, int64_t ld, const double* in, double* out,
                         double* out2 = nullptr) {
    const dim3 grid(w.grid), block(1024);
    if (form == SWEEP_BWD)
        hipLaunchKernelGGL(trsv_bwd_sweep_kernel, grid, block, 0, w.stream, M, ld, w.winv, in, out, w.n, w.ctl, w.fault, w.vec, w.bwd, w.kb);
    else if (form == SWEEP_FWD)
        hipLaunchKernelGGL(sweep_fwd_kernel, grid, block, 0, w.stream, M, ld, w.winv, in, out, w.n, w.ctl, w.fault, w.vec, w.fwd,
                           (double*)nullptr, w.kb);
    else
        hipLaunchKernelGGL(trsv_fwd_sweep_kernel<true>, grid, block, 0, w.stream, M, ld, w.winv, in, out, w.n, w.ctl, w.fault, w.vec, w.bwd,
                           out2, w.kb);
}

// One sweep over a single order-w tile (multi-GPU solves, dist.hip): the same kernels as madqp_chol_solve.
int32_t madqp_trsv_tile(madqp_ctx* ctx, int32_t trans, const double* L, int64_t ld, const double* winv, double* v,
                        int64_t w, double* tmp, int32_t* ctl) {
    ARG_TRY(ctx, L && winv && v && tmp && ctl && w > 0 && ld >= w);
    ProfScope ps(ctx, MADQP_PROF_TRSV);
    HIP_TRY(ctx, hipMemsetAsync(ctl, 0, 4 * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)tmp, 0x7FF8A5A5, 2 * (size_t)w, ctx->stream));
    launch_sweep(solve_sweeps(ctx, w, L, ld, winv, ctl, SweepPlan{nullptr, nullptr, 0, 0}, 0, -1), trans ? SWEEP_BWD : SWEEP_FWD, L, ld, v, tmp);
    LAUNCH_CHECK(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(v, tmp, (size_t)w * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return MADQP_OK;
}

extern "C" int32_t madqp_chol_solve(madqp_chol* s, double* rhs) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    ARG_TRY(ctx, rhs != nullptr || s->n == 0);
    if (!s->A) return madqp_fail(ctx, MADQP_ERR_STATE, "madqp_chol_solve before madqp_chol_factor");
    const int64_t n = s->n, lda = s->lda;
    const double* A = s->A;
    if (n == 0) return MADQP_OK;
    ProfScope ps(ctx, MADQP_PROF_TRSV);
    // one launch per sweep (see trsv_*_sweep_kernel).  Under a bandwidth the band form: the tiles within sweep_kb blocks of
    // the diagonal, along the band's own (shorter) job list
    const bool band = s->band.sweep_kb >= 0;
    double* y = s->sweep_y;
    const SweepPlan jobs{band ? s->band.d_jobs : s->d_jobs, y + (n + NB - 1) / NB * NB, s->sweep_chunk, s->sweep_maxc};
    const Sweeps sw = solve_sweeps(ctx, n, A, lda, s->winv, s->d_info, jobs, band ? s->band.njobs : s->sweep_njobs, (int)s->band.sweep_kb);
    if (s->upper_ok) {  // mid-size factor (no band): y = L^-1 b, then x = U^-1 y with the same kernel on U = L'; three launches
        hipLaunchKernelGGL(sweep_prep_kernel, dim3((unsigned)std::min<int64_t>((s->utmp_len + 255) / 256, 256)), dim3(256), 0,
                           ctx->stream, reinterpret_cast<unsigned long long*>(s->sweep_x), s->utmp_len, s->d_info);
        launch_sweep(sw, SWEEP_FWD, A, lda, rhs, y);
        launch_sweep(sw, SWEEP_REV, s->upper, s->upper_ld, y, s->sweep_x, rhs);
        LAUNCH_CHECK(ctx);
        return MADQP_OK;
    }
    // y = L^-1 b into the scratch, x = L^-T y into rhs
    HIP_TRY(ctx, hipMemsetAsync(s->d_info + 1, 0, 3 * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)y, 0x7FF8A5A5, 2 * (size_t)s->tmp_len, ctx->stream));
    launch_sweep(sw, SWEEP_FWD, A, lda, rhs, y);
    LAUNCH_CHECK(ctx);
    if (s->npos < n) {  // y <- diag(I, -I) y
        const int64_t len = n - s->npos;
        hipLaunchKernelGGL(negate_kernel, dim3((unsigned)std::min<int64_t>((len + 255) / 256, 1024)), dim3(256), 0,
                           ctx->stream, y + s->npos, len);
        LAUNCH_CHECK(ctx);
    }
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)rhs, 0x7FF8A5A5, 2 * (size_t)n, ctx->stream));
    launch_sweep(sw, SWEEP_BWD, A, lda, y, rhs);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}

// ---- many right-hand sides: block substitution on the transposed block T = B' (solve_plan.inc) -------------------------------
// Stream-ordered launches only: a diagonal step per block and sweep (solve_many_diag_kernel), a product on the fp64 MFMA
// kernels per update (madqp_gemm_tn), the transposes of the caller's block and, for a handle without U = L', of one block row
// of L per backward update.  No workgroup waits for another: no tickets, no sentinel, no spin limit, no fault word.
namespace {
// T (ldt x npad, ldt a multiple of 64) <- B' (B: n x nrhs, leading dimension ldb), zeros in the padding: 64 x 64 pieces through LDS
__global__ __launch_bounds__(256) void many_in_kernel(const double* __restrict__ B, int64_t ldb, int64_t n, int64_t nrhs,
                                                      double* __restrict__ T, int64_t ldt) {
    __shared__ double tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int rr = ty + 4 * q;
        tile[rr][tx] = (i0 + tx < n && r0 + rr < nrhs) ? B[i0 + tx + (r0 + rr) * ldb] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ii = ty + 4 * q;
        T[r0 + tx + (i0 + ii) * ldt] = tile[tx][ii];
    }
}
// B <- T' (the entries i < n, r < nrhs only: rows n .. ldb-1 of the caller's columns are never touched)
__global__ __launch_bounds__(256) void many_out_kernel(const double* __restrict__ T, int64_t ldt, int64_t n, int64_t nrhs,
                                                       double* __restrict__ B, int64_t ldb) {
    __shared__ double tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ii = ty + 4 * q;
        tile[ii][tx] = T[r0 + tx + (i0 + ii) * ldt];  // (the padded block exists up to ldt x npad)
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int rr = ty + 4 * q;
        if (i0 + tx < n && r0 + rr < nrhs) B[i0 + tx + (r0 + rr) * ldb] = tile[tx][rr];
    }
}
// S[c + k lds] <- L[k0 + k, row0 + c] for the `cols` (a multiple of 128) columns from row0 on and k < 128: the block row of L
// that a backward update multiplies with, contraction index slow; rows at or beyond n give zeros.  grid (cols / 64, 2).
__global__ __launch_bounds__(256) void many_strip_kernel(const double* __restrict__ A, int64_t lda, int64_t n, int64_t k0,
                                                         int64_t row0, double* __restrict__ S, int64_t lds) {
    __shared__ double tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * 64, kk0 = (int64_t)blockIdx.y * 64;
    const int64_t r = k0 + kk0 + tx;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int c = ty + 4 * q;
        tile[c][tx] = r < n ? A[r + (row0 + c0 + c) * lda] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int kk = ty + 4 * q;
        S[c0 + tx + (kk0 + kk) * lds] = tile[tx][kk];
    }
}
// The diagonal step of a sweep for 16 right-hand sides per wave, X (rows x w, leading dimension ld) in place:
//   forward   X <- X L_jj^-T :  Z = X',  Z_J = W_JJ  (C'_J - sum_{I<J} L_JI  Z_I),  J = 0 .. 7   (panel_sub16_kernel's step)
//   backward  X <- X L_jj^-1 :           Z_J = W_JJ' (C'_J - sum_{I>J} L_IJ' Z_I),  J = 7 .. 0
// by block substitution over the 16 x 16 sub-blocks, multiplying only with the inverses W_JJ of the DIAGONAL sub-blocks that
// the diagonal kernel left in the image Wcm -- never with a stored 128 x 128 inverse.  On the MFMA unit in
// registers as in panel_sub16_kernel: m = index inside the sub-block written, n = one of 16 right-hand sides, k = index
// inside the sub-block read; a finished Z_J (accumulator layout) is the B-operand of the updates as it stands.  A short last
// block (w < 128): entries of L at or beyond w are not loaded (they need not exist) and count as zero, the image is zero
// there, columns at or beyond w are not stored.  A wave reads only what it writes, all up front.
template <bool BWD>
__global__ __launch_bounds__(256) void solve_many_diag_kernel(double* __restrict__ C, int64_t ld, const double* __restrict__ Lkk,
                                                              int64_t ldl, const double* __restrict__ Wcm, int64_t rows, int w) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lo = lane & 15, hi = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * 64 + wave * 16;
    if (i0 >= rows) return;  // (no barrier in this kernel)
    const int64_t gi = i0 + lo;  // (< ld: the block of right-hand sides is padded to whole 128s)
    double* Cp = C + gi + (int64_t)hi * ld;
    double4_t z[8];  // u_J = -(C'_J - ..) until step J, Z_J afterwards: element (16 J + hi + 4 v, right-hand side gi)
#pragma unroll
    for (int J = 0; J < 8; ++J)
#pragma unroll
        for (int v = 0; v < 4; ++v) z[J][v] = -Cp[(int64_t)(16 * J + 4 * v) * ld];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int J = BWD ? 7 - q : q;
        double4_t t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {  // A[m = lo][k = 4 s + hi] = -W_JJ (forward) / -W_JJ' (backward)
            const double aw = BWD ? -Wcm[(16 * J + 4 * s + hi) + (16 * J + lo) * NB] : -Wcm[(16 * J + lo) + (16 * J + 4 * s + hi) * NB];
            t = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, z[J][s], t, 0, 0, 0);
        }
        z[J] = t;  // Z_J
#pragma unroll
        for (int d = 0; d < 7 - q; ++d) {
            const int J2 = BWD ? J - 1 - d : J + 1 + d;
#pragma unroll
            for (int s = 0; s < 4; ++s) {  // u_J2 += L_{J2,J} Z_J (forward) / L_{J,J2}' Z_J (backward)
                const int r = BWD ? 16 * J + 4 * s + hi : 16 * J2 + lo;
                const int c = BWD ? 16 * J2 + lo : 16 * J + 4 * s + hi;
                const double a = r < w ? Lkk[r + (int64_t)c * ldl] : 0.0;
                z[J2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, t[s], z[J2], 0, 0, 0);
            }
        }
    }
    if (gi < rows) {
#pragma unroll
        for (int J = 0; J < 8; ++J)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (16 * J + 4 * v + hi < w) Cp[(int64_t)(16 * J + 4 * v) * ld] = z[J][v];
    }
}
}  // namespace

extern "C" int32_t madqp_chol_set_solve_many_min(madqp_chol* s, int64_t min_nrhs) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, min_nrhs >= 2);
    s->many_min = min_nrhs;
    return MADQP_OK;
}

extern "C" int32_t madqp_chol_solve_many_info(madqp_chol* s, int64_t nrhs, int64_t* out_host) {
    if (!s) return MADQP_ERR_ARG;
    ARG_TRY(s->ctx, out_host != nullptr && nrhs >= 0);
    const bool blocked = nrhs >= s->many_min;
    const bool up = s->upper_ok;  // the last factorisation left U = L'
    SolveCount c;
    if (blocked) {
        std::vector<SolveOp> ops;
        solve_plan(s->n, s->npos, s->band.sweep_kb, nrhs, ops);
        c = solve_plan_count(ops, up);
    } else {
        c = solve_looped_count(s->n, s->npos, s->band.sweep_kb, nrhs, up);
    }
    out_host[0] = blocked ? 1 : 0;
    out_host[1] = c.launches;
    out_host[2] = s->many_ws_len;
    out_host[3] = c.bytes;
    return MADQP_OK;
}

extern "C" int32_t madqp_chol_solve_many(madqp_chol* s, double* B, int64_t ldb, int64_t nrhs) {
    if (!s) return MADQP_ERR_ARG;
    madqp_ctx* ctx = s->ctx;
    const int64_t n = s->n;
    ARG_TRY(ctx, nrhs >= 0 && ldb >= std::max<int64_t>(n, 1) && (B != nullptr || n == 0 || nrhs == 0));
    if (!s->A) return madqp_fail(ctx, MADQP_ERR_STATE, "madqp_chol_solve_many before madqp_chol_factor");
    if (n == 0 || nrhs == 0) return MADQP_OK;
    if (nrhs < s->many_min) {  // column by column through the one-vector sweeps (nrhs == 1: madqp_chol_solve itself)
        for (int64_t c = 0; c < nrhs; ++c)
            if (const int32_t r = madqp_chol_solve(s, B + c * ldb)) return r;
        return MADQP_OK;
    }
    ProfScope ps(ctx, MADQP_PROF_TRSV);
    ProfMute mute(ctx);  // (one timer scope for the call)
    const bool up = s->upper_ok;  // the last factorisation left U = L'
    const int64_t lda = s->lda, npad = (n + NB - 1) / NB * NB, ldt = solve_plan_ldt(nrhs);
    // (grown here, at the first call that needs more: the stream is drained before the old buffer goes)
    if (const int32_t r = s->mem.grow(&s->many_ws, &s->many_ws_len, solve_plan_workspace(n, nrhs, up), "madqp_chol_solve_many: workspace"))
        return r;
    double* T = s->many_ws;
    double* strip = T + ldt * npad;  // (npad x 128, leading dimension npad; only without U)
    const double* A = s->A;
    const bool padded = chol_target(s, s->A, lda).padded();
    std::vector<SolveOp> ops;
    solve_plan(n, s->npos, s->band.sweep_kb, nrhs, ops);
    const dim3 tgrid((unsigned)(npad / 64), (unsigned)(ldt / 64));
    hipLaunchKernelGGL(many_in_kernel, tgrid, dim3(256), 0, ctx->stream, (const double*)B, ldb, n, nrhs, T, ldt);
    LAUNCH_CHECK(ctx);
    for (const SolveOp& o : ops) {
        if (o.kind == SOLVE_DIAG) {
            const auto kern = o.sweep ? solve_many_diag_kernel<true> : solve_many_diag_kernel<false>;
            hipLaunchKernelGGL(kern, dim3((unsigned)((nrhs + 63) / 64)), dim3(256), 0, ctx->stream, T + o.k0 * ldt, ldt,
                               A + o.k0 + o.k0 * lda, lda, (const double*)(s->winv + o.blk * WBLK), nrhs, (int)(o.k1 - o.k0));
            LAUNCH_CHECK(ctx);
        } else if (o.kind == SOLVE_NEGATE) {
            const int64_t len = o.rows * ldt;
            hipLaunchKernelGGL(negate_kernel, dim3((unsigned)std::min<int64_t>((len + 255) / 256, 1024)), dim3(256), 0, ctx->stream,
                               T + o.row0 * ldt, len);
            LAUNCH_CHECK(ctx);
        } else {
            GemmArgs g{};
            g.X = T + o.k0 * ldt;
            g.ldx = ldt;
            g.C = T + o.row0 * ldt;
            g.ldc = ldt;
            g.Cin = g.C;
            g.ldcin = ldt;
            g.alpha = -1.0;
            g.beta = 1.0;
            g.M = nrhs;
            g.Mread = ldt;
            g.N = o.rows;
            if (o.sweep == 0) {  // Y[i + k ldy] = L[row0 + i, k0 + k]
                g.Y = A + o.row0 + o.k0 * lda;
                g.ldy = lda;
                g.K = o.k1 - o.k0;  // (a block with rows below it is a whole one)
                if (padded) g.Nread = (o.rows + NB - 1) / NB * NB;
            } else {  // Y[c + k ldy] = L[k0 + k, row0 + c]: U, or the strip; K = 128 with zeros from n on (T is zero there too)
                if (up) {
                    g.Y = s->upper + o.row0 + o.k0 * s->upper_ld;
                    g.ldy = s->upper_ld;
                } else {
                    hipLaunchKernelGGL(many_strip_kernel, dim3((unsigned)(o.rows / 64), 2), dim3(256), 0, ctx->stream, A, lda, n, o.k0,
                                       o.row0, strip, npad);
                    LAUNCH_CHECK(ctx);
                    g.Y = strip;
                    g.ldy = npad;
                }
                g.K = NB;
                g.Nread = o.rows;
            }
            if (const int32_t r = madqp_gemm_tn(ctx, g, MADQP_PROF_TRSV)) return r;
        }
    }
    hipLaunchKernelGGL(many_out_kernel, tgrid, dim3(256), 0, ctx->stream, (const double*)T, ldt, n, nrhs, B, ldb);
    LAUNCH_CHECK(ctx);
    return MADQP_OK;
}
