// 2-D block-cyclic distributed Cholesky + triangular solves (SURVEY.md 8e; BASELINE configs[4]) -- the orchestration.
//
// No counterpart in the reference (single process, src/linear_solver.jl:10 calls one factorize!); it sits behind the
// same AbstractLinearSolver contract (factorize! / solve!, src/KKT/normalkkt.jl:99-101,196).
//
// This file is compiled twice: by dist.hip (the product: rank-local kernels = the MFMA GEMM core, the diagonal-block
// kernel and the sweep kernels of this library; collectives = RCCL on the context's stream) and by tests/csrc/
// dist_cpu.cpp (test infrastructure: plain C++ loops for the rank-local kernels, host-staged collectives supplied by
// the caller, so that the CPU suite runs THIS schedule with world_size 2..6 over gloo).  The includer defines `Dev`
// (context handle) and the dop_* primitives listed in dist.hip.
//
// Layout.  P x Q process grid, rank = p*Q + q.  The order-n matrix is cut into T = ceil(n/nb) tile rows / columns
// (nb a multiple of 128); tile (I, J), I >= J, lives on rank (I mod P, J mod Q) at local position (I div P, J div Q)
// of a column-major local matrix of mloc x nloc (leading dimension ld, padded to 128 and zero filled).
//
// Factorisation over tile columns k, LEFT-looking in its updates (lazy: a tile column receives the panels it has not seen
// in ONE wide-K product when it is about to become the panel, or ahead of that in the background -- update_col_range --
// from the stored operands of all earlier steps), with look-ahead 1 in its panel phase (the ranks of process column
// (k+1) mod Q bring tile column k+1 up to date first, so that its panel phase overlaps the background work of step k):
//   1. owner (k mod P, k mod Q): Cholesky of the diagonal tile (+ inverse 128-blocks) -> BROADCAST down process
//      column k mod Q;  2. the ranks of that column: L[I, k] = C[I, k] L_kk^-T for their tile rows I > k;
//   3. the panel rows of process row p are BROADCAST along the row (root q = k mod Q): X_p = L[{I = p mod P}, k];
//   4. the column operand Y_q = L[{J = q mod Q}, k] arrives by one BROADCAST down every process column per source row
//      p' (root p'): the tiles J with J mod P = p', which rank (p', q) holds since step 3;
//   5. both operands are FILED (XW / YW: staircase stores of this rank's tile rows / tile columns of L, levels of a few
//      steps each, rows above a level's first diagonal tile not stored); C[I, J] -= sum_k X_p(k)[I] Y_q(k)[J]' is applied
//      per tile column J, over every step k it has not received, when the column is needed: one GEMM launch per level.
// Solves: forward and backward sweeps over GROUPS of G tiles (G nb = 4096 rows by default).  The G x G tile triangle on
// the diagonal of group g is collected on rank g mod world during the factorisation (point-to-point, behind the operand
// broadcasts of each step); per group and sweep: one REDUCE of the group's partial sums to that rank, one local
// triangular solve of order G nb with the stored inverse blocks, one BROADCAST of the solved rows to everyone (so the
// solution ends up replicated), GEMVs on the local tiles outside the triangle -- 2 collectives per group, not per tile.
// The first failing column (LAPACK info) travels in the headers of steps 1 and 3: all ranks agree without a
// collective of its own.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "panel_image.h"  // [info, 0 | inverse 128-blocks | L]: the form diagonal tiles and operands travel in

enum { GRP_WORLD = 0, GRP_ROW = 1, GRP_COL = 2 };
static const int DIST_MAXLEV = 32;  // levels of the operand staircases

struct madqp_dist {
    Dev* dev;
    int32_t rank, world, P, Q, p, q;
    int64_t n, nb, T;
    int64_t mt, nt;        // local tile rows / columns
    int64_t mloc, nloc;    // local rows / columns
    int64_t ld, ncp;       // leading dimension and padded column count of the local matrix
    double* K;             // ld x ncp, owned
    double* Wdiag;         // inverse blocks of the local diagonal tiles: slot (I div P) when (I mod P, I mod Q) == (p, q)
    int64_t wslot;         // doubles per diagonal tile slot
    double* diagbuf;       // [hdr | W blocks | L_kk (w x w)] of the current step
    double* Xrow[2];       // broadcast image of a row operand ([hdr | ldx x nb]), double buffered over k
    // Stored operands of ALL steps (lazy, left-looking updates): block k of XW is the row operand of step k at its local
    // row positions, block k of YW the column operand at its local column positions.  Step k is only ever read from the
    // rows of tiles > k, so the stores are STAIRCASES: the steps are cut into levels of `lev_w` steps, level s keeps the
    // rows from its first step's first tile down (leading dimension ld - row0, (1/2 + 1/(2 nlev)) of the full rectangle:
    // 31 instead of 61 GB per rank at C5 on 2 x 4).  nullptr = the local matrix itself (XW when Q == 1, YW on a 1 x 1
    // grid): one level, nothing allocated.
    double *XW, *YW;
    int32_t nlev;
    int64_t lev_k0[DIST_MAXLEV + 1];                       // steps lev_k0[s] .. lev_k0[s+1]-1 form level s
    int64_t xl_row0[DIST_MAXLEV], xl_ld[DIST_MAXLEV], xl_off[DIST_MAXLEV];  // XW: first stored local row, ld, offset
    int64_t yl_row0[DIST_MAXLEV], yl_ld[DIST_MAXLEV], yl_off[DIST_MAXLEV];  // YW: the same over local columns
    int64_t xw_count, yw_count;                            // doubles allocated (0: in place)
    // device bytes of this handle and of what madqp_dist_memory tells apart: matrix, XW, YW, bands, staging (distcore::buffers)
    int64_t bytes_total, bytes_K, bytes_xw, bytes_yw, bytes_band, bytes_stage;
    double* bstage2;       // force_comm only: where a piece sent to oneself is received (exercises ncclSend / ncclRecv)
    int64_t* done;         // host: per local tile column, the number of panels already applied to it
    double* seg;           // transpose segment: tiles of nb x nb
    double* vtile;         // group-solve scratch (2 G nb doubles)
    double *sloc, *tloc;   // partial sums of the sweeps (mloc / nloc)
    // solve groups: G consecutive tiles; the G x G tile triangle on the diagonal of group g and the inverse 128-blocks of
    // its diagonal tiles live on rank g mod world (slot g div world), collected during the factorisation
    int64_t G, NG, my_groups;  // (my_groups: the band slots of this rank)
    int64_t bslot, bwslot;  // doubles per slot: (G nb)^2 (leading dimension G nb) / G (nb/128) inverse-block images
    double *band, *bandW;
    double* bstage;         // staging of one step's pieces: [diagonal image | G tiles]
    double* gvec;           // G nb doubles: a group's partial sums
    double* info_dev;      // 1 double: first failing column so far (0 = none)
    const madqp_comm_ops* host;  // host-staged collectives (tests) or nullptr (RCCL)
    void* hostbuf;
    size_t hostbuf_bytes;
    void* nccl[3];
    int64_t bytes_sent;    // payload this rank put on the wire as a broadcast root (diagnostics)
    int32_t force_comm;    // issue the collectives even in groups of one rank (RCCL smoke test on a single GPU)
    int32_t factored;      // a factorisation ran to its end (whatever its info)
    char err[256];
    int32_t fits;          // this rank's own verdict: its byte total against its free device memory
};

namespace distcore {

inline int64_t tsize(const madqp_dist* d, int64_t I) { return std::min<int64_t>(d->nb, d->n - I * d->nb); }
inline int64_t count_tiles(int64_t T, int64_t r, int64_t R) { return T > r ? (T - r + R - 1) / R : 0; }
// first local tile index (row direction: modulus P, residue p) whose global tile is > k
inline int64_t first_after(int64_t k, int64_t r, int64_t R) {
    // smallest l with l*R + r > k
    if (k < r) return 0;
    return (k - r) / R + 1;
}
inline int64_t local_extent(const madqp_dist* d, int64_t ntiles, int64_t r, int64_t R) {
    if (ntiles == 0) return 0;
    const int64_t last = r + (ntiles - 1) * R;
    return (ntiles - 1) * d->nb + tsize(d, last);
}
inline int64_t pad128(int64_t v) { return std::max<int64_t>(128, (v + 127) / 128 * 128); }

// ---------------------------------------------------------------- collectives
inline int group_size(const madqp_dist* d, int g) { return g == GRP_WORLD ? d->world : g == GRP_ROW ? d->Q : d->P; }
inline int group_rank(const madqp_dist* d, int g) { return g == GRP_WORLD ? d->rank : g == GRP_ROW ? d->q : d->p; }
// a single rank with nothing forced: no collective runs, the factor stays where it lies
inline bool single_rank(const madqp_dist* d) { return d->world == 1 && !d->force_comm; }
// group g has traffic: more than one member, or the collectives are issued regardless (force_comm)
inline bool group_traffic(const madqp_dist* d, int g) { return group_size(d, g) > 1 || d->force_comm; }

#define DTRY(expr)                 \
    do {                           \
        int32_t r_ = (expr);       \
        if (r_) return r_;         \
    } while (0)

inline int32_t host_reserve(madqp_dist* d, size_t bytes) {
    if (bytes <= d->hostbuf_bytes) return 0;
    free(d->hostbuf);
    d->hostbuf = malloc(bytes);
    d->hostbuf_bytes = d->hostbuf ? bytes : 0;
    return d->hostbuf ? 0 : MADQP_ERR_ALLOC;
}
// The host-staged form of a collective on `count` doubles at buf: through the host buffer, out of the device when this
// rank contributes (`out`), back into it when this rank receives (`in`); call(ops, hostbuf) is the caller's callback
template <class Call>
inline int32_t host_staged(madqp_dist* d, double* buf, int64_t count, bool out, bool in, Call call) {
    const size_t bytes = (size_t)count * 8;
    DTRY(host_reserve(d, bytes));
    if (out) DTRY(dop_d2h(d->dev, d->hostbuf, buf, bytes));
    if (call(d->host, d->hostbuf)) return MADQP_ERR_STATE;
    if (in) DTRY(dop_h2d(d->dev, buf, d->hostbuf, bytes));
    return 0;
}

inline int32_t comm_send(madqp_dist* d, const double* buf, int64_t count, int dst);
inline int32_t comm_recv(madqp_dist* d, double* buf, int64_t count, int src);
inline int32_t comm_p2p_begin(madqp_dist* d);
inline int32_t comm_p2p_end(madqp_dist* d);
// world rank of member i of group g as this rank sees it
inline int group_member(const madqp_dist* d, int g, int i) { return g == GRP_WORLD ? i : g == GRP_ROW ? d->p * d->Q + i : i * d->Q + d->q; }
// MADQP_DIST_BCAST=p2p: a broadcast inside a process row / column / the world as ONE group of point-to-point transfers
// from the root to every peer (<= 3 + 1 peers on 2 x 4) instead of ncclBroadcast.  xGMI is point to point, 7 links per
// GPU: a ring on a 2- or 4-rank sub-communicator is bound by one 153 GB/s link, separate sends to separate peers leave on
// separate links (SURVEY.md 8e).  Same data, same buffers, same stream order; which form is faster only real links can
// say, hence a knob (default: the library collective).  Under force_comm (one rank) the root sends the image to itself
// through RCCL (received beside it, copied back): the calls are exercised on a single GPU.
inline bool bcast_p2p() {
    static const bool on = getenv("MADQP_DIST_BCAST") && strcmp(getenv("MADQP_DIST_BCAST"), "p2p") == 0;
    return on;
}
inline int32_t comm_bcast_p2p(madqp_dist* d, double* buf, int64_t count, int root, int g) {
    const int me = group_rank(d, g), size = group_size(d, g);
    const int64_t sent0 = d->bytes_sent;
    int32_t r = comm_p2p_begin(d);
    if (r) return r;
    if (me == root) {
        for (int i = 0; i < size && !r; ++i)
            if (i != root) r = comm_send(d, buf, count, group_member(d, g, i));
    } else {
        r = comm_recv(d, buf, count, group_member(d, g, root));
    }
    const int32_t r2 = comm_p2p_end(d);  // (the bracket is always closed)
    d->bytes_sent = sent0 + (me == root ? 8 * count : 0);  // counted once per broadcast, as for the collective
    return r ? r : r2;
}
// root: rank WITHIN the group (q for a row group, p for a column group, world rank for the world)
inline int32_t comm_bcast(madqp_dist* d, double* buf, int64_t count, int root, int g) {
    if (count <= 0 || !group_traffic(d, g)) return 0;
    const bool is_root = group_rank(d, g) == root;
    if (bcast_p2p() && group_size(d, g) > 1) return comm_bcast_p2p(d, buf, count, root, g);
    if (bcast_p2p() && d->force_comm && !d->host && d->bstage2) {
        // one rank, RCCL forced: the image goes to this rank itself through ncclSend / ncclRecv, in pieces of the staging
        // buffer's size, and is copied back over the original (bit for bit the same data: the schedule does not notice)
        const int64_t cap = d->wslot + d->nb * d->nb + d->G * d->nb * d->nb;
        d->bytes_sent += 8 * count;
        for (int64_t off = 0; off < count; off += cap) {
            const int64_t c = std::min(cap, count - off), sent0 = d->bytes_sent;
            int32_t r = comm_p2p_begin(d);
            if (r) return r;
            r = comm_send(d, buf + off, c, d->rank);
            if (!r) r = comm_recv(d, d->bstage2, c, d->rank);
            const int32_t r2 = comm_p2p_end(d);
            d->bytes_sent = sent0;
            if (r || r2) return r ? r : r2;
            if ((r = dop_copy(d->dev, buf + off, d->bstage2, c))) return r;
        }
        return 0;
    }
    if (is_root) d->bytes_sent += 8 * count;
    if (d->host)
        return host_staged(d, buf, count, is_root, !is_root, [&](const madqp_comm_ops* h, void* hb) {
            return h->bcast(h->user, hb, count * 8, root, g);
        });
    return dop_nccl_bcast(d->dev, d->nccl[g], buf, count, root);
}
// sum over the group into the root's buffer (in place); other ranks' buffers are left as they are
inline int32_t comm_reduce(madqp_dist* d, double* buf, int64_t count, int root, int g) {
    if (count <= 0 || !group_traffic(d, g)) return 0;
    if (d->host)
        return host_staged(d, buf, count, true, group_rank(d, g) == root, [&](const madqp_comm_ops* h, void* hb) {
            return h->reduce_sum(h->user, (double*)hb, count, root, g);
        });
    return dop_nccl_reduce(d->dev, d->nccl[g], buf, count, root);
}
inline int32_t comm_allreduce(madqp_dist* d, double* buf, int64_t count, int g) {
    if (count <= 0 || !group_traffic(d, g)) return 0;
    if (d->host)
        return host_staged(d, buf, count, true, true, [&](const madqp_comm_ops* h, void* hb) {
            return h->allreduce_sum(h->user, (double*)hb, count, g);
        });
    return dop_nccl_allreduce(d->dev, d->nccl[g], buf, count);
}

// point-to-point between world ranks (never to oneself); a run of them is bracketed by p2p_begin / p2p_end (RCCL group)
inline int32_t comm_send(madqp_dist* d, const double* buf, int64_t count, int dst) {
    if (count <= 0) return 0;
    d->bytes_sent += 8 * count;
    if (d->host)  // (out only: buf is not written)
        return host_staged(d, const_cast<double*>(buf), count, true, false, [&](const madqp_comm_ops* h, void* hb) {
            return h->send(h->user, hb, count * 8, dst);
        });
    return dop_nccl_send(d->dev, d->nccl[GRP_WORLD], buf, count, dst);
}
inline int32_t comm_recv(madqp_dist* d, double* buf, int64_t count, int src) {
    if (count <= 0) return 0;
    if (d->host)
        return host_staged(d, buf, count, false, true, [&](const madqp_comm_ops* h, void* hb) {
            return h->recv(h->user, hb, count * 8, src);
        });
    return dop_nccl_recv(d->dev, d->nccl[GRP_WORLD], buf, count, src);
}
inline int32_t comm_p2p_begin(madqp_dist* d) { return d->host ? 0 : dop_nccl_group(d->dev, 1); }
inline int32_t comm_p2p_end(madqp_dist* d) { return d->host ? 0 : dop_nccl_group(d->dev, 0); }

// ---------------------------------------------------------------- factorisation
// Streams (HIP build; no-ops in the CPU build).  The rank-local KERNELS of a rank all run on one stream, U, in program
// order; the COLLECTIVES (and the small packing kernels between them) run on a second stream, P.  (The chain kernels
// are deliberately NOT put beside the update GEMM on a stream of their own: the diagonal-block kernel needs a whole
// CU's LDS and starves behind a GEMM launch that keeps refilling every slot -- measured on one MI355X: 1.5 ms instead
// of 60 us per block.)
//
// Look-ahead (what U and P see for step k -> k+1; "mine" = my process column holds tile column k+1):
//   U  wait for the operands of step k (P)
//   U  mine:  update k on tile column k+1 -> diagonal tile k+1 (owner) -> [P: its broadcast down the column] ->
//             panel solve k+1 -> pack the row operand of step k+1
//   P  wait for U up to here, then the operand exchange of step k+1: row broadcast, transposed column broadcasts
//   U  the BULK of update k (every other tile column)
// so the whole panel phase of step k+1 and both of its broadcast stages are queued BEFORE the bulk of update k on every
// rank and travel while it runs; X/Y of step k+1 land in the other half of the double buffer, which update k-1 (already
// behind on U when P is released) was the last to read.  tests/csrc/dist_cpu.cpp records the dop_mark() sequence and
// tests/test_dist2d.py asserts this order.
enum { ST_U = 0, ST_P = 1 };
enum { MK_UPDATE_COL = 1, MK_POTRF = 2, MK_DIAG_BCAST = 3, MK_TRSM = 4, MK_PACK = 5, MK_EXCHANGE = 6, MK_BULK = 7 };

struct StepGeom {
    int64_t w, lr, lc, r0, c0, ldx, ldy;
    int kp, kq;
};
inline StepGeom geom(const madqp_dist* d, int64_t k) {
    StepGeom g;
    g.w = tsize(d, k);
    g.kp = (int)(k % d->P);
    g.kq = (int)(k % d->Q);
    g.lr = k / d->P;
    g.lc = k / d->Q;
    g.r0 = first_after(k, d->p, d->P);
    g.c0 = first_after(k, d->q, d->Q);
    g.ldx = g.r0 < d->mt ? d->ld - g.r0 * d->nb : 0;  // rows of the row operand incl. padding (multiple of 128)
    g.ldy = g.c0 < d->nt ? d->ncp - g.c0 * d->nb : 0;
    return g;
}

// Where the operands live.  Every rank keeps the row operands X_p(k) = L[{I = p mod P}, k] and the column operands
// Y_q(k) = L[{J = q mod Q}, k] of ALL steps k it has seen -- its tile rows and tile columns of L, (1/P + 1/Q) n^2/2
// entries -- so that a tile column is brought up to date by ONE wide product when it is needed (update_col_range)
// instead of being read, modified and written once per step.  In a process row of ONE rank (Q == 1) the row operands are
// the factored panels of the local matrix themselves; on a 1 x 1 grid so are the column operands.
inline bool x_in_place(const madqp_dist* d) { return !group_traffic(d, GRP_ROW); }
inline bool y_is_x(const madqp_dist* d) { return single_rank(d); }
inline int level_of(const madqp_dist* d, int64_t k) {
    int s = 0;
    while (s + 1 < d->nlev && k >= d->lev_k0[s + 1]) ++s;
    return s;
}
// Block k of the row operands as a column-major array addressed by LOCAL ROW: element (i, c) at ptr[i + c * (*ld)].
// Only rows >= first_after(k) nb exist (the pointer is virtual above them).  In place (Q == 1): the factored panel k of
// the local matrix.
inline double* xw_block(const madqp_dist* d, int64_t k, int64_t* ld) {
    if (!d->XW) {
        *ld = d->ld;
        return d->K + k * d->nb * d->ld;
    }
    const int s = level_of(d, k);
    *ld = d->xl_ld[s];
    return d->XW + d->xl_off[s] + (k - d->lev_k0[s]) * d->nb * d->xl_ld[s] - d->xl_row0[s];
}
// Block k of the column operands addressed by LOCAL COLUMN (rows >= first_after(k) nb of it exist)
inline double* yw_block(const madqp_dist* d, int64_t k, int64_t* ld) {
    if (!d->YW) return xw_block(d, k, ld);  // 1 x 1 grid: local order = global order, Y = X
    const int s = level_of(d, k);
    *ld = d->yl_ld[s];
    return d->YW + d->yl_off[s] + (k - d->lev_k0[s]) * d->nb * d->yl_ld[s] - d->yl_row0[s];
}

// step k on the ranks of process column k mod Q (stream U, the diagonal tile's broadcast on P in between):
// diagonal tile, panel solve, row operand packed
inline int32_t panel_chain(madqp_dist* d, int64_t k) {
    Dev* dev = d->dev;
    const StepGeom g = geom(d, k);
    if (d->q != g.kq) return 0;
    const int64_t nb = d->nb, ld = d->ld, w = g.w;
    if (!group_traffic(d, GRP_COL)) {
        // A process column of ONE rank holds the whole panel: no diagonal tile to broadcast, no separate panel solve --
        // the panel goes through the one-GPU panel factorisation as it stands (chol.hip: recursive, its in-panel
        // products over the full panel height), which also leaves [info | inverse blocks | L_kk] in diagbuf
        dop_mark(dev, MK_POTRF, k);
        DTRY(dop_panel_local(dev, d->K, ld, g.lc, k, nb, w, d->diagbuf, d->info_dev));
        DTRY(dop_copy(dev, d->Wdiag + g.lr * d->wslot, d->diagbuf + IMG_HDR, img_blocks(w)));  // for the solves
    } else {
        if (d->p == g.kp) {
            dop_mark(dev, MK_POTRF, k);
            DTRY(dop_potrf_tile(dev, d->K + g.lr * nb + g.lc * nb * ld, ld, w, d->diagbuf, k * nb, d->info_dev));
            DTRY(dop_copy(dev, d->Wdiag + g.lr * d->wslot, d->diagbuf + IMG_HDR, img_blocks(w)));  // for the solves
        }
        DTRY(dop_link(dev, ST_U, ST_P));
        DTRY(dop_stream(dev, ST_P));
        dop_mark(dev, MK_DIAG_BCAST, k);
        DTRY(comm_bcast(d, d->diagbuf, img_count(w, w), g.kp, GRP_COL));
        DTRY(dop_link(dev, ST_P, ST_U));
        DTRY(dop_stream(dev, ST_U));
        if (d->p != g.kp) DTRY(dop_info_merge(dev, d->info_dev, d->diagbuf));
        if (g.r0 < d->mt) {  // C <- C L_kk^-T for my tile rows below k
            const double* Wk = d->diagbuf + IMG_HDR;
            const double* Lk = d->diagbuf + img_L(w);  // w x w, leading dimension w
            dop_mark(dev, MK_TRSM, k);
            DTRY(dop_trsm(dev, d->K + g.r0 * nb + g.lc * nb * ld, ld, d->mloc - g.r0 * nb, g.ldx, Lk, w, Wk, w));
        }
    }
    if (!x_in_place(d)) {
        double* X = d->Xrow[k & 1];
        dop_mark(dev, MK_PACK, k);
        DTRY(dop_info_store(dev, d->info_dev, X));  // the header carries info to every rank
        if (g.ldx > 0) DTRY(dop_copy2d(dev, X + IMG_HDR, g.ldx, d->K + g.r0 * nb + g.lc * nb * ld, ld, g.ldx, w));
    }
    return 0;
}

// the tile columns J > k of process column q that process row pr holds in its row operand: lj = lj0 + t*s, t < cnt;
// tile J sits at row ((J div P) - r0(pr)) * nb of that operand and successive ones are (Q/g) * nb rows apart
struct SegPlan {
    int64_t lj0, s, cnt, jstep;
};
inline int64_t gcd64(int64_t a, int64_t b) { return b ? gcd64(b, a % b) : a; }
inline SegPlan seg_plan(const madqp_dist* d, const StepGeom& g, int pr) {
    SegPlan sp{0, 1, 0, 1};
    const int64_t gg = gcd64(d->P, d->Q);
    sp.s = d->P / gg;      // period of (lj*Q + q) mod P in lj
    sp.jstep = d->Q / gg;  // (J_{t+1} - J_t) / P
    int64_t lj = g.c0;
    for (int64_t i = 0; i < sp.s && lj < d->nt; ++i, ++lj)
        if ((lj * d->Q + d->q) % d->P == pr) break;
    if (lj >= d->nt || (lj * d->Q + d->q) % d->P != pr) return sp;
    sp.lj0 = lj;
    sp.cnt = (d->nt - 1 - lj) / sp.s + 1;
    return sp;
}

// step k (stream P): the pieces of tile column k that belong to the diagonal triangle of its solve group -- the diagonal
// image [inverse blocks | L_kk] from rank (k mod P, k mod Q), the tiles (I, k), k < I < end of the group, from ranks
// (I mod P, k mod Q) -- travel to the group's owner, which files them in its band slot (ld = G nb)
inline int32_t band_collect(madqp_dist* d, int64_t k) {
    Dev* dev = d->dev;
    const StepGeom g = geom(d, k);
    const int64_t nb = d->nb, ld = d->ld, w = g.w, G = d->G;
    const int64_t grp = k / G, j = k - grp * G, gend = std::min((grp + 1) * G, d->T);
    const int owner = (int)(grp % d->world);
    const int64_t slot = grp / d->world, ldb = G * nb;
    const int64_t dcount = img_blocks(w) + w * w;  // the diagonal image without its header
    if (single_rank(d)) return 0;  // one rank solves with the factor where it is (solve: dop_solve_local)
    // force_comm (one rank going through every collective of the schedule, RCCL's point-to-point calls included): a piece
    // whose source is the owner is SENT TO ONESELF and received in a second staging area, inside the same group call
    // -- otherwise ncclSend / ncclRecv / the group bracket would never run on the hardware a one-GPU box has
    const bool self_p2p = d->force_comm && d->bstage2;
    double* rstage = self_p2p ? d->bstage2 : d->bstage;  // where the owner finds the pieces
    bool any = false;  // do I send or receive anything?
    for (int64_t I = k; I < gend; ++I) {
        const int src = (int)((I % d->P) * d->Q + g.kq);
        any = any || ((src != owner || self_p2p) && (d->rank == src || d->rank == owner));
    }
    // pack what I hold (stage region of piece I: the diagonal image first, then one nb x w slab per tile)
    for (int64_t I = k; I < gend; ++I) {
        const int src = (int)((I % d->P) * d->Q + g.kq);
        if (d->rank != src) continue;
        if (I == k) {
            DTRY(dop_copy(dev, d->bstage, d->diagbuf + IMG_HDR, dcount));
        } else {
            const int64_t rows = tsize(d, I);
            DTRY(dop_copy2d(dev, d->bstage + d->wslot + nb * nb + (I - k - 1) * nb * nb, rows,
                            d->K + (I / d->P) * nb + g.lc * nb * ld, ld, rows, w));
        }
    }
    if (any) {
        DTRY(comm_p2p_begin(d));
        int32_t rp = 0;  // an error inside the bracket must not leave the RCCL group open: every later collective of this
                         // process would be queued into it and never launch (a hang instead of an error return)
        for (int64_t I = k; I < gend && !rp; ++I) {
            const int src = (int)((I % d->P) * d->Q + g.kq);
            if (src == owner && !self_p2p) continue;
            const int64_t poff = (I == k) ? 0 : d->wslot + nb * nb + (I - k - 1) * nb * nb;
            const int64_t cnt = (I == k) ? dcount : tsize(d, I) * w;
            if (d->rank == src) rp = comm_send(d, d->bstage + poff, cnt, owner);
            if (!rp && d->rank == owner) rp = comm_recv(d, (src == owner ? rstage : d->bstage) + poff, cnt, src);
        }
        const int32_t re = comm_p2p_end(d);
        DTRY(rp);
        DTRY(re);
    }
    if (d->rank == owner) {
        // a piece lies where it was packed (bstage) or received (bstage; bstage2 when it was sent to oneself)
        auto piece = [&](int64_t I, int64_t poff) {
            const int src = (int)((I % d->P) * d->Q + g.kq);
            return (src == owner ? rstage : d->bstage) + poff;
        };
        double* B = d->band + slot * d->bslot;
        const double* dimg = piece(k, 0);
        DTRY(dop_copy(dev, d->bandW + slot * d->bwslot + j * d->wslot, dimg, img_blocks(w)));
        DTRY(dop_copy2d(dev, B + j * nb + j * nb * ldb, ldb, dimg + img_blocks(w), w, w, w));
        for (int64_t I = k + 1; I < gend; ++I) {
            const int64_t rows = tsize(d, I);
            DTRY(dop_copy2d(dev, B + (I - grp * G) * nb + j * nb * ldb, ldb,
                            piece(I, d->wslot + nb * nb + (I - k - 1) * nb * nb), rows, rows, w));
        }
    }
    return 0;
}

// step k on every rank (stream P, after everything queued on U so far): the row operand travels along the process
// rows, the column operand arrives by one broadcast down every process column per source row; both are filed in the
// operand stores (XW / YW block k)
inline int32_t operands_exchange(madqp_dist* d, int64_t k) {
    Dev* dev = d->dev;
    const StepGeom g = geom(d, k);
    const int64_t nb = d->nb, w = g.w;
    DTRY(dop_link(dev, ST_U, ST_P));
    DTRY(dop_stream(dev, ST_P));
    dop_mark(dev, MK_EXCHANGE, k);
    int64_t ldxw = 0, ldyw = 0;
    double* xblk = xw_block(d, k, &ldxw) + g.r0 * nb;  // first valid row of block k of the row operands
    if (!x_in_place(d)) {
        double* X = d->Xrow[k & 1];
        DTRY(comm_bcast(d, X, IMG_HDR + g.ldx * w, g.kq, GRP_ROW));
        if (d->q != g.kq) DTRY(dop_info_merge(dev, d->info_dev, X));
        if (g.ldx > 0) DTRY(dop_copy2d(dev, xblk, ldxw, X + IMG_HDR, g.ldx, g.ldx, w));
    }
    if (!y_is_x(d)) {
        double* yblk = yw_block(d, k, &ldyw);  // block k of the column operands, row = local column (rows >= c0 nb exist)
        for (int pr = 0; pr < d->P; ++pr) {
            const SegPlan sp = seg_plan(d, g, pr);
            if (sp.cnt == 0) continue;
            const int64_t J0 = sp.lj0 * d->Q + d->q;
            const int64_t yoff = sp.lj0 * nb;
            if (!group_traffic(d, GRP_COL)) {  // P == 1, my row operand has every tile: rows -> column operand, one launch
                const int64_t xoff = (J0 / d->P - g.r0) * nb;
                DTRY(dop_gather_tiles(dev, yblk + yoff, ldyw, sp.s * nb, xblk + xoff, ldxw, sp.jstep * nb, sp.cnt, nb, w,
                                      d->ncp - yoff, sp.s * nb, 0));
                continue;
            }
            if (d->p == pr) {  // pack my tiles (zero padded to nb rows): one launch
                const int64_t xoff = (J0 / d->P - g.r0) * nb;
                DTRY(dop_gather_tiles(dev, d->seg, nb, nb * nb, xblk + xoff, ldxw, sp.jstep * nb, sp.cnt, nb, w,
                                      g.ldx - xoff, sp.jstep * nb, 1));
            }
            DTRY(comm_bcast(d, d->seg, sp.cnt * nb * nb, pr, GRP_COL));
            DTRY(dop_gather_tiles(dev, yblk + yoff, ldyw, sp.s * nb, d->seg, nb, nb * nb, sp.cnt, nb, w, d->ncp - yoff,
                                  sp.s * nb, 0));
        }
    }
    DTRY(band_collect(d, k));     // behind the broadcasts: nothing in the factorisation waits for it
    DTRY(dop_stream(dev, ST_U));  // U goes on without waiting; the consumer of the operands links P -> U
    return 0;
}

// first local tile row li with global tile I = li P + p >= J, and whether that tile is the diagonal one (I == J)
inline int64_t first_lower(const madqp_dist* d, int64_t J, bool* has_diag) {
    const int64_t li0 = first_after(J - 1, d->p, d->P);
    *has_diag = (li0 * d->P + d->p == J);
    return li0;
}

// Local tile column lj (global J) receives the panels ka .. kb-1 (all < J) in ONE product:
//   C[I, J] -= sum_{k = ka}^{kb-1} X_p(k)[I] Y_q(k)[J]'   for my tile rows I >= J,   K = (kb - ka) nb
inline int32_t update_col_range(madqp_dist* d, int64_t lj, int64_t ka, int64_t kb) {
    const int64_t nb = d->nb, J = lj * d->Q + d->q;
    if (ka >= kb || lj >= d->nt) return 0;
    bool has_diag = false;
    const int64_t li0 = first_lower(d, J, &has_diag);
    if (li0 >= d->mt) return 0;
    const int64_t M = d->mloc - li0 * nb, N = tsize(d, J);
    if (M <= 0 || N <= 0) return 0;
    // 128-wide tile columns of the nb-wide tile column: when its first local tile is the diagonal tile (I == J) only that
    // tile's lower 128-tiles are needed -- nothing reads the upper triangle of a diagonal tile of K (28 of its 64
    // 128-tiles at nb = 1024: 2 % of a wide update, 1.8 % of the assembly)
    std::vector<int64_t> row0((size_t)((N + 127) / 128), 0);
    if (has_diag)
        for (size_t tc = 0; tc < row0.size(); ++tc) row0[tc] = (int64_t)tc;
    double* C = d->K + li0 * nb + lj * nb * d->ld;
    // one product per level of the operand staircases the range touches (a level has one leading dimension)
    for (int64_t k = ka; k < kb;) {
        const int s = level_of(d, k);
        const int64_t ke = std::min<int64_t>(kb, d->lev_k0[s + 1]);
        int64_t ldx = 0, ldy = 0;
        const double* X = xw_block(d, k, &ldx) + li0 * nb;
        const double* Y = yw_block(d, k, &ldy) + lj * nb;
        DTRY(dop_gemm(d->dev, C, d->ld, C, d->ld, X, ldx, Y, ldy, M, N, (ke - k) * nb, -1.0, 1.0, d->ld - li0 * nb,
                      (d->YW ? d->ncp : d->ld) - lj * nb, row0.data()));
        k = ke;
    }
    return 0;
}

// C[I, J] = Cin[I, J] + X[I] Y[J]' for ALL local lower tiles (I >= J): the assembly K = H + A' Theta A with
// X = the columns of A of my tile rows (k-major), Y = Theta times the columns of A of my tile columns; Cin may be null
inline int32_t assemble_product(madqp_dist* d, const double* Cin, int64_t ldcin, const double* X, int64_t ldx,
                                const double* Y, int64_t ldy, int64_t kdim) {
    if (d->mloc == 0 || d->nloc == 0) return 0;
    const int64_t t128 = d->nb / 128, tiles_n = (d->nloc + 127) / 128;
    std::vector<int64_t> row0((size_t)tiles_n);
    for (int64_t tn = 0; tn < tiles_n; ++tn) {
        bool has_diag = false;  // lower 128-tiles of a diagonal tile only (update_col_range)
        const int64_t li0 = first_lower(d, (tn / t128) * d->Q + d->q, &has_diag);
        row0[(size_t)tn] = li0 * t128 + (has_diag ? tn % t128 : 0);
    }
    return dop_gemm(d->dev, d->K, d->ld, Cin, ldcin, X, ldx, Y, ldy, d->mloc, d->nloc, kdim, 1.0, Cin ? 1.0 : 0.0,
                    d->ld, d->ncp, row0.data());
}

inline int32_t factor_steps(madqp_dist* d) {
    Dev* dev = d->dev;
    for (int64_t lj = 0; lj < d->nt; ++lj) d->done[lj] = 0;
    DTRY(panel_chain(d, 0));
    DTRY(operands_exchange(d, 0));
    for (int64_t k = 0; k + 1 < d->T; ++k) {
        const int64_t nxt = k + 1;
        const bool mine = (d->q == (int)(nxt % d->Q));  // my process column holds tile column k+1
        DTRY(dop_link(dev, ST_P, ST_U));                // the operands of step k have arrived
        if (mine) {  // the column that becomes the panel: whatever it has not received yet (at least panel k)
            const int64_t lj = nxt / d->Q;
            dop_mark(dev, MK_UPDATE_COL, k);
            DTRY(update_col_range(d, lj, d->done[lj], nxt));
            d->done[lj] = nxt;
            DTRY(panel_chain(d, nxt));
        }
        DTRY(operands_exchange(d, nxt));  // queued on P before the background update is queued on U
        // background: my NEXT tile column is brought up to date with every panel that has arrived (the first time:
        // one product over all of them, K = (k+1) nb; afterwards one panel per step) while the chain of the steps
        // in between runs on the other process columns.  A single rank has nobody to overlap with: its next column
        // is the panel of the next step and gets everything there, in one product (the plain left-looking schedule).
        dop_mark(dev, MK_BULK, k);
        if (single_rank(d)) continue;
        int64_t lja = mine ? nxt / d->Q + 1 : first_after(nxt, d->q, d->Q);
        if (lja < d->nt && d->done[lja] < nxt) {
            DTRY(dop_bulk(dev, 1));  // leaves room for the collectives' kernels (dist.hip)
            const int32_t r = update_col_range(d, lja, d->done[lja], nxt);
            DTRY(dop_bulk(dev, 0));
            DTRY(r);
            d->done[lja] = nxt;
        }
    }
    return 0;
}

inline int32_t factor(madqp_dist* d, int32_t* info_host) {
    Dev* dev = d->dev;
    d->factored = 0;
    DTRY(dop_zero(dev, d->info_dev, 1));
    if (d->T == 0) {
        *info_host = 0;
        d->factored = 1;
        return 0;
    }
    DTRY(dop_fork(dev));
    const int32_t r = factor_steps(d);
    const int32_t rj = dop_join(dev);  // ALWAYS: nothing stays queued on the internal streams behind the caller's back
    DTRY(r);
    DTRY(rj);
    double info = 0.0;
    DTRY(dop_d2h(dev, &info, d->info_dev, sizeof(double)));
    *info_host = (int32_t)info;
    d->factored = 1;  // completed (with unit pivots from column `info` on when info > 0, as the one-GPU factorisation)
    return 0;
}

// ---------------------------------------------------------------- solves: rhs (n doubles, replicated) <- (L L')^-1 rhs
// Sweeps over groups of G tiles.  A rank accumulates the partial sums of the tile rows (forward) / tile columns
// (backward) it holds; per group: ONE reduce of the group's partial sums to the group's owner, ONE local triangular
// solve of order <= G nb there (the band slot, sweep kernels of chol.hip), ONE broadcast of the solved rows to everyone
// -- the solution ends up replicated without an all-gather -- then the products with the local tiles outside the
// group's triangle.
// One group of one sweep (trans = 0 forward, 1 backward): the group's partial sums -- `loc`, kept in local order over
// residue r of R -- are reduced to the group's owner, which subtracts them from the group's rows of rhs, solves with its
// band slot and broadcasts the solved rows
inline int32_t group_solve(madqp_dist* d, int32_t trans, int64_t grp, double* rhs, const double* loc, int64_t R, int64_t r) {
    Dev* dev = d->dev;
    const int64_t nb = d->nb, G = d->G, I0 = grp * G, I1 = std::min(I0 + G, d->T);
    const int64_t wg = std::min(d->n, I1 * nb) - I0 * nb, slot = grp / d->world;
    const int owner = (int)(grp % d->world);
    double* bg = rhs + I0 * nb;
    DTRY(dop_group_pack(dev, d->gvec, loc, I0, wg, nb, R, r));
    DTRY(comm_reduce(d, d->gvec, wg, owner, GRP_WORLD));
    if (d->rank == owner) {
        DTRY(dop_vsub(dev, bg, d->gvec, wg));
        DTRY(dop_tile_solve(dev, trans, d->band + slot * d->bslot, G * nb, d->bandW + slot * d->bwslot, bg, wg, d->vtile));
    }
    return comm_bcast(d, bg, wg, owner, GRP_WORLD);
}

inline int32_t solve(madqp_dist* d, double* rhs) {
    Dev* dev = d->dev;
    const int64_t nb = d->nb, ld = d->ld, G = d->G;
    if (d->T == 0) return 0;
    if (single_rank(d)) return dop_solve_local(dev, rhs);  // the factor is the local matrix
    if (d->mloc) DTRY(dop_zero(dev, d->sloc, d->mloc));
    if (d->nloc) DTRY(dop_zero(dev, d->tloc, d->nloc));
    // forward: y_g = B_g^-1 (b_g - sum_{J before g} L[g, J] y_J)
    for (int64_t grp = 0; grp < d->NG; ++grp) {
        const int64_t I0 = grp * G, I1 = std::min(I0 + G, d->T);
        DTRY(group_solve(d, 0, grp, rhs, d->sloc, d->P, d->p));
        const int64_t r0 = first_after(I1 - 1, d->p, d->P);  // my tile rows below the group
        const int64_t rows = d->mloc - r0 * nb;
        if (r0 < d->mt && rows > 0)
            for (int64_t J = I0; J < I1; ++J)  // s[rows] += L[rows, J] y_J: the panel as `w` rows of length `rows`
                if (J % d->Q == d->q)
                    DTRY(dop_gemv(dev, 1, tsize(d, J), rows, 1.0, d->K + r0 * nb + (J / d->Q) * nb * ld, ld, rhs + J * nb, 1.0,
                                  d->sloc + r0 * nb));
    }
    // backward: x_g = B_g^-T (y_g - sum_{I after g} L[I, g]' x_I)
    for (int64_t grp = d->NG - 1; grp >= 0; --grp) {
        const int64_t I0 = grp * G, I1 = std::min(I0 + G, d->T);
        DTRY(group_solve(d, 1, grp, rhs, d->tloc, d->Q, d->q));
        const int64_t cend = first_after(I0 - 1, d->q, d->Q);  // my tile columns with J < I0 (first_after(-1) = 0)
        const int64_t cols = std::min(cend * nb, d->nloc);
        if (I0 > 0 && cols > 0)
            for (int64_t I = I0; I < I1; ++I)  // t[cols] += L[I, cols]' x_I: `cols` rows of length w, stride ld
                if (I % d->P == d->p)
                    DTRY(dop_gemv(dev, 0, cols, tsize(d, I), 1.0, d->K + (I / d->P) * nb, ld, rhs + I * nb, 1.0, d->tloc));
    }
    return 0;
}

// ---------------------------------------------------------------- create / destroy
// Every device buffer of the handle, in the order they are allocated: where its pointer lives, its doubles (0: not
// needed on this grid) and the figure of madqp_dist_memory it counts under.  create sums it, allocate and destroy walk it.
struct DistBuf {
    double** ptr;
    int64_t count;
    int64_t* bytes;
};
inline std::vector<DistBuf> buffers(madqp_dist* d) {
    const int64_t nb = d->nb, stage = d->wslot + nb * nb + d->G * nb * nb;  // [diagonal image | G tiles]
    const int64_t xrow = x_in_place(d) ? 0 : IMG_HDR + d->ld * nb;          // broadcast image of a row operand
    const int64_t slots = std::max<int64_t>(d->my_groups, 1);
    return {
        {&d->K, d->ld * d->ncp + 128, &d->bytes_K},
        {&d->Wdiag, std::max<int64_t>(d->mt, 1) * d->wslot, &d->bytes_stage},
        {&d->diagbuf, img_count(nb, nb), &d->bytes_stage},
        {&d->Xrow[0], xrow, &d->bytes_stage},
        {&d->Xrow[1], xrow, &d->bytes_stage},
        {&d->XW, d->xw_count, &d->bytes_xw},
        {&d->YW, d->yw_count, &d->bytes_yw},
        {&d->seg, group_traffic(d, GRP_COL) ? std::max<int64_t>(d->nt, 1) * nb * nb : 0, &d->bytes_stage},  // transposed broadcasts
        {&d->vtile, 2 * d->G * nb + 64, &d->bytes_stage},
        {&d->band, slots * d->bslot, &d->bytes_band},
        {&d->bandW, slots * d->bwslot, &d->bytes_band},
        {&d->bstage, stage, &d->bytes_stage},
        {&d->bstage2, d->force_comm ? stage : 0, &d->bytes_stage},
        {&d->gvec, d->G * nb, &d->bytes_stage},
        {&d->sloc, d->ld, &d->bytes_stage},
        {&d->tloc, d->ncp, &d->bytes_stage},
        {&d->info_dev, 2, &d->bytes_stage},
    };
}
// out8 of madqp_dist_layout and madqp_dist_memory
inline void layout8(const madqp_dist* d, int64_t* out8) {
    const int64_t v[8] = {d->p, d->q, d->mt, d->nt, d->mloc, d->nloc, d->ld, d->ncp};
    memcpy(out8, v, sizeof(v));
}
inline void memory8(const madqp_dist* d, int64_t* out8) {
    const int64_t v[8] = {d->bytes_total, d->bytes_K, d->bytes_xw, d->bytes_yw, d->bytes_band, d->bytes_stage, d->nlev, 0};
    memcpy(out8, v, sizeof(v));
}

inline int32_t create(Dev* dev, int32_t rank, int32_t world, int32_t P, int32_t Q, int64_t n, int64_t nb,
                      const madqp_comm_ops* host, int32_t force_comm, madqp_dist** out) {
    *out = nullptr;
    if (P < 1 || Q < 1 || P * Q != world || rank < 0 || rank >= world || n < 0 || nb < 128 || nb % 128) return MADQP_ERR_ARG;
    madqp_dist* d = new (std::nothrow) madqp_dist();  // (every field zero)
    if (!d) return MADQP_ERR_ALLOC;
    d->dev = dev;
    d->rank = rank;
    d->world = world;
    d->P = P;
    d->Q = Q;
    d->p = rank / Q;
    d->q = rank % Q;
    d->n = n;
    d->nb = nb;
    d->T = (n + nb - 1) / nb;
    d->mt = count_tiles(d->T, d->p, P);
    d->nt = count_tiles(d->T, d->q, Q);
    d->mloc = local_extent(d, d->mt, d->p, P);
    d->nloc = local_extent(d, d->nt, d->q, Q);
    d->ld = pad128(d->mloc);
    d->ncp = pad128(d->nloc);
    d->host = host;
    d->force_comm = force_comm;  // (decides where the operands live: before anything is allocated)
    d->wslot = img_blocks(nb);
    // solve groups of G tiles: 4096 rows unless MADQP_DIST_GROUP says otherwise
    const char* genv = getenv("MADQP_DIST_GROUP");
    d->G = std::max<int64_t>(1, genv ? atoll(genv) : 4096 / nb);
    d->G = std::min<int64_t>(d->G, std::max<int64_t>(d->T, 1));
    d->NG = (d->T + d->G - 1) / d->G;
    d->bslot = d->G * nb * d->G * nb;
    d->bwslot = d->G * d->wslot;
    // (a single rank solves with the factor where it lies -- dop_solve_local -- and collects no bands)
    d->my_groups = single_rank(d) ? 0 : (d->NG > rank ? (d->NG - rank + world - 1) / world : 0);
    // levels of the operand staircases: ~T/24 steps each (at least 2; MADQP_DIST_LEVEL_STEPS), one level when both
    // operands are read in place.  Memory (1/2 + 1/(2 nlev)) of the rectangles; an update over several levels is one
    // product per level (K = a level's steps x nb >= 2 nb).
    {
        const char* lenv = getenv("MADQP_DIST_LEVEL_STEPS");
        int64_t lw = lenv ? atoll(lenv) : std::max<int64_t>(2, (d->T + 23) / 24);
        lw = std::max<int64_t>(lw, (d->T + DIST_MAXLEV - 1) / DIST_MAXLEV);
        if (lw < 1 || (x_in_place(d) && y_is_x(d))) lw = std::max<int64_t>(d->T, 1);
        d->nlev = (int32_t)std::max<int64_t>(1, (d->T + lw - 1) / lw);
        int64_t xo = 0, yo = 0;
        for (int sl = 0; sl < d->nlev; ++sl) {
            const int64_t k0 = sl * lw, k1 = std::min<int64_t>(d->T, k0 + lw);
            d->lev_k0[sl] = k0;
            d->lev_k0[sl + 1] = std::max<int64_t>(k1, k0);
            // rows a consumer of step >= k0 can read: tiles > k0
            d->xl_row0[sl] = std::min(first_after(k0, d->p, P) * nb, d->ld - 128);
            d->yl_row0[sl] = std::min(first_after(k0, d->q, Q) * nb, d->ncp - 128);
            d->xl_ld[sl] = d->ld - d->xl_row0[sl];
            d->yl_ld[sl] = d->ncp - d->yl_row0[sl];
            d->xl_off[sl] = xo;
            d->yl_off[sl] = yo;
            xo += d->xl_ld[sl] * (k1 - k0) * nb;
            yo += d->yl_ld[sl] * (k1 - k0) * nb;
        }
        d->xw_count = x_in_place(d) ? 0 : xo;
        d->yw_count = y_is_x(d) ? 0 : yo;
    }
    // every device buffer of the handle, sized BEFORE anything is allocated: a problem that does not fit is refused
    // with the figure, not inside the N-th allocation -- and refused by EVERY rank (allocate() below): byte totals and
    // free memory differ between ranks, and a rank that went on alone would wait for the others in the communicator
    // set-up or in its first collective for ever (ADVICE r4)
    for (const DistBuf& b : buffers(d)) *b.bytes += 8 * std::max<int64_t>(b.count, 0);
    d->bytes_total = d->bytes_K + d->bytes_xw + d->bytes_yw + d->bytes_band + d->bytes_stage;
    *out = d;  // (on an error the caller reads d->err and destroys it)
    const int64_t avail = dop_mem_free(dev);  // -1: unknown
    d->fits = !(avail >= 0 && d->bytes_total > avail);
    if (!d->fits)
        snprintf(d->err, sizeof(d->err),
                 "rank %d of the %d x %d grid needs %.2f GB of device memory (local matrix %lld x %lld: %.2f GB, stored "
                 "operands of the lazy updates %.2f + %.2f GB, solve bands %.2f GB) and %.2f GB are free",
                 rank, P, Q, d->bytes_total * 1e-9, (long long)d->ld, (long long)d->ncp, d->bytes_K * 1e-9, d->xw_count * 8e-9,
                 d->yw_count * 8e-9, d->bytes_band * 1e-9, avail * 1e-9);
    return 0;
}

// how many ranks of the world say "no" (mine = 0 / 1): ONE collective every rank takes part in -- the caller's host ops,
// or RCCL on a scratch word once the world communicator exists.  < 0: the collective itself failed.
inline int agree_count(madqp_dist* d, int mine) {
    double v = mine ? 1.0 : 0.0;
    if (single_rank(d)) return mine;
    if (d->host) return d->host->allreduce_sum(d->host->user, &v, 1, GRP_WORLD) ? -1 : (int)(v + 0.5);
    if (!d->nccl[GRP_WORLD]) return -1;
    double* t = (double*)dop_alloc(d->dev, sizeof(double));
    if (!t) return -1;
    int32_t r = dop_h2d(d->dev, t, &v, sizeof(double));
    if (!r) r = dop_nccl_allreduce(d->dev, d->nccl[GRP_WORLD], t, 1);
    if (!r) r = dop_d2h(d->dev, &v, t, sizeof(double));  // (synchronises the stream the collective ran on)
    dop_free(d->dev, t);
    return r ? -1 : (int)(v + 0.5);
}

// Second half of the set-up, COLLECTIVE over the world (after the communicators exist): the ranks agree that every one of
// them can hold its share, allocate, and agree again that every allocation succeeded -- a rank never goes on alone.
inline int32_t allocate(madqp_dist* d) {
    Dev* dev = d->dev;
    int bad = agree_count(d, d->fits ? 0 : 1);
    if (bad != 0) {
        if (bad < 0)
            snprintf(d->err, sizeof(d->err), "the ranks could not agree on the memory verdict (collective failed)");
        else if (d->fits)
            snprintf(d->err, sizeof(d->err), "%d other rank(s) of the %d x %d grid cannot hold their share of the problem "
                     "(rank %d could: %.2f GB); every rank refuses", bad, d->P, d->Q, d->rank, d->bytes_total * 1e-9);
        return bad < 0 ? MADQP_ERR_STATE : MADQP_ERR_ALLOC;
    }
    bool ok = true;
    for (const DistBuf& b : buffers(d)) {
        if (b.count <= 0 || !ok) continue;
        *b.ptr = (double*)dop_alloc(dev, (size_t)b.count * sizeof(double));
        ok = *b.ptr != nullptr;
    }
    d->done = (int64_t*)calloc((size_t)std::max<int64_t>(d->nt, 1), sizeof(int64_t));
    ok = ok && d->done;
    bad = agree_count(d, ok ? 0 : 1);
    if (bad != 0) {
        if (!ok)
            snprintf(d->err, sizeof(d->err), "device allocation failed (%.2f GB in all; local matrix %lld x %lld)",
                     d->bytes_total * 1e-9, (long long)d->ld, (long long)d->ncp);
        else
            snprintf(d->err, sizeof(d->err), "a device allocation failed on %d other rank(s); every rank refuses", bad);
        return MADQP_ERR_ALLOC;
    }
    return 0;
}

inline void destroy(madqp_dist* d) {
    if (!d) return;
    Dev* dev = d->dev;
    dop_sync(dev);
    free(d->done);
    for (const DistBuf& b : buffers(d))
        if (*b.ptr) dop_free(dev, *b.ptr);
    free(d->hostbuf);
    delete d;
}

}  // namespace distcore
