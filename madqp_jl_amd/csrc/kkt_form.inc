// Host-side rules of the KKT object (kkt.hip; the slot map also for batch.hip and dist.hip): plain C++17 -- no HIP, no
// context, no environment -- so that tests/test_kkt_form.py holds them through a CPU build (tests/csrc/kkt_form_cpu.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

enum { KKT_CONDENSED = 0, KKT_NORMAL = 1, KKT_AUGMENTED = 2 };

// Slot map of ind_ineq (ns rows, strictly increasing, in [0, m)): slot_out[row] = slack index of an inequality row, -1 for
// an equality row.  false: the list is not such a list (slot_out is then partly written).
inline bool kkt_slot_map(const int64_t* ind_ineq, int64_t ns, int64_t m, int64_t* slot_out) {
    std::fill(slot_out, slot_out + std::max<int64_t>(m, 0), (int64_t)-1);
    for (int64_t k = 0; k < ns; ++k) {
        const int64_t r = ind_ineq[k];
        if (!(r >= 0 && r < m && (k == 0 || ind_ineq[k - 1] < r))) return false;
        slot_out[r] = k;
    }
    return true;
}

// The two orders of the factorised matrix.  They differ in the augmented form alone, and both are right:
//   rule_order    nx / m / nx + m: the order of the mathematical system -- what the AUTO rule of madqp_kkt_set_refine
//                 (and madqp_jl_amd/options.py) compares with its threshold and madqp_kkt_set_bandwidth bounds bw by;
//   stored_order  nx / m / np + m: the order madqp_chol_create gets and madqp_kkt_chol reports -- the augmented matrix keeps
//                 its constraint rows at np = ceil128(nx), behind identity padding, so that the (2,2) block starts a tile.
// ldk: leading dimension AND column count of dense storage, padded to a multiple of 128 (zero filled) so that every GEMM
// tile of the factorisation is a full tile; k_doubles: that plus 128 doubles of slack behind the last column (room for
// 16-byte tile loads at the edge).
struct KktOrders {
    int64_t rule_order, np, stored_order, ldk, k_doubles;
};
inline KktOrders kkt_orders(int mode, int64_t nx, int64_t m) {
    KktOrders o;
    o.np = (nx + 127) / 128 * 128;
    o.rule_order = (mode == KKT_NORMAL) ? m : (mode == KKT_AUGMENTED) ? nx + m : nx;
    o.stored_order = (mode == KKT_NORMAL) ? m : (mode == KKT_AUGMENTED) ? o.np + m : nx;
    o.ldk = std::max<int64_t>(128, (o.stored_order + 127) / 128 * 128);
    o.k_doubles = o.ldk * o.ldk + 128;
    return o;
}

// Half-bandwidth of V diag(w) V' from the CSR of V' (rows x order, column indices ascending within a row): entry (i, j) needs
// a row of V' that holds both i and j, so it is the max over the rows of (last - first column).
inline int64_t kkt_pattern_halfbandwidth(int64_t rows, const int64_t* ptr, const int64_t* col) {
    int64_t bw = 0;
    for (int64_t i = 0; i < rows; ++i)
        if (ptr[i + 1] > ptr[i]) bw = std::max(bw, col[ptr[i + 1] - 1] - col[ptr[i]]);
    return bw;
}
// Half-bandwidth of a symmetric matrix of order n in CSR: max |col - row|.
inline int64_t kkt_csr_halfbandwidth(int64_t n, const int64_t* ptr, const int64_t* col) {
    int64_t bw = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = ptr[i]; p < ptr[i + 1]; ++p) bw = std::max<int64_t>(bw, std::llabs(col[p] - i));
    return bw;
}
