// Test infrastructure: the host-side rules of the KKT object (madqp_jl_amd/csrc/kkt_form.inc) behind C entry points, so
// that tests/test_kkt_form.py can hold them without a GPU.
#include "../../madqp_jl_amd/csrc/kkt_form.inc"

extern "C" int kkt_slot_map_c(const int64_t* ind_ineq, int64_t ns, int64_t m, int64_t* slot_out) {
    return kkt_slot_map(ind_ineq, ns, m, slot_out) ? 1 : 0;
}

// out[5]: rule_order, np, stored_order, ldk, k_doubles
extern "C" void kkt_orders_c(int mode, int64_t nx, int64_t m, int64_t* out) {
    const KktOrders o = kkt_orders(mode, nx, m);
    const int64_t f[5] = {o.rule_order, o.np, o.stored_order, o.ldk, o.k_doubles};
    for (int i = 0; i < 5; ++i) out[i] = f[i];
}

extern "C" int64_t kkt_pattern_halfbandwidth_c(int64_t rows, const int64_t* ptr, const int64_t* col) {
    return kkt_pattern_halfbandwidth(rows, ptr, col);
}

extern "C" int64_t kkt_csr_halfbandwidth_c(int64_t n, const int64_t* ptr, const int64_t* col) {
    return kkt_csr_halfbandwidth(n, ptr, col);
}
