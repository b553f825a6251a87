// Test infrastructure: the launch plan and the tile table of the fp64 MFMA product (madqp_jl_amd/csrc/gemm_plan.inc)
// behind C entry points, so that tests/test_gemm_plan.py can hold their rules without a GPU.
#include "../../madqp_jl_amd/csrc/gemm_plan.inc"

// modes[7]: splitk, tailsplit, seg_rounds, xcd, batch_xcd, patch_m, patch_n (null: the defaults).
// out[12]: ntiles, whole, ksplit, kchunk, segments, tail_tiles, tail_split, tail_chunk, persistent, batch_xcd, gy,
// work_bytes; seg_out (optional, max_seg entries): the tiles of each segment.
static GemmModes modes_of(const int64_t* modes) {
    GemmModes m;
    if (modes) {
        m.splitk = (int)modes[0], m.tailsplit = (int)modes[1], m.seg_rounds = (int)modes[2], m.xcd = (int)modes[3];
        m.batch_xcd = (int)modes[4], m.patch_m = modes[5], m.patch_n = modes[6];
    }
    return m;
}

extern "C" void gemm_plan_c(int64_t ntiles, int64_t K, int64_t slots, int64_t cap_slots, int form, int64_t B,
                            const int64_t* modes, int64_t* out, int64_t* seg_out, int64_t max_seg) {
    const GemmPlan p = gemm_plan(ntiles, K, slots, cap_slots, (GemmBatchForm)form, B, modes_of(modes));
    const int64_t f[12] = {p.ntiles, p.whole, p.ksplit, p.kchunk, p.segments, p.tail_tiles, p.tail_split, p.tail_chunk,
                           p.persistent, p.batch_xcd, (int64_t)p.gy, (int64_t)p.work_bytes};
    for (int i = 0; i < 12; ++i) out[i] = f[i];
    int64_t n = 0;
    for (int64_t off = 0; p.segments && off < p.whole && n < max_seg; off += seg_out[n++]) seg_out[n] = gemm_segment(p, off);
}

// The table of an M x N product; returns its length and writes up to max_out packed entries.
extern "C" int64_t gemm_tile_table_c(int64_t M, int64_t N, int lower_only, int64_t diag_off, int kind, const int64_t* mask,
                                     int64_t nmask, const int64_t* modes, int32_t* out, int64_t max_out) {
    const GemmModes m = modes_of(modes);
    const std::vector<int32_t> t =
        gemm_tile_table(M, N, lower_only != 0, diag_off, (GemmMask)kind, mask, nmask, m.patch_m, m.patch_n);
    for (size_t i = 0; i < t.size() && (int64_t)i < max_out; ++i) out[i] = t[i];
    return (int64_t)t.size();
}

extern "C" void gemm_default_modes_c(int64_t* modes) {
    const GemmModes m;
    const int64_t f[7] = {m.splitk, m.tailsplit, m.seg_rounds, m.xcd, m.batch_xcd, m.patch_m, m.patch_n};
    for (int i = 0; i < 7; ++i) modes[i] = f[i];
}
