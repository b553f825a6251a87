// Test infrastructure: the layout of packed band storage (madqp_jl_amd/csrc/band_plan.inc) behind C entry points, so that
// tests/test_band_packed.py can check its arithmetic without a GPU.
#include "../../madqp_jl_amd/csrc/band_plan.inc"

// out[0] = leading dimension, out[1] = doubles of storage; returns 0 when ld_in is refused.  pad < 0: the library's default.
extern "C" int64_t band_packed_layout_c(int64_t n, int64_t extent, int64_t ld_in, int64_t pad, int64_t* out) {
    return band_packed_layout(n, extent, ld_in, out, pad < 0 ? BAND_PACKED_PAD : pad) ? 1 : 0;
}
extern "C" int64_t band_packed_default_pad_c() { return BAND_PACKED_PAD; }
