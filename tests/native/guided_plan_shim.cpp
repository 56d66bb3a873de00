// C entries to csrc/bm_guided_plan.h, built with the host compiler alone, for tests/test_guided_plan.py.
#include "../../gpu_stereo_matching_amd/csrc/bm_guided_plan.h"

// out: tile width, tile height, S2H segment width, chain span, chain length at D, the reduce's tiles at D
extern "C" void guided_geometry(int radius, int D, int out[6]) {
    out[0] = sm::guided_tile_w(radius);
    out[1] = sm::kGuidedTileH;
    out[2] = sm::guided_seg_w(radius);
    out[3] = sm::guided_chain_span(radius);
    out[4] = sm::guided_chain_len(radius, D);
    out[5] = sm::guided_reduce_tiles(radius, D);
}
extern "C" unsigned long long guided_partial_bytes(int W, int H, int radius, int D, int batch) {
    return sm::guided_right_partial_bytes(W, H, radius, D, batch);
}
extern "C" int guided_ok(int W, int H, int radius, int d_lo, int d_hi, int batch) {
    return sm::guided_pass_ok(W, H, radius, d_lo, d_hi, batch) ? 1 : 0;
}
