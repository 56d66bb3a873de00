// C entries to csrc/bm_speckle_plan.h, built with the host compiler alone, for tests/test_speckle_ref.py.
#include "../../gpu_stereo_matching_amd/csrc/bm_speckle_plan.h"

// out: tile width, tile height, threads per workgroup, frames per launch group
extern "C" void speckle_constants(int out[4]) {
    out[0] = sm::kSpeckleTileW;
    out[1] = sm::kSpeckleTileH;
    out[2] = sm::kSpeckleThreads;
    out[3] = sm::kSpeckleGroup;
}
// out: tiles_x, tiles_y, seam pairs, seam blocks, pixel blocks, group, plane bytes, bytes
extern "C" void speckle_plan(int W, int H, int batch, long long out[8]) {
    const sm::SpecklePlan p = sm::plan_speckle(W, H, batch);
    out[0] = p.tiles_x;
    out[1] = p.tiles_y;
    out[2] = p.seam_pairs;
    out[3] = p.seam_blocks;
    out[4] = p.pixel_blocks;
    out[5] = p.group;
    out[6] = (long long)p.plane_bytes;
    out[7] = (long long)p.bytes;
}
extern "C" int speckle_ok(int W, int H, int batch) { return sm::speckle_pass_ok(W, H, batch) ? 1 : 0; }
