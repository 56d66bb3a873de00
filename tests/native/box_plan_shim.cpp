// C entries to csrc/bm_box_plan.h (plan_box_pass, box_tile_kernel, box_mfma_scope), built with the host compiler alone, for tests/test_box_plan.py.
#include "../../gpu_stereo_matching_amd/csrc/bm_box_plan.h"

// box_tile_kernel: 0 plain, 1 8-wave tiles, 2 16-wave tiles, 3 the matrix-pipe kernel
extern "C" int box_tile_kernel(int radius, int dspan, long long tiles, int cus, int box_kernel, int in_matrix_scope) {
    return static_cast<int>(sm::box_tile_kernel(radius, dspan, tiles, cus, box_kernel, in_matrix_scope != 0));
}

extern "C" int box_mfma_scope(int radius, int d_lo, int d_hi, int valid_mode) {
    return sm::box_mfma_scope(sm::BoxGeom{64, 64, 64, radius, d_lo, d_hi, 1}, valid_mode);
}

// want: 0 none, 1 map, 2 keys.  out: left (0 tile, 1 strip, 2 wide, 3 direct), right (0 none, 1 fused, 2 mirrored,
// 3 unsupported), rpart_bytes, vol_bytes, mirror_planes
extern "C" void box_plan(int W, int H, int pitch, int radius, int d_lo, int d_hi, int batch, int want,
                         unsigned long long out[5]) {
    const sm::BoxPlan p = sm::plan_box_pass(sm::BoxGeom{W, H, pitch, radius, d_lo, d_hi, batch},
                                            static_cast<sm::RightWant>(want));
    out[0] = static_cast<unsigned long long>(p.left);
    out[1] = static_cast<unsigned long long>(p.right);
    out[2] = p.rpart_bytes;
    out[3] = p.vol_bytes;
    out[4] = static_cast<unsigned long long>(p.mirror_planes);
}
