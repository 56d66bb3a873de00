// bm_speckle_plan.h — the speckle filter's tile geometry, launch sizes, workspace and what its launcher accepts.
//
// Each number is stated once: bm_speckle.hip ties its kernels and launcher to these, and the C API sizes the
// handle's workspace by them.  Host-only and free of HIP, so a plain C++ compiler builds it
// (tests/test_speckle_ref.py through tests/native/speckle_plan_shim.cpp).
//
// Batches: the frames of a batch run in groups of up to kSpeckleGroup frames, one launch of each pass per group
// (the frame is the grid's z index), through one workspace of u32 labels + u32 counts, 8 B per pixel of a frame
// in the group.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sm {

// one workgroup labels one tile in LDS: kSpeckleThreads threads, kSpeckleTileW * kSpeckleTileH / kSpeckleThreads
// pixels each
constexpr int kSpeckleTileW = 32;
constexpr int kSpeckleTileH = 32;
constexpr int kSpeckleTilePixels = kSpeckleTileW * kSpeckleTileH;
constexpr int kSpeckleThreads = 256;
static_assert(kSpeckleTilePixels % kSpeckleThreads == 0, "every thread labels the same number of pixels");
// frames per launch group
constexpr int kSpeckleGroup = 8;
// labels are pixel indices of one frame in 32 bits, 0xFFFFFFFF marks an invalid pixel
constexpr int64_t kSpeckleMaxPixels = ((int64_t)1 << 31) - 1;

struct SpecklePlan {
    int tiles_x, tiles_y;     // the tile pass's grid (x, y); z is the frame of the group
    int64_t seam_pairs;       // neighbour pairs across a tile edge, per frame: one seam-pass thread each
    int seam_blocks;          // seam-pass workgroups of kSpeckleThreads per frame (0: one tile, no seam pass)
    int pixel_blocks;         // count / apply pass workgroups of kSpeckleThreads per frame
    int group;                // frames per launch group
    size_t plane_bytes;       // one of the two workspace planes (labels, counts): 4 B * P * group, 256-B aligned
    size_t bytes;             // the workspace: both planes
};

// what launch_speckle takes: a frame whose pixel indices fit the labels, at least one frame
inline bool speckle_pass_ok(int W, int H, int batch) {
    return W > 0 && H > 0 && batch > 0 && (int64_t)W * H <= kSpeckleMaxPixels;
}

inline SpecklePlan plan_speckle(int W, int H, int batch) {
    SpecklePlan p{};
    if (!speckle_pass_ok(W, H, batch)) return p;
    const int64_t P = (int64_t)W * H;
    p.tiles_x = (W + kSpeckleTileW - 1) / kSpeckleTileW;
    p.tiles_y = (H + kSpeckleTileH - 1) / kSpeckleTileH;
    p.seam_pairs = (int64_t)(p.tiles_x - 1) * H + (int64_t)(p.tiles_y - 1) * W;
    p.seam_blocks = (int)((p.seam_pairs + kSpeckleThreads - 1) / kSpeckleThreads);
    p.pixel_blocks = (int)((P + kSpeckleThreads - 1) / kSpeckleThreads);
    p.group = batch < kSpeckleGroup ? batch : kSpeckleGroup;
    p.plane_bytes = ((size_t)(4 * P * p.group) + 255) & ~(size_t)255;
    p.bytes = 2 * p.plane_bytes;
    return p;
}

}  // namespace sm
