// bm_box_plan.h — which kernels a box-aggregation pass runs and what workspace they take.
//
// One pure function of the pass, plan_box_pass: the C API's runner (run_box_pass, sm_capi.hip) launches what it
// says, the d-slice calls pre-size and reject by it, and the kernels' launchers validate their arguments with
// the same predicates.  Host-only and free of HIP, so a plain C++ compiler builds it (tests/test_box_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace sm {

constexpr int kMaxDisp = 256;      // uint8 output / 8-bit d field of the packed key
constexpr int kMaxFastRadius = 7;  // u16 packed sums stay < 2^16 up to r = 7 (15*15*255 = 57375)
// fused tile kernel (bm_box.hip): u16 packed column prefixes stay < 2^16 up to r = 15 ((32 + 30) * 255 = 15810);
// r 8..15 sum the window's two halves in u32
constexpr int kMaxBoxRadius = 15;
// strip kernel (bm_strip.hip): disparities across the lanes, vertical sums in registers, no workspace.  Past
// r = 37 its 128 - 2r outputs per 128 summed columns make it slower than the separable path (1080p D=128, us per
// frame: r = 37 223.4 vs 236.3, r = 40 256.6 vs 236.6); one lane per disparity of the 8-bit d field
constexpr int kStripMinRadius = 16;
constexpr int kStripMaxRadius = 37;
constexpr int kStripMaxDisp = 256;
// separable wide-window path (bm_wide.hip): one row block of up to 4096 outputs, frames below 2^31 bytes (its
// buffer loads address a frame with 32-bit offsets)
constexpr int kMaxWideWidth = 4096;

struct BoxGeom {
    int W, H, pitch, radius;
    int d_lo, d_hi;   // the disparities of the pass: [d_lo, d_hi)
    int batch;
};
enum class RightWant {
    None,
    Map,    // dR planes (run_device_body)
    Keys,   // the right view's slice keys (d-slices)
};
enum class BoxLeft { Tile, Strip, Wide, Direct };
enum class BoxRight {
    None,
    Fused,        // from the left pass's own costs
    Mirrored,     // a second pass (valid d <= x, no threshold) over the mirrored pair, on Strip or Direct as the left
    Unsupported,  // slice keys outside the wide path: the callers reject the call
};
struct BoxPlan {
    BoxLeft left;
    BoxRight right;
    size_t rpart_bytes;   // of the handle's right-partial workspace
    size_t vol_bytes;     // of its volume workspace
    int mirror_planes;    // dense W x H x batch planes for the mirrored pair
};

inline bool strip_path(const BoxGeom& g) {
    return g.radius >= kStripMinRadius && g.radius <= kStripMaxRadius && g.W >= 4 && g.H >= 1 && g.d_lo < g.d_hi &&
           g.d_hi <= kStripMaxDisp;
}
inline bool wide_frame(int W, int H, int pitch) {
    return W >= 4 && W <= kMaxWideWidth && (int64_t)pitch * H < ((int64_t)1 << 31);
}
inline bool wide_path(const BoxGeom& g) { return g.radius > kMaxBoxRadius && wide_frame(g.W, g.H, g.pitch); }

// Tile kernel geometry (bm_box.hip ties Geo and its constants to these): kBoxTileH-row tiles of kBoxCols - 2r output
// columns, the disparity span rounded up to kBoxChunk and compiled for 64 / 128 / 192 / 256
constexpr int kBoxTileH = 32, kBoxCols = 64, kBoxChunk = 8;
constexpr int box_tile_width(int r) { return kBoxCols - 2 * r; }
constexpr int box_dmax(int D) {
    const int dspan = (D + kBoxChunk - 1) & ~(kBoxChunk - 1);
    return dspan <= 64 ? 64 : (dspan <= 128 ? 128 : (dspan <= 192 ? 192 : 256));
}
// u32 entries per right-key partial row: TW + dmax + 1 keys behind 1..4 pad slots, 16-B aligned groups of 4
constexpr int box_partial_pitch(int r, int dmax) { return (box_tile_width(r) + dmax + 1 + 7 + 3) & ~3; }
// the fused right view's per-tile right-key partials, [frame][ty][tx][kBoxTileH][pitch] (radius <= kMaxBoxRadius)
inline size_t box_right_partial_bytes(int W, int H, int radius, int D, int batch) {
    if (radius < 0 || radius > kMaxBoxRadius) return 0;
    const int TW = box_tile_width(radius);
    const size_t tiles = (size_t)((W + TW - 1) / TW) * ((H + kBoxTileH - 1) / kBoxTileH);
    return tiles * (size_t)batch * kBoxTileH * box_partial_pitch(radius, box_dmax(D)) * 4;
}

// Which kernel a left-only tile pass launches (launch_rd, bm_box.hip).
// the matrix-pipe kernel's scope (bm_box_mfma.hip): the left view alone, radius 1..kMaxFastRadius, valid_mode 0
inline bool box_mfma_scope(const BoxGeom& g, int valid_mode) {
    return g.radius >= 1 && g.radius <= kMaxFastRadius && valid_mode == 0 && g.d_lo >= 0 && g.d_hi > g.d_lo &&
           g.d_hi <= kMaxDisp;
}
enum class BoxTileKernel {
    Plain,    // 4 waves per tile
    Mid8,     // 8 waves
    Wide16,   // kWideTile waves
    Matrix,   // bm_box_mfma.hip
};
// Wide16: no more tiles than CUs (a small frame, batch 1): 16 waves per tile, >= 2 d-pairs each, so every CU runs
// 16 waves instead of <= 4 (r <= 7: the wide-radius kernels need > 128 VGPRs).  Beyond one tile per CU the 4-wave
// kernel wins: with one 16-wave workgroup per CU a tile's staging overlaps no other tile's compute (1080p batch 1:
// 102.8 vs 87.8 us).
constexpr int kWideTile = 16;
// Mid8: launches of more tiles than CUs but at most kMidTilesPerCu tiles per CU (batch 1 of a mid-size frame) take
// 8-wave tiles, the d pairs split over twice the waves: the last round of tiles ends sooner.  Same box, device
// resident, batch 1 (profiles/microbench/r04_box_mid_tiles_latency.txt): 960x540 D=128 47.5 -> 39.7 us, 320x240 D=32
// 16.7 -> 13.6, 1080p D=128 88.5 -> 86.3; maps identical.
constexpr int kMidTile = 8, kMidTilesPerCu = 8;
// Matrix: launches past the 8-wave tiles' range (a batch of frames: the throughput path): 1080p D = 128 r = 5, 128
// frames per launch, 6.91 -> 6.04 ms; D = 256 x 32 frames 3.51 -> 2.94; 4K D = 192 x 8 frames 2.51 -> 2.10; batch 1
// stays on the 8-wave tiles (0.070 against 0.071 ms) (profiles/microbench/box_mfma_headline_ab.txt)
// dspan: d_hi - d_lo; tiles: tiles_x * tiles_y * batch; box_kernel (SM_PARAM_BOX_KERNEL): 0 auto, 1 the kernels of
// bm_box.hip, 2 the matrix-pipe kernel at any launch size; outside that kernel's scope 2 is 0
constexpr BoxTileKernel box_tile_kernel(int radius, int dspan, int64_t tiles, int cus, int box_kernel,
                                        bool in_matrix_scope) {
    const int npairs = ((dspan + kBoxChunk - 1) & ~(kBoxChunk - 1)) / 2;
    const int64_t mid_tiles = (int64_t)kMidTilesPerCu * cus;
    if (in_matrix_scope && box_kernel == 2) return BoxTileKernel::Matrix;
    if (radius <= kMaxFastRadius) {
        if (tiles <= cus && npairs >= 2 * kWideTile) return BoxTileKernel::Wide16;
        if (tiles <= mid_tiles && npairs >= 2 * kMidTile) return BoxTileKernel::Mid8;
    }
    if (in_matrix_scope && box_kernel == 0 && tiles > mid_tiles) return BoxTileKernel::Matrix;
    return BoxTileKernel::Plain;
}

// Wide path: frames per vsum / hwta launch pair: enough row blocks for ~32 per CU (1080 rows of one 1080p frame
// give 4), at most 8 frames and 4.5 GB of V planes (1080p D=128: 8 frames, 4.2 GB).  Same box, 1080p D=128, 8
// frames per call (profiles/microbench/r05_wide_path.txt): 2 / 4 / 8 frames per pair 0.280 / 0.268 / 0.265 ms at
// r = 16, 0.280 / 0.251 / 0.239 at r = 127
inline int wide_group(int W, int H, int D, int batch) {
    const int64_t plane = (int64_t)W * H * D * (int64_t)sizeof(uint16_t);
    const int by_mem = (int)std::max<int64_t>(1, ((int64_t)4608 << 20) / std::max<int64_t>(plane, 1));
    const int want = (8192 + H - 1) / H;
    return std::max(1, std::min({want, batch, 8, by_mem}));
}
// its V planes: u16, D * W * H per frame of a launch group
inline size_t wide_workspace_bytes(int W, int H, int D, int batch) {
    return (size_t)wide_group(W, H, D, batch) * D * W * H * sizeof(uint16_t);
}

inline BoxPlan plan_box_pass(const BoxGeom& g, RightWant want) {
    BoxPlan p{BoxLeft::Tile, BoxRight::None, 0, 0, 0};
    const int D = g.d_hi - g.d_lo;
    if (g.radius <= kMaxBoxRadius) {   // the right view fused with the left pass over per-tile partials
        if (want != RightWant::None) {
            p.right = BoxRight::Fused;
            p.rpart_bytes = box_right_partial_bytes(g.W, g.H, g.radius, D, g.batch);
        }
        return p;
    }
    const bool strip = strip_path(g), wide = wide_path(g);
    // r 16..37: the strip kernel, at any width without the right view; with it the right keys go through the
    // volume workspace (4 B per pixel, filled with 0xFF by the runner) and their low byte is dR
    if (strip && (want == RightWant::None || (want == RightWant::Map && wide))) {
        p.left = BoxLeft::Strip;
        if (want == RightWant::Map) {
            p.right = BoxRight::Fused;
            p.vol_bytes = (size_t)4 * g.W * g.H * g.batch;
        }
        return p;
    }
    if (wide) {   // the right view (map, or sign-flipped slice keys) from the wide kernel's LDS atomic-min row
        p.left = BoxLeft::Wide;
        p.right = want == RightWant::None ? BoxRight::None : BoxRight::Fused;
        p.vol_bytes = wide_workspace_bytes(g.W, g.H, D, g.batch);
        return p;
    }
    // frames the wide path rejects (W < 4, W > 4096, planes of 2^31 bytes and up)
    p.left = strip ? BoxLeft::Strip : BoxLeft::Direct;
    if (want == RightWant::Map) {
        p.right = BoxRight::Mirrored;
        p.mirror_planes = 2;
    } else if (want == RightWant::Keys) {
        p.right = BoxRight::Unsupported;
    }
    return p;
}

}  // namespace sm
