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

// ---- the matrix-pipe kernel's tiles and how its workgroups come by them (bm_box_mfma.hip ties MG to these) ----
// disparities per loop pass: one for spans of at most 32 at r <= 2, else two (launch_rd there)
constexpr int box_mfma_np(int radius, int dspan) { return dspan <= 32 && radius <= 2 ? 1 : 2; }
// output columns and rows of a tile
constexpr int box_mfma_tox(int radius, int np) { return np == 1 || radius <= 6 ? 64 - 2 * radius : 48; }
constexpr int box_mfma_toy(int radius, int np) { return np == 2 ? 48 : 64 - 2 * radius; }
constexpr int64_t box_mfma_tiles(int W, int H, int radius, int dspan, int batch) {
    const int np = box_mfma_np(radius, dspan), tox = box_mfma_tox(radius, np), toy = box_mfma_toy(radius, np);
    return (int64_t)((W + tox - 1) / tox) * ((H + toy - 1) / toy) * batch;
}

#if defined(__HIPCC__)
#define SM_PLAN_HD __host__ __device__
#else
#define SM_PLAN_HD
#endif

// Self-scheduled launches: the workgroups of a launch draw runs of tiles from one counter, grab g
// being the g-th value the counter hands out.  box_queue_grab maps g to its half-open range of the sequence
// [frame][ty][tx]; a workgroup walks the range like a static one (a fresh band at its first tile and at every row
// start, carried bands between).  The schedule is a sequence of levels of equal grabs whose size halves from level
// to level: s0 = kQueueRows rows of tiles, then s0 / 2, s0 / 4, .. 1.  The level of size s hands out whole grabs
// while more than kQueueTail * slots of them remain, so about that many grabs of size s per slot, which is twice as
// many of the next size, are left when the size halves; the last level hands out every remaining tile singly.  So
// sizes never increase, every tile has one owner, the launch ends with single tiles (the slots end within about a
// tile of each other), and a launch with few tiles per slot starts at the level that fits it.  At most 16 levels
// (s0 <= 32768), one 32-bit division each; a grab past the last is empty.
constexpr uint32_t kQueueRows = 1;
constexpr uint32_t kQueueTail = 1;
struct BoxGrab {
    uint32_t begin, end;
};
SM_PLAN_HD inline BoxGrab box_queue_grab(uint32_t g, uint32_t total, uint32_t tiles_x, uint32_t slots) {
    uint32_t s = tiles_x * kQueueRows;
    if (s > 32768u) s = 32768u;
    uint32_t t = 0;   // the first tile of the level
    for (; s > 1; s >>= 1) {
        const uint32_t q = (total - t) / s, keep = slots * kQueueTail;
        if (q <= keep) continue;
        const uint32_t n = q - keep;
        if (g < n) return BoxGrab{t + g * s, t + g * s + s};
        g -= n;
        t += n * s;
    }
    return g < total - t ? BoxGrab{t + g, t + g + 1} : BoxGrab{total, total};
}
// the grabs that are not empty (the counter ends at this plus one empty grab per workgroup)
inline uint32_t box_queue_grabs(uint32_t total, uint32_t tiles_x, uint32_t slots) {
    uint32_t s = tiles_x * kQueueRows, t = 0, grabs = 0;
    if (s > 32768u) s = 32768u;
    for (; s > 1; s >>= 1) {
        const uint32_t q = (total - t) / s, keep = slots * kQueueTail;
        if (q <= keep) continue;
        grabs += q - keep;
        t += (q - keep) * s;
    }
    return grabs + (total - t);
}

// Whether a matrix-pipe launch of `tiles` tiles over dspan disparities draws them from the queue, and with how many
// workgroups (0: it keeps static ranges).  workgroups: SM_PARAM_BOX_WORKGROUPS, queue_workgroups:
// SM_PARAM_BOX_QUEUE_WORKGROUPS, slots: the workgroups the device holds at once.  An explicit range count keeps the
// static ranges, one d per pass keeps its one-tile kernel, an explicit queue size is taken as it is (a test frame of a
// dozen tiles), and auto takes one workgroup per slot where a slot has enough tiles to draw, by what was measured
// against the static ranges, ms per launch (profiles/microbench/box_mfma_queue_ab.txt):
//   138 tiles per slot   1080p D = 128 r = 5 x 128 frames 4.71 -> 4.47: the queue
//   30..38 per slot      1080p x 32 frames at r = 5, D = 8 / 16 / 32 / 64: 0.253 -> 0.233, 0.311 -> 0.286, 0.436 ->
//                        0.402, 0.689 -> 0.651: the queue, for spans up to kQueueShortSpan, whose tiles are mostly
//                        staging, which a carried band saves.  Longer spans are mixed at this size (D = 128 r = 1 / 5 /
//                        7 and D = 256 gain 1.2 / 3.1 / 2.2 / 1.7 %, D = 128 r = 3 and 4K D = 192 x 8 frames lose 0.7 /
//                        1.6 %, and the tile count does not tell them apart): static ranges
//   4..9 per slot        headline x 4 frames, 463 x 370 D = 64 x 96: 0.166 -> 0.189, 0.185 -> 0.190, 0.187 -> 0.200:
//                        static ranges (a run is one or two tiles however they are handed out)
constexpr int kQueueMinTilesPerSlot = 64, kQueueMinTilesPerSlotShort = 28, kQueueShortSpan = 64;
constexpr int kMaxQueueWorkgroups = 1 << 20;
constexpr int box_queue_workgroups(int np, int dspan, int64_t tiles, int slots, int workgroups,
                                   int queue_workgroups) {
    if (np != 2 || workgroups != 0 || slots < 1 || queue_workgroups < 0 || queue_workgroups > kMaxQueueWorkgroups)
        return 0;
    if (queue_workgroups > 0) return queue_workgroups;
    const int per_slot = dspan <= kQueueShortSpan ? kQueueMinTilesPerSlotShort : kQueueMinTilesPerSlot;
    return tiles >= (int64_t)per_slot * slots ? slots : 0;
}

// Whether the runner takes the handle's grab counter for a left-only tile pass: the pass launches the matrix-pipe
// kernel (box_tile_kernel on the VALU kernels' tile count, as launch_rd in bm_box.hip asks it) and
// box_queue_workgroups says it draws from the queue, with the slots the kernel has on every device so far:
// kBoxMfmaWorkgroupsPerCu per CU (its launch bounds; 24 to 48 KB of LDS each).  A pass that keeps static ranges
// takes no workspace, so it joins no ordering and records no event.  The launcher asks again with the slots the
// occupancy query gives it
constexpr int kBoxMfmaWorkgroupsPerCu = 3;
inline bool box_queue_candidate(const BoxGeom& g, int valid_mode, int cus, int box_kernel, int workgroups,
                                int queue_workgroups) {
    if (g.radius < 0 || g.radius > kMaxFastRadius || cus < 1) return false;
    const int TW = box_tile_width(g.radius), dspan = g.d_hi - g.d_lo;
    const int64_t tiles = (int64_t)((g.W + TW - 1) / TW) * ((g.H + kBoxTileH - 1) / kBoxTileH) * g.batch;
    if (box_tile_kernel(g.radius, dspan, tiles, cus, box_kernel, box_mfma_scope(g, valid_mode)) != BoxTileKernel::Matrix)
        return false;
    return box_queue_workgroups(box_mfma_np(g.radius, dspan), dspan, box_mfma_tiles(g.W, g.H, g.radius, dspan, g.batch),
                                kBoxMfmaWorkgroupsPerCu * cus, workgroups, queue_workgroups) > 0;
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
