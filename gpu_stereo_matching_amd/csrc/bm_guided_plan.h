// bm_guided_plan.h — the guided pass's tile geometry, what its launcher accepts and the right view's workspace.
//
// Each number is stated once: bm_guided.hip ties GeoF and its launcher to these, and the C API sizes the handle's
// right-partial workspace by them.  Host-only and free of HIP, so a plain C++ compiler builds it
// (tests/test_guided_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sm {

// the kernel's radii and disparities (bm_guided.hip checks them against kMaxFastRadius and kMaxDisp, bm_box_plan.h)
constexpr int kMaxGuidedRadius = 7;
constexpr int kMaxGuidedDisp = 256;

// output tile: 64 lanes of P columns minus a 2r halo on either side, kGuidedTileH rows
constexpr int kGuidedTileH = 32;
constexpr int guided_tile_w(int r) { return 64 - 4 * r; }
// S2H: 8 segments per output row, each of this many outputs
constexpr int guided_seg_w(int r) { return (guided_tile_w(r) + 7) / 8; }
// right-key chain: a key leaves a row's last segment after at most this many steps
constexpr int guided_chain_span(int r) { return 8 * guided_seg_w(r); }
// steps of a tile's chain over D disparities = right pixels one tile row emits keys for
constexpr int guided_chain_len(int r, int D) { return D + guided_chain_span(r) - 1; }
// tiles the reduce folds per right pixel; its kernel is instantiated for 4, 6, 8 and 10
constexpr int guided_reduce_tiles(int r, int D) {
    return (guided_chain_len(r, D) + guided_tile_w(r) - 1) / guided_tile_w(r) + 1;
}
constexpr int kMaxGuidedReduceTiles = 10;
constexpr bool guided_reduce_fits(int r = 0) {
    return r > kMaxGuidedRadius ||
           (guided_reduce_tiles(r, kMaxGuidedDisp) <= kMaxGuidedReduceTiles && guided_reduce_fits(r + 1));
}
static_assert(guided_reduce_fits(), "the widest reduce folds every tile of a right pixel at D = 256 (r = 7: 10)");

// the fused right view's per-tile right-key partials, [frame][ty][tx][chain step][kGuidedTileH] int32, for a pass
// over D disparities (a slice: d_hi - d_lo); 0 for a radius the kernel does not have
inline size_t guided_right_partial_bytes(int W, int H, int radius, int D, int batch) {
    if (radius < 0 || radius > kMaxGuidedRadius) return 0;
    const int TW = guided_tile_w(radius);
    const int64_t tiles = (int64_t)((W + TW - 1) / TW) * ((H + kGuidedTileH - 1) / kGuidedTileH);
    return (size_t)(tiles * batch * guided_chain_len(radius, D) * kGuidedTileH * 4);
}

// what launch_guided takes: a radius the kernel has, disparities [d_lo, d_hi) of the 8-bit d field, a frame
inline bool guided_pass_ok(int W, int H, int radius, int d_lo, int d_hi, int batch) {
    return radius >= 0 && radius <= kMaxGuidedRadius && d_lo >= 0 && d_lo < d_hi && d_hi <= kMaxGuidedDisp && W > 0 &&
           H > 0 && batch > 0;
}

// ---- the cost volume (launch_guided_volume): every d's cost kept, [D][H][W] dense 32-bit planes ----
// A cost is trunc(q * 2^14) with q clamped to [-512, 512): a signed 24-bit value, the cost field of a slice key.  The
// biased form adds 2^23, so every cost is a uint32 below 2^24, the bound of the sub-pixel WTA (bm_subpix.hip); the
// threshold q < 50 of the 8-bit guided map becomes V < kGuidedInvalidFrom.  A pair that does not exist (d > W - x)
// holds INT32_MAX, or biased the largest cost: it never beats a pair that exists (d = 0 always does, and the WTA
// keeps the first minimum), and it keeps the WTA's arithmetic inside its bound where the right view walks over it.
constexpr int kGuidedCostShift = 14;
constexpr uint32_t kGuidedVolumeBias = 512u << kGuidedCostShift;            // 2^23
constexpr uint32_t kGuidedVolumeNone = 2u * kGuidedVolumeBias - 1u;          // 2^24 - 1
constexpr uint32_t kGuidedInvalidFrom = (50u + 512u) << kGuidedCostShift;   // q >= 50: no match
static_assert(kGuidedVolumeNone < (1u << 24) && kGuidedInvalidFrom < kGuidedVolumeNone, "V < 2^24 (bm_subpix.hip)");

inline size_t guided_volume_bytes(int W, int H, int D) { return (size_t)4 * (size_t)W * (size_t)H * (size_t)D; }

// what launch_guided_volume takes: one frame, d in [0, D)
inline bool guided_volume_ok(int W, int H, int radius, int D) { return guided_pass_ok(W, H, radius, 0, D, 1); }

}  // namespace sm
