// bm_guided.h — guided-filter cost aggregation (absent from the reference).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm_guided_plan.h"

namespace sm {

// One guided-filter aggregation + WTA pass over d in [d_lo, d_hi) of `batch` frames: one launch, every intermediate
// in LDS.  What it writes says what it is.
struct GuidedPass {
    const uint8_t* left;    // [batch][H][pitch]
    const uint8_t* right;
    int W, H, pitch;
    int64_t frame_stride;   // bytes between frames (inputs)
    int batch;
    int radius;             // 0..kMaxGuidedRadius
    int d_lo, d_hi;         // d_hi <= kMaxGuidedDisp
    float eps;
    // Left view, exactly one of:
    // the map [batch][H][out_pitch] (d_lo must be 0): first d with the smallest q below 50, valid d <= W - x
    uint8_t* disp;
    int out_pitch;
    int64_t out_frame_stride;
    // the slice's keys [batch][H][W] (multi-GPU sharding over d): ((int)(q * 2^14) << 8) | d for the
    // best valid d of the slice, no threshold, INT_MAX if none is valid.  Keys of disjoint slices combine with a
    // signed min
    int* keys;
    // Right view, optional, fused into the same pass: STMatching's rule C_R(y, u, d) = C_L(y, u + d, d), strict <
    // from d = 0, no threshold (StereoHelper.cpp:131-180).  gpart: the per-tile right-key partials,
    // guided_right_partial_bytes(W, H, radius, d_hi - d_lo, batch) bytes; nullptr: left view only
    int* gpart;
    // with disp: the right map [batch][H][rpitch], frame stride rstride
    uint8_t* right_map;
    int rpitch;
    int64_t rstride;
    // with keys: the right view's slice keys [batch][H][W], (cost field of q_R, 2^-14 fixed point) | d for the best d
    // of the slice with u + d < W, INT_MAX where none; combined with a signed min
    int* right_keys;
};
// hipErrorInvalidValue unless guided_pass_ok (bm_guided_plan.h) holds, exactly one of disp / keys is given, the map
// starts at d_lo = 0, and the right view is all or nothing: gpart with right_map beside disp or right_keys beside keys
hipError_t launch_guided(const GuidedPass& p, hipStream_t s);

// The guided cost volume of one frame in one pass: the guide statistics once per tile, every d's cost stored
// (bm_guided_plan.h: the planes' values).
struct GuidedVolumePass {
    const uint8_t* left;    // [H][pitch]
    const uint8_t* right;
    int W, H, pitch;
    int radius;             // 0..kMaxGuidedRadius
    int num_disp;           // 1..kMaxGuidedDisp
    float eps;
    // [num_disp][H][W] dense: int32 trunc(q * 2^14), INT32_MAX where d > W - x; biased: uint32, that cost +
    // kGuidedVolumeBias, kGuidedVolumeNone where d > W - x
    void* vol;
    bool biased;
};
// hipErrorInvalidValue unless guided_volume_ok holds, the pointers are set and pitch >= W
hipError_t launch_guided_volume(const GuidedVolumePass& p, hipStream_t s);

// combined keys -> disparity with the Device.cu:37 threshold q < 50
hipError_t launch_guided_keys_to_disp(const int* keys, int W, int H, uint8_t* disp, int out_pitch, hipStream_t s);

}  // namespace sm
