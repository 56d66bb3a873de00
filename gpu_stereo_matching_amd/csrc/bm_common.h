// bm_common.h — shared definitions for the gfx950 block-matching kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "bm_box_plan.h"   // kMaxDisp, kMaxFastRadius and the box pass's predicates

namespace sm {

// Launch parameters of one block-matching pass over a batch of frames.
struct MatchArgs {
    const uint8_t* left;    // [batch][H][pitch]
    const uint8_t* right;
    int W, H, pitch;
    int64_t frame_stride;   // bytes between frames (inputs)
    int radius;             // window = (2r+1)^2 (SADWindowSize, Device.cu:181)
    int d_lo, d_hi;         // disparities handled by this launch: [d_lo, d_hi)
    int valid_mode;         // 0: d <= W - x (Device.cu:44);  1: d <= x (right view, mirrored)
    uint32_t seed_key;      // starting best key: (50*win^2) << 8 (Device.cu:37) or ~0u (no threshold)
    uint32_t thresh_key;    // disparity = key < thresh_key ? key & 0xFF : 0   (Device.cu:38,63)
    uint8_t* disp;          // optional: uint8 disparity [batch][H][out_pitch]
    int out_pitch;
    int64_t out_frame_stride;
    uint32_t* keys;         // optional: packed keys [batch][H][W] (multi-GPU slice reduction)
    uint32_t* rpart;        // fused right view: per-tile right-key partials (box_right_partial_bytes, bm_box_plan.h)
};
// the pass as the plan headers take it
inline BoxGeom box_geom(const MatchArgs& a, int batch) {
    return BoxGeom{a.W, a.H, a.pitch, a.radius, a.d_lo, a.d_hi, batch};
}

// Which pairs (x, k) of a d-major cost volume exist, plane k standing for the disparity d = d0 + k, k = 0 .. D - 1.
// At every column they are a prefix of the planes, k <= min(D - 1, ka + kb * x):
//   the reference's rule (Device.cu:44)   x + d <= W,  d0 = 0:   (ka, kb) = (W, -1)
//   SM_PAIRS_IN_VIEW                      x - d >= 0:            (ka, kb) = (-d0, +1), negative where x < d0
// The kernels take (ka, kb) as arguments, so both rules run the same code.
struct Pairs {
    int in_view = 0;   // SM_PAIRS_IN_VIEW
    int d0 = 0;        // SM_PARAM_MIN_DISP; 0 unless in_view
    int ka(int W) const { return in_view ? -d0 : W; }
    int kb() const { return in_view ? 1 : -1; }
    // what a launcher takes: the largest disparity d0 + D - 1 fits the map (255 or 4095)
    bool ok(int D, int d_limit) const { return d0 >= 0 && (in_view ? d0 + D - 1 <= d_limit : d0 == 0); }
};

// The CU count of the current device, asked once per device index: the handles of a group on several devices size
// each launch by their own device (256 when the query fails).
inline int device_cus() {
    constexpr int kMaxDevices = 64;
    static std::atomic<int> count[kMaxDevices];   // 0: not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const bool cached = dev >= 0 && dev < kMaxDevices;
    int cus = cached ? count[dev].load(std::memory_order_relaxed) : 0;
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        if (cached) count[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// Workgroups of `kernel` (at `threads` threads and `lds_bytes` of dynamic LDS each) that the current device holds at
// once: the occupancy query's answer (at least 1) times device_cus(), asked once per distinct kernel, launch shape
// and device.  Any thread may call it (group members launch from their own).  A failed query is returned and not
// remembered: the caller decides what to launch without it.
inline hipError_t resident_workgroups(const void* kernel, int threads, size_t lds_bytes, int* out) {
    static std::mutex lock;
    static std::map<std::tuple<const void*, int, size_t, int>, int> known;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const auto key = std::make_tuple(kernel, threads, lds_bytes, dev);
    const std::lock_guard<std::mutex> hold(lock);
    auto it = known.find(key);
    if (it == known.end()) {
        int per_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes);
        if (e != hipSuccess) return e;
        it = known.emplace(key, (per_cu > 0 ? per_cu : 1) * device_cus()).first;
    }
    *out = it->second;
    return hipSuccess;
}

// f(std::integral_constant<int, R>{}) for the R in [LO, HI] that equals r (the radius as a kernel's template
// argument), else `fallback`
template <int LO, int HI, class T, class F>
T with_radius(int r, T fallback, F&& f) {
    if constexpr (LO > HI) {
        return fallback;
    } else {
        if (r == LO) return f(std::integral_constant<int, LO>{});
        return with_radius<LO + 1, HI>(r, fallback, f);
    }
}

constexpr int kNumXcd = 8;         // MI355X: 8 XCDs, each with its own L2

// Workgroups are dispatched round-robin over the XCDs (blockIdx % 8).  Remapping so that XCD k
// works through a contiguous run of tile indices keeps neighbouring tiles, whose right bands
// overlap by (D + 64 - TW) / (D + 64), in one L2.
__device__ __forceinline__ int xcd_tile(int b, int nb) {
    const int per = nb / kNumXcd, rem = nb - per * kNumXcd;
    const int x = b % kNumXcd, i = b / kNumXcd;
    return x < rem ? x * (per + 1) + i : rem * (per + 1) + (x - rem) * per + i;
}
// 4 image bytes of row y from column x (little-endian), bytes outside the image read as 0.
// Interior dwords are one (possibly unaligned) global_load_dword; border dwords go byte-wise.
__device__ __forceinline__ uint32_t ld_image_u32(const uint8_t* p, int y, int x, int W, int H, int pitch) {
    if (y < 0 || y >= H) return 0u;
    const uint8_t* row = p + (int64_t)y * pitch;
    if (x >= 0 && x + 3 < W) {
        uint32_t v;
        __builtin_memcpy(&v, row + x, 4);
        return v;
    }
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (x + b >= 0 && x + b < W) v |= (uint32_t)row[x + b] << (8 * b);
    return v;
}

// Host-side launchers (bm_box.hip, bm_aux.hip).  Which box launcher a pass takes, and the workspace sizes named
// below, are bm_box_plan.h's (plan_box_pass); a launcher checks only its own arguments.
// The fused tile kernels, radius <= kMaxBoxRadius (hipErrorInvalidValue beyond).
// box_kernel (SM_PARAM_BOX_KERNEL): 0 auto, 1 the VALU kernels of bm_box.hip, 2 the matrix-pipe kernel
// (bm_box_mfma.hip) wherever box_mfma_scope holds
// box_workgroups (SM_PARAM_BOX_WORKGROUPS): workgroups of a matrix-pipe launch, each walking a contiguous range of
// tiles: 0 auto, n >= 1 that many (at most one per tile)
// box_queue: null, or the u32 counter from which an auto matrix-pipe launch draws its tiles where
// box_queue_workgroups (bm_box_plan.h) says so; the launcher zeroes it on s.  box_queue_wgs
// (SM_PARAM_BOX_QUEUE_WORKGROUPS): 0 one queue workgroup per resident slot, n >= 1 that many at any launch size
hipError_t launch_box_match(const MatchArgs& a, int batch, hipStream_t s, int box_kernel = 0, int box_workgroups = 0,
                            uint32_t* box_queue = nullptr, int box_queue_wgs = 0);
// the plain box pass with both window sums on the matrix pipe: radius 1..kMaxFastRadius, valid_mode 0, no right
// view; bit-exact with launch_box_match.  hipErrorInvalidValue outside box_mfma_scope (bm_box_plan.h)
hipError_t launch_box_match_mfma(const MatchArgs& a, int batch, hipStream_t s, int workgroups = 0,
                                 uint32_t* queue = nullptr, int queue_workgroups = 0);
// any radius: the direct window sum per (pixel, d), straight from the reference formulation; not a performance path
hipError_t launch_box_match_generic(const MatchArgs& a, int batch, hipStream_t s);
// Box matching + right view (+ LR check) in two launches (radius <= kMaxBoxRadius, d_lo == 0).
// check = 1: a.disp receives the checked left disparity, right_out/mask_out (optional) dR and the
// valid mask.  check = 0: a.disp the unchecked left map and right_out (required) dR.
hipError_t launch_box_match_lr(const MatchArgs& a, int batch, int check, uint8_t* right_out, uint8_t* mask_out,
                               int aux_pitch, int64_t aux_stride, hipStream_t s);
// d-slice with LR (multi-GPU): one fused pass over d in [a.d_lo, a.d_hi) (radius <= kMaxBoxRadius)
// writing the left slice keys to a.keys (as launch_box_match) and the right view's slice keys
// min over d in the slice with u + d < W of (C_L(u + d, d) << 8 | d) to right_keys [batch][H][W]
// (0x7FFFFFFF where none; every key < 2^31 at these radii): keys of disjoint slices combine with a MIN.  a.rpart:
// the plan's rpart_bytes (bm_box_plan.h).
hipError_t launch_box_slice_lr_keys(const MatchArgs& a, int batch, uint32_t* right_keys, hipStream_t s);
// acc = min(acc, src) elementwise over n unsigned keys
hipError_t launch_min_keys_u32(uint32_t* acc, const uint32_t* src, int64_t n, hipStream_t s);
// right-view key map -> dR: the d field (low byte) of each key, no threshold (StereoHelper.cpp:131-154).
// in_view (SM_PAIRS_IN_VIEW): the low byte is the plane k, dR = d0 + k, and the key ~0 of a pixel no pair reached
// gives 0, never its low byte
hipError_t launch_keys_low_byte(const uint32_t* keys, int64_t n, uint8_t* out, hipStream_t s, int in_view = 0,
                                int d0 = 0);
hipError_t launch_keys_to_disp(const uint32_t* keys, int W, int H, uint32_t thresh_key,
                               uint8_t* disp, int out_pitch, hipStream_t s);
// acc = min(acc, src) elementwise over n signed keys (the d-slice MIN, rehearsed on one device)
hipError_t launch_min_keys(int* acc, const int* src, int64_t n, hipStream_t s);
hipError_t launch_mirror(const uint8_t* src, int W, int H, int pitch, int64_t stride, int batch,
                         uint8_t* dst, int dst_pitch, int64_t dst_stride, hipStream_t s);
// right_mirrored: 1 if the right map is stored mirrored (index W-1-u holds dR(u)), 0 if plain
hipError_t launch_lr_check(const uint8_t* left_disp, int lpitch, int64_t lstride,
                           const uint8_t* right_disp, int rpitch, int64_t rstride, int right_mirrored,
                           int W, int H, int batch, uint8_t* out, int opitch, int64_t ostride,
                           uint8_t* right_out, uint8_t* mask_out, int aux_pitch, int64_t aux_stride,
                           hipStream_t s);
// AD volume dif[d][y][x] (PreCal / kernalPreCal_V2), d-major planes per frame (bm_volume.hip).  d0
// (SM_PARAM_MIN_DISP, the matching calls alone): plane k holds |L(y, x) - R(y, x - d0 - k)|, 0 for x < d0 + k
hipError_t launch_ad_volume(const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int64_t fstride, int batch,
                            int D, uint8_t* dif, int64_t dstride, hipStream_t s, int d0 = 0);
// staged box path (bm_staged.hip): u16 SAD volume from the AD volume, and WTA over the SAD volume
// `ad` must have 8 readable bytes past its last plane (the handle's volume buffer carries that slack, sm_handle.h)
hipError_t launch_box_sad_volume(const uint8_t* ad, int W, int H, int radius, int D, uint16_t* sad, hipStream_t s);
// getAllSAD's pixel-major uchar volume out[p * D + d] (255 where x + d > W): from the u16 SAD volume
// (radius <= 7), or computed directly at any radius
hipError_t launch_all_sad_transpose(const uint16_t* sad, int W, int H, int D, uint8_t* out, hipStream_t s);
hipError_t launch_all_sad_generic(const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int radius, int D,
                                  uint8_t* out, hipStream_t s);
// (`frames` consecutive frames of D planes each; frame f's map at disp + f * out_stride)
hipError_t launch_volume_wta(const uint16_t* sad, int W, int H, int D, int frames, uint32_t seed_key, uint8_t* disp,
                             int out_pitch, int64_t out_stride, hipStream_t s);
// radius 16..127 (bm_wide.hip): V planes (u16, (d_hi - d_lo) * W * H per frame of a launch group, in `ws`,
// wide_workspace_bytes) then one block per image row; a.valid_mode 0, wide_frame(W, H, pitch).  right (optional): the
// right view's dR [batch][H][rpitch]
// rkeys (d-slices with LR): the right view's raw keys [batch][H][W] of the slice [a.d_lo, a.d_hi), sign bit flipped
// (kRightKeyFlip), instead of / beside `right`
hipError_t launch_box_match_wide(const MatchArgs& a, int batch, uint16_t* ws, uint8_t* right, int rpitch,
                                 int64_t rstride, hipStream_t s, uint32_t* rkeys = nullptr);
// Box right-view slice keys carry the sign bit flipped: (cost << 8 | d) ^ 2^31, so that a signed MIN orders them
// like the unsigned keys at every radius (a wide window's key reaches 255 * 255^2 << 8 > 2^31 from r = 91), and
// "no d of the slice reaches u" (0xFFFFFFFF before the flip) is INT32_MAX, as for the guided keys.
constexpr uint32_t kRightKeyFlip = 0x80000000u;
// radius 16..37 (bm_strip.hip; valid_mode 0 or 1, the mirrored right-view pass of frames the separable path
// rejects): disparities across the lanes, vertical sums in registers, no workspace
hipError_t launch_box_match_strip(const MatchArgs& a, int batch, hipStream_t s);
// the same with the right view (a.valid_mode 0, a.d_lo 0; bm_strip_lr.hip): right_keys [batch][H][W], filled with
// ~0 by the caller, receives the MIN over d of (C_L(u + d, d) << 8 | d) over d <= u + d < W: the separable path's
// right-view keys, whose low byte is dR
hipError_t launch_box_match_strip_lr(const MatchArgs& a, int batch, uint32_t* right_keys, hipStream_t s);
// SM_DEVICE_CU_GRID (bm_literal.hip): Device.cu's literal map, AD only for rows < 256 and cols < 320, all zero
// for W > 1024; needs W >= 320, H >= 256 and literal_workspace_bytes(D) of device scratch in `ws`
size_t literal_workspace_bytes(int D);
hipError_t launch_device_cu_literal(const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int radius, int D,
                                    uint32_t* ws, uint8_t* out, int opitch, hipStream_t s);
// semi-global matching (bm_sgm.hip): the paths' sum S u32 [D][H][W], zeroed by the caller, from the u16 SAD
// volume (0 <= P1 <= P2, 255 * win^2 + P2 <= 65535; paths: 4, or 8 with the diagonals), and the WTA over it: the left map (smallest existing d at
// min S, no threshold) and, when right_keys is given, the right view's keys [H][W], min over the d whose pair
// (u + d, d) exists of (S(u + d, d) << 8 | d)
// pr: which pairs exist (Pairs, above); with pr.in_view the maps hold d0 + k and a pixel with no candidate 0
hipError_t launch_sgm_paths(const uint16_t* sad, int W, int H, int D, int P1, int P2, int paths, const Pairs& pr,
                            uint32_t* S, hipStream_t s);
hipError_t launch_sgm_wta(const uint32_t* S, int W, int H, int D, const Pairs& pr, uint8_t* disp, int out_pitch,
                          uint32_t* right_keys, hipStream_t s);
// the same WTA, thresholdless, over a u16 cost volume [D][H][W] (SM_COST_CENSUS with SM_AGG_BOX)
hipError_t launch_cost_wta_u16(const uint16_t* C, int W, int H, int D, const Pairs& pr, uint8_t* disp, int out_pitch,
                               uint32_t* right_keys, hipStream_t s);
// sub-pixel WTA (bm_subpix.hip) over a d-major volume [D][H][W] of costs < 2^24: disp16 [H][pitch] receives
// q = 16 d0 + delta (1/16 px), right16 (optional, dense) the right view's q, mask (optional, dense) the validity.
// invalid_from: 0, or the left view is invalid where its minimum is >= it; uniq 0..99: the uniqueness ratio (0 off);
// right_pairs: 1 the right view over u + 2 d <= W, 2 over u + d < W; lr: the LR check on the two views' d0, through
// `scratch` (2 W H bytes).  Invalid and occluded pixels get q = 0, mask = 0.
// pr.in_view (SM_PAIRS_IN_VIEW): plane k is d = pr.d0 + k, q = 16 (d0 + k0) + delta up to 16 * 4095 + 8; the left view
// over x - d >= 0, the right view V_R(u, k) = V(u + d0 + k, k) over u + d0 + k <= W - 1 whatever right_pairs says; a
// pixel with no candidate is invalid; the views' disparities of the check are 16-bit, `scratch` 4 W H bytes.
hipError_t launch_subpix_wta_u32(const uint32_t* vol, int W, int H, int D, uint32_t invalid_from, int uniq,
                                 int right_pairs, bool lr, uint16_t* disp16, int pitch, uint16_t* right16,
                                 uint8_t* mask, uint8_t* scratch, hipStream_t s, const Pairs& pr = Pairs());
hipError_t launch_subpix_wta_u16(const uint16_t* vol, int W, int H, int D, uint32_t invalid_from, int uniq,
                                 int right_pairs, bool lr, uint16_t* disp16, int pitch, uint16_t* right16,
                                 uint8_t* mask, uint8_t* scratch, hipStream_t s, const Pairs& pr = Pairs());
// 1/16-px map -> points: xyz [H][xyz_pitch] floats, (X, Y, Z) / w of Q (x, y, q / 16, 1) (Q row-major 4 x 4),
// (0, 0, 0) where q == 0 or w == 0
hipError_t launch_reproject(const uint16_t* disp16, int W, int H, int pitch, const double* Q, float* xyz,
                            int xyz_pitch, hipStream_t s);
// census cost (bm_census.hip): the 9 x 7 census words u64 [H][W] of an image (replicated border, 62 bits), and
// the Hamming volume u8 [D][H][W] of two census images, popcount(cL(y, x) ^ cR(y, x - d)) for x >= d, else 0:
// the AD volume's layout, so launch_box_sad_volume sums it (<= 62 * win^2); W <= 4096
hipError_t launch_census(const uint8_t* img, int W, int H, int pitch, uint64_t* census, hipStream_t s);
// d0 (SM_PARAM_MIN_DISP, the matching calls alone): plane k compares cL(y, x) with cR(y, x - d0 - k), 0 for x < d0 + k
hipError_t launch_census_volume(const uint64_t* cL, const uint64_t* cR, int W, int H, int D, uint8_t* ham,
                                hipStream_t s, int d0 = 0);
// (2r+1)^2 median with replicate borders, radius 1..3 (bm_post.hip)
hipError_t launch_median(const uint8_t* src, int W, int H, int pitch, int64_t stride, int batch, int radius,
                         uint8_t* dst, int dpitch, int64_t dstride, hipStream_t s);
// The same for a 1/16-px map (bm_median16.hip): the element of rank 2r^2 + 2r of the window over the whole 16-bit
// value, replicate borders, radius 1..3, not in place; pitches and strides in elements.  One launch for the batch.
inline bool median16_pass_ok(int W, int H, int batch) {
    return W >= 1 && H >= 1 && batch >= 1 && (int64_t)((W + 63) / 64) * ((H + 31) / 32) * batch <= 0x7FFFFFFFll;
}
hipError_t launch_median16(const uint16_t* src, int W, int H, int pitch, int64_t stride, int batch, int radius,
                           uint16_t* dst, int dpitch, int64_t dstride, hipStream_t s);
// The sub-pixel calls' LR check on two median-filtered maps: d = (q + 8) >> 4 of disp16 and of the dense right map
// right_q (null: no check); occluded pixels get q = 0; mask (optional, dense) = final q != 0
hipError_t launch_subpix_lr_q(const uint16_t* right_q, int W, int H, uint16_t* disp16, int pitch, uint8_t* mask,
                              hipStream_t s);
// speckle filter (bm_speckle.hip), in place on `batch` maps of T = uint8_t or uint16_t (pitch and fstride in
// elements): every connected region (4-neighbours, both != 0, |a - b| <= max_diff) of at most max_size pixels is set
// to 0, and `mask` (dense [batch][H][W], may be null) is cleared at the same pixels.  label / count: the planes of
// plan_speckle(W, H, batch) (bm_speckle_plan.h).  max_size 0 launches nothing.
template <class T>
hipError_t launch_speckle(T* map, int W, int H, int pitch, int64_t fstride, int batch, int max_size, int max_diff,
                          uint8_t* mask, uint32_t* label, uint32_t* count, hipStream_t s);
// row fill (bm_fill.hip), in place on `batch` maps of T = uint8_t or uint16_t (pitch and fstride in elements): every
// run of at most max_gap invalid (0) pixels in a row takes the smaller of its two valid neighbours in that row, or
// the one it has at a border; everything else stays.  One launch for the batch, one workgroup per row, no workspace.
// max_gap 0 launches nothing.  fill_pass_ok: what the launcher takes (the rows of the batch are one grid, and a
// row's columns are walked in int steps of 4096).
inline bool fill_pass_ok(int W, int H, int batch) {
    return W >= 1 && W <= (1 << 30) && H >= 1 && batch >= 1 && (int64_t)H * batch <= 0x7FFFFFFFll;
}
template <class T>
hipError_t launch_fill(T* map, int W, int H, int pitch, int64_t fstride, int batch, int max_gap, hipStream_t s);

hipError_t launch_bgr_to_gray(const uint8_t* src, int W, int H, int pitch, int channels, uint8_t* dst, int dpitch,
                              hipStream_t s);
hipError_t launch_remap(const uint8_t* src, int W, int H, int pitch, const float* mapx, const float* mapy, int mpitch,
                        uint8_t* dst, int dpitch, hipStream_t s);

// rectification (bm_rectify.hip): OpenCV 2.4 stereoRectify (CV_CALIB_ZERO_DISPARITY, alpha = -1) on the
// host, and initUndistortRectifyMap (CV_32FC1) on the GPU.  r_len: 9 (3x3 matrix) or 3 (rotation vector).
bool stereo_rectify(const double* K1, const double* dist1, int ndist1, const double* K2, const double* dist2,
                    int ndist2, int width, int height, const double* R, int r_len, const double* T, double* R1,
                    double* R2, double* P1, double* P2, double* Q);
hipError_t launch_rectify_map(const double* K, const double* dist, int ndist, const double* R, const double* P,
                              int W, int H, float* mapx, float* mapy, int map_pitch, hipStream_t s);

}  // namespace sm
