/*
 * sm_hip.h — C ABI of the MI355X stereo block-matching engine (libsm_hip.so).
 *
 * Drop-in boundary for the reference's GPU proxy
 *     void blockMatching_gpu(cv::Mat &h_left, cv::Mat &h_right, cv::Mat &h_disparity,
 *                            int SADWindowSize, int searchRange);
 * declared at BlockMatching/Device.cuh:50 and defined at BlockMatching/Device.cu:173-301.
 * The reference's argument meaning is kept exactly:
 *   SADWindowSize  -> `radius`    (window is (2*radius+1)^2; Device.cu:181, BlockMatching.cpp:119)
 *   searchRange    -> `num_disp`  (disparities d = 0 .. num_disp-1; Device.cu:43)
 * and so is the output convention: uint8 disparity, 0 where no window SAD falls
 * below 50*win^2 (Device.cu:37-38,63).
 *
 * Everything is plain C: pointers, sizes, int status codes.  No OpenCV or torch
 * types cross this boundary.  include/stereo_bm.hpp maps the reference's Mat API
 * onto it; gpu_stereo_matching_amd/_capi.py binds it with ctypes.
 *
 * Threading: one handle per host thread.  A handle owns its device buffers and a
 * HIP stream; calls on one handle are serialised.
 */
#ifndef SM_HIP_H
#define SM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SM_API __attribute__((visibility("default")))

/* ---- status codes (the reference has none: Device.cu never checks errors) ---- */
enum {
    SM_OK = 0,
    SM_ERR_INVALID_ARG = 1,   /* bad size / pointer / radius / num_disp */
    SM_ERR_OUT_OF_MEMORY = 2, /* hipMalloc / hipHostMalloc failed */
    SM_ERR_DEVICE = 3,        /* no usable gfx950 device */
    SM_ERR_LAUNCH = 4,        /* kernel launch or runtime error */
    SM_ERR_CAPACITY = 5       /* frame larger than the handle was created for */
};

/* ---- aggregation / post-processing flags ---- */
enum {
    SM_AGG_BOX = 0u,        /* (2r+1)^2 zero-padded SAD window: the reference's kernalFindCorr */
    SM_AGG_GUIDED = 1u,     /* guided-filter aggregation of the AD volume (this build's extension) */
    SM_LR_CHECK = 2u,       /* left-right consistency (STMatching/StereoDisparity.cpp:136-147):
                               occluded pixels are written as 0 */
    SM_MEDIAN = 4u,         /* 7x7 median post-filter of the WTA map(s), STMatching's
                               MeanFilter(disp, disp, 3) = ctmf (Toolkit.cpp:33-48); with
                               SM_LR_CHECK both maps are filtered before the check, in the
                               order of StereoDisparity.cpp:119-126 */
    SM_STAGED = 8u,         /* box path through explicit HBM volumes (AD u8 -> SAD u16 -> WTA),
                               the reference's two-kernel data flow (Device.cu:19-64); same
                               output as the fused kernel, bandwidth-bound; not with
                               SM_AGG_GUIDED or SM_LR_CHECK, radius <= 7.  Frames run in launch
                               groups of up to 8 (SM_PARAM_STAGED_GROUP), and the handle keeps the
                               volumes' workspace, 3*P*D (+ P with SM_MEDIAN) bytes per frame of a
                               group: ~6.4 GB at 1080p D=128 with 8-frame groups (capped at 8 GiB),
                               ~0.8 GB with groups of 1.  Lowering SM_PARAM_STAGED_GROUP frees the
                               workspace (after the handle's pending work), so the next staged call
                               allocates the smaller size */
    SM_DEVICE_CU_GRID = 16u,/* opt-in emulation of Device.cu's fixed launch geometry (Device.cu:231-233,
                               253): the AD cost only for rows < 256 and cols < 320, 0 elsewhere (the
                               memset, :193-194), and the all-zero map for width > 1024 (the failed
                               <<<rows, cols>>> launch, :191-192).  Equals the default map at exactly
                               320x256; width < 320 or height < 256 (where the reference reads and writes
                               out of bounds) is SM_ERR_INVALID_ARG.  Box aggregation only (no other flag);
                               whole frames only (not the row-band or d-slice group calls).  Uses
                               ~330 KB * num_disp of the handle's volume workspace */
    SM_AGG_SGM = 32u,       /* semi-global matching (this build's extension) on the box SAD cost C(d, y, x) (the
                               zero-padded (2r+1)^2 SAD of sm_sad_volume_device), radius <= 7, width <= 4096.  Over
                               the pairs that exist, x + d <= W (Device.cu:44), and the four directions rho =
                               (+-1, 0), (0, +-1) by default, the eight with the diagonals (+-1, +-1) too when
                               SM_PARAM_SGM_PATHS is 8, with q = p - rho:
                                 L(p, d) = C(p, d)                                          q outside the image
                                 L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + P1, L(q, d+1) + P1, M + P2) - M,
                                 M = min_k L(q, k);   S = sum of the four (or eight) L.
                               Left map: the smallest existing d at min S, no 50*win^2 threshold (S is no SAD).
                               Right view (SM_LR_CHECK): S_R(u, d) = S(u + d, d) over the d whose pair (u + d, d)
                               exists (u + 2d <= W), first minimum; then the usual check.  SM_MEDIAN filters both
                               maps before the check.  Integer throughout: 0 <= P1 <= P2 and
                               255 * win^2 + P2 <= 65535 (every L fits 16 bits), else SM_ERR_INVALID_ARG; penalties
                               from SM_PARAM_SGM_P1 / _P2.  Frames of a batch run one after another through
                               sm_sgm_workspace_bytes() of the handle's volume workspace (6 B per pixel and
                               disparity: ~1.6 GB at 1080p D=128).  Honoured by sm_block_match_u8, _lr_u8, _bgr_u8,
                               sm_match_device and sm_group_block_match_batch_u8.  SM_ERR_INVALID_ARG with
                               SM_AGG_GUIDED, SM_STAGED or SM_DEVICE_CU_GRID, and in the row-band group calls
                               (vertical paths cross the bands), the d-slice calls and the slice-key calls (the
                               recursion over d crosses the slices) */
    SM_COST_CENSUS = 64u,   /* census / Hamming matching cost (this build's extension) in place of the absolute
                               difference of gray values, with SM_AGG_BOX or SM_AGG_SGM; radius <= 7, width <= 4096.
                               Robust to exposure and gain differences between the cameras, and a bounded integer.
                                 census(y, x): uint64.  The window is 9 wide x 7 high, dx in [-4, 4], dy in [-3, 3],
                                   visited row-major (dy outer, dx inner), the centre skipped: 62 neighbours on bits
                                   0..61 in that order, bits 62-63 zero.  A bit is 1 iff I(clamp(y + dy, 0, H - 1),
                                   clamp(x + dx, 0, W - 1)) < I(y, x) (replicated border: any frame size is legal).
                                 ham[d][y][x] = popcount(censusL(y, x) ^ censusR(y, x - d)) for x >= d, else 0
                                   (<= 62; the layout and zero rule of sm_ad_volume_device).
                                 C = the zero-padded (2r+1)^2 window sum of ham (<= 62 * win^2 = 13950 at r = 7).
                               SM_AGG_BOX | SM_COST_CENSUS: the left map is the smallest existing d (x + d <= W) at
                               min C, with no 50 * win^2 threshold (that threshold is in AD units); the right view
                               (SM_LR_CHECK) is C_R(u, d) = C(u + d, d) over u + 2d <= W, first minimum: SM_AGG_SGM's
                               rules, applied to C; then the usual check.  SM_MEDIAN filters both maps before the
                               check.  SM_AGG_SGM | SM_COST_CENSUS: SM_AGG_SGM exactly, with C above in place of the
                               AD box SAD; the auto penalties become P1 = 10 * win^2, P2 = 120 * win^2 and the bound
                               62 * win^2 + P2 <= 65535 (sm_sgm_check with this bit in `flags`).  Frames of a batch
                               run one after another through sm_census_workspace_bytes() of the handle's volume
                               workspace (3 or 6 B per pixel and disparity, plus 20 B per pixel), allocated by the
                               first call that takes the flag.  Honoured by sm_block_match_u8, _lr_u8, _bgr_u8,
                               sm_match_device and sm_group_block_match_batch_u8.  SM_ERR_INVALID_ARG, before any
                               device work, with SM_AGG_GUIDED, SM_STAGED or SM_DEVICE_CU_GRID, for radius > 7 or
                               width > 4096, in the row-band group calls (the replicated border would differ at
                               the band edges), and in the d-slice and slice-key calls */
    SM_PAIRS_IN_VIEW = 128u /* the stereo-geometry pair rule (this build's extension; StereoSGBM's and libSGM's) for the
                               calls that keep a cost volume, in place of the reference's x + d <= W.  With d0 =
                               SM_PARAM_MIN_DISP, plane k of a volume stands for d = d0 + k, k = 0 .. num_disp - 1:
                                 left view   (x, k) exists iff x - (d0 + k) >= 0: k <= min(num_disp - 1, x - d0), a
                                             prefix, empty where x < d0;
                                 right view  V_R(u, k) = V(u + d0 + k, k) over u + d0 + k <= width - 1; every such pair
                                             exists in the left view.
                               The volumes keep their shape and zero rule: plane k compares L(y, x) with
                               R(y, x - d0 - k) and is 0 for x < d0 + k, and the box window sum is unchanged, so the
                               window of a candidate with x - d < radius still contains zero taps (a bias towards
                               large d in the leftmost columns; not normalised).  The recursion, the penalties, the
                               16-bit bound, the first-minimum rule and the parabola (where 1 <= k0 < kmax) are
                               SM_AGG_SGM's and the sub-pixel calls'; a previous pixel q with no existing k acts as a
                               q outside the image, L(p, .) = C(p, .).  A pixel with no candidate gives 0 in the 8-bit
                               and the 1/16-px map and 0 in the mask, in either view.  The maps hold the absolute
                               disparity, d0 + k0 and 16 (d0 + k0) + delta, so the median, the LR check, the
                               uniqueness test, speckle, fill and reproject run on them unchanged.  Near the right
                               border the true disparity stays a candidate, and near the left border the d > x that
                               the reference's zeroed volume lets win are gone.
                               Honoured by sm_block_match_u8, _lr_u8, _bgr_u8, sm_match_device and
                               sm_group_block_match_batch_u8 with SM_AGG_SGM or SM_COST_CENSUS; by
                               sm_match_subpix_device and sm_block_match_subpix_u16 with every aggregation they take;
                               by sm_volume_wta_subpix_device (the caller's plane k is d0 + k); accepted by
                               sm_sgm_check.  sm_sgm_workspace_bytes and sm_census_workspace_bytes do not depend on
                               it, and the public volume calls (sm_ad_volume_*, sm_census_volume_*,
                               sm_sad_volume_device) keep d0 = 0.  SM_ERR_INVALID_ARG, naming the flag, before any
                               device work: the 8-bit AD SM_AGG_BOX call without SM_COST_CENSUS (its fused kernels and
                               its threshold are the reference-parity path), SM_AGG_GUIDED, SM_STAGED,
                               SM_DEVICE_CU_GRID, and the row-band, d-slice and slice-key calls */
};

/* ---- scalar parameters (sm_set_param_f) ---- */
enum {
    SM_PARAM_GUIDED_EPS = 1,  /* guided-filter epsilon in AD^2 units (default 6.5025 = 1e-4 * 255^2) */
    SM_PARAM_STAGED_GROUP = 2, /* SM_STAGED frames per launch group, 1..8 (default 8): bounds the
                                  handle's staged workspace (see SM_STAGED) */
    SM_PARAM_STAGE_TIMING = 3, /* whether host calls record the upload / match / download split read by
                                  sm_last_stage_ms with two hipEvents (each a marker between the copy and
                                  compute queues, ~10 us per 1080p call together).  2 (default, auto):
                                  recorded once sm_last_stage_ms has been called on the handle (the calls
                                  after that first read), or in every call when the environment sets
                                  SM_VERBOSE; 1: always; 0: never, and sm_last_stage_ms reports 0.
                                  Setting 2 again returns to the unarmed default */
    SM_PARAM_SGM_P1 = 4,       /* SM_AGG_SGM penalty of a disparity step of 1: an integer >= 0, 0 (default) =
                                  auto, 8 * win^2 */
    SM_PARAM_SGM_P2 = 5,       /* SM_AGG_SGM penalty of a larger step: an integer >= 0, 0 (default) = auto,
                                  32 * win^2.  P1 <= P2 and 255 * win^2 + P2 <= 65535 are checked by the matching
                                  call, against its radius (sm_sgm_check) */
    SM_PARAM_BOX_KERNEL = 6,   /* which kernel the plain box pass (no LR, no median workspace needed) runs: 0
                                  (default) auto by launch size, 1 the VALU kernels at every size, 2 the
                                  matrix-pipe kernel at every size.  The maps and keys are the same bit for bit.
                                  The matrix-pipe kernel covers radius 1..7 without the fused right view: with
                                  SM_LR_CHECK, radius 0 or radius >= 8 the value 2 silently runs the VALU
                                  kernels.  Other values: SM_ERR_INVALID_ARG */
    SM_PARAM_UNIQUENESS = 7,   /* uniqueness ratio of the sub-pixel calls (sm_match_subpix_device and friends): an
                                  integer 0..99, 0 (default) = off.  Other values: SM_ERR_INVALID_ARG */
    SM_PARAM_BOX_WORKGROUPS = 8, /* workgroups of a matrix-pipe box launch, each walking a contiguous range of tiles
                                  and keeping the right band along a row of tiles: 0 (default) auto (the queue of
                                  SM_PARAM_BOX_QUEUE_WORKGROUPS, or 16 ranges per workgroup the device holds at
                                  once); an integer n >= 1 that many, at most one per
                                  tile (n >= tiles: one tile per workgroup, nothing kept).  The maps and keys do not
                                  depend on it; the VALU kernels ignore it.  Other values: SM_ERR_INVALID_ARG */
    SM_PARAM_SPECKLE_SIZE = 9, /* StereoSGBM's speckleWindowSize: an integer >= 0 (at most 2^24), 0 (default) = off.
                                  With a size > 0 every whole-frame matching call ends with the speckle filter
                                  (sm_speckle_filter_device) on its final left map, after the median and the LR
                                  check: regions of at most this many pixels become 0.  See "speckle filter" below
                                  for the calls that honour it and those that refuse it */
    SM_PARAM_SPECKLE_RANGE = 10, /* StereoSGBM's speckleRange: whole disparities, an integer 0..255, default 1.  The
                                  8-bit matching calls join neighbours with |a - b| <= range, the 1/16-px calls with
                                  |a - b| <= 16 * range, as StereoSGBM does on its 1/16-px map */
    SM_PARAM_FILL_GAP = 11,    /* the row fill's max_gap: an integer 0 .. 2^24, 0 (default) = off.  With a gap > 0
                                  every matching call that returns a map ends with the row fill
                                  (sm_fill_invalid_device) on its final left map, after the median, the LR check and
                                  the speckle filter: runs of at most this many invalid pixels in a row take the
                                  smaller of their two neighbours.  Other values: SM_ERR_INVALID_ARG.  See "row fill"
                                  below for the calls that honour it and those that refuse it */
    SM_PARAM_BOX_QUEUE_WORKGROUPS = 12, /* workgroups of a matrix-pipe box launch that draws its tiles from a queue
                                  (SM_PARAM_BOX_WORKGROUPS 0, two disparities per pass): 0 (default) auto, one per
                                  workgroup the device holds at once where each has enough tiles to draw, static
                                  ranges elsewhere; an integer n in 1 .. 2^20 that many at any launch size, also more
                                  than there are tiles.  The maps and keys do not depend on it.  Other values:
                                  SM_ERR_INVALID_ARG */
    SM_PARAM_SGM_PATHS = 13,   /* scan directions SM_AGG_SGM sums: 4 (default), rho = (+-1, 0), (0, +-1), or 8, those
                                  and the diagonals (+1, +1), (-1, +1), (+1, -1), (-1, -1), each under the same
                                  recursion, existence rule and penalties (a diagonal path starts, L = C, in the first
                                  row of its walk and in the column it enters the frame by).  S <= 8 * 65535 < 2^19;
                                  sm_sgm_check and sm_sgm_workspace_bytes do not depend on it, and everything after S
                                  (both views' WTA, median, LR check, the sub-pixel calls, speckle, fill) is
                                  unchanged.  Four more path passes per frame.  Other values: SM_ERR_INVALID_ARG */
    SM_PARAM_MIN_DISP = 14,    /* StereoSGBM's minDisparity for the SM_PAIRS_IN_VIEW calls: an integer 0 .. 4095,
                                  default 0; other values: SM_ERR_INVALID_ARG.  The call searches d = d0 .. d0 +
                                  num_disp - 1 in num_disp planes and its maps hold the absolute d.  The 8-bit calls
                                  need d0 + num_disp - 1 <= 255, the 1/16-px calls <= 4095 (q <= 65528), else
                                  SM_ERR_INVALID_ARG; d0 >= width is legal and gives the all-zero map.  With d0 > 0 every
                                  matching call without SM_PAIRS_IN_VIEW is refused, naming the parameter (the
                                  segment-tree calls aside, which have no disparity window of this kind) */
    SM_PARAM_SUBPIX_MEDIAN = 15, /* radius of the 16-bit median the sub-pixel calls run on both views' 1/16-px maps
                                  before the LR check: an integer 0..3, 0 (default) = off; other values:
                                  SM_ERR_INVALID_ARG, and the parameter keeps its value.  Read by sm_match_subpix_device,
                                  sm_block_match_subpix_u16 and sm_volume_wta_subpix_device alone (see "sub-pixel
                                  disparities" and "16-bit median" below); every other call ignores it */
    SM_PARAM_WORKSPACE_POISON = 16, /* a debugging aid: 0 (default) = off; an integer v in 1..256 makes every call fill
                                  each of the handle's shared workspaces it takes (whole capacity and slack, once per
                                  call, before its first kernel) and the frame buffers a host call uploads into (their
                                  whole allocation, before the copies) with byte v - 1, so that no result can depend on
                                  what an earlier call or a fresh allocation left there.  No result changes under any
                                  v; the cost is one fill of each workspace per call.  Off, nothing is enqueued.  The
                                  other staging buffers of the host calls and the segment-tree workspace are not
                                  filled.  Other values: SM_ERR_INVALID_ARG, and the parameter keeps its value, which
                                  the error text names */
    SM_PARAM_GUIDED_SUBPIX = 17 /* 1: sm_match_subpix_device and sm_block_match_subpix_u16 accept SM_AGG_GUIDED and
                                  build the guided cost volume per frame (see "sub-pixel disparity" below); 0
                                  (default): they refuse the flag, as they did before the volume kernel existed, so a
                                  caller that relies on the refusal keeps it.  Other values: SM_ERR_INVALID_ARG, and the
                                  parameter keeps its value.  Every other call ignores it */
};

typedef struct sm_handle sm_handle;

/* Library / device information. */
SM_API const char *sm_version(void);
SM_API const char *sm_last_error_string(void);      /* thread-local message of the last failure */
SM_API int sm_device_count(int *count);

/* Create a handle on HIP device `device`, sized for frames up to max_width x max_height and
 * up to max_disp disparities (1..256).  Device frame buffers are allocated once here (the
 * reference re-allocates and leaks ~2*P*D bytes per call: Device.cu:185-194). */
SM_API int sm_create(int device, int max_width, int max_height, int max_disp, sm_handle **out);
SM_API int sm_destroy(sm_handle *h);
SM_API int sm_set_param_f(sm_handle *h, int param, float value);

/* SM_AGG_SGM's argument rules, host-only (no device, no handle): resolves the penalties (0 = auto: P1 =
 * 8 * win^2, P2 = 32 * win^2) into *p1_out / *p2_out (either may be NULL) and returns SM_ERR_INVALID_ARG, with a
 * message naming the reason, for radius outside 0..7, width outside 1..4096, a negative penalty, P1 > P2,
 * 255 * win^2 + P2 > 65535, or `flags` combining SM_AGG_SGM with SM_AGG_GUIDED, SM_STAGED or SM_DEVICE_CU_GRID.
 * With SM_COST_CENSUS in `flags` the autos are P1 = 10 * win^2, P2 = 120 * win^2 and the bound is
 * 62 * win^2 + P2 <= 65535 (the census cost is at most 62 per pixel).
 * The matching entry points apply exactly this check. */
SM_API int sm_sgm_check(int width, int radius, unsigned flags, int p1, int p2, int *p1_out, int *p2_out);
/* Bytes of the handle's volume workspace one SM_AGG_SGM frame takes (host-only): the u32 sum volume S (whose
 * first bytes hold the u8 AD volume until the SAD volume is built), the u16 SAD volume and the right view's
 * u32 keys, 6 * P * num_disp + 4 * P plus alignment.  p2 (0 = auto) is checked as by sm_sgm_check. */
SM_API int sm_sgm_workspace_bytes(int width, int height, int num_disp, int radius, int p2, size_t *bytes);
/* Bytes of the handle's volume workspace one SM_COST_CENSUS frame takes (host-only).  `flags` chooses the
 * aggregation (SM_COST_CENSUS is implied): SM_AGG_BOX, 3 * P * num_disp + 20 * P (the u8 Hamming volume, the u16
 * cost volume, the right view's u32 keys and the two u64 census images); SM_AGG_SGM, sm_sgm_workspace_bytes + 16 * P
 * (the Hamming volume lies in the head of S); each part 256-B aligned.  The arguments are checked as by the
 * matching call (auto penalties for SM_AGG_SGM). */
SM_API int sm_census_workspace_bytes(int width, int height, int num_disp, int radius, unsigned flags, size_t *bytes);

/* Page-locked host memory for frames and maps (hipHostMalloc, portable).  The host entry points
 * take any host pointer; with buffers from here their copies run as DMA straight from / into the
 * caller's memory instead of through the runtime's pageable bounce buffers (the reference's
 * Mat data is pageable: Device.cu:212-216, 287-291).  sm_host_free(NULL) is a no-op. */
SM_API int sm_host_alloc(size_t bytes, void **out);
SM_API int sm_host_free(void *p);

/* Host-pointer entry point — the blockMatching_gpu replacement.
 * left/right: uint8 gray, `height` rows of `width` bytes at row stride `pitch` (>= width).
 * disp_out: uint8, `height` rows at stride `out_pitch`.  Synchronous, like the reference.
 * flags: SM_AGG_BOX | SM_AGG_GUIDED | SM_AGG_SGM, optionally | SM_LR_CHECK | SM_MEDIAN | SM_COST_CENSUS. */
SM_API int sm_block_match_u8(sm_handle *h, const uint8_t *left, const uint8_t *right,
                             int width, int height, int pitch, int radius, int num_disp,
                             unsigned flags, uint8_t *disp_out, int out_pitch);

/* Same, also returning the right-view disparity (may be NULL) and the LR valid mask
 * (1 = consistent, may be NULL).  Implies SM_LR_CHECK. */
SM_API int sm_block_match_lr_u8(sm_handle *h, const uint8_t *left, const uint8_t *right,
                                int width, int height, int pitch, int radius, int num_disp,
                                unsigned flags, uint8_t *disp_out, uint8_t *right_disp_out,
                                uint8_t *valid_mask_out, int out_pitch);

/* Per-stage timings of the last sm_block_match_* call in ms (hipEvents), mirroring the
 * reference's "upload data / pre calculation / find corr / download data" printouts
 * (Device.cu:218,238,257,292; "pre calculation" is fused into the match stage here).  With the
 * default SM_PARAM_STAGE_TIMING (auto) the first call of this function turns the recording on for
 * the handle's later calls; a call made while recording was off reads 0.  Any pointer may be NULL. */
SM_API int sm_last_stage_ms(sm_handle *h, float *upload_ms, float *match_ms, float *download_ms);

/* Kernel times (ms, hipEvents on the launch stream) of the last SM_STAGED pass, per frame: the
 * pass runs its frames in launch groups of up to 8 (one AD, one SAD and one WTA launch per group),
 * and each figure is the last group's launch time divided by its frame count.  AD volume
 * (kernalPreCal_V2, Device.cu:19-32), SAD volume and WTA (kernalFindCorr's two halves,
 * Device.cu:34-64).  Waits for that pass to finish.  Any pointer may be NULL. */
SM_API int sm_last_staged_kernel_ms(sm_handle *h, float *ad_ms, float *sad_ms, float *wta_ms);

/* ---- device-pointer entry points (inputs already resident in HBM) ----
 * All pointers are device pointers on the handle's device; `stream` is a hipStream_t used as
 * given (NULL = the device's default stream, as in the HIP runtime API).  Asynchronous: nothing
 * waits for completion.  Calls on one handle may use different streams: a pass that uses the
 * handle's workspace (LR, median, staged, guided LR) first waits for the handle's previous pass
 * when that ran on another stream.
 * `batch` frames are stored back to back: frame i starts at ptr + i*frame_stride. */
SM_API int sm_match_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right,
                           int width, int height, int pitch, int batch, int64_t frame_stride,
                           int radius, int num_disp, unsigned flags,
                           uint8_t *d_disp, int out_pitch, int64_t out_frame_stride, void *stream);

/* Disparity-slice keys for multi-GPU sharding over d: for every pixel the
 * minimum over valid d in [d_lo, d_hi) of ((SAD << 8) | d), seeded with (50*win^2) << 8.
 * Keys of disjoint slices combine with an elementwise unsigned min (an all-reduce MIN). */
SM_API int sm_slice_keys_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right,
                                int width, int height, int pitch, int radius, int d_lo, int d_hi,
                                uint32_t *d_keys, void *stream);

/* Key map -> disparity: d where (key >> 8) < 50*win^2, else 0 (Device.cu:37,57,63). */
SM_API int sm_keys_to_disp_device(sm_handle *h, const uint32_t *d_keys, int width, int height,
                                  int radius, uint8_t *d_disp, int out_pitch, void *stream);

/* Guided-aggregation d-slice keys (the same sharding over d for SM_AGG_GUIDED): per pixel the
 * best d in [d_lo, d_hi) (valid d <= W - x, no threshold) of the guided-filtered cost q, as
 * ((int32)(q * 2^14) << 8) | d; INT32_MAX where no d of the slice is valid.  Keys of disjoint
 * slices combine with an elementwise SIGNED min (q may be negative).  The handle's guided eps
 * applies.  The combined map equals the single-device guided map up to the 2^-14 quantisation of q
 * (near-ties of the fp32 costs may resolve to the other d). */
SM_API int sm_guided_slice_keys_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right,
                                       int width, int height, int pitch, int radius, int d_lo, int d_hi,
                                       int32_t *d_keys, void *stream);

/* Guided key map -> disparity: d where q < 50 (the Device.cu:37 seed, strict), else 0. */
SM_API int sm_guided_keys_to_disp_device(sm_handle *h, const int32_t *d_keys, int width, int height,
                                         uint8_t *d_disp, int out_pitch, void *stream);

/* ---- the guided cost volume, one pass (SM_AGG_GUIDED) ----
 * vol[d][y][x] = (int32)trunc(q(d) * 2^14), q the guided-filtered cost of pixel (y, x) at disparity d clamped to
 * [-512, 512): the cost field of sm_guided_slice_keys_device's key for the slice [d, d + 1), key >> 8 (arithmetic),
 * bit for bit, for every d in [0, num_disp) from one launch that computes the guide statistics once per tile
 * instead of once per d.  INT32_MAX where the pair does not exist (d > width - x).  d-major dense planes
 * [num_disp][height][width].  The radii (<= 7), sizes and the handle's SM_PARAM_GUIDED_EPS are the slice call's; a
 * handle with SM_PARAM_MIN_DISP > 0 is refused (plane 0 is d = 0).
 * sm_guided_volume_device: d_vol holds 4 * num_disp * width * height bytes; asynchronous on `stream`, no workspace.
 * sm_guided_volume_i32: the same on one host frame, synchronous, through the handle's volume workspace. */
SM_API int sm_guided_volume_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                                   int pitch, int radius, int num_disp, int32_t *d_vol, void *stream);
SM_API int sm_guided_volume_i32(sm_handle *h, const uint8_t *left, const uint8_t *right, int width, int height,
                                int pitch, int radius, int num_disp, int32_t *vol_out);
/* Bytes of the handle's volume workspace one SM_AGG_GUIDED frame of the sub-pixel calls takes (host-only; see
 * "sub-pixel disparity" below): 4 * P * num_disp for the costs and 4 * P for the LR check's planes, each rounded up
 * to 256.  width 1..4096, radius 0..7, num_disp 1..256. */
SM_API int sm_guided_workspace_bytes(int width, int height, int num_disp, int radius, size_t *bytes);

/* d-slice keys of BOTH views from one fused pass (multi-GPU d-slices with the LR check, SURVEY §8e "LR adds
 * a second packed reduction for the right view"): d_left_keys as sm_slice_keys_device (flags SM_AGG_BOX,
 * uint32) or sm_guided_slice_keys_device (SM_AGG_GUIDED, int32), and d_right_keys the right view's keys,
 * C_R(y, u, d) = C_L(y, u + d, d) (StereoHelper.cpp:156-180): per right pixel the minimum over d in
 * [d_lo, d_hi) with u + d < W of (cost << 8) | d, no threshold (:131-154); box: (SAD << 8 | d), guided:
 * (floor(q * 2^14) << 8 | d); INT32_MAX where no d of the slice reaches u.  Box right keys carry the sign bit
 * flipped, (SAD << 8 | d) ^ 0x80000000, because a wide window's key passes 2^31 from r = 91: right keys of
 * disjoint slices combine with a SIGNED elementwise MIN for both aggregations (box left keys: unsigned, as
 * sm_slice_keys_device's; guided left keys: signed).  Box radius <= 15 (fused right view) or 16..127 through
 * the wide path (width 4..4096); guided radius <= 7.  Uses the handle's right-view / volume workspace. */
SM_API int sm_slice_keys_lr_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                                   int pitch, int radius, int d_lo, int d_hi, unsigned flags, void *d_left_keys,
                                   void *d_right_keys, void *stream);

/* Combined right-view keys -> dR: the d field (low byte) of each of n keys (box or guided). */
SM_API int sm_right_keys_to_disp_device(sm_handle *h, const void *d_keys, int64_t n, uint8_t *d_disp, void *stream);

/* The left-right check of StereoDisparity.cpp:136-147 on device maps: d = dL(x); occluded when x - d < 0, d == 0
 * or |d - dR(x - d)| > 1; d_out = occluded ? 0 : d (may alias d_left_disp), d_mask (may be NULL) = !occluded. */
SM_API int sm_lr_check_device(sm_handle *h, const uint8_t *d_left_disp, const uint8_t *d_right_disp, int width,
                              int height, int pitch, uint8_t *d_out, uint8_t *d_mask, int out_pitch, void *stream);

/* Wait for all work queued on `stream`.  NULL means the default stream, as it does for every
 * device entry point, and also waits for the handle's own stream. */
SM_API int sm_stream_sync(sm_handle *h, void *stream);

/* ---- caller-side steps in front of the path (SURVEY §8f "next") ----
 * BGR(A) -> gray exactly as the reference's caller does it (Caller.cpp:15-16, OpenCV 2.4
 * cvtColor CV_BGR2GRAY, 8-bit fixed point): Y = (1868 B + 9617 G + 4899 R + 8192) >> 14.
 * `channels` is 3 (BGR) or 4 (BGRA; alpha ignored). */
SM_API int sm_bgr_to_gray_device(sm_handle *h, const uint8_t *d_bgr, int width, int height, int pitch,
                                 int channels, uint8_t *d_gray, int gray_pitch, void *stream);

/* Rectification remap with CV_32FC1 maps, the reference's kernalRemap (Device.cu:127-167):
 * bilinear, out-of-range taps -> 0, round half to even + saturate.  map_pitch in floats. */
SM_API int sm_remap_u8_device(sm_handle *h, const uint8_t *d_src, int width, int height, int pitch,
                              const float *d_mapx, const float *d_mapy, int map_pitch,
                              uint8_t *d_dst, int dst_pitch, void *stream);

/* ---- the AD cost volume itself ----
 * dif[d][y][x] = |L(y,x) - R(y,x-d)| for x >= d, else 0, as d-major planes [num_disp][height][width]
 * (PreCal, BlockMatching.cpp:89-109; kernalPreCal_V2 + memset, Device.cu:19-32,193-194).  The
 * matching entry points never build it; this is for callers of the reference's PreCal.
 * Device form: d_dif holds num_disp*width*height bytes.  Host form: synchronous, dif_out likewise.
 * width <= 4096. */
SM_API int sm_ad_volume_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                               int pitch, int num_disp, uint8_t *d_dif, void *stream);
SM_API int sm_ad_volume_u8(sm_handle *h, const uint8_t *left, const uint8_t *right, int width, int height,
                           int pitch, int num_disp, uint8_t *dif_out);

/* ---- the census cost's two stages (SM_COST_CENSUS) ----
 * sm_census_device: the census words of one image (`height` rows of `width` bytes at stride `pitch` >= width) as
 * dense uint64 [height][width]; any frame size.
 * sm_census_volume_*: ham[d][y][x] = popcount(censusL(y,x) ^ censusR(y,x-d)) for x >= d, else 0, as d-major planes
 * [num_disp][height][width] of uint8 (<= 62): the shape and zero rule of sm_ad_volume_*, which they mirror.  Device
 * form: d_ham holds num_disp*width*height bytes; the two census images go through 16 * P bytes of the handle's
 * volume workspace.  Host form: synchronous, ham_out likewise.  width <= 4096. */
SM_API int sm_census_device(sm_handle *h, const uint8_t *d_img, int width, int height, int pitch,
                            uint64_t *d_census, void *stream);
SM_API int sm_census_volume_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                                   int pitch, int num_disp, uint8_t *d_ham, void *stream);
SM_API int sm_census_volume_u8(sm_handle *h, const uint8_t *left, const uint8_t *right, int width, int height,
                               int pitch, int num_disp, uint8_t *ham_out);

/* ---- sub-pixel disparity: 1/16 px in uint16, uniqueness filter, 3-D reprojection (this build's extension) ----
 * The rule, all integer.  A pixel's costs V(d) over the d that exist, d = 0 .. dmax:
 *   left view   dmax = min(num_disp - 1, W - x);
 *   right view  V_R(u, d) = V(u + d, d) over u + 2 d <= W (the pairs of the 8-bit SGM / census right view); the AD
 *               box path (SM_AGG_BOX without SM_COST_CENSUS) takes u + d < W, its 8-bit right view's pairs.
 *   d0    = the first (smallest) d at min V: the d of the 8-bit call with the same flags.
 *   delta = floor((16 (a - c) + den) / (2 den)) with a = V(d0 - 1), b = V(d0), c = V(d0 + 1), den = a + c - 2 b
 *           (>= 1: d0 is the first minimum) where 1 <= d0 < dmax, else 0: round-half-up of 8 (a - c) / den, a floor
 *           division, in [-8, 8]; a two-wide plateau (c == b) gives +8.
 *   q     = 16 d0 + delta <= 4088.
 *   uniqueness u (SM_PARAM_UNIQUENESS, 1..99): the pixel is invalid if some existing d with |d - d0| > 1 has
 *           V(d) * (100 - u) < b * 100 (StereoSGBM's strict comparison); each view with its own V.
 *   threshold: with the AD cost under SM_AGG_BOX the left view is invalid where b >= 50 * win^2, as in the 8-bit
 *           call (whose right view has no threshold either); none for SM_AGG_SGM or SM_COST_CENSUS.
 *   SM_LR_CHECK: the 8-bit rule on the views' d0 (occluded when x - d < 0, d == 0 or |d - d0_R(x - d)| > 1), an
 *           invalid pixel of either view counting as d0 = 0.  With uniqueness off the mask equals the 8-bit call's.
 *   An invalid or occluded pixel gives q = 0 and mask = 0.  Without SM_LR_CHECK the mask is the left view's validity
 *   and the right map is not needed unless asked for.  The right map is never checked (as in the 8-bit calls).
 * The arithmetic is exact for V < 2^24 (the bound under which the 8-bit (V << 8 | d) key fits 32 bits).
 *
 * SM_AGG_GUIDED (optionally | SM_LR_CHECK), on a handle with SM_PARAM_GUIDED_SUBPIX = 1 (with the parameter at 0, the
 *   default, or a null handle, the flag is refused: SM_ERR_INVALID_ARG, "no cost volume", naming the parameter):
 *   per frame the one-pass guided volume (sm_guided_volume_device's costs) as
 *   uint32 V = trunc(q * 2^14) + 512 * 2^14 < 2^24, and the rule above on V; the parabola does not depend on the bias.
 *   Pairs of the 8-bit guided call: left view d <= min(num_disp - 1, W - x); right view V_R(u, d) = V(u + d, d) over
 *   u + d < W.  An entry with d > W - x holds the largest cost, 2^24 - 1: the right view's walk crosses such entries and
 *   never prefers one to a pair that exists.  Threshold: the left view is invalid where q >= 50, V >= (50 + 512) * 2^14,
 *   the 8-bit guided call's rule; the right view has none.  SM_PARAM_UNIQUENESS > 0 is refused (the ratio test has no
 *   meaning on a cost that can be negative), as are SM_PAIRS_IN_VIEW, SM_PARAM_MIN_DISP > 0, SM_COST_CENSUS, SM_AGG_SGM,
 *   SM_STAGED and SM_DEVICE_CU_GRID beside the flag: SM_ERR_INVALID_ARG with a message, before any device work.
 *   SM_PARAM_SUBPIX_MEDIAN, the LR check, the speckle filter and the row fill follow as for the other aggregations.
 *   d0 is the first minimum of the quantised costs; the 8-bit guided call decides on the fp32 q, so the two may differ
 *   where two costs lie within one quantum.  Workspace: sm_guided_workspace_bytes of the volume workspace.
 *
 * sm_match_subpix_device: flags SM_AGG_BOX, SM_AGG_SGM or SM_AGG_GUIDED, optionally | SM_COST_CENSUS (not with
 * SM_AGG_GUIDED) | SM_LR_CHECK; radius <= 7,
 * width <= 4096.  SM_MEDIAN (the flag is the 8-bit ctmf median; these calls take SM_PARAM_SUBPIX_MEDIAN, below),
 * SM_STAGED and SM_DEVICE_CU_GRID (no cost volume to interpolate) return SM_ERR_INVALID_ARG before any
 * device work.  d_disp16: [batch][height]
 * [out_pitch], out_pitch and out_frame_stride in uint16 elements; d_right16 / d_mask: dense [batch][height][width],
 * either may be NULL.  Frames of a batch run one after another through the handle's volume workspace:
 * sm_sgm_workspace_bytes / sm_census_workspace_bytes as for the 8-bit call, 3 * P * num_disp + 4 * P (each part
 * rounded up to 256) for the AD box path.  Asynchronous on `stream`.
 * sm_block_match_subpix_u16: the same on one host frame, synchronous; out_pitch in elements for all three outputs.
 * sm_volume_wta_subpix_device: the rule on a caller's d-major volume [num_disp][height][width] of uint16
 * (elem_bytes 2) or uint32 (elem_bytes 4) costs < 2^24, right view over u + 2 d <= W, with the handle's uniqueness;
 * invalid_from: 0 = no threshold, else the left view is invalid where b >= it; flags: 0 or SM_LR_CHECK (2 * P bytes
 * of the handle's LR workspace), each optionally with SM_PAIRS_IN_VIEW: plane k of the volume is then the disparity
 * SM_PARAM_MIN_DISP + k under that flag's rules for both views (4 * P bytes of the LR workspace with SM_LR_CHECK).
 *
 * SM_PARAM_SUBPIX_MEDIAN = r in 1..3 (all three calls): per frame, both views' WTA, parabola, uniqueness and threshold
 * run as above, without the check, into temporary uint16 planes; the (2r+1)^2 16-bit median (sm_median_u16_device's
 * rule; an invalid pixel's 0 is a value like any other) of the left plane goes to the caller's map and that of the
 * right plane to right16, which therefore returns the filtered right map; the right view is computed and filtered
 * only with SM_LR_CHECK or a right16 output.  With SM_LR_CHECK the rule above then runs on d = (q' + 8) >> 4 of the
 * two filtered maps, the 1/16-px values rounded to whole disparities (32-bit arithmetic: d reaches 4096 under
 * SM_PAIRS_IN_VIEW): occluded when x - d < 0, d == 0 or |d - d_R(x - d)| > 1, and occluded pixels get q = 0.  The mask
 * is (final q != 0), with or without the check.  Then the speckle filter and the row fill, as without the median.
 * This is the order of the 8-bit calls under SM_MEDIAN | SM_LR_CHECK: median of both maps, then the check.
 * The temporary planes, 2 * P bytes each, are one (no right view), two, or three (SM_LR_CHECK without right16) planes
 * of the handle's LR workspace, taken before the first launch and reused by every frame of a batch: at most 6 * P
 * bytes on top of sm_sgm_workspace_bytes / sm_census_workspace_bytes, whose values do not change; the check's
 * d0 planes are not used.  With the parameter at 0 the calls launch and allocate exactly what they did without it. */
SM_API int sm_match_subpix_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                                  int pitch, int batch, int64_t frame_stride, int radius, int num_disp,
                                  unsigned flags, uint16_t *d_disp16, int out_pitch, int64_t out_frame_stride,
                                  uint16_t *d_right16, uint8_t *d_mask, void *stream);
SM_API int sm_block_match_subpix_u16(sm_handle *h, const uint8_t *left, const uint8_t *right, int width, int height,
                                     int pitch, int radius, int num_disp, unsigned flags, uint16_t *disp16_out,
                                     uint16_t *right16_out, uint8_t *mask_out, int out_pitch);
SM_API int sm_volume_wta_subpix_device(sm_handle *h, const void *d_vol, int elem_bytes, int width, int height,
                                       int num_disp, uint32_t invalid_from, unsigned flags, uint16_t *d_disp16,
                                       int out_pitch, uint16_t *d_right16, uint8_t *d_mask, void *stream);
/* reprojectImageTo3D for 1/16-px maps: for q > 0, d = q / 16 and (X, Y, Z, w) = Q (x, y, d, 1), evaluated in double;
 * xyz[y][3 x ..] = (X / w, Y / w, Z / w) as fp32; q == 0 or w == 0 gives (0, 0, 0).  Q: row-major 4 x 4, as
 * sm_stereo_rectify writes it.  pitch in uint16 elements, xyz_pitch in floats per row (>= 3 * width).
 * sm_reproject_u16: host pointers, synchronous, any frame size. */
SM_API int sm_reproject_device(sm_handle *h, const uint16_t *d_disp16, int width, int height, int pitch,
                               const double *Q, float *d_xyz, int xyz_pitch, void *stream);
SM_API int sm_reproject_u16(sm_handle *h, const uint16_t *disp16, int width, int height, int pitch, const double *Q,
                            float *xyz_out, int xyz_pitch);

/* ---- 16-bit median: the (2r+1)^2 median of a 1/16-px map (this build's extension) ----
 * dst(y, x) = the element of rank 2 r^2 + 2 r (0-based) of the (2r+1)^2 window of src around (y, x), coordinates
 * clamped to the frame (replicate borders), over the whole 16-bit value: 0x00FF < 0x0100, and 0 is a value like any
 * other, so a pixel with enough invalid neighbours becomes invalid and an isolated hole is closed.  All integer.  Not
 * in place: d_dst must differ from d_src.  Columns >= width and rows >= height of dst are never written, and those of
 * src never read.  On uint8 values held in uint16 it equals sm_median_u8_device.
 * sm_median_u16_device: `batch` device maps, pitch / dst_pitch and frame_stride / dst_frame_stride in uint16
 * elements; asynchronous on `stream`; one launch, no workspace.  Every argument is checked before the device is
 * touched, each refusal naming what was wrong: radius in 1..3, the frame size, batch >= 1, both pitches >= width, the
 * pointers (null, or d_src == d_dst), frame strides that overlap (batch > 1), the handle and its capacity.
 * sm_median_u16: the same on one host frame, synchronous, staged through the handle. */
SM_API int sm_median_u16_device(sm_handle *h, const uint16_t *d_src, int width, int height, int pitch, int batch,
                                int64_t frame_stride, int radius, uint16_t *d_dst, int dst_pitch,
                                int64_t dst_frame_stride, void *stream);
SM_API int sm_median_u16(sm_handle *h, const uint16_t *src, int width, int height, int pitch, int radius,
                         uint16_t *dst, int dst_pitch);

/* ---- speckle filter: StereoSGBM's speckleWindowSize / speckleRange (this build's extension) ----
 * OpenCV's filterSpeckles(img, newVal = 0, maxSpeckleSize, maxDiff) on a uint8 map or a uint16 (1/16 px) map, in
 * which 0 is this library's invalid value.  All integer:
 *   a pixel is valid iff its value is != 0; invalid pixels belong to no region and are never changed;
 *   two 4-neighbours inside the frame are joined iff both are valid and |a - b| <= max_diff, the difference taken
 *     in 32 bits (255 against 1, or 65535 against 3, does not wrap);
 *   regions are the connected components of that graph (joining is transitive: a ramp with steps of max_diff is
 *     one region);
 *   every pixel of a region of at most max_size pixels is set to 0, and the mask plane, where one is given, is set
 *     to 0 at exactly those pixels; everything else stays byte for byte, the bytes between width and pitch
 *     included.  max_size = 0 removes nothing (no launch, no workspace).
 * sm_speckle_filter_device: in place on `batch` device maps of elem_bytes 1 (uint8) or 2 (uint16), pitch and
 * frame_stride in elements; d_mask: dense [batch][height][width] or NULL; asynchronous on `stream`.  Every argument
 * is checked before the device is touched: elem_bytes, max_size >= 0, 0 <= max_diff <= 255 / 65535, pitch >= width,
 * the handle's capacity.  The frames of a batch run in groups of up to 8, through sm_speckle_workspace_bytes() of
 * the handle: uint32 labels and uint32 counts, 8 B per pixel of a frame in the group.
 * sm_speckle_workspace_bytes: host-only (no device, no handle).
 * sm_speckle_filter_u8 / _u16: the same on one host frame (pitch in elements, mask_pitch in bytes; mask may be
 * NULL), synchronous.
 * With SM_PARAM_SPECKLE_SIZE > 0 the filter is the last step, after the median and the LR check, of
 * sm_block_match_u8, sm_block_match_lr_u8 (whose valid mask is cleared at the removed pixels too; the right map is
 * untouched), sm_block_match_bgr_u8, sm_match_device and sm_group_block_match_batch_u8 for every aggregation and
 * flag, and of sm_match_subpix_device / sm_block_match_subpix_u16 on the 1/16-px left map and the mask.  Calls
 * that cannot honour it return SM_ERR_INVALID_ARG, with a message naming the speckle filter, before any device
 * work: the row-band group calls (regions cross the bands), sm_group_dslice_block_match_u8 and
 * sm_dslice_rehearse_u8, and the slice-key calls (sm_slice_keys_device, sm_guided_slice_keys_device,
 * sm_slice_keys_lr_device).  The segment-tree calls do not apply it: their maps are scaled by `scale`.
 * Parity with OpenCV's filterSpeckles is by construction of the rule above (its flood fill compares each popped
 * pixel with its neighbours, so its regions are these components whatever the visiting order); it is not pinned
 * by a test against OpenCV. */
SM_API int sm_speckle_workspace_bytes(int width, int height, int batch, size_t *bytes);
SM_API int sm_speckle_filter_device(sm_handle *h, void *d_map, int elem_bytes, int width, int height, int pitch,
                                    int batch, int64_t frame_stride, int max_size, int max_diff, uint8_t *d_mask,
                                    void *stream);
SM_API int sm_speckle_filter_u8(sm_handle *h, uint8_t *map, int width, int height, int pitch, int max_size,
                                int max_diff, uint8_t *mask, int mask_pitch);
SM_API int sm_speckle_filter_u16(sm_handle *h, uint16_t *map, int width, int height, int pitch, int max_size,
                                 int max_diff, uint8_t *mask, int mask_pitch);

/* ---- row fill: invalidated disparities closed from their neighbours along the row (this build's extension) ----
 * The last step of a classical SGM pipeline, on a uint8 map or a uint16 (1/16 px) map in which 0 is this library's
 * invalid value.  The LR check and the speckle filter set 0 wherever they distrust a pixel; this step sets a value
 * back.  All integer, in place:
 *   a pixel is valid iff its value is != 0; valid pixels are never changed;
 *   a run is a maximal stretch of invalid pixels in one row, columns a .. b inside [0, width); its left neighbour is
 *     the pixel at a - 1 if a > 0, its right neighbour the pixel at b + 1 if b < width - 1; rows never interact;
 *   a run longer than max_gap (b - a + 1 > max_gap) stays as it is; otherwise every pixel of the run becomes
 *     min(left, right) when both neighbours exist, and the one neighbour's value when the run touches a border; a
 *     row with no valid pixel stays 0;
 *   the minimum is taken on the whole element: on a uint16 map 0x00FF against 0x0100 gives 0x00FF;
 *   max_gap = 0 fills nothing (no launch); any max_gap >= width fills every run; the range is 0 .. 2^24;
 *   the bytes between width and pitch are neither read as neighbours nor written.
 * Why the smaller value: it is the farther surface, and the pixels the check removes next to a depth edge are the
 * ones the nearer object hides in the other view, so what is seen there is the background.
 * Neighbours are valid pixels of the input, so the result does not depend on the order in which runs are filled.
 * A mask plane is not touched: after an LR-checked call, mask == 0 && disp != 0 marks exactly the filled pixels.
 * The map does not say which of its values were measured and which interpolated; a caller who needs the
 * distinction keeps the mask.
 * sm_fill_invalid_device: in place on `batch` device maps of elem_bytes 1 (uint8) or 2 (uint16), pitch and
 * frame_stride in elements; asynchronous on `stream`; one launch for the batch, no workspace.  Every argument is
 * checked before the device is touched: elem_bytes, the frame size, batch >= 1, pitch >= width, 0 <= max_gap <=
 * 2^24, the map pointer, the handle's capacity.
 * sm_fill_invalid_u8 / _u16: the same on one host frame (pitch in elements), synchronous.
 * With SM_PARAM_FILL_GAP > 0 the fill is the last step, after the median, the LR check and the speckle filter, of
 * sm_block_match_u8, sm_block_match_lr_u8 (the right map and the valid mask stay as they are),
 * sm_block_match_bgr_u8, sm_match_device and sm_group_block_match_batch_u8 for every aggregation and flag, and of
 * sm_match_subpix_device / sm_block_match_subpix_u16 on the 1/16-px left map.  The row-band group calls honour it
 * too: the rule never crosses a row, so a band's kept rows get exactly the frame's values (with the speckle filter
 * set as well, that filter's refusal comes first).  A map the caller receives into an sm_host_alloc block is then
 * written to a device buffer and downloaded, not written straight over PCIe: the fill reads the map back.  Calls
 * that cannot honour it return SM_ERR_INVALID_ARG, with a message naming the row fill, before any device work:
 * sm_group_dslice_block_match_u8 and sm_dslice_rehearse_u8 (the d-slice calls do not run the steps it comes
 * after), and the slice-key calls (sm_slice_keys_device, sm_guided_slice_keys_device, sm_slice_keys_lr_device:
 * keys are no map).  The segment-tree calls do not apply it, as with the speckle filter. */
SM_API int sm_fill_invalid_device(sm_handle *h, void *d_map, int elem_bytes, int width, int height, int pitch,
                                  int batch, int64_t frame_stride, int max_gap, void *stream);
SM_API int sm_fill_invalid_u8(sm_handle *h, uint8_t *map, int width, int height, int pitch, int max_gap);
SM_API int sm_fill_invalid_u16(sm_handle *h, uint16_t *map, int width, int height, int pitch, int max_gap);

/* u16 SAD volume sad[d][y][x] = zero-padded (2r+1)^2 window sum of the AD plane d, radius <= 7
 * (the volume kernalFindAllSAD / getAllSAD build, Device.cu:67-103 / BlockMatching.cpp:191-261,
 * without their uint8 truncation).  d_sad holds num_disp*width*height uint16. */
SM_API int sm_sad_volume_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                                int pitch, int radius, int num_disp, uint16_t *d_sad, void *stream);

/* getAllSAD (BlockMatching.cpp:191-261; BlockMatching.h:11): every window SAD, PIXEL-major
 * sad[(y*width + x)*num_disp + d], stored as uint8 (the reference's uchar store truncates mod 256,
 * :258), and 255 where x + d > width (:245-249).  Any radius (r <= 7 and width <= 4096 go through the
 * AD and u16 SAD volumes of SM_STAGED plus a transpose; other sizes through a direct kernel).
 * Device form: d_sad holds width*height*num_disp bytes, asynchronous on `stream`, uses the handle's
 * volume workspace (~4*P*num_disp bytes).  Host form: synchronous, sad_out likewise sized. */
SM_API int sm_all_sad_device(sm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int width, int height,
                             int pitch, int radius, int num_disp, uint8_t *d_sad, void *stream);
SM_API int sm_all_sad_u8(sm_handle *h, const uint8_t *left, const uint8_t *right, int width, int height,
                         int pitch, int radius, int num_disp, uint8_t *sad_out);

/* ---- post-filter ----
 * (2r+1)^2 median with replicate borders, r in 1..3: ctmf (STMatching/ctmf.c:378-433) as called
 * by MeanFilter (Toolkit.cpp:33-48).  Not in place: d_src and d_dst must not overlap. */
SM_API int sm_median_u8_device(sm_handle *h, const uint8_t *d_src, int width, int height, int pitch,
                               int radius, uint8_t *d_dst, int dst_pitch, void *stream);

/* Host-pointer, synchronous forms of the two steps above (the reference's cvtColor_gpu /
 * remap_gpu, Device.cuh:51-52).  Buffers are staged through the handle. */
SM_API int sm_bgr_to_gray_u8(sm_handle *h, const uint8_t *bgr, int width, int height, int pitch, int channels,
                             uint8_t *gray, int gray_pitch);
SM_API int sm_remap_u8(sm_handle *h, const uint8_t *src, int width, int height, int pitch, const float *mapx,
                       const float *mapy, int map_pitch, uint8_t *dst, int dst_pitch);

/* ---- rectification maps (the step before the remap) ----
 * The reference's remapTest (Caller.cpp:27-74) builds its maps with Rectify (Utility.cpp:228-234):
 * OpenCV 2.4 stereoRectify(K1, D1, K2, D2, size, R, T, R1, R2, P1, P2, Q, CV_CALIB_ZERO_DISPARITY)
 * (alpha = -1, newImageSize = size) and initUndistortRectifyMap(Kk, Dk, Rk, Pk, size, CV_32FC1).
 * Matrices are row-major doubles: K 3x3, R 3x3 (r_len 9) or a rotation vector (r_len 3), T 3,
 * R1/R2 3x3, P1/P2 3x4, Q 4x4.  dist: ndist = 0, 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]].
 * sm_stereo_rectify is host-only math (no device, no handle). */
SM_API int sm_stereo_rectify(const double *K1, const double *dist1, int ndist1, const double *K2,
                             const double *dist2, int ndist2, int width, int height, const double *R,
                             int r_len, const double *T, double *R1, double *R2, double *P1, double *P2,
                             double *Q);
/* CV_32FC1 maps for one camera on the GPU (map_pitch in floats).  Device form: asynchronous on
 * `stream`; host form: synchronous, maps staged through the handle. */
SM_API int sm_init_rectify_map_device(sm_handle *h, const double *K, const double *dist, int ndist,
                                      const double *R, const double *P, int width, int height,
                                      float *d_mapx, float *d_mapy, int map_pitch, void *stream);
SM_API int sm_init_rectify_map(sm_handle *h, const double *K, const double *dist, int ndist,
                               const double *R, const double *P, int width, int height, float *mapx,
                               float *mapy, int map_pitch);

/* imread -> cvtColor -> blockMatching_gpu in one call (Caller.cpp:12-19): BGR(A) host frames
 * are uploaded, converted to gray on the GPU and matched.  Synchronous. */
SM_API int sm_block_match_bgr_u8(sm_handle *h, const uint8_t *left_bgr, const uint8_t *right_bgr,
                                 int width, int height, int pitch, int channels, int radius,
                                 int num_disp, unsigned flags, uint8_t *disp_out, int out_pitch);

/* STMatching's segment-tree stereo, ST-1 (stereo_disparity_normal, StereoDisparity.cpp:57-89; SURVEY
 * §8f rank 4): BGR host frames (3 bytes per pixel, row pitch `pitch`) -> truncated colour + gradient
 * cost over d in [0, max_level) -> segment-tree aggregation on the left view's colour tree
 * (sigma, TAU = 1200) -> WTA -> 7x7 median -> disparity x scale (saturated), uint8 [height][out_pitch].
 * The cost, the filter, the WTA and the median run on the GPU; the tree (a sequential Kruskal / BFS,
 * as in the reference) is built on the host from the GPU's edge weights.  Synchronous.
 * Reference defaults (STMatching/main.cpp:49-51): max_level 60, scale 4, sigma 0.1. */
SM_API int sm_segment_tree_match_bgr_u8(sm_handle *h, const uint8_t *left_bgr, const uint8_t *right_bgr,
                                        int width, int height, int pitch, int max_level, int scale, float sigma,
                                        uint8_t *disp_out, int out_pitch);
/* STMatching's ST-2 (stereo_disparity_iteration, StereoDisparity.cpp:91-160; main.cpp's method 1), same
 * arguments and output as sm_segment_tree_match_bgr_u8: first-pass left and right maps on colour trees
 * of each view (sigma SIGMA_ONE = 0.08, Toolkit.h:35; the right cost taken from the left's,
 * StereoHelper.cpp:156-180), each WTA + 7x7 median; the left-right check (:129-147); then a colour +
 * depth tree (CColorDepthWeight, SegmentTree.cpp:196-219) on the left view, the first left map and
 * the check's mask, filtered with `sigma`, WTA, 7x7 median, x scale.  The three trees' segment_graph
 * passes run on the host (the first two on two threads), their BFS on the GPU; everything O(P*D) runs
 * on the GPU.  Synchronous. */
SM_API int sm_segment_tree_refined_bgr_u8(sm_handle *h, const uint8_t *left_bgr, const uint8_t *right_bgr,
                                          int width, int height, int pitch, int max_level, int scale, float sigma,
                                          uint8_t *disp_out, int out_pitch);
/* last segment-tree call (either method): tree-build time (the host's segment_graph passes and the BFS,
 * until its level count is known), whole-call time (ms) and the last tree's BFS level count */
SM_API int sm_last_segment_tree_stats(sm_handle *h, float *tree_ms, float *total_ms, int *levels);
/* diagnostics: the last call's last tree (ST-1 its colour tree, ST-2 the colour + depth tree) in BFS
 * order, as SegmentTree.cpp:97-130 lays it out: ints = rank[P] (pixel -> BFS index), parent[P],
 * first[P] (first child), child[P] (count | distance bytes << 8), level offsets[levels + 1]
 * (n_ints >= 4P + levels + 1); pdist[P] = distance byte to the parent, n_bytes == P exactly (the last
 * call's pixel count; another value is SM_ERR_INVALID_ARG, so a stale width x height cannot mis-slice).
 * Synchronous. */
SM_API int sm_last_segment_tree_arrays(sm_handle *h, int *ints, int64_t n_ints, uint8_t *pdist, int64_t n_bytes,
                                       int *levels);

/* ---- several GPUs from one host thread (sm_create_group) ----
 * A group holds one handle and one host worker thread per device (devices == NULL: 0..ngpu-1;
 * a device may repeat).  Calls are synchronous, like sm_block_match_u8.
 *  - sm_group_block_match[_lr]_u8: ONE frame in row bands of whole 32-row tiles, one band per
 *    device, each matched from its rows plus the window halo (r; guided max(2r, 16); +3 with
 *    SM_MEDIAN) and downloaded straight into its rows of disp_out.  Every flag is row-local, so
 *    the result equals sm_block_match[_lr]_u8 bit for bit (the guided bands start on the full
 *    frame's tile grid).  No device-to-device traffic: the host frame is the gather point.
 *  - sm_group_block_match_batch_u8: nframes independent pairs, frame f on member f mod ngpu. */
typedef struct sm_group sm_group;
SM_API int sm_create_group(int ngpu, const int *devices, int max_width, int max_height, int max_disp,
                           sm_group **out);
SM_API int sm_destroy_group(sm_group *g);
SM_API int sm_group_size(const sm_group *g, int *n);
SM_API int sm_group_set_param_f(sm_group *g, int param, float value);
SM_API int sm_group_block_match_u8(sm_group *g, const uint8_t *left, const uint8_t *right, int width,
                                   int height, int pitch, int radius, int num_disp, unsigned flags,
                                   uint8_t *disp_out, int out_pitch);
SM_API int sm_group_block_match_lr_u8(sm_group *g, const uint8_t *left, const uint8_t *right, int width,
                                      int height, int pitch, int radius, int num_disp, unsigned flags,
                                      uint8_t *disp_out, uint8_t *right_disp_out, uint8_t *valid_mask_out,
                                      int out_pitch);
SM_API int sm_group_block_match_batch_u8(sm_group *g, const uint8_t *const *lefts,
                                         const uint8_t *const *rights, int nframes, int width, int height,
                                         int pitch, int radius, int num_disp, unsigned flags,
                                         uint8_t *const *disps, int out_pitch);
/* ONE frame sharded over the disparity range, the north star's split (Device.cu:43-61: every d
 * plane is independent, so no halo): member k computes packed keys (SAD << 8 | d; guided:
 * (int)(q * 2^14) << 8 | d) for d in [k*D/n, (k+1)*D/n) on its own device, one RCCL MIN
 * reduce-scatter over xGMI gives each member the global argmin of 1/n of the pixels (the
 * reference's first-smallest-d tie rule survives the MIN), each member finalises its pixels to
 * uint8 (the Device.cu:37 threshold) and one RCCL all-gather assembles the map on every member;
 * member 0's copy is downloaded into disp_out.  Bit-identical to sm_block_match_u8 for box
 * aggregation; guided keys quantise q to 2^-14, so two fp32 costs closer than that may resolve
 * differently from a single pass.  flags: 0 (box) or SM_AGG_GUIDED, optionally | SM_LR_CHECK: each
 * member also emits the right view's keys for its slice from the same fused pass
 * (sm_slice_keys_lr_device), a second MIN reduce-scatter + all-gather forms dR, and member 0 applies
 * StereoDisparity.cpp:136-147 before the download (box LR: any radius the wide path takes).  Members must be distinct
 * devices; RCCL (librccl.so.1) is loaded on first use and one communicator per member is created
 * with ncclCommInitAll.
 * Failure handling: the call runs in two phases.  Phase 1 (upload, slice keys, stream sync) runs on
 * every member; if any member fails there, the call returns its error before any collective is
 * enqueued.  In phase 2 (the collectives) a member that cannot take part aborts its communicator
 * and the others, which poll their streams instead of blocking, abort theirs; the call returns the
 * error and the next call re-creates the communicators.  Test hook: the environment variable
 * SM_DSLICE_FAULT="<member>:keys" or "<member>:collective" injects a failure of that member in
 * phase 1 or in place of its phase-2 collectives. */
SM_API int sm_group_dslice_block_match_u8(sm_group *g, const uint8_t *left, const uint8_t *right, int width,
                                          int height, int pitch, int radius, int num_disp, unsigned flags,
                                          uint8_t *disp_out, int out_pitch);

/* The d-slice plan shared by sm_group_dslice_block_match_u8 and the torch path (sharding.py): for a
 * frame of `pixels` pixels split over `members`, member `member` scans d in [*d_lo, *d_hi) =
 * [member*num_disp/members, (member+1)*num_disp/members) (empty when members > num_disp), the keys
 * are padded to *padded_pixels = members * *chunk pixels with the "no match" key, and the MIN
 * reduce-scatter hands the member pixels [member * *chunk, (member+1) * *chunk).  Host-only (no
 * device, no handle); any output pointer may be NULL. */
SM_API int sm_dslice_plan(int64_t pixels, int num_disp, int members, int member, int *d_lo, int *d_hi,
                          int64_t *chunk, int64_t *padded_pixels);

/* The d-slice split rehearsed on ONE device: the `members` members of sm_group_dslice_block_match_u8
 * run one after another on this handle through the same per-member key pass, padding and
 * finalisation; the RCCL MIN reduce-scatter is an elementwise MIN of their key maps and the
 * all-gather puts chunk k at offset k*chunk.  The map must equal sm_block_match_u8's (box) for any
 * member count; it lets the plan for n > 1 be checked on a one-GPU machine.  flags: 0 or
 * SM_AGG_GUIDED, optionally | SM_LR_CHECK (the right keys' MIN and the LR check as in the group call);
 * members 1..64.  Synchronous. */
SM_API int sm_dslice_rehearse_u8(sm_handle *h, const uint8_t *left, const uint8_t *right, int width,
                                 int height, int pitch, int radius, int num_disp, unsigned flags,
                                 int members, uint8_t *disp_out, int out_pitch);

#ifdef __cplusplus
}
#endif
#endif /* SM_HIP_H */
