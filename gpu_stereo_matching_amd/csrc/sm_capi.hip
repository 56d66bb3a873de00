// sm_capi.hip — the C ABI (include/sm_hip.h): handles, parameters, and the matching entry points.
// (sm_capi_volume.hip: the passes that keep a cost volume; sm_capi_aux.hip: the pre- / post-processing and volume
// calls; sm_capi_slice.hip: d-slices; sm_capi_group.hip: multi-GPU groups; sm_capi_speckle.hip: the speckle
// filter; sm_capi_fill.hip: the row fill; sm_handle.h: what they share.)
//
// Replaces blockMatching_gpu (BlockMatching/Device.cu:173-301).  Differences from the
// reference that are deliberate and documented in DESIGN.md:
//   * buffers are allocated once per handle, not per call, and are freed (Device.cu leaks
//     ~2*P*D bytes and the output buffer per call, :185-194, :300);
//   * every HIP call is checked and surfaced as an int status + sm_last_error_string()
//     (the reference never checks, so its W > 1024 launch failure returns all zeros, :253);
//   * any frame size works (the reference's fixed (8,10,D)x(32,32) grid covers 320x256 only, :231-233).
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "sm_handle.h"

namespace smh {

__thread char g_err[512] = "";

int check_geometry(const sm_handle* h, int width, int height, int pitch, int radius, int num_disp) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (width <= 0 || height <= 0) return fail(SM_ERR_INVALID_ARG, "bad frame size %dx%d", width, height);
    if (pitch < width) return fail(SM_ERR_INVALID_ARG, "pitch %d < width %d", pitch, width);
    if (radius < 0 || radius > 127) return fail(SM_ERR_INVALID_ARG, "radius %d out of [0,127]", radius);
    if (num_disp < 1 || num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "num_disp %d out of [1,%d] (uint8 disparity output)", num_disp, sm::kMaxDisp);
    const int64_t win = 2 * radius + 1;
    if (((int64_t)50 * win * win) >= (int64_t)1 << 23)
        return fail(SM_ERR_INVALID_ARG, "radius %d too large for the 32-bit (SAD<<8|d) key", radius);
    return SM_OK;
}

int check_capacity(const sm_handle* h, int width, int height, int num_disp) {
    if (width > h->max_w || height > h->max_h || num_disp > h->max_d)
        return fail(SM_ERR_CAPACITY, "frame %dx%d/D=%d exceeds handle capacity %dx%d/D=%d", width, height, num_disp,
                    h->max_w, h->max_h, h->max_d);
    return SM_OK;
}

// Host<->device 2-D copy.  Contiguous rows (both pitches == row bytes) go as one 1-D copy: the
// 2-D path takes a slow per-row route for widths that are not a multiple of 4 (measured 5.7 ms
// instead of 0.02 ms to upload a 463x370 pair).
// Pitched host buffers are gathered into / scattered from a contiguous host vector around one
// 1-D copy (the pageable 2-D path is the slow one, pitched or not).
static thread_local std::vector<uint8_t> g_host_rows;

hipError_t copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t row_bytes, size_t rows,
                  hipMemcpyKind kind, hipStream_t s) {
    if (dpitch == row_bytes && spitch == row_bytes) return hipMemcpyAsync(dst, src, row_bytes * rows, kind, s);
    if (kind == hipMemcpyHostToDevice && dpitch == row_bytes) {
        g_host_rows.resize(row_bytes * rows);
        for (size_t r = 0; r < rows; ++r)
            std::memcpy(g_host_rows.data() + r * row_bytes, static_cast<const uint8_t*>(src) + r * spitch, row_bytes);
        // a pageable source is staged before the call returns, so the vector may be reused
        return hipMemcpyAsync(dst, g_host_rows.data(), row_bytes * rows, kind, s);
    }
    if (kind == hipMemcpyDeviceToHost && spitch == row_bytes) {
        g_host_rows.resize(row_bytes * rows);
        hipError_t e = hipMemcpyAsync(g_host_rows.data(), src, row_bytes * rows, kind, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        for (size_t r = 0; r < rows; ++r)
            std::memcpy(static_cast<uint8_t*>(dst) + r * dpitch, g_host_rows.data() + r * row_bytes, row_bytes);
        return hipSuccess;
    }
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, row_bytes, rows, kind, s);
}

int upload_pair(sm_handle* h, const uint8_t* left, const uint8_t* right, int W, int H, int pitch, hipStream_t s,
                uint8_t** right_dev) {
    const int64_t P = (int64_t)W * H;
    if (h->ws_poison) {   // SM_PARAM_WORKSPACE_POISON: the frame buffers over all they were allocated with (sm_create)
        const size_t Pmax = (size_t)h->max_w * h->max_h;
        SM_HIP(hipMemsetAsync(h->d_left, h->ws_poison - 1, 2 * align256(Pmax), s));   // d_right lies in it
        SM_HIP(hipMemsetAsync(h->d_disp, h->ws_poison - 1, Pmax, s));
    }
    static const bool pair_copy = env_switch("SM_PAIR_COPY", true);   // 0 (A/B only): always two copies
    // a pair with the right frame right after the left one (one sm_host_alloc block of 2 frames, or any
    // contiguous (2, H, W) array) goes up as one copy into d_left .. d_left + 2P: one DMA transfer
    // instead of two
    if (right_dev && pitch == W &&
        reinterpret_cast<uintptr_t>(right) == reinterpret_cast<uintptr_t>(left) + (uintptr_t)P && pair_copy) {
        *right_dev = h->d_left + P;
        SM_HIP(hipMemcpyAsync(h->d_left, left, (size_t)(2 * P), hipMemcpyHostToDevice, s));
        return SM_OK;
    }
    if (right_dev) *right_dev = h->d_right;
    SM_HIP(copy2d(h->d_left, W, left, pitch, W, H, hipMemcpyHostToDevice, s));
    SM_HIP(copy2d(h->d_right, W, right, pitch, W, H, hipMemcpyHostToDevice, s));
    return SM_OK;
}

int run_box_pass(WsScope& ws, sm_handle* h, sm::MatchArgs a, int batch, const sm::BoxPlan& p, const BoxRightOut& r) {
    using sm::BoxLeft;
    using sm::BoxRight;
    hipStream_t s = ws.stream();
    const int64_t P = (int64_t)a.W * a.H, PB = P * batch;
    if (p.right == BoxRight::Unsupported)
        return fail(SM_ERR_INVALID_ARG, "box radius %d: no right-view keys outside the wide path", a.radius);
    uint8_t* vol = nullptr;
    if (p.rpart_bytes) {
        int rc = ws.get(h->rpart, p.rpart_bytes, &a.rpart);
        if (rc) return rc;
    }
    if (p.vol_bytes) {
        int rc = ws.get(h->vol, p.vol_bytes, &vol);
        if (rc) return rc;
    }
    const bool fused = p.right == BoxRight::Fused;
    switch (p.left) {
        case BoxLeft::Tile:
            if (!fused) {
                // a matrix-pipe launch that may draw its tiles from the queue takes the handle's grab counter
                uint32_t* queue = nullptr;
                if (sm::box_queue_candidate(sm::box_geom(a, batch), a.valid_mode, sm::device_cus(), h->box_kernel,
                                            h->box_workgroups, h->box_queue_workgroups)) {
                    int rc = ws.get(h->boxq, sizeof(uint32_t), &queue);
                    if (rc) return rc;
                }
                SM_HIP(sm::launch_box_match(a, batch, s, h->box_kernel, h->box_workgroups, queue,
                                            h->box_queue_workgroups));
            } else if (r.keys)
                SM_HIP(sm::launch_box_slice_lr_keys(a, batch, r.keys, s));
            else
                SM_HIP(sm::launch_box_match_lr(a, batch, r.check, r.map, r.mask, r.pitch, r.stride, s));
            break;
        case BoxLeft::Strip:
            if (!fused) {
                SM_HIP(sm::launch_box_match_strip(a, batch, s));
            } else {   // the right keys through the volume workspace; their low byte is dR
                uint32_t* rk = reinterpret_cast<uint32_t*>(vol);
                SM_HIP(hipMemsetAsync(rk, 0xFF, (size_t)PB * 4, s));
                SM_HIP(sm::launch_box_match_strip_lr(a, batch, rk, s));
                SM_HIP(sm::launch_keys_low_byte(rk, PB, r.map, s));
            }
            break;
        case BoxLeft::Wide:
            SM_HIP(sm::launch_box_match_wide(a, batch, reinterpret_cast<uint16_t*>(vol), r.map, r.pitch, r.stride, s,
                                             r.keys));
            break;
        case BoxLeft::Direct:
            SM_HIP(sm::launch_box_match_generic(a, batch, s));
            break;
    }
    if (p.right != BoxRight::Mirrored) return SM_OK;
    // the right map on the mirrored pair (StereoHelper.cpp:156-180 + :131-154): valid d <= x, no threshold; the
    // map stays mirrored
    uint8_t* mL = r.mirror;
    uint8_t* mR = mL + PB;
    SM_HIP(sm::launch_mirror(a.right, a.W, a.H, a.pitch, a.frame_stride, batch, mL, a.W, P, s));
    SM_HIP(sm::launch_mirror(a.left, a.W, a.H, a.pitch, a.frame_stride, batch, mR, a.W, P, s));
    sm::MatchArgs b = a;
    b.left = mL;
    b.right = mR;
    b.pitch = a.W;
    b.frame_stride = P;
    b.valid_mode = 1;
    b.seed_key = 0xFFFFFFFFu;
    b.thresh_key = 0xFFFFFFFFu;
    b.disp = r.map;
    b.out_pitch = r.pitch;
    b.out_frame_stride = r.stride;
    if (p.left == BoxLeft::Strip)
        SM_HIP(sm::launch_box_match_strip(b, batch, s));
    else
        SM_HIP(sm::launch_box_match_generic(b, batch, s));
    return SM_OK;
}

}  // namespace smh

using namespace smh;

namespace {

// What an entry point that honours SM_COST_CENSUS and SM_PAIRS_IN_VIEW checks before it touches the device.
int cost_check(const sm_handle* h, int width, int radius, int num_disp, unsigned flags) {
    const int rc = pairs_check(h, flags, num_disp, false, nullptr);
    if (rc) return rc;
    if (!(flags & SM_COST_CENSUS)) return SM_OK;
    if (flags & SM_AGG_SGM) return sgm_check(width, radius, flags, h->sgm_p1, h->sgm_p2, nullptr, nullptr);
    return census_check(width, radius, flags);
}

// Staged box path through AD (u8) + SAD (u16) volume workspaces, in launch groups of up to
// kStagedGroup frames (workspace <= kStagedBytes): one AD, one SAD and one WTA launch per group, as
// the fused path batches frames per launch.  The SAD launch sees the group's g*D planes as one
// volume; the WTA launch takes the frame from blockIdx.y.
constexpr int kStagedGroup = 8;
constexpr int64_t kStagedBytes = (int64_t)8 << 30;
int run_staged(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
               int64_t fstride, int radius, int D, bool med, uint8_t* disp, int opitch, int64_t ostride) {
    hipStream_t s = ws.stream();
    const int64_t P = (int64_t)W * H;
    if (W > 4096) return fail(SM_ERR_INVALID_ARG, "SM_STAGED: width %d exceeds 4096", W);
    const int64_t per_frame = 3 * P * D + (med ? P : 0);
    int group = (int)std::min<int64_t>(h->staged_group, std::max<int64_t>(1, kStagedBytes / per_frame));
    group = std::min(group, std::max(batch, 1));
    uint8_t* ad = nullptr;
    int rc = ws.get(h->vol, (size_t)(per_frame * group), &ad);
    if (rc) return rc;
    uint16_t* sad = reinterpret_cast<uint16_t*>(ad + group * P * D);
    uint8_t* raw = ad + 3 * group * P * D;
    if (!h->kev[0])
        for (auto& e : h->kev) SM_HIP(hipEventCreate(&e));
    h->kev_valid = false;
    for (int f0 = 0; f0 < batch; f0 += group) {
        const int g = std::min(group, batch - f0);
        const bool last = f0 + g >= batch;   // the last group's kernels are bracketed by events
        if (last) SM_HIP(hipEventRecord(h->kev[0], s));
        SM_HIP(sm::launch_ad_volume(L + f0 * fstride, R + f0 * fstride, W, H, pitch, fstride, g, D, ad, P * D, s));
        if (last) SM_HIP(hipEventRecord(h->kev[1], s));
        SM_HIP(sm::launch_box_sad_volume(ad, W, H, radius, g * D, sad, s));
        if (last) SM_HIP(hipEventRecord(h->kev[2], s));
        uint8_t* out = disp + f0 * ostride;
        SM_HIP(sm::launch_volume_wta(sad, W, H, D, g, seed_key(radius), med ? raw : out, med ? W : opitch,
                                     med ? P : ostride, s));
        if (last) SM_HIP(hipEventRecord(h->kev[3], s));
        if (med) SM_HIP(sm::launch_median(raw, W, H, W, P, g, 3, out, opitch, ostride, s));
        if (last) h->kev_frames = g;
    }
    h->kev_valid = batch > 0;
    return SM_OK;
}

// Core device-side pass over `batch` frames.  Workspace planes (lr) are dense W x H frames.
//   left map  : matched straight into `disp`, or into a workspace plane when SM_MEDIAN filters it
//               into `disp` afterwards (StereoDisparity.cpp:85/119);
//   right map : box as plan_box_pass says (bm_box_plan.h: fused with the left pass, or for the frames the wide
//               path rejects from the mirrored pair, kept mirrored); guided fused with the left pass (right keys
//               from the left costs, bm_guided.hip);
//   LR check  : StereoDisparity.cpp:136-147 on the (median-filtered, :119-126) maps.
// Every workspace comes through `ws`, which orders the pass after the handle's last one on another stream: a
// branch that takes none (box r <= 15 or the strip kernel without median and LR, guided without LR) stays
// outside that ordering and pays for no marker.
int run_device_body(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
                    int64_t fstride, int radius, int D, unsigned flags, uint8_t* disp, int opitch, int64_t ostride,
                    uint8_t* right_out, uint8_t* mask_out, int apitch, int64_t astride) {
    hipStream_t s = ws.stream();
    const bool guided = (flags & SM_AGG_GUIDED) != 0;
    const bool sgm = (flags & SM_AGG_SGM) != 0;
    const bool census = (flags & SM_COST_CENSUS) != 0;
    const bool lr = (flags & SM_LR_CHECK) != 0 || right_out || mask_out;
    const bool med = (flags & SM_MEDIAN) != 0;
    constexpr int kMedianRadius = 3;   // MeanFilter(disp, disp, 3)
    const int64_t P = (int64_t)W * H;
    const int64_t PB = P * batch;
    int sgm_p1 = 0, sgm_p2 = 0;
    sm::Pairs pairs;   // SM_PAIRS_IN_VIEW and the handle's minimum disparity: the volume paths alone take them
    {
        const int rc = pairs_check(h, flags, D, false, &pairs);
        if (rc) return rc;
    }
    if (sgm) {   // before the other flags' checks: the combinations are its to reject
        const int rc = sgm_check(W, radius, flags, h->sgm_p1, h->sgm_p2, &sgm_p1, &sgm_p2);
        if (rc) return rc;
    } else if (census) {
        const int rc = census_check(W, radius, flags);
        if (rc) return rc;
    }
    const bool volume = sgm || census;   // both maps come out of one cost volume (run_volume)
    if ((flags & SM_DEVICE_CU_GRID) != 0) {   // Device.cu's launch geometry, frame by frame (bm_literal.hip)
        if (flags != SM_DEVICE_CU_GRID || lr)
            return fail(SM_ERR_INVALID_ARG, "SM_DEVICE_CU_GRID is box aggregation only (flags 0x%x)", flags);
        if (W < 320 || H < 256)
            return fail(SM_ERR_INVALID_ARG,
                        "SM_DEVICE_CU_GRID: %dx%d is below the 320x256 the reference's fixed grid assumes "
                        "(Device.cu:231-233 reads and writes outside the frame)", W, H);
        uint32_t* scratch = nullptr;
        int rc = ws.get(h->vol, sm::literal_workspace_bytes(D), &scratch);
        if (rc) return rc;
        for (int f = 0; f < batch; ++f)
            SM_HIP(sm::launch_device_cu_literal(L + f * fstride, R + f * fstride, W, H, pitch, radius, D, scratch,
                                                disp + f * ostride, opitch, s));
        return SM_OK;
    }
    if ((flags & SM_STAGED) != 0) {
        if (guided || lr || radius > sm::kMaxFastRadius)
            return fail(SM_ERR_INVALID_ARG, "SM_STAGED supports box aggregation without LR, radius <= %d",
                        sm::kMaxFastRadius);
        return run_staged(ws, h, L, R, W, H, pitch, batch, fstride, radius, D, med, disp, opitch, ostride);
    }

    if (guided) {
        const int rc = guided_radius_check(radius);
        if (rc) return rc;
    }
    const bool box = !guided && !volume;
    sm::BoxPlan plan{};
    if (box)
        plan = sm::plan_box_pass({W, H, pitch, radius, 0, D, batch}, lr ? sm::RightWant::Map : sm::RightWant::None);
    // workspace: [left raw (med)] [right (lr)] [right filtered (lr && med)] [mirrored L, R (the plan's)]
    const bool mirrored = plan.right == sm::BoxRight::Mirrored;
    const int64_t n_planes = (med ? 1 : 0) + (lr ? 1 : 0) + (lr && med ? 1 : 0) + plan.mirror_planes;
    uint8_t* planes = nullptr;
    if (n_planes > 0) {
        int rc = ws.get(h->lr, (size_t)(n_planes * PB), &planes);
        if (rc) return rc;
    }
    uint8_t* left_raw = med ? planes : nullptr;
    if (med) planes += PB;
    uint8_t* right_map = lr ? planes : nullptr;   // plain (fused) or mirrored
    if (lr) planes += PB;
    uint8_t* right_med = (lr && med) ? planes : nullptr;
    if (lr && med) planes += PB;
    uint8_t* mirror = mirrored ? planes : nullptr;

    // ---- left map ----
    uint8_t* lmap = med ? left_raw : disp;
    const int lpitch = med ? W : opitch;
    const int64_t lstride = med ? P : ostride;
    sm::MatchArgs a{};   // d_lo 0, valid d <= W - x, no keys
    a.left = L;
    a.right = R;
    a.W = W;
    a.H = H;
    a.pitch = pitch;
    a.frame_stride = fstride;
    a.radius = radius;
    a.d_hi = D;
    a.seed_key = seed_key(radius);
    a.thresh_key = seed_key(radius);
    a.disp = lmap;
    a.out_pitch = lpitch;
    a.out_frame_stride = lstride;
    if (volume) {   // SGM and / or the census cost: the right view comes from the same volume as the left map
        const VolumeOut o{lmap, lpitch, lstride, lr ? right_map : nullptr};
        int rc = run_volume(ws, h, L, R, W, H, pitch, batch, fstride, radius, D, sgm, census, sgm_p1, sgm_p2, pairs, o);
        if (rc) return rc;
    } else if (guided) {
        sm::GuidedPass g{};   // d_lo 0, no keys
        g.left = L;
        g.right = R;
        g.W = W;
        g.H = H;
        g.pitch = pitch;
        g.frame_stride = fstride;
        g.batch = batch;
        g.radius = radius;
        g.d_hi = D;
        g.eps = h->guided_eps;
        g.disp = lmap;
        g.out_pitch = lpitch;
        g.out_frame_stride = lstride;
        if (lr) {   // the right view fused into the same pass (right keys from the left costs)
            int rc = ws.get(h->rpart, sm::guided_right_partial_bytes(W, H, radius, D, batch), &g.gpart);
            if (rc) return rc;
            g.right_map = right_map;
            g.rpitch = W;
            g.rstride = P;
        }
        SM_HIP(sm::launch_guided(g, s));
    } else {
        BoxRightOut ro;
        // without the median the tile kernels match, form the right view and check in one pass over the partials
        const bool one_pass = lr && !med && plan.left == sm::BoxLeft::Tile;
        if (one_pass) {
            ro.map = right_out;
            ro.pitch = apitch;
            ro.stride = astride;
            ro.check = 1;
            ro.mask = mask_out;
        } else if (lr) {
            ro.map = right_map;
            ro.pitch = W;
            ro.stride = P;
        }
        ro.mirror = mirror;
        int rc = run_box_pass(ws, h, a, batch, plan, ro);
        if (rc || one_pass) return rc;
    }
    if (med) SM_HIP(sm::launch_median(left_raw, W, H, W, P, batch, kMedianRadius, disp, opitch, ostride, s));
    if (!lr) return SM_OK;

    const uint8_t* rcheck = right_map;
    if (med) {   // the median commutes with the mirror, so a mirrored map is filtered as is
        SM_HIP(sm::launch_median(right_map, W, H, W, P, batch, kMedianRadius, right_med, W, P, s));
        rcheck = right_med;
    }
    SM_HIP(sm::launch_lr_check(disp, opitch, ostride, rcheck, W, P, mirrored ? 1 : 0, W, H, batch, disp, opitch,
                               ostride, right_out, mask_out, apitch, astride, s));
    return SM_OK;
}

// Page-locked blocks from sm_host_alloc: a map the caller receives into one of them is written by the
// kernel straight over PCIe (zero-copy), with no separate device-to-host copy.
std::mutex g_host_mu;
std::map<uintptr_t, size_t> g_host_blocks;

// Device address of [p, p + bytes) when that range lies in one sm_host_alloc block, else nullptr.
uint8_t* host_block_device_ptr(void* p, size_t bytes) {
    uintptr_t base = 0;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_blocks.upper_bound((uintptr_t)p);
        if (it == g_host_blocks.begin()) return nullptr;
        --it;
        if ((uintptr_t)p + bytes > it->first + it->second) return nullptr;
        base = it->first;
    }
    void* dbase = nullptr;
    if (hipHostGetDevicePointer(&dbase, reinterpret_cast<void*>(base), 0) != hipSuccess || !dbase) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint8_t*>(dbase) + ((uintptr_t)p - base);
}

// The upload / match / download split of a host call (SM_PARAM_STAGE_TIMING), between the handle's ev[0..3]: each
// mark costs a marker between the copy and compute queues, ~10 us per 1080p call for the two
// (profiles/microbench/r03_roundtrip_pair_block.txt), so ev[0..2] are recorded only when the split is wanted.
// ev[3] ends every call: the caller waits on it.
struct StageTimer {
    sm_handle* h;
    hipStream_t s;
    bool on;
    StageTimer(sm_handle* h_, hipStream_t s_) : h(h_), s(s_) {
        static const bool verbose = getenv("SM_VERBOSE") != nullptr;
        on = h->stage_timing == 1 || (h->stage_timing == 2 && (h->stage_requested || verbose));
    }
    hipError_t mark(int i) const { return on ? hipEventRecord(h->ev[i], s) : hipSuccess; }
    int finish() const {
        SM_HIP(hipEventRecord(h->ev[3], s));
        SM_HIP(hipEventSynchronize(h->ev[3]));
        if (on) {
            for (int i = 0; i < 3; ++i) SM_HIP(hipEventElapsedTime(&h->stage_ms[i], h->ev[i], h->ev[i + 1]));
        } else {
            h->stage_ms[0] = h->stage_ms[1] = h->stage_ms[2] = 0.f;
        }
        return SM_OK;
    }
};

}  // namespace

namespace smh {

// run_device_body on stream s inside one workspace scope (the workspaces lr / rpart / vol are per handle,
// ADVICE r1; a box pass at r 16..127 writes its V planes into vol and may grow it).
static int run_device(sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
                      int64_t fstride, int radius, int D, unsigned flags, uint8_t* disp, int opitch, int64_t ostride,
                      uint8_t* right_out, uint8_t* mask_out, int apitch, int64_t astride, hipStream_t s) {
    WsScope ws(h, s);
    // SM_SCRATCH_EVENT=1 (read once, for A/B) keeps the scratch event's wait and record for every pass, as before
    // round 4 dropped them from the passes without a workspace
    static const bool forced = env_switch("SM_SCRATCH_EVENT", false);
    if (forced) {
        const int rc = ws.touch();
        if (rc) return rc;
    }
    int rc = run_device_body(ws, h, L, R, W, H, pitch, batch, fstride, radius, D, flags, disp, opitch, ostride,
                             right_out, mask_out, apitch, astride);
    if (rc) return rc;
    if (h->speckle_size != 0) {
        // the speckle filter: the last step but one of every whole-frame matching call, on the final left map and the
        // valid mask (dense: apitch == W, astride == W * H in every caller); the right map stays as it is
        if (!sm::speckle_pass_ok(W, H, batch))
            return fail(SM_ERR_INVALID_ARG, "speckle filter: frame %dx%d too large", W, H);
        rc = run_speckle(ws, h, disp, 1, W, H, opitch, batch, ostride, h->speckle_size, h->speckle_range, mask_out);
        if (rc) return rc;
    }
    // the row fill: the last step, on the final left map alone; the mask keeps saying which pixels were measured.
    // A row band runs it too: rows never interact, so the kept rows get the frame's values
    return h->fill_gap == 0 ? SM_OK : run_fill(s, disp, 1, W, H, opitch, batch, ostride, h->fill_gap);
}

int host_match_rows(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                    int radius, int num_disp, unsigned flags, int keep0, int keep1, uint8_t* disp_out,
                    uint8_t* right_out, uint8_t* mask_out, int out_pitch) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!left || !right || !disp_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    if (out_pitch < width) return fail(SM_ERR_INVALID_ARG, "out_pitch %d < width %d", out_pitch, width);
    if (keep0 < 0 || keep1 > height || keep0 >= keep1) return fail(SM_ERR_INVALID_ARG, "bad kept rows");
    if (keep0 != 0 || keep1 != height) {
        rc = speckle_refuse(h, "a row band", "regions cross the bands (sm_group_block_match_batch_u8 runs whole frames)");
        if (rc) return rc;
    }
    rc = cost_check(h, width, radius, num_disp, flags);
    if (rc) return rc;
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int64_t P = (int64_t)width * height;
    uint8_t* aux = nullptr;
    if (right_out || mask_out) {
        rc = h->aux.reserve((size_t)(2 * P));
        if (rc) return rc;
        aux = h->aux.p;
    }
    // zero-copy map: a whole-frame call whose map goes to an sm_host_alloc block and is only written by
    // the last kernel (no LR check, no speckle filter and no row fill, which read the left map back)
    uint8_t* mapped = nullptr;
    static const bool zero_copy = env_switch("SM_ZERO_COPY", true);   // 0 (A/B): device buffer + download always
    if (zero_copy && keep0 == 0 && keep1 == height && !right_out && !mask_out && !(flags & SM_LR_CHECK) &&
        h->speckle_size == 0 && h->fill_gap == 0)
        mapped = host_block_device_ptr(disp_out, (size_t)(height - 1) * out_pitch + width);
    // the start event, like the stage marks, only when the split is recorded (round 4; SM_START_EVENT=1, read
    // once, records it in every call as before, for A/B)
    const StageTimer t(h, s);
    static const bool start_event = env_switch("SM_START_EVENT", false);
    if (t.on || start_event) SM_HIP(hipEventRecord(h->ev[0], s));
    uint8_t* dR = nullptr;
    rc = upload_pair(h, left, right, width, height, pitch, s, &dR);
    if (rc) return rc;
    SM_HIP(t.mark(1));
    rc = run_device(h, h->d_left, dR, width, height, width, 1, P, radius, num_disp, flags,
                    mapped ? mapped : h->d_disp, mapped ? out_pitch : width, P, right_out ? aux : nullptr,
                    mask_out ? aux + P : nullptr, width, P, s);
    if (rc) return rc;
    SM_HIP(t.mark(2));
    const int64_t k0 = (int64_t)keep0 * width;
    const int nk = keep1 - keep0;
    if (!mapped) SM_HIP(copy2d(disp_out, out_pitch, h->d_disp + k0, width, width, nk, hipMemcpyDeviceToHost, s));
    if (right_out) SM_HIP(copy2d(right_out, out_pitch, aux + k0, width, width, nk, hipMemcpyDeviceToHost, s));
    if (mask_out) SM_HIP(copy2d(mask_out, out_pitch, aux + P + k0, width, width, nk, hipMemcpyDeviceToHost, s));
    return t.finish();
}

}  // namespace smh

extern "C" {

SM_API const char* sm_version(void) { return "gpu_stereo_matching_amd 0.1.0 (gfx950)"; }

SM_API const char* sm_last_error_string(void) { return g_err; }

SM_API int sm_device_count(int* count) {
    if (!count) return fail(SM_ERR_INVALID_ARG, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return SM_OK;
}

SM_API int sm_create(int device, int max_width, int max_height, int max_disp, sm_handle** out) {
    if (!out) return fail(SM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    if (max_width <= 0 || max_height <= 0 || max_disp < 1 || max_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "bad capacity %dx%d/D=%d", max_width, max_height, max_disp);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SM_ERR_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(SM_ERR_DEVICE, "device %d out of range (%d visible)", device, n);
    hipDeviceProp_t prop;
    SM_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SM_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    SM_HIP(hipSetDevice(device));
    sm_handle* h = new (std::nothrow) sm_handle();
    if (!h) return fail(SM_ERR_OUT_OF_MEMORY, "host alloc");
    h->device = device;
    h->max_w = max_width;
    h->max_h = max_height;
    h->max_d = max_disp;
    const size_t P = (size_t)max_width * max_height;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    // the pair's device frames are one allocation, so a host pair that sits in one block (right frame
    // right after the left one) uploads as one DMA copy into d_left .. d_left + 2P (upload_pair: the right
    // frame is then read at d_left + P).  d_right itself starts 256-B aligned (at
    // d_left + P it was not even dword-aligned for odd max sizes).
    const size_t Pa = align256(P);
    if (e == hipSuccess) e = hipMalloc(&h->d_left, 2 * Pa);
    if (e == hipSuccess) h->d_right = h->d_left + Pa;
    if (e == hipSuccess) e = hipMalloc(&h->d_disp, P);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev[i]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->scratch_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        sm_destroy(h);
        return fail(e == hipErrorOutOfMemory ? SM_ERR_OUT_OF_MEMORY : SM_ERR_DEVICE, "sm_create: %s",
                    hipGetErrorString(e));
    }
    *out = h;
    return SM_OK;
}

SM_API int sm_destroy(sm_handle* h) {
    if (!h) return SM_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->scratch_ev && h->scratch_pending) (void)hipEventSynchronize(h->scratch_ev);   // device calls on other streams
    (void)hipFree(h->d_left);   // d_right lies in the same allocation
    (void)hipFree(h->d_disp);
    (void)h->lr.release();
    (void)h->rpart.release();
    (void)h->vol.release();
    (void)h->spk.release();
    (void)h->boxq.release();
    for (smh::DevBuf* b : {&h->aux, &h->maps, &h->bgr, &h->dsl}) (void)b->release();
    for (auto& ev : h->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : h->kev)
        if (ev) (void)hipEventDestroy(ev);
    if (h->scratch_ev) (void)hipEventDestroy(h->scratch_ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SM_OK;
}

SM_API int sm_set_param_f(sm_handle* h, int param, float value) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (param == SM_PARAM_GUIDED_EPS) {
        if (!(value > 0.f)) return fail(SM_ERR_INVALID_ARG, "guided eps must be > 0");
        h->guided_eps = value;
        return SM_OK;
    }
    if (param == SM_PARAM_STAGED_GROUP) {
        const int g = (int)value;
        if ((float)g != value || g < 1 || g > kStagedGroup)
            return fail(SM_ERR_INVALID_ARG, "staged launch group must be an integer in [1, %d]", kStagedGroup);
        if (g < h->staged_group && h->vol.allocated()) {
            // a smaller group bounds the workspace from now on: drop the larger volume once
            // the handle's pending work is done, and let the next staged call allocate the new size
            SM_HIP(hipSetDevice(h->device));
            SM_HIP(hipStreamSynchronize(h->stream));
            if (h->scratch_pending) SM_HIP(hipEventSynchronize(h->scratch_ev));
            SM_HIP(h->vol.release());
        }
        h->staged_group = g;
        return SM_OK;
    }
    if (param == SM_PARAM_STAGE_TIMING) {
        if (value != 0.f && value != 1.f && value != 2.f) return fail(SM_ERR_INVALID_ARG, "stage timing is 0, 1 or 2");
        h->stage_timing = (int)value;
        if (h->stage_timing == 2) h->stage_requested = false;   // back to the default: unarmed until read
        return SM_OK;
    }
    if (param == SM_PARAM_SGM_P1 || param == SM_PARAM_SGM_P2) {
        const int v = (int)value;
        if (!(value >= 0.f) || value > 65535.f || (float)v != value)
            return fail(SM_ERR_INVALID_ARG, "SGM penalty must be an integer in [0, 65535] (0 = auto)");
        (param == SM_PARAM_SGM_P1 ? h->sgm_p1 : h->sgm_p2) = v;
        return SM_OK;
    }
    if (param == SM_PARAM_SGM_PATHS) {
        if (value != 4.f && value != 8.f)
            return fail(SM_ERR_INVALID_ARG, "SGM paths must be 4 or 8 (8 adds the four diagonal paths)");
        h->sgm_paths = (int)value;
        return SM_OK;
    }
    if (param == SM_PARAM_BOX_KERNEL) {
        if (value != 0.f && value != 1.f && value != 2.f)
            return fail(SM_ERR_INVALID_ARG, "box kernel is 0 (auto), 1 (legacy) or 2 (matrix)");
        h->box_kernel = (int)value;
        return SM_OK;
    }
    if (param == SM_PARAM_BOX_WORKGROUPS) {
        // (the comparison also rejects NaN; floats above 2^24 are not every integer, and no launch has that many slots)
        if (!(value >= 0.f) || value > 16777216.f || (float)(int)value != value)
            return fail(SM_ERR_INVALID_ARG, "box workgroups must be an integer >= 0 (0 = auto)");
        h->box_workgroups = (int)value;
        return SM_OK;
    }
    if (param == SM_PARAM_BOX_QUEUE_WORKGROUPS) {
        if (!(value >= 0.f) || value > (float)sm::kMaxQueueWorkgroups || (float)(int)value != value)
            return fail(SM_ERR_INVALID_ARG, "box queue workgroups must be an integer in [0, %d] (0 = auto)",
                        sm::kMaxQueueWorkgroups);
        h->box_queue_workgroups = (int)value;
        return SM_OK;
    }
    if (param == SM_PARAM_UNIQUENESS) {
        const int v = (int)value;
        if (!(value >= 0.f) || value > 99.f || (float)v != value)
            return fail(SM_ERR_INVALID_ARG, "uniqueness ratio must be an integer in [0, 99] (0 = off)");
        h->uniqueness = v;
        return SM_OK;
    }
    if (param == SM_PARAM_SPECKLE_SIZE) {
        // (the comparison also rejects NaN; floats above 2^24 are not every integer, and a frame of the labels' 2^31 - 1
        // pixels at most has no larger region to keep)
        if (!(value >= 0.f) || value > 16777216.f || (float)(int)value != value)
            return fail(SM_ERR_INVALID_ARG, "speckle size must be an integer in [0, 2^24] (0 = off)");
        h->speckle_size = (int)value;
        return SM_OK;
    }
    if (param == SM_PARAM_SPECKLE_RANGE) {
        const int v = (int)value;
        if (!(value >= 0.f) || value > 255.f || (float)v != value)
            return fail(SM_ERR_INVALID_ARG, "speckle range must be an integer in [0, 255] (whole disparities)");
        h->speckle_range = v;
        return SM_OK;
    }
    if (param == SM_PARAM_FILL_GAP) {
        // (the comparison also rejects NaN; floats above 2^24 are not every integer, and any gap >= the width fills
        // every run)
        if (!(value >= 0.f) || value > 16777216.f || (float)(int)value != value)
            return fail(SM_ERR_INVALID_ARG, "fill gap must be an integer in [0, 2^24] (0 = off)");
        h->fill_gap = (int)value;
        return SM_OK;
    }
    if (param == SM_PARAM_MIN_DISP) {
        const int v = (int)value;
        if (!(value >= 0.f) || value > 4095.f || (float)v != value)
            return fail(SM_ERR_INVALID_ARG, "minimum disparity must be an integer in [0, 4095]");
        h->min_disp = v;
        return SM_OK;
    }
    if (param == SM_PARAM_SUBPIX_MEDIAN) {
        const int v = (int)value;
        if (!(value >= 0.f) || value > 3.f || (float)v != value)
            return fail(SM_ERR_INVALID_ARG,
                        "SM_PARAM_SUBPIX_MEDIAN: the sub-pixel median's radius must be an integer in [0, 3] (0 = off)");
        h->subpix_median = v;
        return SM_OK;
    }
    if (param == SM_PARAM_WORKSPACE_POISON) {
        const int v = (int)value;
        if (!(value >= 0.f) || value > 256.f || (float)v != value)
            return fail(SM_ERR_INVALID_ARG,
                        "SM_PARAM_WORKSPACE_POISON: %g is no integer in [0, 256] (0 = off, v = fill with byte v - 1); "
                        "it stays %d", (double)value, h->ws_poison);
        h->ws_poison = v;
        return SM_OK;
    }
    if (param == SM_PARAM_GUIDED_SUBPIX) {
        if (value != 0.f && value != 1.f)
            return fail(SM_ERR_INVALID_ARG, "SM_PARAM_GUIDED_SUBPIX: %g is neither 0 (off) nor 1 (on); it stays %d",
                        (double)value, h->guided_subpix);
        h->guided_subpix = (int)value;
        return SM_OK;
    }
    return fail(SM_ERR_INVALID_ARG, "unknown param %d", param);
}

SM_API int sm_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(SM_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (bytes == 0) return fail(SM_ERR_INVALID_ARG, "zero-byte host allocation");
    // portable: usable by every device's handle (a group's members copy from one frame); mapped: the
    // kernels may write a map straight into it (host_match_rows)
    SM_HIP(hipHostMalloc(out, bytes, hipHostMallocPortable | hipHostMallocMapped));
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_blocks[(uintptr_t)*out] = bytes;
    return SM_OK;
}

SM_API int sm_host_free(void* p) {
    if (!p) return SM_OK;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_blocks.erase((uintptr_t)p);
    }
    SM_HIP(hipHostFree(p));
    return SM_OK;
}

SM_API int sm_block_match_u8(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                             int pitch, int radius, int num_disp, unsigned flags, uint8_t* disp_out, int out_pitch) {
    return host_match_rows(h, left, right, width, height, pitch, radius, num_disp, flags, 0, height, disp_out, nullptr,
                           nullptr, out_pitch);
}

SM_API int sm_block_match_lr_u8(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                                int pitch, int radius, int num_disp, unsigned flags, uint8_t* disp_out,
                                uint8_t* right_disp_out, uint8_t* valid_mask_out, int out_pitch) {
    return host_match_rows(h, left, right, width, height, pitch, radius, num_disp, flags | SM_LR_CHECK, 0, height,
                           disp_out, right_disp_out, valid_mask_out, out_pitch);
}

SM_API int sm_block_match_bgr_u8(sm_handle* h, const uint8_t* left_bgr, const uint8_t* right_bgr, int width,
                                 int height, int pitch, int channels, int radius, int num_disp, unsigned flags,
                                 uint8_t* disp_out, int out_pitch) {
    int rc = check_geometry(h, width, height, width, radius, num_disp);
    if (rc) return rc;
    if (!left_bgr || !right_bgr || !disp_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    if ((channels != 3 && channels != 4) || pitch < width * channels || out_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad BGR layout");
    rc = cost_check(h, width, radius, num_disp, flags);
    if (rc) return rc;
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    const size_t row = (size_t)width * channels;
    rc = h->bgr.reserve(2 * row * height);
    if (rc) return rc;
    hipStream_t s = h->stream;
    uint8_t* dl = h->bgr.p;
    uint8_t* dr = dl + row * height;
    const int64_t P = (int64_t)width * height;
    // the stage split under the same SM_PARAM_STAGE_TIMING rule as the gray host calls
    const StageTimer t(h, s);
    SM_HIP(t.mark(0));
    SM_HIP(copy2d(dl, row, left_bgr, pitch, row, height, hipMemcpyHostToDevice, s));
    SM_HIP(copy2d(dr, row, right_bgr, pitch, row, height, hipMemcpyHostToDevice, s));
    SM_HIP(t.mark(1));
    SM_HIP(sm::launch_bgr_to_gray(dl, width, height, (int)row, channels, h->d_left, width, s));
    SM_HIP(sm::launch_bgr_to_gray(dr, width, height, (int)row, channels, h->d_right, width, s));
    rc = run_device(h, h->d_left, h->d_right, width, height, width, 1, P, radius, num_disp, flags, h->d_disp, width, P,
                    nullptr, nullptr, width, P, s);
    if (rc) return rc;
    SM_HIP(t.mark(2));
    SM_HIP(copy2d(disp_out, out_pitch, h->d_disp, width, width, height, hipMemcpyDeviceToHost, s));
    return t.finish();
}

SM_API int sm_last_staged_kernel_ms(sm_handle* h, float* ad_ms, float* sad_ms, float* wta_ms) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!h->kev_valid) return fail(SM_ERR_INVALID_ARG, "no SM_STAGED pass has run on this handle");
    SM_HIP(hipEventSynchronize(h->kev[3]));
    float t[3];
    for (int i = 0; i < 3; ++i) {
        SM_HIP(hipEventElapsedTime(&t[i], h->kev[i], h->kev[i + 1]));
        t[i] /= (float)h->kev_frames;
    }
    if (ad_ms) *ad_ms = t[0];
    if (sad_ms) *sad_ms = t[1];
    if (wta_ms) *wta_ms = t[2];
    return SM_OK;
}

SM_API int sm_last_stage_ms(sm_handle* h, float* upload_ms, float* match_ms, float* download_ms) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    h->stage_requested = true;   // auto mode: the calls from now on record the split
    if (upload_ms) *upload_ms = h->stage_ms[0];
    if (match_ms) *match_ms = h->stage_ms[1];
    if (download_ms) *download_ms = h->stage_ms[2];
    return SM_OK;
}

SM_API int sm_match_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                           int pitch, int batch, int64_t frame_stride, int radius, int num_disp, unsigned flags,
                           uint8_t* d_disp, int out_pitch, int64_t out_frame_stride, void* stream) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!d_left || !d_right || !d_disp) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    if (batch < 1) return fail(SM_ERR_INVALID_ARG, "batch %d < 1", batch);
    if (out_pitch < width) return fail(SM_ERR_INVALID_ARG, "out_pitch < width");
    if (batch > 1 && (frame_stride < (int64_t)pitch * height || out_frame_stride < (int64_t)out_pitch * height))
        return fail(SM_ERR_INVALID_ARG, "frame strides overlap");
    rc = cost_check(h, width, radius, num_disp, flags);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    return run_device(h, d_left, d_right, width, height, pitch, batch, frame_stride, radius, num_disp, flags, d_disp,
                      out_pitch, out_frame_stride, nullptr, nullptr, width, (int64_t)width * height, stream_of(stream));
}

SM_API int sm_stream_sync(sm_handle* h, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    SM_HIP(hipSetDevice(h->device));
    if (stream) {
        SM_HIP(hipStreamSynchronize(stream_of(stream)));
        return SM_OK;
    }
    // NULL: the default stream, which is what NULL means to every device entry point, and the
    // handle's own stream (host entry points, FrameStream-style callers)
    SM_HIP(hipStreamSynchronize(nullptr));
    SM_HIP(hipStreamSynchronize(h->stream));
    return SM_OK;
}

}  // extern "C"
