// sm_capi_slice.hip — the C ABI's d-slice calls: key maps over a slice of the disparity range, their
// finalisation, the d-slice plan, and the one-device rehearsal of the group's d-slice mode.
#include <algorithm>

#include "sm_handle.h"

using namespace smh;

namespace {

// keys no d of the slice improves: the Device.cu:37 seed (box) / INT32_MAX (guided, signed keys)
uint32_t dslice_none_key(int radius, bool guided) { return guided ? 0x7FFFFFFFu : seed_key(radius); }
// right-view keys no d of the slice reaches (no seed: StereoHelper.cpp:131-154 has no threshold): INT32_MAX for
// both aggregations, since box right keys are sign-flipped (kRightKeyFlip) and every right-key MIN is signed
constexpr uint32_t kNoRightKey = 0x7FFFFFFFu;

// One frame's guided slice pass into `keys`, left view only
sm::GuidedPass guided_slice_pass(const sm_handle* h, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch,
                                 int64_t fstride, int radius, int d_lo, int d_hi, int* keys) {
    sm::GuidedPass g{};
    g.left = dL;
    g.right = dR;
    g.W = W;
    g.H = H;
    g.pitch = pitch;
    g.frame_stride = fstride;
    g.batch = 1;
    g.radius = radius;
    g.d_lo = d_lo;
    g.d_hi = d_hi;
    g.eps = h->guided_eps;
    g.keys = keys;
    return g;
}

// The slice pass over [d_lo, d_hi) of frames already on the device (pitch `pitch`): left keys, and with
// `rkeys` the right view's keys from the same fused pass (its per-tile partials in the handle's rpart
// workspace).  Keys are [H][W]; no padding.  The box kernels and their workspaces are plan_box_pass's
// (bm_box_plan.h); a pass that takes no workspace stays outside the scope's ordering.
int slice_keys_pass(WsScope& ws, sm_handle* h, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch,
                    int radius, int d_lo, int d_hi, bool guided, uint32_t* keys, uint32_t* rkeys) {
    hipStream_t s = ws.stream();
    const int64_t P = (int64_t)W * H;
    if (guided) {
        sm::GuidedPass g =
            guided_slice_pass(h, dL, dR, W, H, pitch, P, radius, d_lo, d_hi, reinterpret_cast<int*>(keys));
        if (rkeys) {
            int rc = ws.get(h->rpart, sm::guided_right_partial_bytes(W, H, radius, d_hi - d_lo, 1), &g.gpart);
            if (rc) return rc;
            g.right_keys = reinterpret_cast<int*>(rkeys);
        }
        SM_HIP(sm::launch_guided(g, s));
        return SM_OK;
    }
    sm::MatchArgs a{};
    a.left = dL;
    a.right = dR;
    a.W = W;
    a.H = H;
    a.pitch = pitch;
    a.frame_stride = P;
    a.radius = radius;
    a.d_lo = d_lo;
    a.d_hi = d_hi;
    a.seed_key = seed_key(radius);
    a.thresh_key = seed_key(radius);
    a.keys = keys;
    // (right keys from the wide path are sign-flipped, kRightKeyFlip)
    const sm::BoxPlan plan =
        sm::plan_box_pass({W, H, pitch, radius, d_lo, d_hi, 1}, rkeys ? sm::RightWant::Keys : sm::RightWant::None);
    BoxRightOut ro;
    ro.keys = rkeys;
    return run_box_pass(ws, h, a, 1, plan, ro);
}

int slice_check(int d_lo, int d_hi) {
    if (d_lo < 0 || d_hi <= d_lo || d_hi > sm::kMaxDisp) return fail(SM_ERR_INVALID_ARG, "bad slice [%d,%d)", d_lo, d_hi);
    return SM_OK;
}

}  // namespace

namespace smh {

DslicePlan dslice_plan(int64_t P, int D, int n, int k, int H) {
    DslicePlan p;
    p.lo = (int)((int64_t)k * D / n);
    p.hi = (int)((int64_t)(k + 1) * D / n);
    p.chunk = (P + n - 1) / n;
    p.padded = p.chunk * n;
    p.rows_per = (H + n - 1) / n;
    p.row_lo = std::min(H, k * p.rows_per);
    p.row_hi = std::min(H, (k + 1) * p.rows_per);
    return p;
}

int dslice_check(const DsliceCfg& c, unsigned flags) {
    if (flags & SM_AGG_SGM)
        return fail(SM_ERR_INVALID_ARG, "d-slice mode: SM_AGG_SGM's recursion over d crosses the slices");
    if (flags & SM_COST_CENSUS)
        return fail(SM_ERR_INVALID_ARG, "d-slice mode: SM_COST_CENSUS is not built for d-slices (the AD cost only)");
    if ((flags & ~(unsigned)(SM_AGG_GUIDED | SM_LR_CHECK)) != 0u)
        return fail(SM_ERR_INVALID_ARG,
                    "d-slice mode: flags 0x%x (box or SM_AGG_GUIDED, optionally SM_LR_CHECK; no median, staged)", flags);
    if (c.guided) {
        const int rc = guided_radius_check(c.radius);
        if (rc) return rc;
    }
    if (c.lr && !c.guided &&
        sm::plan_box_pass({c.W, c.H, c.W, c.radius, 0, c.D, 1}, sm::RightWant::Keys).right == sm::BoxRight::Unsupported)
        return fail(SM_ERR_INVALID_ARG, "d-slice LR: box radius %d > %d needs the wide path (width <= %d)", c.radius,
                    sm::kMaxBoxRadius, sm::kMaxWideWidth);
    return SM_OK;
}

DsliceWs dslice_ws(uint8_t* base, const DslicePlan& p, int n, int W, bool lr) {
    DsliceWs w;
    w.slot = (int64_t)p.rows_per * W;
    size_t o = 0;
    auto take = [&](int64_t bytes) {
        uint8_t* at = base + o;
        o += align256((size_t)bytes);
        return at;
    };
    w.keys = reinterpret_cast<uint32_t*>(take(p.padded * 4));
    w.mine = reinterpret_cast<uint32_t*>(take(p.chunk * 4));
    w.mine8 = take(p.chunk);
    w.map = take(p.padded);
    w.gl = take(n * w.slot);
    w.gr = take(n * w.slot);
    w.rkeys = w.rmine = nullptr;
    w.rmine8 = w.rmap = nullptr;
    if (lr) {
        w.rkeys = reinterpret_cast<uint32_t*>(take(p.padded * 4));
        w.rmine = reinterpret_cast<uint32_t*>(take(p.chunk * 4));
        w.rmine8 = take(p.chunk);
        w.rmap = take(p.padded);
    }
    w.bytes = o;
    return w;
}

// Member k's rows of the pair into its slot of the gathered frames (host -> device, its own PCIe link).
int dslice_upload_rows(const DslicePlan& p, const DsliceWs& w, int k, const uint8_t* left, const uint8_t* right, int W,
                       int pitch, hipStream_t s) {
    const int nr = p.row_hi - p.row_lo;
    if (nr <= 0) return SM_OK;   // a member past the frame's last row contributes a pad slot only
    const int64_t off = (int64_t)p.row_lo * pitch;
    SM_HIP(copy2d(w.gl + k * w.slot, W, left + off, pitch, W, nr, hipMemcpyHostToDevice, s));
    SM_HIP(copy2d(w.gr + k * w.slot, W, right + off, pitch, W, nr, hipMemcpyHostToDevice, s));
    return SM_OK;
}

// Member-side key pass over its slice: keys[0, padded) (and rkeys with LR) on the scope's stream from the frames
// already on the device (dL / dR, pitch W).
int dslice_keys(WsScope& ws, sm_handle* h, const DslicePlan& p, const DsliceCfg& c, const uint8_t* dL,
                const uint8_t* dR, uint32_t* keys, uint32_t* rkeys) {
    hipStream_t s = ws.stream();
    const int64_t P = c.P();
    const uint32_t none = dslice_none_key(c.radius, c.guided), rnone = kNoRightKey;
    if (p.padded > P) SM_HIP(hipMemsetD32Async(keys + P, (int)none, (size_t)(p.padded - P), s));
    if (rkeys && p.padded > P) SM_HIP(hipMemsetD32Async(rkeys + P, (int)rnone, (size_t)(p.padded - P), s));
    if (p.hi <= p.lo) {   // more members than disparities: an empty slice contributes "no match"
        SM_HIP(hipMemsetD32Async(keys, (int)none, (size_t)P, s));
        if (rkeys) SM_HIP(hipMemsetD32Async(rkeys, (int)rnone, (size_t)P, s));
        return SM_OK;
    }
    return slice_keys_pass(ws, h, dL, dR, c.W, c.H, c.W, c.radius, p.lo, p.hi, c.guided, keys, rkeys);
}

// A reduced key chunk -> uint8 (the Device.cu:37 threshold, after the MIN); a right-view chunk -> its d field
int dslice_finalise(const uint32_t* mine, int64_t chunk, int radius, bool guided, uint8_t* mine8, hipStream_t s) {
    if (guided)
        SM_HIP(sm::launch_guided_keys_to_disp(reinterpret_cast<const int*>(mine), (int)chunk, 1, mine8, (int)chunk, s));
    else
        SM_HIP(sm::launch_keys_to_disp(mine, (int)chunk, 1, seed_key(radius), mine8, (int)chunk, s));
    return SM_OK;
}

}  // namespace smh

extern "C" {

SM_API int sm_slice_keys_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                int pitch, int radius, int d_lo, int d_hi, uint32_t* d_keys, void* stream) {
    int rc = check_geometry(h, width, height, pitch, radius, d_hi > 0 ? d_hi : 1);
    if (rc) return rc;
    rc = speckle_refuse(h, "a slice-key call", "keys are no map; filter the combined map (sm_speckle_filter_device)");
    if (rc) return rc;
    rc = fill_refuse(h, "a slice-key call", "keys are no map; fill the combined map (sm_fill_invalid_device)");
    if (rc) return rc;
    rc = pairs_refuse(h, 0u, "a slice-key call");
    if (rc) return rc;
    rc = slice_check(d_lo, d_hi);
    if (rc) return rc;
    if (!d_left || !d_right || !d_keys) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    SM_HIP(hipSetDevice(h->device));
    WsScope ws(h, stream_of(stream));
    return slice_keys_pass(ws, h, d_left, d_right, width, height, pitch, radius, d_lo, d_hi, false, d_keys, nullptr);
}

SM_API int sm_keys_to_disp_device(sm_handle* h, const uint32_t* d_keys, int width, int height, int radius,
                                  uint8_t* d_disp, int out_pitch, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_keys || !d_disp || width <= 0 || height <= 0 || out_pitch < width || radius < 0)
        return fail(SM_ERR_INVALID_ARG, "bad keys_to_disp arguments");
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_keys_to_disp(d_keys, width, height, seed_key(radius), d_disp, out_pitch, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_guided_slice_keys_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width,
                                       int height, int pitch, int radius, int d_lo, int d_hi, int32_t* d_keys,
                                       void* stream) {
    int rc = check_geometry(h, width, height, pitch, radius, d_hi > 0 ? d_hi : 1);
    if (rc) return rc;
    rc = speckle_refuse(h, "a slice-key call", "keys are no map; filter the combined map (sm_speckle_filter_device)");
    if (rc) return rc;
    rc = fill_refuse(h, "a slice-key call", "keys are no map; fill the combined map (sm_fill_invalid_device)");
    if (rc) return rc;
    rc = pairs_refuse(h, 0u, "a slice-key call");
    if (rc) return rc;
    rc = guided_radius_check(radius);
    if (rc) return rc;
    rc = slice_check(d_lo, d_hi);
    if (rc) return rc;
    if (!d_left || !d_right || !d_keys) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    SM_HIP(hipSetDevice(h->device));
    const sm::GuidedPass g =
        guided_slice_pass(h, d_left, d_right, width, height, pitch, (int64_t)pitch * height, radius, d_lo, d_hi, d_keys);
    SM_HIP(sm::launch_guided(g, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_guided_keys_to_disp_device(sm_handle* h, const int32_t* d_keys, int width, int height,
                                         uint8_t* d_disp, int out_pitch, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_keys || !d_disp || width <= 0 || height <= 0 || out_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad guided_keys_to_disp arguments");
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_guided_keys_to_disp(d_keys, width, height, d_disp, out_pitch, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_slice_keys_lr_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                   int pitch, int radius, int d_lo, int d_hi, unsigned flags, void* d_left_keys,
                                   void* d_right_keys, void* stream) {
    int rc = check_geometry(h, width, height, pitch, radius, d_hi > 0 ? d_hi : 1);
    if (rc) return rc;
    rc = speckle_refuse(h, "a slice-key call", "keys are no map; filter the combined map (sm_speckle_filter_device)");
    if (rc) return rc;
    rc = fill_refuse(h, "a slice-key call", "keys are no map; fill the combined map (sm_fill_invalid_device)");
    if (rc) return rc;
    rc = pairs_refuse(h, flags, "a slice-key call");
    if (rc) return rc;
    if (flags & SM_AGG_SGM)
        return fail(SM_ERR_INVALID_ARG, "slice LR keys: SM_AGG_SGM's recursion over d crosses the slices");
    if (flags & SM_COST_CENSUS)
        return fail(SM_ERR_INVALID_ARG, "slice LR keys: SM_COST_CENSUS is not built for d-slices (the AD cost only)");
    if ((flags & ~(unsigned)SM_AGG_GUIDED) != 0u)
        return fail(SM_ERR_INVALID_ARG, "slice LR keys: flags 0x%x (SM_AGG_BOX or SM_AGG_GUIDED)", flags);
    const bool guided = (flags & SM_AGG_GUIDED) != 0;
    // (whether box right keys exist does not depend on the slice, which is checked below)
    if (guided ? radius > sm::kMaxFastRadius
               : sm::plan_box_pass({width, height, pitch, radius, 0, 1, 1}, sm::RightWant::Keys).right ==
                     sm::BoxRight::Unsupported)
        return fail(SM_ERR_INVALID_ARG, "slice LR keys: radius %d > %d%s", radius,
                    guided ? sm::kMaxFastRadius : sm::kMaxBoxRadius,
                    guided ? "" : " outside the wide path (width 4..4096, frame < 2^31 bytes)");
    rc = slice_check(d_lo, d_hi);
    if (rc) return rc;
    if (!d_left || !d_right || !d_left_keys || !d_right_keys) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    if ((int64_t)width * height > (int64_t)h->max_w * h->max_h)
        return fail(SM_ERR_CAPACITY, "frame %dx%d exceeds handle capacity", width, height);
    SM_HIP(hipSetDevice(h->device));
    WsScope ws(h, stream_of(stream));   // the right view's partials (or the wide path's planes) are handle workspace
    return slice_keys_pass(ws, h, d_left, d_right, width, height, pitch, radius, d_lo, d_hi, guided,
                           static_cast<uint32_t*>(d_left_keys), static_cast<uint32_t*>(d_right_keys));
}

SM_API int sm_right_keys_to_disp_device(sm_handle* h, const void* d_keys, int64_t n, uint8_t* d_disp, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_keys || !d_disp || n < 0) return fail(SM_ERR_INVALID_ARG, "bad right_keys_to_disp arguments");
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_keys_low_byte(static_cast<const uint32_t*>(d_keys), n, d_disp, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_dslice_plan(int64_t pixels, int num_disp, int members, int member, int* d_lo, int* d_hi,
                          int64_t* chunk, int64_t* padded_pixels) {
    if (pixels <= 0 || num_disp < 1 || members < 1 || member < 0 || member >= members)
        return fail(SM_ERR_INVALID_ARG, "d-slice plan: pixels %lld, num_disp %d, member %d of %d", (long long)pixels,
                    num_disp, member, members);
    const DslicePlan p = dslice_plan(pixels, num_disp, members, member);
    if (d_lo) *d_lo = p.lo;
    if (d_hi) *d_hi = p.hi;
    if (chunk) *chunk = p.chunk;
    if (padded_pixels) *padded_pixels = p.padded;
    return SM_OK;
}

SM_API int sm_dslice_rehearse_u8(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                                 int pitch, int radius, int num_disp, unsigned flags, int members, uint8_t* disp_out,
                                 int out_pitch) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!left || !right || !disp_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    if (out_pitch < width) return fail(SM_ERR_INVALID_ARG, "out_pitch %d < width %d", out_pitch, width);
    if (members < 1 || members > 64) return fail(SM_ERR_INVALID_ARG, "members %d out of [1, 64]", members);
    rc = speckle_refuse(h, "the d-slice rehearsal", "the d-slice calls do not run it");
    if (rc) return rc;
    rc = fill_refuse(h, "the d-slice rehearsal", "the d-slice calls do not run it");
    if (rc) return rc;
    rc = pairs_refuse(h, flags, "the d-slice rehearsal");
    if (rc) return rc;
    const bool guided = (flags & SM_AGG_GUIDED) != 0;
    const DsliceCfg cfg{width, height, radius, num_disp, guided, (flags & SM_LR_CHECK) != 0};
    rc = dslice_check(cfg, flags);
    if (rc) return rc;
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    const int64_t P = (int64_t)width * height;
    const int n = members;
    const DslicePlan p0 = dslice_plan(P, num_disp, n, 0, height);
    // workspace: one member's layout (its gathered frames are the all-gather's result, shared by every
    // rehearsed member) followed by the other members' key maps [n - 1][padded] (and right key maps)
    const size_t member_bytes = dslice_ws(nullptr, p0, n, width, cfg.lr).bytes;
    const int nk = cfg.lr ? 2 : 1;
    SM_HIP(hipSetDevice(h->device));
    rc = h->dsl.reserve(member_bytes + (size_t)(nk * (n - 1) * p0.padded * 4));
    if (rc) return rc;
    hipStream_t s = h->stream;
    const DsliceWs w = dslice_ws(h->dsl.p, p0, n, width, cfg.lr);
    uint32_t* extra = reinterpret_cast<uint32_t*>(h->dsl.p + member_bytes);
    auto keys_of = [&](int k) { return k == 0 ? w.keys : extra + (int64_t)(k - 1) * p0.padded; };
    auto rkeys_of = [&](int k) {
        return !cfg.lr ? nullptr : k == 0 ? w.rkeys : extra + (int64_t)(n - 1 + k - 1) * p0.padded;
    };
    uint8_t* map = w.map;
    // the row-split upload: member k's rows into slot k of the gathered frames, which is where the
    // in-place all-gather leaves them on every member; the pad rows of the last slots are never read
    for (int k = 0; k < n; ++k) {
        rc = dslice_upload_rows(dslice_plan(P, num_disp, n, k, height), w, k, left, right, width, pitch, s);
        if (rc) return rc;
    }
    {
        WsScope ws(h, s);
        for (int k = 0; k < n && !rc; ++k)   // every member's key pass, into its own buffers
            rc = dslice_keys(ws, h, dslice_plan(P, num_disp, n, k, height), cfg, w.gl, w.gr, keys_of(k), rkeys_of(k));
        if (rc) return rc;
    }
    // the reduce-scatter's MIN (into member 0's buffers: left keys signed for guided, unsigned for box; right
    // keys signed for both, box ones being sign-flipped), then each member's chunk finalised into slot k
    for (int k = 1; k < n; ++k) {
        if (guided)
            SM_HIP(sm::launch_min_keys(reinterpret_cast<int*>(w.keys), reinterpret_cast<const int*>(keys_of(k)),
                                       p0.padded, s));
        else
            SM_HIP(sm::launch_min_keys_u32(w.keys, keys_of(k), p0.padded, s));
        if (cfg.lr)
            SM_HIP(sm::launch_min_keys(reinterpret_cast<int*>(w.rkeys), reinterpret_cast<const int*>(rkeys_of(k)),
                                       p0.padded, s));
    }
    for (int k = 0; k < n; ++k) {
        const DslicePlan p = dslice_plan(P, num_disp, n, k, height);
        rc = dslice_finalise(w.keys + k * p.chunk, p.chunk, radius, guided, map + k * p.chunk, s);
        if (rc) return rc;
        if (cfg.lr) SM_HIP(sm::launch_keys_low_byte(w.rkeys + k * p.chunk, p.chunk, w.rmap + k * p.chunk, s));
    }
    if (cfg.lr)
        SM_HIP(sm::launch_lr_check(map, width, P, w.rmap, width, P, 0, width, height, 1, map, width, P, nullptr, nullptr,
                                   width, P, s));
    SM_HIP(copy2d(disp_out, out_pitch, map, width, width, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

}  // extern "C"
