// sm_capi_volume.hip — the C ABI's passes that keep a cost volume: SM_AGG_SGM, SM_COST_CENSUS and the sub-pixel
// calls, their argument rules and workspace sizes.
#include "sm_handle.h"

namespace smh {

// ---- SM_COST_CENSUS (bm_census.hip) ----
// The argument rules of the census cost, for box and SGM alike: every entry point that takes the flag goes
// through here (or through sgm_check, which starts with it).
int census_check(int width, int radius, unsigned flags) {
    if (flags & (SM_AGG_GUIDED | SM_STAGED | SM_DEVICE_CU_GRID))
        return fail(SM_ERR_INVALID_ARG,
                    "SM_COST_CENSUS does not combine with SM_AGG_GUIDED, SM_STAGED or SM_DEVICE_CU_GRID (flags 0x%x)",
                    flags);
    if (radius < 0 || radius > sm::kMaxFastRadius)
        return fail(SM_ERR_INVALID_ARG, "SM_COST_CENSUS: radius %d out of [0, %d] (the u16 cost volume)", radius,
                    sm::kMaxFastRadius);
    if (width < 1 || width > 4096) return fail(SM_ERR_INVALID_ARG, "SM_COST_CENSUS: width %d out of [1, 4096]", width);
    return SM_OK;
}

// ---- SM_AGG_SGM (bm_sgm.hip) ----
// The argument rules of sm_sgm_check: every entry point that takes the flag goes through here.  With
// SM_COST_CENSUS in `flags` the cost is at most 62 per pixel instead of 255, and the auto penalties follow it.
int sgm_check(int width, int radius, unsigned flags, int p1, int p2, int* p1_out, int* p2_out) {
    const bool census = (flags & SM_COST_CENSUS) != 0;
    if (census) {
        const int rc = census_check(width, radius, flags);
        if (rc) return rc;
    }
    if (flags & (SM_AGG_GUIDED | SM_STAGED | SM_DEVICE_CU_GRID))
        return fail(SM_ERR_INVALID_ARG,
                    "SM_AGG_SGM does not combine with SM_AGG_GUIDED, SM_STAGED or SM_DEVICE_CU_GRID (flags 0x%x)", flags);
    if (radius < 0 || radius > sm::kMaxFastRadius)
        return fail(SM_ERR_INVALID_ARG, "SM_AGG_SGM: radius %d out of [0, %d] (the u16 SAD volume)", radius,
                    sm::kMaxFastRadius);
    if (width < 1 || width > 4096) return fail(SM_ERR_INVALID_ARG, "SM_AGG_SGM: width %d out of [1, 4096]", width);
    if (p1 < 0 || p2 < 0) return fail(SM_ERR_INVALID_ARG, "SM_AGG_SGM: negative penalty (P1 %d, P2 %d)", p1, p2);
    const int win2 = (2 * radius + 1) * (2 * radius + 1);
    if (p1 == 0) p1 = (census ? 10 : 8) * win2;
    if (p2 == 0) p2 = (census ? 120 : 32) * win2;
    if (p1 > p2) return fail(SM_ERR_INVALID_ARG, "SM_AGG_SGM: P1 %d > P2 %d", p1, p2);
    const int cmax = census ? 62 : 255;   // the largest cost of one pixel
    if (cmax * win2 + p2 > 65535)
        return fail(SM_ERR_INVALID_ARG, "SM_AGG_SGM: %d * win^2 + P2 = %d exceeds 65535 (16-bit path costs) at radius %d",
                    cmax, cmax * win2 + p2, radius);
    if (p1_out) *p1_out = p1;
    if (p2_out) *p2_out = p2;
    return SM_OK;
}

// ---- SM_PAIRS_IN_VIEW and SM_PARAM_MIN_DISP ----
int pairs_check(const sm_handle* h, unsigned flags, int num_disp, bool subpix, sm::Pairs* out) {
    sm::Pairs pr;
    if (out) *out = pr;
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!(flags & SM_PAIRS_IN_VIEW)) {
        if (h->min_disp > 0)
            return fail(SM_ERR_INVALID_ARG,
                        "SM_PARAM_MIN_DISP %d needs SM_PAIRS_IN_VIEW in the call's flags (0x%x): the reference's pair "
                        "rule starts at d = 0", h->min_disp, flags);
        return SM_OK;
    }
    if (flags & (SM_AGG_GUIDED | SM_STAGED | SM_DEVICE_CU_GRID))
        return fail(SM_ERR_INVALID_ARG,
                    "SM_PAIRS_IN_VIEW does not combine with SM_AGG_GUIDED, SM_STAGED or SM_DEVICE_CU_GRID (flags "
                    "0x%x): they are the reference-parity paths", flags);
    if (!subpix && !(flags & (SM_AGG_SGM | SM_COST_CENSUS)))
        return fail(SM_ERR_INVALID_ARG,
                    "SM_PAIRS_IN_VIEW: the 8-bit AD SM_AGG_BOX call is the reference-parity path (its fused kernels "
                    "and its threshold); the flag takes SM_AGG_SGM, SM_COST_CENSUS or a sub-pixel call (flags 0x%x)",
                    flags);
    pr.in_view = 1;
    pr.d0 = h->min_disp;
    const int limit = subpix ? 4095 : 255;
    if (pr.d0 + num_disp - 1 > limit)
        return fail(SM_ERR_INVALID_ARG,
                    "SM_PARAM_MIN_DISP %d + num_disp %d - 1 = %d exceeds %d, the largest disparity of %s", pr.d0,
                    num_disp, pr.d0 + num_disp - 1, limit, subpix ? "a 1/16-px map" : "an 8-bit map");
    if (out) *out = pr;
    return SM_OK;
}

int pairs_refuse(const sm_handle* h, unsigned flags, const char* call) {
    if (flags & SM_PAIRS_IN_VIEW)
        return fail(SM_ERR_INVALID_ARG, "%s cannot honour SM_PAIRS_IN_VIEW (flags 0x%x): it keeps no whole cost volume",
                    call, flags);
    if (h && h->min_disp > 0)
        return fail(SM_ERR_INVALID_ARG,
                    "%s cannot honour SM_PARAM_MIN_DISP %d: it runs the reference's pair rule, d from 0", call,
                    h->min_disp);
    return SM_OK;
}

// Every pass that keeps a cost volume, over `batch` frames, one frame after another through the volume workspace
// (volume_layout):
//   cost volume (AD, or the census words of both frames and their Hamming volume) -> box sums (u16)
//   -> with SGM the zeroed S and the paths' sums over it (the handle's sgm_paths: four, or eight with the diagonals)
//   -> one winner-takes-all over S (SGM) or the u16 costs: 8-bit maps with the right view's keys and their low
//      byte, or subpix_wta_kernel (-> LR check; the two views' d0 of the check take the right-keys region), or with
//      SM_PARAM_SUBPIX_MEDIAN subpix_wta_kernel into planes of the `lr` workspace -> median16 of both views -> the
//      check on the filtered maps (run_subpix_median).
// pr (pairs_check): with SM_PAIRS_IN_VIEW plane k of every volume is d = pr.d0 + k, the cost launchers read the right
// image pr.d0 columns further left, the paths and the WTA take the in-view prefix, and pr.d0 is added where the keys
// become maps.  The shapes, the workspace and the launches are the same under either rule.
int run_volume(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
               int64_t fstride, int radius, int D, bool sgm, bool census, int p1, int p2, const sm::Pairs& pr,
               const VolumeOut& o) {
    const bool subpix = o.disp16 != nullptr;
    const int64_t P = (int64_t)W * H;
    const VolumeLayout w = volume_layout(P, D, sgm, census);
    hipStream_t s = ws.stream();
    uint8_t* vol = nullptr;
    const int rc = ws.get(h->vol, w.bytes, &vol);   // the only allocation of the pass, before any launch
    if (rc) {
        const std::string why = g_err;
        if (subpix) return fail(rc, "sub-pixel: no %zu-byte workspace for %dx%d D=%d: %s", w.bytes, W, H, D, why.c_str());
        return fail(rc, "%s: no %zu-byte workspace for %dx%d D=%d (%s): %s", sgm ? "SM_AGG_SGM" : "SM_COST_CENSUS",
                    w.bytes, W, H, D, census ? "sm_census_workspace_bytes" : "sm_sgm_workspace_bytes", why.c_str());
    }
    uint32_t* S = reinterpret_cast<uint32_t*>(vol);
    uint16_t* cost = reinterpret_cast<uint16_t*>(vol + w.sad);
    uint32_t* rkeys = o.right_map ? reinterpret_cast<uint32_t*>(vol + w.rkeys) : nullptr;
    uint64_t* cl = reinterpret_cast<uint64_t*>(vol + w.cl);
    uint64_t* cr = reinterpret_cast<uint64_t*>(vol + w.cr);
    const uint32_t win = 2u * (uint32_t)radius + 1u;
    const uint32_t invalid_from = sgm || census ? 0u : 50u * win * win;   // Device.cu:37, the AD box path alone
    const int right_pairs = sgm || census ? 1 : 2;
    // SM_PARAM_SUBPIX_MEDIAN: the views' unfiltered maps go through planes of the `lr` workspace, taken here, before
    // the first launch, and reused frame after frame
    const int med = subpix ? h->subpix_median : 0;
    SubpixMedianWs mw;
    if (med) {
        uint8_t* planes = nullptr;
        const int rc2 = ws.get(h->lr, subpix_median_bytes(P, o.lr, o.right16 != nullptr), &planes);
        if (rc2) return rc2;
        mw = subpix_median_ws(planes, P, o.lr, o.right16 != nullptr);
    }
    for (int f = 0; f < batch; ++f) {
        const uint8_t* Lf = L + f * fstride;
        const uint8_t* Rf = R + f * fstride;
        if (census) {
            SM_HIP(sm::launch_census(Lf, W, H, pitch, cl, s));
            SM_HIP(sm::launch_census(Rf, W, H, pitch, cr, s));
            SM_HIP(sm::launch_census_volume(cl, cr, W, H, D, vol, s, pr.d0));
        } else {
            SM_HIP(sm::launch_ad_volume(Lf, Rf, W, H, pitch, fstride, 1, D, vol, P * D, s, pr.d0));
        }
        SM_HIP(sm::launch_box_sad_volume(vol, W, H, radius, D, cost, s));
        if (sgm) {
            SM_HIP(hipMemsetAsync(S, 0, (size_t)(4 * P * D), s));
            SM_HIP(sm::launch_sgm_paths(cost, W, H, D, p1, p2, h->sgm_paths, pr, S, s));
        }
        if (subpix) {
            uint16_t* out = o.disp16 + f * o.ostride;
            uint16_t* rout = o.right16 ? o.right16 + f * P : nullptr;
            uint8_t* mout = o.mask ? o.mask + f * P : nullptr;
            uint8_t* scratch = vol + w.rkeys;
            if (med) {   // both views unchecked into the planes, then median -> check on the filtered maps -> mask
                if (sgm)
                    SM_HIP(sm::launch_subpix_wta_u32(S, W, H, D, invalid_from, h->uniqueness, right_pairs, false,
                                                     mw.left, W, mw.right, nullptr, nullptr, s, pr));
                else
                    SM_HIP(sm::launch_subpix_wta_u16(cost, W, H, D, invalid_from, h->uniqueness, right_pairs, false,
                                                     mw.left, W, mw.right, nullptr, nullptr, s, pr));
                const int rc2 = run_subpix_median(s, mw, W, H, med, out, o.opitch, rout, o.lr, mout);
                if (rc2) return rc2;
                continue;
            }
            if (sgm)
                SM_HIP(sm::launch_subpix_wta_u32(S, W, H, D, invalid_from, h->uniqueness, right_pairs, o.lr, out,
                                                 o.opitch, rout, mout, scratch, s, pr));
            else
                SM_HIP(sm::launch_subpix_wta_u16(cost, W, H, D, invalid_from, h->uniqueness, right_pairs, o.lr, out,
                                                 o.opitch, rout, mout, scratch, s, pr));
            continue;
        }
        if (sgm)
            SM_HIP(sm::launch_sgm_wta(S, W, H, D, pr, o.lmap + f * o.lstride, o.lpitch, rkeys, s));
        else
            SM_HIP(sm::launch_cost_wta_u16(cost, W, H, D, pr, o.lmap + f * o.lstride, o.lpitch, rkeys, s));
        if (o.right_map) SM_HIP(sm::launch_keys_low_byte(rkeys, P, o.right_map + f * P, s, pr.in_view, pr.d0));
    }
    return SM_OK;
}

// ---- SM_AGG_GUIDED in the sub-pixel calls (bm_guided.hip: launch_guided_volume) ----
// Per frame: the guided costs of every d in one pass, biased to uint32 V = trunc(q 2^14) + 2^23 < 2^24, into the head
// of the volume workspace; then run_volume's sub-pixel step on V with the 8-bit guided call's rule: left view
// d <= min(D - 1, W - x) and invalid where q >= 50 (V >= kGuidedInvalidFrom), right view V_R(u, d) = V(u + d, d)
// over u + d < W without a threshold, no uniqueness (subpix_check).  The right view's walk crosses entries with
// d > W - x, which hold the largest cost (bm_guided_plan.h).
int run_guided_subpix(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
                      int64_t fstride, int radius, int D, const VolumeOut& o) {
    const int64_t P = (int64_t)W * H;
    const VolumeLayout w = guided_volume_layout(P, D);
    hipStream_t s = ws.stream();
    uint8_t* vol = nullptr;
    const int rc = ws.get(h->vol, w.bytes, &vol);   // before any launch
    if (rc) {
        const std::string why = g_err;
        return fail(rc, "sub-pixel SM_AGG_GUIDED: no %zu-byte workspace for %dx%d D=%d (sm_guided_workspace_bytes): %s",
                    w.bytes, W, H, D, why.c_str());
    }
    const int med = h->subpix_median;
    SubpixMedianWs mw;
    if (med) {
        uint8_t* planes = nullptr;
        const int rc2 = ws.get(h->lr, subpix_median_bytes(P, o.lr, o.right16 != nullptr), &planes);
        if (rc2) return rc2;
        mw = subpix_median_ws(planes, P, o.lr, o.right16 != nullptr);
    }
    const uint32_t* V = reinterpret_cast<const uint32_t*>(vol);
    const sm::Pairs pr;
    for (int f = 0; f < batch; ++f) {
        const sm::GuidedVolumePass g{L + f * fstride, R + f * fstride, W, H, pitch, radius, D, h->guided_eps, vol, true};
        SM_HIP(sm::launch_guided_volume(g, s));
        uint16_t* out = o.disp16 + f * o.ostride;
        uint16_t* rout = o.right16 ? o.right16 + f * P : nullptr;
        uint8_t* mout = o.mask ? o.mask + f * P : nullptr;
        if (med) {   // both views unchecked into the planes, then median -> check on the filtered maps -> mask
            SM_HIP(sm::launch_subpix_wta_u32(V, W, H, D, sm::kGuidedInvalidFrom, 0, 2, false, mw.left, W, mw.right,
                                             nullptr, nullptr, s, pr));
            const int rc2 = run_subpix_median(s, mw, W, H, med, out, o.opitch, rout, o.lr, mout);
            if (rc2) return rc2;
            continue;
        }
        SM_HIP(sm::launch_subpix_wta_u32(V, W, H, D, sm::kGuidedInvalidFrom, 0, 2, o.lr, out, o.opitch, rout, mout,
                                         vol + w.rkeys, s, pr));
    }
    return SM_OK;
}

}  // namespace smh

using namespace smh;

namespace {

// ---- sub-pixel maps (bm_subpix.hip) ----
// The argument rules of the sub-pixel matching calls, before the device is touched; the resolved SGM penalties
// come back through p1_out / p2_out.
int subpix_check(const sm_handle* h, int width, int height, int pitch, int radius, int num_disp, unsigned flags,
                 int* p1_out, int* p2_out, sm::Pairs* pr) {
    // what the sub-pixel calls cannot do comes first and needs no handle; then the common argument checks
    if (flags & SM_MEDIAN)
        return fail(SM_ERR_INVALID_ARG,
                    "sub-pixel: SM_MEDIAN is not supported (the flag is the 8-bit ctmf median; the 1/16-px maps take "
                    "the 16-bit median of SM_PARAM_SUBPIX_MEDIAN)");
    // SM_AGG_GUIDED builds its volume only on a handle that asked for it (SM_PARAM_GUIDED_SUBPIX); otherwise, and
    // without a handle, it is refused as before the volume kernel existed
    const bool guided = (flags & SM_AGG_GUIDED) != 0 && h && h->guided_subpix;
    if (guided && (flags & (SM_STAGED | SM_DEVICE_CU_GRID)))
        return fail(SM_ERR_INVALID_ARG,
                    "sub-pixel: SM_AGG_GUIDED does not combine with SM_STAGED or SM_DEVICE_CU_GRID (flags 0x%x)", flags);
    if ((flags & (SM_STAGED | SM_DEVICE_CU_GRID)) || ((flags & SM_AGG_GUIDED) && !guided))
        return fail(SM_ERR_INVALID_ARG,
                    "sub-pixel: SM_AGG_GUIDED, SM_STAGED and SM_DEVICE_CU_GRID keep no cost volume to interpolate "
                    "(flags 0x%x; SM_AGG_GUIDED builds one per frame on a handle with SM_PARAM_GUIDED_SUBPIX = 1)", flags);
    if (radius > sm::kMaxFastRadius)
        return fail(SM_ERR_INVALID_ARG, "sub-pixel: radius %d out of [0, %d] (the u16 cost volume)", radius,
                    sm::kMaxFastRadius);
    if (width > 4096) return fail(SM_ERR_INVALID_ARG, "sub-pixel: width %d out of [1, 4096]", width);
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    rc = pairs_check(h, flags, num_disp, true, pr);
    if (rc) return rc;
    if (flags & SM_AGG_SGM) return sgm_check(width, radius, flags, h->sgm_p1, h->sgm_p2, p1_out, p2_out);
    if (flags & SM_COST_CENSUS) return census_check(width, radius, flags);
    // SM_AGG_GUIDED: in-view pairs, a minimum disparity, the census cost and SGM have been refused above
    if (guided && h->uniqueness > 0)
        return fail(SM_ERR_INVALID_ARG,
                    "sub-pixel: SM_PARAM_UNIQUENESS %d does not combine with SM_AGG_GUIDED (flags 0x%x): the ratio "
                    "test has no meaning on a cost that can be negative", h->uniqueness, flags);
    return SM_OK;
}

// The sub-pixel calls' pass by aggregation: the guided volume, or run_volume
int run_subpix(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
               int64_t fstride, int radius, int D, unsigned flags, int p1, int p2, const sm::Pairs& pr,
               const VolumeOut& o) {
    if (flags & SM_AGG_GUIDED) return run_guided_subpix(ws, h, L, R, W, H, pitch, batch, fstride, radius, D, o);
    return run_volume(ws, h, L, R, W, H, pitch, batch, fstride, radius, D, (flags & SM_AGG_SGM) != 0,
                      (flags & SM_COST_CENSUS) != 0, p1, p2, pr, o);
}

// run_volume's last step for the sub-pixel calls: 1/16-px maps, the LR check with SM_LR_CHECK in `flags`
VolumeOut subpix_out(uint16_t* disp16, int pitch, int64_t stride, uint16_t* right16, uint8_t* mask, unsigned flags) {
    VolumeOut o;
    o.disp16 = disp16;
    o.opitch = pitch;
    o.ostride = stride;
    o.right16 = right16;
    o.mask = mask;
    o.lr = (flags & SM_LR_CHECK) != 0;
    return o;
}

// The handle's speckle filter as the sub-pixel calls' last step: on the 1/16-px left map and the mask, regions
// joined within 16 * range, as StereoSGBM's speckleRange on its 1/16-px map; and after it the handle's row fill, on
// the 1/16-px left map alone (whole 16-bit values)
int subpix_speckle(WsScope& ws, sm_handle* h, uint16_t* disp16, int W, int H, int pitch, int batch, int64_t stride,
                   uint8_t* mask) {
    if (h->speckle_size != 0) {
        if (!sm::speckle_pass_ok(W, H, batch))
            return fail(SM_ERR_INVALID_ARG, "speckle filter: frame %dx%d too large", W, H);
        const int rc = run_speckle(ws, h, disp16, 2, W, H, pitch, batch, stride, h->speckle_size,
                                   16 * h->speckle_range, mask);
        if (rc) return rc;
    }
    return h->fill_gap == 0 ? SM_OK : run_fill(ws.stream(), disp16, 2, W, H, pitch, batch, stride, h->fill_gap);
}

}  // namespace

extern "C" {

SM_API int sm_sgm_check(int width, int radius, unsigned flags, int p1, int p2, int* p1_out, int* p2_out) {
    return sgm_check(width, radius, flags, p1, p2, p1_out, p2_out);
}

SM_API int sm_sgm_workspace_bytes(int width, int height, int num_disp, int radius, int p2, size_t* bytes) {
    if (!bytes) return fail(SM_ERR_INVALID_ARG, "null bytes pointer");
    *bytes = 0;
    if (height < 1) return fail(SM_ERR_INVALID_ARG, "bad frame height %d", height);
    if (num_disp < 1 || num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "num_disp %d out of [1,%d]", num_disp, sm::kMaxDisp);
    const int rc = sgm_check(width, radius, SM_AGG_SGM, 0, p2, nullptr, nullptr);
    if (rc) return rc;
    *bytes = volume_layout((int64_t)width * height, num_disp, true, false).bytes;
    return SM_OK;
}

SM_API int sm_census_workspace_bytes(int width, int height, int num_disp, int radius, unsigned flags, size_t* bytes) {
    if (!bytes) return fail(SM_ERR_INVALID_ARG, "null bytes pointer");
    *bytes = 0;
    if (height < 1) return fail(SM_ERR_INVALID_ARG, "bad frame height %d", height);
    if (num_disp < 1 || num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "num_disp %d out of [1,%d]", num_disp, sm::kMaxDisp);
    flags |= SM_COST_CENSUS;
    const bool sgm = (flags & SM_AGG_SGM) != 0;
    const int rc = sgm ? sgm_check(width, radius, flags, 0, 0, nullptr, nullptr) : census_check(width, radius, flags);
    if (rc) return rc;
    *bytes = volume_layout((int64_t)width * height, num_disp, sgm, true).bytes;
    return SM_OK;
}

// ---- the guided cost volume (bm_guided.hip: launch_guided_volume) ----
namespace {
// what both volume calls check before the device is touched: the slice-key call's geometry and radii
int guided_volume_check(const sm_handle* h, int width, int height, int pitch, int radius, int num_disp) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    rc = pairs_refuse(h, 0u, "the guided volume call");
    if (rc) return rc;
    return guided_radius_check(radius);
}
}  // namespace

SM_API int sm_guided_workspace_bytes(int width, int height, int num_disp, int radius, size_t* bytes) {
    if (!bytes) return fail(SM_ERR_INVALID_ARG, "null bytes pointer");
    *bytes = 0;
    if (width < 1 || width > 4096) return fail(SM_ERR_INVALID_ARG, "sub-pixel SM_AGG_GUIDED: width %d out of [1, 4096]", width);
    if (height < 1) return fail(SM_ERR_INVALID_ARG, "bad frame height %d", height);
    if (num_disp < 1 || num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "num_disp %d out of [1,%d]", num_disp, sm::kMaxDisp);
    if (radius < 0) return fail(SM_ERR_INVALID_ARG, "radius %d out of [0, %d]", radius, sm::kMaxGuidedRadius);
    const int rc = guided_radius_check(radius);
    if (rc) return rc;
    *bytes = guided_volume_layout((int64_t)width * height, num_disp).bytes;
    return SM_OK;
}

SM_API int sm_guided_volume_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                   int pitch, int radius, int num_disp, int32_t* d_vol, void* stream) {
    const int rc = guided_volume_check(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!d_left || !d_right || !d_vol) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    SM_HIP(hipSetDevice(h->device));
    const sm::GuidedVolumePass g{d_left, d_right, width, height, pitch, radius, num_disp, h->guided_eps, d_vol, false};
    SM_HIP(sm::launch_guided_volume(g, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_guided_volume_i32(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                                int pitch, int radius, int num_disp, int32_t* vol_out) {
    int rc = guided_volume_check(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!left || !right || !vol_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t need = sm::guided_volume_bytes(width, height, num_disp);
    WsScope ws(h, s);
    uint8_t* vol = nullptr;
    rc = ws.get(h->vol, need, &vol);
    if (rc) return rc;
    rc = upload_pair(h, left, right, width, height, pitch, s);
    if (rc) return rc;
    const sm::GuidedVolumePass g{h->d_left, h->d_right, width, height, width, radius, num_disp, h->guided_eps, vol, false};
    SM_HIP(sm::launch_guided_volume(g, s));
    SM_HIP(hipMemcpyAsync(vol_out, vol, need, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

SM_API int sm_match_subpix_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                  int pitch, int batch, int64_t frame_stride, int radius, int num_disp, unsigned flags,
                                  uint16_t* d_disp16, int out_pitch, int64_t out_frame_stride, uint16_t* d_right16,
                                  uint8_t* d_mask, void* stream) {
    int p1 = 0, p2 = 0;
    sm::Pairs pr;
    int rc = subpix_check(h, width, height, pitch, radius, num_disp, flags, &p1, &p2, &pr);
    if (rc) return rc;
    if (!d_left || !d_right || !d_disp16) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    if (batch < 1) return fail(SM_ERR_INVALID_ARG, "batch %d < 1", batch);
    if (out_pitch < width) return fail(SM_ERR_INVALID_ARG, "out_pitch %d < width %d", out_pitch, width);
    if (batch > 1 && (frame_stride < (int64_t)pitch * height || out_frame_stride < (int64_t)out_pitch * height))
        return fail(SM_ERR_INVALID_ARG, "frame strides overlap");
    SM_HIP(hipSetDevice(h->device));
    WsScope ws(h, stream_of(stream));
    rc = run_subpix(ws, h, d_left, d_right, width, height, pitch, batch, frame_stride, radius, num_disp, flags, p1, p2,
                    pr, subpix_out(d_disp16, out_pitch, out_frame_stride, d_right16, d_mask, flags));
    if (rc) return rc;
    return subpix_speckle(ws, h, d_disp16, width, height, out_pitch, batch, out_frame_stride, d_mask);
}

SM_API int sm_block_match_subpix_u16(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                                     int pitch, int radius, int num_disp, unsigned flags, uint16_t* disp16_out,
                                     uint16_t* right16_out, uint8_t* mask_out, int out_pitch) {
    int p1 = 0, p2 = 0;
    sm::Pairs pr;
    int rc = subpix_check(h, width, height, pitch, radius, num_disp, flags, &p1, &p2, &pr);
    if (rc) return rc;
    if (!left || !right || !disp16_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    if (out_pitch < width) return fail(SM_ERR_INVALID_ARG, "out_pitch %d < width %d", out_pitch, width);
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t P = (size_t)width * height;
    rc = h->aux.reserve(5 * P);   // [q u16][right q u16][mask u8]
    if (rc) return rc;
    uint16_t* dq = h->aux.as<uint16_t>();
    uint16_t* dr = dq + P;
    uint8_t* dm = h->aux.p + 4 * P;
    rc = upload_pair(h, left, right, width, height, pitch, s);
    if (rc) return rc;
    WsScope ws(h, s);
    rc = run_subpix(ws, h, h->d_left, h->d_right, width, height, width, 1, (int64_t)P, radius, num_disp, flags, p1, p2,
                    pr, subpix_out(dq, width, (int64_t)P, right16_out ? dr : nullptr, mask_out ? dm : nullptr, flags));
    if (rc) return rc;
    rc = subpix_speckle(ws, h, dq, width, height, width, 1, (int64_t)P, mask_out ? dm : nullptr);
    if (rc) return rc;
    const size_t row2 = (size_t)width * 2, op2 = (size_t)out_pitch * 2;
    SM_HIP(copy2d(disp16_out, op2, dq, row2, row2, height, hipMemcpyDeviceToHost, s));
    if (right16_out) SM_HIP(copy2d(right16_out, op2, dr, row2, row2, height, hipMemcpyDeviceToHost, s));
    if (mask_out) SM_HIP(copy2d(mask_out, out_pitch, dm, width, width, height, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

SM_API int sm_volume_wta_subpix_device(sm_handle* h, const void* d_vol, int elem_bytes, int width, int height,
                                       int num_disp, uint32_t invalid_from, unsigned flags, uint16_t* d_disp16,
                                       int out_pitch, uint16_t* d_right16, uint8_t* d_mask, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (width <= 0 || height <= 0) return fail(SM_ERR_INVALID_ARG, "bad frame size %dx%d", width, height);
    if (num_disp < 1 || num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "num_disp %d out of [1,%d]", num_disp, sm::kMaxDisp);
    if (elem_bytes != 2 && elem_bytes != 4)
        return fail(SM_ERR_INVALID_ARG, "elem_bytes %d: the volume holds uint16 (2) or uint32 (4) costs", elem_bytes);
    if (flags & ~(unsigned)(SM_LR_CHECK | SM_PAIRS_IN_VIEW))
        return fail(SM_ERR_INVALID_ARG,
                    "sub-pixel WTA of a volume: flags are 0, SM_LR_CHECK, SM_PAIRS_IN_VIEW (0x%x)", flags);
    sm::Pairs pr;   // with the flag, plane k of the caller's volume is d = SM_PARAM_MIN_DISP + k
    {
        const int rc = pairs_check(h, flags, num_disp, true, &pr);
        if (rc) return rc;
    }
    if (!d_vol || !d_disp16) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    if (out_pitch < width) return fail(SM_ERR_INVALID_ARG, "out_pitch %d < width %d", out_pitch, width);
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = stream_of(stream);
    WsScope ws(h, s);
    const bool lr = (flags & SM_LR_CHECK) != 0;
    if (h->subpix_median) {   // SM_PARAM_SUBPIX_MEDIAN: WTA into planes of the LR workspace, median, check on the result
        const int64_t P = (int64_t)width * height;
        uint8_t* planes = nullptr;
        int rc = ws.get(h->lr, subpix_median_bytes(P, lr, d_right16 != nullptr), &planes);
        if (rc) return rc;
        const SubpixMedianWs mw = subpix_median_ws(planes, P, lr, d_right16 != nullptr);
        if (elem_bytes == 4)
            SM_HIP(sm::launch_subpix_wta_u32(static_cast<const uint32_t*>(d_vol), width, height, num_disp,
                                             invalid_from, h->uniqueness, 1, false, mw.left, width, mw.right, nullptr,
                                             nullptr, s, pr));
        else
            SM_HIP(sm::launch_subpix_wta_u16(static_cast<const uint16_t*>(d_vol), width, height, num_disp,
                                             invalid_from, h->uniqueness, 1, false, mw.left, width, mw.right, nullptr,
                                             nullptr, s, pr));
        return run_subpix_median(s, mw, width, height, h->subpix_median, d_disp16, out_pitch, d_right16, lr, d_mask);
    }
    uint8_t* d0 = nullptr;
    if (lr) {   // the two views' d0 go through the LR workspace (16-bit each with SM_PAIRS_IN_VIEW)
        const int rc = ws.get(h->lr, (pr.in_view ? 4 : 2) * (size_t)width * height, &d0);
        if (rc) return rc;
    }
    if (elem_bytes == 4)
        SM_HIP(sm::launch_subpix_wta_u32(static_cast<const uint32_t*>(d_vol), width, height, num_disp, invalid_from,
                                         h->uniqueness, 1, lr, d_disp16, out_pitch, d_right16, d_mask, d0, s, pr));
    else
        SM_HIP(sm::launch_subpix_wta_u16(static_cast<const uint16_t*>(d_vol), width, height, num_disp, invalid_from,
                                         h->uniqueness, 1, lr, d_disp16, out_pitch, d_right16, d_mask, d0, s, pr));
    return SM_OK;
}

}  // extern "C"
