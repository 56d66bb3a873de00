// sm_capi_aux.hip — the C ABI's calls around the matcher: colour conversion, remap and rectification, the AD /
// census / SAD volumes, median, LR check, reprojection, and the segment-tree matcher.
#include <chrono>
#include <new>

#include "sm_handle.h"

using namespace smh;

extern "C" {

// ---- 3-D reprojection (bm_subpix.hip) ----
static int reproject_check(const sm_handle* h, const void* disp16, int width, int height, int pitch, const double* Q,
                           const void* xyz, int xyz_pitch) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (width <= 0 || height <= 0) return fail(SM_ERR_INVALID_ARG, "bad frame size %dx%d", width, height);
    if (!disp16 || !Q || !xyz) return fail(SM_ERR_INVALID_ARG, "null pointer");
    if (pitch < width) return fail(SM_ERR_INVALID_ARG, "pitch %d < width %d", pitch, width);
    if ((int64_t)xyz_pitch < 3 * (int64_t)width)
        return fail(SM_ERR_INVALID_ARG, "xyz_pitch %d < 3 * width (%d floats per row)", xyz_pitch, 3 * width);
    return SM_OK;
}

SM_API int sm_reproject_device(sm_handle* h, const uint16_t* d_disp16, int width, int height, int pitch,
                               const double* Q, float* d_xyz, int xyz_pitch, void* stream) {
    const int rc = reproject_check(h, d_disp16, width, height, pitch, Q, d_xyz, xyz_pitch);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_reproject(d_disp16, width, height, pitch, Q, d_xyz, xyz_pitch, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_reproject_u16(sm_handle* h, const uint16_t* disp16, int width, int height, int pitch, const double* Q,
                            float* xyz_out, int xyz_pitch) {
    int rc = reproject_check(h, disp16, width, height, pitch, Q, xyz_out, xyz_pitch);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t P = (size_t)width * height;
    WsScope ws(h, s);
    uint8_t* vol = nullptr;
    rc = ws.get(h->vol, 16 * P, &vol);   // [xyz 12 P][q 2 P]
    if (rc) return rc;
    float* dx = reinterpret_cast<float*>(vol);
    uint16_t* dq = reinterpret_cast<uint16_t*>(vol + 12 * P);
    const size_t row2 = (size_t)width * 2, row12 = (size_t)width * 12;
    SM_HIP(copy2d(dq, row2, disp16, (size_t)pitch * 2, row2, height, hipMemcpyHostToDevice, s));
    SM_HIP(sm::launch_reproject(dq, width, height, width, Q, dx, 3 * width, s));
    SM_HIP(copy2d(xyz_out, (size_t)xyz_pitch * 4, dx, row12, row12, height, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

SM_API int sm_lr_check_device(sm_handle* h, const uint8_t* d_left_disp, const uint8_t* d_right_disp, int width,
                              int height, int pitch, uint8_t* d_out, uint8_t* d_mask, int out_pitch, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_left_disp || !d_right_disp || !d_out || width <= 0 || height <= 0 || pitch < width || out_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad lr_check arguments");
    if (d_right_disp == d_out) return fail(SM_ERR_INVALID_ARG, "lr_check: the right map cannot be the output");
    SM_HIP(hipSetDevice(h->device));
    const int64_t P = (int64_t)width * height;
    SM_HIP(sm::launch_lr_check(d_left_disp, pitch, P, d_right_disp, pitch, P, 0, width, height, 1, d_out, out_pitch, P,
                               nullptr, d_mask, out_pitch, P, stream_of(stream)));
    return SM_OK;
}

// ---- colour conversion, remap, rectification (bm_pre.hip, bm_rectify.hip) ----
SM_API int sm_bgr_to_gray_device(sm_handle* h, const uint8_t* d_bgr, int width, int height, int pitch, int channels,
                                 uint8_t* d_gray, int gray_pitch, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_bgr || !d_gray || width <= 0 || height <= 0 || (channels != 3 && channels != 4) ||
        pitch < width * channels || gray_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad bgr_to_gray arguments");
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_bgr_to_gray(d_bgr, width, height, pitch, channels, d_gray, gray_pitch, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_remap_u8_device(sm_handle* h, const uint8_t* d_src, int width, int height, int pitch,
                              const float* d_mapx, const float* d_mapy, int map_pitch, uint8_t* d_dst, int dst_pitch,
                              void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_src || !d_mapx || !d_mapy || !d_dst || width <= 0 || height <= 0 || pitch < width || map_pitch < width ||
        dst_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad remap arguments");
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_remap(d_src, width, height, pitch, d_mapx, d_mapy, map_pitch, d_dst, dst_pitch,
                            stream_of(stream)));
    return SM_OK;
}

SM_API int sm_bgr_to_gray_u8(sm_handle* h, const uint8_t* bgr, int width, int height, int pitch, int channels,
                             uint8_t* gray, int gray_pitch) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!bgr || !gray || width <= 0 || height <= 0 || (channels != 3 && channels != 4) || pitch < width * channels ||
        gray_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad BGR layout");
    int rc = check_capacity(h, width, height, 0);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t row = (size_t)width * channels;
    rc = h->bgr.reserve(row * height);
    if (rc) return rc;
    SM_HIP(copy2d(h->bgr.p, row, bgr, pitch, row, height, hipMemcpyHostToDevice, s));
    SM_HIP(sm::launch_bgr_to_gray(h->bgr.p, width, height, (int)row, channels, h->d_left, width, s));
    SM_HIP(copy2d(gray, gray_pitch, h->d_left, width, width, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

SM_API int sm_remap_u8(sm_handle* h, const uint8_t* src, int width, int height, int pitch, const float* mapx,
                       const float* mapy, int map_pitch, uint8_t* dst, int dst_pitch) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!src || !mapx || !mapy || !dst || width <= 0 || height <= 0 || pitch < width || map_pitch < width ||
        dst_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad remap arguments");
    int rc = check_capacity(h, width, height, 0);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t plane = (size_t)width * height, row4 = width * sizeof(float);
    rc = h->maps.reserve(2 * plane * sizeof(float));
    if (rc) return rc;
    float* dmx = h->maps.as<float>();
    float* dmy = dmx + plane;
    SM_HIP(copy2d(dmx, row4, mapx, (size_t)map_pitch * sizeof(float), row4, height, hipMemcpyHostToDevice, s));
    SM_HIP(copy2d(dmy, row4, mapy, (size_t)map_pitch * sizeof(float), row4, height, hipMemcpyHostToDevice, s));
    SM_HIP(copy2d(h->d_left, width, src, pitch, width, height, hipMemcpyHostToDevice, s));
    SM_HIP(sm::launch_remap(h->d_left, width, height, width, dmx, dmy, width, h->d_right, width, s));
    SM_HIP(copy2d(dst, dst_pitch, h->d_right, width, width, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

SM_API int sm_stereo_rectify(const double* K1, const double* dist1, int ndist1, const double* K2, const double* dist2,
                             int ndist2, int width, int height, const double* R, int r_len, const double* T, double* R1,
                             double* R2, double* P1, double* P2, double* Q) {
    if (!K1 || !K2 || !R || !T || !R1 || !R2 || !P1 || !P2 || !Q || width <= 0 || height <= 0)
        return fail(SM_ERR_INVALID_ARG, "bad stereo_rectify arguments");
    auto ndist_ok = [](int n, const double* d) { return (n == 0 || n == 4 || n == 5 || n == 8) && (n == 0 || d); };
    if (!ndist_ok(ndist1, dist1) || !ndist_ok(ndist2, dist2))
        return fail(SM_ERR_INVALID_ARG, "distortion vectors hold 0, 4, 5 or 8 coefficients");
    if (r_len != 9 && r_len != 3) return fail(SM_ERR_INVALID_ARG, "R is a 3x3 matrix (9) or a rotation vector (3)");
    if (!sm::stereo_rectify(K1, dist1, ndist1, K2, dist2, ndist2, width, height, R, r_len, T, R1, R2, P1, P2, Q))
        return fail(SM_ERR_INVALID_ARG, "singular rotation matrix");
    return SM_OK;
}

static int check_map_args(const sm_handle* h, const double* K, const double* dist, int ndist, const double* R,
                          const double* P, int width, int height, const float* mx, const float* my, int map_pitch) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!K || !R || !P || !mx || !my || width <= 0 || height <= 0 || map_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad rectify-map arguments");
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8) || (ndist && !dist))
        return fail(SM_ERR_INVALID_ARG, "distortion vectors hold 0, 4, 5 or 8 coefficients");
    return SM_OK;
}

SM_API int sm_init_rectify_map_device(sm_handle* h, const double* K, const double* dist, int ndist, const double* R,
                                      const double* P, int width, int height, float* d_mapx, float* d_mapy,
                                      int map_pitch, void* stream) {
    int rc = check_map_args(h, K, dist, ndist, R, P, width, height, d_mapx, d_mapy, map_pitch);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    const hipError_t e = sm::launch_rectify_map(K, dist, ndist, R, P, width, height, d_mapx, d_mapy, map_pitch,
                                                stream_of(stream));
    if (e == hipErrorInvalidValue) return fail(SM_ERR_INVALID_ARG, "P[:, :3] * R is singular");
    SM_HIP(e);
    return SM_OK;
}

SM_API int sm_init_rectify_map(sm_handle* h, const double* K, const double* dist, int ndist, const double* R,
                               const double* P, int width, int height, float* mapx, float* mapy, int map_pitch) {
    int rc = check_map_args(h, K, dist, ndist, R, P, width, height, mapx, mapy, map_pitch);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t plane = (size_t)width * height, row4 = width * sizeof(float);
    rc = h->maps.reserve(2 * plane * sizeof(float));
    if (rc) return rc;
    float* dmx = h->maps.as<float>();
    float* dmy = dmx + plane;
    const hipError_t e = sm::launch_rectify_map(K, dist, ndist, R, P, width, height, dmx, dmy, width, s);
    if (e == hipErrorInvalidValue) return fail(SM_ERR_INVALID_ARG, "P[:, :3] * R is singular");
    SM_HIP(e);
    SM_HIP(copy2d(mapx, (size_t)map_pitch * sizeof(float), dmx, row4, row4, height, hipMemcpyDeviceToHost, s));
    SM_HIP(copy2d(mapy, (size_t)map_pitch * sizeof(float), dmy, row4, row4, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

// ---- cost volumes (bm_volume.hip, bm_census.hip) ----
SM_API int sm_ad_volume_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                               int pitch, int num_disp, uint8_t* d_dif, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_left || !d_right || !d_dif || width <= 0 || height <= 0 || pitch < width || num_disp < 1 ||
        num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "bad AD-volume arguments");
    if (width > 4096) return fail(SM_ERR_INVALID_ARG, "width %d exceeds the AD-volume kernel's 4096 columns", width);
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_ad_volume(d_left, d_right, width, height, pitch, (int64_t)pitch * height, 1, num_disp, d_dif,
                                (int64_t)width * height * num_disp, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_ad_volume_u8(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                           int num_disp, uint8_t* dif_out) {
    int rc = check_geometry(h, width, height, pitch, 0, num_disp);
    if (rc) return rc;
    if (!left || !right || !dif_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    if (width > 4096) return fail(SM_ERR_INVALID_ARG, "width %d exceeds the AD-volume kernel's 4096 columns", width);
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t need = (size_t)width * height * num_disp;
    WsScope ws(h, s);
    uint8_t* vol = nullptr;
    rc = ws.get(h->vol, need, &vol);
    if (rc) return rc;
    rc = upload_pair(h, left, right, width, height, pitch, s);
    if (rc) return rc;
    SM_HIP(sm::launch_ad_volume(h->d_left, h->d_right, width, height, width, (int64_t)width * height, 1, num_disp,
                                vol, (int64_t)need, s));
    SM_HIP(hipMemcpyAsync(dif_out, vol, need, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

SM_API int sm_census_device(sm_handle* h, const uint8_t* d_img, int width, int height, int pitch, uint64_t* d_census,
                            void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_img || !d_census || width <= 0 || height <= 0 || pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad census arguments");
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_census(d_img, width, height, pitch, d_census, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_census_volume_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                   int pitch, int num_disp, uint8_t* d_ham, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_left || !d_right || !d_ham || width <= 0 || height <= 0 || pitch < width || num_disp < 1 ||
        num_disp > sm::kMaxDisp)
        return fail(SM_ERR_INVALID_ARG, "bad census-volume arguments");
    if (width > 4096)
        return fail(SM_ERR_INVALID_ARG, "width %d exceeds the census-volume kernel's 4096 columns", width);
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = stream_of(stream);
    WsScope ws(h, s);
    const size_t img = align256((size_t)width * height * 8);
    uint8_t* vol = nullptr;
    const int rc = ws.get(h->vol, 2 * img, &vol);   // the two census images
    if (rc) return rc;
    uint64_t* cl = reinterpret_cast<uint64_t*>(vol);
    uint64_t* cr = reinterpret_cast<uint64_t*>(vol + img);
    SM_HIP(sm::launch_census(d_left, width, height, pitch, cl, s));
    SM_HIP(sm::launch_census(d_right, width, height, pitch, cr, s));
    SM_HIP(sm::launch_census_volume(cl, cr, width, height, num_disp, d_ham, s));
    return SM_OK;
}

SM_API int sm_census_volume_u8(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                               int num_disp, uint8_t* ham_out) {
    int rc = check_geometry(h, width, height, pitch, 0, num_disp);
    if (rc) return rc;
    if (!left || !right || !ham_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    if (width > 4096)
        return fail(SM_ERR_INVALID_ARG, "width %d exceeds the census-volume kernel's 4096 columns", width);
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t need = (size_t)width * height * num_disp;
    const size_t ham = align256(need), img = align256((size_t)width * height * 8);
    WsScope ws(h, s);
    uint8_t* vol = nullptr;
    rc = ws.get(h->vol, ham + 2 * img, &vol);   // [Hamming volume][census L][census R]
    if (rc) return rc;
    uint64_t* cl = reinterpret_cast<uint64_t*>(vol + ham);
    uint64_t* cr = reinterpret_cast<uint64_t*>(vol + ham + img);
    rc = upload_pair(h, left, right, width, height, pitch, s);
    if (rc) return rc;
    SM_HIP(sm::launch_census(h->d_left, width, height, width, cl, s));
    SM_HIP(sm::launch_census(h->d_right, width, height, width, cr, s));
    SM_HIP(sm::launch_census_volume(cl, cr, width, height, num_disp, vol, s));
    SM_HIP(hipMemcpyAsync(ham_out, vol, need, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

SM_API int sm_sad_volume_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                int pitch, int radius, int num_disp, uint16_t* d_sad, void* stream) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!d_left || !d_right || !d_sad) return fail(SM_ERR_INVALID_ARG, "null pointer");
    if (radius > sm::kMaxFastRadius) return fail(SM_ERR_INVALID_ARG, "SAD volume: radius %d > 7", radius);
    if (width > 4096) return fail(SM_ERR_INVALID_ARG, "SAD volume: width %d exceeds 4096", width);
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = stream_of(stream);
    WsScope ws(h, s);
    const int64_t P = (int64_t)width * height;
    uint8_t* ad = nullptr;
    rc = ws.get(h->vol, (size_t)(P * num_disp), &ad);
    if (rc) return rc;
    SM_HIP(sm::launch_ad_volume(d_left, d_right, width, height, pitch, (int64_t)pitch * height, 1, num_disp, ad,
                                P * num_disp, s));
    SM_HIP(sm::launch_box_sad_volume(ad, width, height, radius, num_disp, d_sad, s));
    return SM_OK;
}

// getAllSAD's volume (P * D device bytes, pixel-major) on the scope's stream into `out`, or, with out == nullptr,
// into the first P * D bytes of the handle's volume workspace (*where says which).  r <= 7 and W <= 4096: AD
// volume -> u16 SAD volume behind it -> transpose (the AD volume at the start of the workspace is consumed by the
// SAD kernel before the transpose overwrites it, in stream order); otherwise the direct kernel.
static int run_all_sad(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch,
                       int radius, int D, uint8_t* out, uint8_t** where) {
    hipStream_t s = ws.stream();
    const int64_t P = (int64_t)W * H;
    if (radius <= sm::kMaxFastRadius && W <= 4096) {
        const size_t ad_bytes = align256((size_t)(P * D));   // the u16 volume starts 256-B aligned
        uint8_t* ad = nullptr;
        int rc = ws.get(h->vol, ad_bytes + (size_t)(2 * P * D), &ad);
        if (rc) return rc;
        uint16_t* sad = reinterpret_cast<uint16_t*>(ad + ad_bytes);
        if (!out) out = ad;
        SM_HIP(sm::launch_ad_volume(L, R, W, H, pitch, (int64_t)pitch * H, 1, D, ad, P * D, s));
        SM_HIP(sm::launch_box_sad_volume(ad, W, H, radius, D, sad, s));
        SM_HIP(sm::launch_all_sad_transpose(sad, W, H, D, out, s));
    } else {
        if (!out) {
            int rc = ws.get(h->vol, (size_t)(P * D), &out);
            if (rc) return rc;
        }
        SM_HIP(sm::launch_all_sad_generic(L, R, W, H, pitch, radius, D, out, s));
    }
    if (where) *where = out;
    return SM_OK;
}

SM_API int sm_all_sad_device(sm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                             int pitch, int radius, int num_disp, uint8_t* d_out, void* stream) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!d_left || !d_right || !d_out) return fail(SM_ERR_INVALID_ARG, "null device pointer");
    SM_HIP(hipSetDevice(h->device));
    WsScope ws(h, stream_of(stream));
    return run_all_sad(ws, h, d_left, d_right, width, height, pitch, radius, num_disp, d_out, nullptr);
}

SM_API int sm_all_sad_u8(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                         int radius, int num_disp, uint8_t* sad_out) {
    int rc = check_geometry(h, width, height, pitch, radius, num_disp);
    if (rc) return rc;
    if (!left || !right || !sad_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    rc = check_capacity(h, width, height, num_disp);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    WsScope ws(h, s);
    const size_t need = (size_t)width * height * num_disp;
    rc = upload_pair(h, left, right, width, height, pitch, s);
    if (rc) return rc;
    uint8_t* vol = nullptr;
    rc = run_all_sad(ws, h, h->d_left, h->d_right, width, height, width, radius, num_disp, nullptr, &vol);
    if (rc) return rc;
    SM_HIP(hipMemcpyAsync(sad_out, vol, need, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

SM_API int sm_median_u8_device(sm_handle* h, const uint8_t* d_src, int width, int height, int pitch, int radius,
                               uint8_t* d_dst, int dst_pitch, void* stream) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!d_src || !d_dst || width <= 0 || height <= 0 || pitch < width || dst_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad median arguments");
    if (radius < 1 || radius > 3) return fail(SM_ERR_INVALID_ARG, "median radius %d out of [1,3]", radius);
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_median(d_src, width, height, pitch, (int64_t)pitch * height, 1, radius, d_dst, dst_pitch,
                             (int64_t)dst_pitch * height, stream_of(stream)));
    return SM_OK;
}

// ---- segment-tree stereo (bm_segtree.hip) behind both C entry points: refined = false ST-1, true ST-2 ----
// Its device buffers (bgr, st, d_disp) belong to the host calls on the handle's stream alone: no shared workspace.
static int segment_tree_call(sm_handle* h, const uint8_t* left_bgr, const uint8_t* right_bgr, int width, int height,
                             int pitch, int max_level, int scale, float sigma, uint8_t* disp_out, int out_pitch,
                             bool refined) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!left_bgr || !right_bgr || !disp_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    if (width < 2 || height < 1 || pitch < 3 * width || out_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad frame geometry %dx%d (pitch %d, out_pitch %d)", width, height, pitch,
                    out_pitch);
    if (max_level < 1 || max_level > sm::kMaxDisp) return fail(SM_ERR_INVALID_ARG, "max_level %d out of [1,256]", max_level);
    if (scale < 0) return fail(SM_ERR_INVALID_ARG, "scale %d < 0", scale);
    if (!(sigma > 0.f)) return fail(SM_ERR_INVALID_ARG, "sigma must be > 0");
    int rc = check_capacity(h, width, height, max_level);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    const auto t0 = std::chrono::steady_clock::now();
    const size_t row = (size_t)width * 3;
    rc = h->bgr.reserve(2 * row * height);
    if (rc) return rc;
    hipStream_t s = h->stream;
    uint8_t* dl = h->bgr.p;
    uint8_t* dr = dl + row * height;
    SM_HIP(copy2d(dl, row, left_bgr, pitch, row, height, hipMemcpyHostToDevice, s));
    SM_HIP(copy2d(dr, row, right_bgr, pitch, row, height, hipMemcpyHostToDevice, s));
    h->st_valid = false;
    constexpr float kTau = 1200.0f;   // TAU, Toolkit.h:34
    if (refined)
        SM_HIP(sm::segment_tree_refined_match(h->st, dl, dr, width, height, (int)row, max_level, scale, sigma, kTau,
                                              h->d_disp, s, &h->st_stats));
    else
        SM_HIP(sm::segment_tree_match(h->st, dl, dr, width, height, (int)row, max_level, scale, sigma, kTau, h->d_disp,
                                      s, &h->st_stats));
    SM_HIP(copy2d(disp_out, out_pitch, h->d_disp, width, width, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    h->st_total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->st_valid = true;
    return SM_OK;
}

static int segment_tree_entry(sm_handle* h, const uint8_t* left_bgr, const uint8_t* right_bgr, int width, int height,
                              int pitch, int max_level, int scale, float sigma, uint8_t* disp_out, int out_pitch,
                              bool refined) {
    try {
        return segment_tree_call(h, left_bgr, right_bgr, width, height, pitch, max_level, scale, sigma, disp_out,
                                 out_pitch, refined);
    } catch (const std::bad_alloc&) {   // the host tree's buffers: no C++ exception crosses the C ABI
        return fail(SM_ERR_OUT_OF_MEMORY, "segment tree: host allocation failed");
    }
}

SM_API int sm_segment_tree_match_bgr_u8(sm_handle* h, const uint8_t* left_bgr, const uint8_t* right_bgr, int width,
                                        int height, int pitch, int max_level, int scale, float sigma,
                                        uint8_t* disp_out, int out_pitch) {
    return segment_tree_entry(h, left_bgr, right_bgr, width, height, pitch, max_level, scale, sigma, disp_out,
                              out_pitch, false);
}

SM_API int sm_segment_tree_refined_bgr_u8(sm_handle* h, const uint8_t* left_bgr, const uint8_t* right_bgr, int width,
                                          int height, int pitch, int max_level, int scale, float sigma,
                                          uint8_t* disp_out, int out_pitch) {
    return segment_tree_entry(h, left_bgr, right_bgr, width, height, pitch, max_level, scale, sigma, disp_out,
                              out_pitch, true);
}

SM_API int sm_last_segment_tree_stats(sm_handle* h, float* tree_ms, float* total_ms, int* levels) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!h->st_valid) return fail(SM_ERR_INVALID_ARG, "no segment-tree call has completed on this handle");
    if (tree_ms) *tree_ms = h->st_stats.tree_ms;
    if (total_ms) *total_ms = h->st_total_ms;
    if (levels) *levels = h->st_stats.levels;
    return SM_OK;
}

SM_API int sm_last_segment_tree_arrays(sm_handle* h, int* ints, int64_t n_ints, uint8_t* pdist, int64_t n_bytes,
                                       int* levels) {
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    if (!h->st_valid || h->st.last_pixels() <= 0) return fail(SM_ERR_INVALID_ARG, "no segment-tree call has completed on this handle");
    const int64_t P = h->st.last_pixels(), need = h->st.last_tree_ints();
    // n_bytes must be the last call's pixel count exactly: a caller slicing the ints by its own width *
    // height would mis-slice them after a call on another frame shape
    if (!ints || !pdist || n_ints < need || n_bytes != P)
        return fail(SM_ERR_INVALID_ARG, "need >= %lld ints and exactly %lld pdist bytes (the last call's pixels)",
                    (long long)need, (long long)P);
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(hipStreamSynchronize(h->stream));
    SM_HIP(h->st.copy_last_tree(ints, pdist));
    if (levels) *levels = h->st.last_levels();
    return SM_OK;
}

}  // extern "C"
