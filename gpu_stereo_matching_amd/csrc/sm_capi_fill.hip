// sm_capi_fill.hip — the C ABI's row fill (bm_fill.hip): the device call, the host calls, and run_fill, the step
// the matching calls end with when SM_PARAM_FILL_GAP is set.
#include "sm_handle.h"

namespace smh {

int run_fill(hipStream_t s, void* map, int elem_bytes, int W, int H, int pitch, int batch, int64_t fstride,
             int max_gap) {
    if (max_gap == 0) return SM_OK;   // nothing to fill: no launch
    if (!sm::fill_pass_ok(W, H, batch))
        return fail(SM_ERR_INVALID_ARG, "row fill: %d frames of %dx%d exceed 2^31 - 1 rows or 2^30 columns", batch, W, H);
    if (elem_bytes == 2)
        SM_HIP(sm::launch_fill(static_cast<uint16_t*>(map), W, H, pitch, fstride, batch, max_gap, s));
    else
        SM_HIP(sm::launch_fill(static_cast<uint8_t*>(map), W, H, pitch, fstride, batch, max_gap, s));
    return SM_OK;
}

}  // namespace smh

using namespace smh;

namespace {

constexpr int kMaxFillGap = 1 << 24;   // SM_PARAM_FILL_GAP's range

// What every fill call checks before the device is touched (the frame strides of a batch by the device call), in
// the speckle calls' order: the arguments' own rules first, which need no handle, then the handle and its capacity
int fill_check(const sm_handle* h, const void* map, int elem_bytes, int width, int height, int pitch, int batch,
               int max_gap) {
    if (elem_bytes != 1 && elem_bytes != 2)
        return fail(SM_ERR_INVALID_ARG, "row fill: elem_bytes %d (a uint8 map is 1, a uint16 map 2)", elem_bytes);
    if (width <= 0 || height <= 0) return fail(SM_ERR_INVALID_ARG, "row fill: bad frame size %dx%d", width, height);
    if (batch < 1) return fail(SM_ERR_INVALID_ARG, "row fill: batch %d < 1", batch);
    if (pitch < width) return fail(SM_ERR_INVALID_ARG, "row fill: pitch %d < width %d", pitch, width);
    if (max_gap < 0 || max_gap > kMaxFillGap)
        return fail(SM_ERR_INVALID_ARG, "row fill: max_gap %d out of [0, 2^24]", max_gap);
    if (!map) return fail(SM_ERR_INVALID_ARG, "row fill: null map pointer");
    if (!sm::fill_pass_ok(width, height, batch))
        return fail(SM_ERR_INVALID_ARG, "row fill: %d frames of %dx%d exceed 2^31 - 1 rows or 2^30 columns", batch,
                    width, height);
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    return check_capacity(h, width, height, 0);
}

// One host frame through the handle's staging buffer
int fill_host(sm_handle* h, void* map, int elem_bytes, int width, int height, int pitch, int max_gap) {
    int rc = fill_check(h, map, elem_bytes, width, height, pitch, 1, max_gap);
    if (rc) return rc;
    if (max_gap == 0) return SM_OK;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t P = (size_t)width * height, row = (size_t)width * elem_bytes;
    rc = h->aux.reserve(P * elem_bytes);
    if (rc) return rc;
    uint8_t* dmap = h->aux.p;
    SM_HIP(copy2d(dmap, row, map, (size_t)pitch * elem_bytes, row, height, hipMemcpyHostToDevice, s));
    rc = run_fill(s, dmap, elem_bytes, width, height, width, 1, (int64_t)P, max_gap);
    if (rc) return rc;
    SM_HIP(copy2d(map, (size_t)pitch * elem_bytes, dmap, row, row, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

}  // namespace

extern "C" {

SM_API int sm_fill_invalid_device(sm_handle* h, void* d_map, int elem_bytes, int width, int height, int pitch,
                                  int batch, int64_t frame_stride, int max_gap, void* stream) {
    if (batch > 1 && frame_stride < (int64_t)pitch * height)
        return fail(SM_ERR_INVALID_ARG, "row fill: frame strides overlap");
    const int rc = fill_check(h, d_map, elem_bytes, width, height, pitch, batch, max_gap);
    if (rc) return rc;
    if (max_gap == 0) return SM_OK;
    SM_HIP(hipSetDevice(h->device));
    return run_fill(stream_of(stream), d_map, elem_bytes, width, height, pitch, batch, frame_stride, max_gap);
}

SM_API int sm_fill_invalid_u8(sm_handle* h, uint8_t* map, int width, int height, int pitch, int max_gap) {
    return fill_host(h, map, 1, width, height, pitch, max_gap);
}

SM_API int sm_fill_invalid_u16(sm_handle* h, uint16_t* map, int width, int height, int pitch, int max_gap) {
    return fill_host(h, map, 2, width, height, pitch, max_gap);
}

}  // extern "C"
