// sm_capi_speckle.hip — the C ABI's speckle filter (bm_speckle.hip): the workspace size, the device call, the host
// calls, and run_speckle, the step the matching calls end with when SM_PARAM_SPECKLE_SIZE is set.
#include "sm_handle.h"

namespace smh {

int run_speckle(WsScope& ws, sm_handle* h, void* map, int elem_bytes, int W, int H, int pitch, int batch,
                int64_t fstride, int max_size, int max_diff, uint8_t* mask) {
    if (max_size == 0) return SM_OK;   // nothing to remove: no workspace, no launch
    const sm::SpecklePlan p = sm::plan_speckle(W, H, batch);
    uint8_t* base = nullptr;
    const int rc = ws.get(h->spk, p.bytes, &base);
    if (rc) return rc;
    uint32_t* label = reinterpret_cast<uint32_t*>(base);
    uint32_t* count = reinterpret_cast<uint32_t*>(base + p.plane_bytes);
    if (elem_bytes == 2)
        SM_HIP(sm::launch_speckle(static_cast<uint16_t*>(map), W, H, pitch, fstride, batch, max_size, max_diff, mask,
                                  label, count, ws.stream()));
    else
        SM_HIP(sm::launch_speckle(static_cast<uint8_t*>(map), W, H, pitch, fstride, batch, max_size, max_diff, mask,
                                  label, count, ws.stream()));
    return SM_OK;
}

}  // namespace smh

using namespace smh;

namespace {

// What every speckle call checks before the device is touched (the frame strides of a batch by the device call):
// the arguments' own rules first, which need no handle, then the handle and its capacity
int speckle_check(const sm_handle* h, const void* map, int elem_bytes, int width, int height, int pitch, int batch,
                  int max_size, int max_diff) {
    if (elem_bytes != 1 && elem_bytes != 2)
        return fail(SM_ERR_INVALID_ARG, "speckle filter: elem_bytes %d (a uint8 map is 1, a uint16 map 2)", elem_bytes);
    if (width <= 0 || height <= 0) return fail(SM_ERR_INVALID_ARG, "speckle filter: bad frame size %dx%d", width, height);
    if (batch < 1) return fail(SM_ERR_INVALID_ARG, "speckle filter: batch %d < 1", batch);
    if (pitch < width) return fail(SM_ERR_INVALID_ARG, "speckle filter: pitch %d < width %d", pitch, width);
    if (max_size < 0) return fail(SM_ERR_INVALID_ARG, "speckle filter: max_size %d < 0", max_size);
    const int top = elem_bytes == 1 ? 255 : 65535;
    if (max_diff < 0 || max_diff > top)
        return fail(SM_ERR_INVALID_ARG, "speckle filter: max_diff %d out of [0, %d]", max_diff, top);
    if (!map) return fail(SM_ERR_INVALID_ARG, "speckle filter: null map pointer");
    if (!sm::speckle_pass_ok(width, height, batch))
        return fail(SM_ERR_INVALID_ARG, "speckle filter: frame %dx%d exceeds 2^31 - 1 pixels", width, height);
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    return check_capacity(h, width, height, 0);
}

// One host frame through the handle's staging buffer: [map][mask]
int speckle_host(sm_handle* h, void* map, int elem_bytes, int width, int height, int pitch, int max_size, int max_diff,
                 uint8_t* mask, int mask_pitch) {
    if (mask && mask_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "speckle filter: mask_pitch %d < width %d", mask_pitch, width);
    int rc = speckle_check(h, map, elem_bytes, width, height, pitch, 1, max_size, max_diff);
    if (rc) return rc;
    if (max_size == 0) return SM_OK;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t P = (size_t)width * height, row = (size_t)width * elem_bytes;
    rc = h->aux.reserve(P * elem_bytes + P);
    if (rc) return rc;
    uint8_t* dmap = h->aux.p;
    uint8_t* dmask = mask ? dmap + P * elem_bytes : nullptr;
    SM_HIP(copy2d(dmap, row, map, (size_t)pitch * elem_bytes, row, height, hipMemcpyHostToDevice, s));
    if (mask) SM_HIP(copy2d(dmask, width, mask, mask_pitch, width, height, hipMemcpyHostToDevice, s));
    WsScope ws(h, s);
    rc = run_speckle(ws, h, dmap, elem_bytes, width, height, width, 1, (int64_t)P, max_size, max_diff, dmask);
    if (rc) return rc;
    SM_HIP(copy2d(map, (size_t)pitch * elem_bytes, dmap, row, row, height, hipMemcpyDeviceToHost, s));
    if (mask) SM_HIP(copy2d(mask, mask_pitch, dmask, width, width, height, hipMemcpyDeviceToHost, s));
    return ws.drain();
}

}  // namespace

extern "C" {

SM_API int sm_speckle_workspace_bytes(int width, int height, int batch, size_t* bytes) {
    if (!bytes) return fail(SM_ERR_INVALID_ARG, "null bytes pointer");
    *bytes = 0;
    if (!sm::speckle_pass_ok(width, height, batch))
        return fail(SM_ERR_INVALID_ARG, "speckle filter: bad frame %dx%d x %d (at most 2^31 - 1 pixels)", width, height,
                    batch);
    *bytes = sm::plan_speckle(width, height, batch).bytes;
    return SM_OK;
}

SM_API int sm_speckle_filter_device(sm_handle* h, void* d_map, int elem_bytes, int width, int height, int pitch,
                                    int batch, int64_t frame_stride, int max_size, int max_diff, uint8_t* d_mask,
                                    void* stream) {
    if (batch > 1 && frame_stride < (int64_t)pitch * height)
        return fail(SM_ERR_INVALID_ARG, "speckle filter: frame strides overlap");
    const int rc = speckle_check(h, d_map, elem_bytes, width, height, pitch, batch, max_size, max_diff);
    if (rc) return rc;
    if (max_size == 0) return SM_OK;
    SM_HIP(hipSetDevice(h->device));
    WsScope ws(h, stream_of(stream));
    return run_speckle(ws, h, d_map, elem_bytes, width, height, pitch, batch, frame_stride, max_size, max_diff, d_mask);
}

SM_API int sm_speckle_filter_u8(sm_handle* h, uint8_t* map, int width, int height, int pitch, int max_size,
                                int max_diff, uint8_t* mask, int mask_pitch) {
    return speckle_host(h, map, 1, width, height, pitch, max_size, max_diff, mask, mask_pitch);
}

SM_API int sm_speckle_filter_u16(sm_handle* h, uint16_t* map, int width, int height, int pitch, int max_size,
                                 int max_diff, uint8_t* mask, int mask_pitch) {
    return speckle_host(h, map, 2, width, height, pitch, max_size, max_diff, mask, mask_pitch);
}

}  // extern "C"
