// sm_capi_median16.hip — the C ABI's 16-bit median (bm_median16.hip): the device call, the host call, and
// run_subpix_median, the steps the sub-pixel calls run between their WTA and the speckle filter when
// SM_PARAM_SUBPIX_MEDIAN is set.
#include "sm_handle.h"

namespace smh {

int run_subpix_median(hipStream_t s, const SubpixMedianWs& w, int W, int H, int radius, uint16_t* disp16, int pitch,
                      uint16_t* right16, bool lr, uint8_t* mask) {
    const int64_t P = (int64_t)W * H;
    SM_HIP(sm::launch_median16(w.left, W, H, W, P, 1, radius, disp16, pitch, P, s));
    uint16_t* rq = right16 ? right16 : w.right_out;
    if (w.right) SM_HIP(sm::launch_median16(w.right, W, H, W, P, 1, radius, rq, W, P, s));
    SM_HIP(sm::launch_subpix_lr_q(lr ? rq : nullptr, W, H, disp16, pitch, mask, s));
    return SM_OK;
}

}  // namespace smh

using namespace smh;

namespace {

// What both median calls check before the device is touched, in the fill calls' order: the arguments' own rules
// first, which need no handle, then the handle and its capacity
int median16_check(const sm_handle* h, const uint16_t* src, int width, int height, int pitch, int batch,
                   int64_t frame_stride, int radius, const uint16_t* dst, int dst_pitch, int64_t dst_frame_stride) {
    if (radius < 1 || radius > 3)
        return fail(SM_ERR_INVALID_ARG, "16-bit median: radius %d out of [1, 3]", radius);
    if (width <= 0 || height <= 0)
        return fail(SM_ERR_INVALID_ARG, "16-bit median: bad frame size %dx%d", width, height);
    if (batch < 1) return fail(SM_ERR_INVALID_ARG, "16-bit median: batch %d < 1", batch);
    if (pitch < width) return fail(SM_ERR_INVALID_ARG, "16-bit median: pitch %d < width %d", pitch, width);
    if (dst_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "16-bit median: dst_pitch %d < width %d", dst_pitch, width);
    if (!src) return fail(SM_ERR_INVALID_ARG, "16-bit median: null source pointer");
    if (!dst) return fail(SM_ERR_INVALID_ARG, "16-bit median: null destination pointer");
    if (src == dst)
        return fail(SM_ERR_INVALID_ARG, "16-bit median: source and destination are the same map (it is not in place)");
    if (batch > 1 && (frame_stride < (int64_t)pitch * height || dst_frame_stride < (int64_t)dst_pitch * height))
        return fail(SM_ERR_INVALID_ARG, "16-bit median: frame strides overlap (%lld < %d * %d or %lld < %d * %d)",
                    (long long)frame_stride, pitch, height, (long long)dst_frame_stride, dst_pitch, height);
    if (!sm::median16_pass_ok(width, height, batch))
        return fail(SM_ERR_INVALID_ARG, "16-bit median: %d frames of %dx%d exceed 2^31 - 1 tiles", batch, width, height);
    if (!h) return fail(SM_ERR_INVALID_ARG, "null handle");
    return check_capacity(h, width, height, 0);
}

}  // namespace

extern "C" {

SM_API int sm_median_u16_device(sm_handle* h, const uint16_t* d_src, int width, int height, int pitch, int batch,
                                int64_t frame_stride, int radius, uint16_t* d_dst, int dst_pitch,
                                int64_t dst_frame_stride, void* stream) {
    const int rc = median16_check(h, d_src, width, height, pitch, batch, frame_stride, radius, d_dst, dst_pitch,
                                  dst_frame_stride);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    SM_HIP(sm::launch_median16(d_src, width, height, pitch, frame_stride, batch, radius, d_dst, dst_pitch,
                               dst_frame_stride, stream_of(stream)));
    return SM_OK;
}

SM_API int sm_median_u16(sm_handle* h, const uint16_t* src, int width, int height, int pitch, int radius,
                         uint16_t* dst, int dst_pitch) {
    int rc = median16_check(h, src, width, height, pitch, 1, 0, radius, dst, dst_pitch, 0);
    if (rc) return rc;
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t P = (size_t)width * height, row = (size_t)width * 2;
    rc = h->aux.reserve(4 * P);   // [source u16][median u16]
    if (rc) return rc;
    uint16_t* dsrc = h->aux.as<uint16_t>();
    uint16_t* ddst = dsrc + P;
    SM_HIP(copy2d(dsrc, row, src, (size_t)pitch * 2, row, height, hipMemcpyHostToDevice, s));
    SM_HIP(sm::launch_median16(dsrc, width, height, width, (int64_t)P, 1, radius, ddst, width, (int64_t)P, s));
    SM_HIP(copy2d(dst, (size_t)dst_pitch * 2, ddst, row, row, height, hipMemcpyDeviceToHost, s));
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

}  // extern "C"
