// bm_speckle.hip — the speckle filter (StereoSGBM's speckleWindowSize / speckleRange, OpenCV's filterSpeckles with
// newVal = 0): connected-component labelling of a disparity map, then every component of at most max_size pixels
// is set to 0.
//
// The graph: a pixel is valid iff its value is != 0; two 4-neighbours are joined iff both are valid and
// |a - b| <= max_diff, the difference taken in 32 bits.  Regions are the connected components.
//
// A label is the index y * W + x of a pixel of the same region, never larger than the pixel's own index: a
// region's root is its smallest index, and every link points from a larger index to a smaller one.  Four passes,
// ordered by kernel boundaries only (no workgroup ever waits for another):
//   tile   one workgroup per kSpeckleTileW x kSpeckleTileH tile: lock-free union-find in LDS over the joins inside
//          the tile, the tile-local region sizes counted in LDS; label[p] = the tile-local root's frame index,
//          count[p] = that region's size in the tile at its tile-local root, 0 elsewhere (so neither plane needs
//          a memset); an invalid pixel gets kNoLabel / 0;
//   seam   one thread per joined pair across a tile edge: lock-free union of the two roots in global memory;
//   count  every tile-local root that is not its region's root adds its count to the root's: one global atomic
//          per (tile, region), not one per pixel;
//   apply  out = count[root] <= max_size ? 0 : v, and the mask cleared at the same pixels.
// Inside the seam pass every access to the labels is an agent-scope atomic (a relaxed load or an atomicMin): a
// plain load may be served from the CU's L1 with a value another CU has since lowered.  The count and apply
// passes read labels the seam pass finished before they started, so plain loads do.
// Every data-dependent loop has a trip cap from its monotone argument: a find walks strictly decreasing indices,
// so at most `cap` = the pixel count steps, and stops at any label that does not decrease (which also keeps every
// index it follows inside the plane); a union retries with a strictly smaller larger root, so at most `cap`
// times.  Correct code never reaches a cap; broken code gives a wrong map, not a hang.
#include "bm_common.h"
#include "bm_speckle_plan.h"

namespace sm {

namespace {

constexpr uint32_t kNoLabel = 0xFFFFFFFFu;
constexpr int kPerThread = kSpeckleTilePixels / kSpeckleThreads;

__device__ __forceinline__ bool joined(uint32_t a, uint32_t b, uint32_t max_diff) {
    const int d = (int)a - (int)b;
    return a != 0u && b != 0u && (uint32_t)(d < 0 ? -d : d) <= max_diff;
}

// The root of a: follows labels while they decrease, at most `cap` steps.  SCOPE: the memory scope of the loads
// (workgroup for LDS; agent for labels other workgroups lower while this runs).
template <int SCOPE>
__device__ __forceinline__ uint32_t find_root(const uint32_t* lab, uint32_t a, uint32_t cap) {
    for (uint32_t n = 0; n < cap; ++n) {
        const uint32_t l = __hip_atomic_load(lab + a, __ATOMIC_RELAXED, SCOPE);
        if (l >= a) break;
        a = l;
    }
    return a;
}

// Lock-free union of the regions of a and b: the larger root takes the smaller one as its label with an atomic
// min.  The atomic returning another value than that root means another thread linked the root first: both that
// link's target and ours must end up joined, so the union goes on from what the atomic returned.  Idempotent: two
// pixels already in one region find the same root and leave.
template <int SCOPE>
__device__ __forceinline__ void unite(uint32_t* lab, uint32_t a, uint32_t b, uint32_t cap) {
    for (uint32_t n = 0; n < cap; ++n) {
        a = find_root<SCOPE>(lab, a, cap);
        b = find_root<SCOPE>(lab, b, cap);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;   // < the root it was read as: the larger root strictly decreases from try to try
    }
}

// Root by plain loads: the labels are final (count and apply passes).
__device__ __forceinline__ uint32_t find_root_plain(const uint32_t* lab, uint32_t a, uint32_t cap) {
    for (uint32_t n = 0; n < cap; ++n) {
        const uint32_t l = lab[a];
        if (l >= a) break;
        a = l;
    }
    return a;
}

template <class T>
__global__ __launch_bounds__(kSpeckleThreads) void speckle_tile_kernel(const T* __restrict__ map, int W, int H,
                                                                       int pitch, int64_t fstride,
                                                                       uint32_t max_diff, uint32_t* __restrict__ label,
                                                                       uint32_t* __restrict__ count) {
    __shared__ uint32_t val[kSpeckleTilePixels];
    __shared__ uint32_t lab[kSpeckleTilePixels];
    __shared__ uint32_t cnt[kSpeckleTilePixels];
    const int x0 = blockIdx.x * kSpeckleTileW, y0 = blockIdx.y * kSpeckleTileH;
    const int64_t P = (int64_t)W * H;
    const T* src = map + (int64_t)blockIdx.z * fstride;
    label += (int64_t)blockIdx.z * P;
    count += (int64_t)blockIdx.z * P;
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = t + k * kSpeckleThreads;
        const int x = x0 + (i % kSpeckleTileW), y = y0 + (i / kSpeckleTileW);
        val[i] = (x < W && y < H) ? (uint32_t)src[(int64_t)y * pitch + x] : 0u;   // outside the frame: invalid
        lab[i] = (uint32_t)i;
        cnt[i] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = t + k * kSpeckleThreads;
        const uint32_t v = val[i];
        if (i % kSpeckleTileW < kSpeckleTileW - 1 && joined(v, val[i + 1], max_diff))
            unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, (uint32_t)i, (uint32_t)(i + 1), kSpeckleTilePixels);
        if (i / kSpeckleTileW < kSpeckleTileH - 1 && joined(v, val[i + kSpeckleTileW], max_diff))
            unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, (uint32_t)i, (uint32_t)(i + kSpeckleTileW), kSpeckleTilePixels);
    }
    __syncthreads();
    uint32_t root[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = t + k * kSpeckleThreads;
        root[k] = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, (uint32_t)i, kSpeckleTilePixels);
        if (val[i] != 0u) atomicAdd(&cnt[root[k]], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = t + k * kSpeckleThreads;
        const int x = x0 + (i % kSpeckleTileW), y = y0 + (i / kSpeckleTileW);
        if (x >= W || y >= H) continue;
        const int64_t p = (int64_t)y * W + x;
        const bool valid = val[i] != 0u;
        const uint32_t r = root[k];   // < kSpeckleTilePixels, a valid pixel of this tile: inside the frame
        const uint32_t g = (uint32_t)((int64_t)(y0 + (int)(r / kSpeckleTileW)) * W + x0 + (int)(r % kSpeckleTileW));
        label[p] = valid ? g : kNoLabel;
        count[p] = (valid && r == (uint32_t)i) ? cnt[i] : 0u;
    }
}

// Thread s of a frame: pair s of the vertical tile edges ((tiles_x - 1) * H pairs, left / right pixel), then of
// the horizontal ones ((tiles_y - 1) * W pairs, upper / lower pixel).
template <class T>
__global__ __launch_bounds__(kSpeckleThreads) void speckle_seam_kernel(const T* __restrict__ map, int W, int H,
                                                                       int pitch, int64_t fstride,
                                                                       uint32_t max_diff, int64_t vertical,
                                                                       int64_t pairs, uint32_t* label) {
    const int64_t s = (int64_t)blockIdx.x * kSpeckleThreads + threadIdx.x;
    if (s >= pairs) return;
    const int64_t P = (int64_t)W * H;
    const T* src = map + (int64_t)blockIdx.z * fstride;
    label += (int64_t)blockIdx.z * P;
    int x, y, x2, y2;
    if (s < vertical) {
        x = (int)(s / H + 1) * kSpeckleTileW - 1;
        y = (int)(s % H);
        x2 = x + 1;
        y2 = y;
    } else {
        const int64_t u = s - vertical;
        y = (int)(u / W + 1) * kSpeckleTileH - 1;
        x = (int)(u % W);
        x2 = x;
        y2 = y + 1;
    }
    if (x2 >= W || y2 >= H) return;   // (cannot happen for pairs from plan_speckle: kept as the bounds check)
    const uint32_t a = src[(int64_t)y * pitch + x], b = src[(int64_t)y2 * pitch + x2];
    if (!joined(a, b, max_diff)) return;
    unite<__HIP_MEMORY_SCOPE_AGENT>(label, (uint32_t)((int64_t)y * W + x), (uint32_t)((int64_t)y2 * W + x2),
                                    (uint32_t)P);
}

__global__ __launch_bounds__(kSpeckleThreads) void speckle_count_kernel(int64_t P, const uint32_t* __restrict__ label,
                                                                        uint32_t* count) {
    const int64_t p = (int64_t)blockIdx.x * kSpeckleThreads + threadIdx.x;
    if (p >= P) return;
    label += (int64_t)blockIdx.z * P;
    count += (int64_t)blockIdx.z * P;
    // Only a tile-local root has a count.  The adds of this pass go to region roots alone, and a region root adds
    // nothing itself: a count that is passed on is the tile pass's, never another thread's partial sum.
    const uint32_t c = count[p];
    if (c == 0u) return;
    const uint32_t r = find_root_plain(label, (uint32_t)p, (uint32_t)P);
    if (r != (uint32_t)p) atomicAdd(&count[r], c);
}

template <class T>
__global__ __launch_bounds__(kSpeckleThreads) void speckle_apply_kernel(T* map, int W, int H, int pitch,
                                                                        int64_t fstride, uint32_t max_size,
                                                                        const uint32_t* __restrict__ label,
                                                                        const uint32_t* __restrict__ count,
                                                                        uint8_t* mask) {
    const int64_t P = (int64_t)W * H;
    const int64_t p = (int64_t)blockIdx.x * kSpeckleThreads + threadIdx.x;
    if (p >= P) return;
    label += (int64_t)blockIdx.z * P;
    count += (int64_t)blockIdx.z * P;
    const uint32_t l = label[p];
    if (l > (uint32_t)p) return;   // kNoLabel: an invalid pixel stays as it is
    const uint32_t r = find_root_plain(label, l, (uint32_t)P);
    if (count[r] > max_size) return;
    const int y = (int)(p / W), x = (int)(p % W);
    map[(int64_t)blockIdx.z * fstride + (int64_t)y * pitch + x] = (T)0;
    if (mask) mask[(int64_t)blockIdx.z * P + p] = 0;
}

}  // namespace

template <class T>
hipError_t launch_speckle(T* map, int W, int H, int pitch, int64_t fstride, int batch, int max_size, int max_diff,
                          uint8_t* mask, uint32_t* label, uint32_t* count, hipStream_t s) {
    if (!speckle_pass_ok(W, H, batch) || pitch < W || max_size < 0 || max_diff < 0 || !map || !label || !count)
        return hipErrorInvalidValue;
    if (max_size == 0) return hipSuccess;   // no region has 0 pixels
    const SpecklePlan p = plan_speckle(W, H, batch);
    const int64_t P = (int64_t)W * H;
    const int64_t vertical = (int64_t)(p.tiles_x - 1) * H;
    for (int f0 = 0; f0 < batch; f0 += p.group) {
        const unsigned g = (unsigned)(batch - f0 < p.group ? batch - f0 : p.group);
        T* m = map + (int64_t)f0 * fstride;
        uint8_t* mk = mask ? mask + (int64_t)f0 * P : nullptr;
        hipLaunchKernelGGL(speckle_tile_kernel<T>, dim3((unsigned)p.tiles_x, (unsigned)p.tiles_y, g),
                           dim3(kSpeckleThreads), 0, s, m, W, H, pitch, fstride, (uint32_t)max_diff, label, count);
        if (p.seam_blocks > 0)
            hipLaunchKernelGGL(speckle_seam_kernel<T>, dim3((unsigned)p.seam_blocks, 1, g), dim3(kSpeckleThreads), 0, s,
                               m, W, H, pitch, fstride, (uint32_t)max_diff, vertical, p.seam_pairs, label);
        hipLaunchKernelGGL(speckle_count_kernel, dim3((unsigned)p.pixel_blocks, 1, g), dim3(kSpeckleThreads), 0, s, P,
                           label, count);
        hipLaunchKernelGGL(speckle_apply_kernel<T>, dim3((unsigned)p.pixel_blocks, 1, g), dim3(kSpeckleThreads), 0, s,
                           m, W, H, pitch, fstride, (uint32_t)max_size, label, count, mk);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template hipError_t launch_speckle<uint8_t>(uint8_t*, int, int, int, int64_t, int, int, int, uint8_t*, uint32_t*,
                                            uint32_t*, hipStream_t);
template hipError_t launch_speckle<uint16_t>(uint16_t*, int, int, int, int64_t, int, int, int, uint8_t*, uint32_t*,
                                             uint32_t*, hipStream_t);

}  // namespace sm
