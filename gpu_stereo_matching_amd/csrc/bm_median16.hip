// bm_median16.hip — the (2r+1)^2 median of a 1/16-px map (uint16), and the LR check of the sub-pixel calls on two
// filtered maps.  bm_post.hip's median_kernel is a radix select over 8 bits whose packed counting trick,
// lane = 0x100 + v - cand, needs a spare ninth bit in each 16-bit lane; a 16-bit value leaves none.  Here the packed
// compare is a saturating subtraction instead.
//
// median16_kernel<R>: a 64 x 32 output tile per workgroup; the (32 + 2R) x (64 + 2R) input tile is staged once in LDS
// with clamped coordinates (replicate borders).  Each thread owns one column and 8 consecutive rows.  Per output
// pixel each window row's 2R + 1 values are packed into R + 1 dwords of two u16 (plus one dummy of 0xFFFF), and a
// radix select over the 16 bits, most significant first, keeps the largest `ans` with
//     #{v < ans} <= T,  T = 2R^2 + 2R,
// which is the element of rank T (0-based).  Per dword and bit: v_pk_sub_u16 with clamp, max(cand - v, 0), which is
// non-zero exactly where v < cand; v_pk_min_u16 with 1; one add into two 16-bit counts.  Three instructions for two
// values, none of which writes a condition mask.  0 and 0xFFFF are values like any other.  The row loop is a real
// loop (the window is re-read from LDS), so the code is one unrolled select and every register index is a constant:
// no scratch.  Integer throughout, so bit-exact.
#include "bm_common.h"

namespace sm {
namespace {

constexpr int kTW = 64, kTH = 32, kRows = 8;   // tile, rows per thread
typedef uint16_t us2 __attribute__((ext_vector_type(2)));

// min(max(a - b, 0), 1) in both 16-bit halves: 1 where b < a.  Written as the two instructions: from
// __builtin_elementwise_sub_sat and _min the compiler makes 16-bit compares and selects, each compare followed by a
// wait state for the mask it writes, more than half of the issue slots.
__device__ __forceinline__ uint32_t pk_below(us2 a, us2 b, uint32_t ones) {
    uint32_t d;
    asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(d) : "v"(a), "v"(b));
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(d) : "v"(d), "v"(ones));
    return d;
}

template <int R>
__global__ __launch_bounds__(256) void median16_kernel(const uint16_t* __restrict__ src, int W, int H, int pitch,
                                                       int64_t stride, uint16_t* __restrict__ dst, int dpitch,
                                                       int64_t dstride, int tiles_x, int tiles) {
    constexpr int SW = kTW + 2 * R, SH = kTH + 2 * R;
    constexpr int K = 2 * R + 1;
    constexpr int T = 2 * R * R + 2 * R;   // rank of the median (0-based)
    constexpr int SEG = R + 1;             // packed words per window row: 2R + 1 values and one dummy
    __shared__ uint16_t tile[SH][SW];

    const int frame = blockIdx.x / tiles;
    const int t = blockIdx.x - frame * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const uint16_t* S = src + (int64_t)frame * stride;
    for (int e = threadIdx.x; e < SH * SW; e += 256) {
        const int i = e / SW, j = e - (e / SW) * SW;
        int y = y0 - R + i, x = x0 - R + j;
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        tile[i][j] = S[(int64_t)y * pitch + x];
    }
    __syncthreads();

    const int c = threadIdx.x & 63;               // output column in the tile
    const int r0 = (threadIdx.x >> 6) * kRows;    // first output row in the tile
    const int x = x0 + c;
    uint16_t* D = dst + (int64_t)frame * dstride;
#pragma unroll 1
    for (int o = 0; o < kRows; ++o) {
        const int y = y0 + r0 + o;
        if (y >= H) break;   // uniform per wave: a wave's lanes share r0
        us2 w[K][SEG];
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                w[i][k].x = tile[r0 + o + i][c + 2 * k];
                w[i][k].y = 2 * k + 1 < K ? tile[r0 + o + i][c + 2 * k + 1] : (uint16_t)0xFFFF;   // never < cand
            }
        uint32_t ans = 0;
#pragma unroll
        for (int bit = 15; bit >= 0; --bit) {
            const uint32_t cand = ans | (1u << bit);
            const us2 c2 = {(uint16_t)cand, (uint16_t)cand};
            uint32_t acc = 0;   // two 16-bit counts of at most (2R+1)(R+1) <= 28: no carry between them
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int k = 0; k < SEG; ++k)
                    acc += pk_below(c2, w[i][k], 0x00010001u);
            const uint32_t lt = (acc & 0xFFFFu) + (acc >> 16);
            ans = lt <= (uint32_t)T ? cand : ans;
        }
        if (x < W) D[(int64_t)y * dpitch + x] = (uint16_t)ans;
    }
}

// The sub-pixel calls' last step on two filtered maps (SM_PARAM_SUBPIX_MEDIAN): the LR check of subpix_lr_kernel on
// d = (q + 8) >> 4, the 1/16-px values rounded to whole disparities, of the left map and of the dense right map rq
// (null: no check).  Occluded when x - d < 0, d == 0 or |d - d_R(x - d)| > 1; an occluded pixel's q becomes 0.  mask
// (optional) = final q != 0.  d reaches 4096 with SM_PAIRS_IN_VIEW: int arithmetic.
__global__ __launch_bounds__(256) void subpix_lr_q_kernel(const uint16_t* __restrict__ rq, int W, int H,
                                                          uint16_t* __restrict__ disp16, int pitch,
                                                          uint8_t* __restrict__ mask) {
    const int nxb = (W + 255) / 256;
    const int y = blockIdx.x / nxb, x = (blockIdx.x - y * nxb) * 256 + threadIdx.x;
    if (x >= W) return;
    const int64_t row = (int64_t)y * W;
    uint16_t* q = disp16 + (int64_t)y * pitch + x;
    uint32_t v = *q;
    if (rq) {
        const int d = (int)((v + 8u) >> 4);
        bool occ = true;
        if (d != 0 && x - d >= 0) {
            const int diff = d - (int)(((uint32_t)rq[row + x - d] + 8u) >> 4);
            occ = diff > 1 || diff < -1;
        }
        if (occ) {
            v = 0;
            *q = 0;
        }
    }
    if (mask) mask[row + x] = (uint8_t)(v != 0u);
}

}  // namespace

hipError_t launch_median16(const uint16_t* src, int W, int H, int pitch, int64_t stride, int batch, int radius,
                           uint16_t* dst, int dpitch, int64_t dstride, hipStream_t s) {
    if (!median16_pass_ok(W, H, batch) || pitch < W || dpitch < W || !src || !dst || src == dst)
        return hipErrorInvalidValue;
    const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
    const dim3 g((unsigned)((int64_t)tiles_x * tiles_y * batch)), b(256);
    switch (radius) {
        case 1: hipLaunchKernelGGL(median16_kernel<1>, g, b, 0, s, src, W, H, pitch, stride, dst, dpitch, dstride, tiles_x, tiles_x * tiles_y); break;
        case 2: hipLaunchKernelGGL(median16_kernel<2>, g, b, 0, s, src, W, H, pitch, stride, dst, dpitch, dstride, tiles_x, tiles_x * tiles_y); break;
        case 3: hipLaunchKernelGGL(median16_kernel<3>, g, b, 0, s, src, W, H, pitch, stride, dst, dpitch, dstride, tiles_x, tiles_x * tiles_y); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_subpix_lr_q(const uint16_t* right_q, int W, int H, uint16_t* disp16, int pitch, uint8_t* mask,
                              hipStream_t s) {
    const int64_t blocks = (int64_t)((W + 255) / 256) * H;
    if (W <= 0 || H <= 0 || pitch < W || blocks > 0x7FFFFFFF || !disp16) return hipErrorInvalidValue;
    if (!right_q && !mask) return hipSuccess;   // nothing to do: no launch
    hipLaunchKernelGGL(subpix_lr_q_kernel, dim3((unsigned)blocks), dim3(256), 0, s, right_q, W, H, disp16, pitch, mask);
    return hipGetLastError();
}

}  // namespace sm
