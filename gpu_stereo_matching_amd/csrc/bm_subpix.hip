// bm_subpix.hip — sub-pixel WTA over a d-major cost volume (1/16 px, uint16), the uniqueness filter, the LR check
// on the 16-bit maps, and the reprojection of a 1/16-px map to 3-D points.
//
// A pixel's costs V(d), d = 0 .. dmax, give
//     d0    = the first (smallest) d at min V                                   (the 8-bit paths' d)
//     delta = floor((16 (a - c) + den) / (2 den)),  a = V(d0 - 1), b = V(d0), c = V(d0 + 1), den = a + c - 2 b
//             for 1 <= d0 < dmax, else 0: round-half-up of the parabola's vertex in 1/16 px, in [-8, 8]
//     q     = 16 d0 + delta
// d0 is the first minimum, so a > b and c >= b: den >= 1, and 16 (a - c) >= -16 den.  The division is done on the
// non-negative numerator 16 (a - c) + 33 den (the quotient plus 16).  For V < 2^24, the bound under which the
// (V << 8 | d) key of the 8-bit WTA fits 32 bits, den < 2^25 and the numerator is below 2^28 + 33 * 2^25 < 2^31;
// the uniqueness products V * (100 - u) and b * 100 stay below 2^31 too.  Every value is a 32-bit unsigned integer.
//
// Left view: dmax = min(D - 1, W - x).  Right view: V_R(u, d) = V(u + d, d), over u + 2 d <= W (the pairs of a volume
// that holds a cost only where x + d <= W: SGM's sums, the census cost) or over u + d < W (the AD SAD volume, which
// holds a window sum at every x: the pair set of the fused 8-bit box matcher's right view).
//
// SM_PAIRS_IN_VIEW with the minimum disparity dmin (SM_PARAM_MIN_DISP): plane k of the volume is d = dmin + k.  Left
// view: k <= min(D - 1, x - dmin).  Right view: V_R(u, k) = V(u + dmin + k, k) over u + dmin + k <= W - 1, for every
// volume.  d0 and q are absolute, d0 = dmin + k0 <= 4095 and q = 16 d0 + delta <= 65528, the parabola where
// 1 <= k0 < kmax; a pixel with no candidate (kmax < 0) is invalid, q = 0.  The check's two d0 planes are then 16-bit.
#include "bm_common.h"

namespace sm {
namespace {

struct Wta {
    uint32_t q, d0, valid;
};

// One view of one pixel: v[d * step], d = 0 .. dmax.  Lane = x and step = P (left) or P + 1 (right view, along
// u + d), so every d is one coalesced row segment.  V(d0 - 1) is carried, V(d0 + 1) is latched on the iteration
// after a new best: one pass.  The second walk runs only with the uniqueness filter on.  dmin: what plane 0 stands for.
template <typename T>
__device__ __forceinline__ Wta subpix_walk(const T* __restrict__ v, int64_t step, int dmax, uint32_t invalid_from,
                                           uint32_t uniq, uint32_t dmin) {
    if (dmax < 0) return Wta{0u, 0u, 0u};   // no candidate (SM_PAIRS_IN_VIEW, x < dmin): nothing is read
    uint32_t b = 0xFFFFFFFFu, a = 0, c = 0, prev = 0;
    int d0 = 0;
#pragma unroll 8
    for (int d = 0; d <= dmax; ++d) {
        const uint32_t cur = (uint32_t)v[d * step];
        c = d == d0 + 1 ? cur : c;
        const bool better = cur < b;   // strict: the first minimum stays
        a = better ? prev : a;
        d0 = better ? d : d0;
        b = better ? cur : b;
        prev = cur;
    }
    Wta r;
    r.d0 = (uint32_t)d0 + dmin;
    r.q = 16u * r.d0;
    if (d0 >= 1 && d0 < dmax) {
        const uint32_t den = a + c - 2u * b;
        r.q += (16u * a - 16u * c + 33u * den) / (2u * den) - 16u;   // the numerator is non-negative (header)
    }
    bool ok = invalid_from == 0u || b < invalid_from;
    if (uniq > 0u) {   // wave-uniform
        const uint32_t lim = b * 100u, f = 100u - uniq;
        bool rival = false;
#pragma unroll 8
        for (int d = 0; d <= dmax; ++d) {
            const uint32_t cur = (uint32_t)v[d * step];
            rival |= (d < d0 - 1 || d > d0 + 1) && cur * f < lim;
        }
        ok = ok && !rival;
    }
    r.valid = ok ? 1u : 0u;
    if (!ok) r.q = 0u, r.d0 = 0u;
    return r;
}

// right_pairs: 0 no right view, 1 u + 2 d <= W, 2 u + d < W, 3 SM_PAIRS_IN_VIEW's u + dmin + k <= W - 1.  (ka, kb): the
// left view's k <= min(D - 1, ka + kb * x) (Pairs, bm_common.h).  wide: dl / dr are uint16 planes.
// dl / dr (both or neither): the two views' d0 (0 where
// invalid) for subpix_lr_kernel, which then owns the mask; without them `mask` is the left view's validity.
template <typename T>
__global__ __launch_bounds__(256) void subpix_wta_kernel(const T* __restrict__ S, int W, int H, int D,
                                                         uint32_t invalid_from, uint32_t uniq, int right_pairs,
                                                         int ka, int kb, int dmin, int wide,
                                                         uint16_t* __restrict__ disp16, int pitch,
                                                         uint16_t* __restrict__ right16, uint8_t* __restrict__ mask,
                                                         uint8_t* __restrict__ dl, uint8_t* __restrict__ dr) {
    const int nxb = (W + 255) / 256;
    const int y = blockIdx.x / nxb, x = (blockIdx.x - y * nxb) * 256 + threadIdx.x;
    if (x >= W) return;
    const int64_t P = (int64_t)W * H;
    const int64_t p = (int64_t)y * W + x;
    const Wta l = subpix_walk(S + p, P, min(D - 1, ka + kb * x), invalid_from, uniq, (uint32_t)dmin);
    disp16[(int64_t)y * pitch + x] = (uint16_t)l.q;
    if (dl) {
        if (wide) reinterpret_cast<uint16_t*>(dl)[p] = (uint16_t)l.d0;
        else dl[p] = (uint8_t)l.d0;
    } else if (mask) {
        mask[p] = (uint8_t)l.valid;
    }
    if (right_pairs) {
        // x + dmin + rmax <= W - 1 (dmin is 0 unless right_pairs is 3)
        const int rmax = min(D - 1, right_pairs == 1 ? (W - x) / 2 : W - 1 - x - dmin);
        const Wta r = subpix_walk(S + p + dmin, P + 1, rmax, 0u, uniq, (uint32_t)dmin);
        if (right16) right16[p] = (uint16_t)r.q;
        if (dr) {
            if (wide) reinterpret_cast<uint16_t*>(dr)[p] = (uint16_t)r.d0;
            else dr[p] = (uint8_t)r.d0;
        }
    }
}

// The LR check of launch_lr_check on the views' d0: occluded when x - d < 0, d == 0 or |d - d0_R(x - d)| > 1.
// An occluded pixel's q becomes 0; the mask (optional) is !occluded.
template <typename DT>   // uint8_t, or uint16_t with SM_PAIRS_IN_VIEW (d0 up to 4095)
__global__ __launch_bounds__(256) void subpix_lr_kernel(const DT* __restrict__ dl, const DT* __restrict__ dr,
                                                        int W, int H, uint16_t* __restrict__ disp16, int pitch,
                                                        uint8_t* __restrict__ mask) {
    const int nxb = (W + 255) / 256;
    const int y = blockIdx.x / nxb, x = (blockIdx.x - y * nxb) * 256 + threadIdx.x;
    if (x >= W) return;
    const int64_t row = (int64_t)y * W;
    const int d = dl[row + x];
    bool occ = true;
    if (d != 0 && x - d >= 0) {
        const int diff = d - (int)dr[row + x - d];
        occ = diff > 1 || diff < -1;
    }
    if (occ) disp16[(int64_t)y * pitch + x] = 0;
    if (mask) mask[row + x] = (uint8_t)!occ;
}

struct QMat {
    double m[16];
};

// reprojectImageTo3D of a 1/16-px map: (X, Y, Z, w) = Q (x, y, q / 16, 1) in double, (X, Y, Z) / w rounded once to
// fp32; q == 0 or w == 0 gives (0, 0, 0).  A block's 256 pixels go through LDS so that the 3072 B leave as three
// runs of contiguous dwords.
__global__ __launch_bounds__(256) void reproject_kernel(const uint16_t* __restrict__ disp16, int W, int H, int pitch,
                                                        QMat Q, float* __restrict__ xyz, int xyz_pitch) {
    __shared__ float out[3 * 256];
    const int nxb = (W + 255) / 256;
    const int y = blockIdx.x / nxb, x0 = (blockIdx.x - y * nxb) * 256, x = x0 + threadIdx.x;
    float X = 0.f, Y = 0.f, Z = 0.f;
    if (x < W) {
        const uint32_t q = disp16[(int64_t)y * pitch + x];
        const double d = (double)q * 0.0625, fx = (double)x, fy = (double)y;
        const double w = Q.m[12] * fx + Q.m[13] * fy + Q.m[14] * d + Q.m[15];
        if (q != 0u && w != 0.0) {
            X = (float)((Q.m[0] * fx + Q.m[1] * fy + Q.m[2] * d + Q.m[3]) / w);
            Y = (float)((Q.m[4] * fx + Q.m[5] * fy + Q.m[6] * d + Q.m[7]) / w);
            Z = (float)((Q.m[8] * fx + Q.m[9] * fy + Q.m[10] * d + Q.m[11]) / w);
        }
    }
    out[3 * threadIdx.x] = X;
    out[3 * threadIdx.x + 1] = Y;
    out[3 * threadIdx.x + 2] = Z;
    __syncthreads();
    const int n = 3 * min(256, W - x0);
    float* row = xyz + (int64_t)y * xyz_pitch + 3 * x0;
    for (int i = threadIdx.x; i < n; i += 256) row[i] = out[i];
}

template <typename T>
hipError_t launch_subpix(const T* vol, int W, int H, int D, uint32_t invalid_from, int uniq, int right_pairs, bool lr,
                         uint16_t* disp16, int pitch, uint16_t* right16, uint8_t* mask, uint8_t* scratch,
                         hipStream_t s, const Pairs& pr) {
    const int64_t blocks = (int64_t)((W + 255) / 256) * H;
    if (W <= 0 || H <= 0 || D < 1 || D > kMaxDisp || pitch < W || blocks > 0x7FFFFFFF || uniq < 0 || uniq > 99 ||
        !vol || !disp16 || (lr && !scratch) || !pr.ok(D, 4095))
        return hipErrorInvalidValue;
    if (!lr && !right16) right_pairs = 0;
    else if (pr.in_view) right_pairs = 3;
    else if (right_pairs != 2) right_pairs = 1;
    const int wide = pr.in_view;   // the check's d0 planes: uint16 each
    uint8_t* dl = lr ? scratch : nullptr;
    uint8_t* dr = lr ? scratch + (int64_t)W * H * (wide ? 2 : 1) : nullptr;
    hipLaunchKernelGGL(subpix_wta_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, vol, W, H, D, invalid_from,
                       (uint32_t)uniq, right_pairs, pr.ka(W), pr.kb(), pr.d0, wide, disp16, pitch, right16, mask, dl,
                       dr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !lr) return e;
    if (wide)
        hipLaunchKernelGGL(subpix_lr_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, s,
                           reinterpret_cast<const uint16_t*>(dl), reinterpret_cast<const uint16_t*>(dr), W, H, disp16,
                           pitch, mask);
    else
        hipLaunchKernelGGL(subpix_lr_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, s, dl, dr, W, H, disp16,
                           pitch, mask);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_subpix_wta_u32(const uint32_t* vol, int W, int H, int D, uint32_t invalid_from, int uniq,
                                 int right_pairs, bool lr, uint16_t* disp16, int pitch, uint16_t* right16,
                                 uint8_t* mask, uint8_t* scratch, hipStream_t s, const Pairs& pr) {
    return launch_subpix(vol, W, H, D, invalid_from, uniq, right_pairs, lr, disp16, pitch, right16, mask, scratch, s,
                         pr);
}

hipError_t launch_subpix_wta_u16(const uint16_t* vol, int W, int H, int D, uint32_t invalid_from, int uniq,
                                 int right_pairs, bool lr, uint16_t* disp16, int pitch, uint16_t* right16,
                                 uint8_t* mask, uint8_t* scratch, hipStream_t s, const Pairs& pr) {
    return launch_subpix(vol, W, H, D, invalid_from, uniq, right_pairs, lr, disp16, pitch, right16, mask, scratch, s,
                         pr);
}

hipError_t launch_reproject(const uint16_t* disp16, int W, int H, int pitch, const double* Q, float* xyz,
                            int xyz_pitch, hipStream_t s) {
    const int64_t blocks = (int64_t)((W + 255) / 256) * H;
    if (W <= 0 || H <= 0 || pitch < W || xyz_pitch < 3 * (int64_t)W || blocks > 0x7FFFFFFF || !disp16 || !Q || !xyz)
        return hipErrorInvalidValue;
    QMat q;
    for (int i = 0; i < 16; ++i) q.m[i] = Q[i];
    hipLaunchKernelGGL(reproject_kernel, dim3((unsigned)blocks), dim3(256), 0, s, disp16, W, H, pitch, q, xyz,
                       xyz_pitch);
    return hipGetLastError();
}

}  // namespace sm
