// bm_census.hip — the census matching cost (SM_COST_CENSUS): the 9 x 7 census transform and the
// Hamming cost volume that takes the AD volume's place in front of launch_box_sad_volume.
//
//   census(y, x): uint64; the neighbours dx in [-4, 4], dy in [-3, 3] row-major (dy outer), centre skipped, on
//                 bits 0..61; bit = I(clamp(y + dy), clamp(x + dx)) < I(y, x) (replicated border); bits 62-63 0
//   ham[d][y][x] = popcount(censusL(y, x) ^ censusR(y, x - d)) for x >= d, 0 otherwise: u8 <= 62, d-major planes
//                 [D][H][W], the layout and zero rule of ad_volume_kernel (bm_volume.hip)
#include <algorithm>

#include "bm_common.h"

namespace sm {
namespace {

constexpr int kCDX = 4, kCDY = 3;   // the window's half extents: 9 wide, 7 high

// ---- census transform: one block per 64 x 16 tile, staged once in LDS with the 4 / 3 halo ----
// The clamp of the replicated border is applied while staging, so the compares read the tile unconditionally.
// Thread (tx, ty) of the 64 x 4 block owns column tx of rows ty, ty + 4, ty + 8, ty + 12 and builds each word's
// two 32-bit halves: window index i = (dy + 3) * 9 + (dx + 4) goes to bit i below the centre (i = 31) and to
// bit i - 1 above it, so the low half holds i = 0..30 and 32, the high half i = 33..62.  A wave's 64 lanes read
// 64 consecutive bytes of a tile row (16 banks, no conflict); the words leave as one 512-B row segment per wave.
constexpr int kCTW = 64, kCTH = 16;
constexpr int kCLW = kCTW + 2 * kCDX + 4;   // tile row stride in bytes (72 used, a multiple of 4)
__global__ __launch_bounds__(256) void census_kernel(const uint8_t* __restrict__ img, int W, int H, int pitch,
                                                     uint64_t* __restrict__ out) {
    __shared__ uint8_t tile[(kCTH + 2 * kCDY) * kCLW];
    const int x0 = blockIdx.x * kCTW, y0 = blockIdx.y * kCTH;
    constexpr int kCols = kCTW + 2 * kCDX, kRows = kCTH + 2 * kCDY;
    for (int e = threadIdx.x; e < kRows * kCols; e += 256) {
        const int i = e / kCols, j = e - i * kCols;
        const int yy = min(max(y0 - kCDY + i, 0), H - 1), xx = min(max(x0 - kCDX + j, 0), W - 1);
        tile[i * kCLW + j] = img[(int64_t)yy * pitch + xx];
    }
    __syncthreads();
    const int tx = threadIdx.x & (kCTW - 1), ty = threadIdx.x / kCTW;
    const int x = x0 + tx;
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < kCTH / 4; ++k) {
        const int ly = ty + 4 * k, y = y0 + ly;
        if (y >= H) break;
        const uint8_t* t = tile + ly * kCLW + tx;   // the window's top-left corner (dy = -3, dx = -4)
        const uint32_t c = t[kCDY * kCLW + kCDX];
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 63; ++i) {
            if (i == 31) continue;
            const uint32_t b = (uint32_t)t[(i / 9) * kCLW + i % 9] < c ? 1u : 0u;
            const int bit = i < 31 ? i : i - 1;
            if (bit < 32) lo |= b << bit;
            else hi |= b << (bit - 32);
        }
        out[(int64_t)y * W + x] = ((uint64_t)hi << 32) | lo;
    }
}

// ---- Hamming volume: one block per (band of RB rows, d chunk), the counterpart of ad_volume_kernel ----
// Write-bound (P * D bytes out, 16 P in).  The band's right-image census words sit in LDS (<= 4096 x 8 B per row), so
// cR(x - d) never goes back to HBM.  A thread owns one 16-column segment of a band row: its 16 cL words stay in
// registers, and so does the window of the 16 cR words under them, cR(x0 - d .. x0 - d + 15).  Stepping d by one
// moves that window one word down: one LDS read per d, into the slot of the word that left (the slots form a ring
// whose rotation the 16-fold unrolled d loop resolves at compile time).  Per d the thread forms its 16 popcounts,
// packs them into four dwords and stores them: one 16-B store where the planes are 16-B aligned (VEC), else
// dword stores at 4-B aligned addresses and byte stores for the rest and for the row's tail.
// LDS index of word x is x + (x >> 4): the lanes of a wave read words 16 apart, 17 words = 34 banks with the
// padding, which spreads the 32 lanes of a ds_read_b64 group over all 64 banks (128-B strides would put them on two).
// With RB * nseg segments per block: 256 / (RB * nseg) groups of threads each walk a contiguous share of the
// chunk's disparities.  Bytes at x < d are 0, as the AD volume's.
// d0 (SM_PARAM_MIN_DISP, the matching calls with SM_PAIRS_IN_VIEW alone; the public volume calls pass 0): plane k holds
// the disparity d0 + k, which is plane k of the d0 = 0 volume of a frame whose columns are numbered from -d0: the ring
// and the masks take the segment's first column as xr = x0 - d0 and nothing else changes.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kHT = 256;
constexpr int kHSeg = 16;
// d chunks per band, as ad_volume_kernel's SM_ADV_MAXSPLIT.  Same-box A/B at 1080p D = 128 (hipEvents around the two
// census launches and this kernel, three alternating rounds): 2 chunks 145 us, 4 chunks 148 us, 8 chunks 177 us
constexpr int kHamSplit = 2;

__host__ __device__ __forceinline__ int lds_word(int x) { return x + (x >> 4); }

// Four waves per SIMD, 128 VGPRs, is what the VEC form compiled to before xr; with it the allocator stops at 130,
// a fifth granule and three waves, unless it is told the target (no scratch either way)
template <bool VEC>
__global__ __launch_bounds__(kHT) __attribute__((amdgpu_waves_per_eu(4))) void census_volume_kernel(const uint64_t* __restrict__ cL,
                                                            const uint64_t* __restrict__ cR, int W, int H, int D,
                                                            int RB, int dsp, int d0, uint8_t* __restrict__ ham) {
    extern __shared__ __attribute__((aligned(16))) uint64_t rrow[];   // [RB][rstride]
    const int y0 = blockIdx.x * RB;
    const int dc = (D + dsp - 1) / dsp;
    const int d_begin = blockIdx.y * dc, d_end = min(D, d_begin + dc);
    const int nseg = (W + kHSeg - 1) / kHSeg;
    const int rstride = lds_word(W - 1) + 1;
    const int rows = min(RB, H - y0);
    for (int e = threadIdx.x; e < rows * W; e += kHT) {
        const int i = e / W, x = e - i * W;
        rrow[i * rstride + lds_word(x)] = cR[(int64_t)(y0 + i) * W + x];
    }
    __syncthreads();
    const int nflat = rows * nseg;                       // <= kHT (the launcher's choice of RB)
    const int groups = kHT / nflat;
    const int g = threadIdx.x / nflat;
    if (g >= groups) return;
    const int fl = threadIdx.x - g * nflat;
    const int i = fl / nseg, x0 = (fl - i * nseg) * kHSeg;
    const int dg = (d_end - d_begin + groups - 1) / groups;
    const int lo = d_begin + g * dg, hi = min(d_end, lo + dg);
    if (lo >= hi) return;
    const int xr = x0 - d0;                              // the segment's first column as the right image sees it
    const int y = y0 + i;
    const int n = min(kHSeg, W - x0);                    // columns of this segment inside the row
    uint64_t l[kHSeg], w[kHSeg];
    const uint64_t* lrow = cL + (int64_t)y * W + x0;
    const uint64_t* rr = rrow + i * rstride;
#pragma unroll
    for (int k = 0; k < kHSeg; ++k) {
        l[k] = k < n ? lrow[k] : 0ull;
        // columns left of d (masked below) and right of the row (never stored) read a clamped word
        w[k] = rr[lds_word(min(max(xr + k - lo, 0), W - 1))];
    }
    const int64_t P = (int64_t)W * H;
    uint8_t* dst = ham + (int64_t)lo * P + (int64_t)y * W + x0;   // this segment in plane d, from d = lo on
    // one disparity: the segment's 16 Hamming distances with the ring at rotation j, masked and stored
    auto emit = [&](int d, int j) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = 4 * q + b;
                v |= (uint32_t)__popcll(l[k] ^ w[(k - j) & (kHSeg - 1)]) << (8 * b);
            }
            o[q] = v;
        }
        if (xr < d) {   // dword q drops its low clamp(d - xr - 4q, 0, 4) bytes
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nz = min(max(d - xr - 4 * q, 0), 4);
                o[q] &= (uint32_t)(~0ull << (8 * nz));
            }
        }
        if (VEC) {   // W % 16 == 0 and a 16-B aligned volume: every segment is whole and aligned
            const u32x4 v = {o[0], o[1], o[2], o[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst));
        } else if (n == kHSeg && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) reinterpret_cast<uint32_t*>(dst)[q] = o[q];
        } else {
            for (int b = 0; b < n; ++b) dst[b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
        }
        dst += P;
    };
    // whole runs of 16 disparities: no exit inside the unrolled run, so the ring's rotation costs no moves, and
    // after the run it is back at rotation 0
    int db = lo;
    for (; db + kHSeg <= hi; db += kHSeg) {
#pragma unroll
        for (int j = 0; j < kHSeg; ++j) {
            const int d = db + j;
            if (j > 0 || db > lo) w[(kHSeg - j) & (kHSeg - 1)] = rr[lds_word(max(xr - d, 0))];
            emit(d, j);
        }
    }
    // the last, shorter run: the window moves through the registers instead.  At its first d the ring, back at
    // rotation 0, already holds words 1..15 of that d (a whole run leaves them so), or the initial fill
    for (int d = db; d < hi; ++d) {
        if (d > db) {
#pragma unroll
            for (int k = kHSeg - 1; k > 0; --k) w[k] = w[k - 1];
        }
        if (d > lo) w[0] = rr[lds_word(max(xr - d, 0))];
        emit(d, 0);
    }
}

}  // namespace

hipError_t launch_census(const uint8_t* img, int W, int H, int pitch, uint64_t* census, hipStream_t s) {
    if (!img || !census || W <= 0 || H <= 0 || pitch < W) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((W + kCTW - 1) / kCTW), (unsigned)((H + kCTH - 1) / kCTH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(census_kernel, grid, dim3(256), 0, s, img, W, H, pitch, census);
    return hipGetLastError();
}

hipError_t launch_census_volume(const uint64_t* cL, const uint64_t* cR, int W, int H, int D, uint8_t* ham,
                                hipStream_t s, int d0) {
    if (!cL || !cR || !ham || W <= 0 || W > 4096 || H <= 0 || D < 1 || D > kMaxDisp || d0 < 0 || d0 > 4095)
        return hipErrorInvalidValue;
    const int nseg = (W + kHSeg - 1) / kHSeg;            // <= 256 = kHT
    int rb = 2 * nseg <= kHT ? 2 : 1;
    if (rb > H) rb = H;
    const size_t lds = (size_t)rb * (size_t)(lds_word(W - 1) + 1) * sizeof(uint64_t);   // <= 34.8 KB
    const int dsplit = std::max(1, std::min(D, kHamSplit));
    const dim3 grid((unsigned)((H + rb - 1) / rb), (unsigned)dsplit);
    const bool vec = W % kHSeg == 0 && (reinterpret_cast<uintptr_t>(ham) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(census_volume_kernel<true>, grid, dim3(kHT), lds, s, cL, cR, W, H, D, rb, dsplit, d0, ham);
    else
        hipLaunchKernelGGL(census_volume_kernel<false>, grid, dim3(kHT), lds, s, cL, cR, W, H, D, rb, dsplit, d0, ham);
    return hipGetLastError();
}

}  // namespace sm
