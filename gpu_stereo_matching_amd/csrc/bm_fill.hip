// bm_fill.hip — the row fill: the holes the LR check and the speckle filter leave in a disparity map (0, this
// library's invalid value) are closed from their valid neighbours along the row, the classical last step of an SGM
// pipeline.
//
// The rule (include/sm_hip.h, "row fill"): a run is a maximal stretch of invalid pixels in one row; a run of at most
// max_gap pixels takes min(left neighbour, right neighbour), or the one neighbour it has at a border; valid pixels,
// longer runs and rows without a valid pixel stay.  The smaller value is the farther surface: the pixels the check
// removes next to a depth edge are the ones the nearer object hides in the other view.  Neighbours are valid pixels
// of the input, which the pass never changes, so the order in which runs are filled does not matter and the pass
// runs in place.
//
// One workgroup per row, one pixel per lane.  A row is walked in chunks of kFillChunk = 64 x 64 columns:
//   stage   each wave loads its 64-pixel segments, stages the values in LDS and writes one __ballot of "valid" per
//           segment: 64 masks of 64 bits describe the chunk;
//   scan    a second ballot over "segment has a valid pixel" gives every wave the chunk's non-empty segments.  The
//           nearest valid pixel left of a lane is the highest set bit below it in its segment's mask, else the last
//           bit of the nearest non-empty segment below, else the carry: the last valid pixel of the chunks before.
//           To the right it is the lowest set bit above, else the first bit of the nearest non-empty segment above;
//   write   an invalid pixel whose right neighbour lies in the chunk knows its run's ends, so its length and value:
//           it is written if the run is short enough.  Nothing else is written.
// A run whose right end lies in a later chunk waits: when a chunk's first valid pixel is found, the columns
// between the carry and the chunk's start, all invalid, are filled by the whole workgroup (their part inside the
// chunk is the scan's), and what is still open at the end of the row is a border run with a left neighbour only.
// So a row of any width takes the same two LDS arrays, and every pixel is read once and written at most once.
// Reads and writes stay inside [0, W) of the row: the bytes between width and pitch are neither neighbours nor
// written.
#include "bm_common.h"

namespace sm {

namespace {

constexpr int kFillSeg = 64;                         // one wave, one pixel per lane
constexpr int kFillChunk = kFillSeg * 64;            // the segments one second-level ballot covers
constexpr int kFillThreads = 256;                    // at most; a narrow row takes fewer waves (launch_fill)

__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }   // m != 0
__device__ __forceinline__ int low_bit(uint64_t m) { return __builtin_ctzll(m); }        // m != 0

template <class T>
__global__ __launch_bounds__(kFillThreads) void fill_rows_kernel(T* map, int W, int H, int pitch, int64_t fstride,
                                                                  int max_gap) {
    __shared__ T vals[kFillChunk];
    __shared__ uint64_t smask[kFillChunk / kFillSeg];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kFillSeg - 1), wave = tid / kFillSeg, nwave = nthr / kFillSeg;
    const int frame = (int)(blockIdx.x / (unsigned)H), y = (int)(blockIdx.x % (unsigned)H);
    T* row = map + (int64_t)frame * fstride + (int64_t)y * pitch;
    // the last valid pixel of the chunks walked so far: its column (-1: none yet) and value
    int carry_x = -1;
    uint32_t carry_v = 0u;
    for (int c0 = 0; c0 < W; c0 += kFillChunk) {
        const int n = W - c0 < kFillChunk ? W - c0 : kFillChunk;
        const int nseg = (n + kFillSeg - 1) / kFillSeg;
        for (int seg = wave; seg < nseg; seg += nwave) {
            const int i = seg * kFillSeg + lane;
            const T v = i < n ? row[c0 + i] : (T)0;   // past the row's end: invalid, and never written
            vals[i] = v;
            const uint64_t m = __ballot(v != (T)0);
            if (lane == 0) smask[seg] = m;
        }
        __syncthreads();
        const uint64_t nz = __ballot(lane < nseg && smask[lane] != 0ull);   // the chunk's non-empty segments
        for (int seg = wave; seg < nseg; seg += nwave) {
            const uint64_t m = smask[seg];
            // the segment's neighbours outside itself (the same for every lane): columns, -1 where none is known
            int lx = carry_x, rx = -1;
            uint32_t lv = carry_v, rv = 0u;
            const uint64_t below = nz & ((1ull << seg) - 1ull), above = nz & ~((2ull << seg) - 1ull);
            if (below) {
                const int s = top_bit(below), j = s * kFillSeg + top_bit(smask[s]);
                lx = c0 + j;
                lv = vals[j];
            }
            if (above) {
                const int s = low_bit(above), j = s * kFillSeg + low_bit(smask[s]);
                rx = c0 + j;
                rv = vals[j];
            }
            // the lane's own: a valid pixel of its segment is nearer than any outside
            const uint64_t lo = m & ((1ull << lane) - 1ull), hi = m & ~((2ull << lane) - 1ull);
            if (lo) {
                const int j = seg * kFillSeg + top_bit(lo);
                lx = c0 + j;
                lv = vals[j];
            }
            if (hi) {
                const int j = seg * kFillSeg + low_bit(hi);
                rx = c0 + j;
                rv = vals[j];
            }
            const int i = seg * kFillSeg + lane;
            if (i < n && !((m >> lane) & 1ull) && rx >= 0) {
                const int len = rx - lx - 1;   // lx == -1: the run starts at column 0
                if (len <= max_gap) row[c0 + i] = (T)(lx >= 0 && lv < rv ? lv : rv);
            }
        }
        if (nz) {
            const int sf = low_bit(nz), f = sf * kFillSeg + low_bit(smask[sf]);   // the chunk's first valid pixel
            const int a = carry_x + 1;
            if (a < c0) {   // a run from an earlier chunk ends at c0 + f - 1: its columns before this chunk
                const uint32_t fv = vals[f];
                if (c0 + f - a <= max_gap) {
                    const T v = (T)(carry_x >= 0 && carry_v < fv ? carry_v : fv);
                    for (int x = a + tid; x < c0; x += nthr) row[x] = v;
                }
            }
            const int sl = top_bit(nz), l = sl * kFillSeg + top_bit(smask[sl]);   // and its last
            carry_x = c0 + l;
            carry_v = vals[l];
        }
        __syncthreads();   // the next chunk overwrites vals and smask
    }
    // what is still open touches the right border: the left neighbour alone (none: the row has no valid pixel)
    const int a = carry_x + 1;
    if (carry_x >= 0 && a < W && W - a <= max_gap)
        for (int x = a + tid; x < W; x += nthr) row[x] = (T)carry_v;
}

}  // namespace

template <class T>
hipError_t launch_fill(T* map, int W, int H, int pitch, int64_t fstride, int batch, int max_gap, hipStream_t s) {
    if (!fill_pass_ok(W, H, batch) || pitch < W || max_gap < 0 || !map) return hipErrorInvalidValue;
    if (max_gap == 0) return hipSuccess;   // no run has 0 pixels
    const int waves = (W + kFillSeg - 1) / kFillSeg;
    const int threads = waves * kFillSeg < kFillThreads ? waves * kFillSeg : kFillThreads;
    hipLaunchKernelGGL(fill_rows_kernel<T>, dim3((unsigned)((int64_t)H * batch)), dim3((unsigned)threads), 0, s, map, W,
                       H, pitch, fstride, max_gap);
    return hipGetLastError();
}

template hipError_t launch_fill<uint8_t>(uint8_t*, int, int, int, int64_t, int, int, hipStream_t);
template hipError_t launch_fill<uint16_t>(uint16_t*, int, int, int, int64_t, int, int, hipStream_t);

}  // namespace sm
