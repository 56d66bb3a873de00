// bm_sgm.hip — semi-global matching (SM_AGG_SGM): four- or eight-path aggregation of the u16 box SAD volume and
// the WTA over its sum (the diagonals §31).
//
// The recursion of one path direction rho, with q = p - rho the previous pixel on the path:
//     L(p, d) = C(p, d)                                                              q outside the image
//     L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + P1, L(q, d+1) + P1, M + P2) - M   M = min_k L(q, k)
// over the pairs (x, d) that exist (x + d <= W, Device.cu:44; with SM_PAIRS_IN_VIEW x - d >= 0, below).  A pair that
// does not exist is carried as kInf, which loses every min, so the "dropped terms" of the definition need no
// branches.  L <= C + P2 fits u16 (the entry points check 255 * win^2 + P2 <= 65535); the sum S of the four
// directions (+-1, 0), (0, +-1), and
// with SM_PARAM_SGM_PATHS 8 of the four diagonals (+-1, +-1) too, is u32 [D][H][W] (< 2^18, with eight < 2^19),
// zeroed by the caller and accumulated with no-return global atomic adds, so the directions need no
// order among themselves and integer addition keeps the sum exact.
//
// Which pairs exist is a prefix of the planes at every column, k <= dmax(x) = min(D - 1, ka + kb * x): the kernels
// take (ka, kb) as arguments, (W, -1) for the reference's rule and (-d0, +1) for SM_PAIRS_IN_VIEW, where plane k
// stands for d = d0 + k (SM_PARAM_MIN_DISP) and dmax is negative at the columns x < d0, which have no candidate.
// A previous pixel q with no existing k acts as a q outside the image: every L(q, .) is kInf, so M = kInf,
// min(...) = kInf as well (kInf + P < 2^21, no wrap) and min(...) - M = 0, L(p, .) = C(p, .), without a branch.
#include "bm_common.h"

namespace sm {
namespace {

constexpr uint32_t kInf = 1u << 20;   // "does not exist": above any L + penalty (< 2^17), far from overflow
constexpr int kTX = 64;               // columns per staged tile of the horizontal scan

// DPP controls (gfx9): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror, wave_shl:1, wave_shr:1
constexpr int kDppQuadSwap1 = 0xB1, kDppQuadSwap2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_min(uint32_t v) {
    return min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false));
}

// min over the 64 lanes of a fully active wave, as a wave-uniform value: four DPP steps leave each row of
// 16 lanes holding its min, one lane of each row is read back and the rest is scalar
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = dpp_min<kDppQuadSwap1>(v);
    v = dpp_min<kDppQuadSwap2>(v);
    v = dpp_min<kDppHalfMirror>(v);
    v = dpp_min<kDppMirror>(v);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// lane i receives lane i - 1's value (lane 0: kInf) / lane i + 1's value (lane 63: kInf)
__device__ __forceinline__ uint32_t from_lane_below(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)kInf, (int)v, kDppWaveShr1, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t from_lane_above(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)kInf, (int)v, kDppWaveShl1, 0xF, 0xF, false);
}

// The recursion's min for register j of a lane's N consecutive d: Lp is L(q, .) of those d, lo and hi are L(q, .) of
// the d below the lane's first and above its last.  The caller finishes the update, L = restart ? C : C + best - M;
// with that select in here the column kernel compiles to more registers.
template <int N>
__device__ __forceinline__ uint32_t path_best(const uint32_t (&Lp)[N], int j, uint32_t lo, uint32_t hi, uint32_t M,
                                              uint32_t P1, uint32_t P2) {
    const uint32_t below = j > 0 ? Lp[j > 0 ? j - 1 : 0] : lo;
    const uint32_t above = j < N - 1 ? Lp[j < N - 1 ? j + 1 : 0] : hi;
    return min(min(Lp[j], below + P1), min(above + P1, M + P2));
}

// ---- horizontal paths: one wave per (row, direction), disparities across the lanes ----
// Lane l holds d = l * NJ .. l * NJ + NJ - 1 (NJ = ceil(D / 64)): d +- 1 is a register of the same lane
// except at the lane's two ends, which take one wave shift each; M is the lanes' min (wave_min).  The volume
// is d-major, so the row goes through LDS in tiles of 64 columns: each d's 64 costs are one coalesced 128-B
// row load, the scan overwrites the tile's C with L in place, and the tile leaves as one 256-B row of atomic
// adds per d.  Lane l's costs start at l * LS u16 with LS / 2 = 32 NJ + 1 dwords, odd, so the scan's u16
// reads and writes (one column of the tile, all d) touch each bank once per 32-lane half.
// VEC (W % 8 == 0, so every row segment is 16-B aligned): the tile is staged with 16-B loads, 8 lanes per d
// and 8 d per instruction, all of a tile's loads in flight together; other widths load u16 per lane.
template <int NJ, bool VEC>
__global__ __launch_bounds__(64) void sgm_h_kernel(const uint16_t* __restrict__ C, int W, int H, int D, uint32_t P1,
                                                   uint32_t P2, int ka, int kb, uint32_t* __restrict__ S) {
    constexpr int LS = NJ * kTX + 2;
    __shared__ __align__(16) uint16_t tile[64 * LS];
    const int lane = threadIdx.x;
    const int y = blockIdx.x;
    const int dir = blockIdx.y;   // 0: rho = (+1, 0), left to right; 1: rho = (-1, 0)
    const int64_t P = (int64_t)W * H;
    const int64_t row = (int64_t)y * W;
    const int nt = (W + kTX - 1) / kTX;
    uint32_t Lp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) Lp[j] = kInf;
    bool first = true;
    for (int ti = 0; ti < nt; ++ti) {
        const int t = dir ? nt - 1 - ti : ti;
        const int x0 = t * kTX;
        const int n = min(kTX, W - x0);
        if (VEC) {
            const int xc = (lane & 7) * 8;
            if (xc < n) {   // n is a multiple of 8 here
#pragma unroll 16
                for (int d = lane >> 3; d < D; d += 8) {
                    const uint4 v = *reinterpret_cast<const uint4*>(C + d * P + row + x0 + xc);
                    uint32_t* o = reinterpret_cast<uint32_t*>(tile + (d / NJ) * LS + (d % NJ) * kTX + xc);
                    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
                }
            }
        } else if (lane < n) {
#pragma unroll 32
            for (int d = 0; d < D; ++d) tile[(d / NJ) * LS + (d % NJ) * kTX + lane] = C[d * P + row + x0 + lane];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const int xi = dir ? n - 1 - i : i;
            const int dmax = min(D - 1, ka + kb * (x0 + xi));   // d <= dmax exist at this column
            uint32_t m = Lp[0];
#pragma unroll
            for (int j = 1; j < NJ; ++j) m = min(m, Lp[j]);
            const uint32_t M = wave_min(m);
            const uint32_t lo = from_lane_below(Lp[NJ - 1]), hi = from_lane_above(Lp[0]);
            uint32_t Ln[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint32_t c = tile[lane * LS + j * kTX + xi];
                const uint32_t best = path_best(Lp, j, lo, hi, M, P1, P2);
                const uint32_t v = first ? c : c + best - M;
                tile[lane * LS + j * kTX + xi] = (uint16_t)v;
                Ln[j] = lane * NJ + j <= dmax ? v : kInf;
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) Lp[j] = Ln[j];
            first = false;
        }
        __syncthreads();
        if (lane < n) {
            const int dmax = min(D - 1, ka + kb * (x0 + lane));
#pragma unroll 8
            for (int d = 0; d <= dmax; ++d)
                atomicAdd(&S[d * P + row + x0 + lane], (uint32_t)tile[(d / NJ) * LS + (d % NJ) * kTX + lane]);
        }
        __syncthreads();
    }
}

// ---- vertical and diagonal paths: one workgroup per (32-column tile, direction), columns across the lanes ----
// Half wave w holds d = w * DPT .. w * DPT + DPT - 1 of its 32 columns in registers and walks the rows; every
// cost and sum access is a coalesced row segment (64 B of costs, 128 B of sums).  Per row the waves exchange, through a double-buffered
// LDS block and one barrier, their partial min (for M) and their first and last L (the d +- 1 terms at the
// chunk ends).  The costs of the next kPF rows are always in flight: a row's loads are issued kPF rows ahead.
// !DIAG, rho = (0, +-1): a lane keeps its column, restarts its path (L = C) in the first row only, and the d that
// exist, d <= dmax, are the same in every row.  What follows is switched on by DIAG at compile time, not by dx.
// DIAG (SM_PARAM_SGM_PATHS 8), rho = (dx, dy) with dx, dy = +-1: the columns slide along the path.  At step s of the
// walk (row y0 + s * dy) lane l of tile t is at the column
//     x = (32 t + l + s * dx) mod Wp,   Wp = 32 * ceil(W / 32),
// so the columns of all tiles cover every row exactly once, a lane's previous pixel on the path, q = p - rho, is the
// one it held a row earlier, and its L stays in its registers.  A lane restarts also where x - dx is outside [0, W):
// the column the path enters by, which is also where the wrap brings a lane back into the frame.  A lane at a
// column >= W (the padding of the last tile) is idle: it loads and adds nothing and carries kInf, and so is, with
// either DIAG, a lane at a column where no d exists (SM_PAIRS_IN_VIEW, x < d0): both have a negative dmax.  The 32
// columns of
// a half wave stay one row segment, cut in two only at the wrap, so the cost loads and the atomic adds keep their
// shape, shifted by s columns.  The d that exist change with the column: dmax is per lane and row, and the prefetch
// queue follows the column kPF rows ahead.
constexpr int kPF = 4;
constexpr int kVX = 32;   // columns per workgroup: each half of a wave is one d chunk of 32 columns
template <int DPT, bool DIAG>
__global__ __launch_bounds__(1024) void sgm_col_kernel(const uint16_t* __restrict__ C, int W, int H, int D, uint32_t P1,
                                                       uint32_t P2, int ka, int kb, uint32_t* __restrict__ S) {
    __shared__ uint32_t ex[2][3][32][kVX];
    const int lane = threadIdx.x & (kVX - 1), w = threadIdx.x / kVX, nw = blockDim.x / kVX;
    const int Wp = (int)gridDim.x * kVX;
    const int dir = blockIdx.y;   // rho = (0, +1), (0, -1); DIAG: (+1, +1), (-1, +1), (+1, -1), (-1, -1)
    const int dx = !DIAG ? 0 : (dir & 1 ? -1 : 1), dy = (DIAG ? dir & 2 : dir) ? -1 : 1;
    const int64_t P = (int64_t)W * H;
    const int d0 = w * DPT;
    const int y0 = dy < 0 ? H - 1 : 0;
    // DIAG: one step along the row, modulo Wp
    auto slide = [&](int x) { x += dx; return x < 0 ? x + Wp : (x >= Wp ? x - Wp : x); };
    auto dmax_at = [&](int x) { return x < W ? min(D - 1, ka + kb * x) : -1; };   // d <= dmax exist at this column
    uint32_t Lp[DPT], Cq[kPF][DPT];
#pragma unroll
    for (int j = 0; j < DPT; ++j) Lp[j] = kInf;
    int x = blockIdx.x * kVX + lane, dmax = dmax_at(x);   // this row's column and its dmax; they change with DIAG only
    int xq = x, dmq = dmax;                               // those of the next row to enter the queue
#pragma unroll
    for (int u = 0; u < kPF; ++u) {
        if (DIAG) dmq = dmax_at(xq);
#pragma unroll
        for (int j = 0; j < DPT; ++j)
            Cq[u][j] = u < H && d0 + j <= dmq ? C[(d0 + j) * P + (int64_t)(y0 + u * dy) * W + xq] : 0u;
        if (DIAG) xq = slide(xq);
    }
    for (int s0 = 0; s0 < H; s0 += kPF) {
#pragma unroll
        for (int u = 0; u < kPF; ++u) {
            const int s = s0 + u;
            if (s >= H) break;   // uniform over the workgroup
            const int y = y0 + s * dy;
            if (DIAG) dmax = dmax_at(x), dmq = dmax_at(xq);
            const int xp = x - dx;                                          // q's column, before the wrap
            const bool restart = s == 0 || (DIAG && (xp < 0 || xp >= W));
            uint32_t Cc[DPT];
#pragma unroll
            for (int j = 0; j < DPT; ++j) {   // this row's costs out of the queue, row s + kPF's into it
                Cc[j] = Cq[u][j];
                if (s + kPF < H) Cq[u][j] = d0 + j <= dmq ? C[(d0 + j) * P + (int64_t)(y + kPF * dy) * W + xq] : 0u;
            }
            uint32_t m = Lp[0];
#pragma unroll
            for (int j = 1; j < DPT; ++j) m = min(m, Lp[j]);
            const int b = u & 1;   // kPF is even: the parity of s
            ex[b][0][w][lane] = m;
            ex[b][1][w][lane] = Lp[0];
            ex[b][2][w][lane] = Lp[DPT - 1];
            __syncthreads();
            uint32_t M = kInf;
            for (int k = 0; k < nw; ++k) M = min(M, ex[b][0][k][lane]);
            const uint32_t lo = w > 0 ? ex[b][2][w - 1][lane] : kInf;
            const uint32_t hi = w + 1 < nw ? ex[b][1][w + 1][lane] : kInf;
            uint32_t Ln[DPT];
#pragma unroll
            for (int j = 0; j < DPT; ++j) {
                const uint32_t best = path_best(Lp, j, lo, hi, M, P1, P2);
                const uint32_t v = restart ? Cc[j] : Cc[j] + best - M;
                const bool exists = d0 + j <= dmax;
                if (exists) atomicAdd(&S[(d0 + j) * P + (int64_t)y * W + x], v);
                Ln[j] = exists ? v : kInf;
            }
#pragma unroll
            for (int j = 0; j < DPT; ++j) Lp[j] = Ln[j];
            if (DIAG) x = slide(x), xq = slide(xq);
        }
    }
}

// ---- WTA over S: the left map and, when asked, the right view's keys ----
// Left: the smallest existing d (d <= W - x) attaining min S, no threshold.  Right view: S_R(y, u, d) =
// S(y, u + d, d) (StereoHelper.cpp:156-180) over the d whose pair (u + d, d) exists, u + 2 d <= W (which
// implies u + d < W; d = 0 always exists); key = S << 8 | d, whose low byte is dR.
// SM_PAIRS_IN_VIEW (in_view, d0; ka, kb as above): plane k is d = d0 + k, the left view walks k <= min(D - 1, x - d0)
// and writes d0 + k, the right view is S_R(u, k) = S(u + d0 + k, k) over u + d0 + k <= W - 1, each of which exists
// in the left view; its keys carry k, and d0 is added where they become the map (launch_keys_low_byte).  A pixel
// with no candidate gets 0 in the left map and keeps the key ~0, which that step turns into 0.
// T: uint32_t, the paths' sum S (< 2^19 with eight paths), or uint16_t, a box cost volume taken without SGM (SM_COST_CENSUS with
// SM_AGG_BOX: the census cost, <= 62 * win^2 = 13950); either key fits 32 bits.
template <typename T>
__global__ __launch_bounds__(256) void sgm_wta_kernel(const T* __restrict__ S, int W, int H, int D,
                                                      int ka, int kb, int in_view, int d0,
                                                      uint8_t* __restrict__ disp, int pitch,
                                                      uint32_t* __restrict__ rkeys) {
    const int nxb = (W + 255) / 256;
    const int y = blockIdx.x / nxb, x = (blockIdx.x - y * nxb) * 256 + threadIdx.x;
    if (x >= W) return;
    const int64_t P = (int64_t)W * H;
    const T* s = S + (int64_t)y * W + x;
    const int dmax = min(D - 1, ka + kb * x);
    uint32_t best = 0xFFFFFFFFu;
    for (int d = 0; d <= dmax; ++d) best = min(best, ((uint32_t)s[d * P] << 8) | (uint32_t)d);
    disp[(int64_t)y * pitch + x] = dmax < 0 ? (uint8_t)0 : (uint8_t)((best & 0xFFu) + (uint32_t)d0);
    if (rkeys) {
        const int rmax = min(D - 1, in_view ? W - 1 - x - d0 : (W - x) / 2);   // x + d0 + rmax <= W - 1
        const T* sr = s + d0;
        uint32_t rb = 0xFFFFFFFFu;
        for (int d = 0; d <= rmax; ++d) rb = min(rb, ((uint32_t)sr[d * P + d] << 8) | (uint32_t)d);
        rkeys[(int64_t)y * W + x] = rb;
    }
}

}  // namespace

hipError_t launch_sgm_paths(const uint16_t* sad, int W, int H, int D, int P1, int P2, int paths, const Pairs& pr,
                            uint32_t* S, hipStream_t s) {
    const int ka = pr.ka(W), kb = pr.kb();
    if (W <= 0 || H <= 0 || D < 1 || D > kMaxDisp || P1 < 0 || P2 < P1 || P2 > 65535) return hipErrorInvalidValue;
    if ((paths != 4 && paths != 8) || !pr.ok(D, 4095)) return hipErrorInvalidValue;
    const dim3 hgrid((unsigned)H, 2);
    const int nj = (D + 63) / 64;
#define SM_SGM_H(n)                                                                                                  \
    do {                                                                                                            \
        if (W % 8 == 0 && reinterpret_cast<uintptr_t>(sad) % 16 == 0)                                               \
            hipLaunchKernelGGL((sgm_h_kernel<n, true>), hgrid, dim3(64), 0, s, sad, W, H, D, (uint32_t)P1,          \
                               (uint32_t)P2, ka, kb, S);                                                            \
        else                                                                                                        \
            hipLaunchKernelGGL((sgm_h_kernel<n, false>), hgrid, dim3(64), 0, s, sad, W, H, D, (uint32_t)P1,         \
                               (uint32_t)P2, ka, kb, S);                                                            \
    } while (0)
    if (nj == 1) SM_SGM_H(1);
    else if (nj == 2) SM_SGM_H(2);
    else if (nj == 3) SM_SGM_H(3);
    else SM_SGM_H(4);
#undef SM_SGM_H
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 vgrid((unsigned)((W + kVX - 1) / kVX), 2);
    const int dpt = D <= 64 ? 2 : (D <= 128 ? 4 : 8);   // at most 32 chunks of d
    // whole waves: a last half wave beyond D holds no existing d and only takes part in the exchange
    const dim3 vblock((unsigned)((kVX * ((D + dpt - 1) / dpt) + 63) / 64 * 64));
#define SM_SGM_COL(diag, grid)                                                                                       \
    hipLaunchKernelGGL((dpt == 2 ? sgm_col_kernel<2, diag> : (dpt == 4 ? sgm_col_kernel<4, diag> : sgm_col_kernel<8, diag>)), \
                       grid, vblock, 0, s, sad, W, H, D, (uint32_t)P1, (uint32_t)P2, ka, kb, S)
    SM_SGM_COL(false, vgrid);
    e = hipGetLastError();
    if (e != hipSuccess || paths == 4) return e;
    SM_SGM_COL(true, dim3(vgrid.x, 4));   // the four diagonals: the vertical pass's tiles and chunks
#undef SM_SGM_COL
    return hipGetLastError();
}

namespace {
template <typename T>
hipError_t launch_wta(const T* S, int W, int H, int D, const Pairs& pr, uint8_t* disp, int out_pitch,
                      uint32_t* right_keys, hipStream_t s) {
    const int64_t blocks = (int64_t)((W + 255) / 256) * H;
    if (W <= 0 || H <= 0 || D < 1 || D > kMaxDisp || out_pitch < W || blocks > 0x7FFFFFFF || !pr.ok(D, 255))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sgm_wta_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, S, W, H, D, pr.ka(W), pr.kb(),
                       pr.in_view, pr.d0, disp, out_pitch, right_keys);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_sgm_wta(const uint32_t* S, int W, int H, int D, const Pairs& pr, uint8_t* disp, int out_pitch,
                          uint32_t* right_keys, hipStream_t s) {
    return launch_wta(S, W, H, D, pr, disp, out_pitch, right_keys, s);
}

hipError_t launch_cost_wta_u16(const uint16_t* C, int W, int H, int D, const Pairs& pr, uint8_t* disp, int out_pitch,
                               uint32_t* right_keys, hipStream_t s) {
    return launch_wta(C, W, H, D, pr, disp, out_pitch, right_keys, s);
}

}  // namespace sm
