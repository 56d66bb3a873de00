// bm_segtree.hip — segment-tree cost aggregation: the reference's STMatching ST-1
// pipeline (stereo_disparity_normal, StereoDisparity.cpp:57-89) and ST-2 (stereo_disparity_iteration,
// :91-160) with their O(P*D) parts on the GPU.
//
//   guide + edge weights  GPU: 3x3 median of each BGR channel of the left view (MeanFilter(img, 1)
//                         = ctmf, SegmentTree.cpp:185), max channel |diff| to the right / upper
//                         neighbour (CColorWeight::GetWeight, :189-194)
//   edge order            GPU: the edges in (b, a) order, stably radix-sorted by weight, which is
//                         edge::operator<'s (weight, b, a) order (SegmentTree.h:103-111); the sorted
//                         edges come back to the host page-locked
//   tree                  host: segment_graph's two passes, sequential as the reference's: Kruskal with
//                         Felzenszwalb's size threshold, then the rest of the spanning tree with the
//                         cross-segment penalty (segment-graph.h:48-101; disjoint-set.h:30-82), as per-edge
//                         marks.  GPU (round 4): the neighbour lists in the sorted edge order and the BFS
//                         from pixel 0 (SegmentTree.cpp:71-130), by an Euler tour ranked with pointer
//                         jumping and a depth sort (bm_segtree_build.hip: st_adj_kernel .. st_task_kernel,
//                         gpu_bfs, with the edge sort)
//   cost volume           GPU: truncated colour + gradient cost (StereoHelper.cpp:37-129), written
//                         channel-major in BFS order, C[d][i], so a tree level is a contiguous run
//   filter                GPU: one wave per disparity walks the BFS levels (st_filter_wave_kernel; one
//                         workgroup per disparity for trees wider than its LDS): leaf-to-root sums, then
//                         root-to-leaf (SegmentTree.cpp:148-181); each node sums its children in the
//                         reference's order with separate multiplies and adds
//   WTA, x scale, median  GPU: first d with the smallest cost (StereoHelper.cpp:131-154), times scale
//                         (saturated; a non-decreasing map commutes with the median), then the 7x7
//                         median (MeanFilter(disparity, 3), bm_post.hip)
// ST-2 adds: the right view's cost taken from the left's (GetRightMatchingCostFromLeft,
// StereoHelper.cpp:156-180: C_R(y, x, d) = C(y, min(x + d, W - 1), min(d, W - 1 - x)), computed directly),
// a colour tree of each view filtered in one launch, the left-right check (bm_aux.hip), and a colour +
// depth tree (CColorDepthWeight, SegmentTree.cpp:196-219) whose float weights the GPU forms from the
// colour weights, the first left map and the mask, and orders by a stable radix sort of their bits.
// The maps are bit-exact with the restated oracle (oracle/st_oracle.c).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <thread>
#include <vector>

#include "bm_common.h"
#include "bm_segtree_build.h"

namespace sm {
namespace {

// median of 9 (the classic 19-exchange network)
__device__ __forceinline__ uint8_t med9(uint8_t* v) {
    auto s = [&](int i, int j) {
        const uint8_t a = min(v[i], v[j]), b = max(v[i], v[j]);
        v[i] = a;
        v[j] = b;
    };
    s(1, 2); s(4, 5); s(7, 8); s(0, 1); s(3, 4); s(6, 7); s(1, 2); s(4, 5); s(7, 8);
    s(0, 3); s(5, 8); s(4, 7); s(3, 6); s(1, 4); s(2, 5); s(4, 7); s(4, 2); s(6, 4); s(4, 2);
    return v[4];
}

// per pixel p: wr[p] = weight of edge (p, p+1), wu[p] = weight of edge (p, p-W), on the 3x3-median
// guide (replicate borders, as ctmf)
__global__ __launch_bounds__(kST) void st_weights_kernel(const uint8_t* __restrict__ bgr, int W, int H, int pitch,
                                                         uint8_t* __restrict__ wr, uint8_t* __restrict__ wu) {
    const int x = blockIdx.x * kST + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    auto guide = [&](int gx, int gy, uint8_t out[3]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t v[9];
#pragma unroll
            for (int i = -1; i <= 1; ++i)
#pragma unroll
                for (int j = -1; j <= 1; ++j) {
                    const int yy = min(max(gy + i, 0), H - 1), xx = min(max(gx + j, 0), W - 1);
                    v[(i + 1) * 3 + (j + 1)] = bgr[(int64_t)yy * pitch + 3 * xx + c];
                }
            out[c] = med9(v);
        }
    };
    uint8_t g[3], n[3];
    guide(x, y, g);
    uint8_t r = 0, u = 0;
    if (x + 1 < W) {
        guide(x + 1, y, n);
        r = max(max((uint8_t)abs(g[0] - n[0]), (uint8_t)abs(g[1] - n[1])), (uint8_t)abs(g[2] - n[2]));
    }
    if (y >= 1) {
        guide(x, y - 1, n);
        u = max(max((uint8_t)abs(g[0] - n[0]), (uint8_t)abs(g[1] - n[1])), (uint8_t)abs(g[2] - n[2]));
    }
    wr[(int64_t)y * W + x] = r;
    wu[(int64_t)y * W + x] = u;
}

// GetGradient (StereoHelper.cpp:39-73) of one view: gray (rgb_2_gray, :37, in double) and the
// central / one-sided difference + 127.5 in float
__global__ __launch_bounds__(kST) void st_gradient_kernel(const uint8_t* __restrict__ bgr, int W, int H, int pitch,
                                                          float* __restrict__ grad) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * kST + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    auto gray = [&](int xx) -> float {
        const uint8_t* in = bgr + (int64_t)y * pitch + 3 * xx;
        return (float)(uint8_t)(0.299 * in[2] + 0.587 * in[1] + 0.114 * in[0] + 0.5);
    };
    float g;
    if (x == 0) g = gray(1) - gray(0) + 127.5f;
    else if (x == W - 1) g = gray(W - 1) - gray(W - 2) + 127.5f;
    else g = 0.5f * (gray(x + 1) - gray(x - 1)) + 127.5f;
    grad[(int64_t)y * W + x] = g;
}

// GetMatchingCost (StereoHelper.cpp:75-129) into C[d][rank[p]]; right pixels left of column 0 repeat
// column 0 (:107-110); double arithmetic as the reference's, rounded to float once.  RIGHT: the right
// view's cost at pixel p = (y, x), GetRightMatchingCostFromLeft (StereoHelper.cpp:156-180): the left
// cost at (y, min(x + d, W - 1)) and disparity min(d, W - 1 - x), whose right pixel is (y, x) itself.
// One thread per BFS index i (pixel node[i]), so the D stores of a wave are coalesced (round 4: one thread
// per pixel scattered them through rank; Art D = 60: 81 -> 51 us, rocprof); the image and gradient reads
// gather from L2-resident rows instead.
template <bool RIGHT>
__global__ __launch_bounds__(kST) void st_cost_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R,
                                                      int W, int H, int pitch, const float* __restrict__ gL,
                                                      const float* __restrict__ gR, const int* __restrict__ node, int D,
                                                      float* __restrict__ C) {
#pragma clang fp contract(off)
    const int64_t P = (int64_t)W * H;
    const int i = blockIdx.x * kST + threadIdx.x;
    if (i >= P) return;
    const int p = node[i];
    if ((unsigned)p >= (unsigned)P) return;
    const int y = p / W, x = p - y * W;
    const double wc = 0.11, wg = 1.0 - wc;
    auto cost = [&](int xl, int xr) -> float {
        const uint8_t* l = L + (int64_t)y * pitch + 3 * xl;
        const uint8_t* r = R + (int64_t)y * pitch + 3 * xr;
        double cc = (double)(abs(l[0] - r[0]) + abs(l[1] - r[1]) + abs(l[2] - r[2]));
        cc = cc / 3 < 7.0 ? cc / 3 : 7.0;
        double cg = fabsf(gL[(int64_t)y * W + xl] - gR[(int64_t)y * W + xr]);
        cg = cg < 2.0 ? cg : 2.0;
        return (float)(wc * cc + wg * cg);
    };
    for (int d = 0; d < D; ++d) {
        const float c = RIGHT ? cost(min(x + d, W - 1), x) : cost(x, x >= d ? x - d : 0);
        C[(int64_t)d * P + i] = c;
    }
}

// One tree's filter input: C (in: cost, out: the leaf-to-root sums, the reference's costBuffer) and F
// (out: the filtered cost) are [D][P] in that tree's BFS order; levels are the BFS position ranges
// [lev[l], lev[l + 1]).
struct FilterJob {
    float* C;
    float* F;
    const int* parent;
    const uint8_t* pdist;
    const int* first;
    const uint32_t* child;
    const int* lev;
    int nlev;
    const float* table;
};
struct FilterJobs {
    FilterJob j[2];
};

// Filter (SegmentTree.cpp:148-181) of disparity d = blockIdx.x of job blockIdx.y (ST-2 filters the left
// and right views' volumes in one launch: each job has only D workgroups).
#ifndef SM_ST_FILTER_THREADS
#define SM_ST_FILTER_THREADS 1024
#endif
constexpr int kFT = SM_ST_FILTER_THREADS;
__global__ __launch_bounds__(kFT) void st_filter_kernel(FilterJobs jobs, int P) {
#pragma clang fp contract(off)
    const FilterJob& jb = jobs.j[blockIdx.y];
    const int* __restrict__ parent = jb.parent;
    const uint8_t* __restrict__ pdist = jb.pdist;
    const int* __restrict__ first = jb.first;
    const uint32_t* __restrict__ child = jb.child;
    const int* __restrict__ lev = jb.lev;
    const int nlev = jb.nlev;
    __shared__ float table[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) table[k] = jb.table[k];
    __syncthreads();
    float* __restrict__ U = jb.C + (int64_t)blockIdx.x * P;
    float* __restrict__ Fd = jb.F + (int64_t)blockIdx.x * P;
    // leaf to root: a node adds its children in order, each term multiplied then added
    for (int l = nlev - 1; l >= 0; --l) {
        const int lo = lev[l], hi = lev[l + 1];
        for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
            const uint32_t ch = child[i];                    // count | dist0 << 8 | dist1 << 16 | dist2 << 24
            const int n = (int)(ch & 0xFFu);
            if (n == 0) continue;
            float u = U[i];
            const int f = first[i];
            for (int z = 0; z < n; ++z) {
                const float t = U[f + z] * table[(ch >> (8 * (z + 1))) & 0xFFu];
                u = u + t;
            }
            U[i] = u;
        }
        __syncthreads();
    }
    // root to leaf
    if (threadIdx.x == 0) Fd[0] = U[0];
    __syncthreads();
    for (int l = 1; l < nlev; ++l) {
        const int lo = lev[l], hi = lev[l + 1];
        for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
            const float w = table[pdist[i]], cur = U[i];
            const float t = w * cur;
            Fd[i] = w * (Fd[parent[i]] - t) + cur;
        }
        __syncthreads();
    }
}

// ---- the same filter, one wave per disparity (st_filter_wave_kernel) ----
// A tree level's values depend only on the next (leaf to root) or the previous (root to leaf) level,
// and in BFS order the children of one level are exactly the next level, contiguous.  So one wave per
// disparity walks the levels with the two live levels in LDS (ping-pong buffers of the widest
// level), wave-synchronous: no workgroup barrier and no global store -> load round trip per level,
// which bound st_filter_kernel (~0.7 us per level).  The host cuts every level into tasks of <= 64
// nodes (one node per lane), each an int4 {x = first node, count - 1, LDS byte offset of the task's
// first node in its level buffer, LDS byte offset that the node index of a child (up) / parent (down)
// is added to}.
//
// The tasks run in blocks of kStBlk.  While block b runs, the wave's global loads for block b + 1 (its
// lanes' node operands) and the records of block b + 2 are in flight; they land in LDS at the end of
// the block (a wait that is long satisfied by then), where block b + 1 reads them.  Staging through LDS
// keeps every load and its wait in one loop iteration: a register ring carried across the loop's back
// edge made the compiler drain all loads (vmcnt(0)) once per trip.  Global memory goes through buffer
// descriptors (32-bit offsets).  The LDS layout (kSt*Off) is in bm_segtree_build.h.
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct WaveJob {
    float* C;                  // in: cost, out: leaf-to-root sums (read again by the root-to-leaf pass)
    float* F;                  // out: filtered cost
    const int* parent;
    const uint8_t* pdist;
    const int* first;
    const uint32_t* child;
    const int4* task;          // [n_up tasks, leaf to root][n_dn tasks, root to leaf]
    int n_up, n_dn;            // the task records carry the LDS offsets
    const float* table;
};
struct WaveJobs {
    WaveJob j[2];
};

using BufRsrc = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ BufRsrc buf_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
constexpr int kAuxSc1 = 16;   // sc1: the load misses the (non-coherent) L1, as an agent-scope atomic load
template <int AUX = 0>
__device__ __forceinline__ uint32_t buf_ld(BufRsrc r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, AUX);
}
// one wave per CU at most (D or 2 D waves on 256 CUs): the compiler may schedule for latency, not occupancy
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void st_filter_wave_kernel(WaveJobs jobs,
                                                                                                       int P) {
#pragma clang fp contract(off)
    const WaveJob& jb = jobs.j[blockIdx.y];
    extern __shared__ float sbuf[];          // layout: kSt*Off above
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += 64) sbuf[k] = jb.table[k];
    if (lane == 0) sbuf[kStZeroOff / 4] = 0.0f;
    const uint32_t Pb = (uint32_t)P * 4u;
    const BufRsrc rU = buf_rsrc(jb.C + (int64_t)blockIdx.x * P, Pb);
    const BufRsrc rF = buf_rsrc(jb.F + (int64_t)blockIdx.x * P, Pb);
    char* lds = reinterpret_cast<char*>(sbuf);
    auto lds_f = [&](int off) -> float& { return *reinterpret_cast<float*>(lds + off); };
    u32x3* node_area = reinterpret_cast<u32x3*>(lds + kStNodeOff);   // [k][lane]
    i32x4* rec_area = reinterpret_cast<i32x4*>(lds + kStRecOff);     // [block parity][k]
    __syncthreads();

    // node_load(record) -> u32x3 of this lane's node; body(record, node operands)
    auto pass = [&](const int4* tk0, int nt, auto node_load, auto body) {
        if (nt <= 0) return;
        const BufRsrc rT = buf_rsrc(tk0, (uint32_t)nt * 16u);
        // lane l loads dword l & 3 of record (block start + l / 4), clamped to the last task
        auto rec_block = [&](int blk) {
            const int t = min(blk * kStBlk + (lane >> 2), nt - 1);
            return (int)buf_ld(rT, (uint32_t)t * 16u + (uint32_t)(lane & 3) * 4u);
        };
        auto rec_put = [&](int parity, int v) { reinterpret_cast<int*>(rec_area + parity * kStBlk)[lane] = v; };
        // the node loads of a block need each record's first node and count - 1: one LDS dword per lane
        // (lane l: dword l & 3 of record l / 4) read out with v_readlane, rather than 16 128-bit reads
        // whose registers the compiler overlaps (and then serialises)
        auto gather = [&](int parity, u32x3* g) {
            const int rv = reinterpret_cast<const int*>(rec_area + parity * kStBlk)[lane];
#pragma unroll
            for (int k = 0; k < kStBlk; ++k) {
                i32x4 rr;
                rr.x = __builtin_amdgcn_readlane(rv, 4 * k);
                rr.y = __builtin_amdgcn_readlane(rv, 4 * k + 1);
                rr.z = rr.w = 0;
                g[k] = node_load(rr);
            }
        };
        const int nb = (nt + kStBlk - 1) / kStBlk;
        // prologue: records of blocks 0 and 1, node operands of block 0
        rec_put(0, rec_block(0));
        const int r1 = rec_block(1);
        {
            u32x3 g[kStBlk];
            gather(0, g);
#pragma unroll
            for (int k = 0; k < kStBlk; ++k) node_area[k * 64 + lane] = g[k];
        }
        rec_put(1, r1);
        for (int b = 0; b < nb; ++b) {
            const int cur = b & 1;
            // loads for later blocks: the records of block b + 2, the node operands of block b + 1
            const int rn = rec_block(b + 2);
            u32x3 g[kStBlk];
            gather(cur ^ 1, g);
            // block b: its records and node operands all read before the first level write
            i32x4 rc[kStBlk];
            u32x3 nd[kStBlk];
#pragma unroll
            for (int k = 0; k < kStBlk; ++k) {
                rc[k] = rec_area[cur * kStBlk + k];
                nd[k] = node_area[k * 64 + lane];
            }
            // no branches: a block past the last task repeats the last task (records clamped), which
            // rewrites the same values
#pragma unroll
            for (int k = 0; k < kStBlk; ++k) body(rc[k], nd[k]);
            // stage block b + 1's operands and block b + 2's records
#pragma unroll
            for (int k = 0; k < kStBlk; ++k) node_area[k * 64 + lane] = g[k];
            rec_put(cur, rn);
        }
    };
    // byte offset of this lane's node (lanes past the task's count repeat its last node); the store
    // offset of those lanes lies past the buffer's end, where the hardware drops the store
    auto node_off = [&](const i32x4& r) { return (uint32_t)(r.x + min(lane, r.y)) * 4u; };
    auto store_off = [&](const i32x4& r) { return lane <= r.y ? (uint32_t)(r.x + lane) * 4u : 0x80000000u; };

    // ---- leaf to root: u = C[i] + sum_z table[dist_z] * u(child z), children in order ----
    const BufRsrc rChild = buf_rsrc(jb.child, Pb), rFirst = buf_rsrc(jb.first, Pb);
    pass(jb.task, jb.n_up,
         [&](const i32x4& r) {
             const uint32_t o = node_off(r);
             return u32x3{buf_ld(rU, o), buf_ld(rChild, o), buf_ld(rFirst, o)};
         },
         [&](const i32x4& r, const u32x3& n0) {
             // every lane computes (those past the count into the level buffer's 64-float pad)
             {
                 const uint32_t ch = n0.y;
                 const int n = (int)(ch & 0xFFu);
                 const int rd = r.w + (int)n0.z * 4;
                 float u = __builtin_bit_cast(float, n0.x);
                 // at most 3 children (a grid node has 4 neighbours, one of them its parent; the root is
                 // the corner pixel 0): all six LDS reads issued together.  An absent child reads the
                 // float 0 (its distance byte is 0, weight 1): its term is +0, and u + 0 = u exactly for the
                 // non-negative sums here, so the chain after the reads is one multiply and three adds.
                 float cv[3], wv[3];
#pragma unroll
                 for (int z = 0; z < 3; ++z) {
                     cv[z] = lds_f(z < n ? rd + 4 * z : kStZeroOff);
                     wv[z] = sbuf[(ch >> (8 * (z + 1))) & 0xFFu];
                 }
#pragma unroll
                 for (int z = 0; z < 3; ++z) {
                     const float tt = cv[z] * wv[z];
                     u = u + tt;
                 }
                 lds_f(r.z + lane * 4) = u;
                 // a leaf's u is its C: rewritten unchanged
                 __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, u), rU, store_off(r), 0, 0);
             }
         });
    __syncthreads();   // the U stores have completed (vmcnt) before the root-to-leaf pass reads them back

    // ---- root to leaf: F[i] = w (F[parent] - w U[i]) + U[i] ----
    if (lane == 0) {
        const float u0 = __builtin_bit_cast(float, buf_ld<kAuxSc1>(rU, 0));
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, u0), rF, 0, 0, 0);
        lds_f(kStLvlOff) = u0;   // level 0 (the root) has parity 0
    }
    __builtin_amdgcn_wave_barrier();
    const BufRsrc rParent = buf_rsrc(jb.parent, Pb), rDist = buf_rsrc(jb.pdist, (uint32_t)P);
    pass(jb.task + jb.n_up, jb.n_dn,
         [&](const i32x4& r) {
             const uint32_t o = node_off(r);
             // U was written by this wave's leaf-to-root pass: read past the (non-coherent) L1
             return u32x3{buf_ld<kAuxSc1>(rU, o), buf_ld(rParent, o),
                          (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rDist, o >> 2, 0, 0)};
         },
         [&](const i32x4& r, const u32x3& n0) {
             {
                 const float w = sbuf[n0.z], u = __builtin_bit_cast(float, n0.x);
                 const float tt = w * u;
                 const float fv = w * (lds_f(r.w + (int)n0.y * 4) - tt) + u;
                 lds_f(r.z + lane * 4) = fv;
                 __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, fv), rF, store_off(r), 0, 0);
             }
         });
}

// node[i] = the pixel at BFS index i (the inverse of rank)
__global__ __launch_bounds__(kST) void st_node_kernel(const int* __restrict__ rank, int P, int* __restrict__ node) {
    const int p = blockIdx.x * kST + threadIdx.x;
    if (p >= P) return;
    const int i = rank[p];
    if ((unsigned)i < (unsigned)P) node[i] = p;
}

// GetDisparity_WTA (StereoHelper.cpp:131-154): strict < from d = 0; times scale, saturated.  One thread
// per BFS index, so the D cost reads of a wave are coalesced (round 4: per pixel, they were gathers
// through rank, 62 -> 9 us for Art at D = 60); the result goes to its pixel.
__global__ __launch_bounds__(kST) void st_wta_kernel(const float* __restrict__ F, const int* __restrict__ node, int P,
                                                     int D, int scale, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * kST + threadIdx.x;
    if (i >= P) return;
    float v = F[i];
    int m = 0;
    for (int d = 1; d < D; ++d) {
        const float c = F[(int64_t)d * P + i];
        if (c < v) {
            v = c;
            m = d;
        }
    }
    const int p = node[i];
    if ((unsigned)p < (unsigned)P) out[p] = (uint8_t)min(m * scale, 255);
}

// ---- host: the tree, sequential as the reference's (bm_segtree_host.h) ----
using namespace st_host;

DevTree tree_slot(StWorkspace& ws, int64_t P, int k) {
    DevTree d{};
    d.rank = ws.tree_i.p + (size_t)k * (5 * P + 2);
    d.parent = d.rank + P;
    d.first = d.parent + P;
    d.child = reinterpret_cast<uint32_t*>(d.first + P);
    d.lev = reinterpret_cast<int*>(d.child + P);
    d.pdist = ws.tree_b.p + (size_t)k * P;
    d.table = ws.table.p + (size_t)k * 256;
    return d;
}

// UpdateTable (SegmentTree.cpp:141-146)
void weight_table(float sigma, float* table) {
    const float sg = std::max(0.01f, sigma);
    for (int i = 0; i <= 255; ++i) table[i] = std::exp(-float(i) / (255 * sg));
}

// SM_ST_HOST_BFS=1 builds the BFS on the host instead (st_host::bfs_tree, round 3's path), read at every
// call: the A/B baseline and the reference the GPU test compares the device arrays with
bool host_bfs_requested() {
    const char* e = std::getenv("SM_ST_HOST_BFS");
    return e && e[0] == '1';
}

// A host tree bound to its slot's page-locked block: its level offsets join the ints, which go up as one
// copy (rank .. lev), then pdist and the weight table.  The block and `table` must stay alive until the
// stream has consumed the copies.
hipError_t upload_tree(const HostTree& t, const float* table, int64_t P, DevTree& d, hipStream_t s) {
    d.nlev = (int)t.lev.size() - 1;
    if ((size_t)d.nlev + 1 > (size_t)P + 2) return hipErrorInvalidValue;
    int* ints = t.rank;
    std::copy(t.lev.begin(), t.lev.end(), ints + 4 * P);
    ST_CHK(hipMemcpyAsync(d.rank, ints, ((size_t)4 * P + t.lev.size()) * 4, hipMemcpyHostToDevice, s));
    ST_CHK(hipMemcpyAsync(d.pdist, t.pdist, (size_t)P, hipMemcpyHostToDevice, s));
    return hipMemcpyAsync(d.table, table, 256 * sizeof(float), hipMemcpyHostToDevice, s);
}

// node[i] of tree d (the inverse of its rank) into `node` (P ints), for the cost volume and the WTA
hipError_t launch_node(const DevTree& d, int* node, int P, hipStream_t s) {
    hipLaunchKernelGGL(st_node_kernel, dim3((unsigned)((P + kST - 1) / kST)), dim3(kST), 0, s, d.rank, P, node);
    return hipGetLastError();
}

// the cost volume in tree d's BFS order (node: launch_node's), RIGHT: the right view's
template <bool RIGHT>
hipError_t launch_cost(const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch, const float* grad, const int* node,
                       int D, float* C, hipStream_t s) {
    const int64_t P = (int64_t)W * H;
    hipLaunchKernelGGL(st_cost_kernel<RIGHT>, dim3((unsigned)((P + kST - 1) / kST)), dim3(kST), 0, s, dL, dR, W, H,
                       pitch, grad, grad + P, node, D, C);
    return hipGetLastError();
}

// WTA of the filtered cost F (BFS order) into the map `out` (pixel order); node: launch_node's
hipError_t launch_wta(const float* F, const int* node, int P, int D, int scale, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(st_wta_kernel, dim3((unsigned)((P + kST - 1) / kST)), dim3(kST), 0, s, F, node, P, D, scale, out);
    return hipGetLastError();
}

// a level buffer holds the widest level and 64 floats of pad for the lanes past a task's count
int wave_level_stride(int maxw) { return maxw + 64; }

// The wave filter's tasks of one tree (st_filter_wave_kernel): every level cut into runs of <= 64 nodes,
// leaf to root, then root to leaf from level 1; each task {first node, count - 1, LDS byte offset of its
// first node in the level buffer of its level's parity, LDS byte offset that the index of a node of the
// level it reads (children up, parents down; the other parity's buffer) is added to}.  Returns the
// widest level, which sizes the buffers.
int wave_tasks(const HostTree& t, std::vector<int4>& out, int& n_up, int& n_dn) {
    const int nlev = (int)t.lev.size() - 1;
    out.clear();
    int maxw = 1;
    for (int l = 0; l < nlev; ++l) maxw = std::max(maxw, t.lev[l + 1] - t.lev[l]);
    const int stride = wave_level_stride(maxw);
    auto cut = [&](int l, int other) {
        const int lo = t.lev[l], hi = t.lev[l + 1], q = l & 1;
        const int rb = kStLvlOff + ((q ^ 1) * stride - other) * 4;
        for (int s0 = lo; s0 < hi; s0 += 64)
            out.push_back(make_int4(s0, std::min(64, hi - s0) - 1, kStLvlOff + (q * stride + s0 - lo) * 4, rb));
    };
    for (int l = nlev - 1; l >= 0; --l) cut(l, l + 1 < nlev ? t.lev[l + 1] : t.lev[l]);
    n_up = (int)out.size();
    for (int l = 1; l < nlev; ++l) cut(l, t.lev[l - 1]);
    n_dn = (int)out.size() - n_up;
    return maxw;
}

constexpr int kWaveMaxLevel = (65536 - kStLvlOff) / 8 - 64;   // 64 KB of LDS; wider trees keep st_filter_kernel

// One filter launch over 1 or 2 jobs: the wave filter when every level fits its LDS buffers, else the
// workgroup-per-disparity filter.
// SM_ST_WAVE_FILTER=0 forces the workgroup filter (the path of trees wider than the wave filter's LDS,
// which no bundled image reaches; tests/test_gpu_segtree.py runs it this way)
bool wave_filter_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("SM_ST_WAVE_FILTER");
        return !(e && e[0] == '0');
    }();
    return on;
}

hipError_t launch_filter(const FilterJobs& fj, const WaveJobs& wj, int njobs, int maxw, int D, int P, hipStream_t s) {
    if (maxw <= kWaveMaxLevel && wave_filter_enabled()) {
        hipLaunchKernelGGL(st_filter_wave_kernel, dim3((unsigned)D, (unsigned)njobs), dim3(64),
                           (size_t)kStLvlOff + (size_t)(2 * wave_level_stride(maxw)) * sizeof(float), s, wj, P);
    } else {
        hipLaunchKernelGGL(st_filter_kernel, dim3((unsigned)D, (unsigned)njobs), dim3(kFT), 0, s, fj, P);
    }
    return hipGetLastError();
}

// A built tree's filter inputs: its device slot, its tasks and their counts.  hdr: where the device BFS's
// header {levels, widest level, up tasks, down tasks} lands (read_trees fills the counts from it); null
// when the host built the tree and the counts are known already
struct TreeJob {
    DevTree d;
    int4* task;
    int maxw, n_up, n_dn;
    const int* hdr;
};

// Host memory that a tree build's asynchronous copies read: the weight table and the host BFS path's
// tasks.  Declared before the entry point's StDrain, so it outlives the drain.
struct TreeFeed {
    float table[256];
    std::vector<int4> tv[2];
};

// Drains s, and the side stream once it exists, on every exit of an entry point: the stack arrays that
// feed asynchronous copies (TreeFeed) and the page-locked slots, which the next call's host passes write,
// are not touched by a queued copy after the call.  The success path returns finish()'s error.
struct StDrain {
    StWorkspace& ws;
    hipStream_t s;
    bool done = false;
    hipError_t finish() {
        done = true;
        const hipError_t e1 = ws.side.s ? hipStreamSynchronize(ws.side.s) : hipSuccess;
        const hipError_t e0 = hipStreamSynchronize(s);
        return e0 != hipSuccess ? e0 : e1;
    }
    ~StDrain() {
        if (!done) (void)finish();
    }
};

// joins its thread on every exit from the scope
struct JoinedThread {
    std::thread t;
    ~JoinedThread() {
        if (t.joinable()) t.join();
    }
};

// Builds n trees (1 or 2) from the sorted edges of edge slots [0, n) (nE each, gpu_sorted_edges) into
// device tree slots [0, n) and writes their TreeJobs: segment_graph's passes on the host, each starting on
// the first downloaded chunk of its edges (no stream sync: what s holds runs meanwhile), into the slot's
// page-locked marks, then the device BFS enqueued as soon as the marks are done.  Two trees
// (StereoDisparity.cpp:112-123) are built side by side, slot 1 on a thread and its BFS on the side stream,
// which s then waits for (the two BFSs are chains of small latency-bound kernels: side by side they
// overlap).  f.table: the tree's weight table (weight_table).  Ends with bfs_ev behind the header copies:
// work enqueued after it, e.g. the cost volume, runs while read_trees waits.
hipError_t build_trees(StWorkspace& ws, int n, int64_t P, int W, int nE, float tau, float wscale, TreeFeed& f,
                       hipStream_t s, TreeJob* tj) {
    const bool hbfs = host_bfs_requested();
    // every resource before a build thread starts
    ST_CHK(ws.task.reserve(task_slot_cap(P) * 4 * (size_t)n));
    ST_CHK(ws.h_hdr.reserve(8));
    ST_CHK(ws.bfs_ev.create());
    if (n > 1) {
        ST_CHK(ws.side_ev.create());
        ST_CHK(ws.side.create());
    }
    for (int k = 0; k < n; ++k) {
        StSlot& sl = ws.slot[k];
        ST_CHK(sl.h_marks.reserve((size_t)nE));
        if (!sl.tree) sl.tree.reset(new HostTree());
        if (!hbfs) continue;   // the device BFS: the host keeps only the passes' forest
        // the host BFS writes the tree into the page-locked block (ints, then pdist); the neighbour lists
        // take the tree's own vector
        ST_CHK(sl.h_tree.reserve((size_t)(5 * P + 2) + (size_t)(P + 3) / 4));
        sl.tree->bind((int)P, sl.h_tree.p, reinterpret_cast<uint8_t*>(sl.h_tree.p + 5 * P + 2));
        sl.tree->adj.resize((size_t)P);
    }
    const hipStream_t bs[2] = {s, ws.side.s};
    // tree slot k's device part on stream q: the weight table and the device BFS, or the host tree's upload
    // and its host tasks
    auto enqueue = [&](int k, hipStream_t q) -> hipError_t {
        TreeJob& j = tj[k];
        j = TreeJob{};
        j.d = tree_slot(ws, P, k);
        j.task = reinterpret_cast<int4*>(ws.task.p) + task_slot_cap(P) * (size_t)k;
        if (!hbfs) {
            j.hdr = ws.h_hdr.p + 4 * k;
            ST_CHK(hipMemcpyAsync(j.d.table, f.table, 256 * sizeof(float), hipMemcpyHostToDevice, q));
            return gpu_bfs(ws, k, (int)P, W, nE, wscale, j.d, j.task, ws.h_hdr.p + 4 * k, q);
        }
        const HostTree& t = *ws.slot[k].tree;
        ST_CHK(upload_tree(t, f.table, P, j.d, q));
        j.maxw = wave_tasks(t, f.tv[k], j.n_up, j.n_dn);
        if (f.tv[k].size() > task_slot_cap(P)) return hipErrorInvalidValue;
        return hipMemcpyAsync(j.task, f.tv[k].data(), f.tv[k].size() * sizeof(int4), hipMemcpyHostToDevice, q);
    };
    auto build = [&](int k) -> hipError_t {
        StSlot& sl = ws.slot[k];
        HostTree& t = *sl.tree;
        bool arrived = true;
        auto hook = [&](int upto) { arrived = arrived && wait_edges(ws, k, upto); };
        const Edge* e = reinterpret_cast<const Edge*>(sl.h_edges.p);
        if (hbfs) {   // uploaded below, on s in slot order
            segment_lists(e, nE, (int)P, tau, wscale, t, sl.edge_chunk, hook, t.adj.data());
            return arrived && bfs_tree(t.adj.data(), (int)P, W, t) ? hipSuccess : hipErrorInvalidValue;
        }
        segment_passes(e, nE, (int)P, tau, t, sl.edge_chunk, hook, sl.h_marks.p, [](int) {});
        if (!arrived) return hipErrorInvalidValue;
        const hipError_t er = enqueue(k, bs[k]);
        return er == hipSuccess && k == 1 ? hipEventRecord(ws.side_ev.ev, ws.side.s) : er;
    };
    hipError_t e0 = hipSuccess, e1 = hipSuccess;
    int dev = 0;
    if (n > 1) ST_CHK(hipGetDevice(&dev));
    {
        JoinedThread th;
        // no exception may leave the thread: a failed build there reports an error.  One thrown by build(0)
        // (std::bad_alloc) passes on to the caller once th has joined
        if (n > 1)
            th.t = std::thread([&] {
                try {
                    e1 = hipSetDevice(dev);   // the current device is per thread (the allocations, the launches)
                    if (e1 == hipSuccess) e1 = build(1);
                } catch (...) {
                    e1 = hipErrorInvalidValue;
                }
            });
        e0 = build(0);
    }
    ST_CHK(e0);
    ST_CHK(e1);
    if (hbfs)
        for (int k = 0; k < n; ++k) ST_CHK(enqueue(k, s));
    else if (n > 1)
        ST_CHK(hipStreamWaitEvent(s, ws.side_ev.ev, 0));
    return hipEventRecord(ws.bfs_ev.ev, s);
}

// The device BFS's headers of trees [0, n) once build_trees' event has passed (host-built trees: known already)
hipError_t read_trees(StWorkspace& ws, TreeJob* j, int n, int64_t P) {
    if (!j[0].hdr) return hipSuccess;
    ST_CHK(hipEventSynchronize(ws.bfs_ev.ev));
    for (int k = 0; k < n; ++k) {
        const int* h = j[k].hdr;
        if (h[0] < 1 || h[0] > P || h[1] < 1 || h[1] > P || h[2] < 1 || h[3] != h[2] - 1) return hipErrorUnknown;
        j[k].d.nlev = h[0];
        j[k].maxw = h[1];
        j[k].n_up = h[2];
        j[k].n_dn = h[3];
    }
    return hipSuccess;
}

float ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Aggregation on n built trees (build_trees, started at t0): tree k's cost volume in its BFS order (k = 0
// the left view's cost, k = 1 the right view's), the filter over all of them in one launch, then per tree
// the WTA times `scale` into raw[k] and its 7x7 median into out[k].  The node and cost kernels are enqueued
// before read_trees waits for the BFS headers, so they run meanwhile.  st: the tree time, until the headers
// are back, and tree 0's levels.
hipError_t aggregate(StWorkspace& ws, TreeJob* tj, int n, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch,
                     int D, int scale, uint8_t* const* raw, uint8_t* const* out,
                     std::chrono::steady_clock::time_point t0, hipStream_t s, StStats& st) {
    const int64_t P = (int64_t)W * H;
    for (int k = 0; k < n; ++k) ST_CHK(launch_node(tj[k].d, ws.node.p + k * P, (int)P, s));
    ST_CHK(launch_cost<false>(dL, dR, W, H, pitch, ws.grad.p, ws.node.p, D, ws.vol.p, s));
    if (n > 1)
        ST_CHK(launch_cost<true>(dL, dR, W, H, pitch, ws.grad.p, ws.node.p + P, D, ws.vol.p + (size_t)P * D * 2, s));
    ST_CHK(read_trees(ws, tj, n, P));
    st.tree_ms = ms_since(t0);
    st.levels = tj[0].d.nlev;
    FilterJobs fj{};
    WaveJobs wj{};
    int maxw = 0;
    for (int k = 0; k < n; ++k) {
        const TreeJob& t = tj[k];
        float* C = ws.vol.p + (size_t)P * D * 2 * k;
        float* F = C + (size_t)P * D;
        fj.j[k] = FilterJob{C, F, t.d.parent, t.d.pdist, t.d.first, t.d.child, t.d.lev, t.d.nlev, t.d.table};
        wj.j[k] = WaveJob{C, F, t.d.parent, t.d.pdist, t.d.first, t.d.child, t.task, t.n_up, t.n_dn, t.d.table};
        maxw = std::max(maxw, t.maxw);
    }
    ST_CHK(launch_filter(fj, wj, n, maxw, D, (int)P, s));
    for (int k = 0; k < n; ++k)
        ST_CHK(launch_wta(ws.vol.p + (size_t)P * D * (2 * k + 1), ws.node.p + k * P, (int)P, D, scale, raw[k], s));
    // MeanFilter(disparity, disparity, 3)
    for (int k = 0; k < n; ++k) ST_CHK(launch_median(raw[k], W, H, W, P, 1, 3, out[k], W, P, s));
    return hipSuccess;
}

}  // namespace

StWorkspace::StWorkspace() = default;
StWorkspace::~StWorkspace() = default;

hipError_t StWorkspace::copy_last_tree(int* ints, uint8_t* pdist) const {
    ST_CHK(hipMemcpy(ints, tree_i.p, (size_t)last_tree_ints() * sizeof(int), hipMemcpyDeviceToHost));
    return hipMemcpy(pdist, tree_b.p, (size_t)last_P, hipMemcpyDeviceToHost);
}

hipError_t segment_tree_match(StWorkspace& ws, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch, int D,
                              int scale, float sigma, float tau, uint8_t* d_out, hipStream_t s, StStats* st) {
    if (W < 2 || H < 1 || D < 1 || D > kMaxDisp || scale < 0) return hipErrorInvalidValue;
    const int64_t P = (int64_t)W * H;
    if (P > (1 << 28)) return hipErrorInvalidValue;
    TreeFeed f;
    StDrain drain{ws, s};
    ST_CHK(ws.w8.reserve((size_t)P * 3));
    ST_CHK(ws.grad.reserve((size_t)P * 2));
    ST_CHK(ws.vol.reserve((size_t)P * D * 2));
    ST_CHK(ws.tree_i.reserve((size_t)P * 5 + 2));
    ST_CHK(ws.tree_b.reserve((size_t)P));
    ST_CHK(ws.table.reserve((size_t)256));
    ST_CHK(ws.node.reserve((size_t)P));
    const dim3 rows((unsigned)((W + kST - 1) / kST), (unsigned)H);
    // guide weights -> host
    uint8_t* wr = ws.w8.p;
    uint8_t* wu = ws.w8.p + P;
    hipLaunchKernelGGL(st_weights_kernel, rows, dim3(kST), 0, s, dL, W, H, pitch, wr, wu);
    ST_CHK(hipGetLastError());
    // the edges in the reference's order, sorted on the GPU, -> host
    int nE = 0;
    ST_CHK(gpu_sorted_edges(ws, wr, wu, nullptr, nullptr, 0.f, W, H, false, 0, s, nE));
    // gradients of both views meanwhile (same stream, after the download in order)
    hipLaunchKernelGGL(st_gradient_kernel, rows, dim3(kST), 0, s, dL, W, H, pitch, ws.grad.p);
    hipLaunchKernelGGL(st_gradient_kernel, rows, dim3(kST), 0, s, dR, W, H, pitch, ws.grad.p + P);
    ST_CHK(hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    weight_table(sigma, f.table);
    TreeJob tj{};
    ST_CHK(build_trees(ws, 1, P, W, nE, tau, 1.0f, f, s, &tj));
    uint8_t* raw = ws.w8.p;   // the weights are consumed: reuse for the unfiltered map
    StStats stats;
    ST_CHK(aggregate(ws, &tj, 1, dL, dR, W, H, pitch, D, scale, &raw, &d_out, t0, s, stats));
    if (st) *st = stats;
    ws.last_P = (int)P;
    ws.last_nlev = stats.levels;
    return drain.finish();
}

hipError_t segment_tree_refined_match(StWorkspace& ws, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch,
                                      int D, int scale, float sigma, float tau, uint8_t* d_out, hipStream_t s,
                                      StStats* st) {
    if (W < 2 || H < 1 || D < 1 || D > kMaxDisp || scale < 0) return hipErrorInvalidValue;
    const int64_t P = (int64_t)W * H;
    if (P > (1 << 28)) return hipErrorInvalidValue;
    constexpr float kSigmaOne = 0.08f;   // SIGMA_ONE, Toolkit.h:35
    TreeFeed f1, f2;
    StDrain drain{ws, s};
    ST_CHK(ws.w8.reserve((size_t)P * 10));
    ST_CHK(ws.grad.reserve((size_t)P * 2));
    ST_CHK(ws.vol.reserve((size_t)P * D * 4));
    ST_CHK(ws.tree_i.reserve(((size_t)P * 5 + 2) * 2));
    ST_CHK(ws.tree_b.reserve((size_t)P * 2));
    ST_CHK(ws.table.reserve((size_t)512));
    ST_CHK(ws.node.reserve((size_t)P * 2));
    const dim3 rows((unsigned)((W + kST - 1) / kST), (unsigned)H);
    uint8_t* wrL = ws.w8.p;
    uint8_t* wrR = wrL + 2 * P;
    uint8_t* raw[2] = {wrL + 4 * P, wrL + 5 * P};
    uint8_t* map[2] = {wrL + 6 * P, wrL + 7 * P};   // first-pass maps (left, right) after the 7x7 median
    uint8_t* chk = wrL + 8 * P;
    uint8_t* mask = wrL + 9 * P;
    // colour weights of both views (wr, wu planes each) -> host; gradients
    hipLaunchKernelGGL(st_weights_kernel, rows, dim3(kST), 0, s, dL, W, H, pitch, wrL, wrL + P);
    hipLaunchKernelGGL(st_weights_kernel, rows, dim3(kST), 0, s, dR, W, H, pitch, wrR, wrR + P);
    ST_CHK(hipGetLastError());
    // both views' edges in the reference's order, sorted on the GPU, -> host
    int nE = 0;
    ST_CHK(gpu_sorted_edges(ws, wrL, wrL + P, nullptr, nullptr, 0.f, W, H, false, 0, s, nE));
    ST_CHK(gpu_sorted_edges(ws, wrR, wrR + P, nullptr, nullptr, 0.f, W, H, false, 1, s, nE));
    hipLaunchKernelGGL(st_gradient_kernel, rows, dim3(kST), 0, s, dL, W, H, pitch, ws.grad.p);
    hipLaunchKernelGGL(st_gradient_kernel, rows, dim3(kST), 0, s, dR, W, H, pitch, ws.grad.p + P);
    ST_CHK(hipGetLastError());
    // first run: colour trees of the left and the right view (StereoDisparity.cpp:112-123), unscaled maps
    auto t0 = std::chrono::steady_clock::now();
    weight_table(kSigmaOne, f1.table);
    TreeJob tj[2] = {};
    ST_CHK(build_trees(ws, 2, P, W, nE, tau, 1.0f, f1, s, tj));
    StStats run1, run2;
    ST_CHK(aggregate(ws, tj, 2, dL, dR, W, H, pitch, D, 1, raw, map, t0, s, run1));
    // left-right check (StereoDisparity.cpp:129-147): mask = !occluded
    ST_CHK(launch_lr_check(map[0], W, P, map[1], W, P, 0, W, H, 1, chk, W, P, nullptr, mask, W, P, s));
    // re-segmentation: colour + depth tree on the left view (StereoDisparity.cpp:150-152), its weights
    // from the first left map and mask, sorted on the GPU
    ST_CHK(gpu_sorted_edges(ws, wrL, wrL + P, map[0], mask, (float)D, W, H, true, 0, s, nE));
    // the first run's uploads from page-locked slot 0 were enqueued before this download: once its first
    // chunk has landed, slot 0 is free for the depth tree
    if (!wait_edges(ws, 0, 1)) return hipErrorUnknown;
    // second run on the same cost (the reference recomputes it, :150)
    t0 = std::chrono::steady_clock::now();
    weight_table(sigma, f2.table);
    ST_CHK(build_trees(ws, 1, P, W, nE, tau, 255.0f, f2, s, tj));
    ST_CHK(aggregate(ws, tj, 1, dL, dR, W, H, pitch, D, scale, raw, &d_out, t0, s, run2));
    if (st) *st = StStats{run2.levels, run1.tree_ms + run2.tree_ms};
    ws.last_P = (int)P;
    ws.last_nlev = run2.levels;
    return drain.finish();
}

}  // namespace sm

