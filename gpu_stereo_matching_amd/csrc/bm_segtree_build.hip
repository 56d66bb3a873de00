// bm_segtree_build.hip — the segment tree's stereo (bm_segtree.hip) from edge weights to a tree on the
// device: the edge order (st_edge_keys_kernel, the st_rx_* radix passes, gpu_sorted_edges) and the BFS
// order (st_adj_kernel .. st_task_kernel, gpu_bfs).
#include <algorithm>
#include <climits>

#include "bm_common.h"
#include "bm_segtree_build.h"

namespace sm {
namespace {

// ---- the edge order on the GPU: SegmentTree.cpp:44-69's edges sorted by edge::operator< (weight, then
// b, then a; SegmentTree.h:103-111) ----
// Edges are generated in (b, a) order and sorted stably by weight (LSD radix, 8-bit digits: one pass for
// the integer colour weights, four for the colour + depth floats, whose non-negative values order as
// their bits), which is that order.  Edge index of pixel b = (y, x): in a row y < H - 1 the edges of b
// are (b - 1, b) for x >= 1 then (b + W, b), so row y starts at y (2W - 1); the last row has (b - 1, b)
// only.  Value = 2 b + (edge is (b + W, b)).
__host__ __device__ inline int64_t st_edge_count(int W, int H) { return (int64_t)(H - 1) * (2 * W - 1) + (W - 1); }

// DEPTH = false: key = colour weight (u8); DEPTH = true: CColorDepthWeight::GetWeight (SegmentTree.cpp:
// 204-219) from the colour weight, the first left map and its mask, in the reference's float steps
// (as st_host::depth_weights), key = the float's bits.
template <bool DEPTH>
__global__ __launch_bounds__(kST) void st_edge_keys_kernel(const uint8_t* __restrict__ wr, const uint8_t* __restrict__ wu,
                                                           const uint8_t* __restrict__ disp,
                                                           const uint8_t* __restrict__ mask, float level, int W, int H,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * kST + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int b = y * W + x;
    auto key = [&](int a, int q, uint8_t c) -> uint32_t {
        if constexpr (DEPTH) {
            float w;
            if (mask[a] && mask[q]) {
                const float dispValue = (float)abs((int)disp[a] - (int)disp[q]) / level;
                const float colorValue = (float)c / 255.0f;
                w = 0.5f * dispValue + (1.0f - 0.5f) * colorValue;
            } else {
                w = (float)c / 255.0f;
            }
            return __builtin_bit_cast(uint32_t, w);
        } else {
            return c;
        }
    };
    const int64_t base = (int64_t)y * (2 * W - 1);
    if (y < H - 1) {
        if (x >= 1) {
            keys[base + 2 * x - 1] = key(b - 1, b, wr[b - 1]);   // (b - 1, b): right edge of b - 1
            vals[base + 2 * x - 1] = 2u * (uint32_t)b;
        }
        const int64_t iu = x >= 1 ? base + 2 * x : base;
        keys[iu] = key(b + W, b, wu[b + W]);                     // (b + W, b): upper edge of b + W
        vals[iu] = 2u * (uint32_t)b + 1u;
    } else if (x >= 1) {
        keys[base + x - 1] = key(b - 1, b, wr[b - 1]);
        vals[base + x - 1] = 2u * (uint32_t)b;
    }
}

// one radix pass: single-wave blocks of R * 64 consecutive items, 64 per round (the edge sort: kRxRounds;
// the device BFS's scans and depth sort: kScRounds, 4x the waves for its P-item passes)
constexpr int kRxRounds = 32;
constexpr int kRxIPB = 64 * kRxRounds;
constexpr int kScRounds = 8;
constexpr int kScIPB = 64 * kScRounds;

// gate (the device BFS's sort of depths, st_radix_passes_run): a pass with shift > 0 whose
// digit is 0 for every key (gate[4] = the largest key) does nothing; null for the edge sort
__device__ __forceinline__ bool st_rx_skip(const int* gate, int shift) {
    return gate && shift > 0 && (gate[4] >> shift) == 0;
}

template <int R>
__global__ __launch_bounds__(64) void st_rx_hist_kernel(const uint32_t* __restrict__ keys, int n, int shift,
                                                        uint32_t* __restrict__ hist, int nb, const int* gate) {
    if (st_rx_skip(gate, shift)) return;
    __shared__ uint32_t h[256];
    const int lane = threadIdx.x, blk = blockIdx.x;
    for (int k = lane; k < 256; k += 64) h[k] = 0;
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const int i = blk * R * 64 + r * 64 + lane;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    for (int k = lane; k < 256; k += 64) hist[(size_t)k * nb + blk] = h[k];
}

// exclusive scan of the digit-major counts [256][nb]: each digit's row scanned over the blocks by one
// wave (st_rx_scan_rows_kernel, also writing the row total), then the 256 totals by one wave into the
// digits' bases (st_rx_scan_bases_kernel), which the scatter adds
// wave-wide inclusive scans of uint32_t / U2 (the device BFS's {depth, preorder} pairs, whose halves wrap
// independently: partial sums of the tour's weights go negative)
struct U2 {
    uint32_t a, b;
};
__device__ __forceinline__ U2 operator+(U2 x, U2 y) { return U2{x.a + y.a, x.b + y.b}; }
__device__ __forceinline__ U2 operator-(U2 x, U2 y) { return U2{x.a - y.a, x.b - y.b}; }
__device__ __forceinline__ uint32_t shfl_up_v(uint32_t v, int off) { return __shfl_up(v, off, 64); }
__device__ __forceinline__ U2 shfl_up_v(U2 v, int off) { return U2{__shfl_up(v.a, off, 64), __shfl_up(v.b, off, 64)}; }
__device__ __forceinline__ uint32_t shfl_v(uint32_t v, int l) { return __shfl(v, l, 64); }
__device__ __forceinline__ U2 shfl_v(U2 v, int l) { return U2{__shfl(v.a, l, 64), __shfl(v.b, l, 64)}; }
template <class V>
__device__ __forceinline__ V wave_scan_v(V v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V u = shfl_up_v(v, off);
        if (lane >= off) v = v + u;
    }
    return v;
}
__global__ __launch_bounds__(64) void st_rx_scan_rows_kernel(uint32_t* __restrict__ hist, int nb,
                                                             uint32_t* __restrict__ total, const int* gate, int shift) {
    if (st_rx_skip(gate, shift)) return;
    const int lane = threadIdx.x, dg = blockIdx.x;
    uint32_t* row = hist + (size_t)dg * nb;
    uint32_t run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const uint32_t c = b < nb ? row[b] : 0u;
        const uint32_t inc = wave_scan_v(c, lane);
        if (b < nb) row[b] = run + inc - c;
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) total[dg] = run;
}
__global__ __launch_bounds__(64) void st_rx_scan_bases_kernel(uint32_t* __restrict__ total, const int* gate, int shift) {
    if (st_rx_skip(gate, shift)) return;
    const int lane = threadIdx.x;
    uint32_t run = 0;
    for (int d0 = 0; d0 < 256; d0 += 64) {
        const uint32_t c = total[d0 + lane];
        const uint32_t inc = wave_scan_v(c, lane);
        total[d0 + lane] = run + inc - c;
        run += __shfl(inc, 63, 64);
    }
}

// stable scatter of one pass: an item's position = its digit's offset for the block + the items of the
// same digit before it in the block (earlier rounds: the running counts cnt; this round: the lanes below
// it whose 8 digit bits all agree, from 8 ballots).  FINAL: write the edge records {a, b, w} instead of
// keys and values.
template <bool FINAL, bool DEPTH, int R = kRxRounds>
__global__ __launch_bounds__(64) void st_rx_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                           int n, int shift, const uint32_t* __restrict__ hist,
                                                           const uint32_t* __restrict__ bases, int nb,
                                                           uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                           st_host::Edge* __restrict__ eout, int W, const int* gate,
                                                           int* __restrict__ sidx = nullptr) {
    if (st_rx_skip(gate, shift)) return;
    __shared__ uint32_t cnt[256];
    const int lane = threadIdx.x, blk = blockIdx.x;
    for (int k = lane; k < 256; k += 64) cnt[k] = bases[k] + hist[(size_t)k * nb + blk];
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int r = 0; r < R; ++r) {
        const int i = blk * R * 64 + r * 64 + lane;
        const bool valid = i < n;
        const uint32_t k = valid ? kin[i] : 0u, v = valid ? vin[i] : 0u;
        const uint32_t dg = (k >> shift) & 0xFFu;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (dg >> bit) & 1u;
            const uint64_t bb = __ballot(on);
            peers &= on ? bb : ~bb;
        }
        const uint32_t base = cnt[dg];
        __builtin_amdgcn_wave_barrier();
        // the lowest lane of each digit group advances the digit's count (after every lane has read it)
        if (valid && (peers & lt) == 0) cnt[dg] = base + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            const uint32_t pos = base + (uint32_t)__popcll(peers & lt);
            if constexpr (FINAL) {
                const int b = (int)(v >> 1);
                eout[pos] = st_host::Edge{(v & 1u) ? b + W : b - 1, b,
                                          DEPTH ? __builtin_bit_cast(float, k) : (float)k};
                sidx[v] = (int)pos;   // grid edge v's sorted position (st_adj_kernel)
            } else {
                kout[pos] = k;
                vout[pos] = v;
            }
        }
    }
}

// ---- the BFS order on the GPU (round 4) ----
// The host keeps segment_graph's two passes (sequential: every join's threshold depends on the joins
// before it) and hands over the neighbour lists (st_host::AdjRec, 8 B per pixel: four distance bytes,
// four 2-bit directions, the count).  The BFS of SegmentTree.cpp:97-130 (FIFO from pixel 0, a node's
// children in list order) follows from them without walking the levels one by one:
//  1. an Euler tour of the tree (arc p -> q continues from q to the neighbour after p in q's list,
//     cyclically), ranked by pointer jumping (Wyllie), roots the tree: u is v's parent iff arc u -> v
//     comes before v -> u, and v's subtree has (dist(u -> v) - dist(v -> u) + 1) / 2 nodes, dist being
//     the number of arcs after an arc;
//  2. a node's children in list order (the parent skipped) get the preorder offsets 1 + the sizes of
//     their earlier siblings.  A prefix sum along the tour of {+1, +offset(v)} on each arc into v and
//     {-1, -offset(v)} on each arc out of v's subtree leaves, at the arc into v, exactly the terms of v's
//     ancestors and v (a finished subtree cancels, whatever the tour's order): v's depth and preorder
//     number;
//  3. in a FIFO BFS the nodes of one level come in preorder (by induction over the levels: nodes with
//     different parents follow their parents' order, whose subtrees are disjoint preorder intervals in
//     that order; siblings follow the list order), so the BFS order is the preorder stably sorted by
//     depth (the edge sort's radix passes, those above the deepest level's top bit skipped);
//  4. rank, child words and level offsets from that order; first = 1 + the exclusive scan of the child
//     counts (the BFS appends a node's children at the running end), and each node writes its children's
//     parent index and distance byte there; the wave filter's tasks (wave_tasks' layout) from a scan of
//     the per-level task counts.
// The same arrays as st_host::bfs_tree, bit for bit (tests/test_gpu_segtree.py compares both).
static_assert(sizeof(st_host::AdjRec) == 8, "AdjRec is read as a uint2 {d, dir | n << 16}");

__device__ __forceinline__ int st_nb(int p, uint32_t dir, int k, int W) {
    const uint32_t c = (dir >> (2 * k)) & 3u;
    return c == 0 ? p - 1 : c == 1 ? p + 1 : c == 2 ? p - W : p + W;
}

// The neighbour lists from the host passes' marks (segment_passes): pixel p's tree edges in sorted-edge
// order, as segment_lists appends them (SegmentTree.cpp:74-95), each with its direction code (0: p - 1,
// 1: p + 1, 2: p - W, 3: p + W) and distance min(int(w' * wscale + 0.5), 255), w' = w (+ 5 when
// penalised, st_host::tree_dist).  Grid edge v = 2 b + (edge is (b + W, b)) sits at sorted position
// sidx[v].  Out: AdjRec bits {d, dir | n << 16}.
__global__ __launch_bounds__(kST) void st_adj_kernel(const st_host::Edge* __restrict__ edges, const int* __restrict__ sidx,
                                                     const uint8_t* __restrict__ marks, int W, int P, float wscale,
                                                     uint2* __restrict__ adj) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * kST + threadIdx.x;
    if (p >= P) return;
    const int x = p % W;
    int pos[4];
    uint32_t cd[4];   // direction code | distance << 8
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool ex = c == 0 ? x >= 1 : c == 1 ? x + 1 < W : c == 2 ? p >= W : p + W < P;
        const int v = c == 0 ? 2 * p : c == 1 ? 2 * (p + 1) : c == 2 ? 2 * (p - W) + 1 : 2 * p + 1;
        pos[c] = INT_MAX;
        cd[c] = 0;
        if (ex) {
            const int q = sidx[v];
            const uint8_t m = marks[q];
            if (m & 1u) {
                float w = edges[q].w;
                if (m & 2u) w += 5;
                const float sw = w * wscale;
                pos[c] = q;
                cd[c] = (uint32_t)c | ((uint32_t)min((int)(sw + 0.5f), 255) << 8);
            }
        }
    }
    // sort the (at most 4) tree edges by sorted position
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int j = i; j > 0; --j)
            if (pos[j] < pos[j - 1]) {
                const int tp = pos[j];
                pos[j] = pos[j - 1];
                pos[j - 1] = tp;
                const uint32_t tc = cd[j];
                cd[j] = cd[j - 1];
                cd[j - 1] = tc;
            }
    uint32_t d = 0, dir = 0, n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (pos[k] != INT_MAX) {
            d |= (cd[k] >> 8) << (8 * k);
            dir |= (cd[k] & 3u) << (2 * k);
            ++n;
        }
    adj[p] = make_uint2(d, dir | (n << 16));
}

// arcs: slot k of pixel p is arc 4 p + k {next arc of the tour, 1}; the arc into arc 0 (pixel 0 to its
// first neighbour, where the tour starts) ends it {-1, 0}, and so do the unused slots; rev = the reverse
// arc (an unused slot: itself)
__global__ __launch_bounds__(kST) void st_arc_kernel(const uint2* __restrict__ adj, int P, int W,
                                                     int2* __restrict__ arc, int* __restrict__ rev) {
    const int p = blockIdx.x * kST + threadIdx.x;
    if (p >= P) return;
    const uint2 a = adj[p];
    const int n = (int)(a.y >> 16);
    const uint32_t dir = a.y & 0xFFFFu;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int2 r = make_int2(-1, 0);
        int rv = 4 * p + k;
        if (k < n) {
            const int q = st_nb(p, dir, k, W);
            const uint2 b = adj[q];
            const int nq = (int)(b.y >> 16);
            const uint32_t back = ((dir >> (2 * k)) & 3u) ^ 1u, dq = b.y & 0xFFFFu;
            int j = -1;
#pragma unroll
            for (int z = 0; z < 4; ++z)
                if (z < nq && ((dq >> (2 * z)) & 3u) == back) j = z;
            if (j >= 0) {
                rv = 4 * q + j;
                const int nx = 4 * q + (j + 1 == nq ? 0 : j + 1);
                if (nx != 0) r = make_int2(nx, 1);
            }
        }
        arc[4 * p + k] = r;
        rev[4 * p + k] = rv;
    }
}

// one pointer-jumping step: {next, count} -> {next of next, count + its count}
__global__ __launch_bounds__(kST) void st_list_rank_kernel(const int2* __restrict__ in, int2* __restrict__ out, int n) {
    const int a = blockIdx.x * kST + threadIdx.x;
    if (a >= n) return;
    int2 v = in[a];
    if (v.x >= 0) {
        const int2 w = in[v.x];
        v = make_int2(w.x, v.y + w.y);
    }
    out[a] = v;
}

// parent slot (4: the root) and subtree size of every pixel from the ranked tour
__global__ __launch_bounds__(kST) void st_root_kernel(const uint2* __restrict__ adj, const int2* __restrict__ rk,
                                                      const int* __restrict__ rev, int P, int* __restrict__ psl,
                                                      int* __restrict__ size) {
    const int p = blockIdx.x * kST + threadIdx.x;
    if (p >= P) return;
    int slot = 4, sz = P;
    if (p != 0) {
        const int n = (int)(adj[p].y >> 16);
        for (int k = 0; k < n; ++k) {
            const int da = rk[4 * p + k].y, db = rk[rev[4 * p + k]].y;
            if (db > da) {   // the arc into p comes first: its other end is the parent
                slot = k;
                sz = (db - da + 1) >> 1;
            }
        }
    }
    psl[p] = slot;
    size[p] = sz;
}

// every node writes its children's preorder offsets and its child word (count | distance bytes in list
// order, as bfs_tree's)
__global__ __launch_bounds__(kST) void st_child_kernel(const uint2* __restrict__ adj, const int* __restrict__ psl,
                                                       const int* __restrict__ size, int P, int W,
                                                       int* __restrict__ offs, uint32_t* __restrict__ chw) {
    const int p = blockIdx.x * kST + threadIdx.x;
    if (p >= P) return;
    const uint2 a = adj[p];
    const int n = (int)(a.y >> 16), ps = psl[p];
    int run = 1;
    uint32_t ch = 0, m = 0;
    for (int k = 0; k < n; ++k) {
        if (k == ps) continue;
        const int c = st_nb(p, a.y & 0xFFFFu, k, W);
        const uint32_t dis = (a.x >> (8 * k)) & 0xFFu;
        offs[c] = run;
        run += size[c];
        ch |= dis << (8 * (m + 1));
        ++m;
    }
    chw[p] = ch | m;
    if (p == 0) offs[0] = 0;
}

// {depth, preorder} weights of the arcs in tour order (position = L - 1 - dist, L = 2 (P - 1) arcs):
// into a child {+1, +offset}, to the parent {-1, -offset}; tv = the child an arc enters, else -1
__global__ __launch_bounds__(kST) void st_tour_kernel(const uint2* __restrict__ adj, const int2* __restrict__ rk,
                                                      const int* __restrict__ psl, const int* __restrict__ offs, int P,
                                                      int W, U2* __restrict__ tw, int* __restrict__ tv) {
    const int p = blockIdx.x * kST + threadIdx.x;
    if (p >= P) return;
    const uint2 a = adj[p];
    const int n = (int)(a.y >> 16), ps = psl[p], L = 2 * (P - 1);
    for (int k = 0; k < n; ++k) {
        const int pos = L - 1 - rk[4 * p + k].y;
        if ((unsigned)pos >= (unsigned)L) continue;
        if (k == ps) {
            tw[pos] = U2{~0u, (uint32_t)(-offs[p])};
            tv[pos] = -1;
        } else {
            const int q = st_nb(p, a.y & 0xFFFFu, k, W);
            tw[pos] = U2{1u, (uint32_t)offs[q]};
            tv[pos] = q;
        }
    }
}

// exclusive scan in blocks of kScIPB items, one wave each: the blocks' totals (st_scan_sums_kernel), one
// wave over the totals (st_scan_rows_kernel, also writing the grand total), then the items with their
// block's base (st_scan_apply_kernel: dst(i, exclusive prefix, item))
template <class V, class Src>
__global__ __launch_bounds__(64) void st_scan_sums_kernel(Src src, int n, V* __restrict__ sums) {
    const int lane = threadIdx.x, blk = blockIdx.x;
    V t{};
    for (int r = 0; r < kScRounds; ++r) {
        const int i = blk * kScIPB + r * 64 + lane;
        if (i < n) t = t + src(i);
    }
    t = wave_scan_v(t, lane);
    if (lane == 63) sums[blk] = t;
}
template <class V>
__global__ __launch_bounds__(64) void st_scan_rows_kernel(V* __restrict__ sums, int nb, V* __restrict__ total) {
    const int lane = threadIdx.x;
    V run{};
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const V c = b < nb ? sums[b] : V{};
        const V inc = wave_scan_v(c, lane);
        if (b < nb) sums[b] = run + inc - c;
        run = run + shfl_v(inc, 63);
    }
    if (lane == 0 && total) *total = run;
}
template <class V, class Src, class Dst>
__global__ __launch_bounds__(64) void st_scan_apply_kernel(Src src, int n, const V* __restrict__ sums, Dst dst) {
    const int lane = threadIdx.x, blk = blockIdx.x;
    V run = sums[blk];
    for (int r = 0; r < kScRounds; ++r) {
        const int i = blk * kScIPB + r * 64 + lane;
        const V c = i < n ? src(i) : V{};
        const V inc = wave_scan_v(c, lane);
        if (i < n) dst(i, run + inc - c, c);
        run = run + shfl_v(inc, 63);
    }
}

// the tour's prefix sums -> the nodes in preorder (key = depth, value = pixel); hdr[4] = the largest depth
struct StTourW {
    const U2* tw;
    __device__ U2 operator()(int i) const { return tw[i]; }
};
__global__ __launch_bounds__(64) void st_tour_apply_kernel(const U2* __restrict__ tw, const int* __restrict__ tv, int L,
                                                           const U2* __restrict__ sums, uint32_t* __restrict__ keys,
                                                           uint32_t* __restrict__ vals, int P, int* __restrict__ hdr) {
    const int lane = threadIdx.x, blk = blockIdx.x;
    U2 run = sums[blk];
    uint32_t dmax = 0;
    for (int r = 0; r < kScRounds; ++r) {
        const int i = blk * kScIPB + r * 64 + lane;
        const U2 c = i < L ? tw[i] : U2{0u, 0u};
        const U2 inc = wave_scan_v(c, lane);
        if (i < L) {
            const int v = tv[i];
            const U2 at = run + inc;   // inclusive: the arc into v counts v itself
            if (v >= 0 && at.b < (uint32_t)P) {
                keys[at.b] = at.a;
                vals[at.b] = (uint32_t)v;
                dmax = max(dmax, at.a);
            }
        }
        run = run + shfl_v(inc, 63);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) dmax = max(dmax, (uint32_t)__shfl_xor(dmax, off, 64));
    if (lane == 0) {
        atomicMax(&hdr[4], (int)dmax);
        if (blk == 0) {   // the root: depth 0, preorder 0
            keys[0] = 0;
            vals[0] = 0;
        }
    }
}

// radix passes above the deepest level's top bit are skipped (gate = hdr, gate[4] the largest depth):
// the pass results alternate A -> B -> A.., so the sorted order is in B after an odd number of passes
__device__ __forceinline__ int st_radix_passes_run(const int* hdr, int launched) {
    int e = 0;
    for (int k = 0; k < launched; ++k)
        if (k == 0 || (hdr[4] >> (8 * k)) != 0) ++e;
    return e;
}

// BFS-order arrays from the sorted nodes: rank, child words; lev[d] = the first node of depth d,
// lev[levels] = P; hdr {levels, widest level = 1 (st_level_sums_kernel raises it)}
__global__ __launch_bounds__(kST) void st_bfs_arrays_kernel(const uint32_t* __restrict__ kA, const uint32_t* __restrict__ vA,
                                                            const uint32_t* __restrict__ kB, const uint32_t* __restrict__ vB,
                                                            int launched, const uint32_t* __restrict__ chw, int P,
                                                            int* __restrict__ rank, uint32_t* __restrict__ child,
                                                            int* __restrict__ lev, int* __restrict__ hdr) {
    const int i = blockIdx.x * kST + threadIdx.x;
    if (i >= P) return;
    const bool inB = st_radix_passes_run(hdr, launched) & 1;
    const uint32_t* node = inB ? vB : vA;
    const uint32_t* dep = inB ? kB : kA;
    const uint32_t p = min(node[i], (uint32_t)P - 1u);
    rank[p] = i;
    child[i] = chw[p];
    const int d = (int)min(dep[i], (uint32_t)P - 1u);
    if (i == 0 || dep[i - 1] != dep[i]) lev[d] = i;
    if (i == P - 1) {
        lev[d + 1] = P;
        hdr[0] = d + 1;
        hdr[1] = 1;
    }
}

// first = 1 + the exclusive scan of the child counts; node i writes its children's parent index and
// distance byte (the root's: -1, 0)
struct StChildCount {
    const uint32_t* child;
    __device__ uint32_t operator()(int i) const { return child[i] & 0xFFu; }
};
struct StFirstOut {
    const uint32_t* child;
    int* first;
    int* parent;
    uint8_t* pdist;
    int P;
    __device__ void operator()(int i, uint32_t e, uint32_t n) const {
        const int f = 1 + (int)e;
        first[i] = f;
        const uint32_t ch = child[i];
        for (int z = 0; z < (int)n; ++z) {
            if (f + z < P) {
                parent[f + z] = i;
                pdist[f + z] = (uint8_t)(ch >> (8 * (z + 1)));
            }
        }
        if (i == 0) {
            parent[0] = -1;
            pdist[0] = 0;
        }
    }
};

// tasks of <= 64 nodes per level; the sums pass also raises hdr[1] to the widest level
struct StLevelTasks {
    const int* lev;
    const int* hdr;
    __device__ uint32_t operator()(int l) const { return l < hdr[0] ? (uint32_t)(lev[l + 1] - lev[l] + 63) / 64u : 0u; }
};
struct StIntOut {
    int* out;
    __device__ void operator()(int i, uint32_t e, uint32_t) const { out[i] = (int)e; }
};
__global__ __launch_bounds__(64) void st_level_sums_kernel(const int* __restrict__ lev, int* __restrict__ hdr, int n,
                                                           uint32_t* __restrict__ sums) {
    const int lane = threadIdx.x, blk = blockIdx.x, nlev = hdr[0];
    uint32_t t = 0;
    int wmax = 1;
    for (int r = 0; r < kScRounds; ++r) {
        const int l = blk * kScIPB + r * 64 + lane;
        if (l < n && l < nlev) {
            const int w = lev[l + 1] - lev[l];
            t += (uint32_t)(w + 63) / 64u;
            wmax = max(wmax, w);
        }
    }
    t = wave_scan_v(t, lane);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) wmax = max(wmax, __shfl_xor(wmax, off, 64));
    if (lane == 63) sums[blk] = t;
    if (lane == 0 && blk * kScIPB < nlev) atomicMax(&hdr[1], wmax);
}

// wave_tasks on the device: level l's up tasks after those of the levels below it in the up order
// (levels - 1 .. 0), its down tasks (levels 1 .. levels - 1) after the up list; E = the exclusive scan of
// the per-level task counts, hdr[2] its total (= the up tasks); writes hdr[3] = the down tasks
__global__ __launch_bounds__(kST) void st_task_kernel(const int* __restrict__ lev, const int* __restrict__ E,
                                                      int* __restrict__ hdr, int P, int4* __restrict__ task) {
    const int l = blockIdx.x * kST + threadIdx.x;
    const int nlev = hdr[0];
    if (l >= P || l >= nlev) return;
    const int stride = hdr[1] + 64, total = hdr[2];
    const int lo = lev[l], hi = lev[l + 1], q = l & 1, nt = (hi - lo + 63) / 64;
    auto cut = [&](int4* dst, int other) {
        const int rb = kStLvlOff + ((q ^ 1) * stride - other) * 4;
        for (int t = 0; t < nt; ++t) {
            const int s0 = lo + 64 * t;
            dst[t] = make_int4(s0, min(64, hi - s0) - 1, kStLvlOff + (q * stride + s0 - lo) * 4, rb);
        }
    };
    cut(task + (total - E[l] - nt), l + 1 < nlev ? lev[l + 1] : lo);
    if (l >= 1) cut(task + total + E[l] - 1, lev[l - 1]);   // level 0 has one task
    if (l == 0) hdr[3] = total - 1;
}

// One LSD radix pass on stream s over n items in nb blocks of R * 64: the blocks' digit counts, their
// scans, then the stable scatter from (kin, vin) into (kout, vout) or, FINAL, into the edge records eout
// and their positions sidx (DEPTH: float keys)
template <int R, bool FINAL, bool DEPTH>
void radix_pass(const uint32_t* kin, const uint32_t* vin, int n, int shift, uint32_t* hist, uint32_t* bases, int nb,
                uint32_t* kout, uint32_t* vout, st_host::Edge* eout, int W, const int* gate, int* sidx, hipStream_t s) {
    hipLaunchKernelGGL(st_rx_hist_kernel<R>, dim3((unsigned)nb), dim3(64), 0, s, kin, n, shift, hist, nb, gate);
    hipLaunchKernelGGL(st_rx_scan_rows_kernel, dim3(256), dim3(64), 0, s, hist, nb, bases, gate, shift);
    hipLaunchKernelGGL(st_rx_scan_bases_kernel, dim3(1), dim3(64), 0, s, bases, gate, shift);
    hipLaunchKernelGGL((st_rx_scatter_kernel<FINAL, DEPTH, R>), dim3((unsigned)nb), dim3(64), 0, s, kin, vin, n, shift,
                       hist, bases, nb, kout, vout, eout, W, gate, sidx);
}

// ---- the device BFS (st_adj_kernel ..): scratch and launch sequence ----
struct BfsScratch {
    int2* arcA;        // 4P {next arc, arcs counted}, ping-pong
    int2* arcB;
    U2* tw;            // L = 2 (P - 1) tour weights
    uint2* adj;        // P neighbour lists
    U2* usums;         // tour scan block sums
    int* rev;          // 4P reverse arcs
    int* tv;           // L
    int* psl;          // P parent slots
    int* size;         // P subtree sizes
    int* offs;         // P preorder offsets
    uint32_t* chw;     // P child words per pixel
    uint32_t *kA, *vA, *kB, *vB;   // P each: depth keys and pixels of the radix passes
    uint32_t* hist;    // 256 (nb + 1)
    uint32_t* sums;    // nb + 2
    int* E;            // P + 2
    int* hdr;          // 8: {levels, widest level, up tasks, down tasks, largest depth}
    uint8_t* marks;    // nE: the host passes' marks
};

int64_t rx_blocks(int64_t n) { return (n + kScIPB - 1) / kScIPB; }

// The scratch carved from `base` in this order (8- and 16-B arrays first, at even offsets); `ints`
// receives its size.  A null base only counts.
BfsScratch bfs_scratch(int* base, int64_t P, int64_t nE, size_t& ints) {
    const int64_t L = 2 * (P - 1), nb = rx_blocks(P), nbL = rx_blocks(L);
    BfsScratch b{};
    ints = 0;
    auto take = [&](int64_t n) {
        int* r = base ? base + ints : nullptr;
        ints += (size_t)n;
        return r;
    };
    b.arcA = reinterpret_cast<int2*>(take(8 * P));
    b.arcB = reinterpret_cast<int2*>(take(8 * P));
    b.tw = reinterpret_cast<U2*>(take(2 * L));
    b.adj = reinterpret_cast<uint2*>(take(2 * P));
    b.usums = reinterpret_cast<U2*>(take(2 * (nbL + 2)));
    b.rev = take(4 * P);
    b.tv = take(L);
    b.psl = take(P);
    b.size = take(P);
    b.offs = take(P);
    b.chw = reinterpret_cast<uint32_t*>(take(P));
    b.kA = reinterpret_cast<uint32_t*>(take(P));
    b.vA = reinterpret_cast<uint32_t*>(take(P));
    b.kB = reinterpret_cast<uint32_t*>(take(P));
    b.vB = reinterpret_cast<uint32_t*>(take(P));
    b.hist = reinterpret_cast<uint32_t*>(take(256 * (nb + 1)));
    b.sums = reinterpret_cast<uint32_t*>(take(nb + 2));
    b.E = take(P + 2);
    b.hdr = take(8);
    b.marks = reinterpret_cast<uint8_t*>(take((nE + 3) / 4));
    return b;
}

int ceil_log2(int64_t n) {
    int r = 0;
    while (((int64_t)1 << r) < n) ++r;
    return r;
}

}  // namespace

hipError_t gpu_sorted_edges(StWorkspace& ws, const uint8_t* wr, const uint8_t* wu, const uint8_t* disp,
                            const uint8_t* mask, float level, int W, int H, bool depth, int slot, hipStream_t s,
                            int& nE) {
    const int64_t n64 = st_edge_count(W, H);
    if (n64 <= 0 || n64 > (1 << 30)) return hipErrorInvalidValue;
    const int n = (int)n64, nb = (n + kRxIPB - 1) / kRxIPB;
    StSlot& sl = ws.slot[slot];
    // keys / values x 2, digit counts; the edge records (3 dwords each) and sorted positions per slot
    ST_CHK(ws.sortbuf.reserve((size_t)4 * n + (size_t)256 * (nb + 1)));
    ST_CHK(sl.dedge.reserve((size_t)3 * n));
    ST_CHK(sl.sidx.reserve((size_t)2 * W * H));
    ST_CHK(sl.h_edges.reserve((size_t)3 * n));
    uint32_t* k0 = ws.sortbuf.p;
    uint32_t* v0 = k0 + n;
    uint32_t* k1 = v0 + n;
    uint32_t* v1 = k1 + n;
    uint32_t* hist = v1 + n;
    uint32_t* bases = hist + (size_t)256 * nb;
    static_assert(sizeof(st_host::Edge) == 12, "an edge record is 3 dwords of dedge / h_edges");
    auto* edges = reinterpret_cast<st_host::Edge*>(sl.dedge.p);
    const dim3 rows((unsigned)((W + kST - 1) / kST), (unsigned)H);
    if (depth)
        hipLaunchKernelGGL(st_edge_keys_kernel<true>, rows, dim3(kST), 0, s, wr, wu, disp, mask, level, W, H, k0, v0);
    else
        hipLaunchKernelGGL(st_edge_keys_kernel<false>, rows, dim3(kST), 0, s, wr, wu, disp, mask, level, W, H, k0, v0);
    const int top = depth ? 24 : 0;   // the last pass's shift: four 8-bit passes for the floats, one for the bytes
    for (int shift = 0; shift < top; shift += 8) {
        radix_pass<kRxRounds, false, false>(k0, v0, n, shift, hist, bases, nb, k1, v1, edges, W, nullptr, nullptr, s);
        std::swap(k0, k1);
        std::swap(v0, v1);
    }
    if (depth)
        radix_pass<kRxRounds, true, true>(k0, v0, n, top, hist, bases, nb, k1, v1, edges, W, nullptr, sl.sidx.p, s);
    else
        radix_pass<kRxRounds, true, false>(k0, v0, n, top, hist, bases, nb, k1, v1, edges, W, nullptr, sl.sidx.p, s);
    ST_CHK(hipGetLastError());
    nE = n;
    // down in kEdgeChunks copies, each followed by its event: the host tree's first pass starts on the
    // first chunk (wait_edges) while the rest is still in flight
    constexpr int K = StSlot::kEdgeChunks;
    const int chunk = (n + K - 1) / K;
    sl.edge_chunk = chunk;
    auto* h_edges = reinterpret_cast<st_host::Edge*>(sl.h_edges.p);
    for (int k = 0; k < K; ++k) {
        ST_CHK(sl.edge_ev[k].create());
        const int lo = std::min(n, k * chunk), hi = std::min(n, lo + chunk);
        if (hi > lo)
            ST_CHK(hipMemcpyAsync(h_edges + lo, edges + lo, (size_t)(hi - lo) * sizeof(st_host::Edge),
                                  hipMemcpyDeviceToHost, s));
        ST_CHK(hipEventRecord(sl.edge_ev[k].ev, s));
    }
    return hipSuccess;
}

bool wait_edges(StWorkspace& ws, int slot, int upto) {
    const StSlot& sl = ws.slot[slot];
    const int chunk = std::max(sl.edge_chunk, 1);
    const int last = std::min(StSlot::kEdgeChunks, (upto + chunk - 1) / chunk);
    for (int k = 0; k < last; ++k)
        if (hipEventSynchronize(sl.edge_ev[k].ev) != hipSuccess) return false;
    return true;
}

hipError_t gpu_bfs(StWorkspace& ws, int scr, int P, int W, int nE, float wscale, const DevTree& d, int4* task,
                   int* h_hdr, hipStream_t s) {
    StSlot& sl = ws.slot[scr];
    size_t ints = 0;
    bfs_scratch(nullptr, P, nE, ints);
    ST_CHK(sl.bfs.reserve(ints));
    const BfsScratch b = bfs_scratch(sl.bfs.p, P, nE, ints);
    const int L = 2 * (P - 1), nb = (int)rx_blocks(P), nbL = (int)rx_blocks(L);
    ST_CHK(hipMemsetAsync(b.hdr, 0, 8 * sizeof(int), s));
    ST_CHK(hipMemcpyAsync(b.marks, sl.h_marks.p, (size_t)nE, hipMemcpyHostToDevice, s));
    const dim3 gP((unsigned)((P + kST - 1) / kST)), g4P((unsigned)((4 * (int64_t)P + kST - 1) / kST));
    // 0. the neighbour lists from the marks and the edge slot's sorted edges
    hipLaunchKernelGGL(st_adj_kernel, gP, dim3(kST), 0, s, reinterpret_cast<const st_host::Edge*>(sl.dedge.p),
                       sl.sidx.p, b.marks, W, P, wscale, b.adj);
    // 1. rank the tour: jumps of 2^r cover its L arcs after ceil(log2 L) steps; root it
    hipLaunchKernelGGL(st_arc_kernel, gP, dim3(kST), 0, s, b.adj, P, W, b.arcA, b.rev);
    int2 *ain = b.arcA, *aout = b.arcB;
    for (int r = ceil_log2(L); r > 0; --r) {
        hipLaunchKernelGGL(st_list_rank_kernel, g4P, dim3(kST), 0, s, ain, aout, 4 * P);
        std::swap(ain, aout);
    }
    hipLaunchKernelGGL(st_root_kernel, gP, dim3(kST), 0, s, b.adj, ain, b.rev, P, b.psl, b.size);
    // 2. preorder offsets, the tour's prefix sums -> depth and preorder of every node
    hipLaunchKernelGGL(st_child_kernel, gP, dim3(kST), 0, s, b.adj, b.psl, b.size, P, W, b.offs, b.chw);
    hipLaunchKernelGGL(st_tour_kernel, gP, dim3(kST), 0, s, b.adj, ain, b.psl, b.offs, P, W, b.tw, b.tv);
    hipLaunchKernelGGL((st_scan_sums_kernel<U2, StTourW>), dim3((unsigned)nbL), dim3(64), 0, s, StTourW{b.tw}, L, b.usums);
    hipLaunchKernelGGL(st_scan_rows_kernel<U2>, dim3(1), dim3(64), 0, s, b.usums, nbL, nullptr);
    hipLaunchKernelGGL(st_tour_apply_kernel, dim3((unsigned)nbL), dim3(64), 0, s, b.tw, b.tv, L, b.usums, b.kA, b.vA, P,
                       b.hdr);
    // 3. stable sort by depth (< P): 8-bit digits up to P - 1's top bit, passes above the deepest level's
    // top bit skipped on the device
    uint32_t *k0 = b.kA, *v0 = b.vA, *k1 = b.kB, *v1 = b.vB;
    uint32_t* bases = b.hist + (size_t)256 * nb;
    int launched = 0;
    for (int shift = 0; shift < std::max(1, ceil_log2(P)); shift += 8, ++launched) {
        radix_pass<kScRounds, false, false>(k0, v0, P, shift, b.hist, bases, nb, k1, v1, nullptr, W, b.hdr, nullptr, s);
        std::swap(k0, k1);
        std::swap(v0, v1);
    }
    // 4. the BFS-order arrays, first / parent / pdist, the wave filter's tasks
    hipLaunchKernelGGL(st_bfs_arrays_kernel, gP, dim3(kST), 0, s, b.kA, b.vA, b.kB, b.vB, launched, b.chw, P, d.rank,
                       d.child, d.lev, b.hdr);
    const StChildCount cc{d.child};
    hipLaunchKernelGGL((st_scan_sums_kernel<uint32_t, StChildCount>), dim3((unsigned)nb), dim3(64), 0, s, cc, P, b.sums);
    hipLaunchKernelGGL(st_scan_rows_kernel<uint32_t>, dim3(1), dim3(64), 0, s, b.sums, nb, nullptr);
    hipLaunchKernelGGL((st_scan_apply_kernel<uint32_t, StChildCount, StFirstOut>), dim3((unsigned)nb), dim3(64), 0, s, cc,
                       P, b.sums, StFirstOut{d.child, d.first, d.parent, d.pdist, P});
    hipLaunchKernelGGL(st_level_sums_kernel, dim3((unsigned)nb), dim3(64), 0, s, d.lev, b.hdr, P, b.sums);
    hipLaunchKernelGGL(st_scan_rows_kernel<uint32_t>, dim3(1), dim3(64), 0, s, b.sums, nb,
                       reinterpret_cast<uint32_t*>(b.hdr + 2));
    hipLaunchKernelGGL((st_scan_apply_kernel<uint32_t, StLevelTasks, StIntOut>), dim3((unsigned)nb), dim3(64), 0, s,
                       StLevelTasks{d.lev, b.hdr}, P, b.sums, StIntOut{b.E});
    hipLaunchKernelGGL(st_task_kernel, gP, dim3(kST), 0, s, d.lev, b.E, b.hdr, P, task);
    ST_CHK(hipGetLastError());
    return hipMemcpyAsync(h_hdr, b.hdr, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
}

}  // namespace sm
