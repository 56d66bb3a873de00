// bm_segtree_build.h — between bm_segtree_build.hip ("from edge weights to a tree on the device") and
// bm_segtree.hip (the cost, the filters and the two pipelines).
#pragma once
#include "bm_segtree.h"
#include "bm_segtree_host.h"

#define ST_CHK(x)                          \
    do {                                   \
        const hipError_t e_ = (x);         \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

namespace sm {

constexpr int kST = 256;

// LDS layout of st_filter_wave_kernel (bm_segtree.hip), whose level-buffer offsets st_task_kernel
// (bm_segtree_build.hip) writes into the task records
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));   // 16 B in memory (a 3-vector is padded)
constexpr int kStBlk = 16;                              // tasks per block: the 64 lanes load 16 int4 records
constexpr int kStNodeOff = 1024;                        // LDS: [0, 1024) the weight table
constexpr int kStRecOff = kStNodeOff + kStBlk * 64 * (int)sizeof(u32x3);   // [kStBlk][64 lanes] node operands
constexpr int kStZeroOff = kStRecOff + 2 * kStBlk * 16;  // [2 blocks][kStBlk] records, then a float 0
constexpr int kStLvlOff = kStZeroOff + 16;               // then the level buffers

// One tree on the device: workspace slot k holds int [rank | parent | first | child | lev] (5P + 2),
// uint8 pdist (P) and the 256-entry weight table.
struct DevTree {
    int* rank;
    int* parent;
    int* first;
    uint32_t* child;
    int* lev;
    uint8_t* pdist;
    float* table;
    int nlev;
};

// tasks per tree slot: up and down each <= P / 64 + levels, levels <= P
inline size_t task_slot_cap(int64_t P) { return (size_t)(2 * (P + P / 64 + 2)); }

// The sorted edges of one tree into page-locked host slot `slot` of the workspace (asynchronous on s).
// DEPTH: colour + depth weights from the left map `disp` and its mask.
hipError_t gpu_sorted_edges(StWorkspace& ws, const uint8_t* wr, const uint8_t* wu, const uint8_t* disp,
                            const uint8_t* mask, float level, int W, int H, bool depth, int slot, hipStream_t s,
                            int& nE);

// Blocks until the sorted edges [0, upto) of `slot` have landed on the host (the chunk events of
// gpu_sorted_edges); false if an event reports an error.
bool wait_edges(StWorkspace& ws, int slot, int upto);

// The neighbour lists and their BFS from edge slot scr's marks (h_marks, page-locked, nE bytes, consumed
// once the copy has run) and sorted edges (dedge / sidx, from gpu_sorted_edges) into device tree d and
// the wave filter's tasks into `task` (task_slot_cap(P) int4), all on stream s; the header {levels, widest
// level, up tasks, down tasks} lands in page-locked h_hdr once the stream has passed the copy this
// enqueues last.
hipError_t gpu_bfs(StWorkspace& ws, int scr, int P, int W, int nE, float wscale, const DevTree& d, int4* task,
                   int* h_hdr, hipStream_t s);

}  // namespace sm
