// bm_segtree.h — segment-tree aggregation (STMatching ST-1 and ST-2) on the GPU: internal interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <memory>

namespace sm {
namespace st_host {
struct HostTree;
}

// Grow-only buffers of the workspace: reserve(n) keeps a block of >= n elements (growing frees the old
// block first; a failed allocation leaves the buffer empty), the destructor frees it.  Device memory and
// page-locked host memory.
template <class T, bool PINNED>
struct StBuf {
    T* p = nullptr;
    size_t n = 0;
    StBuf() = default;
    StBuf(const StBuf&) = delete;
    StBuf& operator=(const StBuf&) = delete;
    ~StBuf() { drop(); }
    hipError_t reserve(size_t want) {
        if (n >= want) return hipSuccess;
        drop();
        void* q = nullptr;
        const hipError_t e =
            PINNED ? hipHostMalloc(&q, want * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, want * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q);
        n = want;
        return hipSuccess;
    }

 private:
    void drop() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        n = 0;
    }
};
template <class T>
using StDev = StBuf<T, false>;
template <class T>
using StPinned = StBuf<T, true>;

// An event (no timing) and a non-blocking stream, created by the first create() and destroyed with the owner
struct StEvent {
    hipEvent_t ev = nullptr;
    StEvent() = default;
    StEvent(const StEvent&) = delete;
    StEvent& operator=(const StEvent&) = delete;
    ~StEvent() {
        if (ev) (void)hipEventDestroy(ev);
    }
    hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
};
struct StStream {
    hipStream_t s = nullptr;
    StStream() = default;
    StStream(const StStream&) = delete;
    StStream& operator=(const StStream&) = delete;
    ~StStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

struct StStats {
    int levels = 0;        // BFS levels of the (last) tree
    float tree_ms = 0.f;   // time of the tree builds (host lists + the BFS, until its level count is back)
};

// One edge / tree slot of the workspace: ST-1 uses slot 0, ST-2 slot 0 for the left view's colour tree and
// then its colour + depth tree, slot 1 for the right view's colour tree.
struct StSlot {
    static constexpr int kEdgeChunks = 4;
    StDev<uint32_t> dedge;       // the sorted edges on the device (st_host::Edge, 3 dwords each)
    StPinned<uint32_t> h_edges;  // their page-locked host copy
    // the sorted edges come down in kEdgeChunks copies, each followed by its event (the host passes start
    // on the first chunk)
    StEvent edge_ev[kEdgeChunks];
    int edge_chunk = 0;          // edges per chunk of the last download
    StDev<int> sidx;             // 2P: each grid edge's sorted position
    StPinned<uint8_t> h_marks;   // nE: the host passes' per-edge marks
    StDev<int> bfs;              // the device BFS's scratch (bm_segtree_build.hip: bfs_scratch)
    // the host BFS path's page-locked tree: ints in the device slot's layout (rank, parent, first, child:
    // 4P; level offsets: P + 2), then pdist (P bytes): one DMA copy per tree
    StPinned<int> h_tree;
    std::unique_ptr<st_host::HostTree> tree;   // the host passes' forest (and host BFS), reused across calls
};

// Device workspace of segment_tree_match, owned by a handle, grown on demand.  Not copyable (its members
// own their blocks); the owner drains the streams that used it before destroying it.
struct StWorkspace {
    StDev<uint8_t> w8;      // ST-1 3P: edge weights (2P), then the unfiltered map; ST-2 10P: both views'
                            // weights (4P), then the pass maps, the checked map and the mask
    StDev<float> grad;      // 2P: gradients of both views
    StDev<float> vol;       // ST-1 2PD, ST-2 4PD: cost / leaf-to-root sums, filtered cost ([D][P], BFS order)
    StDev<int> tree_i;      // (5P + 2) per tree: rank, parent, first, child, level offsets
    StDev<uint8_t> tree_b;  // P per tree: distance to the parent
    StDev<float> table;     // 256 per tree: exp(-i / (255 sigma))
    StDev<int> task;        // per tree: the wave filter's level tasks (int4 each), up to 2 * (P + levels)
    StDev<int> node;        // P per tree: BFS index -> pixel (the WTA's output order)
    StDev<uint32_t> sortbuf;   // edge sort: keys and values (2 x 2 nE), digit counts
    StSlot slot[2];
    StStream side;          // ST-2: the right view's BFS runs on it beside the left's
    StEvent side_ev;        // recorded on `side` after that BFS
    StPinned<int> h_hdr;    // per tree slot {levels, widest level, up tasks, down tasks}
    StEvent bfs_ev;         // recorded after the device BFS's header copies
    StWorkspace();
    ~StWorkspace();

    // Tree slot 0 of the last completed call: its pixels (0: none yet), levels, and the ints of its arrays
    // (rank, parent, first, child words: 4 P; level offsets: levels + 1), which copy_last_tree brings to
    // the host with its parent distances (P bytes).  The caller has drained the handle's stream.
    int last_pixels() const { return last_P; }
    int last_levels() const { return last_nlev; }
    int64_t last_tree_ints() const { return 4 * (int64_t)last_P + last_nlev + 1; }
    hipError_t copy_last_tree(int* ints, uint8_t* pdist) const;

 private:
    int last_P = 0, last_nlev = 0;   // written by the two entry points below
    friend hipError_t segment_tree_match(StWorkspace&, const uint8_t*, const uint8_t*, int, int, int, int, int, float,
                                         float, uint8_t*, hipStream_t, StStats*);
    friend hipError_t segment_tree_refined_match(StWorkspace&, const uint8_t*, const uint8_t*, int, int, int, int, int,
                                                 float, float, uint8_t*, hipStream_t, StStats*);
};

// stereo_disparity_normal (StereoDisparity.cpp:57-89) on device BGR frames (3 bytes per pixel, row
// pitch `pitch`): D = max_dis_level, tau = TAU (Toolkit.h:34); d_out [H][W] uint8, pitch W.
// Synchronous on stream s (the tree is built on the host from the GPU's edge weights).
hipError_t segment_tree_match(StWorkspace& ws, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch, int D,
                              int scale, float sigma, float tau, uint8_t* d_out, hipStream_t s, StStats* st);

// stereo_disparity_iteration, ST-2 (StereoDisparity.cpp:91-160), same arguments: first-pass left and
// right maps on colour trees of each view (sigma SIGMA_ONE = 0.08, Toolkit.h:35), the left-right check,
// then a colour + depth tree (CColorDepthWeight) on the left view with `sigma`.
hipError_t segment_tree_refined_match(StWorkspace& ws, const uint8_t* dL, const uint8_t* dR, int W, int H, int pitch,
                                      int D, int scale, float sigma, float tau, uint8_t* d_out, hipStream_t s,
                                      StStats* st);

}  // namespace sm
