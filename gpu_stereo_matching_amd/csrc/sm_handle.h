// sm_handle.h — what the C ABI's translation units (sm_capi*.hip) share: the handle, its device buffers, the
// scope that orders workspace users between streams, error reporting, and the helpers of the host calls.
// Internal: nothing here is exported (the library is built with -fvisibility=hidden).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/sm_hip.h"
#include "bm_box_plan.h"
#include "bm_common.h"
#include "bm_guided.h"
#include "bm_segtree.h"
#include "bm_speckle_plan.h"

namespace smh {

// One error text per thread, shared by every file of the C API (defined in sm_capi.hip; GroupWorker::loop copies
// its thread's text to the caller's).  __thread, not thread_local: a thread_local declared extern is reached
// through an init wrapper whose weak reference does not resolve under hidden visibility.
extern __thread char g_err[512] __attribute__((visibility("hidden")));

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define SM_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return smh::fail(e_ == hipErrorOutOfMemory ? SM_ERR_OUT_OF_MEMORY : SM_ERR_LAUNCH, \
                             "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline hipStream_t stream_of(void* stream) { return static_cast<hipStream_t>(stream); }
// An on/off switch of the A/B runs, from the environment: "0" turns one that is on by default off, "1" another on
inline bool env_switch(const char* name, bool dflt) {
    const char* e = getenv(name);
    return !e ? dflt : dflt ? e[0] != '0' : e[0] == '1';
}

// A grow-only device buffer: `cap` usable bytes, and `slack` readable bytes behind them.
struct DevBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    size_t slack = 0;

    // At least `bytes` usable bytes.  Never shrinks; the old block is freed before the new one is allocated, and
    // an allocation failure leaves the buffer empty (SM_ERR_OUT_OF_MEMORY).
    int reserve(size_t bytes) {
        if (cap >= bytes) return SM_OK;
        (void)release();
        SM_HIP(hipMalloc(&p, bytes + slack));
        cap = bytes;
        return SM_OK;
    }
    hipError_t release() {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return e;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// A DevBuf that calls on different streams share.  Its memory is reached through WsScope::get alone, so no call
// can touch it without taking part in the ordering.
class SharedBuf {
  public:
    explicit SharedBuf(size_t slack = 0) { b_.slack = slack; }
    bool allocated() const { return b_.p != nullptr; }
    hipError_t release() { return b_.release(); }   // the caller has drained the handle's work first

  private:
    friend class WsScope;
    DevBuf b_;
};

}  // namespace smh

struct sm_handle {
    int device = 0;
    int max_w = 0, max_h = 0, max_d = 0;
    hipStream_t stream = nullptr;
    // frame buffers (one frame; batched device calls use caller memory)
    uint8_t* d_left = nullptr;
    uint8_t* d_right = nullptr;
    uint8_t* d_disp = nullptr;
    // Workspaces of the passes, grown on demand and shared by calls on any stream (WsScope):
    // dense planes: raw left map (median), right map, filtered right map, mirrored pair; the sub-pixel calls' d0
    // planes (volume call) or their unfiltered views (SM_PARAM_SUBPIX_MEDIAN, SubpixMedianWs)
    smh::SharedBuf lr;
    smh::SharedBuf rpart;   // fused right view: per-tile right-key partials
    // cost volumes, V planes of the wide path, right keys.  64 readable bytes past the end: box_sad_kernel reads
    // whole 8-byte words at the planes' last bytes
    smh::SharedBuf vol{64};
    smh::SharedBuf spk;     // speckle filter: u32 labels and u32 counts of the frames in flight (bm_speckle_plan.h)
    smh::SharedBuf boxq;    // matrix-pipe box launches that draw their tiles from a queue: the u32 grab counter
    // Staging of the host calls, grown on demand.  Only the handle's own stream touches them, in calls that end
    // in a synchronise, so they need no ordering:
    smh::DevBuf maps;   // float maps of the host remap / rectify-map calls
    smh::DevBuf aux;    // right map / mask (sm_block_match_lr_u8), the sub-pixel host call's outputs
    smh::DevBuf bgr;    // BGR pair of sm_block_match_bgr_u8 and the segment-tree calls
    // RCCL d-slice group mode (sm_group_dslice_block_match_u8): slice keys, this member's reduced
    // key chunk, its uint8 chunk and the gathered map
    smh::DevBuf dsl;
    float guided_eps = 6.5025f;  // 1e-4 * 255^2 (AD units)
    int staged_group = 8;        // SM_STAGED frames per launch group (SM_PARAM_STAGED_GROUP)
    int sgm_p1 = 0, sgm_p2 = 0;  // SM_AGG_SGM penalties (SM_PARAM_SGM_P1 / _P2), 0 = auto
    int sgm_paths = 4;           // SM_PARAM_SGM_PATHS: 4 scan directions, or 8 with the diagonals
    // host calls record the upload / match / download split (SM_PARAM_STAGE_TIMING): 0 off, 1 on, 2 auto
    // (default: on once sm_last_stage_ms has been called on the handle, or when SM_VERBOSE is set)
    int stage_timing = 2;
    int box_kernel = 0;          // SM_PARAM_BOX_KERNEL: 0 auto, 1 VALU kernels, 2 matrix-pipe kernel
    int box_workgroups = 0;      // SM_PARAM_BOX_WORKGROUPS: 0 auto, n >= 1 workgroups per matrix-pipe launch
    int box_queue_workgroups = 0;   // SM_PARAM_BOX_QUEUE_WORKGROUPS: 0 auto, n >= 1 queue workgroups at any launch size
    int uniqueness = 0;          // SM_PARAM_UNIQUENESS: 0 off, 1..99 the sub-pixel calls' uniqueness ratio
    int speckle_size = 0;        // SM_PARAM_SPECKLE_SIZE: 0 off, else the largest region the matching calls remove
    int speckle_range = 1;       // SM_PARAM_SPECKLE_RANGE: whole disparities joined into one region, 0..255
    int fill_gap = 0;            // SM_PARAM_FILL_GAP: 0 off, else the longest run of a row the matching calls fill
    int min_disp = 0;            // SM_PARAM_MIN_DISP: what plane 0 of a cost volume stands for (SM_PAIRS_IN_VIEW calls)
    int subpix_median = 0;       // SM_PARAM_SUBPIX_MEDIAN: 0 off, 1..3 the sub-pixel calls' median radius (bm_median16.hip)
    // SM_PARAM_WORKSPACE_POISON: 0 off, v in 1..256 every call first fills the workspaces it takes (WsScope::get)
    // and the frame buffers it uploads into (upload_pair) with byte v - 1
    int ws_poison = 0;
    int guided_subpix = 0;       // SM_PARAM_GUIDED_SUBPIX: 1 the sub-pixel calls take SM_AGG_GUIDED, 0 they refuse it
    bool stage_requested = false;
    // The shared workspaces serve every call on the handle while calls run on the stream they are given: the
    // end of each pass that used one is recorded here, and a pass on another stream waits for it first, so two
    // streams never write the same workspace at once (WsScope).
    hipEvent_t scratch_ev = nullptr;
    hipStream_t scratch_stream = nullptr;
    bool scratch_pending = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float stage_ms[3] = {0.f, 0.f, 0.f};
    // segment-tree path (sm_segment_tree_match_bgr_u8): device workspace and the last call's stats
    sm::StWorkspace st;
    sm::StStats st_stats;
    float st_total_ms = 0.f;
    bool st_valid = false;
    // staged box path: events around the last launch group's AD / SAD / WTA kernels
    // (sm_last_staged_kernel_ms reports them per frame of that group)
    hipEvent_t kev[4] = {nullptr, nullptr, nullptr, nullptr};
    int kev_frames = 1;
    bool kev_valid = false;
};

namespace smh {

// One call's use of the handle's shared workspaces on stream s.  The first get() makes s wait for the last pass
// that used a workspace, if that ran on another stream and may still be running; leaving a scope that handed out
// a pointer records the event the next pass on another stream waits for.  A call that takes no workspace (the
// headline box pass, guided without LR) neither waits nor records: one marker costs the host call microseconds.
// A scope belongs to one handle and one call.  It takes no lock: a handle belongs to one host thread
// (include/sm_hip.h), and the members of a group (group_bands, the d-slice workers) each run on their
// own thread with their own handle.
class WsScope {
  public:
    WsScope(sm_handle* h, hipStream_t s) : h_(h), s_(s) {}
    WsScope(const WsScope&) = delete;
    WsScope& operator=(const WsScope&) = delete;
    ~WsScope() {
        if (!used_ || drained_) return;
        // a record that fails (a broken context, which the next call reports) falls back to waiting for the stream
        const bool recorded = hipEventRecord(h_->scratch_ev, s_) == hipSuccess;
        if (!recorded) (void)hipStreamSynchronize(s_);
        h_->scratch_stream = s_;
        h_->scratch_pending = recorded;
    }

    hipStream_t stream() const { return s_; }

    // `bytes` of buffer b (grown if need be) for kernels on this scope's stream
    template <class T>
    int get(SharedBuf& b, size_t bytes, T** out) {
        *out = nullptr;
        int rc = touch();
        const uint8_t* before = b.b_.p;
        if (!rc) rc = b.b_.reserve(bytes);
        if (!rc && h_->ws_poison) rc = poison(b, b.b_.p != before);
        if (!rc) *out = b.b_.as<T>();
        return rc;
    }
    // Joins the ordering without taking a buffer (SM_SCRATCH_EVENT=1: every pass waits and records, for A/B)
    int touch() {
        if (used_) return SM_OK;
        used_ = true;
        if (h_->scratch_pending && h_->scratch_stream != s_) SM_HIP(hipStreamWaitEvent(s_, h_->scratch_ev, 0));
        return SM_OK;
    }
    // The end of a host call: waits for the stream, downloads included, so nothing is recorded.  A scope that
    // joined the ordering has then seen the last pass on any other stream finish as well.
    int drain() {
        SM_HIP(hipStreamSynchronize(s_));
        drained_ = true;
        if (used_) h_->scratch_pending = false;
        return SM_OK;
    }

  private:
    // SM_PARAM_WORKSPACE_POISON: the whole of b, slack included, filled on s_ when this scope first takes it, and
    // again when a later get had to grow it (the new block holds none of the call's data).  A second get of a
    // buffer that stays where it is leaves the call's live data alone.
    int poison(SharedBuf& b, bool regrown) {
        const SharedBuf* const all[] = {&h_->lr, &h_->rpart, &h_->vol, &h_->spk, &h_->boxq};
        unsigned bit = 0;
        for (unsigned i = 0; i < sizeof(all) / sizeof(all[0]); ++i)
            if (all[i] == &b) bit = 1u << i;
        if ((poisoned_ & bit) && !regrown) return SM_OK;
        poisoned_ |= bit;
        if (b.b_.cap + b.b_.slack == 0) return SM_OK;
        SM_HIP(hipMemsetAsync(b.b_.p, h_->ws_poison - 1, b.b_.cap + b.b_.slack, s_));
        return SM_OK;
    }

    sm_handle* h_;
    hipStream_t s_;
    bool used_ = false, drained_ = false;
    unsigned poisoned_ = 0;   // the handle's shared buffers this scope has filled
};

// ---- argument checks (sm_capi.hip; the cost rules in sm_capi_volume.hip) ----
int check_geometry(const sm_handle* h, int width, int height, int pitch, int radius, int num_disp);
// SM_ERR_CAPACITY unless the frame fits what sm_create sized the handle for (num_disp 0: a call without one)
int check_capacity(const sm_handle* h, int width, int height, int num_disp);
int census_check(int width, int radius, unsigned flags);
// SM_ERR_INVALID_ARG, naming the speckle filter, when the handle's filter is on: the first check of a call that
// cannot honour it (`why`: what the filter's regions cross there)
inline int speckle_refuse(const sm_handle* h, const char* call, const char* why) {
    if (!h || h->speckle_size == 0) return SM_OK;
    return fail(SM_ERR_INVALID_ARG, "%s cannot honour the speckle filter (SM_PARAM_SPECKLE_SIZE %d): %s", call,
                h->speckle_size, why);
}
// The speckle filter (bm_speckle.hip) in place on `batch` device maps of elem_bytes 1 or 2, through the handle's
// `spk` workspace (sm_capi_speckle.hip).  The arguments have been checked.
int run_speckle(WsScope& ws, sm_handle* h, void* map, int elem_bytes, int W, int H, int pitch, int batch,
                int64_t fstride, int max_size, int max_diff, uint8_t* mask);
// The same for the row fill (SM_PARAM_FILL_GAP): a call whose result is no map, or that does not run the steps the
// fill comes after
inline int fill_refuse(const sm_handle* h, const char* call, const char* why) {
    if (!h || h->fill_gap == 0) return SM_OK;
    return fail(SM_ERR_INVALID_ARG, "%s cannot honour the row fill (SM_PARAM_FILL_GAP %d): %s", call, h->fill_gap, why);
}
// The row fill (bm_fill.hip) in place on `batch` device maps of elem_bytes 1 or 2, on stream s; it takes no
// workspace, so it joins no WsScope (sm_capi_fill.hip).  The arguments have been checked, except the frame
// against fill_pass_ok.
int run_fill(hipStream_t s, void* map, int elem_bytes, int W, int H, int pitch, int batch, int64_t fstride, int max_gap);
// SM_PARAM_SUBPIX_MEDIAN (sm_capi_median16.hip): the sub-pixel calls' steps between the two views' WTA and the
// speckle filter, one frame at a time through dense uint16 planes of P = W * H elements in the `lr` workspace:
// [left q][right q][filtered right q], the second only with a right view (SM_LR_CHECK, or a right16 output) and the
// third only when the check runs without a right16 output.  The caller takes subpix_median_bytes from the workspace
// before its first launch and has the WTA write the unfiltered views into `left` and `right`.
struct SubpixMedianWs {
    uint16_t *left = nullptr, *right = nullptr, *right_out = nullptr;
};
inline size_t subpix_median_bytes(int64_t P, bool lr, bool right16) {
    return (size_t)(2 * P) * (lr && !right16 ? 3 : lr || right16 ? 2 : 1);
}
inline SubpixMedianWs subpix_median_ws(uint8_t* base, int64_t P, bool lr, bool right16) {
    SubpixMedianWs w;
    w.left = reinterpret_cast<uint16_t*>(base);
    if (lr || right16) w.right = w.left + P;
    if (lr && !right16) w.right_out = w.left + 2 * P;
    return w;
}
// median16 of w.left into disp16 and of w.right into right16 (or w.right_out); with lr the check on (q + 8) >> 4 of
// the two filtered maps; mask (optional) = final q != 0
int run_subpix_median(hipStream_t s, const SubpixMedianWs& w, int W, int H, int radius, uint16_t* disp16, int pitch,
                      uint16_t* right16, bool lr, uint8_t* mask);
int sgm_check(int width, int radius, unsigned flags, int p1, int p2, int* p1_out, int* p2_out);
// SM_PAIRS_IN_VIEW and SM_PARAM_MIN_DISP (sm_capi_volume.hip), before any device work.
// A call that keeps a cost volume: the flag needs one (SM_AGG_SGM, SM_COST_CENSUS, or `subpix`, a sub-pixel call,
// with any aggregation it takes) and none of SM_AGG_GUIDED, SM_STAGED, SM_DEVICE_CU_GRID; a minimum disparity > 0
// needs the flag; the largest disparity d0 + num_disp - 1 fits the map (255, sub-pixel 4095).  *out: the rule to run.
int pairs_check(const sm_handle* h, unsigned flags, int num_disp, bool subpix, sm::Pairs* out);
// A call that cannot honour either (`call`: the row-band, d-slice and slice-key calls): names the flag, or the
// parameter when the handle's minimum disparity is > 0
int pairs_refuse(const sm_handle* h, unsigned flags, const char* call);

// SM_AGG_GUIDED's radii (bm_guided_plan.h): every guided entry rejects the others before it takes a workspace
inline int guided_radius_check(int radius) {
    if (radius > sm::kMaxGuidedRadius)
        return fail(SM_ERR_INVALID_ARG, "guided aggregation: radius %d > %d", radius, sm::kMaxGuidedRadius);
    return SM_OK;
}

inline uint32_t seed_key(int radius) {
    const uint32_t win = 2u * (uint32_t)radius + 1u;
    return (50u * win * win) << 8;  // Device.cu:37 start value, d field 0
}

// ---- host <-> device copies (sm_capi.hip) ----
hipError_t copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t row_bytes, size_t rows,
                  hipMemcpyKind kind, hipStream_t s);
// A host pair of W x H frames into the handle's frame buffers, on s.  With right_dev, a pair whose right frame
// sits right behind the left one goes up as one copy, and *right_dev says where the right frame then is
// (d_left + P instead of d_right); without it, always two copies into d_left and d_right.
int upload_pair(sm_handle* h, const uint8_t* left, const uint8_t* right, int W, int H, int pitch, hipStream_t s,
                uint8_t** right_dev = nullptr);

// ---- one frame's cost-volume workspace in `vol` ----
// [head][costs u16 2PD][right keys u32 4P], then with the census cost [census L u64 8P][census R u64 8P]; every
// part starts 256-B aligned.  The head is the u8 cost volume (AD or Hamming, PD), or with SGM the u32 sums S
// (4PD), whose own head doubles as that u8 volume: the box sums have consumed it before S is zeroed.
struct VolumeLayout { size_t sad, rkeys, cl, cr, bytes; };
inline VolumeLayout volume_layout(int64_t P, int D, bool sgm, bool census) {
    VolumeLayout w;
    w.sad = align256((size_t)((sgm ? 4 : 1) * P * D));
    w.rkeys = w.sad + align256((size_t)(2 * P * D));
    w.cl = w.rkeys + align256((size_t)(4 * P));
    w.cr = w.cl + (census ? align256((size_t)(8 * P)) : 0);
    w.bytes = w.cr + (census ? align256((size_t)(8 * P)) : 0);
    return w;
}

// SM_AGG_GUIDED in the sub-pixel calls: [biased u32 costs 4PD][the LR check's d0 planes, the rkeys region 4P]; no
// u16 costs and no census words, so sad == rkeys and cl == cr == bytes
inline VolumeLayout guided_volume_layout(int64_t P, int D) {
    VolumeLayout w;
    w.sad = w.rkeys = align256((size_t)(4 * P * D));
    w.cl = w.cr = w.bytes = w.rkeys + align256((size_t)(4 * P));
    return w;
}

// The last step of run_volume, by where its result goes: the 8-bit maps (left into lmap; right, when right_map
// is given, into dense W x H planes), or with disp16 the 1/16-px maps of bm_subpix.hip (right16 / mask: dense
// W x H planes or null; lr: the LR check runs).
struct VolumeOut {
    uint8_t* lmap = nullptr;
    int lpitch = 0;
    int64_t lstride = 0;
    uint8_t* right_map = nullptr;
    uint16_t* disp16 = nullptr;
    int opitch = 0;
    int64_t ostride = 0;
    uint16_t* right16 = nullptr;
    uint8_t* mask = nullptr;
    bool lr = false;
};
// SM_AGG_SGM, SM_COST_CENSUS and the sub-pixel calls (sm_capi_volume.hip)
int run_volume(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
               int64_t fstride, int radius, int D, bool sgm, bool census, int p1, int p2, const sm::Pairs& pr,
               const VolumeOut& o);
// SM_AGG_GUIDED in the sub-pixel calls (sm_capi_volume.hip): per frame the one-pass guided volume, biased, into the
// volume workspace (guided_volume_layout), then run_volume's sub-pixel step on it.  o.disp16 is set.
int run_guided_subpix(WsScope& ws, sm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, int pitch, int batch,
                      int64_t fstride, int radius, int D, const VolumeOut& o);

// ---- the box pass (sm_capi.hip) ----
// Where the right view of a box pass goes, by what the plan was asked for.
struct BoxRightOut {
    // RightWant::Map: dR [batch][H][pitch], dense (pitch W, stride W * H) unless `check`; stored mirrored when the
    // plan's right view is Mirrored
    uint8_t* map = nullptr;
    int pitch = 0;
    int64_t stride = 0;
    // Tile / Fused only: 1 applies the LR check in the same pass (launch_box_match_lr: a.disp receives the checked
    // map; `map` and `mask`, the valid mask, are optional)
    int check = 0;
    uint8_t* mask = nullptr;
    uint32_t* keys = nullptr;    // RightWant::Keys: the slice's right keys [batch][H][W]
    uint8_t* mirror = nullptr;   // plan.mirror_planes dense planes of W * H * batch bytes
};
// Issues the launches of plan p = plan_box_pass(a's geometry and batch, what `r` receives): the left pass into
// a.disp / a.keys, the right view into `r`.  The plan's workspaces are taken from the handle through ws, each once.
int run_box_pass(WsScope& ws, sm_handle* h, sm::MatchArgs a, int batch, const sm::BoxPlan& p, const BoxRightOut& r);

// Host-pointer pass over one frame (or one row band of a frame: sm_group_*; sm_capi.hip).  Only result rows
// [keep0, keep1) are downloaded, into disp_out / right_out / mask_out pointing at row keep0.
int host_match_rows(sm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                    int radius, int num_disp, unsigned flags, int keep0, int keep1, uint8_t* disp_out,
                    uint8_t* right_out, uint8_t* mask_out, int out_pitch);

// ---- the d-slice split (sm_capi_slice.hip; the group call in sm_capi_group.hip runs it across devices) ----
// One plan for every path that shards a frame over d: the C group call, its one-device rehearsal and
// the torch path (sharding.py calls sm_dslice_plan).  Member k of n scans d in [kD/n, (k+1)D/n)
// (Device.cu:43-61: the d planes are independent); the P keys are padded with the "no match" key to
// Ppad = n * chunk so that the MIN reduce-scatter hands member k the pixels [k*chunk, (k+1)*chunk),
// and the all-gather puts chunk k back at offset k*chunk.
// The pair itself is split by rows (round 4): member k uploads only image rows
// [k*rows_per, (k+1)*rows_per) of each frame over its own PCIe link, into slot k of an n*rows_per-row
// buffer, and an in-place RCCL all-gather over xGMI assembles both frames on every member before the
// key pass.  No halo is needed: the gathered frames are the whole pair.
struct DslicePlan {
    int lo, hi;
    int64_t chunk, padded;
    int rows_per, row_lo, row_hi;   // this member's upload rows [row_lo, row_hi) (empty past the frame)
};
DslicePlan dslice_plan(int64_t P, int D, int n, int k, int H = 1);

// One d-sliced frame: geometry, aggregation and whether the LR check runs (SM_LR_CHECK: a second key map
// for the right view, C_R(u, d) = C_L(u + d, d), reduced with its own MIN; StereoHelper.cpp:156-180)
struct DsliceCfg {
    int W, H, radius, D;
    bool guided, lr;
    int64_t P() const { return (int64_t)W * H; }
};

// What the d-slice mode takes: box or guided, optionally the LR check (the group call and its rehearsal)
int dslice_check(const DsliceCfg& c, unsigned flags);

// Member workspace: keys [padded] | reduced chunk [chunk] | uint8 chunk [chunk] | gathered map [padded] |
// gathered left frame [n * rows_per * W] | gathered right frame [same] | with LR the right view's
// keys [padded] | reduced chunk [chunk] | uint8 chunk [chunk] | gathered right map [padded]
// (each region 256-B aligned)
struct DsliceWs {
    uint32_t *keys, *mine;
    uint8_t *mine8, *map, *gl, *gr;
    uint32_t *rkeys, *rmine;
    uint8_t *rmine8, *rmap;
    int64_t slot;   // bytes of one member's row slot (rows_per * W)
    size_t bytes;
};
DsliceWs dslice_ws(uint8_t* base, const DslicePlan& p, int n, int W, bool lr);
int dslice_upload_rows(const DslicePlan& p, const DsliceWs& w, int k, const uint8_t* left, const uint8_t* right, int W,
                       int pitch, hipStream_t s);
int dslice_keys(WsScope& ws, sm_handle* h, const DslicePlan& p, const DsliceCfg& c, const uint8_t* dL,
                const uint8_t* dR, uint32_t* keys, uint32_t* rkeys);
int dslice_finalise(const uint32_t* mine, int64_t chunk, int radius, bool guided, uint8_t* mine8, hipStream_t s);

}  // namespace smh
