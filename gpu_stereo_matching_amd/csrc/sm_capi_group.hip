// sm_capi_group.hip — the C ABI's multi-GPU groups (sm_create_group): one handle and one persistent host thread
// per device; row bands, frame batches, and the RCCL d-slice mode.
// Pageable host copies block their calling thread, so each device gets its own worker thread; a
// call hands every worker its job (a row band of one frame, or a share of a frame batch) and
// waits for all of them.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "sm_handle.h"

using namespace smh;

namespace {

struct GroupWorker {
    sm_handle* h = nullptr;
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = false, quit = false;
    int rc = SM_OK;
    std::string err;

    void loop() {
        for (;;) {
            std::function<int()> j;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return has_job || quit; });
                if (quit) return;
                j = std::move(job);
                has_job = false;
            }
            const int r = j();
            std::lock_guard<std::mutex> lk(m);
            rc = r;
            err = r ? std::string(g_err) : std::string();   // this thread's text, for the caller's (group_run)
            done = true;
            cv.notify_all();
        }
    }
};

}  // namespace

struct sm_group {
    std::vector<GroupWorker*> w;
    // one RCCL communicator per member for the d-slice mode, created on first use (ncclCommInitAll)
    std::vector<ncclComm_t> comms;
};

namespace {

// Runs jobs[k] on worker k (jobs may be shorter than the group: the rest stay idle) and returns the
// first failure, its message re-raised on the calling thread.
int group_run(sm_group* g, std::vector<std::function<int()>>& jobs) {
    const size_t n = jobs.size() < g->w.size() ? jobs.size() : g->w.size();
    for (size_t k = 0; k < n; ++k) {
        GroupWorker* w = g->w[k];
        std::lock_guard<std::mutex> lk(w->m);
        w->job = std::move(jobs[k]);
        w->has_job = true;
        w->done = false;
        w->cv.notify_all();
    }
    int rc = SM_OK;
    std::string err;
    for (size_t k = 0; k < n; ++k) {
        GroupWorker* w = g->w[k];
        std::unique_lock<std::mutex> lk(w->m);
        w->cv.wait(lk, [&] { return w->done; });
        if (w->rc && !rc) {
            rc = w->rc;
            err = "device " + std::to_string(w->h->device) + ": " + w->err;
        }
    }
    if (rc) return fail(rc, "%s", err.c_str());
    return SM_OK;
}

// RCCL is loaded on first use of the d-slice mode, not linked: callers that never shard a frame over
// disparities carry no RCCL dependency.  The soname matches the copy PyTorch-ROCm ships, so inside a
// torch process dlopen returns the already-loaded library (one RCCL per process).
struct RcclApi {
    decltype(&ncclCommInitAll) init_all;
    decltype(&ncclCommDestroy) destroy;
    decltype(&ncclReduceScatter) reduce_scatter;
    decltype(&ncclAllGather) all_gather;
    decltype(&ncclGetErrorString) error_string;
    decltype(&ncclCommAbort) abort;
    decltype(&ncclCommGetAsyncError) async_error;
};

const RcclApi* rccl_api() {
    static std::mutex mu;
    static RcclApi api;
    static int state = 0;   // 0 untried, 1 loaded, -1 unavailable
    std::lock_guard<std::mutex> lk(mu);
    if (state == 0) {
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        state = -1;
        if (lib) {
            api.init_all = reinterpret_cast<decltype(api.init_all)>(dlsym(lib, "ncclCommInitAll"));
            api.destroy = reinterpret_cast<decltype(api.destroy)>(dlsym(lib, "ncclCommDestroy"));
            api.reduce_scatter = reinterpret_cast<decltype(api.reduce_scatter)>(dlsym(lib, "ncclReduceScatter"));
            api.all_gather = reinterpret_cast<decltype(api.all_gather)>(dlsym(lib, "ncclAllGather"));
            api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(lib, "ncclGetErrorString"));
            api.abort = reinterpret_cast<decltype(api.abort)>(dlsym(lib, "ncclCommAbort"));
            api.async_error = reinterpret_cast<decltype(api.async_error)>(dlsym(lib, "ncclCommGetAsyncError"));
            if (api.init_all && api.destroy && api.reduce_scatter && api.all_gather && api.error_string && api.abort &&
                api.async_error)
                state = 1;
        }
    }
    return state == 1 ? &api : nullptr;
}

#define SM_RCCL(api, call)                                                                         \
    do {                                                                                           \
        ncclResult_t r_ = (call);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return fail(SM_ERR_LAUNCH, "%s failed: %s (%s:%d)", #call, (api)->error_string(r_), __FILE__, \
                        __LINE__);                                                                 \
    } while (0)

int group_comms(sm_group* g) {
    if (!g->comms.empty()) return SM_OK;
    const RcclApi* api = rccl_api();
    if (!api) return fail(SM_ERR_DEVICE, "d-slice mode: librccl.so.1 not loadable (%s)", dlerror());
    const int n = (int)g->w.size();
    std::vector<int> devs(n);
    for (int k = 0; k < n; ++k) {
        devs[k] = g->w[k]->h->device;
        for (int j = 0; j < k; ++j)
            if (devs[j] == devs[k])
                return fail(SM_ERR_INVALID_ARG, "d-slice mode needs distinct devices (device %d twice)", devs[k]);
    }
    std::vector<ncclComm_t> comms(n, nullptr);
    SM_RCCL(api, api->init_all(comms.data(), n, devs.data()));
    g->comms = comms;
    return SM_OK;
}

// Test hook (include/sm_hip.h): SM_DSLICE_FAULT="<member>:<phase>" makes that member fail in phase
// "keys" (before any collective) or "collective" (instead of enqueuing its reduce-scatter).
bool dslice_fault(int k, const char* phase) {
    const char* e = getenv("SM_DSLICE_FAULT");
    if (!e) return false;
    const char* colon = strchr(e, ':');
    return colon && atoi(e) == k && strcmp(colon + 1, phase) == 0;
}

// Phase 1 of member k (its worker thread): workspace and the upload of its rows, then a stream sync
// so that every local failure (allocation, copy) is known before any member enqueues a collective.  A
// member that fails here returns before phase 2 starts, so nobody waits on it.
int dslice_member_upload(sm_handle* h, int k, int n, const uint8_t* left, const uint8_t* right, const DsliceCfg& c,
                         int pitch) {
    const DslicePlan p = dslice_plan(c.P(), c.D, n, k, c.H);
    SM_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (dslice_fault(k, "keys")) return fail(SM_ERR_LAUNCH, "d-slice member %d: injected fault (keys)", k);
    int rc = h->dsl.reserve(dslice_ws(nullptr, p, n, c.W, c.lr).bytes);
    if (rc) return rc;
    // what the key pass will take from the shared workspaces is sized here too, so that no allocation can fail
    // after the pair all-gathers are enqueued: exactly what the slice's box plan takes (none for the
    // strip kernel without LR), or the guided right view's per-tile partials
    WsScope ws(h, s);
    uint8_t* unused = nullptr;
    if (p.hi > p.lo && !c.guided) {
        const sm::BoxPlan plan = sm::plan_box_pass({c.W, c.H, c.W, c.radius, p.lo, p.hi, 1},
                                                   c.lr ? sm::RightWant::Keys : sm::RightWant::None);
        if (plan.vol_bytes) rc = ws.get(h->vol, plan.vol_bytes, &unused);
        if (!rc && plan.rpart_bytes) rc = ws.get(h->rpart, plan.rpart_bytes, &unused);
    } else if (p.hi > p.lo && c.lr) {
        rc = ws.get(h->rpart, sm::guided_right_partial_bytes(c.W, c.H, c.radius, p.hi - p.lo, 1), &unused);
    }
    if (rc) return rc;
    const DsliceWs w = dslice_ws(h->dsl.p, p, n, c.W, c.lr);
    rc = dslice_upload_rows(p, w, k, left, right, c.W, pitch, s);
    if (rc) return rc;
    SM_HIP(hipStreamSynchronize(s));
    return SM_OK;
}

// Shared by the members of one phase-2 call: a member that cannot take part raises `abort`, and
// every member then aborts its communicator instead of waiting for the missing peer.
struct DsliceSync {
    std::atomic<bool> abort{false};
};

// Phase 2 of member k: in-place all-gathers of the pair's row slots, the slice keys, MIN reduce-scatter,
// finalise, all-gather of the map, member 0 downloads.  With LR the right view's keys take the same
// reduce-scatter / finalise (their d field) / all-gather, and member 0 applies StereoDisparity.cpp:136-147
// to the gathered maps before the download.  Waits by polling its stream and the shared abort flag (and
// RCCL's async error), so that no member blocks forever on a collective a failed peer never joined (the
// ncclCommAbort pattern).  On any failure the member's communicator is aborted and its slot set to null
// (the group re-creates them).
int dslice_member_collect(sm_handle* h, const RcclApi* api, ncclComm_t* comm, DsliceSync* sync, int k, int n,
                          const DsliceCfg& c, uint8_t* disp_out, int out_pitch) {
    const DslicePlan p = dslice_plan(c.P(), c.D, n, k, c.H);
    const DsliceWs w = dslice_ws(h->dsl.p, p, n, c.W, c.lr);
    hipStream_t s = h->stream;
    // every failure of phase 2 goes through bail, so the others stop polling for this member
    auto bail = [&](int code, const char* what) {
        sync->abort.store(true);
        if (*comm) (void)api->abort(*comm);
        *comm = nullptr;
        return fail(code, "d-slice member %d: %s", k, what);
    };
    if (hipSetDevice(h->device) != hipSuccess) return bail(SM_ERR_LAUNCH, "hipSetDevice failed");
    if (dslice_fault(k, "collective")) return bail(SM_ERR_LAUNCH, "injected fault (collective)");
    // the pair: every member's row slot to every member (in place: slot k is this member's send buffer)
    if (api->all_gather(w.gl + k * w.slot, w.gl, (size_t)w.slot, ncclUint8, *comm, s) != ncclSuccess ||
        api->all_gather(w.gr + k * w.slot, w.gr, (size_t)w.slot, ncclUint8, *comm, s) != ncclSuccess)
        return bail(SM_ERR_LAUNCH, "ncclAllGather (pair rows) failed");
    {
        WsScope ws(h, s);   // sized in phase 1: nothing is allocated here
        if (dslice_keys(ws, h, p, c, w.gl, w.gr, w.keys, w.rkeys))
            return bail(SM_ERR_LAUNCH, "slice keys launch failed");
    }
    // box keys (SAD << 8 | d) compare as unsigned (the right view's too); guided keys are signed
    const ncclDataType_t kt = c.guided ? ncclInt32 : ncclUint32;
    if (api->reduce_scatter(w.keys, w.mine, (size_t)p.chunk, kt, ncclMin, *comm, s) != ncclSuccess)
        return bail(SM_ERR_LAUNCH, "ncclReduceScatter failed");
    // right keys: signed for both aggregations (box right keys are sign-flipped, kRightKeyFlip)
    if (c.lr && api->reduce_scatter(w.rkeys, w.rmine, (size_t)p.chunk, ncclInt32, ncclMin, *comm, s) != ncclSuccess)
        return bail(SM_ERR_LAUNCH, "ncclReduceScatter (right keys) failed");
    if (dslice_finalise(w.mine, p.chunk, c.radius, c.guided, w.mine8, s) ||
        (c.lr && sm::launch_keys_low_byte(w.rmine, p.chunk, w.rmine8, s) != hipSuccess))
        return bail(SM_ERR_LAUNCH, "finalise launch failed");
    if (api->all_gather(w.mine8, w.map, (size_t)p.chunk, ncclUint8, *comm, s) != ncclSuccess)
        return bail(SM_ERR_LAUNCH, "ncclAllGather failed");
    if (c.lr && api->all_gather(w.rmine8, w.rmap, (size_t)p.chunk, ncclUint8, *comm, s) != ncclSuccess)
        return bail(SM_ERR_LAUNCH, "ncclAllGather (right map) failed");
    if (c.lr && k == 0 &&
        sm::launch_lr_check(w.map, c.W, c.P(), w.rmap, c.W, c.P(), 0, c.W, c.H, 1, w.map, c.W, c.P(), nullptr, nullptr,
                            c.W, c.P(), s) != hipSuccess)
        return bail(SM_ERR_LAUNCH, "LR check launch failed");
    for (;;) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return bail(SM_ERR_LAUNCH, hipGetErrorString(q));
        ncclResult_t async = ncclSuccess;
        if (api->async_error(*comm, &async) != ncclSuccess || async != ncclSuccess)
            return bail(SM_ERR_LAUNCH, "RCCL asynchronous error");
        if (sync->abort.load()) return bail(SM_ERR_LAUNCH, "aborted: another member failed");
        std::this_thread::yield();
    }
    if (k == 0) {
        const hipError_t e = copy2d(disp_out, out_pitch, w.map, c.W, c.W, c.H, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return bail(SM_ERR_LAUNCH, "map download failed");
    }
    return SM_OK;
}

// Rows a band must see on each side of its output rows: the aggregation window (2r for the
// guided filter's nested windows, at least 16 so that the guided kernel's 8-row float running
// sums of the kept rows start on rows the band holds exactly) plus the median's 3.
int group_halo(int radius, unsigned flags) {
    int h = (flags & SM_AGG_GUIDED) ? (2 * radius > 16 ? 2 * radius : 16) : radius;
    return h + ((flags & SM_MEDIAN) ? 3 : 0);
}

// What every call that splits one frame over the group checks first
int group_frame_check(const sm_group* g, const uint8_t* left, const uint8_t* right, const uint8_t* disp_out, int width,
                      int height, int pitch, int out_pitch, unsigned flags) {
    if (!g) return fail(SM_ERR_INVALID_ARG, "null group");
    if (!left || !right || !disp_out) return fail(SM_ERR_INVALID_ARG, "null image pointer");
    if (flags & SM_DEVICE_CU_GRID)   // the literal grid is anchored at the frame's corner: not row-local
        return fail(SM_ERR_INVALID_ARG, "SM_DEVICE_CU_GRID needs whole frames (sm_group_block_match_batch_u8)");
    if (width <= 0 || height <= 0 || pitch < width || out_pitch < width)
        return fail(SM_ERR_INVALID_ARG, "bad frame geometry %dx%d pitch %d out_pitch %d", width, height, pitch,
                    out_pitch);
    return SM_OK;
}

int group_bands(sm_group* g, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                int radius, int num_disp, unsigned flags, uint8_t* disp_out, uint8_t* right_out, uint8_t* mask_out,
                int out_pitch) {
    int rc = group_frame_check(g, left, right, disp_out, width, height, pitch, out_pitch, flags);
    if (rc) return rc;
    for (const GroupWorker* w : g->w) {   // regions cross the bands
        rc = speckle_refuse(w->h, "the row-band group call",
                            "regions cross the bands (sm_group_block_match_batch_u8 runs whole frames)");
        if (rc) return rc;
        rc = pairs_refuse(w->h, flags, "the row-band group call");   // the whole-frame volume paths alone take them
        if (rc) return rc;
    }
    if (flags & SM_AGG_SGM)   // the vertical paths run through every row of the frame
        return fail(SM_ERR_INVALID_ARG,
                    "SM_AGG_SGM needs whole frames: its vertical paths cross the row bands (sm_group_block_match_batch_u8)");
    if (flags & SM_COST_CENSUS)   // a band's replicated border is not the frame's
        return fail(SM_ERR_INVALID_ARG,
                    "SM_COST_CENSUS needs whole frames: the census window's replicated border would differ at the "
                    "band edges (sm_group_block_match_batch_u8)");
    // bands of whole 32-row tiles; each band's input starts on a 32-row boundary so that its tile
    // grid is the full frame's (the kept rows are then bit-identical to a single-device pass)
    constexpr int kAlign = 32;
    const int n = (int)g->w.size();
    const int tiles = (height + kAlign - 1) / kAlign;
    const int per = ((tiles + n - 1) / n) * kAlign;
    const int halo = group_halo(radius, flags);
    std::vector<std::function<int()>> jobs;
    for (int k = 0; k < n; ++k) {
        const int y0 = k * per, y1 = (k + 1) * per < height ? (k + 1) * per : height;
        if (y0 >= height) break;
        const int a = y0 - halo <= 0 ? 0 : ((y0 - halo) / kAlign) * kAlign;
        const int b = y1 + halo < height ? y1 + halo : height;
        sm_handle* h = g->w[k]->h;
        const int64_t ro = (int64_t)a * pitch, oo = (int64_t)y0 * out_pitch;
        jobs.push_back([=]() -> int {
            return host_match_rows(h, left + ro, right + ro, width, b - a, pitch, radius, num_disp, flags, y0 - a,
                                   y1 - a, disp_out + oo, right_out ? right_out + oo : nullptr,
                                   mask_out ? mask_out + oo : nullptr, out_pitch);
        });
    }
    return group_run(g, jobs);
}

}  // namespace

extern "C" {

SM_API int sm_create_group(int ngpu, const int* devices, int max_width, int max_height, int max_disp,
                           sm_group** out) {
    if (!out) return fail(SM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    if (ngpu < 1 || ngpu > 64) return fail(SM_ERR_INVALID_ARG, "group size %d out of [1, 64]", ngpu);
    sm_group* g = new (std::nothrow) sm_group();
    if (!g) return fail(SM_ERR_OUT_OF_MEMORY, "host alloc");
    for (int k = 0; k < ngpu; ++k) {
        sm_handle* h = nullptr;
        const int rc = sm_create(devices ? devices[k] : k, max_width, max_height, max_disp, &h);
        if (rc) {
            const std::string msg = g_err;
            sm_destroy_group(g);
            return fail(rc, "group member %d: %s", k, msg.c_str());
        }
        GroupWorker* w = new (std::nothrow) GroupWorker();
        if (!w) {
            sm_destroy(h);
            sm_destroy_group(g);
            return fail(SM_ERR_OUT_OF_MEMORY, "host alloc");
        }
        w->h = h;
        w->th = std::thread([w] { w->loop(); });
        g->w.push_back(w);
    }
    *out = g;
    return SM_OK;
}

SM_API int sm_destroy_group(sm_group* g) {
    if (!g) return SM_OK;
    if (!g->comms.empty()) {
        const RcclApi* api = rccl_api();
        for (ncclComm_t c : g->comms)
            if (c && api) (void)api->destroy(c);
    }
    for (GroupWorker* w : g->w) {
        {
            std::lock_guard<std::mutex> lk(w->m);
            w->quit = true;
            w->cv.notify_all();
        }
        if (w->th.joinable()) w->th.join();
        sm_destroy(w->h);
        delete w;
    }
    delete g;
    return SM_OK;
}

SM_API int sm_group_size(const sm_group* g, int* n) {
    if (!g || !n) return fail(SM_ERR_INVALID_ARG, "null argument");
    *n = (int)g->w.size();
    return SM_OK;
}

SM_API int sm_group_set_param_f(sm_group* g, int param, float value) {
    if (!g) return fail(SM_ERR_INVALID_ARG, "null group");
    for (GroupWorker* w : g->w) {
        const int rc = sm_set_param_f(w->h, param, value);
        if (rc) return rc;
    }
    return SM_OK;
}

SM_API int sm_group_block_match_u8(sm_group* g, const uint8_t* left, const uint8_t* right, int width, int height,
                                   int pitch, int radius, int num_disp, unsigned flags, uint8_t* disp_out,
                                   int out_pitch) {
    return group_bands(g, left, right, width, height, pitch, radius, num_disp, flags, disp_out, nullptr, nullptr,
                       out_pitch);
}

SM_API int sm_group_block_match_lr_u8(sm_group* g, const uint8_t* left, const uint8_t* right, int width, int height,
                                      int pitch, int radius, int num_disp, unsigned flags, uint8_t* disp_out,
                                      uint8_t* right_disp_out, uint8_t* valid_mask_out, int out_pitch) {
    return group_bands(g, left, right, width, height, pitch, radius, num_disp, flags | SM_LR_CHECK, disp_out,
                       right_disp_out, valid_mask_out, out_pitch);
}

SM_API int sm_group_dslice_block_match_u8(sm_group* g, const uint8_t* left, const uint8_t* right, int width,
                                          int height, int pitch, int radius, int num_disp, unsigned flags,
                                          uint8_t* disp_out, int out_pitch) {
    int rc = group_frame_check(g, left, right, disp_out, width, height, pitch, out_pitch, flags);
    if (rc) return rc;
    const DsliceCfg cfg{width, height, radius, num_disp, (flags & SM_AGG_GUIDED) != 0, (flags & SM_LR_CHECK) != 0};
    for (GroupWorker* w : g->w) {
        rc = pairs_refuse(w->h, flags, "the d-slice group call");
        if (rc) return rc;
    }
    rc = dslice_check(cfg, flags);
    if (rc) return rc;
    for (GroupWorker* w : g->w) {
        rc = speckle_refuse(w->h, "the d-slice group call", "the d-slice calls do not run it");
        if (rc) return rc;
        rc = fill_refuse(w->h, "the d-slice group call", "the d-slice calls do not run it");
        if (rc) return rc;
        rc = check_geometry(w->h, width, height, width, radius, num_disp);
        if (rc) return rc;
        rc = check_capacity(w->h, width, height, num_disp);
        if (rc) return rc;
    }
    rc = group_comms(g);
    if (rc) return rc;
    const int n = (int)g->w.size();
    // phase 1 on every member: workspace + the upload of its rows, stream synchronised (no collective yet)
    std::vector<std::function<int()>> jobs;
    for (int k = 0; k < n; ++k) {
        sm_handle* h = g->w[k]->h;
        jobs.push_back([=]() -> int { return dslice_member_upload(h, k, n, left, right, cfg, pitch); });
    }
    rc = group_run(g, jobs);
    if (rc) return rc;
    // phase 2: the collectives, entered by every member or aborted by all
    const RcclApi* api = rccl_api();
    DsliceSync sync;
    jobs.clear();
    for (int k = 0; k < n; ++k) {
        sm_handle* h = g->w[k]->h;
        ncclComm_t* c = &g->comms[k];
        DsliceSync* sy = &sync;
        jobs.push_back([=]() -> int { return dslice_member_collect(h, api, c, sy, k, n, cfg, disp_out, out_pitch); });
    }
    rc = group_run(g, jobs);
    if (sync.abort.load()) {   // some communicators were aborted: drop the rest, re-create on next use
        for (ncclComm_t& c : g->comms)
            if (c) (void)api->destroy(c);
        g->comms.clear();
    }
    return rc;
}

SM_API int sm_group_block_match_batch_u8(sm_group* g, const uint8_t* const* lefts, const uint8_t* const* rights,
                                         int nframes, int width, int height, int pitch, int radius, int num_disp,
                                         unsigned flags, uint8_t* const* disps, int out_pitch) {
    if (!g) return fail(SM_ERR_INVALID_ARG, "null group");
    if (nframes < 0 || (nframes > 0 && (!lefts || !rights || !disps)))
        return fail(SM_ERR_INVALID_ARG, "bad frame arrays");
    const int n = (int)g->w.size();
    std::vector<std::function<int()>> jobs;
    for (int k = 0; k < n && k < nframes; ++k) {
        sm_handle* h = g->w[k]->h;
        jobs.push_back([=]() -> int {
            for (int f = k; f < nframes; f += n) {   // frame f on member f mod n, in order
                const int rc = host_match_rows(h, lefts[f], rights[f], width, height, pitch, radius, num_disp, flags, 0,
                                               height, disps[f], nullptr, nullptr, out_pitch);
                if (rc) return rc;
            }
            return SM_OK;
        });
    }
    return group_run(g, jobs);
}

}  // extern "C"
