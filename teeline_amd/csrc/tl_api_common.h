// tl_api_common.h — what the host-side translation units of the C ABI share (internal to libteeline_gpu): the context, its
// single-thread guard, error reporting and the grow-only device buffers.  tl_api.hip (context, matrix, tour length),
// tl_api_two_opt.hip, tl_api_scans.hip (3-opt, Or-opt), tl_api_lk.hip (candidate lists, NN seed, Lin-Kernighan), tl_api_greedy.hip
// (greedy-edge, savings, Christofides) and tl_api_bhk.hip (Bellman-Held-Karp) include it; tl_api_sa.hip, tl_api_tabu.hip and
// tl_api_ga.hip (the seeded chains) through tl_api_chains.h, which adds what those three share; tl_api_aco.hip, tl_api_pso.hip,
// tl_api_cs.hip, tl_api_fpa.hip and tl_api_gsa.hip (the population solvers) through tl_api_swarm.h, which is over tl_api_chains.h
// and holds their whole host path.
#pragma once
#include "../../include/teeline_gpu.h"
#include "tl_kernels.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#ifndef TL_MAX_SWEEPS
#define TL_MAX_SWEEPS (1u << 20)  // status 1 beyond (never reached by a descent: every move shortens the tour); tuning variants
                                  // are built with a small cap so that a wrong experimental kernel ends instead of hanging the GPU
#endif

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct tl_ctx {
    int device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    // The context's device workspace shared by asynchronous calls (neighbour lists `nl`, grid coordinates `fx`) belongs to the LAST
    // kernel sequence enqueued with it.  tl_two_opt_batch_dev returns before that sequence has run and takes the caller's stream, so a
    // later call on ANOTHER stream (or on the context's own) must be ordered behind it before it rebuilds that workspace:
    // ev_ws is recorded behind every such sequence on ws_stream; ws_order() makes a different stream wait on it.
    hipEvent_t ev_ws = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_pending = false;
    bool in_callback = false;  // a tl_lk_live callback of this context is running: any entry into this context from inside it is refused
    // out_stats holds the counters of a finished host-buffer 2-opt call (tl_two_opt_last_counters).  The buffer is also the f32 snapshot
    // ring of tl_lk_trace / tl_lk_live and is written behind the caller's back by tl_two_opt_batch_dev: every such user clears this.
    bool stats_valid = false;
    int cus = 0, lds_bytes = 0;
    std::string arch;
    std::string err;
    DevBuf xy, dm, init, out_pos, out_cost, out_stats, misc, work, dmfull, kd, fx, nl, dmx;  // dmx: matrix-form 2-opt, the descents' per-city records of their late sweeps
    bool two_opt_best_force_scan = false;  // tl_two_opt_best_force_scan: best-sweep batches loop over the chip-wide descent at every n
    int lk_pop_force_form = -1;          // tl_lk_population_setting: -1 the plan's choice, 0 the loop over tl_lk, 1 one workgroup per run
    uint32_t lk_pop_slice_scans = 0;     // ... and the scans per launch of that form (0: kLkIlsSlice)
    // tl_lk_candidates: lk_cand_n x lk_cand_k positions every LK entry searches instead of the kd-tree's lists (empty: none set), and
    // the copy the call in progress has put into ascending distance
    std::vector<uint32_t> lk_cand, lk_cand_sorted;
    uint32_t lk_cand_n = 0, lk_cand_k = 0;
    uint64_t three_opt_pop_work = 0;  // tl_three_opt_population: cap on the per-tour matrices' workspace (0: the default)
    uint32_t dm_n = 0;
    int dm_layout = -1;
    // which host thread is inside an entry point with this context (default id: none) and how deep (entries call entries)
    std::atomic<std::thread::id> owner{};
    int depth = 0;
};

// A tl_ctx is single-threaded (include/teeline_gpu.h): its stream, event pair, workspace and error string belong to the call in
// progress.  Every entry point that takes a context enters through this guard; a second host thread that arrives while another is
// inside gets TL_ERR_BUSY back at once — nothing of the context is touched, not even its error string — instead of racing on
// the workspace.  Re-entry by the owning thread (tl_lk -> tl_nearest_neighbor -> tl_tour_length ...) is counted.
struct CtxUse {
    tl_ctx *c;
    bool ok = true;
    explicit CtxUse(tl_ctx *c_) : c(c_)
    {
        if (!c) return;
        const std::thread::id me = std::this_thread::get_id();
        if (c->owner.load(std::memory_order_acquire) == me) {
            if (c->in_callback) {  // re-entry from inside a live-progress callback: the running search owns stream and workspace
                ok = false;
                return;
            }
            ++c->depth;
            return;
        }
        std::thread::id none{};
        if (c->owner.compare_exchange_strong(none, me, std::memory_order_acq_rel)) {
            c->depth = 1;
            return;
        }
        ok = false;
    }
    ~CtxUse()
    {
        if (c && ok && --c->depth == 0) c->owner.store(std::thread::id(), std::memory_order_release);
    }
    CtxUse(const CtxUse &) = delete;
    CtxUse &operator=(const CtxUse &) = delete;
};
// Around a tl_lk_live callback: while it runs, CtxUse refuses every entry into this context from the owning thread.
struct InCallback {
    tl_ctx *c;
    explicit InCallback(tl_ctx *c_) : c(c_) { c->in_callback = true; }
    ~InCallback() { c->in_callback = false; }
    InCallback(const InCallback &) = delete;
    InCallback &operator=(const InCallback &) = delete;
};
#define TL_ENTER(c)      \
    CtxUse tl_use_((c)); \
    if (!tl_use_.ok) return TL_ERR_BUSY


#define HIPCHK(c, expr)                                                                           \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            (void)hipGetLastError(); /* the thread's sticky error: a later launch check must not report this one again */ \
            return fail((c), _e == hipErrorOutOfMemory ? TL_ERR_NOMEM : TL_ERR_HIP, "%s: %s", #expr, \
                        hipGetErrorString(_e));                                                   \
        }                                                                                         \
    } while (0)

namespace tlapi {
int fail(tl_ctx *c, int code, const char *fmt, ...);            // sets the context's (or the thread's create-) error string, returns code
int ensure(tl_ctx *c, DevBuf &b, size_t bytes);                // grow-only device buffer
bool is_permutation(const uint32_t *p, uint32_t n);            // validate_tour, src/tsp/mod.rs:1620-1634
uint32_t lds_max_n(int lds_bytes);                             // largest n of the LDS-resident 2-opt descent
int ws_order(tl_ctx *c, hipStream_t s);                        // before touching nl / fx on stream s: wait for their last user on another stream
int ws_mark(tl_ctx *c, hipStream_t s);                         // behind a kernel sequence that reads nl / fx on stream s
// A tune-only create flag: always clear in the product build (tl_create refuses them), so the branches it selects fold away.
#ifdef TL_TUNE
inline uint32_t tune_flags(const tl_ctx *c) { return c->flags; }
#else
inline uint32_t tune_flags(const tl_ctx *) { return 0u; }
#endif
inline int knn_form(const tl_ctx *c) { return (tune_flags(c) & TL_FLAG_KNN_1LANE) ? 1 : (tune_flags(c) & TL_FLAG_KNN_4LANES) ? 4 : 0; }
// tl_api_lk.hip: device-side candidate lists and NN seed, also used by tl_lk
int build_candidates_dev(tl_ctx *c, const float *xy_host, const float2 *d_xy, uint32_t n, uint32_t k, uint32_t *d_cand);
int nn_seed_dev(tl_ctx *c, const float2 *d_xy, uint32_t n, uint32_t n_nearest, uint32_t *d_path);

inline size_t packed_dm_bytes(uint32_t n) { return (size_t)n * (n - 1) / 2 * 4; }  // the reference's packed lower triangle, f32
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }                  // where a region of a workspace may begin

// The instance onto the device, on the context's stream: the coordinates into c->xy, the packed matrix into c->dm.  The caller's
// arrays are the entry point's arguments, which outlive the call's last synchronise.
inline int upload_xy(tl_ctx *c, const float *xy, uint32_t n, const float2 **dxy)
{
    int rc;
    if ((rc = ensure(c, c->xy, (size_t)n * 8))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->xy.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    *dxy = (const float2 *)c->xy.p;
    return TL_OK;
}
inline int upload_dm(tl_ctx *c, const float *dm_packed, uint32_t n, const float **ddm)
{
    int rc;
    if ((rc = ensure(c, c->dm, packed_dm_bytes(n)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dm.p, dm_packed, packed_dm_bytes(n), hipMemcpyHostToDevice, c->stream));
    *ddm = (const float *)c->dm.p;
    return TL_OK;
}
// The packed matrix (then every distance is read from it) or the coordinates: exactly one of the two, the other pointer stays as it
// is.  (tl_two_opt and its trace upload both where both are given: the matrix drives the descent, c->xy the neighbour lists' cache.)
inline int upload_input(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, const float2 **dxy, const float **ddm)
{
    return dm_packed ? upload_dm(c, dm_packed, n, ddm) : upload_xy(c, xy, n, dxy);
}

// The start permutation (init == NULL: the identity), or `tours` of them one after the other, to d_perm, and a synchronise: the
// identity lives in here, and every host vector whose copy the caller enqueued before this call may go out of scope behind it.
// The last upload of a setup.
inline int upload_start_sync(tl_ctx *c, const uint32_t *init, uint32_t n, void *d_perm, size_t tours = 1)
{
    std::vector<uint32_t> ident;
    if (!init) {
        ident.resize(tours * n);
        for (size_t i = 0; i < ident.size(); ++i) ident[i] = (uint32_t)(i % n);
        init = ident.data();
    }
    HIPCHK(c, hipMemcpyAsync(d_perm, init, tours * n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}

// A device-to-host copy whose length the call learns only from records it has already downloaded, so the host reads it at once: on
// the context's own stream, then a synchronise.  Never a plain hipMemcpy: that one goes through the legacy default stream, and while
// ANOTHER host thread captures a graph on its context's stream (RoundGraph) the runtime refuses it here and invalidates the capture there.
inline int download_sync(tl_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}

// The ending of a call that fills tl_stats: kernel_ms between the context's event pair (0 where none is valid), total_ms since t0.
inline void stamp_times(tl_ctx *c, tl_stats *st, std::chrono::steady_clock::time_point t0)
{
    if (!st) return;
    double kms = 0;
    tl_last_kernel_ms(c, &kms);
    st->kernel_ms = kms;
    st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// `rounds` rounds of a search per host poll of its done flag (the kernels are no-ops once it is set).  The first batch is enqueued
// launch by launch; a search still running after it replays the same rounds as ONE hipGraph launch per poll — a round is a few
// short dependent kernels, and the host's per-launch cost and the gaps between separately enqueued kernels are a visible part of
// it.  Where capture or instantiation fails (or allowed == false) every batch is enqueued launch by launch.
class RoundGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool first = true, ok;

public:
    explicit RoundGraph(bool allowed = true) : ok(allowed) {}
    ~RoundGraph()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
    RoundGraph(const RoundGraph &) = delete;
    RoundGraph &operator=(const RoundGraph &) = delete;
    // enqueue_round(r) -> hipError_t enqueues round r on `stream`
    template <class F>
    hipError_t launch(hipStream_t stream, int rounds, F &&enqueue_round)
    {
        if (!first && ok && !exec) {
            ok = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                hipError_t le = hipSuccess;
                for (int r = 0; r < rounds && le == hipSuccess; ++r) le = enqueue_round((uint32_t)r);
                const hipError_t ce = hipStreamEndCapture(stream, &graph);
                ok = le == hipSuccess && ce == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
            }
            if (!ok) {
                // separately enqueued launches from here on — after making sure the stream has left capture mode (a capture
                // that another thread's legacy-stream operation invalidated stays "active, invalidated" until it is ended)
                (void)hipGetLastError();
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
                    hipGraph_t g2 = nullptr;
                    (void)hipStreamEndCapture(stream, &g2);
                    if (g2) (void)hipGraphDestroy(g2);
                }
                (void)hipGetLastError();
                if (graph) {
                    (void)hipGraphDestroy(graph);
                    graph = nullptr;
                }
            }
        }
        first = false;
        if (exec) return hipGraphLaunch(exec, stream);
        hipError_t e = hipSuccess;
        for (int r = 0; r < rounds && e == hipSuccess; ++r) e = enqueue_round((uint32_t)r);
        return e;
    }
};
}  // namespace tlapi
