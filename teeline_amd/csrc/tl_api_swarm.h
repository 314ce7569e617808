// tl_api_swarm.h — the host path of a call over seeded runs of a population solver (internal to libteeline_gpu), written once:
// swarm_run.  tl_api_pso.hip, tl_api_cs.hip, tl_api_fpa.hip and tl_api_gsa.hip include it and hand it Swarm4<their solver>, which
// adds the trace they share (a 4-word improvement log, its routes, an epoch log); tl_api_aco.hip hands it a solver of its own.
//
// What swarm_run does: the checks of the common arguments, the permutation check of the start tours, the zeroed stats, the answer
// without a device for the smallest n, the workspace, the instance, the 8-word records and the start tours onto the device, the
// launch sequences of at most per_launch runs with their pointer offsets, the event pair, the download, the costs and moves, the
// best run and the stats.
//
// What a solver S supplies (Swarm4 supplies the starred ones):
//   Args                      its kernels' argument struct; swarm_run sets xy, dm_full, init, init_stride, seed, n and, per sequence,
//                             first_run, state, out_pos, out_cost by name
//   kHostN                  * the largest n answered on the host
//   epochs, pop()             after check(): for the stats (sweeps = epochs x runs, candidates = sweeps x pop())
//   check(k)                  its options and their checks, fail()'s code on a bad one
//   trace_reset()           * the trace's lengths to 0, before any check
//   host_answer(k)          * the answer for n <= kHostN: results, trace and its stats
//   plan(k, &per_launch)    * the runs of one launch sequence; fail()'s code where not even one fits
//   layout(k, held)         * the bytes of the workspace: the trace regions, then its tables for `held` runs
//   carve(k, A, w)          * the trace regions and its tables out of the workspace at w, and its own fields of A
//   trace_off(L)            * a sequence behind the first: no trace (the trace is run 0's)
//   enqueue(c, L, cnt)        the launches of one sequence of cnt runs
//   trace_download(k, A)    * what of the trace is copied back before the stream is synchronised
//   verdict(k, state)       * the check of the downloaded records (TL_OK, or fail()'s code)
//   trace_finish(k, A, state) * what of the trace depends on the records: copied after the synchronisation; further stats
#pragma once
#include "tl_api_chains.h"

namespace tlapi {

constexpr uint32_t kSwarmUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
constexpr uint64_t kSwarmWorkDefault = 8ull << 30;    // the tables of one launch sequence
constexpr uint32_t kSwarmMaxRuns = 65535u;            // the run is a grid dimension

// the arguments every entry of these solvers takes
struct SwarmCall {
    tl_ctx *c;
    const char *who;
    const float *xy;
    uint32_t n;
    const float *dm_packed;
    const uint32_t *init_pos;
    uint32_t init_count, first_run, count;
    uint64_t seed;
    uint32_t *out_pos;
    float *out_costs;
    tl_stats *stats;
    uint32_t *out_moves, *best_index;  // the population entries only
};

// the trace of run 0 of a call, as the *_trace entries of the four solvers with a 4-word log take it
struct SwarmTrace {
    uint32_t *log;
    uint32_t log_cap;
    uint32_t *log_len;
    uint32_t *route_log;
    uint32_t route_cap;
    uint32_t *epoch_log;
    uint32_t epoch_cap;
};

template <class S>
int swarm_run(const SwarmCall &k, S sv)
{
    using Args = typename S::Args;
    tl_ctx *c = k.c;
    const uint32_t n = k.n, count = k.count;
    sv.trace_reset();
    if (int rc = check_chain_call(c, k.who, k.xy, k.dm_packed, count, k.out_pos, k.init_pos, k.init_count, k.first_run, "run")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kSwarmUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", k.who, c->flags);
    if (int rc = sv.check(k)) return rc;
    for (uint32_t r = 0; r < k.init_count; ++r)
        if (!is_permutation(k.init_pos + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "%s: the initial tour is not a permutation of 0..n-1", k.who);
    const auto t0 = std::chrono::steady_clock::now();
    if (k.stats) memset(k.stats, 0, sizeof(*k.stats));
    if (k.best_index) *k.best_index = 0u;
    if (n <= S::kHostN) {  // no device
        sv.host_answer(k);
        c->ev_valid = false;
        if (k.stats) stamp_times(c, k.stats, t0);
        return TL_OK;
    }
    uint32_t per_launch = 0;
    if (int rc = sv.plan(k, &per_launch)) return rc;

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const uint32_t held = count < per_launch ? count : per_launch;  // runs whose tables exist at once
    if ((rc = ensure(c, c->init, (size_t)(k.init_count ? k.init_count : 1u) * n * 4)) || (rc = ensure(c, c->out_pos, (size_t)count * n * 4)) ||
        (rc = ensure(c, c->out_cost, (size_t)count * 4)) || (rc = ensure(c, c->misc, (size_t)count * 32)) || (rc = ensure(c, c->work, sv.layout(k, held))))
        return rc;
    Args A{};
    if ((rc = upload_instance_full(c, k.xy, k.dm_packed, n, &A.xy, &A.dm_full))) return rc;
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, (size_t)count * 32, c->stream));
    if (k.init_count) {
        HIPCHK(c, hipMemcpyAsync(c->init.p, k.init_pos, (size_t)k.init_count * n * 4, hipMemcpyHostToDevice, c->stream));
        A.init = (const uint32_t *)c->init.p;
        A.init_stride = k.init_count > 1u ? n : 0u;
    }
    A.seed = k.seed;
    A.n = n;
    sv.carve(k, A, (unsigned char *)c->work.p);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the tables
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        Args L = A;
        L.first_run = k.first_run + b0;
        if (L.init && L.init_stride) L.init += (size_t)b0 * n;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.state = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) sv.trace_off(L);  // the trace is run 0's
        HIPCHK(c, sv.enqueue(c, L, cnt));
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> state;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 8u, k.out_pos, state, costs))) return rc;
    if ((rc = sv.trace_download(k, A))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = sv.verdict(k, state))) return rc;
    uint64_t improved = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (k.out_costs) k.out_costs[r] = costs[r];
        if (k.out_moves) k.out_moves[r] = state[8u * r + 1u];
        improved += state[8u * r + 1u];
    }
    if ((rc = sv.trace_finish(k, A, state))) return rc;
    if (k.best_index) *k.best_index = best_chain(costs, count);
    if (k.stats) {
        k.stats->sweeps = (uint64_t)sv.epochs * count;
        k.stats->candidates = (uint64_t)sv.epochs * count * sv.pop();
        k.stats->moves = improved;
        stamp_times(c, k.stats, t0);
    }
    return TL_OK;
}

// The checks PSO, CS, FPA and GSA make of their sizes, in this order: the epochs, the population `pop` of `members` ("flowers")
// that n_nearest gives, n against the LDS limit (`lds_per_city`: the figure of the text)
inline int check_swarm_sizes(const SwarmCall &k, uint32_t epochs, uint32_t n_nearest, uint32_t pop, uint32_t max_pop, const char *members, uint32_t max_n,
                             const char *lds_per_city)
{
    if (epochs == 0xFFFFFFFFu) return fail(k.c, TL_ERR_UNSUPPORTED, "%s: epochs = 2^32 - 1 is not supported", k.who);
    if (pop > max_pop) return fail(k.c, TL_ERR_UNSUPPORTED, "%s: n_nearest=%u: more than %u %s", k.who, n_nearest, max_pop, members);
    if (k.n > max_n) return fail(k.c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (%s bytes of LDS per city)", k.who, k.n, max_n, lds_per_city);
    return TL_OK;
}

// the runs of one launch sequence of these four: what the workspace holds behind the layout's slack, the grid's limit at most
inline uint32_t swarm_per_launch(uint64_t workspace_bytes, uint64_t slack, uint64_t run_bytes)
{
    const uint64_t per = workspace_bytes > slack ? (workspace_bytes - slack) / run_bytes : 0u;
    return (uint32_t)(per > kSwarmMaxRuns ? kSwarmMaxRuns : per);
}

// tl_*_plan of these four: the population `pop` of n_nearest, the workgroup's threads and the runs of one launch sequence; all 0
// where the instance is not run on the device
inline int swarm_plan(uint32_t n, uint32_t pop, uint32_t max_pop, uint32_t (*max_n)(int), int (*threads)(uint32_t), uint64_t (*run_bytes)(uint32_t, uint32_t),
                      uint64_t slack, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags, uint32_t *out_pop, int *out_threads,
                      uint32_t *out_per_launch)
{
    if (out_pop) *out_pop = 0u;
    if (out_threads) *out_threads = 0;
    if (out_per_launch) *out_per_launch = 0u;
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (flags & kSwarmUnassignedFlags) return TL_ERR_UNSUPPORTED;
    if (n < 2u || n > max_n(lds_bytes) || pop > max_pop) return TL_OK;
    const uint32_t per = swarm_per_launch(workspace_bytes, slack, run_bytes(n, pop));
    if (per == 0u) return TL_OK;
    if (out_pop) *out_pop = pop;
    if (out_threads) *out_threads = threads(n);
    if (out_per_launch) *out_per_launch = per;
    return TL_OK;
}

// The rest of S for a solver P with the 4-word improvement log.  P supplies, besides Args, epochs, check and enqueue:
//   N                       its population, after check()
//   kMembers, kLayoutSlack  "flowers"; the bytes the 256-byte alignment of its arrays can cost
//   row_words()             the words of an epoch-log row
//   log_rows()              the bound on the log's rows: the start and every improvement there can be
//   run_bytes(n)            one run's share of the workspace
//   layout(n, held)         the bytes of its tables for `held` runs (it keeps the sizes for carve)
//   carve(A, w, n)          its tables at w, its own fields of A
//   host_epoch_rows(k, epoch_log, rows)   the rows of the zeroed epoch log that are not 0 where n <= 1
//   verdict(k, state)       see above
template <class P>
struct Swarm4 {
    using Args = typename P::Args;
    static constexpr uint32_t kHostN = 1u;
    P p;
    SwarmTrace t;
    uint32_t epochs = 0;
    uint32_t log_cap = 0, route_cap = 0, epoch_cap = 0;  // the device's share of the trace
    size_t log_bytes = 0, route_bytes = 0, epoch_bytes = 0;

    Swarm4(const P &solver, const SwarmTrace &trace) : p(solver), t(trace) {}
    uint32_t pop() const { return p.N; }
    void trace_reset() const
    {
        if (t.log_len) *t.log_len = 0;
    }
    int check(const SwarmCall &k)
    {
        const int rc = p.check(k);
        epochs = p.epochs;
        return rc;
    }
    // n <= 1: no edge, no device: every individual is the one route (or the empty one) at cost 0 and nothing improves
    void host_answer(const SwarmCall &k)
    {
        for (uint32_t r = 0; r < k.count; ++r) {
            if (k.n) k.out_pos[r] = 0u;
            if (k.out_costs) k.out_costs[r] = 0.0f;
            if (k.out_moves) k.out_moves[r] = 0u;
        }
        if (t.log && t.log_cap) {  // record 0: the start best, individual 0 (all are equal)
            t.log[0] = 0xFFFFFFFFu;
            t.log[1] = t.log[2] = 0u;
            t.log[3] = t.route_log && t.route_cap ? 0u : 0xFFFFFFFFu;
        }
        if (t.route_log && t.route_cap && k.n) t.route_log[0] = 0u;
        if (t.epoch_log) {
            const uint32_t rows = t.epoch_cap < epochs ? t.epoch_cap : epochs;
            memset(t.epoch_log, 0, (size_t)rows * p.row_words() * 4);
            p.host_epoch_rows(k, t.epoch_log, rows);
        }
        if (t.log_len) *t.log_len = 1u;
        if (k.stats) {
            k.stats->sweeps = (uint64_t)epochs * k.count;
            k.stats->candidates = (uint64_t)epochs * k.count * p.N;
        }
    }
    int plan(const SwarmCall &k, uint32_t *per_launch) const
    {
        *per_launch = swarm_per_launch(kSwarmWorkDefault, P::kLayoutSlack, p.run_bytes(k.n));
        if (*per_launch == 0u)
            return fail(k.c, TL_ERR_UNSUPPORTED, "%s: n=%u, %u %s: one run's tables (%llu bytes) exceed the workspace limit", k.who, k.n, p.N, P::kMembers,
                        (unsigned long long)p.run_bytes(k.n));
        return TL_OK;
    }
    size_t layout(const SwarmCall &k, uint32_t held)
    {
        const uint64_t most = p.log_rows();
        log_cap = t.log ? (uint32_t)(t.log_cap < most ? t.log_cap : most) : 0u;
        route_cap = t.route_log ? (uint32_t)(t.route_cap < most ? t.route_cap : most) : 0u;
        epoch_cap = t.epoch_log ? (t.epoch_cap < epochs ? t.epoch_cap : epochs) : 0u;
        log_bytes = up256((size_t)(log_cap ? log_cap : 1u) * 16);
        route_bytes = up256((size_t)(route_cap ? route_cap : 1u) * k.n * 4);
        epoch_bytes = up256((size_t)(epoch_cap ? epoch_cap : 1u) * p.row_words() * 4);
        return log_bytes + route_bytes + epoch_bytes + p.layout(k.n, held);
    }
    void carve(const SwarmCall &k, Args &A, unsigned char *w)
    {
        A.log = t.log ? (uint32_t *)w : nullptr;
        A.log_cap = log_cap;
        A.route_log = t.route_log ? (uint32_t *)(w + log_bytes) : nullptr;
        A.route_cap = route_cap;
        A.epoch_log = t.epoch_log ? (uint32_t *)(w + log_bytes + route_bytes) : nullptr;
        A.epoch_cap = epoch_cap;
        p.carve(A, w + log_bytes + route_bytes + epoch_bytes, k.n);
    }
    void trace_off(Args &L) const { L.log = L.route_log = L.epoch_log = nullptr; }
    hipError_t enqueue(tl_ctx *c, Args &L, uint32_t cnt) { return p.enqueue(c, L, cnt); }
    int trace_download(const SwarmCall &k, const Args &A) const
    {
        if (epoch_cap) HIPCHK(k.c, hipMemcpyAsync(t.epoch_log, A.epoch_log, (size_t)epoch_cap * p.row_words() * 4, hipMemcpyDeviceToHost, k.c->stream));
        return TL_OK;
    }
    int verdict(const SwarmCall &k, const std::vector<uint32_t> &state) const { return p.verdict(k, state); }
    int trace_finish(const SwarmCall &k, const Args &A, const std::vector<uint32_t> &state) const
    {
        const uint64_t rows = 1ull + state[1];
        int rc;
        if (log_cap && (rc = download_sync(k.c, t.log, A.log, (size_t)(rows < log_cap ? rows : log_cap) * 16))) return rc;
        if (route_cap && (rc = download_sync(k.c, t.route_log, A.route_log, (size_t)(rows < route_cap ? rows : route_cap) * k.n * 4))) return rc;
        if (t.log_len) *t.log_len = (uint32_t)(rows < 0xFFFFFFFFull ? rows : 0xFFFFFFFFull);
        return TL_OK;
    }
};

template <class P>
int swarm4_run(const SwarmCall &k, const P &solver, const SwarmTrace &trace)
{
    return swarm_run(k, Swarm4<P>(solver, trace));
}

}  // namespace tlapi
