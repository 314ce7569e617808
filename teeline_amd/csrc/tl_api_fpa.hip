// tl_api_fpa.hip — C ABI, the flower pollination solver: tl_flower_pollination* (src/tsp/flower_pollination.rs:53-151) over
// flower_pollination.hip, the host-only queries of its specification (tl_fpa_draw, tl_fpa_switch_prob, tl_fpa_global_swaps,
// tl_fpa_local_swaps, tl_fpa_partners, tl_flower_pollination_plan) and the device self-test of one move.
//
// n = 0 and n = 1: the reference does not panic (swap_sequence's saturating_sub gives an empty sequence, every flower comes back
// unchanged at cost 0 and 0 < 0 fails), so the entries return the empty route or the one city at cost 0, a log of the start gbest
// alone and epoch rows that hold each flower's draws with nothing accepted — on the host, without a launch.
#include "fpa_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kFpaUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kFpaWorkDefault = 8ull << 30;    // the runs of one launch sequence
static constexpr uint32_t kFpaMaxRuns = 65535u;            // the run is the grid's y
static constexpr uint64_t kFpaLayoutSlack = 9 * 256;       // the arrays of a sequence each start on a 256-byte boundary

// one run's share of the workspace: flowers and staged moves (N n u16 each), gbest, three rows of N words
static inline uint64_t fpa_run_bytes(uint32_t n, uint32_t N) { return 4ull * N * n + 2ull * n + 12ull * N; }

extern "C" uint64_t tl_fpa_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" double tl_fpa_switch_prob(float mutation_probability) { return fpa_switch_prob(mutation_probability); }

extern "C" uint32_t tl_fpa_global_swaps(double levy, uint32_t len) { return fpa_global_swaps(levy, len); }

extern "C" uint32_t tl_fpa_local_swaps(double epsilon, uint32_t len) { return fpa_local_swaps(epsilon, len); }

extern "C" int tl_fpa_partners(uint64_t seed, uint32_t run, uint32_t epoch, uint32_t i, uint32_t flowers, uint32_t *j, uint32_t *k)
{
    if (!j || !k || flowers < 3u || flowers > kFpaMaxFlowers || i >= flowers) return TL_ERR_BADARG;
    fpa_partners(sa_chain_key(seed, run), fpa_event(epoch, flowers, i), i, flowers, j, k);
    return TL_OK;
}

extern "C" uint32_t tl_flower_pollination_max_n(const tl_ctx *c) { return c ? flower_pollination_max_n(c->lds_bytes) : 0u; }

extern "C" int tl_flower_pollination_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                          uint32_t *flowers, int *threads, uint32_t *per_launch)
{
    if (flowers) *flowers = 0u;
    if (threads) *threads = 0;
    if (per_launch) *per_launch = 0u;
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (flags & kFpaUnassignedFlags) return TL_ERR_UNSUPPORTED;
    const uint32_t N = fpa_flowers(n_nearest);
    if (n < 2u || n > flower_pollination_max_n(lds_bytes) || N > kFpaMaxFlowers) return TL_OK;
    uint64_t per = workspace_bytes > kFpaLayoutSlack ? (workspace_bytes - kFpaLayoutSlack) / fpa_run_bytes(n, N) : 0u;
    if (per > kFpaMaxRuns) per = kFpaMaxRuns;
    (void)count;
    if (per == 0u) return TL_OK;
    if (flowers) *flowers = N;
    if (threads) *threads = flower_pollination_threads(n);
    if (per_launch) *per_launch = (uint32_t)per;
    return TL_OK;
}

// What the entries share.  log / route_log / epoch_log: run 0 of the call (a single run's trace), else nullptr
static int fpa_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                   uint32_t first_run, uint32_t count, const tl_fpa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                   uint32_t *best_index, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap,
                   uint32_t *epoch_log, uint32_t epoch_cap)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_run, "run")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kFpaUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    // FPAOptions::default (mod.rs:1003-1010) over HeuristicOptions::default (mod.rs:604-611)
    const uint32_t epochs = opts ? opts->epochs : 10000u, n_nearest = opts ? opts->n_nearest : 3u;
    const float p_mut = opts ? opts->mutation_probability : 0.001f;
    const uint32_t N = fpa_flowers(n_nearest);
    if (!(p_mut >= 0.0f && p_mut <= 1.0f)) return fail(c, TL_ERR_BADARG, "%s: mutation_probability must be in [0, 1] (got %g)", who, (double)p_mut);
    if (epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 2^32 - 1 is not supported", who);
    if (N > kFpaMaxFlowers) return fail(c, TL_ERR_UNSUPPORTED, "%s: n_nearest=%u: more than %u flowers", who, n_nearest, kFpaMaxFlowers);
    if (n > flower_pollination_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (10 bytes of LDS per city)", who, n, flower_pollination_max_n(c->lds_bytes));
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "%s: the initial tour is not a permutation of 0..n-1", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    const double switch_prob = fpa_switch_prob(p_mut);
    if (n <= 1u) {  // no edge, no device: every sequence is empty, every flower comes back unchanged at cost 0, nothing is accepted
        for (uint32_t r = 0; r < count; ++r) {
            if (n) out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
            if (out_moves) out_moves[r] = 0u;
        }
        if (log && log_cap) {  // record 0: the start gbest, flower 0 (all are equal)
            log[0] = 0xFFFFFFFFu;
            log[1] = log[2] = 0u;
            log[3] = route_log && route_cap ? 0u : 0xFFFFFFFFu;
        }
        if (route_log && route_cap && n) route_log[0] = 0u;
        if (epoch_log) {
            const uint64_t key = sa_chain_key(seed, first_run);
            const uint32_t rows = epoch_cap < epochs ? epoch_cap : epochs;
            memset(epoch_log, 0, (size_t)rows * 4 * N * 4);
            for (uint32_t e = 0; e < rows; ++e)
                for (uint32_t i = 0; i < N; ++i) {
                    uint32_t j, k;
                    fpa_partners(key, fpa_event(e, N, i), i, N, &j, &k);
                    epoch_log[(size_t)e * 4 * N + N + i] = fpa_kind_word(fpa_is_global(key, fpa_event(e, N, i), switch_prob), j, k);
                }
        }
        if (log_len) *log_len = 1u;
        c->ev_valid = false;
        if (stats) {
            stats->sweeps = (uint64_t)epochs * count;
            stats->candidates = (uint64_t)epochs * count * N;
            stamp_times(c, stats, t0);
        }
        return TL_OK;
    }
    uint32_t per_launch = 0;
    tl_flower_pollination_plan(n, n_nearest, count, c->cus, c->lds_bytes, kFpaWorkDefault, 0u, nullptr, nullptr, &per_launch);
    if (per_launch == 0u)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u, %u flowers: one run's tables (%llu bytes) exceed the workspace limit", who, n, N,
                    (unsigned long long)fpa_run_bytes(n, N));

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n;
    const uint32_t held = count < per_launch ? count : per_launch;  // runs whose flowers exist at once
    const uint64_t most = 1ull + (uint64_t)epochs * N;               // the start gbest and at most one improvement per move
    const uint32_t dev_log_cap = log ? (uint32_t)(log_cap < most ? log_cap : most) : 0u;
    const uint32_t dev_route_cap = route_log ? (uint32_t)(route_cap < most ? route_cap : most) : 0u;
    const uint32_t dev_epoch_cap = epoch_log ? (epoch_cap < epochs ? epoch_cap : epochs) : 0u;
    const size_t log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16);
    const size_t route_bytes = up256((size_t)(dev_route_cap ? dev_route_cap : 1u) * n * 4);
    const size_t epoch_bytes = up256((size_t)(dev_epoch_cap ? dev_epoch_cap : 1u) * 4 * N * 4);
    const size_t tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), row = up256((size_t)held * N * 4);
    if ((rc = ensure(c, c->init, (size_t)(init_count ? init_count : 1u) * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) ||
        (rc = ensure(c, c->out_cost, (size_t)count * 4)) || (rc = ensure(c, c->misc, (size_t)count * 32)) ||
        (rc = ensure(c, c->work, log_bytes + route_bytes + epoch_bytes + 2 * tab + gb + 3 * row)))
        return rc;
    FpaArgs A{};
    if ((rc = upload_instance_full(c, xy, dm_packed, n, &A.xy, &A.dm_full))) return rc;
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, (size_t)count * 32, c->stream));
    if (init_count) {
        HIPCHK(c, hipMemcpyAsync(c->init.p, init_pos, (size_t)init_count * n * 4, hipMemcpyHostToDevice, c->stream));
        A.init = (const uint32_t *)c->init.p;
        A.init_stride = init_count > 1u ? n : 0u;
    }
    unsigned char *w = (unsigned char *)c->work.p;
    A.log = log ? (uint32_t *)w : nullptr;
    A.log_cap = dev_log_cap;
    A.route_log = route_log ? (uint32_t *)(w + log_bytes) : nullptr;
    A.route_cap = dev_route_cap;
    A.epoch_log = epoch_log ? (uint32_t *)(w + log_bytes + route_bytes) : nullptr;
    A.epoch_cap = dev_epoch_cap;
    w += log_bytes + route_bytes + epoch_bytes;
    A.flower = (uint16_t *)w;
    A.stage = (uint16_t *)(w + tab);
    A.gbest = (uint16_t *)(w + 2 * tab);
    w += 2 * tab + gb;
    A.cost = (float *)w;
    A.scost = (float *)(w + row);
    A.slen = (uint32_t *)(w + 2 * row);
    A.seed = seed;
    A.switch_prob = switch_prob;
    A.n = n;
    A.flowers = N;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the tables
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        FpaArgs L = A;
        L.first_run = first_run + b0;
        if (L.init && L.init_stride) L.init += (size_t)b0 * n;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.state = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) L.log = L.route_log = L.epoch_log = nullptr;  // the trace is run 0's
        L.last = epochs == 0u;
        HIPCHK(c, launch_fpa_init(L, cnt, c->stream));
        for (uint32_t e = 0; e < epochs; ++e) {
            L.epoch = e;
            L.last = e + 1u == epochs;
            HIPCHK(c, launch_fpa_move(L, cnt, c->stream));
            HIPCHK(c, launch_fpa_commit(L, cnt, c->stream));
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> state;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 8u, out_pos, state, costs))) return rc;
    if (dev_epoch_cap) HIPCHK(c, hipMemcpyAsync(epoch_log, A.epoch_log, (size_t)dev_epoch_cap * 4 * N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t improved = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (out_costs) out_costs[r] = costs[r];
        if (out_moves) out_moves[r] = state[8u * r + 1u];
        improved += state[8u * r + 1u];
    }
    const uint64_t rows = 1ull + state[1];
    if (dev_log_cap) HIPCHK(c, hipMemcpy(log, A.log, (size_t)(rows < dev_log_cap ? rows : dev_log_cap) * 16, hipMemcpyDeviceToHost));
    if (dev_route_cap) HIPCHK(c, hipMemcpy(route_log, A.route_log, (size_t)(rows < dev_route_cap ? rows : dev_route_cap) * n * 4, hipMemcpyDeviceToHost));
    if (log_len) *log_len = (uint32_t)(rows < 0xFFFFFFFFull ? rows : 0xFFFFFFFFull);
    if (best_index) *best_index = best_chain(costs, count);
    if (stats) {
        stats->sweeps = (uint64_t)epochs * count;
        stats->candidates = (uint64_t)epochs * count * N;
        stats->moves = improved;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_flower_pollination(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_fpa_opts *opts,
                                     uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return fpa_run(c, "tl_flower_pollination", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats, nullptr,
                   0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_flower_pollination_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_fpa_opts *opts,
                                           uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                           uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_flower_pollination_trace: NULL argument");
    return fpa_run(c, "tl_flower_pollination_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats,
                   log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap);
}

extern "C" int tl_flower_pollination_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                                uint32_t first_run, uint32_t count, const tl_fpa_opts *opts, uint64_t seed, uint32_t *out_pos,
                                                float *out_costs, uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return fpa_run(c, "tl_flower_pollination_population", xy, n, dm_packed, init_pos, init_count, first_run, count, opts, seed, out_pos, out_costs, out_moves,
                   best_index, stats, nullptr, 0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_fpa_selftest_pollinate(tl_ctx *c, const uint32_t *flower, const uint32_t *source, const uint32_t *target, const uint32_t *prefix, uint32_t n,
                                         uint32_t count, uint32_t *out, uint32_t *out_len)
{
    TL_ENTER(c);
    if (!c || !flower || !source || !target || !prefix || !out || !out_len) return fail(c, TL_ERR_BADARG, "tl_fpa_selftest_pollinate: NULL argument");
    if (n < 1u || n > flower_pollination_max_n(c->lds_bytes) || count < 1u || count > kFpaMaxRuns)
        return fail(c, TL_ERR_BADARG, "tl_fpa_selftest_pollinate: n or count out of range");
    const size_t cells = (size_t)count * n;
    std::vector<uint16_t> h(3 * cells);
    const uint32_t *in[3] = {flower, source, target};
    for (int a = 0; a < 3; ++a)
        for (uint32_t r = 0; r < count; ++r) {
            if (!is_permutation(in[a] + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "tl_fpa_selftest_pollinate: row %u is not a permutation of 0..n-1", r);
            for (uint32_t k = 0; k < n; ++k) h[a * cells + (size_t)r * n + k] = (uint16_t)in[a][(size_t)r * n + k];
        }
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t tb = up256(cells * 2), lb = up256((size_t)count * 4);
    if ((rc = ensure(c, c->work, 4 * tb + 2 * lb))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    for (int a = 0; a < 3; ++a) HIPCHK(c, hipMemcpyAsync(w + a * tb, h.data() + a * cells, cells * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + 4 * tb, prefix, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + 3 * tb, 0xFF, cells * 2, c->stream));
    HIPCHK(c, launch_fpa_selftest_pollinate((const uint16_t *)w, (const uint16_t *)(w + tb), (const uint16_t *)(w + 2 * tb), (const uint32_t *)(w + 4 * tb), n, count,
                                            (uint16_t *)(w + 3 * tb), (uint32_t *)(w + 4 * tb + lb), c->stream));
    HIPCHK(c, hipMemcpyAsync(h.data(), w + 3 * tb, cells * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_len, w + 4 * tb + lb, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < cells; ++k) out[k] = h[k];
    return TL_OK;
}
