// tl_api_gsa.hip — C ABI, the gravitational search solver: tl_gravitational_search* (src/tsp/gravitational_search.rs:23-145) over
// gravitational_search.hip, the host-only queries of its specification (tl_gsa_draw, tl_gsa_g, tl_gsa_pull_swaps, tl_gsa_masses,
// tl_gravitational_search_plan) and the device self-test of one pull.
//
// n = 0 and n = 1: the reference does not panic (every cost is 0, the masses are uniform, every swap sequence is empty and 0 < 0
// fails), so the entries return the empty route or the one city at cost 0, a log of the start gbest alone and epoch rows that hold
// each agent's live pulls with nothing applied — on the host, without a launch.
#include "gsa_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kGsaUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kGsaWorkDefault = 8ull << 30;    // the runs of one launch sequence
static constexpr uint32_t kGsaMaxRuns = 65535u;            // the run is the grid's x of the epochs, the grid's y of the start
static constexpr uint64_t kGsaLayoutSlack = 8 * 256;       // the arrays of a sequence each start on a 256-byte boundary
static constexpr uint32_t kGsaSpanEpochs = 4096u;          // epochs of one launch where the options name no span, so that no launch runs without end

// one run's share of the workspace: the positions (N n u16), gbest, the costs, the masses, the ranking
static inline uint64_t gsa_run_bytes(uint32_t n, uint32_t N) { return 2ull * N * n + 2ull * n + 14ull * N; }

extern "C" uint64_t tl_gsa_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" double tl_gsa_g(uint32_t epoch, uint32_t epochs) { return gsa_g(epoch, epochs); }

extern "C" uint32_t tl_gsa_pull_swaps(double r, double g, double mass) { return gsa_pull_swaps(r, g, mass); }

extern "C" int tl_gsa_masses(const float *costs, uint32_t agents, double *out_masses, uint32_t *out_rank)
{
    if (!costs || !out_masses || !out_rank || agents < 1u || agents > kGsaMaxAgents) return TL_ERR_BADARG;
    const float worst = gsa_worst(costs, agents);
    const double sum = gsa_sum_fitness(costs, agents, worst);
    bool nan = false;
    for (uint32_t a = 0; a < agents; ++a) {
        out_masses[a] = gsa_mass(costs[a], worst, sum, agents);
        nan = nan || out_masses[a] != out_masses[a];
    }
    if (nan) return TL_ERR_REF_PANICS;  // partial_cmp(..).unwrap() of the ranking
    for (uint32_t a = 0; a < agents; ++a) out_rank[gsa_rank(out_masses, agents, a)] = a;
    return TL_OK;
}

extern "C" uint32_t tl_gravitational_search_max_n(const tl_ctx *c) { return c ? gravitational_search_max_n(c->lds_bytes) : 0u; }

extern "C" int tl_gravitational_search_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                            uint32_t *agents, int *threads, uint32_t *per_launch)
{
    if (agents) *agents = 0u;
    if (threads) *threads = 0;
    if (per_launch) *per_launch = 0u;
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (flags & kGsaUnassignedFlags) return TL_ERR_UNSUPPORTED;
    const uint32_t N = gsa_agents(n_nearest);
    if (n < 2u || n > gravitational_search_max_n(lds_bytes) || N > kGsaMaxAgents) return TL_OK;
    uint64_t per = workspace_bytes > kGsaLayoutSlack ? (workspace_bytes - kGsaLayoutSlack) / gsa_run_bytes(n, N) : 0u;
    if (per > kGsaMaxRuns) per = kGsaMaxRuns;
    (void)count;
    if (per == 0u) return TL_OK;
    if (agents) *agents = N;
    if (threads) *threads = 256;  // the epochs' workgroup: the ranking and the pulls are spread over the agents, whatever n
    if (per_launch) *per_launch = (uint32_t)per;
    return TL_OK;
}

// What the entries share.  log / route_log / epoch_log: run 0 of the call (a single run's trace), else nullptr
static int gsa_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                   uint32_t first_run, uint32_t count, const tl_gsa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                   uint32_t *best_index, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap,
                   uint32_t *epoch_log, uint32_t epoch_cap)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_run, "run")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kGsaUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    // HeuristicOptions::default (mod.rs:604-611)
    const uint32_t epochs = opts ? opts->epochs : 10000u, n_nearest = opts ? opts->n_nearest : 3u;
    const uint32_t N = gsa_agents(n_nearest), kb = gsa_kbest(N), row_words = 3u * N + 2u;
    if (epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 2^32 - 1 is not supported", who);
    if (N > kGsaMaxAgents) return fail(c, TL_ERR_UNSUPPORTED, "%s: n_nearest=%u: more than %u agents", who, n_nearest, kGsaMaxAgents);
    if (n > gravitational_search_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (8 bytes of LDS per city)", who, n, gravitational_search_max_n(c->lds_bytes));
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "%s: the initial tour is not a permutation of 0..n-1", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    if (n <= 1u) {  // no edge, no device: every cost is 0, the masses are uniform, every sequence is empty, nothing improves
        for (uint32_t r = 0; r < count; ++r) {
            if (n) out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
            if (out_moves) out_moves[r] = 0u;
        }
        if (log && log_cap) {  // record 0: the start gbest, agent 0 (all are equal)
            log[0] = 0xFFFFFFFFu;
            log[1] = log[2] = 0u;
            log[3] = route_log && route_cap ? 0u : 0xFFFFFFFFu;
        }
        if (route_log && route_cap && n) route_log[0] = 0u;
        if (epoch_log) {
            const uint64_t key = sa_chain_key(seed, first_run);
            const uint32_t rows = epoch_cap < epochs ? epoch_cap : epochs;
            const double mass = 1.0 / (double)N;  // kbest is 0 .. kb - 1
            memset(epoch_log, 0, (size_t)rows * row_words * 4);
            for (uint32_t e = 0; e < rows; ++e) {
                uint32_t *erow = epoch_log + (size_t)e * row_words;
                const double g = gsa_g(e, epochs);
                const uint64_t gb = __builtin_bit_cast(uint64_t, g);
                erow[3u * N] = (uint32_t)gb;
                erow[3u * N + 1u] = (uint32_t)(gb >> 32);
                for (uint32_t i = 0; i < N; ++i)
                    for (uint32_t j = 0; j < kb; ++j)
                        if (j != i && gsa_pull_swaps(gsa_r(key, e, N, i, j), g, mass)) ++erow[2u * N + i];
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
    tl_gravitational_search_plan(n, n_nearest, count, c->cus, c->lds_bytes, kGsaWorkDefault, 0u, nullptr, nullptr, &per_launch);
    if (per_launch == 0u)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u, %u agents: one run's tables (%llu bytes) exceed the workspace limit", who, n, N,
                    (unsigned long long)gsa_run_bytes(n, N));

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n;
    const uint32_t held = count < per_launch ? count : per_launch;  // runs whose agents exist at once
    const uint64_t most = 1ull + (uint64_t)epochs * N;               // the start gbest and at most one improvement per move
    const uint32_t dev_log_cap = log ? (uint32_t)(log_cap < most ? log_cap : most) : 0u;
    const uint32_t dev_route_cap = route_log ? (uint32_t)(route_cap < most ? route_cap : most) : 0u;
    const uint32_t dev_epoch_cap = epoch_log ? (epoch_cap < epochs ? epoch_cap : epochs) : 0u;
    const size_t log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16);
    const size_t route_bytes = up256((size_t)(dev_route_cap ? dev_route_cap : 1u) * n * 4);
    const size_t epoch_bytes = up256((size_t)(dev_epoch_cap ? dev_epoch_cap : 1u) * row_words * 4);
    const size_t tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), row4 = up256((size_t)held * N * 4),
                 row8 = up256((size_t)held * N * 8), row2 = up256((size_t)held * N * 2);
    if ((rc = ensure(c, c->init, (size_t)(init_count ? init_count : 1u) * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) ||
        (rc = ensure(c, c->out_cost, (size_t)count * 4)) || (rc = ensure(c, c->misc, (size_t)count * 32)) ||
        (rc = ensure(c, c->work, log_bytes + route_bytes + epoch_bytes + tab + gb + row4 + row8 + row2)))
        return rc;
    GsaArgs A{};
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
    A.mass = (double *)w;
    A.pos = (uint16_t *)(w + row8);
    A.gbest = (uint16_t *)(w + row8 + tab);
    w += row8 + tab + gb;
    A.cost = (float *)w;
    A.kbest = (uint16_t *)(w + row4);
    A.seed = seed;
    A.n = n;
    A.agents = N;
    A.vmax = pso_vmax(n);
    A.epochs = epochs;
    const uint32_t span = opts && opts->span_epochs ? opts->span_epochs : kGsaSpanEpochs;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the tables
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        GsaArgs L = A;
        L.first_run = first_run + b0;
        if (L.init && L.init_stride) L.init += (size_t)b0 * n;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.state = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) L.log = L.route_log = L.epoch_log = nullptr;  // the trace is run 0's
        L.last = epochs == 0u;
        HIPCHK(c, launch_gsa_init(L, cnt, c->stream));
        for (uint32_t e = 0; e < epochs;) {
            L.e0 = e;
            L.e1 = epochs - e > span ? e + span : epochs;
            L.last = L.e1 == epochs;
            HIPCHK(c, launch_gsa_epochs(L, cnt, c->stream));
            e = L.e1;
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> state;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 8u, out_pos, state, costs))) return rc;
    if (dev_epoch_cap) HIPCHK(c, hipMemcpyAsync(epoch_log, A.epoch_log, (size_t)dev_epoch_cap * row_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t r = 0; r < count; ++r)
        if (state[8u * r + 2u])
            return fail(c, TL_ERR_REF_PANICS, "%s: run %u: a cost or a mass is NaN — the reference panics on partial_cmp(..).unwrap()", who, first_run + r);
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

extern "C" int tl_gravitational_search(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_gsa_opts *opts,
                                       uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return gsa_run(c, "tl_gravitational_search", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats,
                   nullptr, 0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_gravitational_search_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_gsa_opts *opts,
                                             uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                             uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_gravitational_search_trace: NULL argument");
    return gsa_run(c, "tl_gravitational_search_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr,
                   stats, log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap);
}

extern "C" int tl_gravitational_search_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                                  uint32_t first_run, uint32_t count, const tl_gsa_opts *opts, uint64_t seed, uint32_t *out_pos,
                                                  float *out_costs, uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return gsa_run(c, "tl_gravitational_search_population", xy, n, dm_packed, init_pos, init_count, first_run, count, opts, seed, out_pos, out_costs, out_moves,
                   best_index, stats, nullptr, 0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_gsa_selftest_pull(tl_ctx *c, const uint32_t *from, const uint32_t *target, const uint32_t *prefix, uint32_t n, uint32_t count,
                                    uint32_t *out_pairs, uint32_t *out_len)
{
    TL_ENTER(c);
    if (!c || !from || !target || !prefix || !out_pairs || !out_len) return fail(c, TL_ERR_BADARG, "tl_gsa_selftest_pull: NULL argument");
    if (n < 1u || n > gravitational_search_max_n(c->lds_bytes) || count < 1u || count > kGsaMaxRuns)
        return fail(c, TL_ERR_BADARG, "tl_gsa_selftest_pull: n or count out of range");
    const size_t cells = (size_t)count * n;
    std::vector<uint16_t> h(2 * cells);
    const uint32_t *in[2] = {from, target};
    for (int a = 0; a < 2; ++a)
        for (uint32_t r = 0; r < count; ++r) {
            if (!is_permutation(in[a] + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "tl_gsa_selftest_pull: row %u is not a permutation of 0..n-1", r);
            for (uint32_t k = 0; k < n; ++k) h[a * cells + (size_t)r * n + k] = (uint16_t)in[a][(size_t)r * n + k];
        }
    for (uint32_t r = 0; r < count; ++r)
        if (prefix[r] > kGsaMaxPull) return fail(c, TL_ERR_BADARG, "tl_gsa_selftest_pull: prefix %u of row %u is above %u", prefix[r], r, kGsaMaxPull);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t tb = up256(cells * 2), lb = up256((size_t)count * 4), pb = up256((size_t)count * kGsaMaxPull * 4);
    if ((rc = ensure(c, c->work, 2 * tb + 2 * lb + pb))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    for (int a = 0; a < 2; ++a) HIPCHK(c, hipMemcpyAsync(w + a * tb, h.data() + a * cells, cells * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + 2 * tb, prefix, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_gsa_selftest_pull((const uint16_t *)w, (const uint16_t *)(w + tb), (const uint32_t *)(w + 2 * tb), n, count, (uint32_t *)(w + 2 * tb + 2 * lb),
                                       (uint32_t *)(w + 2 * tb + lb), c->stream));
    HIPCHK(c, hipMemcpyAsync(out_pairs, w + 2 * tb + 2 * lb, (size_t)count * kGsaMaxPull * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_len, w + 2 * tb + lb, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}
