// tl_api_ga.hip — C ABI, the genetic algorithm: tl_genetic_algorithm* (src/tsp/genetic_algorithm.rs:16-336) over genetic.hip, the
// host-only queries of its specification (tl_ga_draw, tl_genetic_algorithm_plan) and the device self-test of the crossover.
#include "ga_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kGaUnassignedFlags = 1u << 31;   // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kGaWorkDefault = 8ull << 30;     // the populations of one launch sequence (the precedent of tl_tabu_search)
static constexpr uint32_t kGaMaxRuns = 65535u;             // the run is the grid's y

// one run's share of the workspace: two populations of n routes (16-bit entries), two fitness arrays, the order, the prefix
static inline size_t ga_pop_bytes(uint32_t n) { return up256((size_t)n * n * 2); }
static inline size_t ga_row_bytes(uint32_t n) { return up256(((size_t)n + 1) * 4); }
static inline size_t ga_run_bytes(uint32_t n) { return 2 * ga_pop_bytes(n) + 4 * ga_row_bytes(n); }

extern "C" uint64_t tl_ga_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" uint32_t tl_genetic_algorithm_max_n(const tl_ctx *c) { return c ? genetic_max_n(c->lds_bytes) : 0u; }

extern "C" int tl_genetic_algorithm_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t *per_launch, int *threads,
                                         uint64_t *workspace_needed)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    const bool fits = n >= 1u && n <= genetic_max_n(lds_bytes);
    uint64_t per = fits ? workspace_bytes / ga_run_bytes(n) : 0u;
    if (per > kGaMaxRuns) per = kGaMaxRuns;
    if (per_launch) *per_launch = (uint32_t)per;
    if (threads) *threads = per ? genetic_threads(n) : 0;
    if (workspace_needed) *workspace_needed = per ? (uint64_t)(count < per ? count : per) * ga_run_bytes(n) : 0u;
    return TL_OK;
}

// What the entries share.  log / route_log: the generations of run 0 of the call (a single run's trace), else nullptr
static int ga_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t first_run, uint32_t count,
                  uint32_t epochs, float p_mut, uint32_t n_elite, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *best_index, tl_stats *stats,
                  uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_pos ? 1u : 0u, first_run, "run")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kGaUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    if (!(p_mut >= 0.0f && p_mut <= 1.0f)) return fail(c, TL_ERR_BADARG, "%s: mutation_probability must be in [0, 1] (got %g)", who, (double)p_mut);
    if (n == 0u) return fail(c, TL_ERR_REF_PANICS, "%s: n=0: the reference panics (genetic_algorithm.rs:257-262 best() of an empty population)", who);
    if (n > genetic_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (14 bytes of LDS per city)", who, n, genetic_max_n(c->lds_bytes));
    if (init_pos && !is_permutation(init_pos, n)) return fail(c, TL_ERR_BADARG, "%s: the initial tour is not a permutation of 0..n-1", who);
    if (epochs >= 1u && ga_next_len(n, n_elite, n) == 0u)
        return fail(c, TL_ERR_REF_PANICS, "%s: n=%u, n_elite=0: the reference panics (no pair and no elite: best() of an empty population)", who, n);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    const uint32_t pairs = ga_pairs(n, n_elite);
    if (n == 1u) {  // one city: no distance, no draw — every population is the one route, fitness 0
        for (uint32_t r = 0; r < count; ++r) {
            out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
        }
        for (uint32_t g = 0; g < epochs && log && g < log_cap; ++g) {
            log[4u * (size_t)g] = log[4u * (size_t)g + 1u] = log[4u * (size_t)g + 2u] = 0u;
            log[4u * (size_t)g + 3u] = 1u;
        }
        for (uint32_t g = 0; g < epochs && route_log && g < route_cap; ++g) route_log[g] = 0u;
        if (log_len) *log_len = epochs;
        c->ev_valid = false;
        if (stats) {
            stats->sweeps = (uint64_t)epochs * count;
            stamp_times(c, stats, t0);
        }
        return TL_OK;
    }
    uint32_t per_launch = 0;
    tl_genetic_algorithm_plan(n, count, c->cus, c->lds_bytes, kGaWorkDefault, &per_launch, nullptr, nullptr);
    if (per_launch == 0u) return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u: one run's populations (%zu bytes) exceed the workspace limit", who, n, ga_run_bytes(n));

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n;
    const uint32_t held = count < per_launch ? count : per_launch;  // runs whose populations exist at once
    const uint32_t dev_log_cap = log ? (log_cap < epochs ? log_cap : epochs) : 0u;
    const uint32_t dev_route_cap = route_log ? (route_cap < epochs ? route_cap : epochs) : 0u;
    const size_t log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16);
    const size_t route_bytes = up256((size_t)(dev_route_cap ? dev_route_cap : 1u) * n * 4);
    if ((rc = ensure(c, c->init, (size_t)n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) || (rc = ensure(c, c->out_cost, (size_t)count * 4)) ||
        (rc = ensure(c, c->misc, (size_t)count * 32)) || (rc = ensure(c, c->work, log_bytes + route_bytes + (size_t)held * ga_run_bytes(n))))
        return rc;
    GaArgs A{};
    if ((rc = upload_instance_full(c, xy, dm_packed, n, &A.xy, &A.dm_full))) return rc;
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, (size_t)count * 32, c->stream));
    if (init_pos) {
        HIPCHK(c, hipMemcpyAsync(c->init.p, init_pos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        A.init = (const uint32_t *)c->init.p;
    }
    unsigned char *w = (unsigned char *)c->work.p;
    A.log = log ? (uint32_t *)w : nullptr;
    A.log_cap = dev_log_cap;
    A.route_log = route_log ? (uint32_t *)(w + log_bytes) : nullptr;
    A.route_cap = dev_route_cap;
    w += log_bytes + route_bytes;
    A.pop[0] = (uint16_t *)w;
    A.pop[1] = (uint16_t *)(w + (size_t)held * ga_pop_bytes(n));
    A.pop_stride = ga_pop_bytes(n) / 2;
    w += 2 * (size_t)held * ga_pop_bytes(n);
    A.fit[0] = (float *)w;
    A.fit[1] = (float *)(w + (size_t)held * ga_row_bytes(n));
    A.order = (uint32_t *)(w + 2 * (size_t)held * ga_row_bytes(n));
    A.prefix = (float *)(w + 3 * (size_t)held * ga_row_bytes(n));
    A.seed = seed;
    A.n = n;
    A.n_elite = n_elite;
    A.p_mut = p_mut;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the populations
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        GaArgs L = A;
        L.first_run = first_run + b0;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.state = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) L.log = L.route_log = nullptr;  // the trace is run 0's
        HIPCHK(c, launch_ga_init(L, cnt, c->stream));
        L.len = n;
        L.src = 0u;
        L.generation = 0u;
        L.last = epochs == 0u;
        HIPCHK(c, launch_ga_rank(L, cnt, c->stream));
        for (uint32_t g = 0; g < epochs; ++g) {
            const uint32_t next = ga_next_len(n, n_elite, L.len);
            L.generation = g;
            HIPCHK(c, launch_ga_breed(L, cnt, next, c->stream));
            L.src ^= 1u;
            L.len = next;
            L.generation = g + 1u;
            L.last = g + 1u == epochs;
            HIPCHK(c, launch_ga_rank(L, cnt, c->stream));
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> state;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 8u, out_pos, state, costs))) return rc;
    if (dev_log_cap) HIPCHK(c, hipMemcpyAsync(log, A.log, (size_t)dev_log_cap * 16, hipMemcpyDeviceToHost, c->stream));
    if (dev_route_cap) HIPCHK(c, hipMemcpyAsync(route_log, A.route_log, (size_t)dev_route_cap * n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t improved = 0, mutations = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (state[8u * r + 3u]) {
            if (best_index) *best_index = best_chain(costs, r);  // of the runs before it, like the out_costs written so far
            return fail(c, TL_ERR_REF_PANICS, "%s: run %u: the reference panics (genetic_algorithm.rs:277 random_range on an empty range: total fitness not > 0 or not finite)",
                        who, first_run + r);
        }
        if (out_costs) out_costs[r] = costs[r];
        improved += state[8u * r + 1u];
        mutations += state[8u * r + 2u];
    }
    if (best_index) *best_index = best_chain(costs, count);
    if (log_len) *log_len = epochs;
    if (stats) {
        stats->sweeps = (uint64_t)epochs * count;
        stats->candidates = 2ull * pairs * epochs * count;
        stats->moves = improved;
        stats->reversed = mutations;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_genetic_algorithm(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                                    float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return ga_run(c, "tl_genetic_algorithm", xy, n, dm_packed, init_pos, 0u, 1u, epochs, mutation_probability, n_elite, seed, out_pos, out_cost, nullptr, stats,
                  nullptr, 0, nullptr, nullptr, 0);
}

extern "C" int tl_genetic_algorithm_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                                          float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats,
                                          uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_genetic_algorithm_trace: NULL argument");
    return ga_run(c, "tl_genetic_algorithm_trace", xy, n, dm_packed, init_pos, 0u, 1u, epochs, mutation_probability, n_elite, seed, out_pos, out_cost, nullptr,
                  stats, log, log_cap, log_len, route_log, route_cap);
}

extern "C" int tl_genetic_algorithm_trace_run(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                                              float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost,
                                              tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_genetic_algorithm_trace_run: NULL argument");
    return ga_run(c, "tl_genetic_algorithm_trace_run", xy, n, dm_packed, init_pos, run, 1u, epochs, mutation_probability, n_elite, seed, out_pos, out_cost,
                  nullptr, stats, log, log_cap, log_len, route_log, route_cap);
}

extern "C" int tl_genetic_algorithm_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t first_run,
                                               uint32_t count, uint32_t epochs, float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t *out_pos,
                                               float *out_costs, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return ga_run(c, "tl_genetic_algorithm_population", xy, n, dm_packed, init_pos, first_run, count, epochs, mutation_probability, n_elite, seed, out_pos,
                  out_costs, best_index, stats, nullptr, 0, nullptr, nullptr, 0);
}

extern "C" int tl_ga_selftest_crossover(tl_ctx *c, const uint32_t *p1, const uint32_t *p2, uint32_t n, uint32_t from, uint32_t to, uint32_t *out1,
                                        uint32_t *out2)
{
    TL_ENTER(c);
    if (!c || !p1 || !p2 || !out1 || !out2) return fail(c, TL_ERR_BADARG, "tl_ga_selftest_crossover: NULL argument");
    if (n < 2u || n > genetic_max_n(c->lds_bytes) || from > to || to >= n) return fail(c, TL_ERR_BADARG, "tl_ga_selftest_crossover: n, from or to out of range");
    if (!is_permutation(p1, n) || !is_permutation(p2, n)) return fail(c, TL_ERR_BADARG, "tl_ga_selftest_crossover: a parent is not a permutation of 0..n-1");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t row = up256((size_t)n * 2);
    if ((rc = ensure(c, c->work, 4 * row))) return rc;
    std::vector<uint16_t> h(2 * (size_t)n), o(2 * (size_t)n);
    for (uint32_t k = 0; k < n; ++k) {
        h[k] = (uint16_t)p1[k];
        h[n + k] = (uint16_t)p2[k];
    }
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    HIPCHK(c, hipMemcpyAsync(w, h.data(), (size_t)n * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + row, h.data() + n, (size_t)n * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_ga_selftest_crossover((const uint16_t *)w, (const uint16_t *)(w + row), n, from, to, (uint16_t *)(w + 2 * row), (uint16_t *)(w + 3 * row),
                                           c->stream));
    HIPCHK(c, hipMemcpyAsync(o.data(), w + 2 * row, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o.data() + n, w + 3 * row, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n; ++k) {
        out1[k] = o[k];
        out2[k] = o[n + k];
    }
    return TL_OK;
}
