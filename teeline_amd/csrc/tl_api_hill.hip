// tl_api_hill.hip — C ABI, the stochastic hill climb: tl_hill_climb* (src/tsp/stochastic_hill.rs:7-97) over hill_climb.hip and the
// host-only queries of its specification (tl_hill_draw, tl_hill_climb_plan).
#include "hill_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kHillUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static const tl_hill_opts kHillDefaults = {10000u, 500u, 0u, 0u};  // HeuristicOptions, mod.rs:598-608

extern "C" uint64_t tl_hill_draw(uint64_t seed, uint32_t chain, uint64_t event, uint32_t slot) { return hill_draw_key(sa_chain_key(seed, chain), event, slot); }

extern "C" uint32_t tl_hill_climb_lds_max_n(const tl_ctx *c) { return c ? hill_climb_lds_max_n(c->lds_bytes) : 0u; }

// sim_anneal's widths: a chain alone on its CU gets four waves (one per SIMD) and a window as wide; once there are more chains than
// CUs a chain is one wave, and a CU holds as many as its LDS and its 32 wave slots allow.  (Wider single chains: not measured,
// NOTEBOOK.md.)  window_request: 0 the plan's, else 1 .. threads.
extern "C" int tl_hill_climb_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint32_t window_request, uint32_t *window, int *threads,
                                  uint32_t *per_launch)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    const bool fits = n >= 2u && n <= hill_climb_lds_max_n(lds_bytes);
    const int nt = !fits ? 0 : count > (uint32_t)cus ? 64 : 256;
    if (window) *window = 0u;
    if (threads) *threads = 0;
    if (per_launch) *per_launch = 0u;
    if (!fits) return TL_OK;
    if (window_request > (uint32_t)nt) return TL_ERR_BADARG;
    if (window) *window = window_request ? window_request : (uint32_t)nt;
    if (threads) *threads = nt;
    if (per_launch) {
        const uint64_t per = chains_per_cu(lds_bytes, hill_climb_lds_bytes(n), nt) * (uint32_t)cus;
        *per_launch = per > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)per;
    }
    return TL_OK;
}

// What the entries share.  log: the events of chain 0 of the call (a single chain's trace), else nullptr
static int hill_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                    uint32_t first_chain, uint32_t count, const tl_hill_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                    uint32_t *best_index, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_chain, "chain")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kHillUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    const tl_hill_opts o = opts ? *opts : kHillDefaults;
    if (o.reserved != 0u) return fail(c, TL_ERR_BADARG, "%s: opts->reserved is %u, not 0", who, o.reserved);
    if (o.epochs == 0u) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 0 never ends in the reference (stochastic_hill.rs:80-82)", who);
    if (o.epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs + 1 epochs run, and 2^32 do not fit", who);
    if (n < 2u) return fail(c, TL_ERR_REF_PANICS, "%s: n=%u: the reference panics (route.rs:87-89 random_pair, n_items < 2)", who, n);
    if (n > hill_climb_lds_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the LDS-resident limit %u (no HBM form)", who, n, hill_climb_lds_max_n(c->lds_bytes));
    uint32_t window = 0, per_launch = 0;
    int threads = 0;
    if (tl_hill_climb_plan(n, count, c->cus, c->lds_bytes, o.window, &window, &threads, &per_launch) != TL_OK)
        return fail(c, TL_ERR_BADARG, "%s: opts->window is %u: 0 (the plan's) or 1 .. %d, the threads of a chain's workgroup", who, o.window,
                    count > (uint32_t)c->cus ? 64 : 256);
    if (per_launch == 0u) return fail(c, TL_ERR_UNSUPPORTED, "%s: no plan for this device", who);
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n))
            return fail(c, TL_ERR_BADARG, "%s: start tour %u is not a permutation of 0..n-1", who, r);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    const uint32_t total = o.epochs + 1u;  // stochastic_hill.rs:80-82: `epoch > epochs` after the increment

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n, starts = init_count ? init_count : 1u;
    const uint32_t dev_log_cap = move_log ? log_cap : 0u;
    if ((rc = ensure(c, c->init, starts * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) || (rc = ensure(c, c->out_cost, (size_t)count * 4)) ||
        (rc = ensure(c, c->misc, (size_t)count * 16)) || (rc = ensure(c, c->work, up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16))))
        return rc;
    HillArgs A{};
    if ((rc = upload_instance_full(c, xy, dm_packed, n, &A.xy, &A.dm_full))) return rc;
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, (size_t)count * 16, c->stream));
    A.log = move_log ? (uint32_t *)c->work.p : nullptr;
    A.log_cap = dev_log_cap;
    A.seed = seed;
    A.n = n;
    A.epochs = total;
    A.platoo = o.platoo_epochs;
    A.window = window;
    if ((rc = upload_start_sync(c, init_count ? init_pos : nullptr, n, c->init.p, starts))) return rc;  // city order, one tour, or one per chain
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    A.init_stride = init_count == count ? n : 0u;  // (0: every chain from the one tour uploaded)
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        HillArgs L = A;
        L.first_chain = first_chain + b0;
        L.init = (const uint32_t *)c->init.p + (size_t)b0 * A.init_stride;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.out_run = (uint32_t *)c->misc.p + 4u * (size_t)b0;
        if (b0) L.log = nullptr;  // the trace is chain 0's
        HIPCHK(c, launch_hill_climb(L, cnt, threads, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> run;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 4u, out_pos, run, costs))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t events = (uint64_t)run[0] + run[3];  // (at most one event an epoch: below 2^32)
    if (move_log && dev_log_cap && events && (rc = download_sync(c, move_log, A.log, (size_t)(events < dev_log_cap ? events : dev_log_cap) * 16))) return rc;
    if (log_len) *log_len = (uint32_t)events;
    uint64_t moves = 0, reversed = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (out_costs) out_costs[r] = costs[r];
        if (out_moves) out_moves[r] = run[4u * r];
        moves += run[4u * r];
        reversed += (uint64_t)run[4u * r + 2u] << 32 | run[4u * r + 1u];
    }
    if (best_index) *best_index = best_chain(costs, count);
    if (stats) {
        stats->sweeps = stats->candidates = (uint64_t)total * count;
        stats->moves = moves;
        stats->reversed = reversed;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_hill_climb(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_hill_opts *opts, uint64_t seed,
                             uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return hill_run(c, "tl_hill_climb", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats, nullptr,
                    0, nullptr);
}

extern "C" int tl_hill_climb_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_hill_opts *opts,
                                   uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_hill_climb_trace: NULL argument");
    return hill_run(c, "tl_hill_climb_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats,
                    log, log_cap, log_len);
}

extern "C" int tl_hill_climb_trace_chain(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_hill_opts *opts,
                                         uint64_t seed, uint32_t chain, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                         uint32_t *log_len)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_hill_climb_trace_chain: NULL argument");
    return hill_run(c, "tl_hill_climb_trace_chain", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, chain, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr,
                    stats, log, log_cap, log_len);
}

extern "C" int tl_hill_climb_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                        uint32_t first_chain, uint32_t count, const tl_hill_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                        uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return hill_run(c, "tl_hill_climb_population", xy, n, dm_packed, init_pos, init_count, first_chain, count, opts, seed, out_pos, out_costs, out_moves,
                    best_index, stats, nullptr, 0, nullptr);
}
