// tl_api_tabu.hip — C ABI, tabu search: tl_tabu_search* (src/tsp/tabu_search.rs:9-110) over tabu_search.hip and the host-only queries
// of its specification (tl_tabu_draw, tl_tabu_search_plan).
#include "tabu_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kTabuUnassignedFlags = 1u << 31;     // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kTabuWorkDefault = 8ull << 30;       // the rings of one launch (the precedent of tl_three_opt_population)

// one chain's share of the workspace: its ring of n routes (16-bit entries) and their hashes
static inline size_t tabu_ring_bytes(uint32_t n) { return up256((size_t)n * n * 2); }
static inline size_t tabu_hash_bytes(uint32_t n) { return up256((size_t)n * 4); }

extern "C" uint64_t tl_tabu_draw(uint64_t seed, uint32_t chain, uint32_t n, uint32_t epoch, uint32_t attempt, uint32_t slot)
{
    return tabu_draw_key(sa_chain_key(seed, chain), tabu_event(epoch, n, attempt), slot);
}

extern "C" uint32_t tl_tabu_search_lds_max_n(const tl_ctx *c) { return c ? tabu_search_lds_max_n(c->lds_bytes) : 0u; }

// A chain alone on its CU gets four waves (one per SIMD) and a round as wide; once there are more chains than CUs a chain is one
// wave, and a CU holds as many as its LDS and its 32 wave slots allow.  One launch holds no more chains than have their rings in
// workspace_bytes.  (sim_anneal's widths; others not measured: NOTEBOOK.md.)
extern "C" int tl_tabu_search_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags, uint32_t *window,
                                   int *threads, uint32_t *per_launch)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (flags & kTabuUnassignedFlags) return TL_ERR_UNSUPPORTED;
    const bool fits = n >= 2u && n <= tabu_search_lds_max_n(lds_bytes);
    const int nt = !fits ? 0 : count > (uint32_t)cus ? 64 : 256;
    if (window) *window = (uint32_t)nt;
    if (threads) *threads = nt;
    if (per_launch) {
        uint64_t per = fits ? chains_per_cu(lds_bytes, tabu_search_lds_bytes(n), nt) * (uint32_t)cus : 0u;
        const uint64_t held = fits ? workspace_bytes / (tabu_ring_bytes(n) + tabu_hash_bytes(n)) : 0u;
        if (per > held) per = held;
        *per_launch = per > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)per;
    }
    return TL_OK;
}

// What the entries share.  log: every epoch of chain 0 of the call (a single chain's trace), else nullptr
static int tabu_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                    uint32_t first_chain, uint32_t count, uint32_t epochs, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                    uint32_t *best_index, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_chain, "chain")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kTabuUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    if (epochs == 0u) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 0 never ends in the reference (tabu_search.rs:83-85)", who);
    if (epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs + 1 epochs run, and 2^32 do not fit", who);
    if (n < 2u) return fail(c, TL_ERR_REF_PANICS, "%s: n=%u: the reference panics (route.rs:87-89 random_pair, n_items < 2)", who, n);
    if (n > tabu_search_lds_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the LDS-resident limit %u (no HBM form)", who, n, tabu_search_lds_max_n(c->lds_bytes));
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n))
            return fail(c, TL_ERR_BADARG, "%s: start tour %u is not a permutation of 0..n-1", who, r);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    uint32_t per_launch = 0;
    int threads = 0;
    tl_tabu_search_plan(n, count, c->cus, c->lds_bytes, kTabuWorkDefault, c->flags, nullptr, &threads, &per_launch);
    if (per_launch == 0u) return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u: one chain's list (%zu bytes) exceeds the workspace limit", who, n, tabu_ring_bytes(n));
    const uint32_t total = epochs + 1u;  // update_terminate (tabu_search.rs:83-85): `epoch > epochs` after the increment

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n, starts = init_count ? init_count : 1u;
    const uint32_t held = count < per_launch ? count : per_launch;  // chains whose lists exist at once
    const uint32_t dev_log_cap = move_log ? (log_cap < total ? log_cap : total) : 0u;
    const size_t log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16);
    if ((rc = ensure(c, c->init, starts * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) || (rc = ensure(c, c->out_cost, (size_t)count * 4)) ||
        (rc = ensure(c, c->misc, (size_t)count * 32)) || (rc = ensure(c, c->work, log_bytes + (size_t)held * (tabu_ring_bytes(n) + tabu_hash_bytes(n)))))
        return rc;
    TabuArgs A{};
    if ((rc = upload_instance_full(c, xy, dm_packed, n, &A.xy, &A.dm_full))) return rc;
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, (size_t)count * 32, c->stream));
    unsigned char *w = (unsigned char *)c->work.p;
    A.log = move_log ? (uint32_t *)w : nullptr;
    A.log_cap = dev_log_cap;
    A.ring = (uint16_t *)(w + log_bytes);
    A.ring_stride = tabu_ring_bytes(n) / 2;
    A.hashes = (uint32_t *)(w + log_bytes + (size_t)held * tabu_ring_bytes(n));
    A.seed = seed;
    A.n = n;
    A.epochs = total;
    A.full_compare = (c->flags & TL_FLAG_TABU_FULL_COMPARE) ? 1u : 0u;
    if ((rc = upload_start_sync(c, init_count ? init_pos : nullptr, n, c->init.p, starts))) return rc;  // city order, one tour, or one per chain
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    A.init_stride = init_count == count ? n : 0u;  // (0: every chain from the one tour uploaded)
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // launches on one stream follow each other: the next takes over the rings
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        TabuArgs L = A;
        L.first_chain = first_chain + b0;
        L.init = (const uint32_t *)c->init.p + (size_t)b0 * A.init_stride;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.out_run = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) L.log = nullptr;  // the trace is chain 0's
        HIPCHK(c, launch_tabu_search(L, cnt, threads, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> run;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 8u, out_pos, run, costs))) return rc;
    if (move_log && dev_log_cap) HIPCHK(c, hipMemcpyAsync(move_log, A.log, (size_t)dev_log_cap * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (log_len) *log_len = total;
    uint64_t moves = 0, candidates = 0, reversed = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (out_costs) out_costs[r] = costs[r];
        if (out_moves) out_moves[r] = run[8u * r];
        moves += run[8u * r];
        candidates += (uint64_t)run[8u * r + 2u] << 32 | run[8u * r + 1u];
        reversed += (uint64_t)run[8u * r + 4u] << 32 | run[8u * r + 3u];
    }
    if (best_index) *best_index = best_chain(costs, count);
    if (stats) {
        stats->sweeps = (uint64_t)total * count;
        stats->candidates = candidates;
        stats->moves = moves;
        stats->reversed = reversed;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_tabu_search(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, uint64_t seed,
                              uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return tabu_run(c, "tl_tabu_search", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, epochs, seed, out_pos, out_cost, nullptr, nullptr, stats, nullptr,
                    0, nullptr);
}

extern "C" int tl_tabu_search_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, uint64_t seed,
                                    uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    TL_ENTER(c);
    if (!move_log || !log_len) return fail(c, TL_ERR_BADARG, "tl_tabu_search_trace: NULL argument");
    return tabu_run(c, "tl_tabu_search_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, epochs, seed, out_pos, out_cost, nullptr, nullptr, stats,
                    move_log, log_cap, log_len);
}

extern "C" int tl_tabu_search_trace_chain(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                                          uint64_t seed, uint32_t chain, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log,
                                          uint32_t log_cap, uint32_t *log_len)
{
    TL_ENTER(c);
    if (!move_log || !log_len) return fail(c, TL_ERR_BADARG, "tl_tabu_search_trace_chain: NULL argument");
    return tabu_run(c, "tl_tabu_search_trace_chain", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, chain, 1u, epochs, seed, out_pos, out_cost, nullptr,
                    nullptr, stats, move_log, log_cap, log_len);
}

extern "C" int tl_tabu_search_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                         uint32_t first_chain, uint32_t count, uint32_t epochs, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                         uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return tabu_run(c, "tl_tabu_search_population", xy, n, dm_packed, init_pos, init_count, first_chain, count, epochs, seed, out_pos, out_costs, out_moves,
                    best_index, stats, nullptr, 0, nullptr);
}
