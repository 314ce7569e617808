// tl_api_cs.hip — C ABI, the cuckoo search solver: tl_cuckoo_search* (src/tsp/cuckoo_search.rs:26-136) over cuckoo_search.hip, the
// host-only queries of its specification (tl_cs_draw, tl_levy_from_words, tl_cs_flight_length, tl_cs_pa, tl_cuckoo_search_plan)
// and the device self-tests of the Lévy step and of the reversals' gather.
#include "cs_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kCsUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kCsWorkDefault = 8ull << 30;    // the runs of one launch sequence
static constexpr uint32_t kCsMaxRuns = 65535u;            // the run is the grid's y
static constexpr uint64_t kCsLayoutSlack = 11 * 256;      // the arrays of a sequence each start on a 256-byte boundary

// one run's share of the workspace: nests, staged flights and staged replacements (N n u16 each), best, four rows of N words
static inline uint64_t cs_run_bytes(uint32_t n, uint32_t N) { return 6ull * N * n + 2ull * n + 16ull * N; }

namespace {
struct GivenWords {
    const uint64_t *w;
    uint64_t operator()(uint32_t i) const { return w[i]; }
};
}  // namespace

extern "C" uint64_t tl_cs_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" double tl_levy_from_words(const uint64_t *words, uint32_t *resamples)
{
    if (!words) {
        if (resamples) *resamples = 0u;
        return 0.0;
    }
    return levy_step(GivenWords{words}, resamples);
}

extern "C" uint32_t tl_cs_flight_length(double levy, uint32_t n) { return n < 2u ? 0u : cs_flight_length(levy, n); }

extern "C" double tl_cs_pa(float mutation_probability) { return cs_pa(mutation_probability); }

extern "C" uint32_t tl_cuckoo_search_max_n(const tl_ctx *c) { return c ? cuckoo_search_max_n(c->lds_bytes) : 0u; }

extern "C" int tl_cuckoo_search_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                     uint32_t *nests, int *threads, uint32_t *per_launch)
{
    if (nests) *nests = 0u;
    if (threads) *threads = 0;
    if (per_launch) *per_launch = 0u;
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (flags & kCsUnassignedFlags) return TL_ERR_UNSUPPORTED;
    const uint32_t N = cs_nests(n_nearest);
    if (n < 2u || n > cuckoo_search_max_n(lds_bytes) || N > kCsMaxNests) return TL_OK;
    uint64_t per = workspace_bytes > kCsLayoutSlack ? (workspace_bytes - kCsLayoutSlack) / cs_run_bytes(n, N) : 0u;
    if (per > kCsMaxRuns) per = kCsMaxRuns;
    (void)count;
    if (per == 0u) return TL_OK;
    if (nests) *nests = N;
    if (threads) *threads = cuckoo_search_threads(n);
    if (per_launch) *per_launch = (uint32_t)per;
    return TL_OK;
}

// What the entries share.  log / route_log / epoch_log: run 0 of the call (a single run's trace), else nullptr
static int cs_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                  uint32_t first_run, uint32_t count, const tl_cs_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                  uint32_t *best_index, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap,
                  uint32_t *epoch_log, uint32_t epoch_cap)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_run, "run")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kCsUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    // CSOptions::default (mod.rs:918-925) over HeuristicOptions::default (mod.rs:604-611)
    const uint32_t epochs = opts ? opts->epochs : 10000u, n_nearest = opts ? opts->n_nearest : 3u;
    const float p_mut = opts ? opts->mutation_probability : 0.001f;
    const uint32_t N = cs_nests(n_nearest);
    if (!(p_mut >= 0.0f && p_mut <= 1.0f)) return fail(c, TL_ERR_BADARG, "%s: mutation_probability must be in [0, 1] (got %g)", who, (double)p_mut);
    if (epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 2^32 - 1 is not supported", who);
    if (N > kCsMaxNests) return fail(c, TL_ERR_UNSUPPORTED, "%s: n_nearest=%u: more than %u nests", who, n_nearest, kCsMaxNests);
    if (n > cuckoo_search_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (10 bytes of LDS per city)", who, n, cuckoo_search_max_n(c->lds_bytes));
    if (!cs_events_fit(epochs, N, n)) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs x nests x (n + 1) exceeds 2^58 events", who);
    if (n <= 1u && epochs >= 1u)
        return fail(c, TL_ERR_REF_PANICS, "%s: n=%u: the reference panics (cuckoo_search.rs:85 clamp(1, n / 2) with min > max)", who, n);
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "%s: the initial tour is not a permutation of 0..n-1", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    if (n <= 1u) {  // (epochs = 0) no edge, no device: the start best is the one route (or the empty one) at cost 0, nest 0's
        for (uint32_t r = 0; r < count; ++r) {
            if (n) out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
            if (out_moves) out_moves[r] = 0u;
        }
        if (log && log_cap) {
            log[0] = 0xFFFFFFFFu;
            log[1] = log[2] = 0u;
            log[3] = route_log && route_cap ? 0u : 0xFFFFFFFFu;
        }
        if (route_log && route_cap && n) route_log[0] = 0u;
        if (log_len) *log_len = 1u;
        c->ev_valid = false;
        if (stats) stamp_times(c, stats, t0);
        return TL_OK;
    }
    uint32_t per_launch = 0;
    tl_cuckoo_search_plan(n, n_nearest, count, c->cus, c->lds_bytes, kCsWorkDefault, 0u, nullptr, nullptr, &per_launch);
    if (per_launch == 0u)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u, %u nests: one run's tables (%llu bytes) exceed the workspace limit", who, n, N,
                    (unsigned long long)cs_run_bytes(n, N));

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n;
    const uint32_t held = count < per_launch ? count : per_launch;  // runs whose nests exist at once
    const uint64_t most = 1ull + 2ull * epochs * N;                  // the start best, at most one improvement per flight and per abandonment
    const uint32_t dev_log_cap = log ? (uint32_t)(log_cap < most ? log_cap : most) : 0u;
    const uint32_t dev_route_cap = route_log ? (uint32_t)(route_cap < most ? route_cap : most) : 0u;
    const uint32_t dev_epoch_cap = epoch_log ? (epoch_cap < epochs ? epoch_cap : epochs) : 0u;
    const size_t log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16);
    const size_t route_bytes = up256((size_t)(dev_route_cap ? dev_route_cap : 1u) * n * 4);
    const size_t epoch_bytes = up256((size_t)(dev_epoch_cap ? dev_epoch_cap : 1u) * 4 * N * 4);
    const size_t tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), row = up256((size_t)held * N * 4);
    if ((rc = ensure(c, c->init, (size_t)(init_count ? init_count : 1u) * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) ||
        (rc = ensure(c, c->out_cost, (size_t)count * 4)) || (rc = ensure(c, c->misc, (size_t)count * 32)) ||
        (rc = ensure(c, c->work, log_bytes + route_bytes + epoch_bytes + 3 * tab + gb + 4 * row)))
        return rc;
    CsArgs A{};
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
    A.nest = (uint16_t *)w;
    A.fly = (uint16_t *)(w + tab);
    A.repl = (uint16_t *)(w + 2 * tab);
    A.best = (uint16_t *)(w + 3 * tab);
    w += 3 * tab + gb;
    A.cost = (float *)w;
    A.fcost = (float *)(w + row);
    A.rcost = (float *)(w + 2 * row);
    A.fk = (uint32_t *)(w + 3 * row);
    A.seed = seed;
    A.pa = cs_pa(p_mut);
    A.n = n;
    A.nests = N;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the tables
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        CsArgs L = A;
        L.first_run = first_run + b0;
        if (L.init && L.init_stride) L.init += (size_t)b0 * n;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.state = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) L.log = L.route_log = L.epoch_log = nullptr;  // the trace is run 0's
        L.last = epochs == 0u;
        HIPCHK(c, launch_cs_init(L, cnt, c->stream));
        for (uint32_t e = 0; e < epochs; ++e) {
            L.epoch = e;
            L.last = e + 1u == epochs;
            HIPCHK(c, launch_cs_fly(L, cnt, c->stream));
            HIPCHK(c, launch_cs_commit(L, cnt, c->stream));
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

extern "C" int tl_cuckoo_search(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_cs_opts *opts, uint64_t seed,
                                uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return cs_run(c, "tl_cuckoo_search", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats, nullptr, 0,
                  nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_cuckoo_search_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_cs_opts *opts,
                                      uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                      uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_cuckoo_search_trace: NULL argument");
    return cs_run(c, "tl_cuckoo_search_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats, log,
                  log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap);
}

extern "C" int tl_cuckoo_search_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                           uint32_t first_run, uint32_t count, const tl_cs_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                           uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return cs_run(c, "tl_cuckoo_search_population", xy, n, dm_packed, init_pos, init_count, first_run, count, opts, seed, out_pos, out_costs, out_moves, best_index,
                  stats, nullptr, 0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_cs_selftest_levy(tl_ctx *c, const uint64_t *words, uint32_t count, uint32_t n, uint64_t *out_bits, uint32_t *out_k, uint32_t *out_resamples)
{
    TL_ENTER(c);
    if (!c || !words || !out_bits || !out_k || !out_resamples) return fail(c, TL_ERR_BADARG, "tl_cs_selftest_levy: NULL argument");
    if (n < 2u || count < 1u || count > (1u << 24)) return fail(c, TL_ERR_BADARG, "tl_cs_selftest_levy: n or count out of range");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t in = up256((size_t)count * kLevyWords * 8), ob = up256((size_t)count * 8), ow = up256((size_t)count * 4);
    if ((rc = ensure(c, c->work, in + ob + 2 * ow))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    HIPCHK(c, hipMemcpyAsync(w, words, (size_t)count * kLevyWords * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_cs_selftest_levy((const uint64_t *)w, count, n, (uint64_t *)(w + in), (uint32_t *)(w + in + ob), (uint32_t *)(w + in + ob + ow), c->stream));
    HIPCHK(c, hipMemcpyAsync(out_bits, w + in, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_k, w + in + ob, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_resamples, w + in + ob + ow, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}

extern "C" int tl_cs_selftest_reversals(tl_ctx *c, const uint32_t *tours, const uint32_t *pairs, const uint32_t *lens, uint32_t n, uint32_t kcap, uint32_t count,
                                        uint32_t *out)
{
    TL_ENTER(c);
    if (!c || !tours || !pairs || !lens || !out) return fail(c, TL_ERR_BADARG, "tl_cs_selftest_reversals: NULL argument");
    if (n < 2u || n > cuckoo_search_max_n(c->lds_bytes) || count < 1u || count > kCsMaxRuns || kcap < 1u || kcap > n / 2u)
        return fail(c, TL_ERR_BADARG, "tl_cs_selftest_reversals: n, kcap or count out of range");
    const size_t cells = (size_t)count * n, pcells = (size_t)count * kcap;
    std::vector<uint16_t> h(cells);
    std::vector<uint32_t> packed(pcells, 0u);
    for (uint32_t r = 0; r < count; ++r) {
        if (lens[r] > kcap) return fail(c, TL_ERR_BADARG, "tl_cs_selftest_reversals: row %u holds more than kcap pairs", r);
        for (uint32_t k = 0; k < n; ++k) {
            if (tours[(size_t)r * n + k] > 0xFFFFu) return fail(c, TL_ERR_BADARG, "tl_cs_selftest_reversals: row %u holds an element above 65535", r);
            h[(size_t)r * n + k] = (uint16_t)tours[(size_t)r * n + k];
        }
        for (uint32_t k = 0; k < lens[r]; ++k) {
            const uint32_t i = pairs[2 * ((size_t)r * kcap + k)], j = pairs[2 * ((size_t)r * kcap + k) + 1];
            if (!(i < j && j < n)) return fail(c, TL_ERR_BADARG, "tl_cs_selftest_reversals: row %u pair %u is not 0 <= i < j < n", r, k);
            packed[(size_t)r * kcap + k] = i | (j << 16);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t half = up256(cells * 2), pb = up256(pcells * 4), lb = up256((size_t)count * 4);
    if ((rc = ensure(c, c->work, 2 * half + pb + lb))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    HIPCHK(c, hipMemcpyAsync(w, h.data(), cells * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + half, packed.data(), pcells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + half + pb, lens, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + half + pb + lb, 0xFF, cells * 2, c->stream));
    HIPCHK(c, launch_cs_selftest_reversals((const uint16_t *)w, (const uint32_t *)(w + half), (const uint32_t *)(w + half + pb), n, kcap, count,
                                           (uint16_t *)(w + half + pb + lb), c->stream));
    HIPCHK(c, hipMemcpyAsync(h.data(), w + half + pb + lb, cells * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < cells; ++k) out[k] = h[k];
    return TL_OK;
}
