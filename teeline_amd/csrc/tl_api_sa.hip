// tl_api_sa.hip — C ABI, simulated annealing: tl_sim_anneal* (src/tsp/simulated_annealing.rs:10-83) over sim_anneal.hip, the host-only
// queries of its specification (tl_sa_draw, tl_sa_schedule_epochs, tl_sim_anneal_plan) and tl_sa_selftest_accept.
#include "sa_spec.h"
#include "tl_api_chains.h"

#pragma clang fp contract(off)

using namespace tl;
using namespace tlapi;

static constexpr uint64_t kSaMaxEpochs = 0xFFFFFFFFull;
static constexpr uint32_t kSaChunkDefault = 1u << 22;  // epochs per launch: the temperature table goes up in pieces of 16 MB

// The piece length of a schedule.  Tuning builds only (python -m teeline_amd.build --tune) read TL_SA_CHUNK (1 .. 2^22), so that tests
// reach the second piece with a short schedule: the product library never reads the environment.
static inline uint32_t sa_chunk()
{
#ifdef TL_TUNE
    if (const char *e = getenv("TL_SA_CHUNK")) {
        const long v = atol(e);
        if (v >= 1 && v <= (long)kSaChunkDefault) return (uint32_t)v;
    }
#endif
    return kSaChunkDefault;
}
static const tl_sa_opts kSaDefaults = {10000u, 1e-4f, 1e-3f, 1000.0f};  // mod.rs:598-608, 697-705

// SAOptions::validate (mod.rs:707-741): the first complaint, or nullptr
static const char *sa_validate(const tl_sa_opts &o)
{
    if (o.cooling_rate <= 0.0f) return "cooling_rate must be > 0";
    if (o.cooling_rate >= 1.0f) return "cooling_rate must be < 1";
    if (o.max_temperature <= 0.0f) return "max_temperature must be > 0";
    if (o.min_temperature < 0.0f) return "min_temperature must be >= 0";
    if (o.min_temperature >= o.max_temperature) return "min_temperature must be < max_temperature";
    return nullptr;
}

// cooling (probability.rs:30-32): two f32 roundings (this file is compiled without FMA contraction; volatile keeps the product a float)
static inline float sa_cool(float T, float rate)
{
    volatile float prod = rate * T;
    return T - prod;
}

// The length of the schedule `while epoch < epochs || temperature > min_temperature` (simulated_annealing.rs:41).  false: beyond
// 2^32 - 1 epochs, or T stops falling above min_temperature (the reference would loop for ever).
static bool sa_schedule(const tl_sa_opts &o, uint64_t *len)
{
    float T = o.max_temperature;
    uint64_t e = 0;
    while (e < o.epochs || T > o.min_temperature) {
        const float Tn = sa_cool(T, o.cooling_rate);
        if (e >= o.epochs && !(Tn < T)) return false;  // the temperature alone drives the loop and no longer falls
        T = Tn;
        if (++e > kSaMaxEpochs) return false;
    }
    *len = e;
    return true;
}

extern "C" uint64_t tl_sa_draw(uint64_t seed, uint32_t chain, uint32_t epoch, uint32_t slot) { return sa_draw_key(sa_chain_key(seed, chain), epoch, slot); }

extern "C" int tl_sa_schedule_epochs(const tl_sa_opts *opts, uint64_t *epochs)
{
    if (!epochs) return TL_ERR_BADARG;
    *epochs = 0;
    return sa_schedule(opts ? *opts : kSaDefaults, epochs) ? TL_OK : TL_ERR_UNSUPPORTED;
}

extern "C" uint32_t tl_sim_anneal_lds_max_n(const tl_ctx *c) { return c ? sim_anneal_lds_max_n(c->lds_bytes) : 0u; }

// A chain alone on its CU gets four waves (one per SIMD) and a window as wide; once there are more chains than CUs a chain is one
// wave, and a CU holds as many as its LDS and its 32 wave slots allow.  (Not measured yet against other widths: NOTEBOOK.md.)
extern "C" int tl_sim_anneal_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint32_t flags, uint32_t *window, int *threads, uint32_t *per_launch)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    const bool fits = n >= 1u && n <= sim_anneal_lds_max_n(lds_bytes);
    const int nt = !fits ? 0 : (flags & TL_FLAG_SA_NO_SPECULATION) || count > (uint32_t)cus ? 64 : 256;
    if (window) *window = !fits ? 0u : (flags & TL_FLAG_SA_NO_SPECULATION) ? 1u : (uint32_t)nt;
    if (threads) *threads = nt;
    if (per_launch) {
        const uint64_t per_cu = fits ? chains_per_cu(lds_bytes, sim_anneal_lds_bytes(n), nt) : 0u;
        *per_launch = (uint32_t)(per_cu * (uint32_t)cus);
    }
    return TL_OK;
}

// What the three entries share.  log: the accepted epochs of chain 0 of the call (a single chain's trace), else nullptr
static int sa_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                  uint32_t first_chain, uint32_t count, const tl_sa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                  uint32_t *best_index, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_chain, "chain")) return rc;
    if (count == 0) return TL_OK;
    const tl_sa_opts o = opts ? *opts : kSaDefaults;
    const bool empty = o.epochs == 0u && !(o.max_temperature > o.min_temperature);
    if (!empty)
        if (const char *msg = sa_validate(o)) return fail(c, TL_ERR_BADARG, "%s: %s", who, msg);
    uint64_t total = 0;
    if (!sa_schedule(o, &total))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: the schedule has more than 2^32 - 1 epochs (or never ends)", who);
    if (n < 2u && total) return fail(c, TL_ERR_REF_PANICS, "%s: n=%u: the reference panics (route.rs:87-89 random_pair, n_items < 2)", who, n);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    if (n < 2u) {  // (only with an empty schedule: the start tour, which a single city leaves no choice about)
        for (uint32_t r = 0; r < count; ++r) {
            if (n) out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
            if (out_moves) out_moves[r] = 0u;
        }
        return TL_OK;
    }
    if (n > sim_anneal_lds_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the LDS-resident limit %u (no HBM form)", who, n, sim_anneal_lds_max_n(c->lds_bytes));
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n))
            return fail(c, TL_ERR_BADARG, "%s: start tour %u is not a permutation of 0..n-1", who, r);
    uint32_t window = 0, per_launch = 0;
    int threads = 0;
    tl_sim_anneal_plan(n, count, c->cus, c->lds_bytes, c->flags, &window, &threads, &per_launch);
    if (per_launch == 0u) return fail(c, TL_ERR_UNSUPPORTED, "%s: no plan for this device", who);

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n, starts = init_count ? init_count : 1u;
    const uint32_t dev_log_cap = move_log ? log_cap : 0u;
    const uint32_t chunk = sa_chunk();
    const size_t table_cap = total < chunk ? (size_t)total : chunk;
    if ((rc = ensure(c, c->init, starts * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) || (rc = ensure(c, c->out_cost, (size_t)count * 4)) ||
        (rc = ensure(c, c->misc, (size_t)count * 16)) || (rc = ensure(c, c->work, up256((table_cap ? table_cap : 1u) * 4) + (size_t)(dev_log_cap ? dev_log_cap : 1u) * 16)))
        return rc;
    SaArgs A{};
    if ((rc = upload_instance_full(c, xy, dm_packed, n, &A.xy, &A.dm_full))) return rc;
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, (size_t)count * 16, c->stream));
    A.temps = (const float *)c->work.p;
    A.log = move_log ? (uint32_t *)((unsigned char *)c->work.p + up256((table_cap ? table_cap : 1u) * 4)) : nullptr;
    A.log_cap = dev_log_cap;
    A.seed = seed;
    A.n = n;
    A.window = window;
    if ((rc = upload_start_sync(c, init_count ? init_pos : nullptr, n, c->init.p, starts))) return rc;  // city order, one tour, or one per chain
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    std::vector<float> table(table_cap);
    uint64_t done = 0;
    bool first = true;
    float T = o.max_temperature;
    do {  // (an empty schedule is one launch of no epochs: the start tours and their lengths come back)
        const uint64_t end = total - done < chunk ? total : done + chunk;
        if (end > done) {  // the temperatures of [done, end), continued from where the last piece ended
            for (uint64_t e = done; e < end; ++e) {
                table[e - done] = T;
                T = sa_cool(T, o.cooling_rate);
            }
            HIPCHK(c, hipMemcpyAsync(c->work.p, table.data(), (size_t)(end - done) * 4, hipMemcpyHostToDevice, c->stream));
        }
        A.e_begin = (uint32_t)done;
        A.e_end = (uint32_t)end;
        for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {
            const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
            A.first_chain = first_chain + b0;
            if (first) {
                A.init_stride = init_count == count ? n : 0u;  // (0: every chain from the one tour uploaded)
                A.init = (const uint32_t *)c->init.p + (size_t)b0 * A.init_stride;
            } else {
                A.init_stride = n;
                A.init = (const uint32_t *)c->out_pos.p + (size_t)b0 * n;
            }
            A.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
            A.out_cost = (float *)c->out_cost.p + b0;
            A.out_run = (uint32_t *)c->misc.p + 4u * (size_t)b0;
            SaArgs L = A;
            if (b0) L.log = nullptr;  // the trace is chain 0's
            HIPCHK(c, launch_sim_anneal(L, cnt, threads, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the table's host copy is written again for the next piece
        done = end;
        first = false;
    } while (done < total);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> run;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 4u, out_pos, run, costs))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (move_log && dev_log_cap && run[0] && (rc = download_sync(c, move_log, A.log, (size_t)(run[0] < dev_log_cap ? run[0] : dev_log_cap) * 16))) return rc;
    if (log_len) *log_len = run[0];
    uint64_t moves = 0, reversed = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (out_costs) out_costs[r] = costs[r];
        if (out_moves) out_moves[r] = run[4u * r];
        moves += run[4u * r];
        reversed += (uint64_t)run[4u * r + 2u] << 32 | run[4u * r + 1u];
    }
    if (best_index) *best_index = best_chain(costs, count);
    if (stats) {
        stats->sweeps = stats->candidates = total * count;
        stats->moves = moves;
        stats->reversed = reversed;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_sim_anneal(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_sa_opts *opts, uint64_t seed,
                             uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return sa_run(c, "tl_sim_anneal", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats, nullptr, 0,
                  nullptr);
}

extern "C" int tl_sim_anneal_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_sa_opts *opts,
                                   uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    TL_ENTER(c);
    if (!move_log || !log_len) return fail(c, TL_ERR_BADARG, "tl_sim_anneal_trace: NULL argument");
    return sa_run(c, "tl_sim_anneal_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats,
                  move_log, log_cap, log_len);
}

extern "C" int tl_sim_anneal_trace_chain(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_sa_opts *opts,
                                         uint64_t seed, uint32_t chain, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap,
                                         uint32_t *log_len)
{
    TL_ENTER(c);
    if (!move_log || !log_len) return fail(c, TL_ERR_BADARG, "tl_sim_anneal_trace_chain: NULL argument");
    return sa_run(c, "tl_sim_anneal_trace_chain", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, chain, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr,
                  stats, move_log, log_cap, log_len);
}

extern "C" int tl_sim_anneal_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                        uint32_t first_chain, uint32_t count, const tl_sa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                        uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return sa_run(c, "tl_sim_anneal_population", xy, n, dm_packed, init_pos, init_count, first_chain, count, opts, seed, out_pos, out_costs, out_moves,
                  best_index, stats, nullptr, 0, nullptr);
}

extern "C" int tl_sa_selftest_accept(tl_ctx *c, const float *T, const float *old_cost, const float *new_cost, const float *p, uint32_t count,
                                     uint32_t *out_accept, float *out_criteria)
{
    TL_ENTER(c);
    if (!c || !T || !old_cost || !new_cost || !p || !out_accept || !out_criteria) return fail(c, TL_ERR_BADARG, "tl_sa_selftest_accept: NULL argument");
    if (count == 0) return TL_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t b = (size_t)count * 4;
    if ((rc = ensure(c, c->work, 6 * up256(b)))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    const float *src[4] = {T, old_cost, new_cost, p};
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(w + k * up256(b), src[k], b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_sa_selftest((const float *)w, (const float *)(w + up256(b)), (const float *)(w + 2 * up256(b)), (const float *)(w + 3 * up256(b)), count,
                                 (uint32_t *)(w + 4 * up256(b)), (float *)(w + 5 * up256(b)), c->stream));
    HIPCHK(c, hipMemcpyAsync(out_accept, w + 4 * up256(b), b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_criteria, w + 5 * up256(b), b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}
