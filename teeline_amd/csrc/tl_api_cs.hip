// tl_api_cs.hip — C ABI, the cuckoo search solver: tl_cuckoo_search* (src/tsp/cuckoo_search.rs:26-136) over cuckoo_search.hip, the
// host-only queries of its specification (tl_cs_draw, tl_levy_from_words, tl_cs_flight_length, tl_cs_pa, tl_cuckoo_search_plan)
// and the device self-tests of the Lévy step and of the reversals' gather.
#include "cs_spec.h"
#include "tl_api_swarm.h"

using namespace tl;
using namespace tlapi;

// one run's share of the workspace: nests, staged flights and staged replacements (N n u16 each), best, four rows of N words
static uint64_t cs_run_bytes(uint32_t n, uint32_t N) { return 6ull * N * n + 2ull * n + 16ull * N; }

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

namespace {
// what cuckoo search adds to the frame of tl_api_swarm.h
struct CsSolver {
    using Args = CsArgs;
    static constexpr const char *kMembers = "nests";
    static constexpr uint64_t kLayoutSlack = 11 * 256;  // the arrays of a sequence each start on a 256-byte boundary
    const tl_cs_opts *opts;
    uint32_t epochs = 0, N = 0;
    double pa = 0.0;
    size_t tab = 0, gb = 0, row = 0;

    int check(const SwarmCall &k)
    {
        // CSOptions::default (mod.rs:918-925) over HeuristicOptions::default (mod.rs:604-611)
        epochs = opts ? opts->epochs : 10000u;
        const uint32_t n_nearest = opts ? opts->n_nearest : 3u;
        const float p_mut = opts ? opts->mutation_probability : 0.001f;
        N = cs_nests(n_nearest);
        pa = cs_pa(p_mut);
        if (!(p_mut >= 0.0f && p_mut <= 1.0f)) return fail(k.c, TL_ERR_BADARG, "%s: mutation_probability must be in [0, 1] (got %g)", k.who, (double)p_mut);
        if (int rc = check_swarm_sizes(k, epochs, n_nearest, N, kCsMaxNests, kMembers, cuckoo_search_max_n(k.c->lds_bytes), "10")) return rc;
        if (!cs_events_fit(epochs, N, k.n)) return fail(k.c, TL_ERR_UNSUPPORTED, "%s: epochs x nests x (n + 1) exceeds 2^58 events", k.who);
        if (k.n <= 1u && epochs >= 1u)
            return fail(k.c, TL_ERR_REF_PANICS, "%s: n=%u: the reference panics (cuckoo_search.rs:85 clamp(1, n / 2) with min > max)", k.who, k.n);
        return TL_OK;
    }
    uint32_t row_words() const { return 4u * N; }
    uint64_t log_rows() const { return 1ull + 2ull * epochs * N; }  // the start best, at most one improvement per flight and per abandonment
    uint64_t run_bytes(uint32_t n) const { return cs_run_bytes(n, N); }
    void host_epoch_rows(const SwarmCall &, uint32_t *, uint32_t) const {}  // (n <= 1 is answered for epochs = 0 only: no row)
    size_t layout(uint32_t n, uint32_t held)
    {
        tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), row = up256((size_t)held * N * 4);
        return 3 * tab + gb + 4 * row;
    }
    void carve(Args &A, unsigned char *w, uint32_t) const
    {
        A.nest = (uint16_t *)w;
        A.fly = (uint16_t *)(w + tab);
        A.repl = (uint16_t *)(w + 2 * tab);
        A.best = (uint16_t *)(w + 3 * tab);
        w += 3 * tab + gb;
        A.cost = (float *)w;
        A.fcost = (float *)(w + row);
        A.rcost = (float *)(w + 2 * row);
        A.fk = (uint32_t *)(w + 3 * row);
        A.pa = pa;
        A.nests = N;
    }
    hipError_t enqueue(tl_ctx *c, Args &L, uint32_t cnt) const
    {
        L.last = epochs == 0u;
        hipError_t e = launch_cs_init(L, cnt, c->stream);
        for (uint32_t ep = 0; ep < epochs && e == hipSuccess; ++ep) {
            L.epoch = ep;
            L.last = ep + 1u == epochs;
            if ((e = launch_cs_fly(L, cnt, c->stream)) == hipSuccess) e = launch_cs_commit(L, cnt, c->stream);
        }
        return e;
    }
    int verdict(const SwarmCall &, const std::vector<uint32_t> &) const { return TL_OK; }
};
}  // namespace

extern "C" int tl_cuckoo_search_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                     uint32_t *nests, int *threads, uint32_t *per_launch)
{
    (void)count;
    return swarm_plan(n, cs_nests(n_nearest), kCsMaxNests, cuckoo_search_max_n, cuckoo_search_threads, cs_run_bytes, CsSolver::kLayoutSlack, cus, lds_bytes,
                      workspace_bytes, flags, nests, threads, per_launch);
}

extern "C" int tl_cuckoo_search(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_cs_opts *opts, uint64_t seed,
                    uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_cuckoo_search", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, seed, out_pos, out_cost, stats}, CsSolver{opts}, {});
}

extern "C" int tl_cuckoo_search_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_cs_opts *opts, uint64_t seed,
                          uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len,
                          uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_cuckoo_search_trace: NULL argument");
    return swarm4_run({c, "tl_cuckoo_search_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, seed, out_pos, out_cost, stats}, CsSolver{opts},
                      {log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap});
}

extern "C" int tl_cuckoo_search_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                               uint32_t first_run, uint32_t count, const tl_cs_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                               uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_cuckoo_search_population", xy, n, dm_packed, init_pos, init_count, first_run, count, seed, out_pos, out_costs, stats, out_moves, best_index},
                      CsSolver{opts}, {});
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
    if (n < 2u || n > cuckoo_search_max_n(c->lds_bytes) || count < 1u || count > kSwarmMaxRuns || kcap < 1u || kcap > n / 2u)
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
