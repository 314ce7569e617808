// tl_api_gsa.hip — C ABI, the gravitational search solver: tl_gravitational_search* (src/tsp/gravitational_search.rs:23-145) over
// gravitational_search.hip, the host-only queries of its specification (tl_gsa_draw, tl_gsa_g, tl_gsa_pull_swaps, tl_gsa_masses,
// tl_gravitational_search_plan) and the device self-test of one pull.
//
// n = 0 and n = 1: the reference does not panic (every cost is 0, the masses are uniform, every swap sequence is empty and 0 < 0
// fails), so the entries return the empty route or the one city at cost 0, a log of the start gbest alone and epoch rows that hold
// each agent's live pulls with nothing applied — on the host, without a launch.
#include "gsa_spec.h"
#include "tl_api_swarm.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kGsaSpanEpochs = 4096u;  // epochs of one launch where the options name no span, so that no launch runs without end

// one run's share of the workspace: the positions (N n u16), gbest, the costs, the masses, the ranking
static uint64_t gsa_run_bytes(uint32_t n, uint32_t N) { return 2ull * N * n + 2ull * n + 14ull * N; }

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

namespace {
// what gravitational search adds to the frame of tl_api_swarm.h
struct GsaSolver {
    using Args = GsaArgs;
    static constexpr const char *kMembers = "agents";
    static constexpr uint64_t kLayoutSlack = 8 * 256;  // the arrays of a sequence each start on a 256-byte boundary
    const tl_gsa_opts *opts;
    uint32_t epochs = 0, N = 0;
    size_t tab = 0, gb = 0, row4 = 0, row8 = 0, row2 = 0;

    int check(const SwarmCall &k)
    {
        epochs = opts ? opts->epochs : 10000u;  // HeuristicOptions::default (mod.rs:604-611)
        const uint32_t n_nearest = opts ? opts->n_nearest : 3u;
        N = gsa_agents(n_nearest);
        return check_swarm_sizes(k, epochs, n_nearest, N, kGsaMaxAgents, kMembers, gravitational_search_max_n(k.c->lds_bytes), "8");
    }
    uint32_t row_words() const { return 3u * N + 2u; }
    uint64_t log_rows() const { return 1ull + (uint64_t)epochs * N; }  // the start gbest and at most one improvement per move
    uint64_t run_bytes(uint32_t n) const { return gsa_run_bytes(n, N); }
    // every cost is 0 and the masses are uniform: G and each agent's live pulls, with nothing applied
    void host_epoch_rows(const SwarmCall &k, uint32_t *epoch_log, uint32_t rows) const
    {
        const uint64_t key = sa_chain_key(k.seed, k.first_run);
        const uint32_t kb = gsa_kbest(N);
        const double mass = 1.0 / (double)N;  // kbest is 0 .. kb - 1
        for (uint32_t e = 0; e < rows; ++e) {
            uint32_t *erow = epoch_log + (size_t)e * row_words();
            const double g = gsa_g(e, epochs);
            const uint64_t gbits = __builtin_bit_cast(uint64_t, g);
            erow[3u * N] = (uint32_t)gbits;
            erow[3u * N + 1u] = (uint32_t)(gbits >> 32);
            for (uint32_t i = 0; i < N; ++i)
                for (uint32_t j = 0; j < kb; ++j)
                    if (j != i && gsa_pull_swaps(gsa_r(key, e, N, i, j), g, mass)) ++erow[2u * N + i];
        }
    }
    size_t layout(uint32_t n, uint32_t held)
    {
        tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), row4 = up256((size_t)held * N * 4);
        row8 = up256((size_t)held * N * 8), row2 = up256((size_t)held * N * 2);
        return tab + gb + row4 + row8 + row2;
    }
    void carve(Args &A, unsigned char *w, uint32_t n) const
    {
        A.mass = (double *)w;
        A.pos = (uint16_t *)(w + row8);
        A.gbest = (uint16_t *)(w + row8 + tab);
        w += row8 + tab + gb;
        A.cost = (float *)w;
        A.kbest = (uint16_t *)(w + row4);
        A.agents = N;
        A.vmax = pso_vmax(n);
        A.epochs = epochs;
    }
    hipError_t enqueue(tl_ctx *c, Args &L, uint32_t cnt) const
    {
        const uint32_t span = opts && opts->span_epochs ? opts->span_epochs : kGsaSpanEpochs;
        L.last = epochs == 0u;
        hipError_t e = launch_gsa_init(L, cnt, c->stream);
        for (uint32_t ep = 0; ep < epochs && e == hipSuccess; ep = L.e1) {
            L.e0 = ep;
            L.e1 = epochs - ep > span ? ep + span : epochs;
            L.last = L.e1 == epochs;
            e = launch_gsa_epochs(L, cnt, c->stream);
        }
        return e;
    }
    int verdict(const SwarmCall &k, const std::vector<uint32_t> &state) const
    {
        for (uint32_t r = 0; r < k.count; ++r)
            if (state[8u * r + 2u])
                return fail(k.c, TL_ERR_REF_PANICS, "%s: run %u: a cost or a mass is NaN — the reference panics on partial_cmp(..).unwrap()", k.who,
                            k.first_run + r);
        return TL_OK;
    }
};
}  // namespace

extern "C" int tl_gravitational_search_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                            uint32_t *agents, int *threads, uint32_t *per_launch)
{
    (void)count;
    // (the epochs' workgroup is 256 lanes whatever n: the ranking and the pulls are spread over the agents)
    return swarm_plan(n, gsa_agents(n_nearest), kGsaMaxAgents, gravitational_search_max_n, [](uint32_t) { return 256; }, gsa_run_bytes, GsaSolver::kLayoutSlack,
                      cus, lds_bytes, workspace_bytes, flags, agents, threads, per_launch);
}

extern "C" int tl_gravitational_search(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_gsa_opts *opts, uint64_t seed,
                           uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_gravitational_search", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, seed, out_pos, out_cost, stats}, GsaSolver{opts}, {});
}

extern "C" int tl_gravitational_search_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_gsa_opts *opts, uint64_t seed,
                                 uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len,
                                 uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_gravitational_search_trace: NULL argument");
    return swarm4_run({c, "tl_gravitational_search_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, seed, out_pos, out_cost, stats}, GsaSolver{opts},
                      {log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap});
}

extern "C" int tl_gravitational_search_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                      uint32_t first_run, uint32_t count, const tl_gsa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                      uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_gravitational_search_population", xy, n, dm_packed, init_pos, init_count, first_run, count, seed, out_pos, out_costs, stats, out_moves, best_index},
                      GsaSolver{opts}, {});
}

extern "C" int tl_gsa_selftest_pull(tl_ctx *c, const uint32_t *from, const uint32_t *target, const uint32_t *prefix, uint32_t n, uint32_t count,
                                    uint32_t *out_pairs, uint32_t *out_len)
{
    TL_ENTER(c);
    if (!c || !from || !target || !prefix || !out_pairs || !out_len) return fail(c, TL_ERR_BADARG, "tl_gsa_selftest_pull: NULL argument");
    if (n < 1u || n > gravitational_search_max_n(c->lds_bytes) || count < 1u || count > kSwarmMaxRuns)
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
