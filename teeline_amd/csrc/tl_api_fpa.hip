// tl_api_fpa.hip — C ABI, the flower pollination solver: tl_flower_pollination* (src/tsp/flower_pollination.rs:53-151) over
// flower_pollination.hip, the host-only queries of its specification (tl_fpa_draw, tl_fpa_switch_prob, tl_fpa_global_swaps,
// tl_fpa_local_swaps, tl_fpa_partners, tl_flower_pollination_plan) and the device self-test of one move.
//
// n = 0 and n = 1: the reference does not panic (swap_sequence's saturating_sub gives an empty sequence, every flower comes back
// unchanged at cost 0 and 0 < 0 fails), so the entries return the empty route or the one city at cost 0, a log of the start gbest
// alone and epoch rows that hold each flower's draws with nothing accepted — on the host, without a launch.
#include "fpa_spec.h"
#include "tl_api_swarm.h"

using namespace tl;
using namespace tlapi;

// one run's share of the workspace: flowers and staged moves (N n u16 each), gbest, three rows of N words
static uint64_t fpa_run_bytes(uint32_t n, uint32_t N) { return 4ull * N * n + 2ull * n + 12ull * N; }

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

namespace {
// what flower pollination adds to the frame of tl_api_swarm.h
struct FpaSolver {
    using Args = FpaArgs;
    static constexpr const char *kMembers = "flowers";
    static constexpr uint64_t kLayoutSlack = 9 * 256;  // the arrays of a sequence each start on a 256-byte boundary
    const tl_fpa_opts *opts;
    uint32_t epochs = 0, N = 0;
    double switch_prob = 0.0;
    size_t tab = 0, gb = 0, row = 0;

    int check(const SwarmCall &k)
    {
        // FPAOptions::default (mod.rs:1003-1010) over HeuristicOptions::default (mod.rs:604-611)
        epochs = opts ? opts->epochs : 10000u;
        const uint32_t n_nearest = opts ? opts->n_nearest : 3u;
        const float p_mut = opts ? opts->mutation_probability : 0.001f;
        N = fpa_flowers(n_nearest);
        switch_prob = fpa_switch_prob(p_mut);
        if (!(p_mut >= 0.0f && p_mut <= 1.0f)) return fail(k.c, TL_ERR_BADARG, "%s: mutation_probability must be in [0, 1] (got %g)", k.who, (double)p_mut);
        return check_swarm_sizes(k, epochs, n_nearest, N, kFpaMaxFlowers, kMembers, flower_pollination_max_n(k.c->lds_bytes), "10");
    }
    uint32_t row_words() const { return 4u * N; }
    uint64_t log_rows() const { return 1ull + (uint64_t)epochs * N; }  // the start gbest and at most one improvement per move
    uint64_t run_bytes(uint32_t n) const { return fpa_run_bytes(n, N); }
    // every flower's draws, with nothing accepted
    void host_epoch_rows(const SwarmCall &k, uint32_t *epoch_log, uint32_t rows) const
    {
        const uint64_t key = sa_chain_key(k.seed, k.first_run);
        for (uint32_t e = 0; e < rows; ++e)
            for (uint32_t i = 0; i < N; ++i) {
                uint32_t j, kk;
                fpa_partners(key, fpa_event(e, N, i), i, N, &j, &kk);
                epoch_log[(size_t)e * 4 * N + N + i] = fpa_kind_word(fpa_is_global(key, fpa_event(e, N, i), switch_prob), j, kk);
            }
    }
    size_t layout(uint32_t n, uint32_t held)
    {
        tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), row = up256((size_t)held * N * 4);
        return 2 * tab + gb + 3 * row;
    }
    void carve(Args &A, unsigned char *w, uint32_t) const
    {
        A.flower = (uint16_t *)w;
        A.stage = (uint16_t *)(w + tab);
        A.gbest = (uint16_t *)(w + 2 * tab);
        w += 2 * tab + gb;
        A.cost = (float *)w;
        A.scost = (float *)(w + row);
        A.slen = (uint32_t *)(w + 2 * row);
        A.switch_prob = switch_prob;
        A.flowers = N;
    }
    hipError_t enqueue(tl_ctx *c, Args &L, uint32_t cnt) const
    {
        L.last = epochs == 0u;
        hipError_t e = launch_fpa_init(L, cnt, c->stream);
        for (uint32_t ep = 0; ep < epochs && e == hipSuccess; ++ep) {
            L.epoch = ep;
            L.last = ep + 1u == epochs;
            if ((e = launch_fpa_move(L, cnt, c->stream)) == hipSuccess) e = launch_fpa_commit(L, cnt, c->stream);
        }
        return e;
    }
    int verdict(const SwarmCall &, const std::vector<uint32_t> &) const { return TL_OK; }
};
}  // namespace

extern "C" int tl_flower_pollination_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                          uint32_t *flowers, int *threads, uint32_t *per_launch)
{
    (void)count;
    return swarm_plan(n, fpa_flowers(n_nearest), kFpaMaxFlowers, flower_pollination_max_n, flower_pollination_threads, fpa_run_bytes, FpaSolver::kLayoutSlack, cus,
                      lds_bytes, workspace_bytes, flags, flowers, threads, per_launch);
}

extern "C" int tl_flower_pollination(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_fpa_opts *opts,
                                     uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_flower_pollination", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, seed, out_pos, out_cost, stats}, FpaSolver{opts}, {});
}

extern "C" int tl_flower_pollination_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_fpa_opts *opts,
                                           uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                           uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_flower_pollination_trace: NULL argument");
    return swarm4_run({c, "tl_flower_pollination_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, seed, out_pos, out_cost, stats}, FpaSolver{opts},
                      {log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap});
}

extern "C" int tl_flower_pollination_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                                uint32_t first_run, uint32_t count, const tl_fpa_opts *opts, uint64_t seed, uint32_t *out_pos,
                                                float *out_costs, uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_flower_pollination_population", xy, n, dm_packed, init_pos, init_count, first_run, count, seed, out_pos, out_costs, stats, out_moves,
                       best_index},
                      FpaSolver{opts}, {});
}

extern "C" int tl_fpa_selftest_pollinate(tl_ctx *c, const uint32_t *flower, const uint32_t *source, const uint32_t *target, const uint32_t *prefix, uint32_t n,
                                         uint32_t count, uint32_t *out, uint32_t *out_len)
{
    TL_ENTER(c);
    if (!c || !flower || !source || !target || !prefix || !out || !out_len) return fail(c, TL_ERR_BADARG, "tl_fpa_selftest_pollinate: NULL argument");
    if (n < 1u || n > flower_pollination_max_n(c->lds_bytes) || count < 1u || count > kSwarmMaxRuns)
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
