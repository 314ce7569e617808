// tl_api_pso.hip — C ABI, the particle swarm solver: tl_particle_swarm* (src/tsp/particle_swarm.rs:22-129) over particle_swarm.hip,
// the host-only queries of its specification (tl_pso_draw, tl_pso_weight, tl_pso_keep, tl_particle_swarm_plan) and the device
// self-test of the swap sequence.
#include "pso_spec.h"
#include "tl_api_swarm.h"

using namespace tl;
using namespace tlapi;

// one run's share of the workspace: two position tables and pbest (P n u16), gbest, two velocity tables (P vmax words), two length
// rows, cost and pbest_cost (P words each)
static uint64_t pso_run_bytes(uint32_t n, uint32_t P) { return 6ull * P * n + 2ull * n + 8ull * P * pso_vmax(n) + 16ull * P; }

extern "C" uint64_t tl_pso_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" double tl_pso_weight(uint32_t epoch, uint32_t epochs) { return pso_weight(epoch, epochs); }

extern "C" uint32_t tl_pso_keep(double x) { return pso_keep(x); }

extern "C" uint32_t tl_particle_swarm_max_n(const tl_ctx *c) { return c ? particle_swarm_max_n(c->lds_bytes) : 0u; }

namespace {
// what the particle swarm adds to the frame of tl_api_swarm.h
struct PsoSolver {
    using Args = PsoArgs;
    static constexpr const char *kMembers = "particles";
    static constexpr uint64_t kLayoutSlack = 10 * 256;  // the ten arrays of a sequence each start on a 256-byte boundary
    const tl_pso_opts *opts;
    uint32_t epochs = 0, N = 0;
    size_t tab = 0, gb = 0, vt = 0, row = 0;

    int check(const SwarmCall &k)
    {
        epochs = opts ? opts->epochs : 10000u;  // HeuristicOptions::default (mod.rs:604-611)
        const uint32_t n_nearest = opts ? opts->n_nearest : 3u;
        N = pso_particles(n_nearest);
        return check_swarm_sizes(k, epochs, n_nearest, N, kPsoMaxParticles, kMembers, particle_swarm_max_n(k.c->lds_bytes), "15.4");
    }
    uint32_t row_words() const { return 2u * N; }
    uint64_t log_rows() const { return 1ull + (uint64_t)epochs * N; }  // the start gbest and at most one improvement per particle step
    uint64_t run_bytes(uint32_t n) const { return pso_run_bytes(n, N); }
    void host_epoch_rows(const SwarmCall &, uint32_t *, uint32_t) const {}  // (no draw that matters: every word is 0)
    size_t layout(uint32_t n, uint32_t held)
    {
        tab = up256((size_t)held * N * n * 2), gb = up256((size_t)held * n * 2), vt = up256((size_t)held * N * pso_vmax(n) * 4), row = up256((size_t)held * N * 4);
        return 3 * tab + gb + 2 * vt + 4 * row;
    }
    void carve(Args &A, unsigned char *w, uint32_t n) const
    {
        A.pos[0] = (uint16_t *)w;
        A.pos[1] = (uint16_t *)(w + tab);
        A.pbest = (uint16_t *)(w + 2 * tab);
        A.gbest = (uint16_t *)(w + 3 * tab);
        w += 3 * tab + gb;
        A.vel[0] = (uint32_t *)w;
        A.vel[1] = (uint32_t *)(w + vt);
        w += 2 * vt;
        A.vlen[0] = (uint32_t *)w;
        A.vlen[1] = (uint32_t *)(w + row);
        A.cost = (float *)(w + 2 * row);
        A.pcost = (float *)(w + 3 * row);
        A.particles = N;
        A.vmax = pso_vmax(n);
        A.epochs = epochs;
    }
    hipError_t enqueue(tl_ctx *c, Args &L, uint32_t cnt) const
    {
        L.last = epochs == 0u;
        hipError_t e = launch_pso_init(L, cnt, c->stream);
        for (uint32_t ep = 0; ep < epochs && e == hipSuccess; ++ep) {
            L.epoch = ep;
            L.last = ep + 1u == epochs;
            if ((e = launch_pso_move(L, cnt, c->stream)) == hipSuccess) e = launch_pso_commit(L, cnt, c->stream);
            L.src ^= 1u;
        }
        return e;
    }
    int verdict(const SwarmCall &, const std::vector<uint32_t> &) const { return TL_OK; }
};
}  // namespace

extern "C" int tl_particle_swarm_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                      uint32_t *particles, int *threads, uint32_t *per_launch)
{
    (void)count;
    return swarm_plan(n, pso_particles(n_nearest), kPsoMaxParticles, particle_swarm_max_n, particle_swarm_threads, pso_run_bytes, PsoSolver::kLayoutSlack, cus,
                      lds_bytes, workspace_bytes, flags, particles, threads, per_launch);
}

extern "C" int tl_particle_swarm(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_pso_opts *opts, uint64_t seed,
                     uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_particle_swarm", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, seed, out_pos, out_cost, stats}, PsoSolver{opts}, {});
}

extern "C" int tl_particle_swarm_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_pso_opts *opts, uint64_t seed,
                           uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len,
                           uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_particle_swarm_trace: NULL argument");
    return swarm4_run({c, "tl_particle_swarm_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, seed, out_pos, out_cost, stats}, PsoSolver{opts},
                      {log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap});
}

extern "C" int tl_particle_swarm_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                uint32_t first_run, uint32_t count, const tl_pso_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm4_run({c, "tl_particle_swarm_population", xy, n, dm_packed, init_pos, init_count, first_run, count, seed, out_pos, out_costs, stats, out_moves, best_index},
                      PsoSolver{opts}, {});
}

extern "C" int tl_pso_selftest_swap_sequence(tl_ctx *c, const uint32_t *from, const uint32_t *to, uint32_t n, uint32_t count, uint32_t *out_pairs,
                                             uint32_t *out_len)
{
    TL_ENTER(c);
    if (!c || !from || !to || !out_pairs || !out_len) return fail(c, TL_ERR_BADARG, "tl_pso_selftest_swap_sequence: NULL argument");
    if (n < 1u || n > particle_swarm_max_n(c->lds_bytes) || count < 1u || count > kSwarmMaxRuns)
        return fail(c, TL_ERR_BADARG, "tl_pso_selftest_swap_sequence: n or count out of range");
    for (uint32_t r = 0; r < count; ++r)
        if (!is_permutation(from + (size_t)r * n, n) || !is_permutation(to + (size_t)r * n, n))
            return fail(c, TL_ERR_BADARG, "tl_pso_selftest_swap_sequence: pair %u holds a row that is not a permutation of 0..n-1", r);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t cells = (size_t)count * n, half = up256(cells * 2), full = up256(cells * 4), lens = up256((size_t)count * 4);
    if ((rc = ensure(c, c->work, 2 * half + full + lens))) return rc;
    std::vector<uint16_t> h(2 * cells);
    for (size_t k = 0; k < cells; ++k) {
        h[k] = (uint16_t)from[k];
        h[cells + k] = (uint16_t)to[k];
    }
    std::vector<uint32_t> pairs(cells), len(count);
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    HIPCHK(c, hipMemcpyAsync(w, h.data(), cells * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + half, h.data() + cells, cells * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + 2 * half, 0xFF, cells * 4, c->stream));
    HIPCHK(c, launch_pso_selftest_swap_sequence((const uint16_t *)w, (const uint16_t *)(w + half), n, count, (uint32_t *)(w + 2 * half),
                                                (uint32_t *)(w + 2 * half + full), c->stream));
    HIPCHK(c, hipMemcpyAsync(pairs.data(), w + 2 * half, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(len.data(), w + 2 * half + full, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t r = 0; r < count; ++r) {
        out_len[r] = len[r];
        for (uint32_t k = 0; k < n; ++k) {  // rows of n pairs: (i, j) up to the length, 0xFFFFFFFF beyond
            const uint32_t s = pairs[(size_t)r * n + k];
            const bool live = k < len[r];
            out_pairs[2 * ((size_t)r * n + k)] = live ? s & 0xFFFFu : 0xFFFFFFFFu;
            out_pairs[2 * ((size_t)r * n + k) + 1] = live ? s >> 16 : 0xFFFFFFFFu;
        }
    }
    return TL_OK;
}
