// tl_api_pso.hip — C ABI, the particle swarm solver: tl_particle_swarm* (src/tsp/particle_swarm.rs:22-129) over particle_swarm.hip,
// the host-only queries of its specification (tl_pso_draw, tl_pso_weight, tl_pso_keep, tl_particle_swarm_plan) and the device
// self-test of the swap sequence.
#include "pso_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kPsoUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kPsoWorkDefault = 8ull << 30;    // the swarms of one launch sequence
static constexpr uint32_t kPsoMaxRuns = 65535u;            // the run is the grid's y
static constexpr uint64_t kPsoLayoutSlack = 10 * 256;      // the ten arrays of a sequence each start on a 256-byte boundary

// one run's share of the workspace: two position tables and pbest (P n u16), gbest, two velocity tables (P vmax words), two length
// rows, cost and pbest_cost (P words each)
static inline uint64_t pso_run_bytes(uint32_t n, uint32_t P) { return 6ull * P * n + 2ull * n + 8ull * P * pso_vmax(n) + 16ull * P; }

extern "C" uint64_t tl_pso_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" double tl_pso_weight(uint32_t epoch, uint32_t epochs) { return pso_weight(epoch, epochs); }

extern "C" uint32_t tl_pso_keep(double x) { return pso_keep(x); }

extern "C" uint32_t tl_particle_swarm_max_n(const tl_ctx *c) { return c ? particle_swarm_max_n(c->lds_bytes) : 0u; }

extern "C" int tl_particle_swarm_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                      uint32_t *particles, int *threads, uint32_t *per_launch)
{
    if (particles) *particles = 0u;
    if (threads) *threads = 0;
    if (per_launch) *per_launch = 0u;
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (flags & kPsoUnassignedFlags) return TL_ERR_UNSUPPORTED;
    const uint32_t P = pso_particles(n_nearest);
    if (n < 2u || n > particle_swarm_max_n(lds_bytes) || P > kPsoMaxParticles) return TL_OK;
    uint64_t per = workspace_bytes > kPsoLayoutSlack ? (workspace_bytes - kPsoLayoutSlack) / pso_run_bytes(n, P) : 0u;
    if (per > kPsoMaxRuns) per = kPsoMaxRuns;
    (void)count;
    if (per == 0u) return TL_OK;
    if (particles) *particles = P;
    if (threads) *threads = particle_swarm_threads(n);
    if (per_launch) *per_launch = (uint32_t)per;
    return TL_OK;
}

// What the entries share.  log / route_log / epoch_log: run 0 of the call (a single run's trace), else nullptr
static int pso_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                   uint32_t first_run, uint32_t count, const tl_pso_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *out_moves,
                   uint32_t *best_index, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap,
                   uint32_t *epoch_log, uint32_t epoch_cap)
{
    if (log_len) *log_len = 0;
    if (int rc = check_chain_call(c, who, xy, dm_packed, count, out_pos, init_pos, init_count, first_run, "run")) return rc;
    if (count == 0) return TL_OK;
    if (c->flags & kPsoUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    const uint32_t epochs = opts ? opts->epochs : 10000u, n_nearest = opts ? opts->n_nearest : 3u;  // HeuristicOptions::default (mod.rs:604-611)
    const uint32_t P = pso_particles(n_nearest);
    if (epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 2^32 - 1 is not supported", who);
    if (P > kPsoMaxParticles) return fail(c, TL_ERR_UNSUPPORTED, "%s: n_nearest=%u: more than %u particles", who, n_nearest, kPsoMaxParticles);
    if (n > particle_swarm_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (15.4 bytes of LDS per city)", who, n, particle_swarm_max_n(c->lds_bytes));
    for (uint32_t r = 0; r < init_count; ++r)
        if (!is_permutation(init_pos + (size_t)r * n, n)) return fail(c, TL_ERR_BADARG, "%s: the initial tour is not a permutation of 0..n-1", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    if (n <= 1u) {  // no edge, no draw that matters, no device: every position is the one route (or the empty one) at cost 0
        for (uint32_t r = 0; r < count; ++r) {
            if (n) out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
            if (out_moves) out_moves[r] = 0u;
        }
        if (log && log_cap) {  // record 0: the start gbest, particle 0 (all are equal)
            log[0] = 0xFFFFFFFFu;
            log[1] = log[2] = 0u;
            log[3] = route_log && route_cap ? 0u : 0xFFFFFFFFu;
        }
        if (route_log && route_cap && n) route_log[0] = 0u;
        if (epoch_log) memset(epoch_log, 0, (size_t)(epoch_cap < epochs ? epoch_cap : epochs) * 2 * P * 4);
        if (log_len) *log_len = 1u;
        c->ev_valid = false;
        if (stats) {
            stats->sweeps = (uint64_t)epochs * count;
            stats->candidates = (uint64_t)epochs * count * P;
            stamp_times(c, stats, t0);
        }
        return TL_OK;
    }
    uint32_t per_launch = 0;
    tl_particle_swarm_plan(n, n_nearest, count, c->cus, c->lds_bytes, kPsoWorkDefault, 0u, nullptr, nullptr, &per_launch);
    if (per_launch == 0u)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u, %u particles: one run's tables (%llu bytes) exceed the workspace limit", who, n, P,
                    (unsigned long long)pso_run_bytes(n, P));

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t words = (size_t)count * n;
    const uint32_t held = count < per_launch ? count : per_launch;  // runs whose swarms exist at once
    const uint32_t vmax = pso_vmax(n);
    const uint64_t most = 1ull + (uint64_t)epochs * P;               // the start gbest and at most one improvement per particle step
    const uint32_t dev_log_cap = log ? (uint32_t)(log_cap < most ? log_cap : most) : 0u;
    const uint32_t dev_route_cap = route_log ? (uint32_t)(route_cap < most ? route_cap : most) : 0u;
    const uint32_t dev_epoch_cap = epoch_log ? (epoch_cap < epochs ? epoch_cap : epochs) : 0u;
    const size_t log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 16);
    const size_t route_bytes = up256((size_t)(dev_route_cap ? dev_route_cap : 1u) * n * 4);
    const size_t epoch_bytes = up256((size_t)(dev_epoch_cap ? dev_epoch_cap : 1u) * 2 * P * 4);
    const size_t tab = up256((size_t)held * P * n * 2), gb = up256((size_t)held * n * 2), vt = up256((size_t)held * P * vmax * 4), row = up256((size_t)held * P * 4);
    if ((rc = ensure(c, c->init, (size_t)(init_count ? init_count : 1u) * n * 4)) || (rc = ensure(c, c->out_pos, words * 4)) ||
        (rc = ensure(c, c->out_cost, (size_t)count * 4)) || (rc = ensure(c, c->misc, (size_t)count * 32)) ||
        (rc = ensure(c, c->work, log_bytes + route_bytes + epoch_bytes + 3 * tab + gb + 2 * vt + 4 * row)))
        return rc;
    PsoArgs A{};
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
    A.seed = seed;
    A.n = n;
    A.particles = P;
    A.vmax = vmax;
    A.epochs = epochs;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the tables
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        PsoArgs L = A;
        L.first_run = first_run + b0;
        if (L.init && L.init_stride) L.init += (size_t)b0 * n;
        L.out_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        L.out_cost = (float *)c->out_cost.p + b0;
        L.state = (uint32_t *)c->misc.p + 8u * (size_t)b0;
        if (b0) L.log = L.route_log = L.epoch_log = nullptr;  // the trace is run 0's
        L.last = epochs == 0u;
        HIPCHK(c, launch_pso_init(L, cnt, c->stream));
        for (uint32_t e = 0; e < epochs; ++e) {
            L.epoch = e;
            L.last = e + 1u == epochs;
            HIPCHK(c, launch_pso_move(L, cnt, c->stream));
            HIPCHK(c, launch_pso_commit(L, cnt, c->stream));
            L.src ^= 1u;
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> state;
    std::vector<float> costs;
    if ((rc = download_chains(c, count, n, 8u, out_pos, state, costs))) return rc;
    if (dev_epoch_cap) HIPCHK(c, hipMemcpyAsync(epoch_log, A.epoch_log, (size_t)dev_epoch_cap * 2 * P * 4, hipMemcpyDeviceToHost, c->stream));
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
        stats->candidates = (uint64_t)epochs * count * P;
        stats->moves = improved;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_particle_swarm(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_pso_opts *opts, uint64_t seed,
                                 uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return pso_run(c, "tl_particle_swarm", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats, nullptr,
                   0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_particle_swarm_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_pso_opts *opts,
                                       uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                       uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_particle_swarm_trace: NULL argument");
    return pso_run(c, "tl_particle_swarm_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, opts, seed, out_pos, out_cost, nullptr, nullptr, stats,
                   log, log_cap, log_len, route_log, route_cap, epoch_log, epoch_cap);
}

extern "C" int tl_particle_swarm_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                            uint32_t first_run, uint32_t count, const tl_pso_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                            uint32_t *out_moves, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return pso_run(c, "tl_particle_swarm_population", xy, n, dm_packed, init_pos, init_count, first_run, count, opts, seed, out_pos, out_costs, out_moves,
                   best_index, stats, nullptr, 0, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int tl_pso_selftest_swap_sequence(tl_ctx *c, const uint32_t *from, const uint32_t *to, uint32_t n, uint32_t count, uint32_t *out_pairs,
                                             uint32_t *out_len)
{
    TL_ENTER(c);
    if (!c || !from || !to || !out_pairs || !out_len) return fail(c, TL_ERR_BADARG, "tl_pso_selftest_swap_sequence: NULL argument");
    if (n < 1u || n > particle_swarm_max_n(c->lds_bytes) || count < 1u || count > kPsoMaxRuns)
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
