// tl_api_aco.hip — C ABI, the ant colony solver: tl_ant_colony* (src/tsp/ant_colony.rs:97-252) over ant_colony.hip, the host-only
// queries of its specification (tl_aco_draw, tl_aco_pow, tl_ant_colony_plan) and the device self-test of the selection.
#include "aco_spec.h"
#include "tl_api_swarm.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kAcoMaxAnts = 4096u;             // k_aco_best keeps a 16-bit list of the improving ants in LDS

// one run's share of the workspace: tau, eta^beta and W (n^2 f32 each); tour, successor, predecessor (A n u16 each); cost, start, fallbacks
static inline size_t aco_mat_bytes(uint32_t n) { return up256((size_t)n * n * 4); }
static inline size_t aco_tab_bytes(uint32_t n, uint32_t ants) { return up256((size_t)ants * n * 2); }
static inline size_t aco_ant_bytes(uint32_t ants) { return up256((size_t)ants * 4); }
static inline size_t aco_run_bytes(uint32_t n, uint32_t ants) { return 3 * aco_mat_bytes(n) + 3 * aco_tab_bytes(n, ants) + 3 * aco_ant_bytes(ants); }

static uint32_t aco_limit(int lds_bytes)
{
    uint32_t top = ant_colony_max_n(lds_bytes);
    while (top > 0u && aco_run_bytes(top, 1u) > kSwarmWorkDefault) --top;  // (12 n^2 bytes per run; the LDS layout binds first on 160 KiB)
    return top;
}

extern "C" uint64_t tl_aco_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot) { return ga_draw_key(sa_chain_key(seed, run), event, slot); }

extern "C" float tl_aco_pow(float x, float a) { return aco_pow(x, a); }

extern "C" uint32_t tl_ant_colony_max_n(const tl_ctx *c) { return c ? aco_limit(c->lds_bytes) : 0u; }

extern "C" int tl_ant_colony_plan(uint32_t n, uint32_t num_ants, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t *per_launch,
                                  int *threads, uint64_t *workspace_needed)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    const bool fits = n >= 3u && n <= aco_limit(lds_bytes) && num_ants >= 1u && num_ants <= kAcoMaxAnts;
    uint64_t per = fits ? workspace_bytes / aco_run_bytes(n, num_ants) : 0u;
    if (per > kSwarmMaxRuns) per = kSwarmMaxRuns;
    if (per_launch) *per_launch = (uint32_t)per;
    if (threads) *threads = per ? ant_colony_threads() : 0;
    if (workspace_needed) *workspace_needed = per ? (uint64_t)(count < per ? count : per) * aco_run_bytes(n, num_ants) : 0u;
    return TL_OK;
}

static float aco_host_dist(const float *xy, const float *dm_packed, uint32_t a, uint32_t b)  // n <= 2 only
{
    if (dm_packed) return a == b ? 0.0f : dm_packed[0];
    const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
    volatile float xx = dx * dx, yy = dy * dy;
    return sqrtf(xx + yy);
}

namespace {
// What the ant colony hands the frame of tl_api_swarm.h.  Its trace is another format than Swarm4's — a row of 3 num_ants words per
// epoch, route rows of n + 3 words, the two lengths — so the trace's steps are written here, as is the n <= 2 answer.
struct AcoSolver {
    using Args = AcoArgs;
    static constexpr uint32_t kHostN = 2u;
    uint32_t epochs;
    float alpha, beta, rate;
    uint32_t num_ants;
    // log / route_log: the epochs and improving ants of run 0 of the call (a single run's trace), else nullptr
    uint32_t *log = nullptr;
    uint32_t log_cap = 0;
    uint32_t *log_len = nullptr, *route_log = nullptr;
    uint32_t route_cap = 0;
    uint32_t *route_len = nullptr;
    uint32_t dev_log_cap = 0, dev_route_cap = 0, held = 0;
    size_t log_bytes = 0, route_bytes = 0;

    uint32_t pop() const { return num_ants; }
    void trace_reset() const
    {
        if (log_len) *log_len = 0;
        if (route_len) *route_len = 0;
    }
    int check(const SwarmCall &k) const
    {
        tl_ctx *c = k.c;
        const char *who = k.who;
        // AcoOptions::validate (mod.rs:1115-1153)
        if (!(alpha >= 0.0f) || alpha > 3.4028234663852886e38f) return fail(c, TL_ERR_BADARG, "%s: alpha must be >= 0 (got %g)", who, (double)alpha);
        if (!(beta >= 0.0f && beta <= 6.0f)) return fail(c, TL_ERR_BADARG, "%s: beta must be in [0, 6] (got %g)", who, (double)beta);
        if (!(rate > 0.0f && rate < 1.0f)) return fail(c, TL_ERR_BADARG, "%s: evaporation_rate must be in (0, 1) (got %g)", who, (double)rate);
        if (num_ants == 0u) return fail(c, TL_ERR_BADARG, "%s: num_ants must be >= 1", who);
        if (num_ants > kAcoMaxAnts) return fail(c, TL_ERR_UNSUPPORTED, "%s: num_ants=%u exceeds the limit %u", who, num_ants, kAcoMaxAnts);
        if (k.n > aco_limit(c->lds_bytes))
            return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the limit %u (12 bytes of LDS per city)", who, k.n, aco_limit(c->lds_bytes));
        if (k.n >= 3u && (unsigned __int128)epochs * num_ants * k.n > kAcoEventLimit)
            return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs x num_ants x n exceeds 2^58 draw events", who);
        return TL_OK;
    }
    // n <= 2 (ant_colony.rs:109-115): city order, no draw, no device; Solution::from_parts computes its tour_length
    void host_answer(const SwarmCall &k) const
    {
        const float cost = k.n == 2u ? aco_host_dist(k.xy, k.dm_packed, 1, 0) + aco_host_dist(k.xy, k.dm_packed, 0, 1) : 0.0f;
        for (uint32_t r = 0; r < k.count; ++r) {
            for (uint32_t i = 0; i < k.n; ++i) k.out_pos[(size_t)r * k.n + i] = i;
            if (k.out_costs) k.out_costs[r] = cost;
        }
    }
    int plan(const SwarmCall &k, uint32_t *per_launch) const
    {
        tl_ant_colony_plan(k.n, num_ants, k.count, k.c->cus, k.c->lds_bytes, kSwarmWorkDefault, per_launch, nullptr, nullptr);
        if (*per_launch == 0u)
            return fail(k.c, TL_ERR_UNSUPPORTED, "%s: n=%u, num_ants=%u: one run's matrices and tables (%zu bytes) exceed the workspace limit", k.who, k.n,
                        num_ants, aco_run_bytes(k.n, num_ants));
        return TL_OK;
    }
    size_t layout(const SwarmCall &k, uint32_t held_runs)
    {
        held = held_runs;
        dev_log_cap = log ? (log_cap < epochs ? log_cap : epochs) : 0u;
        dev_route_cap = route_log ? route_cap : 0u;
        log_bytes = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 3 * num_ants * 4);
        route_bytes = up256((size_t)(dev_route_cap ? dev_route_cap : 1u) * (k.n + 3) * 4);
        return log_bytes + route_bytes + (size_t)held * aco_run_bytes(k.n, num_ants);
    }
    void carve(const SwarmCall &k, Args &A, unsigned char *w) const
    {
        A.log = log ? (uint32_t *)w : nullptr;
        A.log_cap = dev_log_cap;
        A.route_log = route_log ? (uint32_t *)(w + log_bytes) : nullptr;
        A.route_cap = dev_route_cap;
        w += log_bytes + route_bytes;
        const size_t mb = aco_mat_bytes(k.n), tb = aco_tab_bytes(k.n, num_ants), ab = aco_ant_bytes(num_ants);
        A.tau = (float *)w;
        A.eta = (float *)(w + (size_t)held * mb);
        A.w = (float *)(w + 2 * (size_t)held * mb);
        A.mat_stride = mb / 4;
        w += 3 * (size_t)held * mb;
        // (the tables of a run are num_ants x n entries: a run's stride is that product, so they are laid out run after run, unpadded)
        A.tour = (uint16_t *)w;
        A.succ = (uint16_t *)(w + (size_t)held * tb);
        A.pred = (uint16_t *)(w + 2 * (size_t)held * tb);
        w += 3 * (size_t)held * tb;
        A.cost = (float *)w;
        A.start = (uint32_t *)(w + (size_t)held * ab);
        A.fb = (uint32_t *)(w + 2 * (size_t)held * ab);
        A.num_ants = num_ants;
        A.alpha = alpha;
        A.beta = beta;
        A.rate = rate;
    }
    void trace_off(Args &L) const { L.log = L.route_log = nullptr; }
    hipError_t enqueue(tl_ctx *c, Args &L, uint32_t cnt) const
    {
        hipError_t e = launch_aco_init(L, cnt, c->stream);
        if (epochs == 0u || e != hipSuccess) return e;
        L.pre = 1u;
        e = launch_aco_update(L, cnt, c->lds_bytes, c->stream);
        L.pre = 0u;
        for (uint32_t g = 0; g < epochs && e == hipSuccess; ++g) {
            L.epoch = g;
            if ((e = launch_aco_construct(L, cnt, c->stream)) == hipSuccess) e = launch_aco_best(L, cnt, c->stream);
            if (g + 1u < epochs && e == hipSuccess) e = launch_aco_update(L, cnt, c->lds_bytes, c->stream);  // (the last epoch's deposit is read by nobody)
        }
        return e;
    }
    int trace_download(const SwarmCall &k, const Args &A) const
    {
        if (dev_log_cap) HIPCHK(k.c, hipMemcpyAsync(log, A.log, (size_t)dev_log_cap * 3 * num_ants * 4, hipMemcpyDeviceToHost, k.c->stream));
        return TL_OK;
    }
    int verdict(const SwarmCall &, const std::vector<uint32_t> &) const { return TL_OK; }
    int trace_finish(const SwarmCall &k, const Args &A, const std::vector<uint32_t> &state) const
    {
        if (dev_route_cap) {
            const uint64_t rows = 1ull + state[1];
            const uint32_t have = (uint32_t)(rows < dev_route_cap ? rows : dev_route_cap);
            if (int rc = download_sync(k.c, route_log, A.route_log, (size_t)have * (k.n + 3) * 4)) return rc;
        }
        if (route_len) *route_len = 1u + state[1];
        if (log_len) *log_len = epochs;
        if (k.stats)  // the fallback selections of every run
            for (uint32_t r = 0; r < k.count; ++r) k.stats->reversed += ((uint64_t)state[8u * r + 5u] << 32) | state[8u * r + 2u];
        return TL_OK;
    }
};
}  // namespace

extern "C" int tl_ant_colony(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, float alpha, float beta,
                             float evaporation_rate, uint32_t num_ants, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm_run({c, "tl_ant_colony", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, seed, out_pos, out_cost, stats},
                     AcoSolver{epochs, alpha, beta, evaporation_rate, num_ants});
}

extern "C" int tl_ant_colony_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, float alpha,
                                   float beta, float evaporation_rate, uint32_t num_ants, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats,
                                   uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *route_len)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_ant_colony_trace: NULL argument");
    return swarm_run({c, "tl_ant_colony_trace", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, 0u, 1u, seed, out_pos, out_cost, stats},
                     AcoSolver{epochs, alpha, beta, evaporation_rate, num_ants, log, log_cap, log_len, route_log, route_cap, route_len});
}

extern "C" int tl_ant_colony_trace_run(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, float alpha,
                                       float beta, float evaporation_rate, uint32_t num_ants, uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost,
                                       tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap,
                                       uint32_t *route_len)
{
    TL_ENTER(c);
    if (!log || !log_len) return fail(c, TL_ERR_BADARG, "tl_ant_colony_trace_run: NULL argument");
    return swarm_run({c, "tl_ant_colony_trace_run", xy, n, dm_packed, init_pos, init_pos ? 1u : 0u, run, 1u, seed, out_pos, out_cost, stats},
                     AcoSolver{epochs, alpha, beta, evaporation_rate, num_ants, log, log_cap, log_len, route_log, route_cap, route_len});
}

extern "C" int tl_ant_colony_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                        uint32_t first_run, uint32_t count, uint32_t epochs, float alpha, float beta, float evaporation_rate, uint32_t num_ants,
                                        uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return swarm_run({c, "tl_ant_colony_population", xy, n, dm_packed, init_pos, init_count, first_run, count, seed, out_pos, out_costs, stats, nullptr, best_index},
                     AcoSolver{epochs, alpha, beta, evaporation_rate, num_ants});
}

extern "C" int tl_aco_selftest_select(tl_ctx *c, const float *weights, const float *eta, const uint32_t *visited, uint32_t n, float r1, float r2, uint32_t *out)
{
    TL_ENTER(c);
    if (!c || !weights || !eta || !visited || !out) return fail(c, TL_ERR_BADARG, "tl_aco_selftest_select: NULL argument");
    if (n < 1u || n > aco_limit(c->lds_bytes)) return fail(c, TL_ERR_BADARG, "tl_aco_selftest_select: n out of range");
    uint32_t candidates = 0;
    for (uint32_t k = 0; k < n; ++k) candidates += visited[k] == 0u;
    if (candidates == 0u) return fail(c, TL_ERR_BADARG, "tl_aco_selftest_select: the candidate set must be non-empty");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t row = up256((size_t)n * 4);
    if ((rc = ensure(c, c->work, 3 * row + 256))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    c->ev_valid = false;
    HIPCHK(c, hipMemcpyAsync(w, weights, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + row, eta, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + 2 * row, visited, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_aco_selftest_select((const float *)w, (const float *)(w + row), (const uint32_t *)(w + 2 * row), n, r1, r2, (uint32_t *)(w + 3 * row),
                                         c->stream));
    HIPCHK(c, hipMemcpyAsync(out, w + 3 * row, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}
