// tl_api_onetree.hip — C ABI, the Held-Karp lower bound: tl_one_tree_bound* over one_tree_bound.hip, the sequential restatement
// tl_one_tree_bound_host and the host-only queries (plan, max_n, work_bytes).  DESIGN.md §4.29; one_tree_spec.h is the text the
// device and the restatement share.
//
// A batch is a list of option sets (root, lambda0, patience, ..) on one problem, one workgroup each.  The ascent's state lives in
// the workspace between launches; a launch runs at most `span` iterations of every job still running.
#include "one_tree_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kOneTreeMaxJobs = 65535u;  // the job is the grid's x
static constexpr float kOneTreeMaxCoord = 0x1p62f;   // |dx| <= 2^63, dx dx + dy dy <= 2^127: every distance is finite

// nullptr: valid
static const char *one_tree_invalid(const tl_one_tree_opts &o, uint32_t n)
{
    if (o.root >= (n ? n : 1u)) return "root is not a position";
    if (o.iterations < 1u) return "iterations must be >= 1";
    if (!(std::isfinite(o.lambda0) && o.lambda0 > 0.0)) return "lambda0 must be finite and > 0";
    if (o.patience < 1u) return "patience must be >= 1";
    if (!(std::isfinite(o.upper) && o.upper > 0.0)) return "upper must be finite and > 0";
    if (o.reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// nullptr: every distance of the instance is finite and >= +0.0 (tl_api_alpha.hip holds its input to the same rules)
const char *tlapi::one_tree_bad_input(const float *xy, const float *dm_packed, uint32_t n)
{
    if (dm_packed) {
        const size_t m = (size_t)n * (n - 1) / 2;
        for (size_t k = 0; k < m; ++k)
            if (!std::isfinite(dm_packed[k]) || std::signbit(dm_packed[k])) return "a matrix entry is not finite or is negative";
        return nullptr;
    }
    for (size_t k = 0; k < 2 * (size_t)n; ++k)
        if (!(std::fabs(xy[k]) <= kOneTreeMaxCoord)) return "a coordinate is not finite or beyond 2^62";
    return nullptr;
}

static void one_tree_result_of(const OneTreeState &S, tl_one_tree_result *r)
{
    r->bound = S.best;
    r->lambda = S.lambda;
    r->best_iter = S.best_iter;
    r->iterations_run = S.k;
    r->stop = S.stop;
    r->is_tour = S.is_tour;
    for (int e = 0; e < 2; ++e) {
        r->root_nb[e] = S.best_nb[e];
        r->tour_nb[e] = S.tour_nb[e];
    }
}

// n <= 2: no tree to build
static void one_tree_trivial(const float *xy, const float *dm_packed, uint32_t n, tl_one_tree_result *r, double *pi, uint32_t *parent, uint32_t *tour)
{
    if (r) {
        memset(r, 0, sizeof(*r));
        r->root_nb[0] = r->root_nb[1] = r->tour_nb[0] = r->tour_nb[1] = kOneTreeNone;
        r->is_tour = 1u;
        if (n == 2u) {
            float d;
            if (dm_packed) d = dm_packed[0];
            else {
                const float dx = xy[2] - xy[0], dy = xy[3] - xy[1];
                const float sx = dx * dx, sy = dy * dy;
                d = sqrtf(sx + sy);
            }
            r->bound = 2.0 * (double)d;
        }
    }
    for (uint32_t v = 0; v < n; ++v) {
        if (pi) pi[v] = 0.0;
        if (parent) parent[v] = kOneTreeNone;
        if (tour) tour[v] = v;
    }
}

// the tour a 1-tree of degrees 2 is: from the root towards its first chosen neighbour
static void one_tree_tour(const uint32_t *par, const uint32_t *nb, uint32_t s, uint32_t n, uint32_t *tour)
{
    std::vector<uint32_t> adj(2 * (size_t)n, kOneTreeNone);
    auto add = [&](uint32_t a, uint32_t b) {
        if (adj[2 * (size_t)a] == kOneTreeNone) adj[2 * (size_t)a] = b;
        else adj[2 * (size_t)a + 1] = b;
    };
    for (uint32_t v = 0; v < n; ++v)
        if (v != s && par[v] < n) {
            add(v, par[v]);
            add(par[v], v);
        }
    uint32_t prev = kOneTreeNone, cur = nb[0];
    tour[0] = s;
    for (uint32_t i = 1; i < n && cur < n; ++i) {
        tour[i] = cur;
        const uint32_t nx = adj[2 * (size_t)cur] != prev ? adj[2 * (size_t)cur] : adj[2 * (size_t)cur + 1];
        prev = cur;
        cur = nx;
    }
}

extern "C" uint32_t tl_one_tree_bound_max_n(int lds_bytes) { return one_tree_max_n(lds_bytes); }

static uint32_t one_tree_span(uint32_t n) { return n >= 16384u ? 1u : 16384u / n; }  // about 16 384 Prim rounds a launch

extern "C" int tl_one_tree_bound_plan(uint32_t n, int lds_bytes, int *threads, uint32_t *iters_per_launch)
{
    if (threads) *threads = 0;
    if (iters_per_launch) *iters_per_launch = 0u;
    if (lds_bytes < 0) return TL_ERR_BADARG;
    if (n <= 2u) return TL_OK;
    if (n > one_tree_max_n(lds_bytes)) return TL_ERR_UNSUPPORTED;
    if (threads) *threads = one_tree_threads(n);
    if (iters_per_launch) *iters_per_launch = one_tree_span(n);
    return TL_OK;
}

namespace {
struct OneTreeLayout {
    size_t jobs, state, pi, best_pi, best_par, tour_par, log, total;
};
OneTreeLayout one_tree_layout(uint32_t J, uint32_t n, uint32_t log_cap)
{
    OneTreeLayout W;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += up256(bytes ? bytes : 1u);
        return here;
    };
    W.jobs = take((size_t)J * sizeof(OneTreeJob));
    W.state = take((size_t)J * sizeof(OneTreeState));
    W.pi = take((size_t)J * n * 8);
    W.best_pi = take((size_t)J * n * 8);
    W.best_par = take((size_t)J * n * 4);
    W.tour_par = take((size_t)J * n * 4);
    W.log = take((size_t)J * log_cap * 24);
    W.total = at;
    return W;
}
}  // namespace

extern "C" uint64_t tl_one_tree_bound_work_bytes(uint32_t n, uint32_t jobs, uint32_t log_cap)
{
    if (n <= 2u || jobs == 0u || jobs > kOneTreeMaxJobs) return 0u;
    return one_tree_layout(jobs, n, log_cap).total;
}

extern "C" int tl_one_tree_bound_host(const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, tl_one_tree_result *result,
                                      double *out_pi, uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap)
{
    const char *who = "tl_one_tree_bound_host";
    if (!opts || (n && !xy && !dm_packed)) return fail(nullptr, TL_ERR_BADARG, "%s: NULL argument", who);
    if (const char *why = one_tree_invalid(*opts, n)) return fail(nullptr, TL_ERR_BADARG, "%s: %s", who, why);
    if (n > 65535u) return fail(nullptr, TL_ERR_UNSUPPORTED, "%s: n above 65 535", who);
    if (const char *why = one_tree_bad_input(xy, dm_packed, n)) return fail(nullptr, TL_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (n <= 2u) {
        one_tree_trivial(xy, dm_packed, n, result, out_pi, out_parent, out_tour);
        return TL_OK;
    }
    const OneTreeJob J{opts->lambda0, opts->upper, opts->root, opts->iterations, opts->patience, 0u};
    OneTreeState S;
    one_tree_start(S, J);
    auto d_of = [&](uint32_t a, uint32_t b) -> float {  // a != b
        if (dm_packed) return a > b ? dm_packed[(size_t)a * (a - 1) / 2 + b] : dm_packed[(size_t)b * (b - 1) / 2 + a];
        const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
        const float sx = dx * dx, sy = dy * dy;
        return sqrtf(sx + sy);
    };
    const uint32_t s = J.root, start = s == 0u ? 1u : 0u;
    const double inf = __builtin_huge_val();
    std::vector<double> pi(n, 0.0), key(n), best_pi(n, 0.0);
    std::vector<uint32_t> par(n), best_par(n, kOneTreeNone), tour_par(n, kOneTreeNone);
    std::vector<int> deg(n);
    std::vector<char> in(n);
    while (S.stop == kOneTreeStopNone) {
        for (uint32_t v = 0; v < n; ++v) {
            key[v] = v == start ? 0.0 : inf;
            par[v] = kOneTreeNone;
            deg[v] = 0;
            in[v] = v == s;
        }
        double sum = 0.0;
        for (uint32_t r = 0; r + 1u < n; ++r) {
            uint32_t u = kOneTreeNone;
            for (uint32_t v = 0; v < n; ++v)
                if (!in[v] && (u == kOneTreeNone || key[v] < key[u])) u = v;
            in[u] = 1;
            sum = sum + key[u];
            if (par[u] != kOneTreeNone) {
                ++deg[u];
                ++deg[par[u]];
            }
            for (uint32_t v = 0; v < n; ++v) {
                if (in[v]) continue;
                const double w = (double)d_of(u, v) + (pi[u] + pi[v]);
                if (w < key[v]) {
                    key[v] = w;
                    par[v] = u;
                }
            }
        }
        uint32_t nb[2] = {kOneTreeNone, kOneTreeNone};
        for (int e = 0; e < 2; ++e) {
            double bw = 0.0;
            for (uint32_t v = 0; v < n; ++v) {
                if (v == s || v == nb[0]) continue;
                const double w = (double)d_of(s, v) + (pi[s] + pi[v]);
                if (nb[e] == kOneTreeNone || w < bw) {
                    bw = w;
                    nb[e] = v;
                }
            }
            sum = sum + bw;
            ++deg[nb[e]];
        }
        deg[s] = 2;
        double P = 0.0;
        for (uint32_t v = 0; v < n; ++v) P = P + pi[v];
        const double L = sum - 2.0 * P;
        uint32_t g2 = 0;
        for (uint32_t v = 0; v < n; ++v) g2 += (uint32_t)((deg[v] - 2) * (deg[v] - 2));
        const uint32_t it = S.k;
        double t;
        const bool improved = one_tree_decide(S, J, L, g2, &t);
        if (improved) {
            best_pi = pi;
            best_par = par;
            S.best_nb[0] = nb[0];
            S.best_nb[1] = nb[1];
        }
        if (S.is_tour) {
            tour_par = par;
            S.tour_nb[0] = nb[0];
            S.tour_nb[1] = nb[1];
        }
        if (log && it < log_cap) {
            log[3 * (size_t)it] = L;
            log[3 * (size_t)it + 1] = (double)g2;
            log[3 * (size_t)it + 2] = S.lambda;
        }
        if (S.stop == kOneTreeStopNone)
            for (uint32_t v = 0; v < n; ++v) pi[v] = pi[v] + t * (double)(deg[v] - 2);
    }
    if (result) one_tree_result_of(S, result);
    if (out_pi) memcpy(out_pi, best_pi.data(), (size_t)n * 8);
    if (out_parent) memcpy(out_parent, best_par.data(), (size_t)n * 4);
    if (out_tour && S.is_tour) one_tree_tour(tour_par.data(), S.tour_nb, s, n, out_tour);
    return TL_OK;
}

static int one_tree_run(tl_ctx *c, const char *who, const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, uint32_t J,
                        tl_one_tree_result *results, double *out_pi, uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap,
                        uint32_t *best_index, tl_stats *stats)
{
    if (!c) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (J == 0u) return TL_OK;
    if (!opts || (n && !xy && !dm_packed)) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (J > kOneTreeMaxJobs) return fail(c, TL_ERR_BADARG, "%s: more than %u jobs", who, kOneTreeMaxJobs);
    for (uint32_t j = 0; j < J; ++j)
        if (const char *why = one_tree_invalid(opts[j], n)) return fail(c, TL_ERR_BADARG, "%s: job %u: %s", who, j, why);
    if (n > one_tree_max_n(c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n = %u is above %u, the largest whose keys, penalties, parents and degrees fit the LDS", who, n,
                    one_tree_max_n(c->lds_bytes));
    if (const char *why = one_tree_bad_input(xy, dm_packed, n)) return fail(c, TL_ERR_UNSUPPORTED, "%s: %s", who, why);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    if (n <= 2u) {
        for (uint32_t j = 0; j < J; ++j)
            one_tree_trivial(xy, dm_packed, n, results ? results + j : nullptr, out_pi ? out_pi + (size_t)j * n : nullptr,
                             out_parent ? out_parent + (size_t)j * n : nullptr, out_tour ? out_tour + (size_t)j * n : nullptr);
        c->ev_valid = false;
        stamp_times(c, stats, t0);
        return TL_OK;
    }
    std::vector<OneTreeJob> jobs(J);
    std::vector<OneTreeState> state(J);
    uint32_t max_iters = 0, span = 0;
    for (uint32_t j = 0; j < J; ++j) {
        const tl_one_tree_opts &o = opts[j];
        jobs[j] = OneTreeJob{o.lambda0, o.upper, o.root, o.iterations, o.patience, 0u};
        one_tree_start(state[j], jobs[j]);
        if (o.iterations > max_iters) max_iters = o.iterations;
        if (o.iters_per_launch != opts[0].iters_per_launch)
            return fail(c, TL_ERR_BADARG, "%s: iters_per_launch is a launch parameter: the same for every job of a batch", who);
    }
    span = opts[0].iters_per_launch ? opts[0].iters_per_launch : one_tree_span(n);
    const OneTreeLayout W = one_tree_layout(J, n, log ? log_cap : 0u);

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->work, W.total))) return rc;
    OneTreeArgs A{};
    {
        const float2 *dxy = nullptr;
        const float *dfull = nullptr;
        if ((rc = upload_instance_full(c, xy, dm_packed, n, &dxy, &dfull))) return rc;
        A.xy = dxy;
        A.dm_full = dfull;
    }
    unsigned char *w = (unsigned char *)c->work.p;
    HIPCHK(c, hipMemcpyAsync(w + W.jobs, jobs.data(), (size_t)J * sizeof(OneTreeJob), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + W.state, state.data(), (size_t)J * sizeof(OneTreeState), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + W.pi, 0, (size_t)J * n * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(w + W.best_pi, 0, (size_t)J * n * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(w + W.best_par, 0xFF, (size_t)J * n * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(w + W.tour_par, 0xFF, (size_t)J * n * 4, c->stream));
    A.jobs = (const OneTreeJob *)(w + W.jobs);
    A.state = (OneTreeState *)(w + W.state);
    A.pi = (double *)(w + W.pi);
    A.best_pi = (double *)(w + W.best_pi);
    A.best_par = (uint32_t *)(w + W.best_par);
    A.tour_par = (uint32_t *)(w + W.tour_par);
    A.log = log && log_cap ? (double *)(w + W.log) : nullptr;
    A.log_cap = A.log ? log_cap : 0u;
    A.n = n;
    A.span = span;
    const int threads = one_tree_threads(n);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    uint32_t launches = 0;
    double polled_ms = 0.0;  // kernel time of the launch groups that ended in a look at the states: the host's look is not counted
    for (uint64_t k = 0; k < max_iters; k += span) {  // a job runs [its k, its k + span) or returns at once where it has stopped
        HIPCHK(c, launch_one_tree_ascent(A, J, threads, c->stream));
        if (++launches % 16u == 0u && k + span < max_iters) {  // every job may have stopped long before the largest iteration cap: look now and then
            HIPCHK(c, hipEventRecord(c->ev1, c->stream));
            if ((rc = download_sync(c, state.data(), A.state, (size_t)J * sizeof(OneTreeState)))) return rc;
            float ms = 0.f;
            HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
            polled_ms += (double)ms;
            HIPCHK(c, hipEventRecord(c->ev0, c->stream));
            bool running = false;
            for (uint32_t j = 0; j < J && !running; ++j) running = state[j].stop == kOneTreeStopNone;
            if (!running) break;
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    HIPCHK(c, hipMemcpyAsync(state.data(), A.state, (size_t)J * sizeof(OneTreeState), hipMemcpyDeviceToHost, c->stream));
    if (out_pi) HIPCHK(c, hipMemcpyAsync(out_pi, A.best_pi, (size_t)J * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_parent) HIPCHK(c, hipMemcpyAsync(out_parent, A.best_par, (size_t)J * n * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint32_t> tour_par;
    if (out_tour) {
        tour_par.resize((size_t)J * n);
        HIPCHK(c, hipMemcpyAsync(tour_par.data(), A.tour_par, (size_t)J * n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t iters = 0;
    uint32_t best = 0;
    for (uint32_t j = 0; j < J; ++j) {
        const OneTreeState &S = state[j];
        if (S.stop == kOneTreeStopNone) return fail(c, TL_ERR_HIP, "%s: job %u did not finish", who, j);
        if (results) one_tree_result_of(S, results + j);
        if (out_tour && S.is_tour) one_tree_tour(tour_par.data() + (size_t)j * n, S.tour_nb, jobs[j].root, n, out_tour + (size_t)j * n);
        if (S.best > state[best].best) best = j;
        iters += S.k;
    }
    if (A.log) {  // the rows a job wrote: its iterations_run, at most log_cap
        std::vector<double> rows((size_t)J * log_cap * 3);
        if ((rc = download_sync(c, rows.data(), A.log, rows.size() * 8))) return rc;
        for (uint32_t j = 0; j < J; ++j) {
            const uint32_t cnt = state[j].k < log_cap ? state[j].k : log_cap;
            memcpy(log + (size_t)j * log_cap * 3, rows.data() + (size_t)j * log_cap * 3, (size_t)cnt * 24);
        }
    }
    if (best_index) *best_index = best;
    if (stats) {
        stats->sweeps = iters;
        stats->candidates = iters * (n - 1u);
        stamp_times(c, stats, t0);
        stats->kernel_ms += polled_ms;  // every group of launches between its own event pair: the host's looks in between are left out
    }
    return TL_OK;
}

extern "C" int tl_one_tree_bound(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, tl_one_tree_result *result,
                                 double *out_pi, uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap, tl_stats *stats)
{
    TL_ENTER(c);
    return one_tree_run(c, "tl_one_tree_bound", xy, dm_packed, n, opts, 1u, result, out_pi, out_parent, out_tour, log, log_cap, nullptr, stats);
}

extern "C" int tl_one_tree_bound_batch(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, uint32_t jobs,
                                       tl_one_tree_result *results, double *out_pi, uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap,
                                       uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return one_tree_run(c, "tl_one_tree_bound_batch", xy, dm_packed, n, opts, jobs, results, out_pi, out_parent, out_tour, log, log_cap, best_index, stats);
}
