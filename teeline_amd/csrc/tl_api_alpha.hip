// tl_api_alpha.hip — C ABI, alpha-nearness candidate lists: tl_alpha_candidates over alpha_candidates.hip, the sequential restatement
// tl_alpha_candidates_host and the host-only queries (plan, max_n).  DESIGN.md §4.32; alpha_spec.h is the text the device, the
// restatement and the one-core probe share.
//
// The device entry builds §4.29's 1-tree under the caller's pi with ONE iteration of k_one_tree_ascent (its Prim round is the only
// one on the device), prepares the tree's parent weights and level order on the host (O(n), once per call) and runs one workgroup
// per source city.
#include "alpha_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr double kAlphaMaxPi = 0x1p1020;  // |pi_i + pi_j| <= 2^1021 and d < 2^65: every w is finite

// nullptr: valid
static const char *alpha_bad_pi(const double *pi, uint32_t n)
{
    if (pi)
        for (uint32_t v = 0; v < n; ++v)
            if (!(std::fabs(pi[v]) <= kAlphaMaxPi)) return "a penalty is not finite or beyond 2^1020";
    return nullptr;
}

// what both entries check before anything of size n is read; kk: min(k, n - 1)
static int alpha_check(tl_ctx *c, const char *who, const float *xy, const float *dm_packed, uint32_t n, uint32_t root, uint32_t k, const uint32_t *out_cand,
                       uint32_t max_n)
{
    if ((n && !xy && !dm_packed) || (n > 1u && !out_cand)) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (root >= (n ? n : 1u)) return fail(c, TL_ERR_BADARG, "%s: root is not a position", who);
    if (k < 1u) return fail(c, TL_ERR_BADARG, "%s: k must be >= 1", who);
    if (k > kAlphaMaxK) return fail(c, TL_ERR_UNSUPPORTED, "%s: k = %u is above %u", who, k, kAlphaMaxK);
    if (n > max_n) return fail(c, TL_ERR_UNSUPPORTED, "%s: n = %u is above %u, the largest whose 1-tree and rows fit the LDS", who, n, max_n);
    return TL_OK;
}

// n <= 2: no tree to build.  n == 2: each position's only candidate is the other, alpha 0
static void alpha_trivial(uint32_t n, uint32_t *out_cand, double *out_alpha, uint32_t *out_parent, uint32_t *out_root_nb)
{
    for (uint32_t v = 0; v < n; ++v) {
        if (out_parent) out_parent[v] = kOneTreeNone;
        if (n == 2u) {
            out_cand[v] = 1u - v;
            if (out_alpha) out_alpha[v] = 0.0;
        }
    }
    if (out_root_nb) out_root_nb[0] = out_root_nb[1] = kOneTreeNone;
}

namespace {
struct HostDist {  // d(a, b), a != b, as the library's kernels round it
    const float *xy, *dm_packed;
    float operator()(uint32_t a, uint32_t b) const
    {
        if (dm_packed) return a > b ? dm_packed[(size_t)a * (a - 1) / 2 + b] : dm_packed[(size_t)b * (b - 1) / 2 + a];
        const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
        const float sx = dx * dx, sy = dy * dy;
        return sqrtf(sx + sy);
    }
};
}  // namespace

extern "C" uint32_t tl_alpha_candidates_max_n(int lds_bytes)
{
    const uint32_t a = one_tree_max_n(lds_bytes), b = alpha_rows_max_n(lds_bytes);
    return a < b ? a : b;
}

extern "C" int tl_alpha_candidates_plan(uint32_t n, uint32_t k, int lds_bytes, int *threads, uint32_t *lds_used)
{
    if (threads) *threads = 0;
    if (lds_used) *lds_used = 0u;
    if (lds_bytes < 0 || k < 1u) return TL_ERR_BADARG;
    if (k > kAlphaMaxK) return TL_ERR_UNSUPPORTED;
    if (n <= 2u) return TL_OK;
    if (n > tl_alpha_candidates_max_n(lds_bytes)) return TL_ERR_UNSUPPORTED;
    if (threads) *threads = alpha_rows_threads(n);
    if (lds_used) *lds_used = (uint32_t)alpha_rows_lds_bytes(n);
    return TL_OK;
}

extern "C" int tl_alpha_candidates_host(const float *xy, const float *dm_packed, uint32_t n, const double *pi, uint32_t root, uint32_t k, uint32_t *out_cand,
                                        double *out_alpha, uint32_t *out_parent, uint32_t *out_root_nb)
{
    const char *who = "tl_alpha_candidates_host";
    if (int rc = alpha_check(nullptr, who, xy, dm_packed, n, root, k, out_cand, 65535u)) return rc;
    if (const char *why = one_tree_bad_input(xy, dm_packed, n)) return fail(nullptr, TL_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (const char *why = alpha_bad_pi(pi, n)) return fail(nullptr, TL_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (n <= 2u) {
        alpha_trivial(n, out_cand, out_alpha, out_parent, out_root_nb);
        return TL_OK;
    }
    std::vector<double> zero;
    if (!pi) {
        zero.assign(n, 0.0);
        pi = zero.data();
    }
    const uint32_t kk = k > n - 1u ? n - 1u : k;
    if (!alpha_candidates_seq(HostDist{xy, dm_packed}, pi, n, root, kk, out_cand, out_alpha, out_parent, out_root_nb))
        return fail(nullptr, TL_ERR_HIP, "%s: the 1-tree is no tree", who);
    return TL_OK;
}

extern "C" int tl_alpha_candidates(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, const double *pi, uint32_t root, uint32_t k, uint32_t threads,
                                   uint32_t *out_cand, double *out_alpha, uint32_t *out_parent, uint32_t *out_root_nb, tl_stats *stats)
{
    TL_ENTER(c);
    const char *who = "tl_alpha_candidates";
    if (!c) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (int rc = alpha_check(c, who, xy, dm_packed, n, root, k, out_cand, tl_alpha_candidates_max_n(c->lds_bytes))) return rc;
    if (threads != 0u && (threads % 64u != 0u || threads > 1024u))
        return fail(c, TL_ERR_BADARG, "%s: threads = %u is neither 0 (the plan's) nor whole waves up to 1024", who, threads);
    if (const char *why = one_tree_bad_input(xy, dm_packed, n)) return fail(c, TL_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (const char *why = alpha_bad_pi(pi, n)) return fail(c, TL_ERR_UNSUPPORTED, "%s: %s", who, why);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n <= 2u) {
        alpha_trivial(n, out_cand, out_alpha, out_parent, out_root_nb);
        c->ev_valid = false;
        stamp_times(c, stats, t0);
        return TL_OK;
    }
    const uint32_t kk = k > n - 1u ? n - 1u : k;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += up256(bytes);
        return here;
    };
    const size_t o_job = take(sizeof(OneTreeJob)), o_state = take(sizeof(OneTreeState)), o_pi = take((size_t)n * 8), o_best_pi = take((size_t)n * 8),
                 o_par = take((size_t)n * 4), o_tour_par = take((size_t)n * 4), o_by_pos = take((size_t)n * sizeof(AlphaNode)),
                 o_by_level = take((size_t)n * sizeof(AlphaNode)), o_level_at = take(((size_t)n + 1u) * 4), o_cand = take((size_t)n * kk * 4),
                 o_alpha = take((size_t)n * kk * 8);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->work, at))) return rc;
    const float2 *dxy = nullptr;
    const float *dfull = nullptr;
    if ((rc = upload_instance_full(c, xy, dm_packed, n, &dxy, &dfull))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;

    // the 1-tree under pi: one ascent iteration from pi keeps its tree as the best (any L is above the start's -inf)
    const OneTreeJob J{1.0, 1.0, root, 1u, 1u, 0u};
    OneTreeState S;
    one_tree_start(S, J);
    HIPCHK(c, hipMemcpyAsync(w + o_job, &J, sizeof(J), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + o_state, &S, sizeof(S), hipMemcpyHostToDevice, c->stream));
    if (pi) HIPCHK(c, hipMemcpyAsync(w + o_pi, pi, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(w + o_pi, 0, (size_t)n * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(w + o_par, 0xFF, (size_t)n * 4, c->stream));
    OneTreeArgs T{};
    T.jobs = (const OneTreeJob *)(w + o_job);
    T.state = (OneTreeState *)(w + o_state);
    T.xy = dxy;
    T.dm_full = dfull;
    T.pi = (double *)(w + o_pi);
    T.best_pi = (double *)(w + o_best_pi);
    T.best_par = (uint32_t *)(w + o_par);
    T.tour_par = (uint32_t *)(w + o_tour_par);
    T.n = n;
    T.span = 1u;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_one_tree_ascent(T, 1u, one_tree_threads(n), c->stream));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    std::vector<uint32_t> par(n);
    HIPCHK(c, hipMemcpyAsync(&S, T.state, sizeof(S), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(par.data(), T.best_par, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float tree_ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&tree_ms, c->ev0, c->ev1));
    const uint32_t nb[2] = {S.best_nb[0], S.best_nb[1]};
    if (S.k != 1u || S.best_iter != 0u || nb[0] >= n || nb[1] >= n || nb[0] == root || nb[1] == root || nb[0] == nb[1])
        return fail(c, TL_ERR_HIP, "%s: the 1-tree was not built", who);

    // its parent weights and level order, once per call (pi on the device is unchanged: the ascent stopped before its step)
    std::vector<double> zero;
    const double *hpi = pi;
    if (!hpi) {
        zero.assign(n, 0.0);
        hpi = zero.data();
    }
    std::vector<AlphaNode> by_pos, by_level;
    std::vector<uint32_t> level_at;
    if (!alpha_levels_host(HostDist{xy, dm_packed}, hpi, par.data(), n, root, by_pos, by_level, level_at))
        return fail(c, TL_ERR_HIP, "%s: the 1-tree is no tree", who);
    HIPCHK(c, hipMemcpyAsync(w + o_by_pos, by_pos.data(), (size_t)n * sizeof(AlphaNode), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + o_by_level, by_level.data(), by_level.size() * sizeof(AlphaNode), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + o_level_at, level_at.data(), level_at.size() * 4, hipMemcpyHostToDevice, c->stream));
    AlphaArgs A{};
    A.xy = dxy;
    A.dm_full = dfull;
    A.pi = T.pi;
    A.by_pos = (const AlphaNode *)(w + o_by_pos);
    A.by_level = (const AlphaNode *)(w + o_by_level);
    A.level_at = (const uint32_t *)(w + o_level_at);
    A.out_cand = (uint32_t *)(w + o_cand);
    A.out_alpha = out_alpha ? (double *)(w + o_alpha) : nullptr;
    A.n = n;
    A.kk = kk;
    A.levels = (uint32_t)level_at.size() - 1u;
    A.root = root;
    A.nb0 = nb[0];
    A.nb1 = nb[1];
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_alpha_rows(A, threads ? (int)threads : alpha_rows_threads(n), c->stream));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    HIPCHK(c, hipMemcpyAsync(out_cand, A.out_cand, (size_t)n * kk * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_alpha) HIPCHK(c, hipMemcpyAsync(out_alpha, A.out_alpha, (size_t)n * kk * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (out_parent) memcpy(out_parent, par.data(), (size_t)n * 4);
    if (out_root_nb) {
        out_root_nb[0] = nb[0];
        out_root_nb[1] = nb[1];
    }
    if (stats) {
        stats->sweeps = A.levels;                 // the tree's levels (depth + 1); a source's sweep takes levels - 1 barriers
        stats->candidates = (uint64_t)n * (n - 1u);  // alpha values formed
        stamp_times(c, stats, t0);                // the rows' kernel (tl_last_kernel_ms reports it alone) ...
        stats->kernel_ms += (double)tree_ms;      // ... and the 1-tree's launch; the host's preparation in between is left out
    }
    return TL_OK;
}
