// tl_api_bhk.hip — tl_bellman_karp: the Bellman-Held-Karp exact solver (bellman_karp.rs:24-165), the host side of
// csrc/bellman_karp.hip.  The DP table lives in the context's grow-only workspace and never crosses to the host: what comes back is
// the route, its tour_length, the optimum and whether the route is a permutation.
#include "tl_api_common.h"

#include <cfloat>

using namespace tl;
using namespace tlapi;

namespace {

struct Event {  // a HIP event of one call
    hipEvent_t e = nullptr;
    ~Event()
    {
        if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

extern "C" int tl_bellman_karp(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos, float *out_cost,
                               float *out_optimal, uint32_t *out_is_tour, tl_stats *stats)
{
    TL_ENTER(c);
    if (!c || (!xy && !dm_packed && n > 1) || (!out_pos && n)) return fail(c, TL_ERR_BADARG, "tl_bellman_karp: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    // the limit first: nothing is allocated for an instance whose table this build does not hold
    if (n > TL_BHK_MAX_N)
        return fail(c, TL_ERR_UNSUPPORTED, "tl_bellman_karp: n=%u > %u (TL_BHK_MAX_N: the table of n cities is 2^(n-1) rows of 128 bytes)", n,
                    TL_BHK_MAX_N);
    if (n <= 1) {
        // n = 0: nothing to write (the reference underflows there).  n = 1 (bellman_karp.rs:33-86 with no other city): the fold
        // over an empty range leaves f32::MAX, the walk's loop does not run, the route is [0] and its length d(0, 0) = 0.
        if (n) out_pos[0] = 0;
        if (out_cost) *out_cost = 0.0f;
        if (out_optimal) *out_optimal = n ? FLT_MAX : 0.0f;
        if (out_is_tour) *out_is_tour = 1;
        if (stats) {
            stats->moves = n;
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return TL_OK;
    }
    const uint32_t k = n - 1;
    const bool exact = (c->flags & TL_FLAG_BHK_EXACT_WALK) != 0;
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->out_pos, (size_t)n * 4)) || (rc = ensure(c, c->work, bhk_ws_bytes(n)))) return rc;
    const float2 *dxy = nullptr;
    const float *ddm = nullptr;
    if ((rc = upload_input(c, xy, dm_packed, n, &dxy, &ddm))) return rc;
    const BhkWs w = bhk_ws_layout(c->work.p, n);
    uint32_t binom[32 * 32];
    bhk_binomials(binom);
    HIPCHK(c, hipMemcpyAsync(w.binom, binom, sizeof(binom), hipMemcpyHostToDevice, c->stream));
    Event layers_begin, layers_end;
    HIPCHK(c, hipEventCreate(&layers_begin.e));
    HIPCHK(c, hipEventCreate(&layers_end.e));
    c->ev_valid = false;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_bhk_init(w, dxy, ddm, n, c->stream));
    HIPCHK(c, hipEventRecord(layers_begin.e, c->stream));
    uint64_t layers = 0;
    for (uint32_t p = 2; p <= k; ++p, ++layers) HIPCHK(c, launch_bhk_layer(w, n, p, binom[k * 32 + p], c->cus, c->stream));
    HIPCHK(c, hipEventRecord(layers_end.e, c->stream));
    HIPCHK(c, launch_bhk_walk(w, n, exact, (uint32_t *)c->out_pos.p, c->stream));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    float res_f[2] = {0.f, 0.f};
    uint32_t res_u = 0;
    HIPCHK(c, hipMemcpyAsync(out_pos, c->out_pos.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(res_f, w.out_f, sizeof(res_f), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&res_u, w.out_u, sizeof(res_u), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t a = 0; a < n; ++a)
        if (out_pos[a] >= n) return fail(c, TL_ERR_HIP, "tl_bellman_karp: position %u of n=%u in the route", out_pos[a], n);
    if (out_cost) *out_cost = res_f[0];
    if (out_optimal) *out_optimal = res_f[1];
    if (out_is_tour) *out_is_tour = res_u;
    if (stats) {
        float ms = 0.f, layer_ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        HIPCHK(c, hipEventElapsedTime(&layer_ms, layers_begin.e, layers_end.e));
        stats->sweeps = layers;
        stats->candidates = k >= 2 ? (uint64_t)k * (k - 1) << (k - 2) : 0;  // every (S, c, i) with i != c, both in S
        stats->moves = n;
        stats->reversed = (uint64_t)((double)layer_ms * 1e6);  // the DP layers alone, ns (tl_christofides' precedent for the field)
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return TL_OK;
}
