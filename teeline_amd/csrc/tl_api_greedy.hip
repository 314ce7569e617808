// tl_api_greedy.hip — tl_greedy_edge: greedy-edge construction (greedy_edge.rs:21-65), tl_savings / tl_savings_hub: savings
// construction (savings.rs:34-163), and tl_christofides (christofides.rs:12-241) — the host side of csrc/greedy_edge.hip and
// csrc/christofides.hip.  All three run the same bands; only the key and what the walk accepts differ.
#include "tl_api_common.h"

#include <cfloat>

using namespace tl;
using namespace tlapi;

namespace {

constexpr uint32_t kGeMaxN = 65535;  // positions are 16-bit in the sort keys; 0xFFFF is the end table's degree-2 mark
// the key is read as digits of 12, 12, 12, 12, 12 and 4 bits from the top
constexpr uint32_t kGeWidth[6] = {12, 12, 12, 12, 12, 4};
constexpr uint32_t kGeShift[6] = {52, 40, 28, 16, 4, 0};

// The band after t_prev: the largest T whose keys (among pairs of free cities, above t_prev) number at most cap — to the
// resolution of a histogram bin, refined digit by digit while the bin at the edge holds more than half the band; at the last
// digit a bin is one key, so the band is never empty while keys remain.  *count: keys in (t_prev, T].
int band_threshold(tl_ctx *c, const GreedyWs &w, const float2 *dxy, const float *ddm, uint32_t f, uint64_t t_prev, int blocks, GreedyKey key,
                   std::vector<uint32_t> &hist, uint64_t *t_out, uint64_t *count)
{
    uint64_t prefix = 0, t = t_prev, cum = 0;
    const uint64_t cap = w.cap;
    for (int lvl = 0; lvl < 6; ++lvl) {
        const uint32_t wd = kGeWidth[lvl], sh = kGeShift[lvl];
        HIPCHK(c, launch_greedy_hist(w, dxy, ddm, f, t_prev, prefix, sh, wd, blocks, key, c->stream));
        HIPCHK(c, hipMemcpyAsync(hist.data(), w.hist, (size_t)4 << wd, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint32_t bins = 1u << wd;
        uint32_t b = 0;
        for (; b < bins; ++b) {
            if (cum + hist[b] > cap) break;
            cum += hist[b];
        }
        const uint64_t digit_prefix = prefix << wd;
        if (b == bins) {  // the whole prefix range fits
            t = ((digit_prefix + bins) << sh) - 1;  // wraps to 2^64 - 1 at the top level
            break;
        }
        if (b > 0) {  // the end of bin b - 1 (bins below t_prev's are empty: t never moves back)
            const uint64_t e = ((digit_prefix + b) << sh) - 1;
            if (e > t) t = e;
        }
        if (cum * 2 >= cap || lvl == 5) break;
        prefix = digit_prefix | b;  // refine inside the crowded bin
    }
    *t_out = t;
    *count = cum;
    return TL_OK;
}

// savings.rs:94-117 in f32: sequential left-to-right sums, each divided by n as f32, d2 = dx*dx + dy*dy with separate roundings
// (the pragma holds whatever the build's flags say), the first i with d2 < best_d2 — so NaN / inf coordinates give 0.
uint32_t savings_hub(const float *xy, uint32_t n)
{
#pragma clang fp contract(off)
    float cx = 0.0f, cy = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        cx += xy[2 * (size_t)k];
        cy += xy[2 * (size_t)k + 1];
    }
    cx /= (float)n;
    cy /= (float)n;
    uint32_t best = 0;
    float best_d2 = FLT_MAX;
    for (uint32_t k = 0; k < n; ++k) {
        const float dx = xy[2 * (size_t)k] - cx, dy = xy[2 * (size_t)k + 1] - cy;
        const float d2 = dx * dx + dy * dy;
        if (d2 < best_d2) {
            best_d2 = d2;
            best = k;
        }
    }
    return best;
}

// The band loop all three constructions share: bands of sorted keys over the pairs of the free list, walked until `target` edges
// (greedy-edge, savings: n) or pairs (matching: k / 2) are accepted.  st: the state block as the start kernel left it (st[0]
// accepted, st[4] the free list's length), updated to the last band's.
int run_bands(tl_ctx *c, const char *who, const GreedyWs &w, const float2 *dxy, const float *ddm, uint32_t n, GreedyKey key, uint32_t target,
              uint32_t (&st)[8], uint64_t *bands_out)
{
    int rc;
    const int blocks = (c->cus > 0 ? c->cus : 256) * 8;
    std::vector<uint32_t> hist(4096);
    uint64_t t_prev = 0, bands = 0;  // every key is > 0 (j >= 1 in its low bits)
    while (st[0] < target) {
        uint64_t t = 0, count = 0;
        if ((rc = band_threshold(c, w, dxy, ddm, st[4], t_prev, blocks, key, hist, &t, &count))) return rc;
        if (count == 0)  // cannot happen on a complete graph (graph.rs:85-96); refuse rather than loop
            return fail(c, TL_ERR_HIP, "%s: no edge left after %u of %u accepted", who, st[0], target);
        HIPCHK(c, launch_greedy_band(w, dxy, ddm, n, st[4], t_prev, t, blocks, key, target, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, w.state, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (st[3] != count)
            return fail(c, TL_ERR_HIP, "%s: band %llu holds %u keys, its histogram %llu", who, (unsigned long long)bands, st[3],
                        (unsigned long long)count);
        ++bands;
        t_prev = t;
        if (st[0] < target && t == ~(uint64_t)0) return fail(c, TL_ERR_HIP, "%s: every edge walked, %u of %u accepted", who, st[0], target);
    }
    *bands_out = bands;
    return TL_OK;
}

// The limits the bands set, and the identity answer of the smallest inputs (n <= small_n: the cities in file order).  Returns
// TL_OK with *done = true when the answer is already written.
int limits_and_small(tl_ctx *c, const char *who, uint32_t small_n, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos,
                     float *out_cost, tl_stats *stats, std::chrono::steady_clock::time_point t0, bool *done)
{
    *done = false;
    if (n > kGeMaxN) return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u > %u (positions are 16-bit in the sort keys)", who, n, kGeMaxN);
    if ((size_t)n * 2 + 1024 > (size_t)c->lds_bytes)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the LDS-resident end table (%d bytes of LDS)", who, n, c->lds_bytes);
    if (n > small_n) return TL_OK;
    int rc;
    for (uint32_t k = 0; k < n; ++k) out_pos[k] = k;
    if (out_cost && (rc = tl_tour_length(c, dm_packed ? nullptr : xy, dm_packed, n, out_pos, out_cost))) return rc;
    if (stats) {
        stats->moves = n;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    *done = true;
    return TL_OK;
}

// The construction tl_greedy_edge and tl_savings share (the caller holds the context): savings = false walks the edges by length, true by their
// saving against `hub` (< n).
int construct(tl_ctx *c, const char *who, bool savings, uint32_t hub, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos,
              float *out_cost, tl_stats *stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc;
    bool done;
    // greedy_edge.rs:33-39, savings.rs:46-52: n <= 2 is the cities in file order
    if ((rc = limits_and_small(c, who, 2, xy, dm_packed, n, out_pos, out_cost, stats, t0, &done)) || done) return rc;
    const uint32_t cap = greedy_band_cap(c->lds_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->out_pos, (size_t)n * 4)) || (rc = ensure(c, c->out_cost, 4)) || (rc = ensure(c, c->work, greedy_ws_bytes(n, cap))))
        return rc;
    const float2 *dxy = nullptr;
    const float *ddm = nullptr;
    if ((rc = upload_input(c, xy, dm_packed, n, &dxy, &ddm))) return rc;
    const GreedyWs w = greedy_ws_layout(c->work.p, n, cap);
    uint32_t st[8] = {0, 0, 0, 0, n, 0, 0, 0};
    c->ev_valid = false;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_greedy_init(w, n, c->stream));
    if (savings) HIPCHK(c, launch_savings_dh(w, dxy, ddm, n, hub, c->stream));
    uint64_t bands = 0;
    if ((rc = run_bands(c, who, w, dxy, ddm, n, savings ? kGeKeySavings : kGeKeyLength, n, st, &bands))) return rc;
    HIPCHK(c, launch_greedy_path(w, n, (uint32_t *)c->out_pos.p, c->stream));
    if (out_cost) HIPCHK(c, launch_tour_length(dxy, ddm, n, (const uint32_t *)c->out_pos.p, (float *)c->out_cost.p, c->stream));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    HIPCHK(c, hipMemcpyAsync(out_pos, c->out_pos.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_cost) HIPCHK(c, hipMemcpyAsync(out_cost, c->out_cost.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (stats) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        stats->sweeps = bands;
        stats->candidates = (uint64_t)st[2] << 32 | st[1];
        stats->moves = n;
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return TL_OK;
}

// build_multigraph + hierholzer + shortcut (christofides.rs:172-241), literally: the tree edges (child, parent) in join order, then
// the matched pairs in acceptance order, each pushed on both ends' lists; from position 0 the walk pops the BACK of adj[v] and
// removes the FIRST single occurrence of v from adj[u] by swap_remove; the circuit is reversed and first occurrences are kept.
// The lists are slices of one array (their final lengths are known), so the walk allocates nothing per vertex.
void euler_shortcut(uint32_t n, const uint16_t *order, const uint16_t *parent, const uint32_t *pairs, uint32_t npairs, uint32_t *out_pos)
{
    std::vector<uint32_t> off(n + 1, 0), len(n, 0);
    for (uint32_t r = 1; r < n; ++r) {
        ++off[order[r] + 1u];
        ++off[parent[order[r]] + 1u];
    }
    for (uint32_t a = 0; a < 2 * npairs; ++a) ++off[pairs[a] + 1u];
    for (uint32_t v = 0; v < n; ++v) off[v + 1] += off[v];
    std::vector<uint32_t> adj(off[n]);
    auto push = [&](uint32_t u, uint32_t v) {
        adj[off[u] + len[u]++] = v;
        adj[off[v] + len[v]++] = u;
    };
    for (uint32_t r = 1; r < n; ++r) push(order[r], parent[order[r]]);
    for (uint32_t a = 0; a < npairs; ++a) push(pairs[2 * a], pairs[2 * a + 1]);
    std::vector<uint32_t> stack, circuit;
    stack.reserve(off[n] / 2 + 1);
    circuit.reserve(off[n] / 2 + 1);
    stack.push_back(0);
    while (!stack.empty()) {
        const uint32_t v = stack.back();
        if (len[v]) {
            const uint32_t u = adj[off[v] + --len[v]];
            uint32_t *au = adj.data() + off[u];
            for (uint32_t k = 0; k < len[u]; ++k)
                if (au[k] == v) {
                    au[k] = au[--len[u]];
                    break;
                }
            stack.push_back(u);
        } else {
            circuit.push_back(v);
            stack.pop_back();
        }
    }
    std::vector<unsigned char> seen(n, 0);
    uint32_t m = 0;
    for (size_t k = circuit.size(); k-- > 0;) {
        const uint32_t v = circuit[k];
        if (!seen[v]) {
            seen[v] = 1;
            out_pos[m++] = v;
        }
    }
}

struct Event {  // a HIP event of one call
    hipEvent_t e = nullptr;
    ~Event()
    {
        if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

extern "C" int tl_christofides(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos, float *out_cost,
                               tl_stats *stats)
{
    TL_ENTER(c);
    if (!c || (!xy && !dm_packed) || (!out_pos && n)) return fail(c, TL_ERR_BADARG, "tl_christofides: NULL argument");
    const char *who = "tl_christofides";
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc;
    bool done;
    // christofides.rs:24-30: n < 4 is the cities in file order
    if ((rc = limits_and_small(c, who, 3, xy, dm_packed, n, out_pos, out_cost, stats, t0, &done)) || done) return rc;
    const uint32_t cap = greedy_band_cap(c->lds_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->out_pos, (size_t)n * 4)) || (rc = ensure(c, c->out_cost, 4)) || (rc = ensure(c, c->work, greedy_ws_bytes(n, cap))))
        return rc;
    const float2 *dxy = nullptr;
    const float *ddm = nullptr;
    if ((rc = upload_input(c, xy, dm_packed, n, &dxy, &ddm))) return rc;
    const GreedyWs w = greedy_ws_layout(c->work.p, n, cap);
    const ChrWs cw = chr_ws_layout(w, n);
    Event prim_done;
    HIPCHK(c, hipEventCreate(&prim_done.e));
    // steps 1 and 2: the tree, then its odd vertices as the bands' start state
    c->ev_valid = false;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_chr_prim(cw, dxy, ddm, n, c->lds_bytes, c->stream));
    HIPCHK(c, hipEventRecord(prim_done.e, c->stream));
    HIPCHK(c, launch_chr_odd(w, cw, n, c->stream));
    std::vector<uint16_t> order(n), parent(n);
    uint32_t st[8], bad[2];
    HIPCHK(c, hipMemcpyAsync(order.data(), cw.order, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(parent.data(), cw.parent, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bad, cw.status, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, w.state, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad[0])
        return fail(c, TL_ERR_UNSUPPORTED,
                    "%s: no distance below f32::MAX reaches position %u (all NaN or too large): the spanning tree is incomplete and the "
                    "reference's result is not a tour",
                    who, bad[1]);
    // step 3: the greedy matching of the k odd vertices, k / 2 pairs
    const uint32_t k_odd = st[4], npairs = k_odd / 2;
    if (k_odd & 1u) return fail(c, TL_ERR_HIP, "%s: %u odd-degree vertices", who, k_odd);
    uint64_t bands = 0;
    if ((rc = run_bands(c, who, w, dxy, ddm, n, kGeKeyMatching, npairs, st, &bands))) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> pairs(2 * (size_t)npairs);
    if (npairs) HIPCHK(c, hipMemcpyAsync(pairs.data(), w.slots, (size_t)npairs * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t a = 0; a < 2 * npairs; ++a)
        if (pairs[a] >= n) return fail(c, TL_ERR_HIP, "%s: matched position %u of n=%u", who, pairs[a], n);
    // steps 4 to 6 on the host: O(n) dependent pointer chasing whose order is the result
    euler_shortcut(n, order.data(), parent.data(), pairs.data(), npairs, out_pos);
    if (out_cost) {
        HIPCHK(c, hipMemcpyAsync(c->out_pos.p, out_pos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_tour_length(dxy, ddm, n, (const uint32_t *)c->out_pos.p, (float *)c->out_cost.p, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_cost, c->out_cost.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (stats) {
        float ms = 0.f, prim_ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        HIPCHK(c, hipEventElapsedTime(&prim_ms, c->ev0, prim_done.e));
        stats->sweeps = bands;
        stats->candidates = (uint64_t)st[2] << 32 | st[1];
        stats->moves = n;
        stats->reversed = (uint64_t)((double)prim_ms * 1e6);  // the tree's launch, ns (the field has no other meaning for a construction)
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return TL_OK;
}

extern "C" int tl_greedy_edge(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos, float *out_cost,
                              tl_stats *stats)
{
    TL_ENTER(c);
    if (!c || (!xy && !dm_packed) || (!out_pos && n)) return fail(c, TL_ERR_BADARG, "tl_greedy_edge: NULL argument");
    return construct(c, "tl_greedy_edge", false, 0, xy, dm_packed, n, out_pos, out_cost, stats);
}

extern "C" int tl_savings_hub(const float *xy, uint32_t n, uint32_t *out_hub)
{
    if (!out_hub || (!xy && n)) return TL_ERR_BADARG;
    *out_hub = savings_hub(xy, n);
    return TL_OK;
}

extern "C" int tl_savings(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, uint32_t hub, uint32_t *out_pos, float *out_cost,
                          uint32_t *out_hub, tl_stats *stats)
{
    TL_ENTER(c);
    if (!c || (!xy && (!dm_packed || hub == TL_SAVINGS_HUB_AUTO)) || (!out_pos && n)) return fail(c, TL_ERR_BADARG, "tl_savings: NULL argument");
    if (hub == TL_SAVINGS_HUB_AUTO) hub = savings_hub(xy, n);  // 0 at n = 0
    else if (hub >= n) return fail(c, TL_ERR_BADARG, "tl_savings: hub=%u is not a position of n=%u cities", hub, n);
    if (out_hub) *out_hub = hub;
    return construct(c, "tl_savings", true, hub, xy, dm_packed, n, out_pos, out_cost, stats);
}
