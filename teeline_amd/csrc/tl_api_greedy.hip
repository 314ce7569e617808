// tl_api_greedy.hip — tl_greedy_edge: greedy-edge construction (greedy_edge.rs:21-65), and tl_savings / tl_savings_hub: savings
// construction (savings.rs:34-163) — the host side of csrc/greedy_edge.hip.  Both run the same bands; only the key differs.
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
int band_threshold(tl_ctx *c, const GreedyWs &w, const float2 *dxy, const float *ddm, uint32_t f, uint64_t t_prev, int blocks, bool savings,
                   std::vector<uint32_t> &hist, uint64_t *t_out, uint64_t *count)
{
    uint64_t prefix = 0, t = t_prev, cum = 0;
    const uint64_t cap = w.cap;
    for (int lvl = 0; lvl < 6; ++lvl) {
        const uint32_t wd = kGeWidth[lvl], sh = kGeShift[lvl];
        HIPCHK(c, launch_greedy_hist(w, dxy, ddm, f, t_prev, prefix, sh, wd, blocks, savings, c->stream));
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

// The construction both entries share (the caller holds the context): savings = false walks the edges by length, true by their
// saving against `hub` (< n).
int construct(tl_ctx *c, const char *who, bool savings, uint32_t hub, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos,
              float *out_cost, tl_stats *stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n > kGeMaxN) return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u > %u (positions are 16-bit in the sort keys)", who, n, kGeMaxN);
    const uint32_t cap = greedy_band_cap(c->lds_bytes);
    if ((size_t)n * 2 + 1024 > (size_t)c->lds_bytes)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u exceeds the LDS-resident end table (%d bytes of LDS)", who, n, c->lds_bytes);
    int rc;
    if (n <= 2) {  // greedy_edge.rs:33-39, savings.rs:46-52: the cities in file order
        for (uint32_t k = 0; k < n; ++k) out_pos[k] = k;
        if (out_cost && (rc = tl_tour_length(c, dm_packed ? nullptr : xy, dm_packed, n, out_pos, out_cost))) return rc;
        if (stats) {
            stats->moves = n;
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return TL_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->out_pos, (size_t)n * 4)) || (rc = ensure(c, c->out_cost, 4)) || (rc = ensure(c, c->work, greedy_ws_bytes(n, cap))))
        return rc;
    const float2 *dxy = nullptr;
    const float *ddm = nullptr;
    if (dm_packed) {
        const size_t b = (size_t)n * (n - 1) / 2 * 4;
        if ((rc = ensure(c, c->dm, b))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->dm.p, dm_packed, b, hipMemcpyHostToDevice, c->stream));
        ddm = (const float *)c->dm.p;
    } else {
        if ((rc = ensure(c, c->xy, (size_t)n * 8))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->xy.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        dxy = (const float2 *)c->xy.p;
    }
    const GreedyWs w = greedy_ws_layout(c->work.p, n, cap);
    const int blocks = (c->cus > 0 ? c->cus : 256) * 8;
    std::vector<uint32_t> hist(4096);
    uint32_t st[8] = {0, 0, 0, 0, n, 0, 0, 0};
    c->ev_valid = false;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_greedy_init(w, n, c->stream));
    if (savings) HIPCHK(c, launch_savings_dh(w, dxy, ddm, n, hub, c->stream));
    uint64_t t_prev = 0, bands = 0;  // every key is > 0 (j >= 1 in its low bits)
    while (st[0] < n) {
        uint64_t t = 0, count = 0;
        if ((rc = band_threshold(c, w, dxy, ddm, st[4], t_prev, blocks, savings, hist, &t, &count))) return rc;
        if (count == 0)  // cannot happen on a complete graph (graph.rs:85-96); refuse rather than loop
            return fail(c, TL_ERR_HIP, "%s: no edge left after %u of %u accepted", who, st[0], n);
        HIPCHK(c, launch_greedy_band(w, dxy, ddm, n, st[4], t_prev, t, blocks, savings, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, w.state, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (st[3] != count)
            return fail(c, TL_ERR_HIP, "%s: band %llu holds %u keys, its histogram %llu", who, (unsigned long long)bands, st[3],
                        (unsigned long long)count);
        ++bands;
        t_prev = t;
        if (st[0] < n && t == ~(uint64_t)0) return fail(c, TL_ERR_HIP, "%s: every edge walked, %u of %u accepted", who, st[0], n);
    }
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

}  // namespace

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
