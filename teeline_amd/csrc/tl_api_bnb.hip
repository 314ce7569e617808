// tl_api_bnb.hip — tl_branch_and_bound, its sequential restatement tl_branch_and_bound_host and tl_branch_and_bound_plan: the host
// side of csrc/branch_and_bound.hip.  The restatement is ONE text for three uses: the CPU entry, the frontier the
// device entry queues, and the timing baseline.  The device entry owns the queue: it builds the frontier, relaunches the bounded
// kernel, and while the queue is shorter than the waves it splits untried siblings off the unfinished searches.
#include "tl_api_common.h"

#include <algorithm>
#include <cfloat>

using namespace tl;
using namespace tlapi;

namespace {

using Clock = std::chrono::steady_clock;

inline uint32_t f_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
inline float bits_f(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct Inst {
    float D[64 * 64];
    uint64_t nk[64];
    uint32_t n = 0, start = 0;
    uint64_t full = 0;
    double factor = 1.0;
};

// D with tl_bellman_karp's bits (dist() of tl_device.h: fl(fl(dx dx) + fl(dy dy)), a correctly rounded root; this file is built
// without contraction as the kernels are — or the packed triangle), the candidate masks, the prune's factor.
int build_instance(tl_ctx *c, const float *xy, const float *dm, uint32_t n, uint32_t start, uint32_t K, Inst &I)
{
    I.n = n;
    I.start = start;
    I.full = n >= 64u ? ~(uint64_t)0 : (((uint64_t)1 << n) - 1u);
    I.factor = 1.0 + (double)(n + 1u) * 0x1p-23;
    memset(I.D, 0, sizeof(I.D));
    for (uint32_t a = 1; a < n; ++a)
        for (uint32_t b = 0; b < a; ++b) {
            float d;
            if (dm) d = dm[(size_t)a * (a - 1) / 2 + b];
            else {
                const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
                const float sx = dx * dx, sy = dy * dy;
                d = sqrtf(sx + sy);
            }
            if (!(d >= 0.0f) || std::signbit(d) || !(d < FLT_MAX))
                return fail(c, TL_ERR_UNSUPPORTED, "tl_branch_and_bound: the distance of positions %u and %u (%g) is NaN, negative or >= f32::MAX", a, b,
                            (double)d);
            I.D[a * 64 + b] = I.D[b * 64 + a] = d;
        }
    for (uint32_t cty = 0; cty < 64; ++cty) I.nk[cty] = I.full;
    if (K > 0 && K < n)
        for (uint32_t cty = 0; cty < n; ++cty) {
            std::vector<std::pair<uint32_t, uint32_t>> ord;
            for (uint32_t j = 0; j < n; ++j)
                if (j != cty) ord.emplace_back(f_bits(I.D[cty * 64 + j]), j);
            std::sort(ord.begin(), ord.end());
            uint64_t m = (uint64_t)1 << cty;
            for (uint32_t t = 0; t + 1 < K; ++t) m |= (uint64_t)1 << ord[t].second;
            I.nk[cty] = m;
        }
    return TL_OK;
}

template <class P>
float tour_len(const Inst &I, const P *p)
{
    const uint32_t n = I.n;
    float total = I.D[(uint32_t)p[n - 1] * 64 + (uint32_t)p[0]];
    for (uint32_t a = 0; a + 1 < n; ++a) total += I.D[(uint32_t)p[a] * 64 + (uint32_t)p[a + 1]];
    return total;
}

struct Best {
    bool has = false;
    uint32_t bits = 0;
    uint8_t p[64];
    template <class P>
    void offer(uint32_t b, const P *q, uint32_t n)  // kept if it beats the record by (L, p)
    {
        if (has) {
            if (b > bits) return;
            if (b == bits) {
                uint32_t a = 0;
                while (a < n && (uint32_t)q[a] == p[a]) ++a;
                if (a == n || (uint32_t)q[a] > p[a]) return;
            }
        }
        has = true;
        bits = b;
        for (uint32_t a = 0; a < n; ++a) p[a] = (uint8_t)q[a];
    }
};

struct Budget {
    uint64_t max_nodes = 0;
    bool timed = false;
    Clock::time_point deadline;
    bool spent(uint64_t nodes) const { return (max_nodes && nodes >= max_nodes) || (timed && Clock::now() >= deadline); }
};

// The search, one node at a time.  limit_len = 0: to the leaves.  Otherwise every surviving prefix of limit_len positions is put
// into `items` instead of being expanded (2 <= limit_len <= n - 1: no leaf is reached).
struct HostSearch {
    const Inst &I;
    uint32_t ub_bits, ub0_bits;
    bool has_start;
    Best best;
    uint64_t nodes = 0, leaves = 0;
    uint8_t path[64];
    uint64_t untried[65];
    double cost[64], mst[65];

    HostSearch(const Inst &i, bool hs, uint32_t ub0) : I(i), ub_bits(hs ? ub0 : f_bits(FLT_MAX)), ub0_bits(ub0), has_start(hs) {}

    double prim(uint64_t unv) const
    {
        uint32_t key[64];
        for (uint64_t m = unv; m; m &= m - 1) {
            const uint32_t v = (uint32_t)__builtin_ctzll(m);
            key[v] = f_bits(I.D[I.start * 64 + v]);
        }
        double total = 0.0;
        for (uint64_t left = unv; left;) {
            uint32_t u = 0, mn = 0xFFFFFFFFu;
            for (uint64_t m = left; m; m &= m - 1) {
                const uint32_t v = (uint32_t)__builtin_ctzll(m);
                if (key[v] < mn) {
                    mn = key[v];
                    u = v;
                }
            }
            total += (double)bits_f(mn);
            left &= ~((uint64_t)1 << u);
            for (uint64_t m = left; m; m &= m - 1) {
                const uint32_t v = (uint32_t)__builtin_ctzll(m);
                const uint32_t d = f_bits(I.D[u * 64 + v]);
                if (d < key[v]) key[v] = d;
            }
        }
        return total;
    }
    void expand(uint32_t k, uint64_t V)
    {
        const uint64_t unv = I.full & ~V;
        mst[k] = prim(unv);
        const uint64_t cand = I.nk[path[k - 1]] & unv;
        untried[k] = cand ? cand : unv;
        ++nodes;
    }
    // false: the budget ended the search
    bool run(uint32_t limit_len, std::vector<BnbItem> *items, const Budget &budget)
    {
        const uint32_t n = I.n;
        path[0] = (uint8_t)I.start;
        cost[0] = 0.0;
        uint64_t V = (uint64_t)1 << I.start;
        uint32_t k = 1;
        expand(k, V);
        for (;;) {
            const uint64_t U = untried[k];
            if (!U) {
                if (k == 1) return true;
                --k;
                V &= ~((uint64_t)1 << path[k]);
                continue;
            }
            const uint32_t prev = path[k - 1];
            uint32_t c = 0, mn = 0xFFFFFFFFu;
            for (uint64_t m = U; m; m &= m - 1) {
                const uint32_t v = (uint32_t)__builtin_ctzll(m);
                const uint32_t d = f_bits(I.D[prev * 64 + v]);
                if (d < mn) {
                    mn = d;
                    c = v;
                }
            }
            const double nc = cost[k - 1] + (double)bits_f(mn);
            if (nc + mst[k] > (double)bits_f(ub_bits) * I.factor) {
                untried[k] = 0;
                continue;
            }
            untried[k] = U & ~((uint64_t)1 << c);
            path[k] = (uint8_t)c;
            cost[k] = nc;
            if (k + 1 == n) {
                const uint32_t Lb = f_bits(tour_len(I, path));
                ++leaves;
                if (Lb <= ub_bits) {
                    ub_bits = Lb;
                    if (!has_start || Lb < ub0_bits) best.offer(Lb, path, n);
                }
                continue;
            }
            if (items && k + 1 == limit_len) {
                BnbItem it;
                memset(&it, 0, sizeof(it));
                memcpy(it.path, path, limit_len);
                it.depth = limit_len;
                items->push_back(it);
                continue;
            }
            if (budget.spent(nodes)) return false;
            V |= (uint64_t)1 << c;
            ++k;
            expand(k, V);
        }
    }
};

struct Event {  // a HIP event of one call
    hipEvent_t e = nullptr;
    ~Event()
    {
        if (e) (void)hipEventDestroy(e);
    }
};

// what both entries check before anything else; *trivial: the call is answered (n <= 1)
int bnb_enter(tl_ctx *c, const float *xy, const float *dm, uint32_t n, const uint32_t *init_pos, const tl_bnb_opts &o, uint32_t *out_pos,
              float *out_cost, uint32_t *out_proved, uint32_t *out_improved, tl_bnb_stats *stats, bool *trivial)
{
    *trivial = false;
    if ((!xy && !dm && n > 1) || (!out_pos && n)) return fail(c, TL_ERR_BADARG, "tl_branch_and_bound: NULL argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n > TL_BNB_MAX_N)
        return fail(c, TL_ERR_UNSUPPORTED, "tl_branch_and_bound: n=%u > %u (TL_BNB_MAX_N: one wave's lanes, one 64-bit mask)", n, TL_BNB_MAX_N);
    if (n && o.start >= n) return fail(c, TL_ERR_BADARG, "tl_branch_and_bound: start=%u is no position of n=%u", o.start, n);
    if (init_pos && n && !is_permutation(init_pos, n)) return fail(c, TL_ERR_BADARG, "tl_branch_and_bound: init_pos is not a permutation of 0..n-1");
    if (n <= 1) {
        if (n) out_pos[0] = 0;
        if (out_cost) *out_cost = 0.0f;
        if (out_proved) *out_proved = 1;
        if (out_improved) *out_improved = 0;
        *trivial = true;
    }
    return TL_OK;
}

// the call's ending: R against the start tour, the outputs
int bnb_finish(tl_ctx *c, const Inst &I, const Best &best, const uint32_t *init_pos, bool proved, uint32_t *out_pos, float *out_cost,
               uint32_t *out_proved, uint32_t *out_improved)
{
    const uint32_t n = I.n;
    uint32_t improved = 0;
    if (best.has) {  // with a start tour only leaves with L < L(init_pos) were kept
        for (uint32_t a = 0; a < n; ++a) out_pos[a] = best.p[a];
        improved = 1;
    } else if (init_pos) {
        for (uint32_t a = 0; a < n; ++a) out_pos[a] = init_pos[a];
    } else if (proved) {
        return fail(c, TL_ERR_UNSUPPORTED, "tl_branch_and_bound: no tour of this instance has a length <= f32::MAX");
    } else {  // the budget ended the search before its first leaf: start, then the other positions in order
        uint32_t at = 0;
        out_pos[at++] = I.start;
        for (uint32_t a = 0; a < n; ++a)
            if (a != I.start) out_pos[at++] = a;
    }
    if (!is_permutation(out_pos, n)) return fail(c, TL_ERR_HIP, "tl_branch_and_bound: the result is no permutation");
    const float L = tour_len(I, out_pos);
    if (best.has && f_bits(L) != best.bits) return fail(c, TL_ERR_HIP, "tl_branch_and_bound: the recorded length is not the route's");
    if (out_cost) *out_cost = L;
    if (out_proved) *out_proved = proved ? 1u : 0u;
    if (out_improved) *out_improved = improved;
    return TL_OK;
}

Budget make_budget(const tl_bnb_opts &o, Clock::time_point t0)
{
    Budget b;
    b.max_nodes = o.max_nodes;
    b.timed = o.time_limit_ms != 0;
    b.deadline = t0 + std::chrono::milliseconds(o.time_limit_ms);
    return b;
}

double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

void plan(uint32_t n, int cus, uint32_t *workgroups, uint32_t *frontier_depth, uint32_t *nodes_per_launch)
{
    // waves per CU: small instances finish in a few thousand nodes and a launch loads and stores every wave's state
    const uint32_t cu = (uint32_t)(cus > 0 ? cus : 256);
    *workgroups = n <= 20 ? std::max(1u, cu / 4) : n <= 32 ? cu : n <= 40 ? 2 * cu : 4 * cu;
    *frontier_depth = n >= 4 ? std::min(2u, n - 2) : 1u;
    // a node is at most n Prim steps, so the slice shrinks with n.  Measured on an MI355X: a launch lasts 7 ms at n = 26, 20 to 33 ms
    // at n = 33 to 48 and 45 ms at n = 64 — above the 10 ms aimed at; a smaller slice was not measured
    *nodes_per_launch = 4096u * 64u / std::max(n, 8u);
}

}  // namespace

extern "C" int tl_branch_and_bound_plan(uint32_t n, int cus, int lds_bytes, int *threads, int *workgroups, uint32_t *frontier_depth,
                                        uint32_t *nodes_per_launch)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    if (n > TL_BNB_MAX_N) return TL_ERR_UNSUPPORTED;
    uint32_t wg, fd, npl;
    plan(n, cus, &wg, &fd, &npl);
    if (threads) *threads = kBnbThreads;
    if (workgroups) *workgroups = (int)wg;
    if (frontier_depth) *frontier_depth = fd;
    if (nodes_per_launch) *nodes_per_launch = npl;
    return TL_OK;
}

extern "C" int tl_branch_and_bound_host(const float *xy, const float *dm_packed, uint32_t n, const uint32_t *init_pos, const tl_bnb_opts *opts,
                                        uint32_t *out_pos, float *out_cost, uint32_t *out_proved, uint32_t *out_improved, tl_bnb_stats *stats)
{
    const auto t0 = Clock::now();
    const tl_bnb_opts o = opts ? *opts : tl_bnb_opts{};
    bool trivial;
    int rc;
    if ((rc = bnb_enter(nullptr, xy, dm_packed, n, init_pos, o, out_pos, out_cost, out_proved, out_improved, stats, &trivial)) || trivial) return rc;
    auto I = std::make_unique<Inst>();
    if ((rc = build_instance(nullptr, xy, dm_packed, n, o.start, o.n_nearest, *I))) return rc;
    HostSearch S(*I, init_pos != nullptr, init_pos ? f_bits(tour_len(*I, init_pos)) : 0u);
    const bool proved = S.run(0, nullptr, make_budget(o, t0));
    if (stats) {
        stats->nodes = S.nodes;
        stats->leaves = S.leaves;
        stats->total_ms = ms_since(t0);
    }
    return bnb_finish(nullptr, *I, S.best, init_pos, proved, out_pos, out_cost, out_proved, out_improved);
}

extern "C" int tl_branch_and_bound(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, const uint32_t *init_pos, const tl_bnb_opts *opts,
                                   uint32_t *out_pos, float *out_cost, uint32_t *out_proved, uint32_t *out_improved, tl_bnb_stats *stats)
{
    TL_ENTER(c);
    if (!c) return fail(c, TL_ERR_BADARG, "tl_branch_and_bound: NULL context");
    const auto t0 = Clock::now();
    const tl_bnb_opts o = opts ? *opts : tl_bnb_opts{};
    bool trivial;
    int rc;
    if ((rc = bnb_enter(c, xy, dm_packed, n, init_pos, o, out_pos, out_cost, out_proved, out_improved, stats, &trivial)) || trivial) return rc;
    auto I = std::make_unique<Inst>();
    if ((rc = build_instance(c, xy, dm_packed, n, o.start, o.n_nearest, *I))) return rc;
    const bool has_start = init_pos != nullptr;
    const uint32_t ub0 = has_start ? f_bits(tour_len(*I, init_pos)) : 0u;
    const Budget budget = make_budget(o, t0);
    HostSearch S(*I, has_start, ub0);
    tl_bnb_stats st;
    memset(&st, 0, sizeof(st));
    Best best;
    bool proved;
    if (n <= 3) {  // one or two tours: nothing for a device to do
        proved = S.run(0, nullptr, budget);
        best = S.best;
    } else {
        uint32_t wg, fd, npl;
        plan(n, c->cus, &wg, &fd, &npl);
        if (o.workgroups) wg = std::min(o.workgroups, 16384u);
        if (o.frontier_depth) fd = o.frontier_depth;
        if (o.nodes_per_launch) npl = o.nodes_per_launch;
        fd = std::max(1u, std::min(fd, n - 2));
        std::vector<BnbItem> items;
        proved = S.run(1 + fd, &items, budget);
        st.queue_start = st.queue_end = items.size();
        if (proved && !items.empty()) {
            const uint32_t waves = wg * kBnbWavesPerGroup;
            const uint32_t cap = (uint32_t)std::max<size_t>(items.size(), (size_t)waves + 64);
            HIPCHK(c, hipSetDevice(c->device));
            if ((rc = ensure(c, c->work, bnb_ws_bytes(waves, cap)))) return rc;
            const BnbWs w = bnb_ws_layout(c->work.p, waves, cap);
            BnbCtrl ctrl;
            memset(&ctrl, 0, sizeof(ctrl));
            ctrl.ub_bits = has_start ? ub0 : f_bits(FLT_MAX);
            ctrl.queue_len = (uint32_t)items.size();
            // the searches start empty: everything behind the queue is zero
            HIPCHK(c, hipMemsetAsync(w.hdr, 0, (size_t)((unsigned char *)c->work.p + bnb_ws_bytes(waves, cap) - (unsigned char *)w.hdr), c->stream));
            HIPCHK(c, hipMemcpyAsync(w.D, I->D, sizeof(I->D), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(w.nk, I->nk, sizeof(I->nk), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(w.ctrl, &ctrl, sizeof(ctrl), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(w.queue, items.data(), items.size() * sizeof(BnbItem), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            Event e0, e1;
            HIPCHK(c, hipEventCreate(&e0.e));
            HIPCHK(c, hipEventCreate(&e1.e));
            c->ev_valid = false;
            std::vector<BnbWaveHdr> hdr(waves);
            std::vector<uint32_t> wpath((size_t)waves * 64);
            std::vector<uint64_t> wunt((size_t)waves * 64);
            uint64_t idle_before = 0;
            proved = false;
            for (;;) {
                // the slice: the plan's, or what is left of the node budget shared out over the waves
                uint64_t slice = npl;
                const uint64_t done = S.nodes + ctrl.nodes;
                if (budget.max_nodes) slice = std::max<uint64_t>(1, std::min<uint64_t>(slice, (budget.max_nodes - std::min(done, budget.max_nodes)) / waves));
                const auto tl0 = Clock::now();
                HIPCHK(c, hipEventRecord(e0.e, c->stream));
                HIPCHK(c, launch_bnb(w, n, o.start, (uint32_t)slice, wg, ub0, has_start, I->factor, c->stream));
                HIPCHK(c, hipEventRecord(e1.e, c->stream));
                HIPCHK(c, hipMemcpyAsync(&ctrl, w.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                float ms = 0.f;
                HIPCHK(c, hipEventElapsedTime(&ms, e0.e, e1.e));
                st.kernel_ms += ms;
                st.max_launch_ms = std::max(st.max_launch_ms, ms_since(tl0));
                ++st.launches;
                st.wave_launches += waves;
                const uint64_t idle_now = ctrl.idle - idle_before;
                idle_before = ctrl.idle;
                const uint32_t taken = std::min(ctrl.ticket, ctrl.queue_len);
                const uint32_t left = ctrl.queue_len - taken;
                if (left == 0 && idle_now == waves) {  // every wave ended without a subtree and found the queue empty
                    proved = true;
                    break;
                }
                if (budget.spent(S.nodes + ctrl.nodes)) break;
                if (left >= waves) continue;
                // the queue is shorter than the waves: untried siblings of the shallowest levels of unfinished searches become
                // items of their own (a level at a time, the searches in turn) until every wave can have one
                HIPCHK(c, hipMemcpyAsync(hdr.data(), w.hdr, hdr.size() * sizeof(BnbWaveHdr), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(wpath.data(), w.path, wpath.size() * 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(wunt.data(), w.untried, wunt.size() * 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                std::vector<BnbItem> fresh;
                for (bool any = true; any && left + fresh.size() < waves;) {
                    any = false;
                    for (uint32_t v = 0; v < waves && left + fresh.size() < waves; ++v) {
                        const BnbWaveHdr &h = hdr[v];
                        if (!h.active) continue;
                        if (h.k >= n || h.base < 1 || h.base > h.k) return fail(c, TL_ERR_HIP, "tl_branch_and_bound: a wave's search state is out of range");
                        for (uint32_t l = h.base; l <= h.k && l + 2 <= n; ++l) {  // (a prefix of n positions is a leaf, not a subtree)
                            uint64_t &U = wunt[(size_t)v * 64 + l];
                            if (!U) continue;
                            for (uint64_t m = U; m; m &= m - 1) {
                                BnbItem it;
                                memset(&it, 0, sizeof(it));
                                for (uint32_t a = 0; a < l; ++a) it.path[a] = (uint8_t)wpath[(size_t)v * 64 + a];
                                it.path[l] = (uint8_t)__builtin_ctzll(m);
                                it.depth = l + 1;
                                fresh.push_back(it);
                            }
                            U = 0;
                            any = true;
                            break;
                        }
                    }
                }
                if (!fresh.empty()) {
                    std::vector<BnbItem> q(items.begin() + taken, items.begin() + ctrl.queue_len);
                    q.insert(q.end(), fresh.begin(), fresh.end());
                    if (q.size() > cap) return fail(c, TL_ERR_HIP, "tl_branch_and_bound: the queue outgrew its buffer");
                    items.swap(q);
                    st.queue_end += fresh.size();
                    ctrl.ticket = 0;
                    ctrl.queue_len = (uint32_t)items.size();
                    HIPCHK(c, hipMemcpyAsync(w.queue, items.data(), items.size() * sizeof(BnbItem), hipMemcpyHostToDevice, c->stream));
                    HIPCHK(c, hipMemcpyAsync(w.untried, wunt.data(), wunt.size() * 8, hipMemcpyHostToDevice, c->stream));
                } else {
                    ctrl.ticket = taken;
                }
                // ticket and queue_len are the first words behind ub_bits; the bound and the counters stay the device's
                HIPCHK(c, hipMemcpyAsync(&w.ctrl->ticket, &ctrl.ticket, 8, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
            // the waves' records: R is the least of them by (L, p)
            std::vector<uint32_t> rec((size_t)waves * 64);
            HIPCHK(c, hipMemcpyAsync(hdr.data(), w.hdr, hdr.size() * sizeof(BnbWaveHdr), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(rec.data(), w.rec, rec.size() * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (uint32_t v = 0; v < waves; ++v)
                if (hdr[v].rec_has) {
                    for (uint32_t a = 0; a < n; ++a)
                        if (rec[(size_t)v * 64 + a] >= n) return fail(c, TL_ERR_HIP, "tl_branch_and_bound: position %u of n=%u in a record", rec[(size_t)v * 64 + a], n);
                    best.offer(hdr[v].rec_bits, &rec[(size_t)v * 64], n);
                }
            st.nodes = ctrl.nodes;
            st.leaves = ctrl.leaves;
            st.idle_wave_launches = ctrl.idle;
        }
    }
    st.nodes += S.nodes;
    st.leaves += S.leaves;
    st.total_ms = ms_since(t0);
    if (stats) *stats = st;
    return bnb_finish(c, *I, best, init_pos, proved, out_pos, out_cost, out_proved, out_improved);
}
