// ant_colony.hip — the ant colony solver (ant_colony.rs:97-252): R independent runs (colonies), the run a grid dimension, the matrices
// tau, eta^beta and W = tau^alpha eta^beta (f32, n x n each) and the ants' tables in the context's workspace, three launches per epoch.
//
// The draws of ant a of epoch g are a pure function of (seed, run, g, a, step) (aco_spec.h: this project's specification — the
// reference draws from an unseeded thread RNG), and within an epoch the ants only read the matrices: all of them walk at once.
//
//   k_aco_init       one workgroup per run: the start tour (given, or ga_spec.h's Fisher-Yates pass by one lane), its cost in the
//                    reference's order, tau0, tau_min, and the start tour as "ant 0" for the deposit before epoch 0.
//   k_aco_fill       one workgroup per (row, run): tau = tau0, eta^beta = aco_pow(1 / max(d, 1e-6), beta), the diagonal 0.
//   k_aco_construct  one workgroup per (group of up to 64 ants, run): wave 0 is the CHAIN wave, one ant per lane, all ants at the same
//                    step; waves 1 .. 4 are STAGERS.  A selection is a sequential f32 sum over the n cities of row `cur` of W with
//                    the visited cities' weights forced to +0.0f (aco_spec.h: why that is exact).  For a chunk of 64 cities and
//                    every ant the stagers write that masked row segment (a coalesced 256-byte read) into an LDS tile whose rows
//                    are 65 words apart — lane a reading column i hits bank (a + i) mod 32, conflict-free for ds_read_b32 — and the
//                    tile is double buffered: the chain wave adds chunk c while chunk c + 1 is staged, one workgroup barrier per
//                    chunk, no flags.  The chain wave keeps each chunk's end prefix (LDS, 4 bytes per city); with the total known,
//                    target = r1 total, the first chunk whose end prefix exceeds the target is staged again — each ant its own —
//                    and re-added from its start prefix, which finds the city: the reference's second walk bit for bit, at
//                    n + 64 serial adds.  A ballot decides whether any ant needs the eta-only pass.  The visited bits live in LDS
//                    (8 bytes per city); tour, successor and predecessor go to the workspace as the ant moves; the tour cost is
//                    the same chain over staged edge lengths.
//   k_aco_best       one workgroup per run: the ants whose cost is below the best so far, strictly and in ant order; the last of
//                    them becomes the best tour; the trace record and the route log of run 0.
//   k_aco_update     one workgroup per (block of rows, run), the rows in LDS: evaporate and floor; one thread per row applies that
//                    row's 2 A deposits in ant order from the successor and predecessor tables (a cell is touched at most once per
//                    ant, so each cell's adds happen in the reference's order, without atomics); W = aco_pow(tau, alpha) eta.
//                    With `pre` it is the deposit of the initial tour before epoch 0: one ant (or none), no evaporation.
#include "aco_spec.h"
#include "swarm_tour.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr uint32_t kAcoChunk = 64;     // cities per tile: one stager lane each
constexpr uint32_t kAcoPitch = 65;     // words between two ants' tile rows
constexpr uint32_t kAcoStagers = 4;    // stager waves
constexpr uint32_t kAcoThreads = 64u * (1u + kAcoStagers);
constexpr size_t kAcoFixedBytes = 768;  // hdr[64] | cur[64] | cst[64]
constexpr size_t kAcoTileBytes = 64 * kAcoPitch * 4;
constexpr uint32_t kAcoNone = 0xFFFFFFFFu;

struct AcoLds {
    uint32_t *hdr, *cur, *cst, *vis;
    float *tile[2], *prefix;
    uint32_t vw;  // words of an ant's visited bits
    __device__ AcoLds(unsigned char *smem, uint32_t n)
    {
        hdr = reinterpret_cast<uint32_t *>(smem);
        cur = hdr + 64;
        cst = hdr + 128;
        tile[0] = reinterpret_cast<float *>(smem + kAcoFixedBytes);
        tile[1] = tile[0] + 64 * kAcoPitch;
        prefix = tile[1] + 64 * kAcoPitch;
        vw = (n + 31u) / 32u;
        vis = reinterpret_cast<uint32_t *>(prefix + (size_t)((n + kAcoChunk - 1u) / kAcoChunk) * 64u);
    }
};

__device__ __forceinline__ uint32_t aco_free_bits(const uint32_t *vis, uint32_t w, uint32_t vw, uint32_t n)
{
    uint32_t free = ~vis[w];
    if (w + 1u == vw && (n & 31u)) free &= (1u << (n & 31u)) - 1u;
    return free;
}
__device__ __forceinline__ uint32_t aco_first_unvisited(const uint32_t *vis, uint32_t vw, uint32_t n)
{
    for (uint32_t w = 0; w < vw; ++w) {
        const uint32_t free = aco_free_bits(vis, w, vw, n);
        if (free) return w * 32u + (uint32_t)__ffs((int)free) - 1u;
    }
    return 0u;
}
__device__ __forceinline__ uint32_t aco_last_unvisited(const uint32_t *vis, uint32_t vw, uint32_t n)
{
    for (uint32_t w = vw; w-- > 0u;) {
        const uint32_t free = aco_free_bits(vis, w, vw, n);
        if (free) return w * 32u + 31u - (uint32_t)__clz((int)free);
    }
    return 0u;
}

// The sequential sum of stage(a, v), v = 0 .. 64 nc - 1, for every ant a < na at once: lane a of wave 0 adds, the stagers fill the
// tiles one chunk ahead.  keep: the end prefix of every chunk stays in L.prefix.  Called by the whole workgroup; the tiles must be
// free (a barrier since their last read); ends behind a barrier.
template <class F>
__device__ __forceinline__ float aco_sum_pass(const AcoLds &L, uint32_t nc, uint32_t na, float acc, bool keep, F stage)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool chain = wave == 0u;
    if (!chain)
        for (uint32_t a = wave - 1u; a < na; a += kAcoStagers) L.tile[0][a * kAcoPitch + lane] = stage(a, lane);
    TL_SYNC();
    for (uint32_t c = 0; c < nc; ++c) {
        if (!chain) {
            if (c + 1u < nc) {
                float *t = L.tile[(c + 1u) & 1u];
                for (uint32_t a = wave - 1u; a < na; a += kAcoStagers) t[a * kAcoPitch + lane] = stage(a, (c + 1u) * kAcoChunk + lane);
            }
        } else {
            // (a lane >= na has no ant: its tile row is unwritten LDS, inside the tile; what it adds up is never used — every caller
            // masks its chain lanes by `active`, lane < na)
            const float *t = L.tile[c & 1u] + lane * kAcoPitch;
#pragma unroll
            for (uint32_t i = 0; i < kAcoChunk; ++i) acc += t[i];
            if (keep) L.prefix[c * 64u + lane] = acc;
        }
        TL_SYNC();
    }
    return acc;
}

// roulette_select's walk (probability.rs:69-79) after aco_sum_pass(keep) of the same stage: the city at which the running sum first
// exceeds the target, or kAcoNone (the walk is exhausted, or !want).  Ends behind a barrier.
template <class F>
__device__ __forceinline__ uint32_t aco_pick_pass(const AcoLds &L, uint32_t nc, uint32_t na, bool want, float target, F stage)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool chain = wave == 0u;
    uint32_t cs = nc;
    if (chain) {
        if (want)
            for (uint32_t c = 0; c < nc; ++c)
                if (L.prefix[c * 64u + lane] > target) {
                    cs = c;
                    break;
                }
        L.cst[lane] = cs < nc ? cs : 0u;
    }
    TL_SYNC();
    if (!chain)
        for (uint32_t a = wave - 1u; a < na; a += kAcoStagers) L.tile[0][a * kAcoPitch + lane] = stage(a, L.cst[a] * kAcoChunk + lane);
    TL_SYNC();
    uint32_t city = kAcoNone;
    if (chain && cs < nc) {
        float acc = cs ? L.prefix[(cs - 1u) * 64u + lane] : 0.0f;
        const float *t = L.tile[0] + lane * kAcoPitch;
#pragma unroll
        for (uint32_t i = 0; i < kAcoChunk; ++i) {
            acc += t[i];
            if (city == kAcoNone && acc > target) city = cs * kAcoChunk + i;
        }
    }
    TL_SYNC();
    return city;
}

struct AcoChoice {
    uint32_t city, path;  // path 0: the primary weights, 1: eta only, 2: the first candidate
    float total, eta_total;
};

// select_next (ant_colony.rs:65-78) for every ant of the group at once; the result is the chain lanes'.  stage_w / stage_e(a, v): the
// masked weight of city v for ant a (+0.0f where visited or v >= n).  Called by the whole workgroup.
template <class FW, class FE>
__device__ __forceinline__ AcoChoice aco_select(const AcoLds &L, uint32_t n, uint32_t na, bool active, float r1, float r2, FW stage_w, FE stage_e)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool chain = (threadIdx.x >> 6) == 0u;
    const uint32_t nc = (n + kAcoChunk - 1u) / kAcoChunk;
    AcoChoice out{kAcoNone, 0u, 0.0f, 0.0f};
    out.total = aco_sum_pass(L, nc, na, 0.0f, true, stage_w);
    const bool ok1 = aco_sum_usable(out.total);
    if (chain) {
        const uint64_t need = __ballot(active && !ok1);
        if (lane == 0u) L.hdr[0] = need != 0ull;
    }
    out.city = aco_pick_pass(L, nc, na, chain && active && ok1, r1 * out.total, stage_w);
    if (L.hdr[0]) {  // (uniform: written before the pick's barriers, next written behind the barriers of the next selection)
        out.eta_total = aco_sum_pass(L, nc, na, 0.0f, true, stage_e);
        const bool ok2 = aco_sum_usable(out.eta_total);
        const uint32_t c2 = aco_pick_pass(L, nc, na, chain && active && !ok1 && ok2, r2 * out.eta_total, stage_e);
        if (chain && active && !ok1) {
            out.path = ok2 ? 1u : 2u;
            out.city = ok2 ? c2 : aco_first_unvisited(L.vis + lane * L.vw, L.vw, n);
        }
    }
    if (chain && active && out.city == kAcoNone) out.city = aco_last_unvisited(L.vis + lane * L.vw, L.vw, n);  // the exhausted walk
    return out;
}

// tour_length's sum (distance_matrix.rs:235-245) of E[k] = d(route[k], route[k + 1]), E[n - 1] the closing edge: one lane
__device__ __forceinline__ float aco_sum_edges(const float *E, uint32_t n)
{
    if (n < 2u) return 0.0f;
    float tot = E[n - 1u];
    for (uint32_t k = 0; k + 1u < n; ++k) tot += E[k];
    return tot;
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_aco_init(AcoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    float *E = reinterpret_cast<float *>(smem);
    uint16_t *r = reinterpret_cast<uint16_t *>(E + n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    const uint32_t *init = A.init ? A.init + (size_t)run * A.init_stride : nullptr;
    for (uint32_t k = tid; k < n; k += nt) r[k] = (uint16_t)(init ? init[k] : k);
    TL_SYNC();
    if (tid == 0 && !init) {
        for (uint32_t j = n - 1u; j >= 1u && j < n; --j) {
            const uint32_t k = sa_position(ga_draw_key(key, aco_shuffle_event(j), kGaSlotShuffle), j + 1u);
            const uint16_t x = r[j];
            r[j] = r[k];
            r[k] = x;
        }
    }
    TL_SYNC();
    uint32_t *out = A.out_pos + (size_t)run * n;
    const size_t ant0 = (size_t)run * A.num_ants * n;
    for (uint32_t k = tid; k < n; k += nt) {
        const uint32_t k1 = k + 1u == n ? 0u : k + 1u;
        out[k] = r[k];
        E[k] = D(r[k], r[k1]);
        if (init) {
            A.tour[ant0 + k] = r[k];
            A.succ[ant0 + r[k]] = r[k1];
            A.pred[ant0 + r[k1]] = r[k];
        }
    }
    const bool routed = A.route_log && run == 0u && A.route_cap > 0u;
    if (routed)
        for (uint32_t k = tid; k < n; k += nt) A.route_log[3u + k] = r[k];
    TL_SYNC();
    if (tid == 0) {
        const float cost = aco_sum_edges(E, n);
        const float tau0 = init && cost > 0.0f ? (float)A.num_ants / cost : 1.0f;
        uint32_t *state = A.state + 8u * (size_t)run;
        state[0] = __builtin_bit_cast(uint32_t, cost);
        state[3] = __builtin_bit_cast(uint32_t, tau0);
        state[4] = __builtin_bit_cast(uint32_t, tau0 * kAcoTauMinRatio);
        A.out_cost[run] = cost;
        A.cost[(size_t)run * A.num_ants] = cost;
        if (routed) {
            A.route_log[0] = kAcoNone;
            A.route_log[1] = kAcoNone;
            A.route_log[2] = __builtin_bit_cast(uint32_t, cost);
        }
    }
}

template <bool DM>
__global__ __launch_bounds__(256) void k_aco_fill(AcoArgs A)
{
    const uint32_t n = A.n, u = blockIdx.x, run = blockIdx.y;
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const float tau0 = __builtin_bit_cast(float, A.state[8u * (size_t)run + 3u]);
    float *tau = A.tau + (size_t)run * A.mat_stride + (size_t)u * n, *eta = A.eta + (size_t)run * A.mat_stride + (size_t)u * n;
    for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
        tau[v] = tau0;
        eta[v] = u == v ? 0.0f : aco_eta(D(u, v), A.beta);
    }
}

template <bool DM>
__global__ __launch_bounds__(kAcoThreads) void k_aco_construct(AcoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, lane = tid & 63u, run = blockIdx.y;
    const bool chain = (tid >> 6) == 0u;
    const AcoLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint32_t a0 = blockIdx.x * 64u, na = A.num_ants - a0 < 64u ? A.num_ants - a0 : 64u;
    const float *W = A.w + (size_t)run * A.mat_stride, *eta = A.eta + (size_t)run * A.mat_stride;
    const size_t base = ((size_t)run * A.num_ants + a0) * n;  // the group's first ant in the tables
    uint16_t *gtour = A.tour + base;
    uint16_t *tour = gtour + (size_t)lane * n, *succ = A.succ + base + (size_t)lane * n, *pred = A.pred + base + (size_t)lane * n;
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    const bool active = chain && lane < na;
    uint32_t *myvis = L.vis + lane * L.vw;

    for (uint32_t i = tid; i < 64u * L.vw; i += kAcoThreads) L.vis[i] = 0u;
    TL_SYNC();
    const uint64_t ev0 = aco_event(A.epoch, A.num_ants, a0 + lane, n, 0u);
    uint32_t cur = 0u, first = 0u, fallbacks = 0u;
    if (chain) {
        if (active) {
            first = cur = sa_position(ga_draw_key(key, ev0, kAcoSlotStart), n);
            myvis[cur >> 5] |= 1u << (cur & 31u);
            tour[0] = (uint16_t)cur;
        }
        L.cur[lane] = cur;
    }
    TL_SYNC();
    const auto masked = [&](const float *M, uint32_t a, uint32_t v) -> float {
        if (v >= n) return 0.0f;
        if ((L.vis[a * L.vw + (v >> 5)] >> (v & 31u)) & 1u) return 0.0f;
        return M[(size_t)L.cur[a] * n + v];
    };
    const auto stage_w = [&](uint32_t a, uint32_t v) { return masked(W, a, v); };
    const auto stage_e = [&](uint32_t a, uint32_t v) { return masked(eta, a, v); };
    for (uint32_t s = 1; s < n; ++s) {
        float r1 = 0.0f, r2 = 0.0f;
        if (active) {
            r1 = ga_uniform(ga_draw_key(key, ev0 + s, kAcoSlotR1));
            r2 = ga_uniform(ga_draw_key(key, ev0 + s, kAcoSlotR2));
        }
        const AcoChoice ch = aco_select(L, n, na, active, r1, r2, stage_w, stage_e);
        if (active) {
            const uint32_t next = ch.city < n ? ch.city : 0u;  // (always < n; stay inside whatever happens)
            fallbacks += ch.path != 0u;
            myvis[next >> 5] |= 1u << (next & 31u);
            succ[cur] = (uint16_t)next;
            pred[next] = (uint16_t)cur;
            tour[s] = (uint16_t)next;
            cur = next;
            L.cur[lane] = cur;
        }
        TL_SYNC();
    }
    // tour_length_by_pos: the closing edge, then the n - 1 windows in order
    float acc = 0.0f;
    if (active) {
        succ[cur] = (uint16_t)first;
        pred[first] = (uint16_t)cur;
        acc = D(cur, first);
    }
    const auto stage_c = [&](uint32_t a, uint32_t k) -> float {
        if (k + 1u >= n) return 0.0f;
        const uint16_t *t = gtour + (size_t)a * n;
        return D(t[k], t[k + 1u]);
    };
    acc = aco_sum_pass(L, (n - 1u + kAcoChunk - 1u) / kAcoChunk, na, acc, false, stage_c);
    if (active) {
        const size_t ant = (size_t)run * A.num_ants + a0 + lane;
        A.cost[ant] = acc;
        A.start[ant] = first;
        A.fb[ant] = fallbacks;
    }
}

__global__ __launch_bounds__(256) void k_aco_best(AcoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, na = A.num_ants, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    uint32_t *hdr = reinterpret_cast<uint32_t *>(smem);
    uint16_t *list = reinterpret_cast<uint16_t *>(smem + 64);
    const float *cost = A.cost + (size_t)run * na;
    const uint32_t *start = A.start + (size_t)run * na, *fb = A.fb + (size_t)run * na;
    uint32_t *state = A.state + 8u * (size_t)run;
    if (A.log && run == 0u && A.epoch < A.log_cap) {
        uint32_t *rec = A.log + (size_t)A.epoch * 3u * na;
        for (uint32_t a = tid; a < na; a += nt) {
            rec[a] = __builtin_bit_cast(uint32_t, cost[a]);
            rec[na + a] = start[a];
            rec[2u * na + a] = fb[a];
        }
    }
    if (tid == 0) {
        float best = __builtin_bit_cast(float, state[0]);
        uint32_t cnt = 0;
        uint64_t fbs = ((uint64_t)state[5] << 32) | state[2];
        for (uint32_t a = 0; a < na; ++a) {
            fbs += fb[a];
            if (cost[a] < best) {
                best = cost[a];
                list[cnt++] = (uint16_t)a;
            }
        }
        hdr[0] = cnt;
        hdr[1] = state[1];
        state[0] = __builtin_bit_cast(uint32_t, best);
        state[1] += cnt;
        state[2] = (uint32_t)fbs;
        state[5] = (uint32_t)(fbs >> 32);
        if (cnt) A.out_cost[run] = best;
    }
    TL_SYNC();
    const uint32_t cnt = hdr[0], before = hdr[1];
    if (cnt == 0u) return;
    const uint16_t *tours = A.tour + (size_t)run * na * n;
    const uint16_t *bt = tours + (size_t)list[cnt - 1u] * n;
    uint32_t *out = A.out_pos + (size_t)run * n;
    for (uint32_t k = tid; k < n; k += nt) out[k] = bt[k];
    if (A.route_log && run == 0u) {
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t row = (uint64_t)before + 1u + j;
            if (row >= A.route_cap) break;
            const uint32_t a = list[j];
            uint32_t *rec = A.route_log + (size_t)row * (n + 3u);
            if (tid == 0) {
                rec[0] = A.epoch;
                rec[1] = a;
                rec[2] = __builtin_bit_cast(uint32_t, cost[a]);
            }
            for (uint32_t k = tid; k < n; k += nt) rec[3u + k] = tours[(size_t)a * n + k];
        }
    }
}

__global__ __launch_bounds__(256) void k_aco_update(AcoArgs A, uint32_t rows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, u0 = blockIdx.x * rows, run = blockIdx.y;
    const uint32_t nr = n - u0 < rows ? n - u0 : rows;
    float *row = reinterpret_cast<float *>(smem);
    const size_t off = (size_t)run * A.mat_stride + (size_t)u0 * n;
    float *tau = A.tau + off, *w = A.w + off;
    const float *eta = A.eta + off;
    const float tau_min = __builtin_bit_cast(float, A.state[8u * (size_t)run + 4u]), keep = 1.0f - A.rate;
    const uint32_t ants = A.pre ? (A.init ? 1u : 0u) : A.num_ants, cells = nr * n;
    for (uint32_t i = tid; i < cells; i += nt) {
        float t = tau[i];
        if (!A.pre) {  // evaporate_and_floor (ant_colony.rs:25-32)
            t *= keep;
            if (t < tau_min) t = tau_min;
        }
        row[i] = t;
    }
    TL_SYNC();
    if (tid < nr) {  // deposit_tour (ant_colony.rs:43-53) of every ant, in ant order, on this row's cells
        const uint32_t u = u0 + tid;
        float *r = row + (size_t)tid * n;
        const size_t tab = (size_t)run * A.num_ants * n;
        const float *cost = A.cost + (size_t)run * A.num_ants;
        for (uint32_t a = 0; a < ants; ++a) {
            const float c = cost[a];
            if (c <= 0.0f) continue;
            const float amount = 1.0f / c;
            const uint32_t sv = A.succ[tab + (size_t)a * n + u], pv = A.pred[tab + (size_t)a * n + u];
            if (sv < n) r[sv] += amount;  // (always < n: a tour visits every city; stay inside the row whatever the tables hold)
            if (pv < n) r[pv] += amount;
        }
    }
    TL_SYNC();
    for (uint32_t i = tid; i < cells; i += nt) {
        const float t = row[i];
        tau[i] = t;
        w[i] = aco_pow(t, A.alpha) * eta[i];
    }
}

// the device's selection for one ant on a given row (tl_aco_selftest_select)
__global__ __launch_bounds__(kAcoThreads) void k_aco_selftest_select(const float *weights, const float *eta, const uint32_t *visited, uint32_t n, float r1, float r2,
                                                                     uint32_t *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x;
    const AcoLds L(smem, n);
    for (uint32_t w = tid; w < L.vw; w += kAcoThreads) {
        uint32_t bitsw = 0;
        for (uint32_t b = 0; b < 32u && w * 32u + b < n; ++b) bitsw |= (visited[w * 32u + b] ? 1u : 0u) << b;
        L.vis[w] = bitsw;
    }
    if (tid < 64u) L.cur[tid] = 0u;
    TL_SYNC();
    const auto masked = [&](const float *M, uint32_t v) -> float {
        if (v >= n) return 0.0f;
        if ((L.vis[v >> 5] >> (v & 31u)) & 1u) return 0.0f;
        return M[v];
    };
    const auto stage_w = [&](uint32_t, uint32_t v) { return masked(weights, v); };
    const auto stage_e = [&](uint32_t, uint32_t v) { return masked(eta, v); };
    const AcoChoice ch = aco_select(L, n, 1u, tid == 0u, r1, r2, stage_w, stage_e);
    if (tid == 0) {
        out[0] = ch.city;
        out[1] = ch.path;
        out[2] = __builtin_bit_cast(uint32_t, ch.total);
        out[3] = __builtin_bit_cast(uint32_t, ch.eta_total);
    }
}

size_t ant_colony_lds_bytes(uint32_t n)
{
    return kAcoFixedBytes + 2 * kAcoTileBytes + (size_t)((n + kAcoChunk - 1u) / kAcoChunk) * 256 + (size_t)((n + 31u) / 32u) * 256;
}

uint32_t ant_colony_max_n(int lds_budget)
{
    uint32_t lo = 0, hi = 0xFFFFu;  // (the tables' entries are 16 bits wide); the layout grows with n
    if (lds_budget < 0 || ant_colony_lds_bytes(1) > (size_t)lds_budget) return 0u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (ant_colony_lds_bytes(mid) <= (size_t)lds_budget) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

int ant_colony_threads() { return (int)kAcoThreads; }

hipError_t launch_aco_init(const AcoArgs &A, uint32_t runs, hipStream_t s)
{
    hipError_t e = launch_max_lds(A.dm_full ? k_aco_init<true> : k_aco_init<false>, dim3(runs), 256, (size_t)A.n * 6 + 16, s, A);
    if (e != hipSuccess) return e;
    return launch_max_lds(A.dm_full ? k_aco_fill<true> : k_aco_fill<false>, dim3(A.n, runs), 256, 0, s, A);
}

hipError_t launch_aco_construct(const AcoArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_aco_construct<true> : k_aco_construct<false>, dim3((A.num_ants + 63u) / 64u, runs), (int)kAcoThreads, ant_colony_lds_bytes(A.n),
                      s, A);
}

hipError_t launch_aco_best(const AcoArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(k_aco_best, dim3(runs), 256, 64 + (size_t)A.num_ants * 2 + 16, s, A);
}

hipError_t launch_aco_update(const AcoArgs &A, uint32_t runs, int lds_budget, hipStream_t s)
{
    const size_t budget = (size_t)lds_budget < (48u << 10) ? (size_t)lds_budget : (48u << 10);
    size_t rows = budget / ((size_t)A.n * 4);
    rows = rows < 1 ? 1 : rows > 16 ? 16 : rows;  // (one row is 4 n bytes <= the construct kernel's 12 n: it fits wherever that does)
    return launch_max_lds(k_aco_update, dim3((uint32_t)((A.n + rows - 1) / rows), runs), 256, rows * (size_t)A.n * 4, s, A, (uint32_t)rows);
}

hipError_t launch_aco_selftest_select(const float *weights, const float *eta, const uint32_t *visited, uint32_t n, float r1, float r2, uint32_t *out, hipStream_t s)
{
    return launch_max_lds(k_aco_selftest_select, dim3(1), (int)kAcoThreads, ant_colony_lds_bytes(n), s, weights, eta, visited, n, r1, r2, out);
}

}  // namespace tl
