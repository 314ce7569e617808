// hill_climb.hip — the stochastic hill climb (stochastic_hill.rs:7-97): one workgroup per chain, the whole chain resident in that
// CU's LDS, W consecutive epochs evaluated at once.
//
// The random draws of epoch e are a pure function of (seed, chain, e) (hill_spec.h: this project's specification — the reference
// draws from an unseeded thread RNG), and a candidate is accepted iff its cost is below the BEST cost, so an epoch's verdict
// depends on the current tour and the best cost alone.  Lane l of a window that starts at epoch e0 evaluates epoch e0 + l against
// them.  A window has at most one event: the lowest accepting lane a, or the lane r = platoo_epochs - n_stale whose rejection
// trips the plateau, whichever comes first (a == r: the acceptance, which clears n_stale).  The event is applied, the later
// verdicts are thrown away and their epochs evaluated again.  A descended chain rejects nearly every epoch, so most windows have
// no event and advance by their full width behind one barrier.  No verdict differs from the one-epoch-at-a-time chain (window = 1).
//
//   LDS: perm[n] | E[n] tour-edge lengths, E[n-1] the closing edge | S[n] the running sequential sum before edge k is added
//        (S[0] = E[n-1]; S[n-1] = the tour's length) | the window's verdict and move.
//   Uniform registers: the best cost, n_stale, whether the best route is the current one, the counters.  The best route lives in
//   global memory (out_pos): written when a restart is about to shuffle a current tour that is the best, and at the end.
//   A candidate's cost is the reference's full re-sum of the candidate tour (closing edge first, then the n - 1 edges in order,
//   sequential f32), started from S[from-1] where the closing edge stays: sim_anneal.hip's walk.
#include "chain_tour.h"
#include "hill_spec.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kHillSlotBytes = 32;  // three winner slots (rotating), from, to

}  // namespace

template <bool DM>
__global__ __launch_bounds__(1024) void k_hill_climb(HillArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, blk = blockIdx.x, W = A.window, e_end = A.epochs, platoo = A.platoo;
    uint32_t *perm = reinterpret_cast<uint32_t *>(smem);
    float *E = reinterpret_cast<float *>(perm + n);
    float *S = E + n;
    // [0..2] the lowest accepting lane of a window, window w in slot w % 3 (sim_anneal.hip's scheme: a window without an event ends
    // without a second barrier; the slot of window w + 2 is cleared behind window w's barrier).  [3] from, [4] to
    uint32_t *slot = reinterpret_cast<uint32_t *>(S + n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_chain + blk);
    uint32_t *out = A.out_pos + (size_t)blk * n;

    const uint32_t *init = A.init + (size_t)blk * A.init_stride;
    for (uint32_t k = tid; k < n; k += nt) perm[k] = init[k];
    if (tid < 3u) slot[tid] = 0xFFFFFFFFu;
    TL_SYNC();

    uint32_t e0 = 0, moves = 0, restarts = 0, n_stale = 0, w3 = 0;  // w3: the window's number mod 3
    uint64_t reversed = 0;
    float best = 0.0f;
    bool best_is_cur = true, fresh = true;  // fresh: perm is new (the start tour, a restart's shuffle): E and S are to be built
    while (true) {
        if (fresh) {  // (uniform)
            for (uint32_t k = tid; k < n; k += nt) E[k] = D(perm[k], perm[k + 1u == n ? 0u : k + 1u]);
            TL_SYNC();
            if (tid == 0) {
                float tot = E[n - 1u];
                for (uint32_t k = 0; k + 1u < n; ++k) {
                    S[k] = tot;
                    tot += E[k];
                }
                S[n - 1u] = tot;
            }
            TL_SYNC();
            if (e0 == 0u && restarts == 0u) best = S[n - 1u];  // the start tour's length
            fresh = false;
        }
        if (e0 >= e_end) break;
        const uint32_t live_n = e_end - e0 < W ? e_end - e0 : W;
        const bool live = tid < live_n;
        const uint32_t e = e0 + tid;
        uint32_t from = 0, to = 0, start = n;
        float tot = 0.0f, ea = 0.0f, eb = 0.0f;
        if (live) {
            sa_pair(key, e, n, &from, &to);
            const bool closing = from == 0u || to == n - 1u;
            if (from > 0u) ea = D(perm[from - 1u], perm[to]);
            if (to < n - 1u) eb = D(perm[from], perm[to + 1u]);
            if (closing) {
                tot = D(to == n - 1u ? perm[from] : perm[n - 1u], from == 0u ? perm[to] : perm[0]);
                start = 0u;
            } else {
                start = from - 1u;
                tot = S[start];
            }
        }
        // (this costing and the commit below are sim_anneal.hip's and tabu_search.hip's: change all three — chain_tour.h says why)
        // the wave's lanes walk k together from the lowest start among them
        const uint32_t k0 = wave_min_u32(start);
        const uint32_t rsum = from + to - 1u;
#pragma unroll 4
        for (uint32_t k = k0; k + 1u < n; ++k) {
            const bool inside = k >= from && k < to;
            float v = E[inside ? rsum - k : k];
            v = k + 1u == from ? ea : v;
            v = k == to ? eb : v;
            if (k >= start) tot += v;
        }
        if (live && tot < best) atomicMin(&slot[w3], tid);
        TL_SYNC();
        const uint32_t win = slot[w3];
        w3 = w3 == 2u ? 0u : w3 + 1u;
        if (tid == 0) slot[w3 == 2u ? 0u : w3 + 1u] = 0xFFFFFFFFu;
        const uint32_t r = platoo - n_stale;  // (platoo > 0: n_stale <= platoo here) the lane whose rejection trips the plateau
        const bool accept = win != 0xFFFFFFFFu && (platoo == 0u || win <= r);
        if (!accept) {  // (uniform)
            if (platoo == 0u || r >= live_n) {  // no event: the whole window is behind us
                n_stale += live_n;
                e0 += live_n;
                continue;
            }
            // the plateau after epoch e0 + r: the current tour is shuffled in place, the best stays (stochastic_hill.rs:65-78)
            if (best_is_cur) {
                for (uint32_t k = tid; k < n; k += nt) out[k] = perm[k];
                best_is_cur = false;
            }
            TL_SYNC();
            if (tid == 0) {
                hill_shuffle(key, e0 + r, n, perm);
                if (A.log && blk == 0u) {
                    const uint32_t m = moves + restarts;
                    if (m < A.log_cap) {
                        A.log[4u * m + 0u] = e0 + r;
                        A.log[4u * m + 1u] = 0xFFFFFFFFu;
                        A.log[4u * m + 2u] = 0u;
                        A.log[4u * m + 3u] = 0u;
                    }
                }
            }
            TL_SYNC();
            ++restarts;
            n_stale = 0u;
            e0 += r + 1u;
            fresh = true;
            continue;
        }
        if (tid == win) {
            slot[3] = from;
            slot[4] = to;
        }
        TL_SYNC();
        const uint32_t f = slot[3], t = slot[4];
        // swap_cities (route.rs:102-113): positions f..=t reversed; the edges between them travel with them
        for (uint32_t i = tid; 2u * i + 1u < t - f + 1u; i += nt) {
            const uint32_t a = perm[f + i], b = perm[t - i];
            perm[f + i] = b;
            perm[t - i] = a;
        }
        for (uint32_t i = tid; 2u * i + 1u < t - f; i += nt) {
            const float a = E[f + i], b = E[t - 1u - i];
            E[f + i] = b;
            E[t - 1u - i] = a;
        }
        TL_SYNC();
        const bool closing = f == 0u || t == n - 1u;
        if (tid == 0 && f > 0u) E[f - 1u] = D(perm[f - 1u], perm[f]);
        if (tid == 1u && t < n - 1u) E[t] = D(perm[t], perm[t + 1u]);
        if (tid == 2u && closing) E[n - 1u] = D(perm[n - 1u], perm[0]);
        TL_SYNC();
        if (tid == 0) {
            uint32_t k = closing ? 0u : f - 1u;
            float s = closing ? E[n - 1u] : S[k];
            for (; k + 1u < n; ++k) {
                S[k] = s;
                s += E[k];
            }
            S[n - 1u] = s;
            if (A.log && blk == 0u) {
                const uint32_t m = moves + restarts;
                if (m < A.log_cap) {
                    A.log[4u * m + 0u] = e0 + win;
                    A.log[4u * m + 1u] = f;
                    A.log[4u * m + 2u] = t;
                    A.log[4u * m + 3u] = __builtin_bit_cast(uint32_t, s);
                }
            }
        }
        ++moves;
        reversed += t - f + 1u;
        TL_SYNC();
        best = S[n - 1u];  // current = best = the candidate (stochastic_hill.rs:43-49)
        best_is_cur = true;
        n_stale = 0u;
        e0 += win + 1u;
    }

    if (best_is_cur)
        for (uint32_t k = tid; k < n; k += nt) out[k] = perm[k];
    if (tid == 0) {
        A.out_cost[blk] = best;
        uint32_t *run = A.out_run + 4u * (size_t)blk;
        run[0] = moves;
        run[1] = (uint32_t)reversed;
        run[2] = (uint32_t)(reversed >> 32);
        run[3] = restarts;
    }
}

size_t hill_climb_lds_bytes(uint32_t n) { return (size_t)n * 12 + kHillSlotBytes; }

uint32_t hill_climb_lds_max_n(int lds_budget)
{
    if ((size_t)lds_budget <= kHillSlotBytes) return 0u;
    const size_t m = ((size_t)lds_budget - kHillSlotBytes) / 12;
    return m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m;
}

hipError_t launch_hill_climb(const HillArgs &A, uint32_t count, int threads, hipStream_t s)
{
    void (*const kern)(HillArgs) = A.dm_full ? k_hill_climb<true> : k_hill_climb<false>;
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(count), dim3(threads), hill_climb_lds_bytes(A.n), s, A);
    return hipGetLastError();
}

}  // namespace tl
