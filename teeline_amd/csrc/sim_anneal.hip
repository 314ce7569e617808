// sim_anneal.hip — simulated annealing (simulated_annealing.rs:10-83): one workgroup per chain, the whole chain resident in
// that CU's LDS, W consecutive epochs evaluated at once.
//
// The random draws of epoch e are a pure function of (seed, chain, e) and the temperature a pure function of e (sa_spec.h: this
// project's specification — the reference draws from an unseeded thread RNG), so an epoch's verdict depends on the current
// tour alone.  Lane l of a window that starts at epoch e0 evaluates epoch e0 + l against that tour; the first accepting lane in
// order is committed, the later verdicts are thrown away and their epochs evaluated again against the new tour.  No verdict
// differs from the one-epoch-at-a-time chain (window = 1, TL_FLAG_SA_NO_SPECULATION, is that chain).
//
//   LDS: perm[n] | E[n] tour-edge lengths, E[n-1] the closing edge | S[n] the running sequential sum before edge k is added
//        (S[0] = E[n-1]; S[n-1] = the tour's length) | the window's verdict and move.
//   A candidate's cost is the reference's full re-sum of the candidate tour (closing edge first, then the n - 1 edges in order,
//   sequential f32).  Positions before from - 1 are untouched, so the lane starts from S[from-1]: the new edge, E[to-1] ... E[from]
//   backwards, the second new edge, E[to+1 ... n-2].  With from = 0 or to = n - 1 the closing edge changes and the sum starts
//   from scratch.  The lanes of a wave walk k together, so most of them read the same E[k] (an LDS broadcast).
#include "chain_tour.h"
#include "sa_spec.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kSaSlotBytes = 32;  // three winner slots (rotating), from, to

}  // namespace

template <bool DM>
__global__ __launch_bounds__(1024) void k_sim_anneal(SaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, blk = blockIdx.x, W = A.window;
    uint32_t *perm = reinterpret_cast<uint32_t *>(smem);
    float *E = reinterpret_cast<float *>(perm + n);
    float *S = E + n;
    // [0..2] the lowest accepting lane of a window, window w in slot w % 3: a window that accepts nothing ends without a second
    // barrier, so a fast wave posts its next verdict while a slow one still reads this one; the slot of window w + 2 is cleared
    // behind window w's barrier, when every wave has read it (as window w - 1's) and none can post to it yet.  [3] from, [4] to
    uint32_t *slot = reinterpret_cast<uint32_t *>(S + n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_chain + blk);

    const uint32_t *init = A.init + (size_t)blk * A.init_stride;
    for (uint32_t k = tid; k < n; k += nt) perm[k] = init[k];
    if (tid < 3u) slot[tid] = 0xFFFFFFFFu;
    TL_SYNC();
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

    uint32_t e0 = A.e_begin, moves = 0, w3 = 0;  // w3: the window's number mod 3
    uint64_t reversed = 0;
    while (e0 < A.e_end) {
        const float cost = S[n - 1u];
        const uint32_t e = e0 + tid;
        const bool live = tid < W && e < A.e_end && e >= e0;  // (e >= e0: no wrap at the top of the epoch range)
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
        // (this costing and the commit below stand in tabu_search.hip and hill_climb.hip too, character for character: change all three — chain_tour.h says why)
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
        if (live) {
            bool acc;
            if (tot < cost) {
                acc = true;
            } else if (__builtin_fabsf(tot - cost) < 1.1920929e-07f) {
                acc = false;
            } else {
                const float T = A.temps[e - A.e_begin];
                acc = sa_p(key, e) < sa_criteria((-(tot - cost)) / T);
            }
            if (acc) atomicMin(&slot[w3], tid);
        }
        TL_SYNC();
        const uint32_t win = slot[w3];
        w3 = w3 == 2u ? 0u : w3 + 1u;
        if (tid == 0) slot[w3 == 2u ? 0u : w3 + 1u] = 0xFFFFFFFFu;
        if (win == 0xFFFFFFFFu) {  // (uniform) nothing accepted: the whole window is behind us
            e0 = A.e_end - e0 <= W ? A.e_end : e0 + W;
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
                const uint32_t m = A.out_run[0] + moves;
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
        e0 += win + 1u;
    }

    uint32_t *out = A.out_pos + (size_t)blk * n;
    for (uint32_t k = tid; k < n; k += nt) out[k] = perm[k];
    if (tid == 0) {
        A.out_cost[blk] = S[n - 1u];
        uint32_t *run = A.out_run + 4u * (size_t)blk;  // moves, elements moved (64 bits), unused: summed over the launches of a schedule
        const uint64_t r = ((uint64_t)run[2] << 32 | run[1]) + reversed;
        run[0] += moves;
        run[1] = (uint32_t)r;
        run[2] = (uint32_t)(r >> 32);
    }
}

// the acceptance rule on given values (tl_sa_selftest_accept): the device's own evaluation of sa_criteria
__global__ void k_sa_selftest(const float *T, const float *oldc, const float *newc, const float *p, uint32_t count, uint32_t *out_accept,
                              float *out_criteria)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float o = oldc[i], c = newc[i];
    const float crit = sa_criteria((-(c - o)) / T[i]);
    bool acc;
    if (c < o) acc = true;
    else if (__builtin_fabsf(c - o) < 1.1920929e-07f) acc = false;
    else acc = p[i] < crit;
    out_accept[i] = acc ? 1u : 0u;
    out_criteria[i] = crit;
}

size_t sim_anneal_lds_bytes(uint32_t n) { return (size_t)n * 12 + kSaSlotBytes; }

uint32_t sim_anneal_lds_max_n(int lds_budget)
{
    if ((size_t)lds_budget <= kSaSlotBytes) return 0u;
    const size_t m = ((size_t)lds_budget - kSaSlotBytes) / 12;
    return m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m;
}

hipError_t launch_sim_anneal(const SaArgs &A, uint32_t count, int threads, hipStream_t s)
{
    void (*const kern)(SaArgs) = A.dm_full ? k_sim_anneal<true> : k_sim_anneal<false>;
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(count), dim3(threads), sim_anneal_lds_bytes(A.n), s, A);
    return hipGetLastError();
}

hipError_t launch_sa_selftest(const float *T, const float *oldc, const float *newc, const float *p, uint32_t count, uint32_t *out_accept,
                              float *out_criteria, hipStream_t s)
{
    hipLaunchKernelGGL(k_sa_selftest, dim3((count + 255u) / 256u), dim3(256), 0, s, T, oldc, newc, p, count, out_accept, out_criteria);
    return hipGetLastError();
}

}  // namespace tl
