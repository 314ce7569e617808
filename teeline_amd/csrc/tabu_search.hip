// tabu_search.hip — tabu search (tabu_search.rs:9-110): one workgroup per chain, the current tour resident in that CU's LDS, the
// candidates of an epoch evaluated a round of W at once, the tabu list a ring of n routes in the context's workspace.
//
// The draws of candidate a of epoch e are a pure function of (seed, chain, e (n + 1) + a) (tabu_spec.h: this project's
// specification — the reference draws from an unseeded thread RNG), so all n + 1 candidates of an epoch are known up front.  Lane l
// of the round that starts at attempt a0 costs candidate a0 + l: sim_anneal.hip's walk (the reference's full re-sum of the candidate,
// closing edge first, started from S[from-1] where the closing edge stays).  The improving lanes of a round are then tried in
// ascending order against the list and the lowest one that is not listed is taken; a round without one is followed by the next,
// and when attempts 0 .. n-1 all fail attempt n is taken unchecked (select, tabu_search.rs:65-81).
//
//   LDS: the rounds' ballots (two sets, alternating) and the membership test's words | perm[n] | E[n] | S[n] as in sim_anneal.hip.
//   Workspace, per chain: ring[n][n] of 16-bit positions (newest at head - 1; a full ring overwrites its oldest) and one hash per
//   listed route: the sum of a symmetric hash of the open path's n - 1 edges — a reversal changes two of them, so a candidate's
//   hash costs its lane four edge hashes — combined with the bits of the route's cost.  A lane-parallel look-up over the hashes
//   names the listed routes that may equal the candidate; a wave then compares each of them with the candidate element for
//   element.  The hash never decides alone: with full_compare every listed route is compared.
#include "chain_tour.h"
#include "tabu_spec.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kTabuFixedBytes = 2 * 16 * 8 + 32;  // two sets of 16 wave ballots; listed[2], from, to, hash, the start tour's edge hash

// the hash of the undirected edge {a, b}
__device__ __forceinline__ uint32_t tabu_edge_hash(uint32_t a, uint32_t b)
{
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return (uint32_t)(sa_mix((uint64_t)lo << 32 | hi) >> 32);
}
__device__ __forceinline__ uint32_t tabu_route_hash(uint32_t edges, float cost) { return edges ^ (__builtin_bit_cast(uint32_t, cost) * 0x9E3779B1u); }

// what a reversal of positions f..=t does to the sum of the path's edge hashes
__device__ __forceinline__ uint32_t tabu_edges_after(uint32_t edges, const uint32_t *perm, uint32_t n, uint32_t f, uint32_t t)
{
    if (f > 0u) edges += tabu_edge_hash(perm[f - 1u], perm[t]) - tabu_edge_hash(perm[f - 1u], perm[f]);
    if (t < n - 1u) edges += tabu_edge_hash(perm[f], perm[t + 1u]) - tabu_edge_hash(perm[t], perm[t + 1u]);
    return edges;
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(1024) void k_tabu_search(TabuArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, blk = blockIdx.x, lane = tid & 63u, wave = tid >> 6, nw = nt >> 6;
    // mask[rp][w]: the improving lanes of wave w in the current round.  Two sets: a round that finds nothing ends without a second
    // barrier, so a fast wave posts its next ballot while a slow one still reads this round's.
    uint64_t *mask = reinterpret_cast<uint64_t *>(smem);
    // [0], [1] "the candidate is listed", test i in slot i % 2 (cleared by the publishing lane before the test's first barrier, while a
    // slow wave may still read the last test's); [2] from, [3] to, [4] hash of the candidate under test; [5] the start tour's edge hash
    uint32_t *slot = reinterpret_cast<uint32_t *>(mask + 32);
    uint32_t *perm = slot + 8;
    float *E = reinterpret_cast<float *>(perm + n);
    float *S = E + n;
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_chain + blk);
    uint16_t *ring = A.ring + (size_t)blk * A.ring_stride;
    uint32_t *rhash = A.hashes + (size_t)blk * n;
    uint32_t *best = A.out_pos + (size_t)blk * n;

    // best = u = the start tour, which the list receives (tabu_search.rs:23-26,32)
    const uint32_t *init = A.init + (size_t)blk * A.init_stride;
    for (uint32_t k = tid; k < n; k += nt) {
        const uint32_t v = init[k];
        perm[k] = v;
        best[k] = v;
        ring[k] = (uint16_t)v;
    }
    TL_SYNC();
    for (uint32_t k = tid; k < n; k += nt) E[k] = D(perm[k], perm[k + 1u == n ? 0u : k + 1u]);
    TL_SYNC();
    if (tid == 0) {
        float tot = E[n - 1u];
        uint32_t h = 0;
        for (uint32_t k = 0; k + 1u < n; ++k) {
            S[k] = tot;
            tot += E[k];
            h += tabu_edge_hash(perm[k], perm[k + 1u]);
        }
        S[n - 1u] = tot;
        slot[5] = h;
        rhash[0] = tabu_route_hash(h, tot);
    }
    TL_SYNC();

    uint32_t edges = slot[5];                 // the sum of u's edge hashes
    uint32_t ring_len = 1u, head = 1u;        // (n >= 2) head: where the next route goes
    float best_cost = S[n - 1u];
    uint32_t moves = 0, rp = 0, par = 0;
    uint64_t candidates = 0, reversed = 0;
    for (uint32_t e = 0; e < A.epochs; ++e) {
        const float local = S[n - 1u];
        bool found = false;
        uint32_t taken = n, f = 0, t = 0;
        for (uint32_t base = 0; base < n && !found; base += nt) {
            const uint32_t a = base + tid;
            const bool live = a < n;
            uint32_t from = 0, to = 0, start = n;
            float tot = 0.0f, ea = 0.0f, eb = 0.0f;
            if (live) {
                tabu_pair(key, tabu_event(e, n, a), n, &from, &to);
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
            // (this costing and the commit below stand in sim_anneal.hip and hill_climb.hip too, character for character: change all three — chain_tour.h says why)
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
            const bool improving = live && tot < local;
            const uint64_t b = __ballot(improving);
            if (lane == 0u) mask[rp * 16u + wave] = b;
            TL_SYNC();
            // (uniform) the improving attempts in ascending order against the list
            for (uint32_t w = 0; w < nw && !found; ++w) {
                uint64_t m = mask[rp * 16u + w];
                while (m) {
                    const uint32_t c = w * 64u + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1u;
                    if (tid == c) {
                        slot[2] = from;
                        slot[3] = to;
                        slot[4] = tabu_route_hash(tabu_edges_after(edges, perm, n, from, to), tot);
                        slot[par] = 0u;
                    }
                    TL_SYNC();
                    const uint32_t cf = slot[2], ct = slot[3], ch = slot[4], csum = cf + ct;
                    bool done = false;
                    for (uint32_t j0 = wave * 64u; j0 < ring_len && !done; j0 += nt) {  // (wave-uniform) 64 listed routes at a time
                        const uint32_t j = j0 + lane;
                        uint64_t hm = __ballot(j < ring_len && (A.full_compare || rhash[j] == ch));
                        while (hm && !done) {
                            const uint16_t *r = ring + (size_t)(j0 + (uint32_t)__builtin_ctzll(hm)) * n;
                            hm &= hm - 1u;
                            bool same = true;
                            for (uint32_t q0 = 0; q0 < n && same; q0 += 64u) {
                                const uint32_t q = q0 + lane;
                                const bool differs = q < n && perm[q >= cf && q <= ct ? csum - q : q] != (uint32_t)r[q];
                                same = !__any(differs);
                            }
                            if (same) {
                                if (lane == 0u) slot[par] = 1u;
                                done = true;
                            }
                        }
                    }
                    TL_SYNC();
                    const bool listed = slot[par] != 0u;
                    par ^= 1u;
                    if (!listed) {
                        found = true;
                        taken = base + c;
                        f = cf;
                        t = ct;
                        break;
                    }
                }
            }
            rp ^= 1u;
        }
        if (!found) tabu_pair(key, tabu_event(e, n, n), n, &f, &t);  // attempt n, with no check at all
        candidates += (uint64_t)taken + 1u;

        // the old u and its hash into the ring (tabu_search.rs:52), then u <- the taken candidate
        {
            uint16_t *dst = ring + (size_t)head * n;
            for (uint32_t k = tid; k < n; k += nt) dst[k] = (uint16_t)perm[k];
            if (tid == 0) rhash[head] = tabu_route_hash(edges, local);
            head = head + 1u == n ? 0u : head + 1u;
            ring_len = ring_len < n ? ring_len + 1u : n;
            edges = tabu_edges_after(edges, perm, n, f, t);
        }
        TL_SYNC();
        // swap_cities (route.rs:102-113): positions f..=t reversed; the edges between them travel with them
        for (uint32_t i = tid; 2u * i + 1u < t - f + 1u; i += nt) {
            const uint32_t x = perm[f + i], y = perm[t - i];
            perm[f + i] = y;
            perm[t - i] = x;
        }
        for (uint32_t i = tid; 2u * i + 1u < t - f; i += nt) {
            const float x = E[f + i], y = E[t - 1u - i];
            E[f + i] = y;
            E[t - 1u - i] = x;
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
            if (A.log && blk == 0u && e < A.log_cap) {
                A.log[4u * (size_t)e + 0u] = taken;
                A.log[4u * (size_t)e + 1u] = f;
                A.log[4u * (size_t)e + 2u] = t;
                A.log[4u * (size_t)e + 3u] = __builtin_bit_cast(uint32_t, s);
            }
        }
        reversed += t - f + 1u;
        TL_SYNC();
        const float cost = S[n - 1u];
        if (cost < best_cost) {  // (uniform) tabu_search.rs:38-40
            best_cost = cost;
            ++moves;
            for (uint32_t k = tid; k < n; k += nt) best[k] = perm[k];
        }
    }

    if (tid == 0) {
        A.out_cost[blk] = best_cost;
        uint32_t *run = A.out_run + 8u * (size_t)blk;  // new bests, candidates (64 bits), elements moved (64 bits)
        run[0] = moves;
        run[1] = (uint32_t)candidates;
        run[2] = (uint32_t)(candidates >> 32);
        run[3] = (uint32_t)reversed;
        run[4] = (uint32_t)(reversed >> 32);
    }
}

size_t tabu_search_lds_bytes(uint32_t n) { return (size_t)n * 12 + kTabuFixedBytes; }

uint32_t tabu_search_lds_max_n(int lds_budget)
{
    if ((size_t)lds_budget <= kTabuFixedBytes) return 0u;
    const size_t m = ((size_t)lds_budget - kTabuFixedBytes) / 12;
    return m > 0xFFFFu ? 0xFFFFu : (uint32_t)m;  // (the ring's entries are 16 bits wide)
}

hipError_t launch_tabu_search(const TabuArgs &A, uint32_t count, int threads, hipStream_t s)
{
    void (*const kern)(TabuArgs) = A.dm_full ? k_tabu_search<true> : k_tabu_search<false>;
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(count), dim3(threads), tabu_search_lds_bytes(A.n), s, A);
    return hipGetLastError();
}

}  // namespace tl
