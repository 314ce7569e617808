// lk_scan.h — the chip-wide form (a part of lk.hip): the same algorithm as k_lk_solve, cut at its only grid-wide seam.
//   k_lk_scan     every (t1, orientation) pair of find_lk_move at once, one lane each, over all CUs; lanes with a valid chain store
//                 it in their slot and atomicMin the pair index — the reference's "first in order" is the minimum.
//   k_lk_scan_sub (+ k_lk_scan_pick where the workgroup does not pick for itself) the same with a pair's search split over lanes.
//   k_lk_control  a device-side state machine: apply the winning chain and rescan, or — when the scan found nothing, i.e. the
//                 lk_pass is over — evaluate the tour, accept/reject, kick (double_bridge) or finish.
// The host only enqueues rounds (launch_lk_round: scan, [pick,] control, [rebuild]) in batches and polls `finished`.
#pragma once

template <bool LDS>
__global__ __launch_bounds__(256) void k_lk_scan(LkArgs G)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lk_smem[];
    LkState *S = G.state;
    if (S->finished) return;
    const uint32_t n = G.n, idx = blockIdx.x * 256u + threadIdx.x;
    // The chain search is a divergent, latency-bound walk over xy[] and next[]: stage both in this CU's LDS
    // (8 B + 2 B per city) so a node costs one L2 access (the candidate list) instead of four.
    float2 *xyL = reinterpret_cast<float2 *>(lk_smem);
    uint16_t *nextL = reinterpret_cast<uint16_t *>(lk_smem + (size_t)n * 8);
    if (LDS) {
        for (uint32_t c = threadIdx.x; c < n; c += 256u) {
            xyL[c] = G.xy[c];
            nextL[c] = (uint16_t)G.next[c];
        }
        TL_SYNC();
    }
    if (idx >= 2u * n || idx >= S->window) return;
    uint32_t chain[kLkMaxChain];
    uint32_t clen = 0;
    const uint32_t t1 = G.city_ids[idx >> 1];
    const uint32_t t2 = (idx & 1u) ? G.prev[t1] : G.next[t1];
    const float2 p1 = G.xy[t1], p2 = G.xy[t2];
    chain[0] = t1;
    chain[1] = t2;
    const float g0 = t1 == t2 ? 0.0f : dist(p1, p2);
    bool found;
    if (LDS) {
        LkViewT<uint16_t> V{xyL, G.cand, nextL, G.k, G.max_depth};
        found = lk_chain<0, LkViewT<uint16_t>>(V, chain, clen, p1, t2, p2, g0);
    } else {
        LkView V{G.xy, G.cand, G.next, G.k, G.max_depth};
        found = lk_chain<0, LkView>(V, chain, clen, p1, t2, p2, g0);
    }
    if (found && chain_valid(chain, clen, G.tour, G.pos, n)) {
        uint32_t *slot = G.chains + (size_t)idx * kLkSlot;
        slot[0] = clen;
        for (uint32_t t = 0; t < clen; ++t) slot[1 + t] = chain[t];
        atomicMin(&S->key, idx);
    }
}

// ---- split scan: the chain search of one (t1, orientation) pair is itself cut into k*(k+1) independent
// sub-searches — branch q1 at depth 0 and, at depth 1, either the closing test (s = 0) or branch q2 = s-1 — so a
// find_lk_move becomes 2n*k*(k+1) short walks (810 K lanes at n = 13 509, k = 5) instead of 2n long divergent ones.
// Exactness: candidates are sorted by the same f32 distances, so g1 is non-increasing along a list and the
// reference's `break` at g1 <= EPS (:292-295) is implied by each sub-search's own test; `used[]` depends only on the
// chain.  The reference keeps the FIRST chain found in DFS order and drops the pair if that one is invalid (:373-381),
// hence two steps: k_lk_scan_sub records the minimum (q1, s) with a chain per pair, k_lk_scan_pick re-derives that
// chain, checks it, and posts the pair.
template <typename VT>
__device__ bool lk_subsearch(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1,
                             const uint32_t t1, const uint32_t t2, const float2 p2, const float g0, const uint32_t q1, const uint32_t s)
{
    // depth 0 (find_lk_chain :290-337 with depth = 0)
    const uint32_t t3 = V.cand[(size_t)t2 * V.k + q1];
    const float2 p3 = V.xy[t3];
    const float g1 = g0 - dist(p2, p3);
    if (g1 <= kLkEps) return false;
    if (t3 == t1 || t3 == t2) return false;
    const uint32_t t4 = V.next[t3];
    if ((uint32_t)V.next[t2] == t3 || t4 == t2) return false;
    if (t4 == t1 || t4 == t2) return false;
    const float2 p4 = V.xy[t4];
    const float g2 = g1 + dist(p3, p4);
    chain[2] = t3;
    chain[3] = t4;
    // depth 1
    const float close_gain = g2 - dist(p4, p1);
    if (s == 0u) {
        if (close_gain > kLkEps) {
            clen = 4;
            return true;
        }
        return false;
    }
    if (close_gain > kLkEps) return false;  // the sequential search returned at s = 0
    if (1u >= V.max_depth) return false;
    const uint32_t t5 = V.cand[(size_t)t4 * V.k + (s - 1u)];
    const float2 p5 = V.xy[t5];
    const float g3 = g2 - dist(p4, p5);
    if (g3 <= kLkEps) return false;
    if (in_chain<4>(chain, t5)) return false;
    const uint32_t t6 = V.next[t5];
    if ((uint32_t)V.next[t4] == t5 || t6 == t4) return false;
    if (in_chain<4>(chain, t6)) return false;
    const float2 p6 = V.xy[t6];
    const float g4 = g3 + dist(p5, p6);
    chain[4] = t5;
    chain[5] = t6;
    return lk_chain<2, VT>(V, chain, clen, p1, t6, p6, g4);
}

// One explicit branch of find_lk_chain's loop (:290-337) at depth D: candidate q of t_open.  On success the chain grows by
// (t_next, t_break) and (t_open, p_open, gain) move on; a rejected branch returns false (for the `break` at g1 <= EPS see
// the exactness note above: it is implied by the later branches' own tests).
template <int D, typename VT>
__device__ __forceinline__ bool lk_branch(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &t_open, float2 &p_open,
                                          float &gain, const uint32_t q)
{
    uint32_t t_next;
    float2 p_next, p_break;
    float d1, d2;
    float4 rec;
    lk_probe(V, t_open, p_open, q, t_next, p_next, d1);
    const float g1 = gain - d1;
    if (g1 <= kLkEps) return false;
    if (in_chain<2 * D + 2>(chain, t_next)) return false;
    const uint32_t t_break = lk_break_id(V, t_next, rec);
    if (lk_next_of(V, t_open) == t_next || t_break == t_open) return false;
    if (in_chain<2 * D + 2>(chain, t_break)) return false;
    lk_break_pt(V, t_break, p_next, rec, p_break, d2);
    chain[2 * D + 2] = t_next;
    chain[2 * D + 3] = t_break;
    gain = g1 + d2;
    t_open = t_break;
    p_open = p_break;
    return true;
}

// Three split levels: sub = (q1 (k+1) + s1)(k+1) + s2 — branch q1 at depth 0; at depth 1 the closing test (s1 = 0) or
// branch s1-1; at depth 2 the closing test (s2 = 0) or branch s2-1, below which the walk is sequential (lk_chain<3>: at most
// k^2 nodes instead of k^3).  Lexicographic order of (q1, s1, s2) is the reference's DFS order, so the minimum index with a
// chain is the chain the sequential search returns; (q1, 0, s2 > 0) does not exist.
template <typename VT>
__device__ bool lk_subsearch3(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1,
                              const uint32_t t2, const float2 p2, const float g0, const uint32_t q1, const uint32_t s1, const uint32_t s2)
{
    uint32_t t_open = t2;
    float2 p_open = p2;
    float gain = g0;
    if (0u >= V.max_depth) return false;
    if (!lk_branch<0, VT>(V, chain, t_open, p_open, gain, q1)) return false;
    {   // depth 1 (:280-288)
        const float close_gain = gain - dist(p_open, p1);
        if (s1 == 0u) {
            if (s2 == 0u && close_gain > kLkEps) {
                clen = 4;
                return true;
            }
            return false;
        }
        if (close_gain > kLkEps) return false;  // the sequential search returned at s1 = 0
        if (1u >= V.max_depth) return false;
    }
    if (!lk_branch<1, VT>(V, chain, t_open, p_open, gain, s1 - 1u)) return false;
    {   // depth 2
        const float close_gain = gain - dist(p_open, p1);
        if (s2 == 0u) {
            if (close_gain > kLkEps) {
                clen = 6;
                return true;
            }
            return false;
        }
        if (close_gain > kLkEps) return false;
        if (2u >= V.max_depth) return false;
    }
    if (!lk_branch<2, VT>(V, chain, t_open, p_open, gain, s2 - 1u)) return false;
    return lk_chain<3, VT>(V, chain, clen, p1, t_open, p_open, gain);
}

// lk_subsearch3 cut in two for the fused scan (k_lk_scan_sub): the FRONT walks the three split levels and stops where the
// sequential walk lk_chain<3> would begin — 0: no chain, 1: chain (clen set), 2: a walk is pending at depth 3 with
// (chain[0..8), t_open = chain[7], p_open, gain), its depth-3 closing test already failed.
template <typename VT>
__device__ int lk_subsearch3_front(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1, const uint32_t t2,
                                   const float2 p2, const float g0, const uint32_t q1, const uint32_t s1, const uint32_t s2, float2 &p_open_out,
                                   float &gain_out)
{
    uint32_t t_open = t2;
    float2 p_open = p2;
    float gain = g0;
    if (0u >= V.max_depth) return 0;
    if (!lk_branch<0, VT>(V, chain, t_open, p_open, gain, q1)) return 0;
    {
        const float close_gain = gain - dist(p_open, p1);
        if (s1 == 0u) {
            if (s2 == 0u && close_gain > kLkEps) {
                clen = 4;
                return 1;
            }
            return 0;
        }
        if (close_gain > kLkEps) return 0;
        if (1u >= V.max_depth) return 0;
    }
    if (!lk_branch<1, VT>(V, chain, t_open, p_open, gain, s1 - 1u)) return 0;
    {
        const float close_gain = gain - dist(p_open, p1);
        if (s2 == 0u) {
            if (close_gain > kLkEps) {
                clen = 6;
                return 1;
            }
            return 0;
        }
        if (close_gain > kLkEps) return 0;
        if (2u >= V.max_depth) return 0;
    }
    if (!lk_branch<2, VT>(V, chain, t_open, p_open, gain, s2 - 1u)) return 0;
    // lk_chain<3>'s head (:280-288)
    if (gain - dist(p_open, p1) > kLkEps) {
        clen = 8;
        return 1;
    }
    if (3u >= V.max_depth) return 0;
    p_open_out = p_open;
    gain_out = gain;
    return 2;
}

// One (q3, s4) branch of a pending depth-3 walk: candidate q3 of t_open at depth 3; at depth 4 the closing test (s4 = 0) or
// candidate s4 - 1, below which lk_chain<5> is a closing test (and, only for max_depth = 6, one more candidate loop).
// Lexicographic order of (q3, s4) is the DFS order of lk_chain<3>, for the reasons given at lk_subsearch.
template <typename VT>
__device__ bool lk_tail_branch(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1, float2 p_open, float gain,
                               const uint32_t q3, const uint32_t s4)
{
    uint32_t t_open = chain[7];
    if (!lk_branch<3, VT>(V, chain, t_open, p_open, gain, q3)) return false;
    const float close_gain = gain - dist(p_open, p1);
    if (s4 == 0u) {
        if (close_gain > kLkEps) {
            clen = 10;
            return true;
        }
        return false;
    }
    if (close_gain > kLkEps) return false;  // the sequential walk returned at s4 = 0
    if (4u >= V.max_depth) return false;
    if (!lk_branch<4, VT>(V, chain, t_open, p_open, gain, s4 - 1u)) return false;
    return lk_chain<5, VT>(V, chain, clen, p1, t_open, p_open, gain);
}

// the rest of lk_chain<3> for a walk whose head (closing test, depth limit) the front has already passed: the head is
// repeated (it fails again) — only used when the workgroup's queue of parked walks is full
template <typename VT>
__device__ bool lk_chain_from3(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1, const float2 p_open, const float gain)
{
    return lk_chain<3, VT>(V, chain, clen, p1, chain[7], p_open, gain);
}

// the sub-search `sub` of pair (t1, t2) under the launch's split depth
__device__ __forceinline__ bool lk_run_sub(const LkArgs &G, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1, const uint32_t t1,
                                           const uint32_t t2, const float2 p2, const float g0, const uint32_t sub)
{
    LkView V{G.xy, G.cand, G.next, G.k, G.max_depth};
    const uint32_t k1 = G.k + 1u;
    if (G.split_levels == 3u) return lk_subsearch3<LkView>(V, chain, clen, p1, t2, p2, g0, sub / (k1 * k1), (sub / k1) % k1, sub % k1);
    return lk_subsearch<LkView>(V, chain, clen, p1, t1, t2, p2, g0, sub / k1, sub % k1);
}

// BLOCK3D: one workgroup = one pair, threadIdx = (s2, s1, q1) — the sub-search digits come for free; the flat form (for
// k(k+1)^2 > 1024) recovers them with a 64-bit and three 32-bit divisions per lane, which is most of what a lane that fails
// its first test executes.
template <bool BLOCK3D, bool PK = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_lk_scan_sub(LkArgs G)
{
    if (G.state->finished) return;
    const uint32_t n = G.n, subs = lk_subs(G);
    uint32_t idx, sub, q1, s1, s2;
    uint64_t g;
    if (BLOCK3D) {
        // workgroups are dispatched in index order: the pairs at the END of the window — around the previous hit, where the next
        // chain most likely is and the long walks are — go first, so their walks overlap with the bulk instead of trailing it
        const uint32_t win = G.state->window;
        if (blockIdx.x >= win) return;
        idx = win - 1u - blockIdx.x;
        const uint32_t k1 = G.k + 1u;
        if (G.split_levels == 3u) {
            q1 = threadIdx.z; s1 = threadIdx.y; s2 = threadIdx.x;
            sub = (q1 * k1 + s1) * k1 + s2;
        } else {
            q1 = threadIdx.y; s1 = threadIdx.x; s2 = 0u;
            sub = q1 * k1 + s1;
        }
        g = (uint64_t)idx * subs + sub;
    } else {
        g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (g >= (uint64_t)2u * n * subs) return;
        idx = (uint32_t)(g / subs);
        sub = (uint32_t)(g % subs);
        const uint32_t k1 = G.k + 1u;
        if (G.split_levels == 3u) { q1 = sub / (k1 * k1); s1 = (sub / k1) % k1; s2 = sub % k1; }
        else { q1 = sub / k1; s1 = sub % k1; s2 = 0u; }
    }
    if (idx >= G.state->window) return;  // prefix window (k_lk_control)
    // fused pick (one workgroup = one pair): the pair's first chain in DFS order = the lowest sub-search index that found one;
    // its lane still holds the chain, validates it and posts the pair (what k_lk_scan_pick does from pairmin / subchains)
    __shared__ uint32_t s_minkey, s_qn;
    __shared__ uint32_t s_q[kLkTailCap][kLkTailWords];
    const bool fused = BLOCK3D && G.fused_pick != 0u;
    if (fused) {
        if (sub == 0u) {
            s_minkey = 0xFFFFFFFFu;
            s_qn = 0u;
            // chip-wide step: which of the two tour buffers is current changes hands here — no kernel reads it during a scan
            if (G.chip_step && idx == 0u) G.state->flip = G.state->flip_next;
        }
        TL_SYNC();
    }
    const uint32_t t1 = G.city_ids[idx >> 1];
    const uint32_t t2 = (idx & 1u) ? G.prev[t1] : G.next[t1];
    const float2 p1 = G.xy[t1], p2 = G.xy[t2];
    uint32_t chain[kLkMaxChain];
    uint32_t clen = 0;
    chain[0] = t1;
    chain[1] = t2;
    const float g0 = t1 == t2 ? 0.0f : dist(p1, p2);
    if (fused && G.split_levels == 3u) {
        // (PK: the packed view, where the step kernel keeps LkArgs::nx — an instantiation of its own, the classic one's code is untouched)
        using VT = typename std::conditional<PK, LkViewPk, LkView>::type;
        VT V;
        if constexpr (PK) V = LkViewPk{G.candd, G.nx, G.k, G.max_depth};
        else V = LkView{G.xy, G.cand, G.next, G.k, G.max_depth};
        // Deferred tails.  What a scan waits for is the few lanes whose walk survives the three split levels and goes on
        // alone through up to k + k^2 candidates, three dependent look-ups each (measured: 58 us per scan, 23 us with
        // those walks cut off).  So a surviving lane parks its state in LDS and the workgroup — most of whose lanes failed
        // their first test long ago — deals the next two levels out again: lane = (parked walk, candidate q3 at depth 3,
        // closing test or candidate at depth 4).  The order key (sub, q3, s4) is the walk's DFS order, so the smallest
        // key with a chain is the reference's first chain.
        const uint32_t nthr = blockDim.x * blockDim.y * blockDim.z, k1 = G.k + 1u, per = G.k * k1;
        uint32_t mykey = 0xFFFFFFFFu;
        float2 p_open;
        float gain;
        const int st = lk_subsearch3_front(V, chain, clen, p1, t2, p2, g0, q1, s1, s2, p_open, gain);
        if (st == 1) mykey = sub * (per + 1u);
        if (st == 2) {
            const uint32_t slot = atomicAdd(&s_qn, 1u);
            if (slot < kLkTailCap) {
#pragma unroll
                for (int t = 0; t < 6; ++t) s_q[slot][t] = chain[2 + t];
                s_q[slot][6] = __float_as_uint(gain);
                s_q[slot][7] = sub;
                s_q[slot][8] = __float_as_uint(p_open.x);
                s_q[slot][9] = __float_as_uint(p_open.y);
            } else if (lk_chain_from3(V, chain, clen, p1, p_open, gain)) {  // queue full: walk on alone
                mykey = sub * (per + 1u);
            }
        }
        TL_SYNC();
        const uint32_t nq = s_qn < kLkTailCap ? s_qn : kLkTailCap;
        for (uint32_t w = sub; w < nq * per; w += nthr) {
            const uint32_t e = w / per, r = w - e * per, q3 = r / k1, s4 = r - q3 * k1;
            const uint32_t key = s_q[e][7] * (per + 1u) + 1u + r;
            if (key >= mykey) continue;  // this lane already holds an earlier chain
            uint32_t c2[kLkMaxChain];
            uint32_t l2 = 0;
            c2[0] = t1;
            c2[1] = t2;
#pragma unroll
            for (int t = 0; t < 6; ++t) c2[2 + t] = s_q[e][t];
            const float2 po = make_float2(__uint_as_float(s_q[e][8]), __uint_as_float(s_q[e][9]));
            if (lk_tail_branch(V, c2, l2, p1, po, __uint_as_float(s_q[e][6]), q3, s4)) {
                mykey = key;
                clen = l2;
#pragma unroll
                for (int t = 0; t < kLkMaxChain; ++t) chain[t] = c2[t];
            }
        }
        if (mykey != 0xFFFFFFFFu) atomicMin(&s_minkey, mykey);
        TL_SYNC();
        if (mykey != 0xFFFFFFFFu && s_minkey == mykey && chain_valid(chain, clen, G.tour, G.pos, n)) {
            uint32_t *slot = G.chains + (size_t)idx * kLkSlot;
            slot[0] = clen;
            for (uint32_t t = 0; t < clen; ++t) slot[1 + t] = chain[t];
            if (G.chip_step) {  // the chain's tour positions and the move's segment table, for the step kernel (a call: see lk_file_move)
                lk_file_move(slot, clen, G.pos, n);
                atomicMin(&G.state->key2[G.parity], idx);
            } else {
                atomicMin(&G.state->key, idx);
            }
        }
        return;
    }
    LkView V{G.xy, G.cand, G.next, G.k, G.max_depth};
    const bool got = G.split_levels == 3u ? lk_subsearch3<LkView>(V, chain, clen, p1, t2, p2, g0, q1, s1, s2)
                                          : lk_subsearch<LkView>(V, chain, clen, p1, t1, t2, p2, g0, q1, s1);
    if (fused) {
        if (got) atomicMin(&s_minkey, sub);
        TL_SYNC();
        if (got && s_minkey == sub && chain_valid(chain, clen, G.tour, G.pos, n)) {
            uint32_t *slot = G.chains + (size_t)idx * kLkSlot;
            slot[0] = clen;
            for (uint32_t t = 0; t < clen; ++t) slot[1 + t] = chain[t];
            atomicMin(&G.state->key, idx);
        }
        return;
    }
    if (got) {
        if (G.subchains) {  // keep the chain: the pick step reads the winner's instead of walking it again
            uint32_t *slot = G.subchains + g * kLkSubSlot;
            slot[0] = clen;
#pragma unroll
            for (int t = 0; t < kLkMaxChain; ++t) slot[1 + t] = chain[t];
        }
        atomicMin(&G.pairmin[idx], sub);
    }
}

#ifdef TL_TUNE
#include "lk_scan_persist.h"
#endif

__global__ __launch_bounds__(256) void k_lk_scan_pick(LkArgs G)
{
    LkState *S = G.state;
    if (S->finished) return;
    const uint32_t n = G.n, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= 2u * n || idx >= S->window) return;
    const uint32_t sub = G.pairmin[idx];
    if (sub == 0xFFFFFFFFu) return;
    G.pairmin[idx] = 0xFFFFFFFFu;  // ready for the next scan
    const uint32_t t1 = G.city_ids[idx >> 1];
    const uint32_t t2 = (idx & 1u) ? G.prev[t1] : G.next[t1];
    const float2 p1 = G.xy[t1], p2 = G.xy[t2];
    uint32_t chain[kLkMaxChain];
    uint32_t clen = 0;
    bool have;
    if (G.subchains) {
        const uint32_t *src = G.subchains + ((uint64_t)idx * lk_subs(G) + sub) * kLkSubSlot;
        clen = src[0];
#pragma unroll
        for (int t = 0; t < kLkMaxChain; ++t) chain[t] = src[1 + t];
        have = true;
    } else {
        chain[0] = t1;
        chain[1] = t2;
        const float g0 = t1 == t2 ? 0.0f : dist(p1, p2);
        have = lk_run_sub(G, chain, clen, p1, t1, t2, p2, g0, sub);
    }
    if (have && chain_valid(chain, clen, G.tour, G.pos, n)) {
        uint32_t *slot = G.chains + (size_t)idx * kLkSlot;
        slot[0] = clen;
        for (uint32_t t = 0; t < clen; ++t) slot[1 + t] = chain[t];
        atomicMin(&S->key, idx);
    }
}

// The state machine behind a scan.  CHIP (n >= kLkRebuildSplitN with the fused scan): one launch of ceil(n / 1024) workgroups
// does what k_lk_control + k_lk_rebuild do in two — every workgroup reads the move's segment table (which the scan lane that
// validated the chain left in the pair's slot, lk_file_move) and writes its slice of the new tour into the OTHER tour buffer
// together with rank / successor / predecessor; workgroup 0 also keeps the counters, and runs the pass-end logic alone when the
// scan found nothing.  What other workgroups of the same launch read is never written in it: the scan's key is double-buffered
// by the round's parity (a launch argument) and the current-buffer flag changes hands in the next scan.
template <bool CHIP>
__global__ __launch_bounds__(kLkNT) void k_lk_control(LkArgs G)
{
    __shared__ uint32_t s_nseg;
    __shared__ LkSeg s_seg[kLkMaxSeg];
    __shared__ float s_part[kLkNT];
    LkState *S = G.state;
    if (S->finished) return;
    const uint32_t tid = threadIdx.x, n = G.n;
    uint32_t *tour = G.tour, *alt = G.alt, *pos = G.pos, *next = G.next, *prev = G.prev, *best = G.best;
    if (CHIP && S->flip) {
        tour = G.alt;
        alt = G.tour;
    }
    const float2 *__restrict__ xy = G.xy;

    auto rebuild = [&]() {
        for (uint32_t r = tid; r < n; r += kLkNT) {
            const uint32_t c = tour[r], cn = tour[r + 1u == n ? 0u : r + 1u];
            pos[c] = r;
            next[c] = cn;
            prev[c] = tour[r == 0u ? n - 1u : r - 1u];
            if (G.nx) G.nx[c] = nx_record(xy, c, cn);
        }
    };

    // tour_distance (:118-122): sequential f32 from 0, closing edge last (k_lk_solve's copy: lk_chain.h's header says why there are two)
    auto tour_distance = [&](const uint32_t *t) -> float {
        float total = 0.0f;
        for (uint32_t base = 0; base < n; base += kLkNT) {
            const uint32_t r = base + tid;
            if (r < n) {
                const uint32_t a = t[r], b = t[r + 1u == n ? 0u : r + 1u];
                s_part[tid] = a == b ? 0.0f : dist(xy[a], xy[b]);
            }
            TL_SYNC();
            if (tid == 0) {
                const uint32_t cnt = (n - base) < (uint32_t)kLkNT ? (n - base) : (uint32_t)kLkNT;
                for (uint32_t q = 0; q < cnt; ++q) total += s_part[q];
            }
            TL_SYNC();
        }
        if (tid == 0) s_part[0] = total;
        TL_SYNC();
        const float r = s_part[0];
        TL_SYNC();
        return r;
    };

    // lin_kernighan.rs:71,90 send_progress(best_tour, best_dist): the tour just copied into `best` and its length, appended to
    // the caller's snapshot list (tl_lk_trace)
    auto snapshot = [&](const uint32_t *t, float d) {
        if (!G.snap) return;
        const uint32_t sidx = S->snaps;
        TL_SYNC();  // every thread has read the count
        if (G.snap_ring || sidx < G.snap_cap) {  // ring (tl_lk_live: the host drains it between polls) or a list of the first snap_cap
            const uint32_t at = G.snap_ring ? sidx % G.snap_cap : sidx;
            for (uint32_t r = tid; r < n; r += kLkNT) G.snap[(size_t)at * n + r] = t[r];
            if (tid == 0) G.snap_dist[at] = d;
        }
        if (tid == 0) S->snaps = sidx + 1u;
    };

    const uint32_t key = CHIP ? S->key2[G.parity] : S->key;
    if (!CHIP && tid == 0) S->applied = 0u;  // set again below if this round applies a move (k_lk_rebuild runs after every control)
    TL_SYNC();
    if (key != 0xFFFFFFFFu) {
        // ---- apply_lk_chain (:397-450), then rescan (lk_pass loop :468-478)
        const uint32_t *slot = G.chains + (size_t)key * kLkSlot;
        const uint32_t clen = slot[0];
        if (CHIP) {
            // the scan lane that validated this chain filed the move's segment table in the slot (lk_file_move)
            if (tid == 0) s_nseg = slot[kLkSlotSeg];
            if (tid < 4u * kLkMaxSeg) reinterpret_cast<uint32_t *>(s_seg)[tid] = slot[kLkSlotSeg + 1u + tid];
        } else if (tid == 0) {
            uint32_t chain[kLkMaxChain];
            for (uint32_t t = 0; t < clen; ++t) chain[t] = slot[1 + t];
            uint32_t cpos[kLkMaxChain];
            chain_positions(chain, clen, pos, cpos);
            s_nseg = lk_build_segments(cpos, clen, n, s_seg);
        }
        TL_SYNC();
        const uint32_t nseg = s_nseg;
        if (CHIP) {
            // this workgroup's slice of the new tour: the city at new position d comes from old position seg_src(d)
            for (uint32_t r = blockIdx.x * kLkNT + tid; r < n; r += gridDim.x * kLkNT) {
                const uint32_t c = tour[seg_src(s_seg, nseg, r, n)], cn = tour[seg_src(s_seg, nseg, r + 1u == n ? 0u : r + 1u, n)],
                               cp = tour[seg_src(s_seg, nseg, r == 0u ? n - 1u : r - 1u, n)];
                alt[r] = c;
                pos[c] = r;
                next[c] = cn;
                prev[c] = cp;
                if (G.nx) G.nx[c] = nx_record(xy, c, cn);
            }
            if (blockIdx.x == 0 && tid == 0) {
                S->scans += 1;
                S->searches += (uint64_t)key + 1u;
                S->moves += 1;
                S->exchanged += clen / 2u;
                if (++S->pass_moves > lk_pass_cap(n)) S->finished = 2u;  // a cycling lk_pass (see lk_pass_cap): the host reports it
                S->key2[G.parity ^ 1u] = 0xFFFFFFFFu;  // the next scan's key
                const uint32_t w = key + kLkWindowMargin;
                S->window = w < 2u * n ? w : 2u * n;
                S->flip_next = S->flip ^ 1u;
            }
            return;
        }
        for (uint32_t sidx = 0; sidx < nseg; ++sidx) {
            const LkSeg sg = s_seg[sidx];
            for (uint32_t t = tid; t < sg.len; t += kLkNT) alt[sg.dst + t] = tour[seg_pos(sg, t, n)];
        }
        // the new tour is in `alt`: copy it back and rebuild rank / successor / predecessor — here for small tours, in
        // k_lk_rebuild on all CUs for large ones (3n scattered stores are slow from one CU)
        if (n < kLkRebuildSplitN) {
            TL_SYNC();
            for (uint32_t r = tid; r < n; r += kLkNT) {
                const uint32_t c = alt[r];
                tour[r] = c;
                pos[c] = r;
                next[c] = alt[r + 1u == n ? 0u : r + 1u];
                prev[c] = alt[r == 0u ? n - 1u : r - 1u];
            }
        }
        if (tid == 0) {
            S->applied = n < kLkRebuildSplitN ? 0u : 1u;
            S->scans += 1;
            S->searches += (uint64_t)key + 1u;
            S->moves += 1;
            S->exchanged += clen / 2u;
            if (++S->pass_moves > lk_pass_cap(n)) S->finished = 2u;
            S->key = 0xFFFFFFFFu;
            // find_lk_move restarts at pair 0 after every move (:468-478) and keeps the LOWEST pair with a valid chain, so a
            // scan of a prefix that contains a hit is a complete scan.  The pairs before this hit had no valid chain a moment
            // ago; the next hit is most often near or behind this one: look at [0, key + margin) first.
            const uint32_t w = key + kLkWindowMargin;
            S->window = w < 2u * n ? w : 2u * n;
        }
        return;
    }
    if (CHIP) {  // no move: workgroup 0 is the state machine
        if (blockIdx.x != 0) return;
        if (tid == 0) {
            S->key2[G.parity ^ 1u] = 0xFFFFFFFFu;
            S->flip_next = S->flip;
        }
    }
    if (S->window < 2u * n) {  // nothing inside the prefix: the same find_lk_move goes on over all pairs
        TL_SYNC();
        if (tid == 0) S->window = 2u * n;
        return;
    }
    // ---- the scan found nothing: this lk_pass is over (:472-473)
    if (tid == 0) {
        S->scans += 1;
        S->searches += 2ull * n;
        S->pass_moves = 0u;
    }
    bool kick = false;
    if (S->stage == 0) {                       // initial pass done (:61-70)
        for (uint32_t r = tid; r < n; r += kLkNT) best[r] = tour[r];
        TL_SYNC();
        const float bd = tour_distance(best);
        if (tid == 0) {
            S->best_dist = bd;
            S->stage = 1;
            S->epoch = 0;
            S->platoo = 0;
        }
        snapshot(tour, bd);
        kick = G.epochs > 0;
    } else {                                    // an epoch's pass done (:85-96)
        const float dcur = tour_distance(tour);
        const bool better = dcur < S->best_dist;
        TL_SYNC();
        bool stop = false;
        if (better) {
            for (uint32_t r = tid; r < n; r += kLkNT) best[r] = tour[r];
            snapshot(tour, dcur);
        }
        uint32_t platoo = S->platoo, epoch = S->epoch;
        TL_SYNC();
        if (better) platoo = 0;
        else if (++platoo >= G.platoo_epochs) stop = true;
        ++epoch;
        if (tid == 0) {
            if (better) S->best_dist = dcur;
            S->platoo = platoo;
            S->epoch = epoch;
        }
        kick = !stop && epoch < G.epochs;
    }
    TL_SYNC();
    if (!kick) {
        if (tid == 0) S->finished = 1;
        return;
    }
    // ---- double_bridge (:485-499) into `tour`, then a fresh lk_pass: city_ids = tour (:466)
    if (n < 8) {
        for (uint32_t r = tid; r < n; r += kLkNT) tour[r] = best[r];
    } else {
        const uint64_t draws = S->draws;
        uint32_t p1, p2, p3;
        double_bridge_cuts(G.seed, draws, n, p1, p2, p3);
        for (uint32_t w = tid; w < n; w += kLkNT) tour[w] = best[double_bridge_src(w, p1, p2, p3)];
        TL_SYNC();
        if (tid == 0) S->draws = draws + 3;
    }
    TL_SYNC();
    for (uint32_t r = tid; r < n; r += kLkNT) G.city_ids[r] = tour[r];
    rebuild();
    if (tid == 0) {
        S->key = 0xFFFFFFFFu;
        S->window = kLkWindowFirst < 2u * n ? kLkWindowFirst : 2u * n;  // a fresh pass: hits start at the front
    }
}

// after a move: tour = alt, rank / successor / predecessor of every city — spread over the chip
__global__ __launch_bounds__(256) void k_lk_rebuild(LkArgs G)
{
    LkState *S = G.state;
    if (S->finished || !S->applied) return;
    const uint32_t n = G.n, r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t c = G.alt[r];
    G.tour[r] = c;
    G.pos[c] = r;
    G.next[c] = G.alt[r + 1u == n ? 0u : r + 1u];
    G.prev[c] = G.alt[r == 0u ? n - 1u : r - 1u];
}

// first lk_pass of solve(): city_ids = tour, next/prev/pos from tour, state reset
__global__ __launch_bounds__(kLkNT) void k_lk_begin(LkArgs G)
{
    const uint32_t tid = threadIdx.x, n = G.n;
    for (uint32_t r = tid; r < n; r += kLkNT) {
        const uint32_t c = G.tour[r], cn = G.tour[r + 1u == n ? 0u : r + 1u];
        G.city_ids[r] = c;
        G.best[r] = c;
        G.pos[c] = r;
        G.next[c] = cn;
        G.prev[c] = G.tour[r == 0u ? n - 1u : r - 1u];
        if (G.nx) G.nx[c] = nx_record(G.xy, c, cn);
    }
    if (G.candd) {  // the candidates with their distances, once per call
        for (size_t e = tid; e < (size_t)n * G.k; e += kLkNT) {
            const uint32_t c = G.cand[e];
            G.candd[e] = make_uint2(c, __float_as_uint(dist(G.xy[e / G.k], G.xy[c])));
        }
    }
    if (tid == 0) {
        LkState *S = G.state;
        S->snaps = 0u;
        S->key = 0xFFFFFFFFu;
        S->key2[0] = S->key2[1] = 0xFFFFFFFFu;
        S->flip = S->flip_next = 0u;
        S->finished = n < 4 ? 1u : 0u;  // :57-59
        S->stage = 0;
        S->epoch = 0;
        S->platoo = 0;
        S->best_dist = 0.0f;
        S->draws = 0;
        S->scans = S->searches = S->moves = S->exchanged = 0;
        S->window = kLkWindowFirst < 2u * n ? kLkWindowFirst : 2u * n;
        S->applied = 0u;
        S->pass_moves = 0u;
    }
}

hipError_t launch_lk_begin(const LkArgs &G, hipStream_t s)
{
    hipLaunchKernelGGL(k_lk_begin, dim3(1), dim3(kLkNT), 0, s, G);
    return hipGetLastError();
}

hipError_t launch_lk_round(const LkArgs &G0, hipStream_t s, uint32_t round)
{
    LkArgs G = G0;
    G.parity = round & 1u;
    if (G.pairmin) {  // split scan
        const uint64_t lanes = (uint64_t)2u * G.n * G.k * (G.k + 1u) * (G.split_levels == 3u ? G.k + 1u : 1u);
        const uint32_t k1 = G.k + 1u, per_pair = lk_subs(G);
#ifdef TL_TUNE
        if (per_pair <= 1024u && G.persist_blocks && G.fused_pick && G.split_levels == 3u) {
            // persistent form: a fixed grid strides over the window's pairs (k_lk_scan_persist)
            const uint32_t grid = G.persist_blocks < 2u * G.n ? G.persist_blocks : 2u * G.n;
            hipLaunchKernelGGL(k_lk_scan_persist, dim3(grid), dim3(k1, k1, G.k), 0, s, G);
        } else
#endif
        if (per_pair <= 1024u) {  // one workgroup per pair, thread coordinates = sub-search digits
            const dim3 blk = G.split_levels == 3u ? dim3(k1, k1, G.k) : dim3(k1, G.k, 1);
            if (G.nx && G.fused_pick && G.split_levels == 3u) hipLaunchKernelGGL((k_lk_scan_sub<true, true>), dim3(2u * G.n), blk, 0, s, G);
            else hipLaunchKernelGGL(k_lk_scan_sub<true>, dim3(2u * G.n), blk, 0, s, G);
        } else {
            hipLaunchKernelGGL(k_lk_scan_sub<false>, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, s, G);
        }
        if (!(G.fused_pick && per_pair <= 1024u)) hipLaunchKernelGGL(k_lk_scan_pick, dim3((2u * G.n + 255u) / 256u), dim3(256), 0, s, G);
    } else {
        const size_t lds = (size_t)G.n * 10;
        if (G.n < 65536u && lds <= (size_t)G.lds_budget) {
            hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_lk_scan<true>));
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_lk_scan<true>, dim3((2u * G.n + 255u) / 256u), dim3(256), lds, s, G);
        } else {
            hipLaunchKernelGGL(k_lk_scan<false>, dim3((2u * G.n + 255u) / 256u), dim3(256), 0, s, G);
        }
    }
    if (G.chip_step) {
        hipLaunchKernelGGL(k_lk_control<true>, dim3((G.n + kLkNT - 1u) / kLkNT), dim3(kLkNT), 0, s, G);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_lk_control<false>, dim3(1), dim3(kLkNT), 0, s, G);
    if (G.n >= kLkRebuildSplitN) hipLaunchKernelGGL(k_lk_rebuild, dim3((G.n + 255u) / 256u), dim3(256), 0, s, G);
    return hipGetLastError();
}

size_t lk_chain_slot_words() { return (size_t)kLkSlot; }
size_t lk_sub_slot_words() { return (size_t)kLkSubSlot; }
uint32_t lk_max_depth() { return (uint32_t)kLkMaxDepth; }
