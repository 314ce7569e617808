// lk_chain.h — what every form of the Lin–Kernighan solver shares on the device (a part of lk.hip, included inside its namespace;
// lk.hip's header is the map of the forms): the constants and slot layouts, the two views of a tour with their probes, the chain
// search find_lk_chain (lin_kernighan.rs:265-340), the arc model of a closed chain with its validity walk and segment table, and
// the small index helpers of the move application (seg_pos, seg_src), of the packed view (nx_record) and of the double-bridge
// kick (double_bridge_cuts, double_bridge_src).
//
// The reference checks chain validity and applies chains by rebuilding adjacency lists and tracing n cities
// (:181-250, :397-450).  Here both are O(k): the k removed edges cut the tour into k arcs; walking arcs through
// the k added edges visits all k arcs iff the result is one cycle (the new graph is 2-regular), and the new flat
// tour is those arcs copied in walk order starting at tour[0] — forward if the edge (tour[0],tour[1]) survives,
// else backward, which is what the reference's trace from `adj[start][0]` does.
//
// The rule of chain_tour.h's and swarm_tour.h's headers holds here: a helper is in this file only while every kernel that uses it
// compiles to the instructions it had with its own copy (scripts/isa_diff.py; NOTEBOOK.md, the entry of this header).  What that
// rule kept in the kernels, to be changed in step:
//   the ordered tour_distance lambda (k_lk_solve, k_lk_control): as one function 19 of k_lk_control<true>'s 1 519 instructions went;
//   the segment-by-segment copy (k_lk_solve, k_lk_control<false>): as one function 2 of 2 230 instructions changed; both call seg_pos;
//   kick_from_best of k_lk_ils: with double_bridge_cuts / _src 18 of <256>'s 5 625 instructions went, 21 of <512>'s, 7 of <1024>'s;
//   apply_move of k_lk_ils: with seg_src <256> and <512> gained 8 instructions, <1024> 6;
//   rank / successor / predecessor of a flat tour (five copies): they load and store in five orders, and no pointer is restrict.
// k_lk_solve is the one kernel that changed: it calls lk_build_segments where it had the table's loop written out (7 023 -> 7 003).
#pragma once

namespace {

constexpr float kLkEps = 1e-6f;  // lin_kernighan.rs:252
// moves after which an lk_pass is taken to be cycling (the reference's loop does not end on such an input: lin_kernighan.rs:468-478
// goes on while find_lk_move returns a chain, and a chain's "gain" is a sum of rounded f32 terms).  A pass from a random tour takes
// about n moves.
__host__ __device__ __forceinline__ uint64_t lk_pass_cap(uint32_t n) { return 64ull * n + 4096ull; }
constexpr int kLkNT = 1024;
#ifndef TL_LK_WINDOW_MARGIN
#define TL_LK_WINDOW_MARGIN 2048
#endif
constexpr uint32_t kLkWindowMargin = TL_LK_WINDOW_MARGIN;  // pairs scanned beyond the previous hit before the whole pass is looked at
constexpr uint32_t kLkRebuildSplitN = 1500;                // from this size on the post-move rebuild is its own chip-wide kernel
constexpr uint32_t kLkWindowFirst = 4096;                  // prefix of a fresh pass

template <typename NextT>
struct LkViewT {
    const float2 *xy;      // global, or an LDS copy (k_lk_scan)
    const uint32_t *cand;
    const NextT *next;     // successor in the current tour; u16 LDS copy in k_lk_scan
    uint32_t k;
    uint32_t max_depth;
};
using LkView = LkViewT<uint32_t>;

// The packed view (round 5): what a branch of the chain search needs of a candidate and of a tour successor sits
// NEXT TO the index it follows from — candd[t][q] = (candidate id, d(t, candidate)), nx[c] = (next[c], x, y of next[c], d(c, next[c])) —
// so that a branch costs two dependent look-ups (candd -> nx) instead of four (cand -> xy -> next -> xy) and one square root (the
// closing edge) instead of three.  The two distances are the same f32 values the classic view computes (same operands, same order).
struct LkViewPk {
    const uint2 *candd;   // [n][k]: candidate id, bits of d(t, candidate)
    const float4 *nx;     // [n]: bits of next[c], next[c]'s x, y, d(c, next[c]) of the CURRENT tour (kept by the step kernel)
    uint32_t k;
    uint32_t max_depth;
};
// candidate q of t_open: its id, d(t_open, id), and next[t_open] (for is_tour_edge)
template <typename NextT>
__device__ __forceinline__ void lk_probe(const LkViewT<NextT> &V, uint32_t t_open, float2 p_open, uint32_t q, uint32_t &t_next, float2 &p_next, float &d1)
{
    t_next = V.cand[(size_t)t_open * V.k + q];
    p_next = V.xy[t_next];
    d1 = dist(p_open, p_next);
}
__device__ __forceinline__ void lk_probe(const LkViewPk &V, uint32_t t_open, float2, uint32_t q, uint32_t &t_next, float2 &p_next, float &d1)
{
    const uint2 c = V.candd[(size_t)t_open * V.k + q];
    t_next = c.x;
    p_next = make_float2(0.0f, 0.0f);  // (not needed: both of its distances come ready)
    d1 = __uint_as_float(c.y);
}
template <typename NextT>
__device__ __forceinline__ uint32_t lk_next_of(const LkViewT<NextT> &V, uint32_t c) { return (uint32_t)V.next[c]; }
__device__ __forceinline__ uint32_t lk_next_of(const LkViewPk &V, uint32_t c) { return __float_as_uint(V.nx[c].x); }
// regime A: t_break = next[t_next], its point, d(t_next, t_break)
template <typename NextT>
__device__ __forceinline__ uint32_t lk_break_id(const LkViewT<NextT> &V, uint32_t t_next, float4 &rec)
{
    (void)rec;
    return (uint32_t)V.next[t_next];
}
__device__ __forceinline__ uint32_t lk_break_id(const LkViewPk &V, uint32_t t_next, float4 &rec)
{
    rec = V.nx[t_next];
    return __float_as_uint(rec.x);
}
template <typename NextT>
__device__ __forceinline__ void lk_break_pt(const LkViewT<NextT> &V, uint32_t t_break, float2 p_next, const float4 &, float2 &p_break, float &d2)
{
    p_break = V.xy[t_break];
    d2 = dist(p_next, p_break);
}
__device__ __forceinline__ void lk_break_pt(const LkViewPk &, uint32_t, float2, const float4 &rec, float2 &p_break, float &d2)
{
    p_break = make_float2(rec.y, rec.z);
    d2 = rec.w;
}
// the packed view's record of c, whose successor is cn: the successor, its point, the tour edge's length
__device__ __forceinline__ float4 nx_record(const float2 *xy, uint32_t c, uint32_t cn)
{
    const float2 pn = xy[cn];
    return make_float4(__uint_as_float(cn), pn.x, pn.y, dist(xy[c], pn));
}

__host__ __device__ __forceinline__ uint32_t lk_subs(const LkArgs &G)  // sub-searches per (t1, orientation) pair
{
    return G.k * (G.k + 1u) * (G.split_levels == 3u ? G.k + 1u : 1u);
}

constexpr int kLkMaxDepth = TL_LK_MAX_DEPTH;         // compile-time recursion bound (6: default max_depth = 5; 16: the deep build, lk_deep.hip)
constexpr int kLkMaxChain = 2 * kLkMaxDepth + 2;
// u32 words per pair in LkArgs::chains: length, the chain's cities, (chip-wide step) their tour positions, then the segment count and
// the move's segment table (src, len, dst, dir per segment: the scan's validating lane builds it, round 4) — 96 at depth 6
constexpr uint32_t kLkMaxSeg = 2u * ((uint32_t)kLkMaxDepth + 2u);
constexpr uint32_t kLkSlotSeg = 1u + 2u * (uint32_t)kLkMaxChain;  // word of the segment count; the table follows
constexpr uint32_t kLkSlot = ((kLkSlotSeg + 1u + 4u * kLkMaxSeg + 31u) / 32u) * 32u;
constexpr uint32_t kLkTailCap = 48, kLkTailWords = 10;  // parked depth-3 walks of one scan workgroup (k_lk_scan_sub)
// u32 words per kept sub-search chain (len + kLkMaxChain cities, 64-byte slots): 16 at depth 6
constexpr uint32_t kLkSubSlot = ((1u + (uint32_t)kLkMaxChain + 15u) / 16u) * 16u;
static_assert(kLkMaxChain + 1 <= (int)kLkSubSlot && 1 + 2 * kLkMaxChain <= (int)kLkSlot, "chain slots");
static_assert(TL_LK_MAX_DEPTH != 6 || (kLkSlot == 96u && kLkSubSlot == 16u), "the default build's layout");

template <int LEN>
__device__ __forceinline__ bool in_chain(const uint32_t (&chain)[kLkMaxChain], uint32_t x)
{
    bool f = false;
#pragma unroll
    for (int t = 0; t < LEN; ++t) f |= (chain[t] == x);
    return f;
}

// lin_kernighan.rs:265-340 find_lk_chain; DEPTH is the reference's `depth`, chain holds 2*DEPTH+2 cities on entry.
template <int DEPTH, typename VT>
__device__ bool lk_chain(const VT &V, uint32_t (&chain)[kLkMaxChain], uint32_t &clen, const float2 p1,
                         const uint32_t t_open, const float2 p_open, const float gain)
{
    if (DEPTH >= 1) {
        const float close_gain = gain - dist(p_open, p1);  // :280-283
        if (close_gain > kLkEps) {
            clen = 2 * DEPTH + 2;
            return true;
        }
    }
    if ((uint32_t)DEPTH >= V.max_depth) return false;  // :286-288
    if constexpr (DEPTH < kLkMaxDepth) {
        for (uint32_t q = 0; q < V.k; ++q) {
            uint32_t t_next;
            float2 p_next, p_break;
            float d1, d2;
            float4 rec;
            lk_probe(V, t_open, p_open, q, t_next, p_next, d1);
            const float g1 = gain - d1;
            if (g1 <= kLkEps) break;                                   // :292-295 candidates are sorted
            if (in_chain<2 * DEPTH + 2>(chain, t_next)) continue;      // used[t_next]
            const uint32_t t_break = lk_break_id(V, t_next, rec);      // :305 regime A
            if (lk_next_of(V, t_open) == t_next || t_break == t_open) continue;  // is_tour_edge: prev[a]==b <=> next[b]==a
            if (in_chain<2 * DEPTH + 2>(chain, t_break)) continue;     // used[t_break]
            lk_break_pt(V, t_break, p_next, rec, p_break, d2);
            const float g2 = g1 + d2;
            chain[2 * DEPTH + 2] = t_next;
            chain[2 * DEPTH + 3] = t_break;
            if (lk_chain<DEPTH + 1, VT>(V, chain, clen, p1, t_break, p_break, g2)) return true;
        }
    }
    return false;
}

// Arc model of a closed chain c[0..2k): removed edges (c[2i],c[2i+1]), added edges (c[2i+1],c[2i+2]) and (c[2k-1],c[0]).
struct Arcs {
    uint32_t lo[kLkMaxDepth + 1];  // sorted: removed edge m joins positions lo[m] and lo[m]+1 (mod n)
    uint32_t k;
};

// Tour positions of the chain's cities, all loads independent (one L2 latency).  Every arc boundary of the arc model is the
// position of a chain city, so the validity walk and the application need no further pos[] / tour[] look-ups: the city
// at a boundary position is found among these (index_at), its added-edge partner by index (partner_index).
template <typename PosT>
__device__ __forceinline__ void chain_positions(const uint32_t (&chain)[kLkMaxChain], uint32_t clen, const PosT *pos,
                                                uint32_t (&cpos)[kLkMaxChain])
{
#pragma unroll
    for (int t = 0; t < kLkMaxChain; ++t) cpos[t] = (uint32_t)t < clen ? pos[chain[t]] : 0xFFFFFFFFu;
}
__device__ __forceinline__ uint32_t sel_at(const uint32_t (&a)[kLkMaxChain], uint32_t idx)
{
    uint32_t r = 0xFFFFFFFFu;
#pragma unroll
    for (int t = 0; t < kLkMaxChain; ++t) r = ((uint32_t)t == idx) ? a[t] : r;
    return r;
}
__device__ __forceinline__ uint32_t index_at(const uint32_t (&cpos)[kLkMaxChain], uint32_t clen, uint32_t p)
{
    uint32_t idx = 0xFFFFFFFFu;
#pragma unroll
    for (int t = kLkMaxChain - 1; t >= 0; --t) idx = ((uint32_t)t < clen && cpos[t] == p) ? (uint32_t)t : idx;
    return idx;
}
__device__ __forceinline__ uint32_t partner_index(uint32_t t, uint32_t clen)  // the city joined to chain[t] by an added edge
{
    if (t == 0u) return clen - 1u;
    if (t == clen - 1u) return 0u;
    return (t & 1u) ? t + 1u : t - 1u;
}

__device__ __forceinline__ void arcs_build(const uint32_t (&cpos)[kLkMaxChain], uint32_t clen, uint32_t n, Arcs &A)
{
    A.k = clen / 2;
#pragma unroll
    for (int m = 0; m < kLkMaxDepth + 1; ++m) {
        if ((uint32_t)m >= A.k) break;
        const uint32_t pu = cpos[2 * m], pv = cpos[2 * m + 1];
        // adjacent positions: the edge sits after the one whose successor is the other
        A.lo[m] = ((pu + 1u == pv) || (pu == n - 1u && pv == 0u)) ? pu : pv;
    }
    for (uint32_t a = 1; a < A.k; ++a) {  // insertion sort, k <= 7
        const uint32_t v = A.lo[a];
        uint32_t b = a;
        while (b > 0 && A.lo[b - 1] > v) { A.lo[b] = A.lo[b - 1]; --b; }
        A.lo[b] = v;
    }
}

// endpoint city at position p: is its removed edge behind it (p is an arc START) and where is the arc's other end
__device__ __forceinline__ bool arc_is_start(const Arcs &A, uint32_t p, uint32_t n)
{
    const uint32_t before = p == 0u ? n - 1u : p - 1u;
    for (uint32_t m = 0; m < A.k; ++m)
        if (A.lo[m] == before) return true;
    return false;
}
__device__ __forceinline__ uint32_t arc_end_from_start(const Arcs &A, uint32_t p)
{
    // smallest lo >= p, else (wrap) the smallest lo
    for (uint32_t m = 0; m < A.k; ++m)
        if (A.lo[m] >= p) return A.lo[m];
    return A.lo[0];
}
__device__ __forceinline__ uint32_t arc_start_from_end(const Arcs &A, uint32_t p, uint32_t n)
{
    // largest lo < p, +1; else (wrap) largest lo + 1
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t m = 0; m < A.k; ++m)
        if (A.lo[m] < p) best = A.lo[m];
    if (best == 0xFFFFFFFFu) best = A.lo[A.k - 1];
    return best + 1u == n ? 0u : best + 1u;
}
// chain_is_valid_tour (lin_kernighan.rs:181-250): one Hamiltonian cycle <=> the arc walk sees all k arcs
// (cpos: the chain's tour positions — chain_positions — which the caller may want to keep for lk_build_segments)
__device__ bool chain_valid_at(const uint32_t (&cpos)[kLkMaxChain], uint32_t clen, uint32_t n)
{
    if (clen < 4) return false;
    Arcs A;
    arcs_build(cpos, clen, n, A);
    uint32_t ti = 0, arcs = 0;  // chain cities are distinct: back at index 0 <=> back at chain[0]
    do {
        const uint32_t p = sel_at(cpos, ti);
        const uint32_t other = arc_is_start(A, p, n) ? arc_end_from_start(A, p) : arc_start_from_end(A, p, n);
        ++arcs;
        if (arcs > A.k) return false;
        const uint32_t tj = index_at(cpos, clen, other);  // the city at an arc boundary is a chain city
        if (tj == 0xFFFFFFFFu) return false;
        ti = partner_index(tj, clen);
    } while (ti != 0u);
    return arcs == A.k;
}
__device__ bool chain_valid(const uint32_t (&chain)[kLkMaxChain], uint32_t clen, const uint32_t *tour, const uint32_t *pos, uint32_t n)
{
    (void)tour;
    if (clen < 4) return false;
    uint32_t cpos[kLkMaxChain];
    chain_positions(chain, clen, pos, cpos);
    return chain_valid_at(cpos, clen, n);
}

struct LkSeg {
    uint32_t src, len, dst;
    int dir;
};

// apply_lk_chain (lin_kernighan.rs:397-450) as a table: the new flat tour is the old tour's arcs copied in walk order starting at
// tour[0] — forward if the edge (tour[0], tour[1]) survives, else backward.  cpos: tour positions of the chain's cities.
__device__ __forceinline__ uint32_t lk_build_segments(const uint32_t (&cpos)[kLkMaxChain], uint32_t clen, uint32_t n, LkSeg *seg)
{
    Arcs A;
    arcs_build(cpos, clen, n, A);
    bool first_removed = false;  // is the edge (tour[0], tour[1]) one of the removed ones?
    for (uint32_t m = 0; m < A.k; ++m) first_removed |= (A.lo[m] == 0u);
    uint32_t nseg = 0, emitted = 0, p = 0;
    int dir = first_removed ? -1 : +1;
    while (emitted < n && nseg < kLkMaxSeg) {
        const uint32_t endp = dir > 0 ? arc_end_from_start(A, p) : arc_start_from_end(A, p, n);
        uint32_t len = dir > 0 ? (endp >= p ? endp - p + 1u : endp + n - p + 1u) : (p >= endp ? p - endp + 1u : p + n - endp + 1u);
        if (len > n - emitted) len = n - emitted;
        seg[nseg].src = p;
        seg[nseg].len = len;
        seg[nseg].dst = emitted;
        seg[nseg].dir = dir;
        ++nseg;
        emitted += len;
        if (emitted >= n) break;
        p = sel_at(cpos, partner_index(index_at(cpos, clen, endp), clen));  // position of the boundary city's added-edge partner
        dir = arc_is_start(A, p, n) ? +1 : -1;
    }
    return nseg;
}

// the old position of the t-th city of segment sg
__device__ __forceinline__ uint32_t seg_pos(const LkSeg &sg, uint32_t t, uint32_t n)
{
    uint32_t sp = sg.dir > 0 ? sg.src + t : sg.src + n - t;
    if (sp >= n) sp -= n;
    return sp;
}
// the old position behind new position d (segments are in dst order)
__device__ __forceinline__ uint32_t seg_src(const LkSeg *seg, uint32_t nseg, uint32_t d, uint32_t n)
{
    uint32_t sidx = 0;
    while (sidx + 1u < nseg && d >= seg[sidx + 1u].dst) ++sidx;
    const LkSeg sg = seg[sidx];
    return seg_pos(sg, d - sg.dst, n);
}

// What the chip-wide step needs of a pair's valid chain, filed in the pair's slot by the scan lane that validated it (a call, not
// inlined: the scan kernel lives on 64 VGPRs, and this runs for the few pairs of a scan that hold a valid chain): the chain's tour
// positions (the step kernel rebuilds pos[] while its other workgroups still read it) and the move's segment table — which used
// to be ONE thread's serial prologue of every step workgroup (k_lk_control<true>: 8.5 us per round, of which ~3 were this).
__device__ __attribute__((noinline)) void lk_file_move(uint32_t *slot, uint32_t clen, const uint32_t *pos, uint32_t n)
{
    uint32_t cpos[kLkMaxChain];
#pragma unroll
    for (int t = 0; t < kLkMaxChain; ++t) cpos[t] = (uint32_t)t < clen ? pos[slot[1 + t]] : 0xFFFFFFFFu;
#pragma unroll
    for (int t = 0; t < kLkMaxChain; ++t) slot[1 + kLkMaxChain + t] = cpos[t];
    LkSeg seg[kLkMaxSeg];
    const uint32_t nseg = lk_build_segments(cpos, clen, n, seg);
    slot[kLkSlotSeg] = nseg;
    for (uint32_t q = 0; q < nseg; ++q) {
        slot[kLkSlotSeg + 1u + 4u * q] = seg[q].src;
        slot[kLkSlotSeg + 2u + 4u * q] = seg[q].len;
        slot[kLkSlotSeg + 3u + 4u * q] = seg[q].dst;
        slot[kLkSlotSeg + 4u + 4u * q] = (uint32_t)seg[q].dir;
    }
}

// double_bridge (lin_kernighan.rs:485-499) with seeded draws r = splitmix64 % (n / 4), n >= 8: the kick's three cut positions
__device__ __forceinline__ void double_bridge_cuts(uint64_t seed, uint64_t draws, uint32_t n, uint32_t &p1, uint32_t &p2, uint32_t &p3)
{
    const uint32_t qn = n / 4u;
    const uint32_t r1 = (uint32_t)(splitmix64_at(seed, draws) % qn), r2 = (uint32_t)(splitmix64_at(seed, draws + 1) % qn),
                   r3 = (uint32_t)(splitmix64_at(seed, draws + 2) % qn);
    p1 = 1u + r1;
    p2 = p1 + 1u + r2;
    p3 = p2 + 1u + r3;
}
// the old position behind position w of the kicked tour: tour[0..p1] ++ tour[p2..p3] ++ tour[p1..p2] ++ tour[p3..n]
__device__ __forceinline__ uint32_t double_bridge_src(uint32_t w, uint32_t p1, uint32_t p2, uint32_t p3)
{
    if (w < p1) return w;
    if (w < p1 + (p3 - p2)) return p2 + (w - p1);
    if (w < p3) return p1 + (w - p1 - (p3 - p2));
    return w;
}

}  // namespace
