// christofides.hip — the two stages of Christofides (reference: src/tsp/christofides.rs:12-166) that are not greedy_edge.hip's
// bands, DESIGN.md §4.13:
//   k_chr_prim   prim_mst (:75-114): n rounds, each taking the non-tree vertex of smallest key — the FIRST in position order
//                among equals (Iterator::min_by keeps the first minimum; the comparison is partial_cmp, so -0.0 equals +0.0) — and
//                then lowering key[v] to d(u, v), parent[v] = u, wherever d(u, v) < key[v] STRICTLY.  The rounds are a dependent
//                chain, so the whole tree is one launch of one workgroup: a grid-wide exchange per round would cost more than the
//                round.  A thread owns the cities tid, tid + 1024, ...; round r's update pass and round r + 1's argmin are one
//                sweep over them; the minimum of (ordered key bits << 32 | position) goes through the wave, then through one
//                LDS slot per wave, double-buffered by the round's parity so that a round has ONE barrier.
//   k_chr_odd    odd_degree_nodes (:120-127) from parent[], written as the band pipeline's start state: the odd vertices in
//                position order in the free list, "full" in the end table for every other city.
// The matching itself is greedy_edge.hip's walk in its matching mode; multigraph, Euler walk and shortcut are host code
// (tl_api_greedy.hip).
#include "tl_kernels.h"

#include <cfloat>

namespace tl {

namespace {

constexpr int kPrimThreads = 1024;
constexpr int kPrimWaves = kPrimThreads / 64;
constexpr uint16_t kChrNone = 0xFFFFu;  // no parent; also greedy_edge.hip's "full" mark of the end table (n <= 65 535)

// partial_cmp among non-NaN keys as an unsigned order: zero canonicalised (-0.0 == +0.0), then the total-order key.
// Keys are never NaN: a key is f32::MAX, 0.0, or a distance that passed `d < key`.
__device__ __forceinline__ uint32_t ordered_key(float k)
{
    uint32_t b = __builtin_bit_cast(uint32_t, k);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// LDS: key / par live in dynamic LDS (6n bytes), else in the workspace (key_g / par_g).  Which cities of a thread are in the tree
// is a 64-bit mask in a register either way: n <= 65 535 gives a thread at most 64 cities.
template <bool DM, bool LDS>
__global__ __launch_bounds__(kPrimThreads) void k_chr_prim(const float2 *__restrict__ xy, const float *__restrict__ dm, uint32_t n,
                                                           float *__restrict__ key_g, uint16_t *__restrict__ par_g,
                                                           uint16_t *__restrict__ parent, uint16_t *__restrict__ order,
                                                           uint32_t *__restrict__ status)
{
    extern __shared__ unsigned char chr_lds[];
    __shared__ uint64_t slot[2][kPrimWaves];
    __shared__ uint32_t sh_bad[2];
    float *key;
    uint16_t *par;
    if constexpr (LDS) {
        key = (float *)chr_lds;
        par = (uint16_t *)(chr_lds + (size_t)n * 4);
    } else {
        key = key_g;
        par = par_g;
    }
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t v = tid; v < n; v += kPrimThreads) {
        key[v] = v ? FLT_MAX : 0.0f;
        par[v] = kChrNone;
    }
    if (tid == 0) sh_bad[0] = sh_bad[1] = 0u;
    uint64_t mine = 0;  // bit k: city tid + 1024 k is in the tree
    uint32_t u = 0;     // round 0 takes position 0: its key 0.0 is below every f32::MAX, and it is the first
    for (uint32_t r = 0;; ++r) {
        if ((u & (kPrimThreads - 1)) == tid) {  // u's owner (its state is this thread's alone; sh_bad is a barrier behind its last writer)
            mine |= (uint64_t)1 << (u >> 10);
            const uint16_t p = par[u];
            parent[u] = p;
            order[r] = (uint16_t)u;
            if (r > 0 && p == kChrNone && sh_bad[0] == 0u) {  // no distance to u was below f32::MAX: the tree does not span
                sh_bad[1] = u;
                sh_bad[0] = 1u;
            }
        }
        if (r + 1 == n) break;
        float2 pu = make_float2(0.f, 0.f);
        if (!DM) pu = xy[u];
        uint64_t best = ~(uint64_t)0;
        uint32_t k = 0;
        for (uint32_t v = tid; v < n; v += kPrimThreads, ++k) {
            if ((mine >> k) & 1u) continue;
            float d;
            if (DM) d = v < u ? dm[(uint64_t)u * (u - 1) / 2 + v] : dm[(uint64_t)v * (v - 1) / 2 + u];  // (v != u: u is in the tree)
            else d = dist(pu, xy[v]);
            float kv = key[v];
            if (d < kv) {
                kv = d;
                key[v] = d;
                par[v] = (uint16_t)u;
            }
            const uint64_t c = ((uint64_t)ordered_key(kv) << 32) | v;
            best = c < best ? c : best;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
        if (lane == 0) slot[r & 1u][wave] = best;
        TL_SYNC();
        uint64_t m = slot[r & 1u][0];
        for (int w = 1; w < kPrimWaves; ++w) {
            const uint64_t o = slot[r & 1u][w];
            m = o < m ? o : m;
        }
        u = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
    }
    TL_SYNC();
    if (tid == 0) {
        status[0] = sh_bad[0];
        status[1] = sh_bad[1];
    }
}

constexpr int kOddWords = 65536 / 32;

__global__ __launch_bounds__(1024) void k_chr_odd(const uint16_t *__restrict__ parent, uint32_t n, uint16_t *__restrict__ end_g,
                                                  uint16_t *__restrict__ free, uint32_t *__restrict__ state)
{
    __shared__ uint32_t bits[kOddWords];  // degree parity of every city
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < (uint32_t)kOddWords; k += 1024) bits[k] = 0u;
    TL_SYNC();
    for (uint32_t v = tid; v < n; v += 1024) {
        const uint32_t p = parent[v];
        if (p < n) {  // the tree edge (v, parent[v])
            atomicXor(&bits[v >> 5], 1u << (v & 31u));
            atomicXor(&bits[p >> 5], 1u << (p & 31u));
        }
    }
    TL_SYNC();
    if (tid >= 64) return;
    uint32_t nf = 0;  // ballot compaction in position order by one wave, as at the end of the band walk
    for (uint32_t b0 = 0; b0 < n; b0 += 64) {
        const uint32_t c = b0 + tid;
        const bool odd = c < n && ((bits[c >> 5] >> (c & 31u)) & 1u);
        if (c < n) end_g[c] = odd ? (uint16_t)c : kChrNone;
        const uint64_t m = __builtin_amdgcn_ballot_w64(odd);
        if (odd) free[nf + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)c;
        nf += (uint32_t)__builtin_popcountll(m);
    }
    if (tid < 8) state[tid] = tid == 4 ? nf : 0u;
}

}  // namespace

ChrWs chr_ws_layout(const GreedyWs &w, uint32_t n)
{
    ChrWs c;
    c.key = (float *)w.succ[0];       // 8n bytes each: 4n used
    c.par = (uint16_t *)w.succ[1];    // 2n used
    c.parent = (uint16_t *)w.dte[0];  // 2n used
    c.order = (uint16_t *)w.dte[1];   // 2n used
    c.status = w.state + 8;           // the state block is 64 words; the bands use the first 8
    (void)n;
    return c;
}

hipError_t launch_chr_prim(const ChrWs &cw, const float2 *xy, const float *dm, uint32_t n, int lds_bytes, hipStream_t s)
{
    const size_t need = ((size_t)n * 6 + 15) & ~(size_t)15;
    const bool lds = need + 1024 <= (size_t)lds_bytes;
    const void *k = dm ? (lds ? (const void *)k_chr_prim<true, true> : (const void *)k_chr_prim<true, false>)
                       : (lds ? (const void *)k_chr_prim<false, true> : (const void *)k_chr_prim<false, false>);
    hipError_t e = allow_max_lds(k);
    if (e != hipSuccess) return e;
    const dim3 g(1), b(kPrimThreads);
    const size_t dyn = lds ? need : 0;
    if (dm) {
        if (lds) hipLaunchKernelGGL((k_chr_prim<true, true>), g, b, dyn, s, xy, dm, n, cw.key, cw.par, cw.parent, cw.order, cw.status);
        else hipLaunchKernelGGL((k_chr_prim<true, false>), g, b, dyn, s, xy, dm, n, cw.key, cw.par, cw.parent, cw.order, cw.status);
    } else {
        if (lds) hipLaunchKernelGGL((k_chr_prim<false, true>), g, b, dyn, s, xy, dm, n, cw.key, cw.par, cw.parent, cw.order, cw.status);
        else hipLaunchKernelGGL((k_chr_prim<false, false>), g, b, dyn, s, xy, dm, n, cw.key, cw.par, cw.parent, cw.order, cw.status);
    }
    return hipGetLastError();
}

hipError_t launch_chr_odd(const GreedyWs &w, const ChrWs &cw, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_chr_odd, dim3(1), dim3(1024), 0, s, cw.parent, n, w.end, w.free, w.state);
    return hipGetLastError();
}

}  // namespace tl
