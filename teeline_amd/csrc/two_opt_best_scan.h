// two_opt_best_scan.h — how TL_MODE_BEST_SWEEP decides one row, for both forms of the descent: the chip-wide one (two_opt_best.hip:
// tour, tile metadata and row keys in HBM, one wave per row and launch) and the population's (two_opt_best_lds.hip: all of it in
// the workgroup's LDS, rows strided over its waves).  The callers hand in where P, the tile metadata and the row keys live; the
// body is the same instructions on either memory.
#pragma once
#include "two_opt_common.h"

#pragma clang fp contract(off)

namespace tl {

constexpr unsigned long long kNoKey64 = ~0ULL;

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off);
        v = o < v ? o : v;
    }
    return __shfl(v, 0);
}

// A row's best candidate among the columns [jlo, jhi] (clipped to the row's own [i+2, n-2]) as a packed key, or kNoKey64.
__device__ __forceinline__ unsigned long long bs_row_best(const float2 *__restrict__ P, const float4 *tbox, const float *tmsq, uint32_t n, uint32_t i, uint32_t jlo,
                                                          uint32_t jhi, int lane)
{
    unsigned long long best = kNoKey64;
    const float2 a = P[i], b = P[i + 1u];
    const float sqab = sqdist(a, b);
    const float dab_a = __builtin_amdgcn_sqrtf(sqab);
    const uint32_t jmin = i + 2u > jlo ? i + 2u : jlo, jmax = n - 2u < jhi ? n - 2u : jhi;
    if (jmin > jmax) return best;
    const uint32_t tmin = jmin >> 6, tmax = jmax >> 6;
    for (uint32_t g = tmin >> 6; g <= (tmax >> 6); ++g) {
        const uint32_t tl = (g << 6) + (uint32_t)lane;
        const float4 box = tbox[tl];
        const float msq = tmsq[tl];
        const bool live = (tl >= tmin) && (tl <= tmax) && ((box_lb(a.x, a.y, box) < sqab) || (box_lb(b.x, b.y, box) < msq));  // L0
        uint64_t m = __builtin_amdgcn_ballot_w64(live);
        while (m) {
            const uint32_t t = (g << 6) + (uint32_t)(__builtin_ffsll((long long)m) - 1);
            m &= m - 1;
            const uint32_t j = (t << 6) + (uint32_t)lane;
            const float2 c = P[j], e = P[j + 1u];
            const float sqce = sqdist(c, e), s1 = sqdist(a, c), s2 = sqdist(b, e);
            bool test = (j >= jmin) & (j <= jmax) & ((s1 < sqab) | (s2 < sqce));  // L1
            if (!__builtin_amdgcn_ballot_w64(test)) continue;
            // L2: discard what the hardware sqrt already shows to be non-improving by a safe margin
            const float neu_a = __builtin_amdgcn_sqrtf(s1) + __builtin_amdgcn_sqrtf(s2);
            const float cur_a = dab_a + __builtin_amdgcn_sqrtf(sqce);
            test = test & !(neu_a > cur_a + cur_a * 1.9073486e-6f);
            if (!__builtin_amdgcn_ballot_w64(test)) continue;
            const float neu = sqrt_rn(s1) + sqrt_rn(s2);
            const float cur = sqrt_rn(sqab) + sqrt_rn(sqce);
            if (test & (neu < cur)) {
                const float delta = neu - cur;
                const unsigned long long key = ((unsigned long long)(~__builtin_bit_cast(uint32_t, delta)) << 32) | (i << 16) | j;
                best = key < best ? key : best;
            }
        }
    }
    return wave_min_u64(best);
}

// Row i's best key in a sweep, through the row cache (Round 5): a row's best candidate is CACHED (rowkey) and a sweep decides only what
// the previous move can have changed.  mv: a move has been applied, and it reversed positions [is+1 .. js]: a row r > js reads none of
// them — its cached key stands; a row is <= r <= js has a new a or b — decided afresh; a row r < is keeps its a and b, and of its
// columns only j in [is .. js] have a new c = p[j] or e = p[j+1]: its new best is the smaller of the cached key and the best over
// those columns — unless the cached key's own column lies in that range (then afresh).
// Same keys, hence the same argmin with the same tie rule (lowest delta, then lowest (i, j)), as deciding every row afresh.
// One wave per call; lane 0 keeps the cache.
__device__ __forceinline__ unsigned long long bs_row_decide(const float2 *__restrict__ P, const float4 *tbox, const float *tmsq, unsigned long long *rowkey, uint32_t n,
                                                            uint32_t i, uint32_t mv, uint32_t is, uint32_t js, int lane)
{
    unsigned long long best;
    if (mv == 0u || (i >= is && i <= js)) {
        best = bs_row_best(P, tbox, tmsq, n, i, 0u, n, lane);
        if (lane == 0) rowkey[i] = best;
    } else if (i > js) {
        best = rowkey[i];
    } else {
        const unsigned long long ck = rowkey[i];
        const uint32_t cj = (uint32_t)(ck & 0xFFFFu);
        if (ck != kNoKey64 && cj >= is && cj <= js) {
            best = bs_row_best(P, tbox, tmsq, n, i, 0u, n, lane);
        } else {
            const unsigned long long pk = bs_row_best(P, tbox, tmsq, n, i, is, js, lane);
            best = pk < ck ? pk : ck;
        }
        if (best != ck && lane == 0) rowkey[i] = best;
    }
    return best;
}

}  // namespace tl
