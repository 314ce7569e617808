// swap_seq.h — swap_sequence (route.rs:118-134) in its orbit form, by a whole workgroup: what particle_swarm.hip and
// flower_pollination.hip share.  With pi(p) = from^-1[target[p]] the sequence is, in ascending i, (i, q) for every i that is not
// the largest position of its pi-cycle, q the first of pi(i), pi^2(i), .. above i (DESIGN.md §4.20 has the argument) — one lane per
// position walking its orbit, then a ballot/popcount compaction.  A pair is one word, i | q << 16 (pso_spec.h: pso_swap).
//
// L is the caller's view of its LDS: L.inv[n] u16, the inverse of `from` (whole before the call); L.pi[n] u16, scratch; L.wsum,
// 2 x 16 words for the wave counts of the compaction's two parities.
#pragma once
#include "tl_device.h"

namespace tl {

// swap_sequence(from, target) by the whole workgroup, L.inv being the inverse of `from`: the pairs go to
// out[0 .. len) in ascending i, len (= n - cycles of pi) is returned to every lane.  Begins and ends behind a barrier.
template <class Lds>
__device__ uint32_t swap_sequence_orbit(const uint16_t *target, uint32_t n, const Lds &L, uint32_t *out)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, nw = nt >> 6;
    for (uint32_t k = tid; k < n; k += nt) L.pi[k] = L.inv[target[k]];
    TL_SYNC();
    uint32_t base = 0, par = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += nt) {
        const uint32_t i = t0 + tid;
        bool has = false;
        uint32_t q = 0;
        if (i < n) {
            uint32_t p = L.pi[i];
            for (uint32_t steps = 0; p < i && steps < n; ++steps) p = L.pi[p];  // (a permutation comes back to i within its cycle: the bound is never met)
            has = p > i;
            q = p;
        }
        const uint64_t b = __ballot(has), below = (1ull << lane) - 1ull;
        uint32_t *ws = L.wsum + par * 16u;
        if (lane == 0u) ws[wave] = (uint32_t)__popcll(b);
        TL_SYNC();
        uint32_t off = base, tot = 0;
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t a = ws[w];
            if (w < wave) off += a;
            tot += a;
        }
        if (has) out[off + (uint32_t)__popcll(b & below)] = i | (q << 16);
        base += tot;
        par ^= 1u;
    }
    TL_SYNC();
    return base;
}

}  // namespace tl
