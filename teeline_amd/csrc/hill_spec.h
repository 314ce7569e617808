// hill_spec.h — the part of the stochastic hill climb that is this project's specification rather than the reference's (DESIGN.md
// §4.25): the random stream.  One text for the device (hill_climb.hip), the host (tl_api_hill.hip: tl_hill_draw) and the stand-alone
// CPU restatement (tests/probes/hill_cpu_baseline.cpp); tests/_hill_oracle.py states the same in numpy.
//
// The stream is sa_spec.h's, indexed by a 64-bit event as in tabu_spec.h and ga_spec.h:
//   u(seed, chain, event, slot) = mix(chain_key(seed, chain) + G (32 event + slot + 1))          (arithmetic mod 2^64)
// The pair of epoch e is sa_pair(chain_key, e, n): event e (below 2^32), slots 0 .. 21, simulated annealing's draws unchanged.
// The restart that follows epoch e (e: the epoch index before the increment) is ga_spec.h's Fisher-Yates pass on the current
// contents: step j = n - 1 .. 1 does swap(a[j], a[position(u, j + 1)]) with u on slot 26 of the event 2^58 + e n + j
// (e n + j < 2^46: n is bounded by the LDS).  No draw depends on an earlier one — which is what lets a window of epochs be
// evaluated at once.
#pragma once
#include "ga_spec.h"

namespace tl {

__host__ __device__ inline uint64_t hill_shuffle_event(uint32_t epoch, uint32_t n, uint32_t j) { return kGaInitEvent + (uint64_t)epoch * n + j; }
__host__ __device__ inline uint64_t hill_draw_key(uint64_t key, uint64_t event, uint32_t slot) { return sa_mix(key + kSaG * (32ull * event + slot + 1u)); }

// the restart's shuffle of a[0 .. n), in place (Route::shuffle's role; the draws are this project's)
template <typename T>
__host__ __device__ inline void hill_shuffle(uint64_t key, uint32_t epoch, uint32_t n, T *a)
{
    for (uint32_t j = n - 1u; j >= 1u; --j) {
        const uint32_t p = sa_position(hill_draw_key(key, hill_shuffle_event(epoch, n, j), kGaSlotShuffle), j + 1u);
        const T x = a[j];
        a[j] = a[p];
        a[p] = x;
    }
}

}  // namespace tl
