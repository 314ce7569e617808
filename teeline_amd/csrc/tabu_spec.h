// tabu_spec.h — the part of tabu search that is this project's specification rather than the reference's: the
// random stream.  One text for the device (tabu_search.hip), the host (tl_api_tabu.hip: tl_tabu_draw) and the stand-alone CPU
// restatement (tests/probes/tabu_cpu_baseline.cpp); tests/_tabu_oracle.py states the same in numpy.
//
// The stream is sa_spec.h's, indexed by a 64-bit event instead of an epoch.  Candidate a = 0 .. n of epoch e is event
// e (n + 1) + a, and
//   u(seed, chain, event, slot) = mix(chain_key(seed, chain) + G (32 event + slot + 1))        (arithmetic mod 2^64)
// Pair attempt t = 0 .. 10 uses slots 2t and 2t + 1 (random_position_pair, route.rs:69-83: the first attempt with hi - lo > 1, and
// after 10 redraws the last pair whatever it is); a position is ((u >> 32) n) >> 32.  No draw depends on an earlier one — which
// is what lets all the candidates of an epoch be evaluated at once.
#pragma once
#include "sa_spec.h"

namespace tl {

__host__ __device__ inline uint64_t tabu_event(uint32_t epoch, uint32_t n, uint32_t attempt) { return (uint64_t)epoch * ((uint64_t)n + 1u) + attempt; }
__host__ __device__ inline uint64_t tabu_draw_key(uint64_t key, uint64_t event, uint32_t slot) { return sa_mix(key + kSaG * (32ull * event + slot + 1u)); }

__host__ __device__ inline void tabu_pair(uint64_t key, uint64_t event, uint32_t n, uint32_t *from, uint32_t *to)
{
    uint32_t lo = 0, hi = 0;
    for (uint32_t t = 0; t < 11u; ++t) {
        const uint32_t p1 = sa_position(tabu_draw_key(key, event, 2u * t), n), p2 = sa_position(tabu_draw_key(key, event, 2u * t + 1u), n);
        lo = p1 < p2 ? p1 : p2;
        hi = p1 < p2 ? p2 : p1;
        if (hi - lo > 1u) break;
    }
    *from = lo;
    *to = hi;
}

}  // namespace tl
