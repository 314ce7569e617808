// ga_spec.h — the part of the genetic algorithm that is this project's specification rather than the reference's:
// the random stream.  One text for the device (genetic.hip), the host (tl_api_ga.hip: tl_ga_draw) and the stand-alone CPU
// restatement (tests/probes/ga_cpu_baseline.cpp); tests/_ga_oracle.py states the same in numpy.
//
// The stream is sa_spec.h's, indexed by a 64-bit event as in tabu_spec.h:
//   u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1))              (arithmetic mod 2^64)
// Breeding.  Pair p of generation g (the p-th of the reference's `for _ in n_elite..P/2`, counted from 0) owns the events
// 4 (g n + p) + part:
//   part 0   slots 0 .. 21: the crossover's random_position_pair (attempt t on slots 2t, 2t + 1: sa_spec.h's rule);
//            slots 22, 23: the roulette draws of parent 1 and parent 2; slots 24, 25: the mutation trials of child 1 and child 2
//   part 1   slots 0 .. 21: the mutation pair of child 1
//   part 2   slots 0 .. 21: the mutation pair of child 2
// The start population.  Individual i owns the events 2^58 + i n + j, j = 0 .. n - 1 (generation events stay below 2^51):
//   j = 0        slot 27: the number of mutations of a seeded individual, 2 + position(u, 3)
//   j = 1 + m    slots 0 .. 21: the pair of its mutation m = 0 .. 3
//   j = i'       slot 26: step i' = n - 1 .. 1 of a shuffled individual's Fisher-Yates pass: swap(a[i'], a[position(u, i' + 1)])
// A uniform f32 is float(u >> 40) 2^-24; a roulette draw is that times the total, one f32 multiply; a trial succeeds when p > uniform.
// No draw depends on an earlier one — which is what lets all the pairs of a generation be bred at once.
#pragma once
#include "sa_spec.h"

namespace tl {

constexpr uint64_t kGaInitEvent = 1ull << 58;
constexpr uint32_t kGaSlotSelect = 22;   // + 0 / 1: parent 1 / parent 2
constexpr uint32_t kGaSlotMutate = 24;   // + 0 / 1: child 1 / child 2
constexpr uint32_t kGaSlotShuffle = 26;
constexpr uint32_t kGaSlotCount = 27;

__host__ __device__ inline uint64_t ga_pair_event(uint32_t generation, uint32_t n, uint32_t pair, uint32_t part)
{
    return 4ull * ((uint64_t)generation * n + pair) + part;
}
__host__ __device__ inline uint64_t ga_init_event(uint32_t n, uint32_t individual, uint32_t j) { return kGaInitEvent + (uint64_t)individual * n + j; }
__host__ __device__ inline uint64_t ga_draw_key(uint64_t key, uint64_t event, uint32_t slot) { return sa_mix(key + kSaG * (32ull * event + slot + 1u)); }
__host__ __device__ inline float ga_uniform(uint64_t u) { return (float)(uint32_t)(u >> 40) * 5.9604644775390625e-08f; }

// random_position_pair (route.rs:69-83) on the event's slots 0 .. 21
__host__ __device__ inline void ga_pair(uint64_t key, uint64_t event, uint32_t n, uint32_t *from, uint32_t *to)
{
    uint32_t lo = 0, hi = 0;
    for (uint32_t t = 0; t < 11u; ++t) {
        const uint32_t p1 = sa_position(ga_draw_key(key, event, 2u * t), n), p2 = sa_position(ga_draw_key(key, event, 2u * t + 1u), n);
        lo = p1 < p2 ? p1 : p2;
        hi = p1 < p2 ? p2 : p1;
        if (hi - lo > 1u) break;
    }
    *from = lo;
    *to = hi;
}

// random_selection (genetic_algorithm.rs:273-290) over prefix[0 .. len], prefix[0] = 0, prefix[i + 1] = prefix[i] + fitness_i in
// f32: the first i with r < prefix[i + 1], else the last individual.  The prefix never decreases (fitness >= 0), so the
// reference's linear walk is this search.  len >= 1.
__host__ __device__ inline uint32_t ga_select(const float *prefix, uint32_t len, float r)
{
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (r < prefix[mid + 1u]) hi = mid;
        else lo = mid + 1u;
    }
    return lo < len ? lo : len - 1u;
}

// the population's length after a generation (solve_ga:65-107): the elites that exist, then two children per pair
__host__ __device__ inline uint32_t ga_pairs(uint32_t n, uint32_t n_elite) { return n / 2u > n_elite ? n / 2u - n_elite : 0u; }
__host__ __device__ inline uint32_t ga_next_len(uint32_t n, uint32_t n_elite, uint32_t len)
{
    return (n_elite < len ? n_elite : len) + 2u * ga_pairs(n, n_elite);
}

}  // namespace tl
