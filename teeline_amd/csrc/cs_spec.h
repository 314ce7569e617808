// cs_spec.h — the part of the cuckoo search solver that is this project's specification rather than the reference's (DESIGN.md
// §4.21): the random stream (the Lévy step itself is levy_spec.h).  One text for the device (cuckoo_search.hip), the host
// (tl_api_cs.hip: tl_cs_draw, tl_levy_from_words, tl_cs_flight_length, tl_cs_pa) and the stand-alone CPU restatement
// (tests/probes/cs_cpu_baseline.cpp); tests/_cs_oracle.py states the same in numpy and literal loops.
//
// The stream is ga_spec.h's:
//   u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1))              (arithmetic mod 2^64)
// Cuckoo c and nest c of epoch e (N nests, n cities) own the n + 1 events from B = (e N + c) (n + 1):
//   B           slots 0 .. 3: the Lévy step's words (u1, u2 of u; u1, u2 of v); slots 4 .. 11: v's resample pairs (levy_spec.h);
//               slot 12: the flight's target nest, position(u, N); slot 13: nest c's abandonment trial, (u >> 11) 2^-53 < pa
//   B + 1 + r   slots 0, 1: reversal r = 0 .. n/2 - 1 of the flight: i = position(u, n - 1), j = i + 1 + position(u', n - 1 - i)
//   B + 1 + j   slot 2: step j = n - 1 .. 1 of the Fisher-Yates pass of nest c's replacement: swap(a[j], a[position(u, j + 1)])
// Start nest i owns the events 2^58 + i n + j, slot 26: step j = n - 1 .. 1 of its pass — ga_spec.h's init stream, unchanged.
// Epoch events stay below 2^58: calls with epochs N (n + 1) > 2^58 are refused.  No draw depends on an earlier one and no two
// uses share an (event, slot) — which is what lets every flight and every replacement of an epoch be built at once.
#pragma once
#include "ga_spec.h"
#include "levy_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kCsSlotLevy = 0;      // .. 3, the resample pairs on 4 .. 4 + 2 kLevyResamples - 1
constexpr uint32_t kCsSlotTarget = 12, kCsSlotAbandon = 13;
constexpr uint32_t kCsSlotRevI = 0, kCsSlotRevJ = 1, kCsSlotReplace = 2;
constexpr uint32_t kCsDefaultNests = 25;  // cuckoo_search.rs:10
constexpr uint32_t kCsMaxNests = 4096;    // the cuckoo is the grid's x
constexpr uint64_t kCsEventLimit = 1ull << 58;
static_assert(4 + 2 * kLevyResamples <= kCsSlotTarget, "the Lévy words end below the target's slot");

__host__ __device__ inline uint32_t cs_nests(uint32_t n_nearest) { return n_nearest > kCsDefaultNests ? n_nearest : kCsDefaultNests; }
__host__ __device__ inline uint64_t cs_base(uint32_t epoch, uint32_t nests, uint32_t c, uint32_t n) { return ((uint64_t)epoch * nests + c) * ((uint64_t)n + 1u); }
__host__ __device__ inline bool cs_events_fit(uint32_t epochs, uint32_t nests, uint32_t n) { return (uint64_t)epochs * nests * ((uint64_t)n + 1u) <= kCsEventLimit; }

// pa = clamp(mutation_probability as f64, 0.01, 0.99) (cuckoo_search.rs:35)
__host__ __device__ inline double cs_pa(float mutation_probability)
{
    const double p = (double)mutation_probability;
    return p < 0.01 ? 0.01 : p > 0.99 ? 0.99 : p;
}

struct CsLevyWords {
    uint64_t key, base;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return ga_draw_key(key, base, kCsSlotLevy + i); }
};

// |levy_step| of the flight whose events begin at `base` (cuckoo_search.rs:79)
__host__ __device__ inline double cs_levy(uint64_t key, uint64_t base) { return fabs(levy_step(CsLevyWords{key, base}, nullptr)); }

// k = (ceil(levy (n 0.1)) as usize).clamp(1, n / 2) for n >= 2 (cuckoo_search.rs:85): Rust's `as` — NaN gives 0, a negative
// value 0, +inf or anything too large saturates — so NaN ends at 1 and +inf at n / 2
__host__ __device__ inline uint32_t cs_flight_length(double levy, uint32_t n)
{
    const double x = ceil(levy * ((double)n * 0.1));
    const uint32_t top = n / 2u;
    if (!(x > 1.0)) return 1u;
    if (x >= (double)top) return top;
    return (uint32_t)x;
}

// reversal r of a flight: [i ..= j], 0 <= i < j <= n - 1 (apply_k_random_2opt, cuckoo_search.rs:18-22)
__host__ __device__ inline void cs_reversal(uint64_t key, uint64_t base, uint32_t r, uint32_t n, uint32_t *i, uint32_t *j)
{
    const uint32_t a = sa_position(ga_draw_key(key, base + 1u + r, kCsSlotRevI), n - 1u);
    *i = a;
    *j = a + 1u + sa_position(ga_draw_key(key, base + 1u + r, kCsSlotRevJ), n - 1u - a);
}

__host__ __device__ inline uint32_t cs_target(uint64_t key, uint64_t base, uint32_t nests) { return sa_position(ga_draw_key(key, base, kCsSlotTarget), nests); }
__host__ __device__ inline bool cs_abandoned(uint64_t key, uint64_t base, double pa) { return levy_uniform(ga_draw_key(key, base, kCsSlotAbandon)) < pa; }
__host__ __device__ inline uint32_t cs_replace_position(uint64_t key, uint64_t base, uint32_t j) { return sa_position(ga_draw_key(key, base + 1u + j, kCsSlotReplace), j + 1u); }

// where position p of the tour AFTER the reversals pairs[0 .. k) (i | j << 16 each, applied in order) comes from in the tour before
// them: a reversal is its own inverse, so the position is followed back through them from the last to the first
__host__ __device__ inline uint32_t cs_source_position(const uint32_t *pairs, uint32_t k, uint32_t p)
{
    uint32_t q = p;
    for (uint32_t r = k; r-- > 0u;) {
        const uint32_t w = pairs[r], i = w & 0xFFFFu, j = w >> 16;
        q = (i <= q && q <= j) ? i + j - q : q;
    }
    return q;
}

}  // namespace tl
