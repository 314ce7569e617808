// fpa_spec.h — the part of the flower pollination solver that is this project's specification rather than the reference's
// (DESIGN.md §4.22): the random stream (the Lévy step itself is levy_spec.h, unchanged).  One text for the device
// (flower_pollination.hip), the host (tl_api_fpa.hip: tl_fpa_draw, tl_fpa_switch_prob, tl_fpa_global_swaps, tl_fpa_local_swaps,
// tl_fpa_partners) and the stand-alone CPU restatement (tests/probes/fpa_cpu_baseline.cpp); tests/_fpa_oracle.py states the same
// in numpy and literal loops.
//
// The stream is ga_spec.h's:
//   u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1))              (arithmetic mod 2^64)
// Flower i of epoch e (N flowers) owns the event e N + i:
//   slot 0        the switch trial: (u >> 11) 2^-53 < switch_prob is a global pollination
//   slots 1 .. 12 the Lévy step's words (u1, u2 of u; u1, u2 of v; v's four resample pairs: levy_spec.h) — a global move with a
//                 sequence that is not empty
//   slot 13       j of a local move: position(u, N - 1), stepped over i
//   slot 14       k of a local move: position(u, N - 2), stepped over i and j in ascending order
//   slot 15       epsilon of a local move with a sequence that is not empty: (u >> 11) 2^-53
// Start flower i owns the events 2^58 + i n + j, slot 26: step j = n - 1 .. 1 of its Fisher-Yates pass — ga_spec.h's init stream,
// unchanged.  Epoch events stay below 2^44 (epochs < 2^32, N <= 4096).  No draw depends on an earlier one and no two uses share
// an (event, slot); a draw the reference would not have made is simply not read.
//
// j and k.  The reference's sample_without_replacement is a rejection loop of unbounded length; stepping a draw over the excluded
// indices has the same distribution (uniform over the allowed ones) with no loop.
#pragma once
#include "ga_spec.h"
#include "levy_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kFpaSlotSwitch = 0, kFpaSlotLevy = 1;  // the Lévy words on 1 .. kLevyWords
constexpr uint32_t kFpaSlotJ = 13, kFpaSlotK = 14, kFpaSlotEpsilon = 15;
constexpr uint32_t kFpaDefaultFlowers = 25;  // flower_pollination.rs:10
constexpr uint32_t kFpaMaxFlowers = 4096;    // the flower is the grid's x; j and k take 12 bits each of an epoch row's word
static_assert(kFpaSlotLevy + kLevyWords <= kFpaSlotJ, "the Lévy words end below j's slot");

__host__ __device__ inline uint32_t fpa_flowers(uint32_t n_nearest) { return n_nearest > kFpaDefaultFlowers ? n_nearest : kFpaDefaultFlowers; }
__host__ __device__ inline uint64_t fpa_event(uint32_t epoch, uint32_t flowers, uint32_t i) { return (uint64_t)epoch * flowers + i; }

// switch_prob (flower_pollination.rs:65-69): the comparison is in f32, so the default 0.001 gives 0.8
__host__ __device__ inline double fpa_switch_prob(float mutation_probability) { return mutation_probability < 0.01f ? 0.8 : (double)mutation_probability; }

// bernoulli(switch_prob): u < p in f64
__host__ __device__ inline bool fpa_is_global(uint64_t key, uint64_t event, double switch_prob)
{
    return levy_uniform(ga_draw_key(key, event, kFpaSlotSwitch)) < switch_prob;
}

struct FpaLevyWords {
    uint64_t key, event;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return ga_draw_key(key, event, kFpaSlotLevy + i); }
};

// |levy_step| of a global move (flower_pollination.rs:17)
__host__ __device__ inline double fpa_levy(uint64_t key, uint64_t event) { return fabs(levy_step(FpaLevyWords{key, event}, nullptr)); }
__host__ __device__ inline double fpa_epsilon(uint64_t key, uint64_t event) { return levy_uniform(ga_draw_key(key, event, kFpaSlotEpsilon)); }

// `(x.ceil() as usize).clamp(1, len)` for len >= 1, Rust's `as`: NaN and anything <= 1 end at 1, +inf and anything >= len at len
__host__ __device__ inline uint32_t fpa_clamped_ceil(double x, uint32_t len)
{
    const double c = ceil(x);
    if (!(c > 1.0)) return 1u;
    if (c >= (double)len) return len;
    return (uint32_t)c;
}

// n_swaps of a global move (flower_pollination.rs:23): (levy len) 0.5, left to right; 0 for an empty sequence (nothing is applied)
__host__ __device__ inline uint32_t fpa_global_swaps(double levy, uint32_t len) { return len ? fpa_clamped_ceil(levy * (double)len * 0.5, len) : 0u; }
// n_swaps of a local move (flower_pollination.rs:49)
__host__ __device__ inline uint32_t fpa_local_swaps(double epsilon, uint32_t len) { return len ? fpa_clamped_ceil(epsilon * (double)len, len) : 0u; }

// j != i, then k outside {i, j}, of flower i's local move (flowers >= 3)
__host__ __device__ inline void fpa_partners(uint64_t key, uint64_t event, uint32_t i, uint32_t flowers, uint32_t *j, uint32_t *k)
{
    uint32_t a = sa_position(ga_draw_key(key, event, kFpaSlotJ), flowers - 1u);
    if (a >= i) ++a;
    uint32_t b = sa_position(ga_draw_key(key, event, kFpaSlotK), flowers - 2u);
    const uint32_t lo = a < i ? a : i, hi = a < i ? i : a;
    if (b >= lo) ++b;
    if (b >= hi) ++b;
    *j = a;
    *k = b;
}

// the words of an epoch row that describe flower i's move: the kind with j and k; the sequence and the prefix length
__host__ __device__ inline uint32_t fpa_kind_word(bool global, uint32_t j, uint32_t k) { return global ? 1u << 31 : j | (k << 12); }
__host__ __device__ inline uint32_t fpa_length_word(uint32_t len, uint32_t prefix) { return len | (prefix << 16); }

}  // namespace tl
