// sa_spec.h — the parts of simulated annealing that are this project's specification rather than the reference's:
// the random stream and the evaluation of the Metropolis criterion.  One text for the device (sim_anneal.hip) and the host
// (tl_api_sa.hip: tl_sa_draw); tests/_sa_oracle.py states the same in numpy.
//
// Draws.  mix = splitmix64's output function, G = 0x9E3779B97F4A7C15, arithmetic mod 2^64:
//   u(seed, chain, epoch, slot) = mix(mix(seed + G (chain + 1)) + G (32 epoch + slot + 1))
// A draw never depends on an earlier one — which is what lets a window of epochs be evaluated at once.  Pair attempt a = 0 .. 10
// uses slots 2a and 2a + 1 (random_position_pair, route.rs:69-83: the first attempt with hi - lo > 1, and after 10 redraws the
// last pair whatever it is), a position is ((u >> 32) n) >> 32, and p uses slot 22: float(u >> 40) 2^-24.
//
// Criterion.  exp(x) for the f32 x = (-(new - old)) / T: 0 below -87, otherwise in f64 without FMA: k = rint(x log2 e),
// r = (x - k ln2_hi) - k ln2_lo, q = the Horner sum of r^i / i! up to i = 13, (float) ldexp(q, k).  No library exp: the
// same operations on the device, on the host and in the oracle.
#pragma once
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#else  // a plain host compiler (the stand-alone CPU restatements under tests/probes): the same text without the qualifiers
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace tl {

constexpr uint64_t kSaG = 0x9E3779B97F4A7C15ULL;
constexpr uint32_t kSaSlotP = 22;  // the slot of p; slots 0 .. 21 are the eleven pair attempts

__host__ __device__ inline uint64_t sa_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t sa_chain_key(uint64_t seed, uint64_t chain) { return sa_mix(seed + kSaG * (chain + 1u)); }
__host__ __device__ inline uint64_t sa_draw_key(uint64_t key, uint32_t epoch, uint32_t slot)
{
    return sa_mix(key + kSaG * (32ull * epoch + slot + 1u));
}
__host__ __device__ inline uint32_t sa_position(uint64_t u, uint32_t n) { return (uint32_t)(((u >> 32) * n) >> 32); }

__host__ __device__ inline void sa_pair(uint64_t key, uint32_t epoch, uint32_t n, uint32_t *from, uint32_t *to)
{
    uint32_t lo = 0, hi = 0;
    for (uint32_t a = 0; a < 11u; ++a) {
        const uint32_t p1 = sa_position(sa_draw_key(key, epoch, 2u * a), n), p2 = sa_position(sa_draw_key(key, epoch, 2u * a + 1u), n);
        lo = p1 < p2 ? p1 : p2;
        hi = p1 < p2 ? p2 : p1;
        if (hi - lo > 1u) break;
    }
    *from = lo;
    *to = hi;
}

__host__ __device__ inline float sa_p(uint64_t key, uint32_t epoch) { return (float)(uint32_t)(sa_draw_key(key, epoch, kSaSlotP) >> 40) * 5.9604644775390625e-08f; }

// (outside the range an annealing chain reaches: a NaN x gives NaN, x > 89 gives +inf)
__host__ __device__ inline float sa_criteria(float x)
{
    if (x != x) return x;
    if (x < -87.0f) return 0.0f;
    if (x > 89.0f) return __builtin_inff();
    constexpr double c[14] = {1.0,
                              1.0,
                              1.0 / 2.0,
                              1.0 / 6.0,
                              1.0 / 24.0,
                              1.0 / 120.0,
                              1.0 / 720.0,
                              1.0 / 5040.0,
                              1.0 / 40320.0,
                              1.0 / 362880.0,
                              1.0 / 3628800.0,
                              1.0 / 39916800.0,
                              1.0 / 479001600.0,
                              1.0 / 6227020800.0};
    const double xd = (double)x;
    const double k = rint(xd * 1.4426950408889634);
    const double r = (xd - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double q = c[13];
#pragma unroll
    for (int i = 12; i >= 0; --i) q = q * r + c[i];
    return (float)ldexp(q, (int)k);
}

}  // namespace tl
