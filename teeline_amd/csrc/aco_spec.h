// aco_spec.h — the parts of the ant colony solver that are this project's specification rather than the reference's (DESIGN.md
// §4.19): the random stream and the power function.  One text for the device (ant_colony.hip), the host (tl_api_aco.hip: tl_aco_draw,
// tl_aco_pow) and the stand-alone CPU restatement (tests/probes/aco_cpu_baseline.cpp); tests/_aco_oracle.py states the same in numpy.
//
// Draws.  The stream is ga_spec.h's: u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1)).
// Ant a (of A) of epoch g at step s = 0 .. n - 1 owns the event (g A + a) n + s:
//   s = 0          slot 0: the start city, position(u, n)
//   s = 1 .. n-1   slot 1: r1, slot 2: r2 of the selection that fills position s of the tour, each float(u >> 40) 2^-24
// The start tour of a run without an initial tour is ga_spec.h's Fisher-Yates pass on the events 2^58 + j, j = n - 1 .. 1, slot
// kGaSlotShuffle: swap(a[j], a[position(u, j + 1)]).  Epoch events stay below 2^58: calls with epochs A n > 2^58 are refused.
// No draw depends on an earlier one.
//
// aco_pow(x, a) for x >= 0 or NaN and finite a >= 0 — the reference's f32 powf, whose result is the platform's; no library pow, exp or
// log here: a = 0 gives 1; NaN x gives x; x = 0 gives 0; x = +inf gives +inf; a = 1 gives x; a = 2 gives x x in f32; otherwise in
// f64 without FMA:
//   (m, e) = frexp(x), by the bits, renormalised so that m is in [sqrt 1/2, sqrt 2); s = (m - 1) / (m + 1);
//   log x = e ln2_hi + (2 s Horner(s^2; 1, 1/3, .., 1/23) + e ln2_lo); y = (double)a log x;
//   y > 89 gives +inf, y < -104 gives 0 (e^-104 < 2^-150, half the least f32), else sa_criteria's reduction and 13-term Horner on the
//   double y: k = rint(y log2 e), r = (y - k ln2_hi) - k ln2_lo, q = the sum of r^i / i!, (float) ldexp(q, k): one rounding to f32.
//
// Exactness of the masked walk (cf. ga_select).  The reference's select_next sums and walks the weights of the UNVISITED cities in city
// order.  Adding +0.0f to a sum that is +0 or positive leaves every bit of it (weights are >= +0 or NaN; a NaN or an infinity makes the
// total non-finite in either form), so a walk over all n cities in which a visited city's weight is forced to +0.0f produces the
// same total, the same running sums at the unvisited cities and no new `acc > target` verdict at a visited one: acc has not moved
// since the last unvisited city, where the verdict was already "no" (and before the first it is 0 > target, false for target >= 0).
// The walk therefore selects the same city as the reference's compacted walk.  Only the exhausted-walk fallback needs care: it is
// the last UNVISITED city (the compacted list's last element), not city n - 1; likewise "the first candidate" is the first unvisited.
#pragma once
#include "ga_spec.h"
#include "sa_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint64_t kAcoEventLimit = 1ull << 58;  // epochs A n may not exceed it (the shuffle's events begin there)
constexpr uint32_t kAcoSlotStart = 0, kAcoSlotR1 = 1, kAcoSlotR2 = 2;
constexpr float kAcoTauMinRatio = 1e-4f;  // ant_colony.rs:16
constexpr float kAcoMinDist = 1e-6f;      // ant_colony.rs:22

__host__ __device__ inline uint64_t aco_event(uint32_t epoch, uint32_t num_ants, uint32_t ant, uint32_t n, uint32_t step)
{
    return ((uint64_t)epoch * num_ants + ant) * n + step;
}
__host__ __device__ inline uint64_t aco_shuffle_event(uint32_t j) { return kGaInitEvent + j; }

__host__ __device__ inline float aco_pow(float x, float a)
{
    if (a == 0.0f) return 1.0f;
    if (x != x) return x;
    if (x == 0.0f) return 0.0f;
    if (x == __builtin_inff()) return x;
    if (a == 1.0f) return x;
    if (a == 2.0f) return x * x;
    constexpr double lc[12] = {1.0, 1.0 / 3.0, 1.0 / 5.0, 1.0 / 7.0, 1.0 / 9.0, 1.0 / 11.0, 1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0, 1.0 / 21.0, 1.0 / 23.0};
    constexpr double ec[14] = {1.0,
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
    // a positive f32, subnormals included, is a normal f64: frexp by the bits, m in [1/2, 1)
    const uint64_t b = __builtin_bit_cast(uint64_t, (double)x);
    double e = (double)((int)((b >> 52) & 0x7FFu) - 1022);
    double m = __builtin_bit_cast(double, (b & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull);
    if (m < 0.70710678118654752440) {
        m = m * 2.0;
        e = e - 1.0;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double p = lc[11];
#pragma unroll
    for (int i = 10; i >= 0; --i) p = p * s2 + lc[i];
    const double lx = e * 6.93147180369123816490e-01 + ((2.0 * s) * p + e * 1.90821492927058770002e-10);
    const double y = (double)a * lx;
    if (y > 89.0) return __builtin_inff();
    if (y < -104.0) return 0.0f;
    const double k = rint(y * 1.4426950408889634);
    const double r = (y - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double q = ec[13];
#pragma unroll
    for (int i = 12; i >= 0; --i) q = q * r + ec[i];
    return (float)ldexp(q, (int)k);
}

// eta_beta of an edge of length d (ant_colony.rs:169-170)
__host__ __device__ inline float aco_eta(float d, float beta) { return aco_pow(1.0f / (d > kAcoMinDist ? d : kAcoMinDist), beta); }

// select_next's verdict on a sum (ant_colony.rs:67,71)
__host__ __device__ inline bool aco_sum_usable(float sum) { return sum > 0.0f && sum <= 3.4028234663852886e38f; }

}  // namespace tl
