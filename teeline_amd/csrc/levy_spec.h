// levy_spec.h — Mantegna's Lévy step (probability.rs:8-22: normal_sample, levy_step) as this project's specification: a fixed
// sequence of IEEE f64 operations, the same on the device, on the host and in the oracle (tests/_cs_oracle.py states it in numpy).
// cs_spec.h includes it; a later flower pollination solver can.  f64 throughout, contraction off, NO library log, cos or pow:
//
//   uniform(w)    = (w >> 11) 2^-53, a dyadic f64 in [0, 1)
//   normal(w1,w2) = sqrt(-2 log(max(uniform(w1), MIN_POSITIVE))) cos2pi(uniform(w2))                          (Box-Muller)
//   log(x)        for a positive normal x: (m, e) = frexp by the bits, renormalised so that m is in [sqrt 1/2, sqrt 2);
//                 s = (m - 1) / (m + 1); e ln2_hi + (2 s Horner(s^2; 1, 1/3, .., 1/23) + e ln2_lo)         (aco_spec.h's sequence)
//   cos2pi(u)     for a dyadic u in [0, 1), with an EXACT reduction: t = 4 u, q = floor(t), f = t - q (all exact); with
//                 g = f <= 1/2 ? f : 1 - f (exact) and x = g (pi/2) (one rounding), S = x Horner(x^2; 1, -1/3!, .., -1/19!) and
//                 C = Horner(x^2; 1, -1/2!, .., +1/20!): cos(pi/2 f) = f <= 1/2 ? C : S, sin(pi/2 f) = f <= 1/2 ? S : C, and
//                 q = 0: cos, q = 1: -sin, q = 2: -cos, q = 3: sin.  u = 1/4 and u = 3/4 give exactly -0 and +0.
//   exp(y)        sa_spec.h's reduction kept in f64: k = rint(y log2 e), r = (y - k ln2_hi) - k ln2_lo, ldexp(Horner(r; 1/i!, i <= 13), k)
//   levy(words)   u = normal(w0, w1) 0.6966; v = normal(w2, w3); while |v| < MIN_POSITIVE and fewer than kLevyResamples resamples
//                 have been made: v = normal of the next word pair (w4, w5), (w6, w7), ..; a v still below MIN_POSITIVE after the
//                 last resample is taken as 1.0; levy = u / exp((1 / 1.5) log |v|).
// sqrt and / are the IEEE operations (correctly rounded on the host and on the device: tl_cs_selftest_levy compares the two).
//
// Accuracy, measured on the CPU against numpy's libm evaluation of the reference formula (tests/test_cs_oracle.py, 2^20 seeded
// draws plus the edge words): the largest relative difference is kLevyMeasuredRelDiff below — it is reached where cos(2 pi u2) is
// near a zero, where libm's rounded argument 2 pi u2 moves ITS result, not this one's; elsewhere the two agree to a few ulps.
#pragma once
#include "sa_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kLevyResamples = 4;                      // resample attempts of v after the first pair
constexpr uint32_t kLevyWords = 4 + 2 * kLevyResamples;     // words a Lévy step may read
constexpr double kLevyMinPositive = 2.2250738585072014e-308;  // f64::MIN_POSITIVE
constexpr double kLevySigmaU = 0.6966;                      // probability.rs:5
constexpr double kLevyMeasuredRelDiff = 7.6e-10;            // see above; the test's bound is twice its own measurement

__host__ __device__ inline double levy_uniform(uint64_t w) { return (double)(w >> 11) * 1.1102230246251565e-16; }  // 2^-53: both factors exact

// log of a positive NORMAL f64
__host__ __device__ inline double levy_log(double x)
{
    constexpr double lc[12] = {1.0, 1.0 / 3.0, 1.0 / 5.0, 1.0 / 7.0, 1.0 / 9.0, 1.0 / 11.0, 1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0, 1.0 / 21.0, 1.0 / 23.0};
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
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
    return e * 6.93147180369123816490e-01 + ((2.0 * s) * p + e * 1.90821492927058770002e-10);
}

// exp of a finite y with |y| < 700, in f64
__host__ __device__ inline double levy_exp(double y)
{
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
    const double k = rint(y * 1.4426950408889634);
    const double r = (y - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double q = ec[13];
#pragma unroll
    for (int i = 12; i >= 0; --i) q = q * r + ec[i];
    return ldexp(q, (int)k);
}

// cos(2 pi u) for a dyadic u in [0, 1)
__host__ __device__ inline double levy_cos2pi(double u)
{
    constexpr double sc[10] = {1.0,
                               -1.0 / 6.0,
                               1.0 / 120.0,
                               -1.0 / 5040.0,
                               1.0 / 362880.0,
                               -1.0 / 39916800.0,
                               1.0 / 6227020800.0,
                               -1.0 / 1307674368000.0,
                               1.0 / 355687428096000.0,
                               -1.0 / 121645100408832000.0};
    constexpr double cc[11] = {1.0,
                               -1.0 / 2.0,
                               1.0 / 24.0,
                               -1.0 / 720.0,
                               1.0 / 40320.0,
                               -1.0 / 3628800.0,
                               1.0 / 479001600.0,
                               -1.0 / 87178291200.0,
                               1.0 / 20922789888000.0,
                               -1.0 / 6402373705728000.0,
                               1.0 / 2432902008176640000.0};
    const double t = u * 4.0;
    const double qf = floor(t);
    const double f = t - qf;
    const bool low = f <= 0.5;
    const double g = low ? f : 1.0 - f;
    const double x = g * 1.5707963267948966;
    const double x2 = x * x;
    double ps = sc[9];
#pragma unroll
    for (int i = 8; i >= 0; --i) ps = ps * x2 + sc[i];
    double pc = cc[10];
#pragma unroll
    for (int i = 9; i >= 0; --i) pc = pc * x2 + cc[i];
    const double S = x * ps, Cc = pc;
    const double c = low ? Cc : S, s = low ? S : Cc;
    const int q = (int)qf;
    return q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// normal_sample (probability.rs:8-12)
__host__ __device__ inline double levy_normal(uint64_t w1, uint64_t w2)
{
    double u1 = levy_uniform(w1);
    if (u1 < kLevyMinPositive) u1 = kLevyMinPositive;
    return sqrt(-2.0 * levy_log(u1)) * levy_cos2pi(levy_uniform(w2));
}

// levy_step (probability.rs:15-22) on the words word(0) .. word(kLevyWords - 1); *resamples (optional): how many further pairs v took
template <class W>
__host__ __device__ inline double levy_step(W word, uint32_t *resamples)
{
    const double u = levy_normal(word(0u), word(1u)) * kLevySigmaU;
    double v = levy_normal(word(2u), word(3u));
    uint32_t t = 0;
    while (fabs(v) < kLevyMinPositive && t < kLevyResamples) {
        v = levy_normal(word(4u + 2u * t), word(5u + 2u * t));
        ++t;
    }
    if (fabs(v) < kLevyMinPositive) v = 1.0;
    if (resamples) *resamples = t;
    return u / levy_exp((1.0 / 1.5) * levy_log(fabs(v)));
}

}  // namespace tl
