// som_spec.h — the part of the Kohonen self-organising map solver that is this project's specification rather than the reference's
// (DESIGN.md §4.24): the city draw, the fixed exp with its cut, the start ring, and the spelled-out f64 sequence of everything the
// training reads or writes.  One text for the device (kohonen_som.hip), the host (tl_api_som.hip: tl_som_draw, tl_som_schedule,
// tl_som_h, tl_som_ring_init) and the stand-alone CPU restatement (tests/probes/som_cpu_baseline.cpp); tests/_som_oracle.py states the
// same in numpy and literal loops.  All f64, contraction off, NO library exp, cos or sin.
//
// The draw.  The stream is ga_spec.h's: u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1)).  Epoch
// t = 1 .. epochs of run r owns the event t, slot 0: its city is position(u, n) = ((u >> 32) n) >> 32 (sa_spec.h: a bounded draw, no
// rejection loop).  No draw depends on another.
//
// The schedule (som.rs:79-82).  decay = levy_exp(-((double)t) / (double)epochs) — the argument lies in [-1, 0) —,
// eta = eta0 decay, sigma = max(sigma0 decay, 1.0) with sigma0 = radius_fraction (double)M, two_sigma_sq = (2.0 sigma) sigma.
//
// The neighbourhood (som.rs:104-113).  For the ring distance d = min(|i - bmu|, M - |i - bmu|) as an f64: y = ((-d) d) / two_sigma_sq.
// A neuron with y < -8.0 is skipped WITHOUT an exp: exp(-8) = 3.4e-4 is far below the reference's cut of 1e-3, so no neuron the
// reference would move is lost to it, and levy_exp's stated domain ends at |y| < 700 where a ring can reach y = -1e7.  Otherwise
// h = levy_exp(y), skipped when h < 1e-3; else neuron += (eta h) (city - neuron) per axis, left to right as som.rs writes it.
//
// The radius of an epoch.  radius = min(M, floor(sqrt(8.0 two_sigma_sq)) + 2) (sqrt the IEEE operation).  It is CONSERVATIVE: a
// neuron with d > radius has d >= sqrt(8 tss) + 1 (floor loses less than 1, the correctly rounded sqrt less than 1 again), so
// d^2 >= 8 tss + 2 sqrt(8 tss) + 1 and the exact quotient d^2 / tss exceeds 8 by the relative amount 1 / sqrt(2 tss) or more.  With
// M <= 2^16, tss <= 2^33 and that is above 2^-17 — thousands of billions of ulps; d d is exact (d < 2^26) and one correctly rounded
// division cannot bring the quotient back to 8.  So y < -8.0 holds for every neuron outside the radius: a device that applies the two
// tests only inside it skips exactly the neurons the full loop skips.
//
// The start ring (som.rs:54-59).  u = (double)i / (double)M, neuron i = (cx + 0.1 cos 2 pi u, cy + 0.1 sin 2 pi u), both from
// som_cossin2pi: levy_cos2pi's reduction and its two polynomials (levy_spec.h; the coefficient tables are repeated here so that
// levy_spec.h stays as it is), with the sine read off the same quadrant.  The reduction is exact for ANY f64 u in [0, 1), not only
// the dyadic ones levy_spec.h feeds it: t = 4 u is a scaling by a power of two; q = floor(t) <= 3 is an integer; f = t - q is a
// multiple of ulp(t) that is no larger than t, so it has a 53-bit significand at t's exponent or below — representable; and for
// f in (1/2, 1), 1 - f is exact by Sterbenz's lemma (1/2 <= f <= 2).  The one rounding is x = g (pi / 2), as before.  i / M < 1 for
// i < M <= 2^16: the correctly rounded quotient of (M - 1) / M = 1 - 2^-16 or less is below 1.
#pragma once
#include "ga_spec.h"
#include "levy_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kSomSlotCity = 0;
constexpr uint32_t kSomMaxNeurons = 65536;  // the cap on M = n neuron_multiplier: d d and i / M stay exact, counting ranks stays cheap
constexpr double kSomCutY = -8.0;           // below: skipped without an exp
constexpr double kSomCutH = 1e-3;           // som.rs:109
constexpr double kSomRingRadius = 0.1;      // som.rs:57
constexpr double kSomSigmaFloor = 1.0;      // som.rs:61
constexpr double kSomMinSpan = 1e-9;        // som.rs:35-36
// levy_exp on the arguments this solver feeds it (the schedule's [-1, 0), the neighbourhood's [-8, 0]) against numpy's libm exp,
// measured on the CPU (tests/test_som_oracle.py, 3e5 arguments): the largest relative difference; the test's bound is twice this
constexpr double kSomExpMeasuredRelDiff = 2.3e-16;

__host__ __device__ inline uint32_t som_city(uint64_t key, uint32_t t, uint32_t n) { return sa_position(ga_draw_key(key, (uint64_t)t, kSomSlotCity), n); }

struct SomEpoch {
    double eta, two_sigma_sq;
    uint32_t radius, pad;
};

// the schedule of epoch t = 1 .. epochs (som.rs:79-82); *sigma_out optional
__host__ __device__ inline SomEpoch som_schedule(uint32_t t, uint32_t epochs, uint32_t M, double eta0, double radius_fraction, double *sigma_out)
{
    const double decay = levy_exp((-(double)t) / (double)epochs);
    const double sigma0 = radius_fraction * (double)M;
    double sigma = sigma0 * decay;
    if (!(sigma > kSomSigmaFloor)) sigma = kSomSigmaFloor;  // f64::max(sigma, 1.0); sigma is never NaN
    SomEpoch e;
    e.eta = eta0 * decay;
    e.two_sigma_sq = (2.0 * sigma) * sigma;
    const double r = floor(sqrt(8.0 * e.two_sigma_sq)) + 2.0;
    e.radius = r < (double)M ? (uint32_t)r : M;
    e.pad = 0u;
    if (sigma_out) *sigma_out = sigma;
    return e;
}

__host__ __device__ inline uint32_t som_ring_distance(uint32_t i, uint32_t bmu, uint32_t M)
{
    const uint32_t d = i > bmu ? i - bmu : bmu - i;
    return d < M - d ? d : M - d;
}

// h of a ring distance; false: the neuron is skipped (then *h is 0 where the exp was not taken, else the h below the cut)
__host__ __device__ inline bool som_h(double d, double two_sigma_sq, double *h)
{
    const double y = ((-d) * d) / two_sigma_sq;
    if (y < kSomCutY) {
        *h = 0.0;
        return false;
    }
    *h = levy_exp(y);
    return !(*h < kSomCutH);
}

// one axis of the update (som.rs:112-113)
__host__ __device__ inline double som_pull(double neuron, double city, double eta, double h) { return neuron + (eta * h) * (city - neuron); }

// sq_dist (som.rs:8-10), the neuron first
__host__ __device__ inline double som_sq_dist(double nx, double ny, double cx, double cy)
{
    const double dx = nx - cx, dy = ny - cy;
    return (dx * dx) + (dy * dy);
}

// cos(2 pi u) and sin(2 pi u) for an f64 u in [0, 1); the cosine is levy_cos2pi(u) bit for bit
__host__ __device__ inline void som_cossin2pi(double u, double *cos_out, double *sin_out)
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
    *cos_out = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
    *sin_out = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
}

// neuron i of the start ring around the centroid (cx, cy)
__host__ __device__ inline void som_ring_neuron(uint32_t i, uint32_t M, double cx, double cy, double *x, double *y)
{
    double c, s;
    som_cossin2pi((double)i / (double)M, &c, &s);
    *x = cx + kSomRingRadius * c;
    *y = cy + kSomRingRadius * s;
}

// The cities as the solver trains on them (som.rs:27-50): normalised per axis in f64 into nx[n], ny[n], and the centroid, a sequential
// sum in city order.  xy: n f32 pairs, all finite.  n >= 1.
inline void som_normalise(const float *xy, uint32_t n, double *nx, double *ny, double *cx, double *cy)
{
    double mnx = (double)xy[0], mxx = mnx, mny = (double)xy[1], mxy = mny;
    for (uint32_t c = 1; c < n; ++c) {
        const double x = (double)xy[2u * c], y = (double)xy[2u * c + 1u];
        if (x < mnx) mnx = x;
        if (x > mxx) mxx = x;
        if (y < mny) mny = y;
        if (y > mxy) mxy = y;
    }
    double sx = mxx - mnx, sy = mxy - mny;
    if (!(sx > kSomMinSpan)) sx = kSomMinSpan;
    if (!(sy > kSomMinSpan)) sy = kSomMinSpan;
    double ax = 0.0, ay = 0.0;
    for (uint32_t c = 0; c < n; ++c) {
        nx[c] = ((double)xy[2u * c] - mnx) / sx;
        ny[c] = ((double)xy[2u * c + 1u] - mny) / sy;
        ax += nx[c];
        ay += ny[c];
    }
    *cx = ax / (double)n;
    *cy = ay / (double)n;
}

// The ranking key of extract_tour (som.rs:171-183): (neuron, distance, city index), a total order (no distance is NaN)
__host__ __device__ inline bool som_key_less(uint32_t bmu_a, double dist_a, uint32_t a, uint32_t bmu_b, double dist_b, uint32_t b)
{
    if (bmu_a != bmu_b) return bmu_a < bmu_b;
    if (dist_a != dist_b) return dist_a < dist_b;
    return a < b;
}

// checkpoint (som.rs:65)
__host__ __device__ inline uint32_t som_checkpoint(uint32_t epochs) { return epochs / 10u > 1u ? epochs / 10u : 1u; }

}  // namespace tl
