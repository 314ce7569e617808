// fourier_spec.h — the Fourier-curve solver (src/tsp/fourier.rs:10-312) as this project specifies it.  One text for
// the device (fourier_curve.hip), the host (tl_api_fourier.hip) and the stand-alone CPU restatement
// (tests/probes/fourier_cpu_baseline.cpp); tests/_fourier_oracle.py states the same in numpy and literal loops.  All f64 except the
// nearest-sample search, contraction off, NO library cos, sin, exp or hypot.
//
// The solver draws nothing.  A closed curve gamma(s) = sum_k c_k e^{2 pi i k s}, k = -k_max .. k_max, is sampled at s = j / m and
// descends on 0.5 sum_cities |gamma(nearest sample) - city|^2 + tension: k_max stages (stage s frees the modes |k| <= s + 1) of
// `epochs` gradient steps each, lambda multiplied by lambda_decay after every stage.  The tour is the cities by nearest sample.
//
// Everything is the reference's sequence of operations, spelled out — the sequential sums over the cities in city order included —
// except the FIVE departures:
//
// 1. The basis.  e^{2 pi i k j / m} = E[(k j) mod m] (the non-negative remainder for k < 0) with E[r] = som_cossin2pi((double)r /
//    (double)m), som_spec.h's exact quadrant reduction, used as it is.  The reduction of k j is exact, so the whole basis is one table
//    of m complex numbers, read by gamma and by the gradient alike.  The reference takes libm's cos and sin of the rounded angle
//    2 pi k (j / m), twice (eval_curve, compute_basis).
// 2. The radius.  |z| = sqrt(re re + im im), the IEEE sqrt, not libm's hypot.
// 3. The nearest sample.  Samples and city as f32; d_j = sqrt(dx dx + dy dy) in f32 with dx = sample - city (kdtree.rs:291-295).
//    The nearest sample is the one with the least d_j, the LOWEST index among equal d_j; equality is decided AFTER the f32 sqrt
//    (two different squares can round to one root).  Stated as a total order so that any partition of the samples among lanes gives
//    the same answer: the least (key(d_j), j) with key = the bits of d_j (d_j >= +0, so the bits order as the values do) and
//    0xFFFFFFFF for a NaN (a curve that has left the finite numbers: a NaN is never nearer than a number; all NaN: sample 0).  The
//    reference takes the first nearest its kd-tree visits, which depends on select_nth_unstable_by and cannot be restated.
// 4. (2 pi k)^2 = t t with t = 6.283185307179586 (double)k.
// 5. lambda of stage s is the running product lambda, lambda decay, (lambda decay) decay, .. as the reference forms it, not a power.
//
// Measured sizes of the departures (tests/_fourier_oracle.py's libm variant against this text, on the CPU; the reference itself
// was not run: no Rust toolchain where this was built — none of these is "the reference's" number):
#pragma once
#include "som_spec.h"
#if defined(__HIPCC__)
#include "tl_device.h"
#endif

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kFourierMaxK = 32;       // k_max: k j < 2^17 stays far inside 32 bits, L = 65 coefficient slots
constexpr uint32_t kFourierMaxM = 4096;     // samples: the basis table, gamma and its f32 copy fit one CU's LDS
constexpr uint32_t kFourierMaxN = 65536;    // what kohonen_som accepts with multiplier 1
constexpr double kFourierTwoPi = 6.283185307179586;
// departure 1: the largest |E[(k j) mod m] - (cos, sin)(2 pi k (j / m))| over m in {2, 50, 200, 4096}, |k| <= 32, all j
constexpr double kFourierBasisMeasuredAbsDiff = 3.6e-14;  // (at m = 200; a test's bound is twice this)
// departures 1-3 together, default options: cities whose final tour position differs from the libm variant's, of 52 and of 280
constexpr uint32_t kFourierBerlin52MovedCities = 0;
constexpr uint32_t kFourierA280MovedCities = 0;
// departure 3: queries (city, step) of those two runs, decode included, whose least f32 root is shared by two samples or more
constexpr uint32_t kFourierBerlin52TiedQueries = 1;  // of 52 x 1 601
constexpr uint32_t kFourierA280TiedQueries = 0;      // of 280 x 1 601

struct FourierCx {
    double re, im;
};

// num_complex's product
__host__ __device__ inline FourierCx fourier_mul(FourierCx a, FourierCx b) { return FourierCx{(a.re * b.re) - (a.im * b.im), (a.re * b.im) + (a.im * b.re)}; }

// the table index of e^{2 pi i k j / m}: (k j) mod m, non-negative.  |k| <= 32, j < m <= 4096
__host__ __device__ inline uint32_t fourier_index(int32_t k, uint32_t j, uint32_t m)
{
    const int32_t r = (k * (int32_t)j) % (int32_t)m;
    return (uint32_t)(r < 0 ? r + (int32_t)m : r);
}

// E[r], r < m
__host__ __device__ inline FourierCx fourier_basis(uint32_t r, uint32_t m)
{
    FourierCx e;
    som_cossin2pi((double)r / (double)m, &e.re, &e.im);
    return e;
}

// gamma[j] (eval_curve): from zero, the modes in order.  c: L = 2 k_max + 1 pairs (re, im); E: m pairs
template <class CP, class EP>
__host__ __device__ inline FourierCx fourier_gamma(const CP c, const EP E, uint32_t k_max, uint32_t m, uint32_t j)
{
    FourierCx g{0.0, 0.0};
    uint32_t r = fourier_index(-(int32_t)k_max, j, m);
    for (uint32_t ki = 0; ki <= 2u * k_max; ++ki) {
        const FourierCx p = fourier_mul(FourierCx{c[2u * ki], c[2u * ki + 1u]}, FourierCx{E[2u * r], E[2u * r + 1u]});
        g.re = g.re + p.re;
        g.im = g.im + p.im;
        r += j;  // (k + 1) j mod m
        if (r >= m) r -= m;
    }
    return g;
}

// departure 3: the key of one sample against one city; the search keeps the least (key << 32 | j)
__host__ __device__ inline float fourier_root(float sx, float sy, float cx, float cy)
{
    const float dx = sx - cx, dy = sy - cy;
    const float sq = (dx * dx) + (dy * dy);
#if defined(__HIP_DEVICE_COMPILE__)
    return sqrt_rn(sq);  // correctly rounded (tl_device.h; tests/test_gpu_numerics.py sweeps every non-negative float)
#else
    return sqrtf(sq);
#endif
}
__host__ __device__ inline uint64_t fourier_key(float d, uint32_t j)
{
    const uint32_t b = d != d ? 0xFFFFFFFFu : __builtin_bit_cast(uint32_t, d);
    return ((uint64_t)b << 32) | j;
}
__host__ __device__ inline uint64_t fourier_pair_key(float sx, float sy, float cx, float cy, uint32_t j) { return fourier_key(fourier_root(sx, sy, cx, cy), j); }

// one city's term of the attraction for mode ki: (gamma[j] - city) conj(E[(k j) mod m])
__host__ __device__ inline FourierCx fourier_term(FourierCx gamma_j, float cx, float cy, FourierCx e)
{
    const FourierCx err{gamma_j.re - (double)cx, gamma_j.im - (double)cy};
    return fourier_mul(err, FourierCx{e.re, -e.im});
}

// tension and update of one COMPONENT (re or im) of mode k: the reference's scalar-times-complex is per component
__host__ __device__ inline double fourier_update(double c, double grad, int32_t k, uint32_t k_active, double lambda, double lr_over_n)
{
    const double t = kFourierTwoPi * (double)k;
    const double g = grad + ((lambda * (t * t)) * c);
    const uint32_t ak = (uint32_t)(k < 0 ? -k : k);
    return ak <= k_active ? c - (lr_over_n * g) : c;
}

// The start coefficients (fourier.rs:23-32, 53-58): the centroid a sequential complex sum in city order over n, the radius the mean
// of |z - centroid| (departure 2).  c: 2 (2 k_max + 1) doubles.  n >= 1
inline void fourier_init(const float *xy, uint32_t n, uint32_t k_max, double *c)
{
    double sr = 0.0, si = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        sr = sr + (double)xy[2u * i];
        si = si + (double)xy[2u * i + 1u];
    }
    const double cr = sr / (double)n, ci = si / (double)n;
    double rs = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const double dr = (double)xy[2u * i] - cr, di = (double)xy[2u * i + 1u] - ci;
        rs = rs + sqrt((dr * dr) + (di * di));
    }
    const double radius = rs / (double)n;
    for (uint32_t q = 0; q < 2u * (2u * k_max + 1u); ++q) c[q] = 0.0;
    c[2u * k_max] = cr;
    c[2u * k_max + 1u] = ci;
    c[2u * (k_max + 1u)] = radius * 0.5;
}

}  // namespace tl
