// fourier_curve.hip — the Fourier-curve solver (src/tsp/fourier.rs:10-312, fourier_spec.h): J independent jobs (option sets on one
// problem), the job a grid dimension, one workgroup per job, a span of gradient steps per launch.  The state is the 2 k_max + 1
// complex coefficients of a closed curve, not a tour.
//
//   k_fourier_steps   the steps [s0, s1) of a job, all in one CU's LDS: the coefficients, the basis table E (16 m bytes), the curve
//                     as f64 and its f32 copy for the search, every city's sample index, the cities, and two chunk buffers of
//                     gradient terms (LDS form); the workspace form keeps E, the cities and the sample indices in the job's
//                     workspace block instead — the same body, the other pointers.  A step is four phases:
//                       1. gamma: a lane per sample, the modes in order (fourier_gamma).
//                       2. search: S lanes a city (S a power of two, as many as the workgroup has for n cities), each over the
//                          samples j = s, s + S, ..; the least (root bits, index) of fourier_spec.h's total order, first per lane,
//                          then over the S lanes by shuffles.  The order is total, so the partition does not show in the answer.
//                       3. terms and sums: all lanes form the terms err conj(E[(k j) mod m]) of a chunk of cities into one of two
//                          LDS buffers; lanes 0 .. 2 L - 1, one per coefficient component, add the chunk in city order — ONE
//                          dependent f64 add per city, the loads independent of the accumulator — while the workgroup forms the
//                          next chunk into the other buffer: one barrier per chunk.
//                       4. tension and update: the same 2 L lanes, a component each (the reference's scalar-times-complex is per
//                          component).
//   k_fourier_decode  per job: the basis, one more curve, the search, the rank of every city by counting on (sample, city
//                     position) — a stable sort by sample —, the tour, its edge lengths by all lanes and their f32 sum by one, in
//                     the reference's order (closing edge first).
//   k_fourier_selftest_search  phase 2 alone on a curve given by the caller.
#include "chain_tour.h"
#include "fourier_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

__device__ __forceinline__ uint32_t fourier_lanes_per_city(uint32_t n, uint32_t nt)
{
    uint32_t S = 1;
    while (S < 64u && (uint64_t)n * (2u * S) <= nt) S *= 2u;
    return S;
}

__device__ __forceinline__ uint64_t fourier_shfl_xor(uint64_t v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}

// every city's nearest sample (fourier_spec.h, departure 3) by the whole workgroup; S lanes a city, S | 64
template <class GP, class CP, class SP>
__device__ __forceinline__ void fourier_search(const GP g32, uint32_t m, const CP cities, uint32_t n, SP sidx, uint32_t S)
{
    const uint32_t groups = blockDim.x / S, sub = threadIdx.x & (S - 1u), grp = threadIdx.x / S;
    for (uint32_t base = 0; base < n; base += groups) {  // (a uniform trip count: every lane takes part in the shuffles)
        const uint32_t c = base + grp;
        uint64_t best = ~0ull;
        if (c < n) {
            const float2 z = cities[c];
            for (uint32_t j = sub; j < m; j += S) {
                const float2 g = g32[j];
                const uint64_t k = fourier_pair_key(g.x, g.y, z.x, z.y, j);
                best = k < best ? k : best;
            }
        }
        for (uint32_t off = S >> 1; off > 0u; off >>= 1) {
            const uint64_t o = fourier_shfl_xor(best, (int)off);
            best = o < best ? o : best;
        }
        if (c < n && sub == 0u) sidx[c] = (uint32_t)best;  // (the low word is the index: sample 0 always has a key below ~0)
    }
}

}  // namespace

template <bool LDS>
__global__ __launch_bounds__(1024) void k_fourier_steps(FourierArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t job = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, n = A.n;
    const FourierJob P = A.jobs[job];
    const uint32_t s_end = A.s1 < P.total ? A.s1 : P.total;
    if (A.s0 >= s_end) return;  // (the whole workgroup)
    const uint32_t m = P.m, L = 2u * P.k_max + 1u, L2 = 2u * L, chunk = A.chunk;
    const size_t buf_stride = (size_t)chunk * 2u * A.max_l;
    double *c = reinterpret_cast<double *>(smem);
    double *gamma = c + 2u * A.max_l;
    double *terms = gamma + 2u * (size_t)A.max_m;
    double *e_lds = terms + 2u * buf_stride;
    double *E = LDS ? e_lds : A.basis + 2u * (size_t)P.off_m;
    float2 *g32 = reinterpret_cast<float2 *>(LDS ? e_lds + 2u * (size_t)A.max_m : e_lds);
    float2 *cities_lds = g32 + A.max_m;
    uint32_t *sidx = LDS ? reinterpret_cast<uint32_t *>(cities_lds + n) : A.sidx + (size_t)job * n;
    double *cg = A.coeffs + P.off_c;

    if (tid < L2) c[tid] = cg[tid];
    for (uint32_t r = tid; r < m; r += nt) {
        const FourierCx e = fourier_basis(r, m);
        E[2u * r] = e.re;
        E[2u * r + 1u] = e.im;
    }
    if (LDS)
        for (uint32_t i = tid; i < n; i += nt) cities_lds[i] = A.cities[i];
    uint32_t stage = A.s0 / P.epochs, within = A.s0 % P.epochs;
    double lambda = P.lambda;
    for (uint32_t i = 0; i < stage; ++i) lambda = lambda * P.lambda_decay;
    const uint32_t S = fourier_lanes_per_city(n, nt), nch = (n + chunk - 1u) / chunk;
    const int32_t my_k = (int32_t)(tid >> 1) - (int32_t)P.k_max;
    TL_SYNC();

    // the terms of chunk ch into buffer ch & 1: a lane per (city, mode)
    auto form = [&](uint32_t ch) {
        double *buf = terms + (size_t)(ch & 1u) * buf_stride;
        const uint32_t first = ch * chunk, cnt = n - first < chunk ? n - first : chunk;
        for (uint32_t p = tid; p < cnt * L; p += nt) {
            const uint32_t ci = p / L, ki = p - ci * L, i = first + ci;
            const uint32_t j = sidx[i];
            const float2 z = LDS ? cities_lds[i] : A.cities[i];
            const uint32_t r = fourier_index((int32_t)ki - (int32_t)P.k_max, j, m);
            const FourierCx t = fourier_term(FourierCx{gamma[2u * j], gamma[2u * j + 1u]}, z.x, z.y, FourierCx{E[2u * r], E[2u * r + 1u]});
            buf[(size_t)ci * L2 + 2u * ki] = t.re;
            buf[(size_t)ci * L2 + 2u * ki + 1u] = t.im;
        }
    };

    for (uint32_t s = A.s0; s < s_end; ++s) {
        for (uint32_t j = tid; j < m; j += nt) {
            const FourierCx g = fourier_gamma(c, E, P.k_max, m, j);
            gamma[2u * j] = g.re;
            gamma[2u * j + 1u] = g.im;
            g32[j] = make_float2((float)g.re, (float)g.im);
        }
        TL_SYNC();
        if (LDS) fourier_search(g32, m, cities_lds, n, sidx, S);
        else fourier_search(g32, m, A.cities, n, sidx, S);
        TL_SYNC();
        if (A.log && job == 0u && s < A.log_cap)
            for (uint32_t i = tid; i < n; i += nt) A.log[(size_t)s * n + i] = sidx[i];
        double acc = 0.0;
        form(0u);
        TL_SYNC();
        for (uint32_t ch = 0; ch < nch; ++ch) {
            if (ch + 1u < nch) form(ch + 1u);
            if (tid < L2) {
                const double *t = terms + (size_t)(ch & 1u) * buf_stride + tid;
                const uint32_t first = ch * chunk, cnt = n - first < chunk ? n - first : chunk;
                for (uint32_t ci = 0; ci < cnt; ++ci) acc = acc + t[(size_t)ci * L2];
            }
            TL_SYNC();
        }
        if (tid < L2) c[tid] = fourier_update(c[tid], acc, my_k, stage + 1u, lambda, P.lr_over_n);
        TL_SYNC();
        if (++within == P.epochs) {
            if (A.stage_c && job == 0u && tid < L2) A.stage_c[(size_t)stage * L2 + tid] = c[tid];
            within = 0u;
            ++stage;
            lambda = lambda * P.lambda_decay;
        }
    }
    if (tid < L2) cg[tid] = c[tid];
}

template <bool DM>
__global__ __launch_bounds__(256) void k_fourier_decode(FourierArgs A)
{
    const uint32_t job = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, n = A.n;
    const FourierJob P = A.jobs[job];
    const uint32_t m = P.m;
    const double *c = A.coeffs + P.off_c;
    double *E = A.basis + 2u * (size_t)P.off_m;
    float2 *g32 = A.g32 + P.off_m;
    uint32_t *sidx = A.sidx + (size_t)job * n, *tour = A.out_pos + (size_t)job * n;
    float *Ed = A.edge + (size_t)job * n;
    const CityDist<DM> D{A.xy, A.dm_full, n};
    for (uint32_t r = tid; r < m; r += nt) {
        const FourierCx e = fourier_basis(r, m);
        E[2u * r] = e.re;
        E[2u * r + 1u] = e.im;
    }
    TL_SYNC();
    for (uint32_t j = tid; j < m; j += nt) {
        const FourierCx g = fourier_gamma(c, E, P.k_max, m, j);
        g32[j] = make_float2((float)g.re, (float)g.im);
    }
    TL_SYNC();
    fourier_search(g32, m, A.cities, n, sidx, fourier_lanes_per_city(n, nt));
    TL_SYNC();
    for (uint32_t a = tid; a < n; a += nt) {  // sort_by_key(sample) is stable: ties fall in city order
        const uint32_t sa = sidx[a];
        uint32_t rank = 0;
        for (uint32_t b = 0; b < n; ++b) {
            const uint32_t sb = sidx[b];
            rank += (sb < sa || (sb == sa && b < a)) ? 1u : 0u;
        }
        tour[rank] = a;
    }
    TL_SYNC();
    for (uint32_t k = tid; k < n; k += nt) Ed[k] = D(tour[k], tour[k + 1u == n ? 0u : k + 1u]);
    TL_SYNC();
    if (tid == 0) {  // tour_length (distance_matrix.rs:235-245): the closing edge first, then the edges in order
        float tot = Ed[n - 1u];
        for (uint32_t k = 0; k + 1u < n; ++k) tot += Ed[k];
        A.out_cost[job] = tot;
    }
}

__global__ __launch_bounds__(1024) void k_fourier_selftest_search(FourierArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, nt = blockDim.x, n = A.n, m = A.max_m;
    float2 *g32 = reinterpret_cast<float2 *>(smem);
    float2 *cities = g32 + m;
    for (uint32_t j = tid; j < m; j += nt) g32[j] = make_float2((float)A.gamma_in[2u * j], (float)A.gamma_in[2u * j + 1u]);
    for (uint32_t i = tid; i < n; i += nt) cities[i] = A.cities[i];
    TL_SYNC();
    fourier_search(g32, m, cities, n, A.sidx, fourier_lanes_per_city(n, nt));
}

size_t fourier_curve_lds_bytes(uint32_t n, uint32_t max_l, uint32_t max_m, uint32_t chunk, bool lds_form)
{
    const size_t fixed = 16u * (size_t)max_l + 16u * (size_t)max_m + 2u * (size_t)chunk * 16u * max_l + 8u * (size_t)max_m;
    return fixed + (lds_form ? 16u * (size_t)max_m + 12u * (size_t)n : 0u);
}

int fourier_curve_threads(uint32_t n, uint32_t m)
{
    const uint64_t t = (((uint64_t)n * m / 32u) + 63u) & ~63ull;  // about 32 (city, sample) pairs a lane, in whole waves
    return t < 256u ? 256 : t > 1024u ? 1024 : (int)t;
}

template <class K>
static hipError_t fourier_launch(K kern, dim3 grid, int threads, size_t lds, hipStream_t s, const FourierArgs &A)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, A);
    return hipGetLastError();
}

hipError_t launch_fourier_steps(const FourierArgs &A, uint32_t jobs, int threads, bool lds_form, hipStream_t s)
{
    return fourier_launch(lds_form ? k_fourier_steps<true> : k_fourier_steps<false>, dim3(jobs), threads,
                          fourier_curve_lds_bytes(A.n, A.max_l, A.max_m, A.chunk, lds_form), s, A);
}

hipError_t launch_fourier_decode(const FourierArgs &A, uint32_t jobs, hipStream_t s)
{
    if (A.dm_full) hipLaunchKernelGGL(k_fourier_decode<true>, dim3(jobs), dim3(256), 0, s, A);
    else hipLaunchKernelGGL(k_fourier_decode<false>, dim3(jobs), dim3(256), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_fourier_selftest_search(const FourierArgs &A, int threads, hipStream_t s)
{
    return fourier_launch(k_fourier_selftest_search, dim3(1), threads, 8u * ((size_t)A.max_m + A.n), s, A);
}

}  // namespace tl
