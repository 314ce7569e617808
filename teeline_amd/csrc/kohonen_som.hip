// kohonen_som.hip — the Kohonen self-organising map solver (src/tsp/som.rs:12-186): R independent runs, the run a grid dimension,
// one workgroup per run, a span of epochs per launch.  The state is a ring of M = n neuron_multiplier f64 points, not a tour.
//
//   k_som_train    the epochs [t0, t1) of a run.  The ring is two f64 arrays, x[M] and y[M] apart (8-byte LDS reads of consecutive
//                  neurons fall on consecutive banks), in LDS for the whole span (LDS form) or in the run's workspace block, which
//                  stays in L2 (workspace form: the same body, the other pointer).  Lane `tid` OWNS the neurons i = tid, tid + T,
//                  tid + 2 T, .. for the whole run: nobody else reads or writes them, so neither form needs a barrier or a fence
//                  for the ring — not at the load, not between the epochs, not at the store.  In one upward pass over its neurons
//                  a lane applies epoch t's update and measures the (updated) neuron against the city of epoch t + 1, keeping its
//                  first minimum (strict <).  The only workgroup step of an epoch is the BMU reduction, lexicographic on (distance,
//                  index): a wave reduction by shuffles, then the waves' results through LDS slots that are double-buffered by
//                  the epoch's parity — a wave may be writing epoch t + 1's slot while a slower one still reads epoch t's — which
//                  makes it ONE barrier per epoch.
//                  The update looks only at the neurons within the epoch's radius of the BMU (som_spec.h: host-computed from
//                  two_sigma_sq, conservative — outside it the specification's y < -8 test always skips) and applies the
//                  specification's two tests inside it.  The window is an integer test on the ring distance inside the one
//                  upward pass, so a window wider than the ring cannot visit a neuron twice.
//   k_som_extract  per run: every city's first-minimum neuron (the lanes over the cities, each scanning the ring upwards), the
//                  rank of every city under the key (neuron, distance, city index) by counting — the key is a total order, any
//                  correct sort gives the same tour —, the tour, its edge lengths by all lanes and their f32 sum by one, in the
//                  reference's order (closing edge first).
//   k_som_selftest_bmu  the training's scan and reduction alone, for cities 0 .. n - 1 in turn on a ring given by the caller.
//
// Threads of a training workgroup: about eight neurons a lane, in whole waves — T = clamp(round_up(ceil(M / 8), 64), 64, 1024).  A
// small ring gets one wave (its barrier is then nearly free), n = 1 002 x 8 the full 16.
#include "chain_tour.h"
#include "som_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr uint32_t kSomMaxWaves = 16;
constexpr uint32_t kSomNone = 0xFFFFFFFFu;

struct SomBest {
    double d;
    uint32_t i;
};

__device__ __forceinline__ bool som_better(double d, uint32_t i, const SomBest &b) { return d < b.d || (d == b.d && i < b.i); }

// the first minimum over the workgroup of every lane's (distance, index): to every lane.  par: the slot pair of this call; a call
// with the other parity may follow without a barrier in between, a call with the same parity only behind that one's barrier.
__device__ __forceinline__ uint32_t som_reduce_bmu(SomBest b, unsigned char *smem, uint32_t par)
{
    double *sd = reinterpret_cast<double *>(smem) + par * kSomMaxWaves;
    uint32_t *si = reinterpret_cast<uint32_t *>(smem + 2 * kSomMaxWaves * 8) + par * kSomMaxWaves;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(b.d, off, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)b.i, off, 64);
        if (som_better(od, oi, b)) {
            b.d = od;
            b.i = oi;
        }
    }
    if (nw == 1u) return b.i;
    if (lane == 0u) {
        sd[wave] = b.d;
        si[wave] = b.i;
    }
    TL_SYNC();
    SomBest r{sd[0], si[0]};
    for (uint32_t w = 1; w < nw; ++w) {
        const double od = sd[w];
        const uint32_t oi = si[w];
        if (som_better(od, oi, r)) {
            r.d = od;
            r.i = oi;
        }
    }
    return r.i;
}
static_assert(2 * kSomMaxWaves * 8 + 2 * kSomMaxWaves * 4 <= kSomLdsFixedBytes, "the slots fit the fixed part of the LDS");

// a lane's neurons against one city, upwards
__device__ __forceinline__ SomBest som_scan_own(const double *rx, const double *ry, uint32_t M, double cx, double cy)
{
    SomBest b{__builtin_huge_val(), kSomNone};
    for (uint32_t i = threadIdx.x; i < M; i += blockDim.x) {
        const double d = som_sq_dist(rx[i], ry[i], cx, cy);
        if (d < b.d) {
            b.d = d;
            b.i = i;
        }
    }
    return b;
}

}  // namespace

template <bool LDS>
__global__ __launch_bounds__(1024) void k_som_train(SomArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, M = A.M, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    double *blk = A.ring + (size_t)run * 2u * M;
    double *rx = LDS ? reinterpret_cast<double *>(smem + kSomLdsFixedBytes) : blk;
    double *ry = rx + M;
    const double *src = A.fresh ? A.ring0 : blk;
    if (LDS || A.fresh)
        for (uint32_t i = tid; i < M; i += nt) {  // a lane loads what it owns: no barrier
            rx[i] = src[i];
            ry[i] = src[M + i];
        }
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    uint32_t city = A.t0 < A.t1 ? som_city(key, A.t0, n) : 0u;
    double cx = A.cities[city], cy = A.cities[n + city];
    SomBest best = som_scan_own(rx, ry, M, cx, cy);
    for (uint32_t t = A.t0; t < A.t1; ++t) {
        const uint32_t bmu = som_reduce_bmu(best, smem, t & 1u);
        if (A.log && run == 0u && tid == 0u && t - 1u < A.log_cap) {
            A.log[2u * (size_t)(t - 1u)] = city;
            A.log[2u * (size_t)(t - 1u) + 1u] = bmu;
        }
        const SomEpoch E = A.sched[t - 1u];
        const bool more = t + 1u < A.t1;
        const uint32_t ncity = more ? som_city(key, t + 1u, n) : 0u;
        const double ncx = A.cities[ncity], ncy = A.cities[n + ncity];
        best.d = __builtin_huge_val();
        best.i = kSomNone;
        for (uint32_t i = tid; i < M; i += nt) {
            double x = rx[i], y = ry[i];
            const uint32_t dr = som_ring_distance(i, bmu, M);
            if (dr <= E.radius) {
                double h;
                if (som_h((double)dr, E.two_sigma_sq, &h)) {
                    x = som_pull(x, cx, E.eta, h);
                    y = som_pull(y, cy, E.eta, h);
                    rx[i] = x;
                    ry[i] = y;
                }
            }
            if (more) {
                const double d = som_sq_dist(x, y, ncx, ncy);
                if (d < best.d) {
                    best.d = d;
                    best.i = i;
                }
            }
        }
        city = ncity;
        cx = ncx;
        cy = ncy;
    }
    if (LDS)
        for (uint32_t i = tid; i < M; i += nt) {
            blk[i] = rx[i];
            blk[M + i] = ry[i];
        }
}

template <bool DM>
__global__ __launch_bounds__(256) void k_som_extract(SomArgs A)
{
    const uint32_t n = A.n, M = A.M, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const double *rx = A.ring + (size_t)run * 2u * M, *ry = rx + M;
    uint32_t *bmu = A.bmu + (size_t)run * n, *tour = A.out_pos + (size_t)run * n;
    double *bd = A.bdist + (size_t)run * n;
    float *E = A.edge + (size_t)run * n;
    const CityDist<DM> D{A.xy, A.dm_full, n};
    for (uint32_t c = tid; c < n; c += nt) {
        const double cx = A.cities[c], cy = A.cities[n + c];
        double best = som_sq_dist(rx[0], ry[0], cx, cy);
        uint32_t at = 0;
        for (uint32_t i = 1; i < M; ++i) {
            const double d = som_sq_dist(rx[i], ry[i], cx, cy);
            if (d < best) {
                best = d;
                at = i;
            }
        }
        bmu[c] = at;
        bd[c] = best;
    }
    TL_SYNC();
    for (uint32_t c = tid; c < n; c += nt) {
        const uint32_t mb = bmu[c];
        const double md = bd[c];
        uint32_t rank = 0;
        for (uint32_t b = 0; b < n; ++b) rank += som_key_less(bmu[b], bd[b], b, mb, md, c) ? 1u : 0u;
        tour[rank] = c;
    }
    TL_SYNC();
    for (uint32_t k = tid; k < n; k += nt) E[k] = D(tour[k], tour[k + 1u == n ? 0u : k + 1u]);
    TL_SYNC();
    if (tid == 0) {  // tour_length (distance_matrix.rs:235-245): the closing edge first, then the edges in order
        float tot = E[n - 1u];
        for (uint32_t k = 0; k + 1u < n; ++k) tot += E[k];
        A.out_cost[run] = tot;
    }
}

template <bool LDS>
__global__ __launch_bounds__(1024) void k_som_selftest_bmu(SomArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, M = A.M, tid = threadIdx.x, nt = blockDim.x;
    double *rx = LDS ? reinterpret_cast<double *>(smem + kSomLdsFixedBytes) : A.ring;
    double *ry = rx + M;
    if (LDS)
        for (uint32_t i = tid; i < M; i += nt) {
            rx[i] = A.ring[i];
            ry[i] = A.ring[M + i];
        }
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t b = som_reduce_bmu(som_scan_own(rx, ry, M, A.cities[c], A.cities[n + c]), smem, c & 1u);
        if (tid == 0) A.bmu[c] = b;
    }
}

int kohonen_som_threads(uint32_t M)
{
    const uint32_t t = ((M + 7u) / 8u + 63u) & ~63u;
    return t < 64u ? 64 : t > 1024u ? 1024 : (int)t;
}

template <class K>
static hipError_t som_launch(K kern, dim3 grid, int threads, size_t lds, hipStream_t s, const SomArgs &A)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, A);
    return hipGetLastError();
}

hipError_t launch_som_train(const SomArgs &A, uint32_t runs, bool lds_form, hipStream_t s)
{
    return som_launch(lds_form ? k_som_train<true> : k_som_train<false>, dim3(runs), kohonen_som_threads(A.M), kohonen_som_lds_bytes(A.M, lds_form), s, A);
}

hipError_t launch_som_extract(const SomArgs &A, uint32_t runs, hipStream_t s)
{
    if (A.dm_full) hipLaunchKernelGGL(k_som_extract<true>, dim3(runs), dim3(256), 0, s, A);
    else hipLaunchKernelGGL(k_som_extract<false>, dim3(runs), dim3(256), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_som_selftest_bmu(const SomArgs &A, int threads, bool lds_form, hipStream_t s)
{
    return som_launch(lds_form ? k_som_selftest_bmu<true> : k_som_selftest_bmu<false>, dim3(1), threads, kohonen_som_lds_bytes(A.M, lds_form), s, A);
}

}  // namespace tl
