// swarm_tour.h — what the kernels of the population solvers share on the device (internal to libteeline_gpu): the reference-order
// sum of a tour's edge lengths (particle_swarm.hip, cuckoo_search.hip, flower_pollination.hip, gravitational_search.hip,
// genetic.hip), the costing of a tour held in LDS, the row of the 4-word improvement log, and the launch that lifts the LDS limit
// (ant_colony.hip too).
//
// The rule of chain_tour.h's header holds here: a helper is in this file only while the kernels that use it compile to the
// instructions they had with their own copy (scripts/isa_diff.py; NOTEBOOK.md, the entry of this header).  What that rule kept in
// the kernel files, to be changed in step:
//   the start tour of k_{pso,fpa,gsa}_init: as one helper, k_fpa_init and k_gsa_init came out with their first scalar loads in another order;
//   the body of k_{pso,cs,fpa}_first: as one helper, 10 of ~158 instructions moved in each;
//   aco_sum_edges: ant_colony.hip's sum is the plain loop, and sum_edges in its place made k_aco_init 28 instructions longer.
// Each is once per call; the timing runs could not tell them from the parent beyond the box's own noise, but they were not identical.
#pragma once
#include "chain_tour.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

// tour_length's sum (distance_matrix.rs:235-245) of the n edge lengths E[k] = d(route[k], route[k + 1]), E[n - 1] the closing edge:
// one lane, the reference's order.  E is 16-byte aligned.
__device__ __forceinline__ float sum_edges(const float *E, uint32_t n)
{
    if (n < 2u) return 0.0f;
    float tot = E[n - 1u];
    uint32_t k = 0;
#pragma unroll 4
    for (; k + 4u <= n - 1u; k += 4u) {
        const float4 v = *reinterpret_cast<const float4 *>(E + k);
        tot += v.x;
        tot += v.y;
        tot += v.z;
        tot += v.w;
    }
    for (; k + 1u < n; ++k) tot += E[k];
    return tot;
}

// the tour in LDS to dst, its edge lengths into E (LDS) by all lanes and its cost by one.  Begins behind a barrier (the tour is
// whole), ends behind one.
template <bool DM>
__device__ void write_and_cost(const uint16_t *tour, float *E, const CityDist<DM> &D, uint32_t n, uint16_t *dst, float *cost)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    for (uint32_t p = tid; p < n; p += nt) {
        const uint16_t c = tour[p];
        dst[p] = c;
        E[p] = D(c, tour[p + 1u == n ? 0u : p + 1u]);
    }
    TL_SYNC();
    if (tid == 0) *cost = sum_edges(E, n);
    TL_SYNC();
}

// the row of the improvement log (epoch, who, cost bits, route index) and its route: by every lane
template <class Args>
__device__ void log_improvement(const Args &A, uint32_t k, uint32_t epoch, uint32_t who, float cost, const uint16_t *route)
{
    if (A.log && k < A.log_cap && threadIdx.x == 0) {
        uint32_t *rec = A.log + 4u * (size_t)k;
        rec[0] = epoch;
        rec[1] = who;
        rec[2] = __builtin_bit_cast(uint32_t, cost);
        rec[3] = A.route_log && k < A.route_cap ? k : 0xFFFFFFFFu;
    }
    if (A.route_log && k < A.route_cap) {
        uint32_t *dst = A.route_log + (size_t)k * A.n;
        for (uint32_t j = threadIdx.x; j < A.n; j += blockDim.x) dst[j] = route[j];
    }
}

}  // namespace

// a launch of `kern` with as much dynamic LDS as the device has
template <class K, class... KArgs>
static hipError_t launch_max_lds(K kern, dim3 grid, int threads, size_t lds, hipStream_t s, KArgs... args)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, args...);
    return hipGetLastError();
}

}  // namespace tl
