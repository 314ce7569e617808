// chain_tour.h — what the kernels of the seeded solvers share on the device (internal to libteeline_gpu): the distance between two
// cities (sim_anneal.hip, tabu_search.hip, hill_climb.hip, and through swarm_tour.h genetic.hip and the population solvers) and the
// minimum over a wave (the first three of them).
//
// The resident tour itself — perm | E | S, the costing walk of a reversal and its commit — is NOT in here: sim_anneal.hip,
// tabu_search.hip and hill_climb.hip each keep their copy.  Folding two into always-inlined helpers gave kernels with the parent's
// registers and LDS but 2–4 % more kernel time on the same box, in both forms that were measured (NOTEBOOK.md, the entry of this
// header), so the three copies have to be changed in step until a form is found that compiles to the code they have now.
#pragma once
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

// The distance between two cities: the coordinates, or the full matrix.
template <bool DM>
struct CityDist {
    const float2 *xy;
    const float *full;
    uint32_t n;
    __device__ __forceinline__ float operator()(uint32_t a, uint32_t b) const  // city indices
    {
        if (DM) return full[(size_t)a * n + b];
        return dist(xy[a], xy[b]);
    }
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace

}  // namespace tl
