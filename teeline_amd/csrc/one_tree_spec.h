// one_tree_spec.h — the Held-Karp lower bound as this project specifies it: the scalar part of the subgradient
// ascent and the order of the 1-tree's keys.  One text for the device (one_tree_bound.hip), the host (tl_api_onetree.hip: the
// sequential restatement tl_one_tree_bound_host) and the stand-alone one-core probe (tests/probes/one_tree_cpu_baseline.cpp);
// tests/_one_tree_oracle.py states the same in numpy and is the statement of record.  All f64, contraction off.
//
// A 1-tree under node penalties pi with special position s: Prim's tree over the positions other than s by prim_mst's rule
// (christofides.hip: the non-tree position of smallest key, the FIRST in position order among equals; key[v] = w(u, v), parent[v] = u
// wherever w(u, v) < key[v] strictly) plus the two smallest w(s, v), with w(i, j) = (double)d(i, j) + (pi_i + pi_j).
//   L = (the taken keys summed in the order Prim took them, then the two root edges in the order chosen) - 2 (pi summed in position order)
// every sum sequential.  g_i = degree_i - 2.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace tl {

constexpr uint32_t kOneTreeNone = 0xFFFFFFFFu;  // the parent of Prim's start and of the root
enum : uint32_t { kOneTreeStopNone = 0, kOneTreeStopTour = 1, kOneTreeStopLambda = 2, kOneTreeStopUpper = 3, kOneTreeStopIterations = 4 };
constexpr double kOneTreeLambdaFloor = 0x1p-20;

struct OneTreeJob {  // one option set of a batch
    double lambda0, upper;
    uint32_t root, iterations, patience, pad_;
};

struct OneTreeState {  // a job's ascent between two iterations: what a launch loads and stores
    double lambda, best;
    uint32_t stall, best_iter, k, stop, is_tour, pad_;
    uint32_t best_nb[2];  // the best tree's root neighbours in the order chosen
    uint32_t tour_nb[2];  // those of the tree that was a tour
};

__host__ __device__ inline void one_tree_start(OneTreeState &S, const OneTreeJob &J)
{
    S.lambda = J.lambda0;
    S.best = -__builtin_huge_val();
    S.stall = S.best_iter = S.k = S.stop = S.is_tour = S.pad_ = 0u;
    S.best_nb[0] = S.best_nb[1] = S.tour_nb[0] = S.tour_nb[1] = kOneTreeNone;
}

// An f64 key as an unsigned order: -0.0 is +0.0 (the comparison is `<` on numbers), then the total-order bits.  Keys are never NaN.
__host__ __device__ inline uint64_t one_tree_ordered(double k)
{
    uint64_t b = __builtin_bit_cast(uint64_t, k);
    if (b == 0x8000000000000000ull) b = 0ull;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double one_tree_unordered(uint64_t o)
{
    const uint64_t b = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o;
    return __builtin_bit_cast(double, b);
}

// Steps 2 - 7 of iteration S.k on its 1-tree's value L and sum of squared subgradients g2.  Returns whether L is the new best; S.stop
// is set where the ascent ends with this iteration, else *t is the step of pi_i += t g_i.  S.k counts the iterations run.
__host__ __device__ inline bool one_tree_decide(OneTreeState &S, const OneTreeJob &J, double L, uint32_t g2, double *t)
{
    const bool improved = L > S.best;
    if (improved) {
        S.best = L;
        S.best_iter = S.k;
        S.stall = 0u;
    } else if (++S.stall == J.patience) {
        S.lambda = S.lambda * 0.5;
        S.stall = 0u;
    }
    ++S.k;
    *t = 0.0;
    if (g2 == 0u) {
        S.stop = kOneTreeStopTour;
        S.is_tour = 1u;
    } else if (S.lambda < kOneTreeLambdaFloor) {
        S.stop = kOneTreeStopLambda;
    } else if (J.upper - L <= 0.0) {
        S.stop = kOneTreeStopUpper;
    } else {
        *t = S.lambda * (J.upper - L) / (double)g2;
        if (S.k == J.iterations) S.stop = kOneTreeStopIterations;
    }
    return improved;
}

}  // namespace tl
