// gsa_spec.h — the part of the gravitational search solver that is this project's specification rather than the reference's
// (DESIGN.md §4.23): the random stream, the order among equal masses, the fixed exp and the spelled-out rounding.  One text for
// the device (gravitational_search.hip), the host (tl_api_gsa.hip: tl_gsa_draw, tl_gsa_g, tl_gsa_pull_swaps, tl_gsa_masses) and
// the stand-alone CPU restatement (tests/probes/gsa_cpu_baseline.cpp); tests/_gsa_oracle.py states the same in numpy and literal
// loops.
//
// The stream is ga_spec.h's:
//   u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1))              (arithmetic mod 2^64)
// The pull of agent j on agent i in epoch e (N agents) owns the event (e N + i) N + j — keyed by the agent index j, not by its
// rank: slot 0 is r = (u >> 11) 2^-53.  Start agent i owns the events 2^58 + i n + j, slot 26: step j = n - 1 .. 1 of its
// Fisher-Yates pass — ga_spec.h's init stream, unchanged.  Epoch events stay below 2^56 < 2^58 (epochs < 2^32, N <= 4096).  No
// draw depends on another; a draw the reference would not have made (j == i, j outside kbest) is simply not read.
//
// The ranking.  The reference ranks with sort_unstable_by on the masses (gravitational_search.rs:96), whose order among equal
// masses is unspecified — and equal masses are common: the uniform case, duplicated tours.  Here the order is descending mass,
// TIES IN ASCENDING AGENT INDEX (what a stable sort gives): rank(a) = #{b : m_b > m_a or (m_b == m_a and b < a)}.
//
// g = 20 levy_exp(-((1.0 e) / max(epochs, 1))): levy_spec.h's fixed-sequence exp, not libm's, as the annealing schedule's.
// n_swaps = round((r g) mass), left to right without FMA, f64::round spelled out (pso_spec.h: pso_keep).
//
// A pull is short.  r < 1; g <= G0 = 20, because the argument of exp is never positive, levy_exp of a non-positive argument is at
// most 1 and levy_exp(0) is exactly 1 (k = 0, r = 0, q = ec[0]); mass <= 1 (one term of a sum of non-negative terms, over that
// sum).  So (r g) mass < 20 and n_swaps <= kGsaMaxPull = 20: only the first 20 pairs of a swap sequence are ever needed.
#pragma once
#include "ga_spec.h"
#include "levy_spec.h"
#include "pso_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kGsaSlotR = 0;
constexpr uint32_t kGsaDefaultAgents = 25;  // gravitational_search.rs:17
constexpr uint32_t kGsaMaxAgents = 4096;    // epoch events stay below the init events
constexpr uint32_t kGsaMaxPull = 20;        // n_swaps <= round(r G0 1) with r < 1 (above)
constexpr double kGsaG0 = 20.0, kGsaAlpha = 1.0, kGsaInertiaW = 0.0;  // gravitational_search.rs:11-15
constexpr double kGsaEpsilon = 2.220446049250313e-16;                  // f64::EPSILON

__host__ __device__ inline uint32_t gsa_agents(uint32_t n_nearest) { return n_nearest > kGsaDefaultAgents ? n_nearest : kGsaDefaultAgents; }
__host__ __device__ inline uint32_t gsa_kbest(uint32_t agents) { return (agents + 1u) / 2u; }  // div_ceil(2)
__host__ __device__ inline uint64_t gsa_event(uint32_t epoch, uint32_t agents, uint32_t i, uint32_t j) { return ((uint64_t)epoch * agents + i) * agents + j; }
__host__ __device__ inline double gsa_r(uint64_t key, uint32_t epoch, uint32_t agents, uint32_t i, uint32_t j)
{
    return levy_uniform(ga_draw_key(key, gsa_event(epoch, agents, i, j), kGsaSlotR));
}

// g of an epoch (gravitational_search.rs:101)
__host__ __device__ inline double gsa_g(uint32_t epoch, uint32_t epochs)
{
    return kGsaG0 * levy_exp(-((kGsaAlpha * (double)epoch) / (double)(epochs > 1u ? epochs : 1u)));
}

// what is kept of the old velocity (gravitational_search.rs:105): round(0 len) = 0, spelled out as the reference has it
__host__ __device__ inline uint32_t gsa_inertia_keep(uint32_t vel_len) { return pso_keep(kGsaInertiaW * (double)vel_len); }

// n_swaps of a pull (gravitational_search.rs:114)
__host__ __device__ inline uint32_t gsa_pull_swaps(double r, double g, double mass) { return pso_keep((r * g) * mass); }

// `fold(NEG_INFINITY, f32::max)` (gravitational_search.rs:79): f32::max ignores a NaN operand
__host__ __device__ inline float gsa_worst(const float *costs, uint32_t agents)
{
    float w = -__builtin_huge_valf();
    for (uint32_t a = 0; a < agents; ++a)
        if (costs[a] > w) w = costs[a];
    return w;
}

// sum_fitness (gravitational_search.rs:81): the subtraction in f32, the sum in f64 in agent order (from 0.0)
__host__ __device__ inline double gsa_sum_fitness(const float *costs, uint32_t agents, float worst)
{
    double s = 0.0;
    for (uint32_t a = 0; a < agents; ++a) s += (double)(worst - costs[a]);
    return s;
}

// the mass of an agent of cost c (gravitational_search.rs:83-91)
__host__ __device__ inline double gsa_mass(float c, float worst, double sum_fitness, uint32_t agents)
{
    return sum_fitness < kGsaEpsilon ? 1.0 / (double)agents : (double)(worst - c) / sum_fitness;
}

// the rank of agent a: descending mass, ties in ascending agent index (no mass is NaN)
__host__ __device__ inline uint32_t gsa_rank(const double *mass, uint32_t agents, uint32_t a)
{
    const double m = mass[a];
    uint32_t r = 0;
    for (uint32_t b = 0; b < agents; ++b) r += (mass[b] > m || (mass[b] == m && b < a)) ? 1u : 0u;
    return r;
}

}  // namespace tl
