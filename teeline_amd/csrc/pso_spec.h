// pso_spec.h — the part of the particle swarm solver that is this project's specification rather than the reference's (DESIGN.md
// §4.20): the random stream and the spelled-out rounding.  One text for the device (particle_swarm.hip), the host
// (tl_api_pso.hip: tl_pso_draw, tl_pso_weight, tl_pso_keep) and the stand-alone CPU restatement
// (tests/probes/pso_cpu_baseline.cpp); tests/_pso_oracle.py states the same in numpy and literal loops.
//
// The stream is ga_spec.h's:
//   u(seed, run, event, slot) = mix(chain_key(seed, run) + G (32 event + slot + 1))              (arithmetic mod 2^64)
// Particle i of epoch e (P particles) owns the event e P + i: slot 0 is r1, slot 1 is r2, each (u >> 11) 2^-53, an f64 in [0, 1).
// Start particle i owns the events 2^58 + i n + j, slot 26: step j = n - 1 .. 1 of its Fisher-Yates pass,
// swap(a[j], a[position(u, j + 1)]) — ga_spec.h's init stream, unchanged.  Epoch events stay below 2^44 (epochs < 2^32, P <= 4096).
//
// The rounding.  f64::round is half away from zero; for x >= 0 it is spelled out as t = trunc(x), t + (x - t >= 0.5): no library
// round (np.round is half to even, floor(x + 0.5) is wrong just below .5), the same operations everywhere.  Every f64 product is
// evaluated left to right as the reference writes it — (1.5 r) len, w len — without FMA.
#pragma once
#include "ga_spec.h"

#pragma clang fp contract(off)

namespace tl {

constexpr uint32_t kPsoSlotR1 = 0, kPsoSlotR2 = 1;
constexpr uint32_t kPsoDefaultParticles = 30;  // particle_swarm.rs:15
constexpr uint32_t kPsoMaxParticles = 4096;    // the particle is the grid's x; epoch events stay far below the init events

__host__ __device__ inline uint32_t pso_particles(uint32_t n_nearest) { return n_nearest > kPsoDefaultParticles ? n_nearest : kPsoDefaultParticles; }
__host__ __device__ inline uint64_t pso_step_event(uint32_t epoch, uint32_t particles, uint32_t particle) { return (uint64_t)epoch * particles + particle; }
__host__ __device__ inline double pso_uniform(uint64_t u) { return (double)(u >> 11) * 1.1102230246251565e-16; }  // 2^-53: both factors exact

// v_max = max(ceil(n 0.35), 1) in f64 (particle_swarm.rs:33)
__host__ __device__ inline uint32_t pso_vmax(uint32_t n)
{
    const uint32_t v = (uint32_t)ceil((double)n * 0.35);
    return v > 1u ? v : 1u;
}

// w of an epoch (particle_swarm.rs:79): 0.9 - (0.9 - 0.4) (e / max(epochs, 1))
__host__ __device__ inline double pso_weight(uint32_t epoch, uint32_t epochs)
{
    const double frac = (double)epoch / (double)(epochs > 1u ? epochs : 1u);
    return 0.9 - (0.9 - 0.4) * frac;
}

// `x.round() as usize` for the x a keep can be: x >= 0 rounds half away from zero; NaN and x < 0 give 0, x >= 2^32 saturates
__host__ __device__ inline uint32_t pso_keep(double x)
{
    if (!(x > 0.0)) return 0u;
    if (x >= 4294967295.0) return 0xFFFFFFFFu;
    const double t = trunc(x);
    const uint32_t k = (uint32_t)t;
    return x - t >= 0.5 ? k + 1u : k;
}

// the keeps of a particle step, before `take` clamps them to their lists (particle_swarm.rs:86-94)
__host__ __device__ inline uint32_t pso_inertia_keep(double w, uint32_t vel_len) { return pso_keep(w * (double)vel_len); }
__host__ __device__ inline uint32_t pso_pull_keep(double r, uint32_t diff_len) { return pso_keep((1.5 * r) * (double)diff_len); }

// a swap (i, j) of positions, i < j, in one word
__host__ __device__ inline uint32_t pso_swap(uint32_t i, uint32_t j) { return i | (j << 16); }

}  // namespace tl
