// particle_swarm.hip — the particle swarm solver (particle_swarm.rs:22-129): R independent swarms, the run a grid dimension, the
// positions and personal bests (16-bit cities), the velocities (a swap in one word) and the costs in the context's workspace, two
// launches per epoch.
//
// The draws of particle i of epoch e are a pure function of (seed, run, e, i) (pso_spec.h: this project's specification — the
// reference draws from an unseeded thread RNG), so a particle's step depends on the other particles of its epoch through gbest
// alone.  Every particle is therefore moved at once against the epoch-start gbest, and the commit walks them in index order: at the
// first particle that improves gbest, the particles behind it are moved AGAIN, one after the other, against the new gbest — the
// reference's order, without a host round trip.  Most epochs improve nothing, so the second pass is rare.
//
//   k_pso_init    one workgroup per (particle, run): the start position (the initial tour, or a Fisher-Yates pass by one lane in
//                 LDS), its edge lengths by all lanes and their sum by one, in the reference's order (closing edge first).
//   k_pso_first   one workgroup per run: the FIRST minimum of the start costs is gbest.
//   k_pso_move    one workgroup per (particle, run): pso_step.
//   k_pso_commit  one workgroup per run: pbest and gbest in particle order, pso_step again where gbest has changed.
//
// pso_step: position and its inverse into LDS; the two swap sequences (route.rs:118-134) from their orbit form — with
// pi(p) = pos^-1[target[p]] the sequence is, in ascending i, (i, q) for every i that is not the largest position of its pi-cycle,
// q the first of pi(i), pi^2(i), .. above i (DESIGN.md §4.20 has the argument) — one lane per position walking its orbit, then a
// ballot/popcount compaction; the keeps; the new velocity; its swaps applied by one lane (they may share positions); the edge
// lengths in parallel and their sum by one lane.
//
//   LDS of a workgroup: 256 bytes of header and wave counts | la[n], lb[n] u32 (the two sequences; la's block holds the edge
//   lengths afterwards) | nv[vmax] u32 | pos[n], inv[n], pi[n] u16  (14 n + 4 vmax bytes).
#include "swarm_tour.h"
#include "pso_spec.h"
#include "swap_seq.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kPsoFixedBytes = 256;  // header (16 words), then the wave counts (2 parities x 16 waves)

__host__ __device__ __forceinline__ size_t pso_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

struct PsoLds {
    uint32_t *hdr, *wsum, *la, *lb, *nv;
    float *E;
    uint16_t *pos, *inv, *pi;
    __device__ PsoLds(unsigned char *smem, uint32_t n, uint32_t vmax)
    {
        hdr = reinterpret_cast<uint32_t *>(smem);
        wsum = hdr + 16;
        const size_t wd = pso_up16((size_t)n * 4), vl = pso_up16((size_t)vmax * 4), sh = pso_up16((size_t)n * 2);
        unsigned char *p = smem + kPsoFixedBytes;
        la = reinterpret_cast<uint32_t *>(p);
        E = reinterpret_cast<float *>(p);
        lb = reinterpret_cast<uint32_t *>(p + wd);
        nv = reinterpret_cast<uint32_t *>(p + 2 * wd);
        pos = reinterpret_cast<uint16_t *>(p + 2 * wd + vl);
        inv = reinterpret_cast<uint16_t *>(p + 2 * wd + vl + sh);
        pi = reinterpret_cast<uint16_t *>(p + 2 * wd + vl + 2 * sh);
    }
};

// One particle step (particle_swarm.rs:82-105) by the whole workgroup: from pos / vel / vlen[src] of particle i, its pbest and the
// run's gbest as they stand, to pos / vel / vlen[src ^ 1] and cost.  Ends behind a barrier.
template <bool DM>
__device__ void pso_step(const PsoArgs &A, const PsoLds &L, const CityDist<DM> &D, uint32_t run, uint32_t i, uint64_t key)
{
    const uint32_t n = A.n, P = A.particles, vmax = A.vmax, tid = threadIdx.x, nt = blockDim.x;
    const size_t idx = (size_t)run * P + i;
    const uint16_t *pos = A.pos[A.src] + idx * n;
    const uint32_t *vel = A.vel[A.src] + idx * vmax;
    const uint32_t vl = A.vlen[A.src][idx] < vmax ? A.vlen[A.src][idx] : vmax;
    for (uint32_t k = tid; k < n; k += nt) {
        const uint16_t c = pos[k];
        L.pos[k] = c;
        L.inv[c] = (uint16_t)k;
    }
    TL_SYNC();
    const uint32_t len_c = swap_sequence_orbit(A.pbest + idx * n, n, L, L.la);
    const uint32_t len_s = swap_sequence_orbit(A.gbest + (size_t)run * n, n, L, L.lb);
    const uint64_t ev = pso_step_event(A.epoch, P, i);
    const double r1 = pso_uniform(ga_draw_key(key, ev, kPsoSlotR1)), r2 = pso_uniform(ga_draw_key(key, ev, kPsoSlotR2));
    uint32_t ik = pso_inertia_keep(pso_weight(A.epoch, A.epochs), vl), ck = pso_pull_keep(r1, len_c), sk = pso_pull_keep(r2, len_s);
    ik = ik < vl ? ik : vl;  // (`take` clamps)
    ck = ck < len_c ? ck : len_c;
    sk = sk < len_s ? sk : len_s;
    const uint32_t total = ik + ck + sk < vmax ? ik + ck + sk : vmax;  // the concatenation, then truncate(v_max)
    uint32_t *dvel = A.vel[A.src ^ 1u] + idx * vmax;
    for (uint32_t t = tid; t < total; t += nt) {
        const uint32_t s = t < ik ? vel[t] : t < ik + ck ? L.la[t - ik] : L.lb[t - ik - ck];
        L.nv[t] = s;
        dvel[t] = s;
    }
    TL_SYNC();
    if (tid == 0) {  // apply_swaps (route.rs:137-143): in order — swaps may share positions
        for (uint32_t t = 0; t < total; ++t) {
            const uint32_t s = L.nv[t], a = s & 0xFFFFu, b = s >> 16;
            if (a < n && b < n) {
                const uint16_t x = L.pos[a];
                L.pos[a] = L.pos[b];
                L.pos[b] = x;
            }
        }
    }
    TL_SYNC();
    uint16_t *dpos = A.pos[A.src ^ 1u] + idx * n;
    for (uint32_t k = tid; k < n; k += nt) {
        const uint16_t c = L.pos[k];
        dpos[k] = c;
        L.E[k] = D(c, L.pos[k + 1u == n ? 0u : k + 1u]);
    }
    TL_SYNC();
    if (tid == 0) {
        A.cost[idx] = sum_edges(L.E, n);
        A.vlen[A.src ^ 1u][idx] = total;
    }
    TL_SYNC();
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_pso_init(PsoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, ind = blockIdx.x, run = blockIdx.y;
    const PsoLds L(smem, n, A.vmax);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    const bool given = ind == 0u && A.init != nullptr;
    uint16_t *r = L.pos;
    if (given) {
        const uint32_t *src = A.init + (size_t)run * A.init_stride;
        for (uint32_t k = tid; k < n; k += nt) r[k] = (uint16_t)src[k];
    } else {
        for (uint32_t k = tid; k < n; k += nt) r[k] = (uint16_t)k;
    }
    TL_SYNC();
    if (tid == 0 && !given) {
        for (uint32_t j = n - 1u; j >= 1u && j < n; --j) {
            const uint32_t k = sa_position(ga_draw_key(key, ga_init_event(n, ind, j), kGaSlotShuffle), j + 1u);
            const uint16_t x = r[j];
            r[j] = r[k];
            r[k] = x;
        }
    }
    TL_SYNC();
    const size_t idx = (size_t)run * A.particles + ind;
    uint16_t *dpos = A.pos[0] + idx * n, *dbest = A.pbest + idx * n;
    for (uint32_t k = tid; k < n; k += nt) {
        const uint16_t c = r[k];
        dpos[k] = c;
        dbest[k] = c;
        L.E[k] = D(c, r[k + 1u == n ? 0u : k + 1u]);
    }
    TL_SYNC();
    if (tid == 0) {
        A.pcost[idx] = sum_edges(L.E, n);
        A.vlen[0][idx] = 0u;
    }
}

// gbest of the start: the FIRST minimum of pbest_cost (min_by keeps the first of equals)
__global__ __launch_bounds__(256) void k_pso_first(PsoArgs A)
{
    __shared__ uint32_t pick;
    const uint32_t n = A.n, P = A.particles, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const float *pc = A.pcost + (size_t)run * P;
    if (tid == 0) {
        uint32_t b = 0;
        float best = pc[0];
        for (uint32_t i = 1; i < P; ++i) {
            if (pc[i] < best) {
                best = pc[i];
                b = i;
            }
        }
        pick = b;
        A.state[8u * (size_t)run] = __builtin_bit_cast(uint32_t, best);
        A.state[8u * (size_t)run + 1u] = 0u;
        if (A.last) A.out_cost[run] = best;
    }
    TL_SYNC();
    const uint32_t b = pick;
    const uint16_t *src = A.pbest + ((size_t)run * P + b) * n;
    for (uint32_t k = tid; k < n; k += nt) {
        A.gbest[(size_t)run * n + k] = src[k];
        if (A.last) A.out_pos[(size_t)run * n + k] = src[k];
    }
    if (run == 0u) log_improvement(A, 0u, 0xFFFFFFFFu, b, pc[b], src);
}

template <bool DM>
__global__ __launch_bounds__(256) void k_pso_move(PsoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PsoLds L(smem, A.n, A.vmax);
    const CityDist<DM> D{A.xy, A.dm_full, A.n};
    pso_step<DM>(A, L, D, blockIdx.y, blockIdx.x, sa_chain_key(A.seed, (uint64_t)A.first_run + blockIdx.y));
}

template <bool DM>
__global__ __launch_bounds__(256) void k_pso_commit(PsoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, P = A.particles, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const PsoLds L(smem, n, A.vmax);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    uint32_t *state = A.state + 8u * (size_t)run;
    float g = __builtin_bit_cast(float, state[0]);
    uint32_t improved = state[1];
    bool again = false;  // gbest has changed in this epoch: the particles from here on are moved against it before they count
    uint16_t *gbest = A.gbest + (size_t)run * n;
    for (uint32_t i = 0; i < P; ++i) {  // (every condition below is the same on every lane: the barriers are met by all)
        if (again) pso_step<DM>(A, L, D, run, i, key);
        const size_t idx = (size_t)run * P + i;
        const float c = A.cost[idx], pc = A.pcost[idx];
        const bool up = c < pc, ug = c < g;
        if (up || ug) {
            const uint16_t *p = A.pos[A.src ^ 1u] + idx * n;
            if (up) {
                uint16_t *pb = A.pbest + idx * n;
                for (uint32_t k = tid; k < n; k += nt) pb[k] = p[k];
            }
            if (ug) {
                for (uint32_t k = tid; k < n; k += nt) gbest[k] = p[k];
                ++improved;
                if (run == 0u) log_improvement(A, improved, A.epoch, i, c, p);
                g = c;
                again = true;
            }
            TL_SYNC();  // every lane has read pcost[idx]; gbest is whole before the next step reads it
            if (tid == 0 && up) A.pcost[idx] = c;
        }
    }
    if (tid == 0) {
        state[0] = __builtin_bit_cast(uint32_t, g);
        state[1] = improved;
        if (A.last) A.out_cost[run] = g;
    }
    if (A.epoch_log && run == 0u && A.epoch < A.epoch_cap) {
        uint32_t *rec = A.epoch_log + (size_t)A.epoch * 2u * P;
        for (uint32_t i = tid; i < P; i += nt) {
            rec[i] = __builtin_bit_cast(uint32_t, A.cost[(size_t)run * P + i]);
            rec[P + i] = A.vlen[A.src ^ 1u][(size_t)run * P + i];
        }
    }
    if (A.last) {
        for (uint32_t k = tid; k < n; k += nt) A.out_pos[(size_t)run * n + k] = gbest[k];
    }
}

// the device swap sequence on given permutation pairs (tl_pso_selftest_swap_sequence): one workgroup per pair
__global__ __launch_bounds__(256) void k_pso_selftest_swap_sequence(const uint16_t *from, const uint16_t *to, uint32_t n, uint32_t *out_pairs, uint32_t *out_len)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PsoLds L(smem, n, pso_vmax(n));
    const uint16_t *f = from + (size_t)blockIdx.x * n, *t = to + (size_t)blockIdx.x * n;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) L.inv[f[k]] = (uint16_t)k;
    TL_SYNC();
    const uint32_t len = swap_sequence_orbit(t, n, L, L.la);
    for (uint32_t k = threadIdx.x; k < len; k += blockDim.x) out_pairs[(size_t)blockIdx.x * n + k] = L.la[k];
    if (threadIdx.x == 0) out_len[blockIdx.x] = len;
}

size_t particle_swarm_lds_bytes(uint32_t n)
{
    return kPsoFixedBytes + 2 * pso_up16((size_t)n * 4) + pso_up16((size_t)pso_vmax(n) * 4) + 3 * pso_up16((size_t)n * 2);
}

uint32_t particle_swarm_max_n(int lds_budget)
{
    if (lds_budget <= 0) return 0u;
    uint64_t m = (uint64_t)lds_budget / 14u;
    if (m > 0xFFFFu) m = 0xFFFFu;  // (positions and swaps are 16 bits wide)
    while (m > 0u && particle_swarm_lds_bytes((uint32_t)m) > (size_t)lds_budget) --m;
    return (uint32_t)m;
}

int particle_swarm_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 64u ? 64 : t > 256u ? 256 : (int)t;
}

hipError_t launch_pso_init(const PsoArgs &A, uint32_t runs, hipStream_t s)
{
    hipError_t e = launch_max_lds(A.dm_full ? k_pso_init<true> : k_pso_init<false>, dim3(A.particles, runs), particle_swarm_threads(A.n), particle_swarm_lds_bytes(A.n), s, A);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pso_first, dim3(runs), dim3(particle_swarm_threads(A.n)), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_pso_move(const PsoArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_pso_move<true> : k_pso_move<false>, dim3(A.particles, runs), particle_swarm_threads(A.n), particle_swarm_lds_bytes(A.n), s, A);
}

hipError_t launch_pso_commit(const PsoArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_pso_commit<true> : k_pso_commit<false>, dim3(runs), particle_swarm_threads(A.n), particle_swarm_lds_bytes(A.n), s, A);
}

hipError_t launch_pso_selftest_swap_sequence(const uint16_t *from, const uint16_t *to, uint32_t n, uint32_t count, uint32_t *out_pairs, uint32_t *out_len,
                                             hipStream_t s)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_pso_selftest_swap_sequence));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pso_selftest_swap_sequence, dim3(count), dim3(particle_swarm_threads(n)), particle_swarm_lds_bytes(n), s, from, to, n, out_pairs, out_len);
    return hipGetLastError();
}

}  // namespace tl
