// gravitational_search.hip — the gravitational search solver (gravitational_search.rs:23-145): R independent runs, the run a grid
// dimension, the positions (16-bit cities), the costs, the masses, the ranking and gbest in the context's workspace, one launch
// for a span of epochs.
//
// Every agent moves in every epoch, and agent i reads the positions of the ceil(N / 2) heaviest agents AS THEY STAND: those of a
// lower index have already moved in this epoch.  Building every move against the epoch-start state — the siblings' form — would
// build most of them twice, so the agents are walked in order by one workgroup per run and the parallelism lies inside an agent's
// step: its pulls are all computed against the same unchanged positions[i], a wave per pull, the lanes over the positions.
//
// The r of a pull is a pure function of (seed, run, e, i, j) (gsa_spec.h: this project's specification — the reference draws from
// an unseeded thread RNG), and n_swaps = round((r g) mass_j) <= kGsaMaxPull = 20, so of swap_sequence(positions[i], positions[j])
// only the first n_swaps pairs are ever looked for: with pi(p) = inv_i[positions[j][p]] computed on the fly — no pi table is
// built — a lane walks the orbit of its position p while the image is below p, a pair (p, q) exists where the walk ends at q > p
// (swap_seq.h has the rule), and a ballot/popcount compaction puts the pairs of a chunk of 64 ascending positions into the pull's
// 20-word slot.  The wave stops at the first chunk that completes the prefix.
//
//   k_gsa_init    one workgroup per (agent, run): the start position (the initial tour, or a Fisher-Yates pass by one lane in
//                 LDS), its edge lengths by all lanes and their sum by one, in the reference's order (closing edge first).
//   k_gsa_first   one workgroup per run: gbest is a copy of the FIRST minimum agent; a NaN start cost is where the reference
//                 panics (state word 2).
//   k_gsa_epochs  one workgroup per run, the epochs [e0, e1).  Per epoch: worst and sum_fitness by one lane (the f64 sum in agent
//                 order), the masses and the ranks by counting, a lane per agent; a NaN mass is where the reference panics.  Per
//                 agent: positions[i] and its inverse into LDS; the live pulls (n_swaps > 0) compacted in kbest order, 256 ranks
//                 at a time; a wave per live pull; one lane applies the slots in kbest order until v_max swaps are applied —
//                 the inverse in LDS stays that of the unchanged positions[i], so later pulls still read it; the edge lengths
//                 by all lanes, their sum by one; the gbest rule, the log, the epoch row; the position goes back to the
//                 workspace behind a barrier before the next agent reads it.
//
//   LDS of a workgroup: 1536 bytes (header, wave counts, 256 live pulls, 4 slots of 20 pairs) | E[n] f32 | cur[n], inv[n] u16
//   (8 n bytes).
#include "swarm_tour.h"
#include "gsa_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kGsaFixedBytes = 1536;
constexpr uint32_t kGsaLiveChunk = 256;  // ranks looked at at once: a workgroup has at most 256 lanes
constexpr uint32_t kGsaMaxWaves = 4;
// header words
constexpr uint32_t kGsaHdrBad = 0, kGsaHdrTotal = 1, kGsaHdrCost = 2, kGsaHdrWorst = 3, kGsaHdrSum = 4;  // (the f64 sum takes words 4 and 5)

__host__ __device__ __forceinline__ size_t gsa_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

struct GsaLds {
    uint32_t *hdr, *wsum, *live, *slots, *slot_len;
    float *E;
    uint16_t *cur, *inv;
    __device__ GsaLds(unsigned char *smem, uint32_t n)
    {
        hdr = reinterpret_cast<uint32_t *>(smem);
        wsum = hdr + 16;                              // 2 parities x 8
        live = hdr + 32;                              // kGsaLiveChunk words: j | n_swaps << 16
        slots = live + kGsaLiveChunk;                 // kGsaMaxWaves x kGsaMaxPull pairs
        slot_len = slots + kGsaMaxWaves * kGsaMaxPull;  // kGsaMaxWaves words
        const size_t wd = gsa_up16((size_t)n * 4), sh = gsa_up16((size_t)n * 2);
        unsigned char *p = smem + kGsaFixedBytes;
        E = reinterpret_cast<float *>(p);
        cur = reinterpret_cast<uint16_t *>(p + wd);
        inv = reinterpret_cast<uint16_t *>(p + wd + sh);
    }
};
static_assert((32 + kGsaLiveChunk + kGsaMaxWaves * kGsaMaxPull + kGsaMaxWaves) * 4 <= kGsaFixedBytes, "the fixed part of the LDS holds its tables");

// the tour in L.cur to dst, its edge lengths by all lanes and its cost by one, to every lane.  Begins behind a barrier (L.cur is
// whole), ends behind one: dst is whole for every lane of the workgroup.
template <bool DM>
__device__ float gsa_write_and_cost(const GsaLds &L, const CityDist<DM> &D, uint32_t n, uint16_t *dst)
{
    write_and_cost<DM>(L.cur, L.E, D, n, dst, reinterpret_cast<float *>(L.hdr + kGsaHdrCost));
    return __builtin_bit_cast(float, L.hdr[kGsaHdrCost]);
}

// One pull by one wave: the first `want` (<= kGsaMaxPull) pairs of swap_sequence(from, target), `inv` the inverse of `from` in
// LDS, into slot[0 .. ) in ascending position; how many there are (the sequence may be shorter), to every lane of the wave.
__device__ uint32_t gsa_pull(const uint16_t *inv, const uint16_t *target, uint32_t n, uint32_t want, uint32_t *slot)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t cnt = 0;
    for (uint32_t p0 = 0; p0 < n && cnt < want; p0 += 64u) {  // (cnt is the same on every lane of the wave)
        const uint32_t p = p0 + lane;
        bool has = false;
        uint32_t q = 0;
        if (p < n) {
            q = inv[target[p]];
            for (uint32_t steps = 0; q < p && steps < n; ++steps) q = inv[target[q]];  // (a permutation comes back to p within its cycle: the bound is never met)
            has = q > p;
        }
        const uint64_t b = __ballot(has);
        const uint32_t at = cnt + (uint32_t)__popcll(b & below);
        if (has && at < want) slot[at] = pso_swap(p, q);
        cnt += (uint32_t)__popcll(b);
    }
    return cnt < want ? cnt : want;
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_gsa_init(GsaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, ind = blockIdx.x, run = blockIdx.y;
    const GsaLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    const bool given = ind == 0u && A.init != nullptr;
    uint16_t *r = L.cur;
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
    const size_t idx = (size_t)run * A.agents + ind;
    const float c = gsa_write_and_cost<DM>(L, D, n, A.pos + idx * n);
    if (tid == 0) A.cost[idx] = c;
}

// gbest of the start: a copy of the FIRST minimum agent (min_by keeps the first of equals; its partial_cmp(..).unwrap() panics on
// a NaN cost)
__global__ __launch_bounds__(256) void k_gsa_first(GsaArgs A)
{
    __shared__ uint32_t pick;
    const uint32_t n = A.n, N = A.agents, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const float *pc = A.cost + (size_t)run * N;
    if (tid == 0) {
        uint32_t b = 0, nan = pc[0] != pc[0] ? 1u : 0u;
        float best = pc[0];
        for (uint32_t i = 1; i < N; ++i) {
            if (pc[i] != pc[i]) nan = 1u;
            if (pc[i] < best) {
                best = pc[i];
                b = i;
            }
        }
        pick = b;
        A.state[8u * (size_t)run] = __builtin_bit_cast(uint32_t, best);
        A.state[8u * (size_t)run + 1u] = 0u;
        A.state[8u * (size_t)run + 2u] = nan;
        if (A.last) A.out_cost[run] = best;
    }
    TL_SYNC();
    const uint32_t b = pick;
    const uint16_t *src = A.pos + ((size_t)run * N + b) * n;
    for (uint32_t k = tid; k < n; k += nt) {
        A.gbest[(size_t)run * n + k] = src[k];
        if (A.last) A.out_pos[(size_t)run * n + k] = src[k];
    }
    if (run == 0u) log_improvement(A, 0u, 0xFFFFFFFFu, b, pc[b], src);
}

template <bool DM>
__global__ __launch_bounds__(256) void k_gsa_epochs(GsaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, N = A.agents, kb = gsa_kbest(N), tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, nw = nt >> 6;
    const GsaLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    uint32_t *state = A.state + 8u * (size_t)run;
    if (state[2]) return;  // the reference has panicked (every lane reads the same word)
    float gcost = __builtin_bit_cast(float, state[0]);
    uint32_t improved = state[1];
    uint16_t *gbest = A.gbest + (size_t)run * n;
    float *cost = A.cost + (size_t)run * N;
    double *mass = A.mass + (size_t)run * N;
    uint16_t *kbest = A.kbest + (size_t)run * N;
    uint32_t par = 0;
    if (tid == 0) L.hdr[kGsaHdrBad] = 0u;
    for (uint32_t e = A.e0; e < A.e1; ++e) {  // (every condition below is the same on every lane: the barriers are met by all)
        uint32_t *erow = A.epoch_log && run == 0u && e < A.epoch_cap ? A.epoch_log + (size_t)e * (3u * N + 2u) : nullptr;
        // the masses and the ranking, from the costs at the epoch's start
        if (tid == 0) {
            const float worst = gsa_worst(cost, N);
            const double sum = gsa_sum_fitness(cost, N, worst);
            L.hdr[kGsaHdrWorst] = __builtin_bit_cast(uint32_t, worst);
            *reinterpret_cast<double *>(L.hdr + kGsaHdrSum) = sum;
        }
        TL_SYNC();
        {
            const float worst = __builtin_bit_cast(float, L.hdr[kGsaHdrWorst]);
            const double sum = *reinterpret_cast<const double *>(L.hdr + kGsaHdrSum);
            for (uint32_t a = tid; a < N; a += nt) {
                const double m = gsa_mass(cost[a], worst, sum, N);
                mass[a] = m;
                if (m != m) L.hdr[kGsaHdrBad] = 1u;  // (every writer writes the same word)
            }
        }
        TL_SYNC();
        if (L.hdr[kGsaHdrBad]) {  // partial_cmp(..).unwrap() of the ranking panics
            if (tid == 0) {
                state[0] = __builtin_bit_cast(uint32_t, gcost);
                state[1] = improved;
                state[2] = 1u;
            }
            return;
        }
        for (uint32_t a = tid; a < N; a += nt) kbest[gsa_rank(mass, N, a)] = (uint16_t)a;
        TL_SYNC();
        const double g = gsa_g(e, A.epochs);
        if (erow && tid == 0) {
            const uint64_t gb = __builtin_bit_cast(uint64_t, g);
            erow[3u * N] = (uint32_t)gb;
            erow[3u * N + 1u] = (uint32_t)(gb >> 32);
        }
        for (uint32_t i = 0; i < N; ++i) {
            uint16_t *pi = A.pos + ((size_t)run * N + i) * n;
            for (uint32_t p = tid; p < n; p += nt) {
                const uint16_t c = pi[p];
                L.cur[p] = c;
                L.inv[c] = (uint16_t)p;
            }
            if (tid == 0) L.hdr[kGsaHdrTotal] = gsa_inertia_keep(0u);  // nothing of the old velocity is kept: its length is not even stored
            TL_SYNC();
            uint32_t total = L.hdr[kGsaHdrTotal], live_pulls = 0;
            for (uint32_t r0 = 0; r0 < kb; r0 += kGsaLiveChunk) {
                // the live pulls among the ranks r0 .. r0 + 255, in rank order
                uint32_t found = 0;  // live pulls of this chunk so far
                for (uint32_t rr = r0; rr < kb && rr < r0 + kGsaLiveChunk; rr += nt) {
                    const uint32_t rank = rr + tid;
                    uint32_t j = 0, m = 0;
                    if (rank < kb && rank < r0 + kGsaLiveChunk) {
                        j = kbest[rank];
                        if (j != i) m = gsa_pull_swaps(gsa_r(key, e, N, i, j), g, mass[j]);
                    }
                    const bool has = m != 0u;
                    const uint64_t b = __ballot(has), below = (1ull << lane) - 1ull;
                    uint32_t *ws = L.wsum + par * 8u;
                    if (lane == 0u) ws[wave] = (uint32_t)__popcll(b);
                    TL_SYNC();
                    uint32_t off = found, tot = 0;
                    for (uint32_t w = 0; w < nw; ++w) {
                        const uint32_t a = ws[w];
                        if (w < wave) off += a;
                        tot += a;
                    }
                    if (has) L.live[off + (uint32_t)__popcll(b & below)] = j | (m << 16);
                    found += tot;
                    par ^= 1u;
                }
                TL_SYNC();
                live_pulls += found;
                // a wave per live pull, nw at a time; one lane applies them in order
                for (uint32_t b0 = 0; b0 < found && total < A.vmax; b0 += nw) {
                    const uint32_t b = b0 + wave;
                    if (b < found) {
                        const uint32_t word = L.live[b], j = word & 0xFFFFu, m = word >> 16;
                        const uint32_t got = gsa_pull(L.inv, A.pos + ((size_t)run * N + j) * n, n, m < kGsaMaxPull ? m : kGsaMaxPull, L.slots + wave * kGsaMaxPull);
                        if (lane == 0u) L.slot_len[wave] = got;
                    }
                    TL_SYNC();
                    if (tid == 0) {  // apply_swaps (route.rs:137-143) in order — swaps may share positions
                        uint32_t t = total;
                        for (uint32_t w = 0; w < nw && b0 + w < found; ++w) {
                            const uint32_t len = L.slot_len[w];
                            for (uint32_t k = 0; k < len && t < A.vmax; ++k, ++t) {
                                const uint32_t s = L.slots[w * kGsaMaxPull + k], a = s & 0xFFFFu, c = s >> 16;
                                if (a < n && c < n) {
                                    const uint16_t x = L.cur[a];
                                    L.cur[a] = L.cur[c];
                                    L.cur[c] = x;
                                }
                            }
                        }
                        L.hdr[kGsaHdrTotal] = t;
                    }
                    TL_SYNC();
                    total = L.hdr[kGsaHdrTotal];
                }
            }
            const float c = gsa_write_and_cost<DM>(L, D, n, pi);  // (ends behind a barrier: positions[i] is whole before the next agent reads it)
            if (tid == 0) cost[i] = c;  // (the masses of this epoch are already built)
            if (erow && tid == 0) {
                erow[i] = __builtin_bit_cast(uint32_t, c);
                erow[N + i] = total;
                erow[2u * N + i] = live_pulls;
            }
            if (c < gcost) {
                for (uint32_t p = tid; p < n; p += nt) gbest[p] = L.cur[p];
                ++improved;
                if (run == 0u) log_improvement(A, improved, e, i, c, pi);
                gcost = c;
            }
        }
    }
    TL_SYNC();
    if (tid == 0) {
        state[0] = __builtin_bit_cast(uint32_t, gcost);
        state[1] = improved;
        if (A.last) A.out_cost[run] = gcost;
    }
    if (A.last) {
        for (uint32_t p = tid; p < n; p += nt) A.out_pos[(size_t)run * n + p] = gbest[p];
    }
}

// the device's pull on given (from, target, prefix length) tuples (tl_gsa_selftest_pull): one workgroup per tuple, its wave 0 the
// pull, as k_gsa_epochs has it
__global__ __launch_bounds__(256) void k_gsa_selftest_pull(const uint16_t *from, const uint16_t *target, const uint32_t *want, uint32_t n, uint32_t *out_pairs,
                                                           uint32_t *out_len)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const GsaLds L(smem, n);
    const size_t at = (size_t)blockIdx.x * n;
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) L.inv[from[at + p]] = (uint16_t)p;
    TL_SYNC();
    if ((threadIdx.x >> 6) == 0u) {
        const uint32_t m = want[blockIdx.x] < kGsaMaxPull ? want[blockIdx.x] : kGsaMaxPull;
        const uint32_t got = gsa_pull(L.inv, target + at, n, m, L.slots);
        if (threadIdx.x == 0) {
            L.slot_len[0] = got;
            out_len[blockIdx.x] = got;
        }
    }
    TL_SYNC();
    const uint32_t got = L.slot_len[0];
    for (uint32_t k = threadIdx.x; k < kGsaMaxPull; k += blockDim.x) out_pairs[(size_t)blockIdx.x * kGsaMaxPull + k] = k < got ? L.slots[k] : 0xFFFFFFFFu;
}

size_t gravitational_search_lds_bytes(uint32_t n) { return kGsaFixedBytes + gsa_up16((size_t)n * 4) + 2 * gsa_up16((size_t)n * 2); }

uint32_t gravitational_search_max_n(int lds_budget)
{
    if (lds_budget <= 0) return 0u;
    uint64_t m = (uint64_t)lds_budget / 8u;
    if (m > 0xFFFFu) m = 0xFFFFu;  // (cities and the positions of a pair are 16 bits wide)
    while (m > 0u && gravitational_search_lds_bytes((uint32_t)m) > (size_t)lds_budget) --m;
    return (uint32_t)m;
}

int gravitational_search_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 64u ? 64 : t > 256u ? 256 : (int)t;
}

hipError_t launch_gsa_init(const GsaArgs &A, uint32_t runs, hipStream_t s)
{
    hipError_t e = launch_max_lds(A.dm_full ? k_gsa_init<true> : k_gsa_init<false>, dim3(A.agents, runs), gravitational_search_threads(A.n),
                              gravitational_search_lds_bytes(A.n), s, A);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gsa_first, dim3(runs), dim3(gravitational_search_threads(A.n)), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_gsa_epochs(const GsaArgs &A, uint32_t runs, hipStream_t s)
{
    // a workgroup of four waves whatever n: the ranking and the pulls are spread over the agents, not over the cities
    return launch_max_lds(A.dm_full ? k_gsa_epochs<true> : k_gsa_epochs<false>, dim3(runs), 256, gravitational_search_lds_bytes(A.n), s, A);
}

hipError_t launch_gsa_selftest_pull(const uint16_t *from, const uint16_t *to, const uint32_t *want, uint32_t n, uint32_t count, uint32_t *out_pairs,
                                    uint32_t *out_len, hipStream_t s)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_gsa_selftest_pull));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gsa_selftest_pull, dim3(count), dim3(gravitational_search_threads(n)), gravitational_search_lds_bytes(n), s, from, to, want, n, out_pairs,
                       out_len);
    return hipGetLastError();
}

}  // namespace tl
