// genetic.hip — the genetic algorithm (genetic_algorithm.rs:16-336): R independent runs, the run a grid dimension, the populations
// (16-bit cities) in the context's workspace, two launches per generation.
//
// The draws of pair p of generation g are a pure function of (seed, run, g, p) (ga_spec.h: this project's specification — the
// reference draws from an unseeded thread RNG), so once a generation is ranked all its pairs are known and are bred at once.
//
//   k_ga_init   one workgroup per (individual, run): the start population.  The Fisher-Yates pass (or the 2 .. 4 mutations of a seeded
//               individual) is one lane's work in LDS; the edge lengths are computed by all lanes and summed by one, in the
//               reference's order (closing edge first).
//   k_ga_rank   one workgroup per run: the stable descending rank of every individual by counting (#{j : f_j > f_i or f_j = f_i and
//               j < i}, the fitness values in LDS, one thread per individual), the roulette prefix — a SEQUENTIAL f32 sum by
//               definition, n dependent adds by one lane — and, by a lane of another wave meanwhile, the population's best (the
//               last of equal maxima), its recomputed tour_length and the trace record.
//   k_ga_breed  one workgroup per elite (a copy) or per pair: both parents by binary search over the prefix, the two segments'
//               cities marked in LDS flags, both children built by a ballot/popcount compaction over the n positions in rotated
//               order (the parallel form of the reference's loop), the edge lengths in parallel, the two sums by one lane each (of
//               two waves, at once), fitness by IEEE division, and the mutation applied to the stored genotype only.
//
//   LDS of a workgroup: 384 bytes of header and wave counts | E1[n], E2[n] f32 | c1[n], c2[n] u16 | fa[n], fb[n] u8 (14 n bytes).
#include "swarm_tour.h"
#include "ga_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kGaFixedBytes = 384;  // header (16 words), then the wave counts (2 parities x 2 children x 16 waves)

__device__ __forceinline__ size_t ga_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

struct GaLds {
    uint32_t *hdr, *wsum;
    float *E1, *E2;
    uint16_t *c1, *c2;
    uint8_t *fa, *fb;
    __device__ GaLds(unsigned char *smem, uint32_t n)
    {
        hdr = reinterpret_cast<uint32_t *>(smem);
        wsum = hdr + 16;
        const size_t fl = ga_up16((size_t)n * 4), sh = ga_up16((size_t)n * 2);
        unsigned char *p = smem + kGaFixedBytes;
        E1 = reinterpret_cast<float *>(p);
        E2 = reinterpret_cast<float *>(p + fl);
        c1 = reinterpret_cast<uint16_t *>(p + 2 * fl);
        c2 = reinterpret_cast<uint16_t *>(p + 2 * fl + sh);
        fa = p + 2 * fl + 2 * sh;
        fb = fa + ga_up16(n);
    }
};

__device__ __forceinline__ float ga_fitness(float len) { return len == 0.0f ? 0.0f : 1.0f / len; }

// ordered_crossover_genes (genetic_algorithm.rs:140-177) by the whole workgroup: c1, c2 in LDS.  Ends behind a barrier.
__device__ void ga_crossover(const uint16_t *p1, const uint16_t *p2, uint32_t n, uint32_t from, uint32_t to, const GaLds &L)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, nw = nt >> 6;
    for (uint32_t k = tid; k < n; k += nt) {
        L.fa[k] = 0;
        L.fb[k] = 0;
    }
    TL_SYNC();
    for (uint32_t k = from + tid; k <= to; k += nt) {
        const uint16_t a = p1[k], b = p2[k];
        L.fa[a] = 1;
        L.fb[b] = 1;
        L.c1[k] = b;
        L.c2[k] = a;
    }
    TL_SYNC();
    uint32_t base1 = 0, base2 = 0, par = 0;
    const uint32_t start = to + 1u;  // <= n
    for (uint32_t t0 = 0; t0 < n; t0 += nt) {
        const uint32_t t = t0 + tid;
        const bool live = t < n;
        uint32_t k = start + t;      // < 2 n
        if (k >= n) k -= n;
        if (!live) k = 0;
        const uint16_t x1 = p1[k], x2 = p2[k];
        const bool keep1 = live && !L.fb[x1], keep2 = live && !L.fa[x2];
        const uint64_t b1 = __ballot(keep1), b2 = __ballot(keep2), below = (1ull << lane) - 1ull;
        uint32_t *ws = L.wsum + par * 32u;
        if (lane == 0u) {
            ws[wave] = (uint32_t)__popcll(b1);
            ws[16u + wave] = (uint32_t)__popcll(b2);
        }
        TL_SYNC();
        uint32_t o1 = base1, o2 = base2, tot1 = 0, tot2 = 0;
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t a = ws[w], b = ws[16u + w];
            if (w < wave) {
                o1 += a;
                o2 += b;
            }
            tot1 += a;
            tot2 += b;
        }
        if (keep1) {
            uint32_t j = start + o1 + (uint32_t)__popcll(b1 & below);
            if (j >= n) j -= n;
            L.c1[j] = x1;
        }
        if (keep2) {
            uint32_t j = start + o2 + (uint32_t)__popcll(b2 & below);
            if (j >= n) j -= n;
            L.c2[j] = x2;
        }
        base1 += tot1;
        base2 += tot2;
        par ^= 1u;
    }
    TL_SYNC();
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_ga_init(GaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, ind = blockIdx.x, run = blockIdx.y;
    const GaLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    const uint32_t n_seeded = A.init ? (n / 5u > 1u ? n / 5u : 1u) : 0u;
    uint16_t *r = L.c1;
    if (ind < n_seeded) {
        for (uint32_t k = tid; k < n; k += nt) r[k] = (uint16_t)A.init[k];
    } else {
        for (uint32_t k = tid; k < n; k += nt) r[k] = (uint16_t)k;
    }
    TL_SYNC();
    if (tid == 0) {
        if (ind < n_seeded) {
            if (ind > 0u) {  // (n >= 10)
                const uint32_t count = 2u + sa_position(ga_draw_key(key, ga_init_event(n, ind, 0), kGaSlotCount), 3u);
                for (uint32_t m = 0; m < count; ++m) {
                    uint32_t f, t;
                    ga_pair(key, ga_init_event(n, ind, 1u + m), n, &f, &t);
                    while (f < t) {
                        const uint16_t x = r[f];
                        r[f++] = r[t];
                        r[t--] = x;
                    }
                }
            }
        } else {
            for (uint32_t j = n - 1u; j >= 1u && j < n; --j) {
                const uint32_t k = sa_position(ga_draw_key(key, ga_init_event(n, ind, j), kGaSlotShuffle), j + 1u);
                const uint16_t x = r[j];
                r[j] = r[k];
                r[k] = x;
            }
        }
    }
    TL_SYNC();
    uint16_t *dst = A.pop[0] + (size_t)run * A.pop_stride + (size_t)ind * n;
    for (uint32_t k = tid; k < n; k += nt) {
        dst[k] = r[k];
        L.E1[k] = D(r[k], r[k + 1u == n ? 0u : k + 1u]);
    }
    TL_SYNC();
    if (tid == 0) A.fit[0][(size_t)run * n + ind] = ga_fitness(sum_edges(L.E1, n));
}

// state words of a run: 0 best fitness bits of the population ranked last, 1 generations whose best improved, 2 mutations applied,
// 3 status (1: the reference panics in random_selection), 4 best index
template <bool DM>
__global__ __launch_bounds__(1024) void k_ga_rank(GaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, len = A.len, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x, gen = A.generation;
    uint32_t *hdr = reinterpret_cast<uint32_t *>(smem);
    float *f = reinterpret_cast<float *>(smem + 256);
    float *sf = f + ((len + 3u) & ~3u);
    float *E = sf + ((len + 3u) & ~3u);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const float *fit = A.fit[A.src] + (size_t)run * n;
    const uint16_t *pop = A.pop[A.src] + (size_t)run * A.pop_stride;
    uint32_t *order = A.order + (size_t)run * n;
    uint32_t *state = A.state + 8u * (size_t)run;
    const bool select = !A.last && ga_pairs(n, A.n_elite) > 0u;  // a roulette follows
    const bool logged = A.log && run == 0u && gen >= 1u && gen - 1u < A.log_cap;
    const bool routed = A.route_log && run == 0u && gen >= 1u && gen - 1u < A.route_cap;

    for (uint32_t i = tid; i < len; i += nt) f[i] = fit[i];
    if (tid == 0) hdr[0] = 0u;
    TL_SYNC();
    for (uint32_t i = tid; i < len; i += nt) {
        const float fi = f[i];
        uint32_t gt = 0, eq_before = 0, eq_after = 0;
        for (uint32_t j = 0; j < len; ++j) {
            const float fj = f[j];
            gt += fj > fi;
            eq_before += fj == fi && j < i;
            eq_after += fj == fi && j > i;
        }
        const uint32_t rank = gt + eq_before;
        order[rank] = i;
        sf[rank] = fi;
        if (gt + eq_after == 0u) hdr[0] = i;  // best(): the last of equal maxima (exactly one i)
    }
    TL_SYNC();
    const uint32_t b = hdr[0] < len ? hdr[0] : len - 1u;  // (a NaN fitness — coordinates that are not finite — ranks nowhere: stay inside)
    const uint16_t *best = pop + (size_t)b * n;
    if (logged || A.last) {
        for (uint32_t k = tid; k < n; k += nt) E[k] = D(best[k], best[k + 1u == n ? 0u : k + 1u]);
    }
    if (routed) {
        uint32_t *dst = A.route_log + (size_t)(gen - 1u) * n;
        for (uint32_t k = tid; k < n; k += nt) dst[k] = best[k];
    }
    if (A.last) {
        uint32_t *dst = A.out_pos + (size_t)run * n;
        for (uint32_t k = tid; k < n; k += nt) dst[k] = best[k];
    }
    TL_SYNC();
    if (tid == 0 && select) {
        float *prefix = A.prefix + (size_t)run * (n + 1u);
        float tot = 0.0f;
        prefix[0] = tot;
        for (uint32_t i = 0; i < len; ++i) {
            tot += sf[i];
            prefix[i + 1u] = tot;
        }
        if (!(tot > 0.0f) || tot > 3.4028234663852886e38f) state[3] = 1u;  // an empty range: random_selection panics
    }
    if (tid == 64u) {
        const float bf = f[b];
        if (gen >= 1u && bf > __builtin_bit_cast(float, state[0])) ++state[1];
        state[0] = __builtin_bit_cast(uint32_t, bf);
        state[4] = b;
        if (logged || A.last) {
            const float cost = sum_edges(E, n);
            if (logged) {
                uint32_t *rec = A.log + 4u * (size_t)(gen - 1u);
                rec[0] = b;
                rec[1] = __builtin_bit_cast(uint32_t, bf);
                rec[2] = __builtin_bit_cast(uint32_t, cost);
                rec[3] = len;
            }
            if (A.last) A.out_cost[run] = cost;
        }
    }
}

template <bool DM>
__global__ __launch_bounds__(256) void k_ga_breed(GaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, len = A.len, tid = threadIdx.x, nt = blockDim.x, slot = blockIdx.x, run = blockIdx.y;
    const uint32_t ne = A.n_elite < len ? A.n_elite : len;
    const uint16_t *src = A.pop[A.src] + (size_t)run * A.pop_stride;
    uint16_t *dst = A.pop[A.src ^ 1u] + (size_t)run * A.pop_stride;
    const float *sfit = A.fit[A.src] + (size_t)run * n;
    float *dfit = A.fit[A.src ^ 1u] + (size_t)run * n;
    const uint32_t *order = A.order + (size_t)run * n;
    if (slot < ne) {  // an elite: the slot-th of the sorted population, as it is
        const uint32_t i = order[slot] < len ? order[slot] : len - 1u;
        for (uint32_t k = tid; k < n; k += nt) dst[(size_t)slot * n + k] = src[(size_t)i * n + k];
        if (tid == 0) dfit[slot] = sfit[i];
        return;
    }
    const GaLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint32_t p = slot - ne;
    if (tid == 0) {
        const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
        const uint64_t ev = ga_pair_event(A.generation, n, p, 0);
        const float *prefix = A.prefix + (size_t)run * (n + 1u);
        const float total = prefix[len];
        uint32_t from, to;
        ga_pair(key, ev, n, &from, &to);
        L.hdr[0] = from;
        L.hdr[1] = to;
        for (uint32_t k = 0; k < 2u; ++k) {
            const float r = ga_uniform(ga_draw_key(key, ev, kGaSlotSelect + k)) * total;
            const uint32_t w = order[ga_select(prefix, len, r)];
            L.hdr[2u + k] = w < len ? w : len - 1u;
            const bool mutate = A.p_mut > ga_uniform(ga_draw_key(key, ev, kGaSlotMutate + k));
            uint32_t mf = 0, mt = 0;
            if (mutate) ga_pair(key, ga_pair_event(A.generation, n, p, 1u + k), n, &mf, &mt);
            L.hdr[4u + 3u * k] = mutate ? 1u : 0u;
            L.hdr[5u + 3u * k] = mf;
            L.hdr[6u + 3u * k] = mt;
        }
        if (L.hdr[4] + L.hdr[7]) atomicAdd(A.state + 8u * (size_t)run + 2u, L.hdr[4] + L.hdr[7]);
    }
    TL_SYNC();
    const uint32_t from = L.hdr[0], to = L.hdr[1];
    const uint16_t *p1 = src + (size_t)L.hdr[2] * n, *p2 = src + (size_t)L.hdr[3] * n;
    ga_crossover(p1, p2, n, from, to, L);
    for (uint32_t k = tid; k < n; k += nt) {
        const uint32_t k1 = k + 1u == n ? 0u : k + 1u;
        L.E1[k] = D(L.c1[k], L.c1[k1]);
        L.E2[k] = D(L.c2[k], L.c2[k1]);
    }
    TL_SYNC();
    const uint32_t s1 = ne + 2u * p, s2 = s1 + 1u;  // (add, genetic_algorithm.rs:239-243, keeps no more than n; never reached: 2 (n / 2) <= n)
    if (tid == 0 && s1 < n) dfit[s1] = ga_fitness(sum_edges(L.E1, n));
    if (tid == 64u && s2 < n) dfit[s2] = ga_fitness(sum_edges(L.E2, n));
    // mutate (genetic_algorithm.rs:327-335) on the stored genotype: the fitness above stays
    const uint32_t m1 = L.hdr[4], f1 = L.hdr[5], t1 = L.hdr[6], m2 = L.hdr[7], f2 = L.hdr[8], t2 = L.hdr[9];
    for (uint32_t k = tid; k < n; k += nt) {
        if (s1 < n) dst[(size_t)s1 * n + k] = L.c1[m1 && k >= f1 && k <= t1 ? f1 + t1 - k : k];
        if (s2 < n) dst[(size_t)s2 * n + k] = L.c2[m2 && k >= f2 && k <= t2 ? f2 + t2 - k : k];
    }
}

// the device crossover on given parents (tl_ga_selftest_crossover)
__global__ __launch_bounds__(256) void k_ga_selftest_crossover(const uint16_t *p1, const uint16_t *p2, uint32_t n, uint32_t from, uint32_t to, uint16_t *out1,
                                                               uint16_t *out2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const GaLds L(smem, n);
    ga_crossover(p1, p2, n, from, to, L);
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        out1[k] = L.c1[k];
        out2[k] = L.c2[k];
    }
}

size_t genetic_lds_bytes(uint32_t n) { return (size_t)n * 14 + 6 * 16 + kGaFixedBytes; }

uint32_t genetic_max_n(int lds_budget)
{
    const size_t fixed = 6 * 16 + kGaFixedBytes;
    if ((size_t)lds_budget <= fixed) return 0u;
    const size_t m = ((size_t)lds_budget - fixed) / 14;
    return m > 0xFFFFu ? 0xFFFFu : (uint32_t)m;  // (the populations' entries are 16 bits wide)
}

int genetic_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 128u ? 128 : t > 256u ? 256 : (int)t;  // at least two waves: the two children's sums run on one lane each
}

template <class K>
static hipError_t ga_launch(K kern, dim3 grid, int threads, size_t lds, hipStream_t s, const GaArgs &A)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, A);
    return hipGetLastError();
}

hipError_t launch_ga_init(const GaArgs &A, uint32_t runs, hipStream_t s)
{
    return ga_launch(A.dm_full ? k_ga_init<true> : k_ga_init<false>, dim3(A.n, runs), genetic_threads(A.n), genetic_lds_bytes(A.n), s, A);
}

hipError_t launch_ga_rank(const GaArgs &A, uint32_t runs, hipStream_t s)
{
    uint32_t t = (A.len + 63u) & ~63u;
    t = t < 128u ? 128u : t > 1024u ? 1024u : t;
    const size_t lds = 256 + 2 * (size_t)((A.len + 3u) & ~3u) * 4 + (size_t)A.n * 4 + 16;  // <= genetic_lds_bytes(n): len <= n
    return ga_launch(A.dm_full ? k_ga_rank<true> : k_ga_rank<false>, dim3(runs), (int)t, lds, s, A);
}

hipError_t launch_ga_breed(const GaArgs &A, uint32_t runs, uint32_t next_len, hipStream_t s)
{
    const uint32_t ne = A.n_elite < A.len ? A.n_elite : A.len;
    const uint32_t blocks = ne + (next_len - ne) / 2u;
    if (blocks == 0u) return hipSuccess;
    return ga_launch(A.dm_full ? k_ga_breed<true> : k_ga_breed<false>, dim3(blocks, runs), genetic_threads(A.n), genetic_lds_bytes(A.n), s, A);
}

hipError_t launch_ga_selftest_crossover(const uint16_t *p1, const uint16_t *p2, uint32_t n, uint32_t from, uint32_t to, uint16_t *out1, uint16_t *out2,
                                        hipStream_t s)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_ga_selftest_crossover));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ga_selftest_crossover, dim3(1), dim3(genetic_threads(n)), genetic_lds_bytes(n), s, p1, p2, n, from, to, out1, out2);
    return hipGetLastError();
}

}  // namespace tl
