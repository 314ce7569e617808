// cuckoo_search.hip — the cuckoo search solver (cuckoo_search.rs:26-136): R independent runs, the run a grid dimension, the nests
// (16-bit cities), a staged flight per cuckoo, a staged replacement per nest and the costs in the context's workspace, two launches
// per epoch.
//
// The draws of cuckoo c and nest c of epoch e are a pure function of (seed, run, e, c) (cs_spec.h: this project's specification —
// the reference draws from an unseeded thread RNG): the Lévy length, the k reversals, the target nest, the abandonment trial and
// the replacement's shuffle.  A flight reads its own nest alone, so every flight of an epoch is built at once from the epoch-start
// nests, and so is every replacement whose trial succeeds.  The commit then walks the cuckoos in order: a cuckoo whose nest an
// earlier flight of the epoch has overwritten flies AGAIN, inside the commit's workgroup, from the nest as it stands — the
// reference's order, without a host round trip.  Late epochs accept little, so the second flight is rare.
//
//   k_cs_init    one workgroup per (nest, run): the start nest (the initial tour, or a Fisher-Yates pass by one lane in LDS), its
//                edge lengths by all lanes and their sum by one, in the reference's order (closing edge first).
//   k_cs_first   one workgroup per run: best is a copy of the FIRST minimum nest.
//   k_cs_fly     one workgroup per (cuckoo, run): cs_fly; and one per (nest, run) that leaves at once unless the nest's
//                abandonment trial succeeds: the init body on the epoch's shuffle events.
//   k_cs_commit  one workgroup per run: the target test, the copy and the best rule in cuckoo order, cs_fly again where the
//                source nest has changed; then the abandonments in nest order; the log.
//
// cs_fly: k from the Lévy step (every lane computes it: the same instructions as one lane would take); the k pairs (i, j) into
// LDS, one lane per reversal; the nest into LDS; then the k reversals AS A GATHER — a lane owns output positions p, p + T, .. and
// follows each back through the reversals from the last to the first, q = (i_r <= q <= j_r) ? i_r + j_r - q : q (a reversal is its
// own inverse, so this is where the literal loop's element at p came from; cs_spec.h: cs_source_position), new[p] = old[q].  No
// barrier and no LDS write inside the walk; the pair reads are broadcasts.  Then the edge lengths in parallel and their sum by one
// lane.
//
//   LDS of a workgroup: 576 bytes of header and the commit's "overwritten" bits | pairs[n / 2] u32 | E[n] f32 | old[n], new[n] u16
//   (10 n bytes).
#include "swarm_tour.h"
#include "cs_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kCsFixedBytes = 576;  // header (16 words), then one bit per nest (128 words)

__host__ __device__ __forceinline__ size_t cs_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

struct CsLds {
    uint32_t *hdr, *touched, *pairs;
    float *E;
    uint16_t *old, *neu;
    __device__ CsLds(unsigned char *smem, uint32_t n)
    {
        hdr = reinterpret_cast<uint32_t *>(smem);
        touched = hdr + 16;
        const size_t pr = cs_up16((size_t)(n / 2u) * 4), wd = cs_up16((size_t)n * 4), sh = cs_up16((size_t)n * 2);
        unsigned char *p = smem + kCsFixedBytes;
        pairs = reinterpret_cast<uint32_t *>(p);
        E = reinterpret_cast<float *>(p + pr);
        old = reinterpret_cast<uint16_t *>(p + pr + wd);
        neu = reinterpret_cast<uint16_t *>(p + pr + wd + sh);
    }
};

// a Fisher-Yates pass over city order by one lane in L.neu, step j drawing position(u(event0 + j, slot), j + 1).  Ends behind a
// barrier.
__device__ void cs_shuffle(const CsLds &L, uint32_t n, uint64_t key, uint64_t event0, uint32_t slot)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    uint16_t *r = L.neu;
    for (uint32_t k = tid; k < n; k += nt) r[k] = (uint16_t)k;
    TL_SYNC();
    if (tid == 0) {
        for (uint32_t j = n - 1u; j >= 1u && j < n; --j) {
            const uint32_t k = sa_position(ga_draw_key(key, event0 + j, slot), j + 1u);
            const uint16_t x = r[j];
            r[j] = r[k];
            r[k] = x;
        }
    }
    TL_SYNC();
}

// the gather of the reversals L.pairs[0 .. k) from L.old into L.neu.  Begins behind a barrier (pairs and old are whole), ends
// behind one.
__device__ void cs_gather(const CsLds &L, uint32_t n, uint32_t k)
{
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) L.neu[p] = L.old[cs_source_position(L.pairs, k, p)];
    TL_SYNC();
}

// One flight (cuckoo_search.rs:79-88) by the whole workgroup: from nest c as it stands to fly[c], fcost[c], fk[c].  Ends behind a
// barrier.
template <bool DM>
__device__ void cs_fly(const CsArgs &A, const CsLds &L, const CityDist<DM> &D, uint32_t run, uint32_t c, uint64_t key)
{
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x;
    const size_t idx = (size_t)run * A.nests + c;
    const uint64_t base = cs_base(A.epoch, A.nests, c, n);
    const uint32_t k = cs_flight_length(cs_levy(key, base), n);  // (<= n / 2: the pairs fit their block)
    const uint16_t *src = A.nest + idx * n;
    for (uint32_t r = tid; r < k; r += nt) {
        uint32_t i, j;
        cs_reversal(key, base, r, n, &i, &j);
        L.pairs[r] = i | (j << 16);
    }
    for (uint32_t p = tid; p < n; p += nt) L.old[p] = src[p];
    TL_SYNC();
    cs_gather(L, n, k);
    write_and_cost<DM>(L.neu, L.E, D, n, A.fly + idx * n, A.fcost + idx);
    if (tid == 0) A.fk[idx] = k;
}

struct CsGivenWords {
    const uint64_t *w;
    __device__ uint64_t operator()(uint32_t i) const { return w[i]; }
};

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_cs_init(CsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, ind = blockIdx.x, run = blockIdx.y;
    const CsLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    if (ind == 0u && A.init != nullptr) {
        const uint32_t *src = A.init + (size_t)run * A.init_stride;
        for (uint32_t k = tid; k < n; k += nt) L.neu[k] = (uint16_t)src[k];
        TL_SYNC();
    } else {
        cs_shuffle(L, n, key, ga_init_event(n, ind, 0u), kGaSlotShuffle);
    }
    const size_t idx = (size_t)run * A.nests + ind;
    write_and_cost<DM>(L.neu, L.E, D, n, A.nest + idx * n, A.cost + idx);
}

// best of the start: a copy of the FIRST minimum nest (min_by keeps the first of equals)
__global__ __launch_bounds__(256) void k_cs_first(CsArgs A)
{
    __shared__ uint32_t pick;
    const uint32_t n = A.n, N = A.nests, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const float *pc = A.cost + (size_t)run * N;
    if (tid == 0) {
        uint32_t b = 0;
        float best = pc[0];
        for (uint32_t i = 1; i < N; ++i) {
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
    const uint16_t *src = A.nest + ((size_t)run * N + b) * n;
    for (uint32_t k = tid; k < n; k += nt) {
        A.best[(size_t)run * n + k] = src[k];
        if (A.last) A.out_pos[(size_t)run * n + k] = src[k];
    }
    if (run == 0u) log_improvement(A, 0u, 0xFFFFFFFFu, b, pc[b], src);
}

template <bool DM>
__global__ __launch_bounds__(256) void k_cs_fly(CsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, N = A.nests, run = blockIdx.y;
    const CsLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    if (blockIdx.x < N) {
        cs_fly<DM>(A, L, D, run, blockIdx.x, key);
        return;
    }
    const uint32_t c = blockIdx.x - N;  // nest c's replacement, where its trial succeeds (the same verdict on every lane)
    const uint64_t base = cs_base(A.epoch, N, c, n);
    if (!cs_abandoned(key, base, A.pa)) return;
    cs_shuffle(L, n, key, base + 1u, kCsSlotReplace);
    const size_t idx = (size_t)run * N + c;
    write_and_cost<DM>(L.neu, L.E, D, n, A.repl + idx * n, A.rcost + idx);
}

template <bool DM>
__global__ __launch_bounds__(256) void k_cs_commit(CsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, N = A.nests, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const CsLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    uint32_t *state = A.state + 8u * (size_t)run;
    float best = __builtin_bit_cast(float, state[0]);
    uint32_t improved = state[1];
    uint16_t *bestr = A.best + (size_t)run * n;
    float *cost = A.cost + (size_t)run * N;
    const float *fcost = A.fcost + (size_t)run * N, *rcost = A.rcost + (size_t)run * N;
    uint32_t *erow = A.epoch_log && run == 0u && A.epoch < A.epoch_cap ? A.epoch_log + (size_t)A.epoch * 4u * N : nullptr;
    for (uint32_t w = tid; w < (kCsMaxNests >> 5); w += nt) L.touched[w] = 0u;
    TL_SYNC();
    for (uint32_t c = 0; c < N; ++c) {  // (every condition below is the same on every lane: the barriers are met by all)
        const bool again = (L.touched[c >> 5] >> (c & 31u)) & 1u;  // an earlier flight of this epoch has overwritten nest c
        if (again) cs_fly<DM>(A, L, D, run, c, key);
        const uint32_t t = cs_target(key, cs_base(A.epoch, N, c, n), N);
        const float f = fcost[c];
        const bool acc = f < cost[t];
        if (erow && tid == 0) erow[2u * N + c] = t | (acc ? 1u << 31 : 0u) | (again ? 1u << 30 : 0u);
        if (acc) {
            const uint16_t *src = A.fly + ((size_t)run * N + c) * n;
            uint16_t *dst = A.nest + ((size_t)run * N + t) * n;
            for (uint32_t k = tid; k < n; k += nt) dst[k] = src[k];
            if (f < best) {
                for (uint32_t k = tid; k < n; k += nt) bestr[k] = src[k];
                ++improved;
                if (run == 0u) log_improvement(A, improved, A.epoch, c, f, src);
                best = f;
            }
            TL_SYNC();  // every lane has read cost[t]; nest t is whole before a later flight reads it
            if (tid == 0) {
                cost[t] = f;
                L.touched[t >> 5] |= 1u << (t & 31u);
            }
            TL_SYNC();
        }
    }
    for (uint32_t c = 0; c < N; ++c) {  // the abandonments, in nest order (cuckoo_search.rs:105-125): unconditional
        const bool ab = cs_abandoned(key, cs_base(A.epoch, N, c, n), A.pa);
        if (erow && tid == 0) erow[3u * N + c] = ab ? 1u : 0u;
        if (!ab) continue;
        const uint16_t *src = A.repl + ((size_t)run * N + c) * n;
        uint16_t *dst = A.nest + ((size_t)run * N + c) * n;
        for (uint32_t k = tid; k < n; k += nt) dst[k] = src[k];
        const float rc = rcost[c];
        if (rc < best) {
            for (uint32_t k = tid; k < n; k += nt) bestr[k] = src[k];
            ++improved;
            if (run == 0u) log_improvement(A, improved, A.epoch, N + c, rc, src);
            best = rc;
        }
        if (tid == 0) cost[c] = rc;
    }
    TL_SYNC();
    if (tid == 0) {
        state[0] = __builtin_bit_cast(uint32_t, best);
        state[1] = improved;
        if (A.last) A.out_cost[run] = best;
    }
    if (erow) {
        for (uint32_t i = tid; i < N; i += nt) {
            erow[i] = __builtin_bit_cast(uint32_t, cost[i]);
            erow[N + i] = A.fk[(size_t)run * N + i];
        }
    }
    if (A.last) {
        for (uint32_t k = tid; k < n; k += nt) A.out_pos[(size_t)run * n + k] = bestr[k];
    }
}

// the device's Lévy step and flight length on given word tuples (tl_cs_selftest_levy): one lane per tuple
__global__ __launch_bounds__(256) void k_cs_selftest_levy(const uint64_t *words, uint32_t count, uint32_t n, uint64_t *out_bits, uint32_t *out_k, uint32_t *out_resamples)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t tries = 0;
    const double v = levy_step(CsGivenWords{words + (size_t)i * kLevyWords}, &tries);
    out_bits[i] = __builtin_bit_cast(uint64_t, v);
    out_k[i] = cs_flight_length(fabs(v), n);
    out_resamples[i] = tries;
}

// the device's gather on given tours and pair lists (tl_cs_selftest_reversals): one workgroup per tour
__global__ __launch_bounds__(256) void k_cs_selftest_reversals(const uint16_t *tours, const uint32_t *pairs, const uint32_t *lens, uint32_t n, uint32_t kcap,
                                                               uint16_t *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const CsLds L(smem, n);
    const uint32_t row = blockIdx.x, cap = kcap < n / 2u ? kcap : n / 2u, k = lens[row] < cap ? lens[row] : cap;
    for (uint32_t r = threadIdx.x; r < k; r += blockDim.x) L.pairs[r] = pairs[(size_t)row * kcap + r];
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) L.old[p] = tours[(size_t)row * n + p];
    TL_SYNC();
    cs_gather(L, n, k);
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) out[(size_t)row * n + p] = L.neu[p];
}

size_t cuckoo_search_lds_bytes(uint32_t n) { return kCsFixedBytes + cs_up16((size_t)(n / 2u) * 4) + cs_up16((size_t)n * 4) + 2 * cs_up16((size_t)n * 2); }

uint32_t cuckoo_search_max_n(int lds_budget)
{
    if (lds_budget <= 0) return 0u;
    uint64_t m = (uint64_t)lds_budget / 10u;
    if (m > 0xFFFFu) m = 0xFFFFu;  // (cities and the positions of a pair are 16 bits wide)
    while (m > 0u && cuckoo_search_lds_bytes((uint32_t)m) > (size_t)lds_budget) --m;
    return (uint32_t)m;
}

int cuckoo_search_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 64u ? 64 : t > 256u ? 256 : (int)t;
}

hipError_t launch_cs_init(const CsArgs &A, uint32_t runs, hipStream_t s)
{
    hipError_t e = launch_max_lds(A.dm_full ? k_cs_init<true> : k_cs_init<false>, dim3(A.nests, runs), cuckoo_search_threads(A.n), cuckoo_search_lds_bytes(A.n), s, A);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cs_first, dim3(runs), dim3(cuckoo_search_threads(A.n)), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_cs_fly(const CsArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_cs_fly<true> : k_cs_fly<false>, dim3(2u * A.nests, runs), cuckoo_search_threads(A.n), cuckoo_search_lds_bytes(A.n), s, A);
}

hipError_t launch_cs_commit(const CsArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_cs_commit<true> : k_cs_commit<false>, dim3(runs), cuckoo_search_threads(A.n), cuckoo_search_lds_bytes(A.n), s, A);
}

hipError_t launch_cs_selftest_levy(const uint64_t *words, uint32_t count, uint32_t n, uint64_t *out_bits, uint32_t *out_k, uint32_t *out_resamples, hipStream_t s)
{
    hipLaunchKernelGGL(k_cs_selftest_levy, dim3((count + 255u) / 256u), dim3(256), 0, s, words, count, n, out_bits, out_k, out_resamples);
    return hipGetLastError();
}

hipError_t launch_cs_selftest_reversals(const uint16_t *tours, const uint32_t *pairs, const uint32_t *lens, uint32_t n, uint32_t kcap, uint32_t count,
                                        uint16_t *out, hipStream_t s)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_cs_selftest_reversals));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cs_selftest_reversals, dim3(count), dim3(cuckoo_search_threads(n)), cuckoo_search_lds_bytes(n), s, tours, pairs, lens, n, kcap, out);
    return hipGetLastError();
}

}  // namespace tl
