// flower_pollination.hip — the flower pollination solver (flower_pollination.rs:53-151): R independent runs, the run a grid
// dimension, the flowers (16-bit cities), a staged move per flower, the costs and gbest in the context's workspace, two launches
// per epoch.
//
// The draws of flower i of epoch e are a pure function of (seed, run, e, i) (fpa_spec.h: this project's specification — the
// reference draws from an unseeded thread RNG): the switch trial, the Lévy length of a global move, the partners j and k and
// epsilon of a local one.  A global move reads flower i and gbest, a local one flower i and the flowers j and k, so every move of
// an epoch is built at once against the epoch-start state.  The commit then walks the flowers in order and builds flower i AGAIN,
// inside its workgroup and through the same device function, exactly when its staged move read something that has since changed:
// a global move after gbest changed, a local move whose j or k was accepted earlier in the epoch (flower i itself cannot have
// changed before its own turn, a j or k above i not yet) — the reference's order, without a host round trip.
//
//   k_fpa_init    one workgroup per (flower, run): the start flower (the initial tour, or a Fisher-Yates pass by one lane in
//                 LDS), its edge lengths by all lanes and their sum by one, in the reference's order (closing edge first).
//   k_fpa_first   one workgroup per run: gbest is a copy of the FIRST minimum flower.
//   k_fpa_move    one workgroup per (flower, run): fpa_build.
//   k_fpa_commit  one workgroup per run: the strict test, the copy and the gbest rule in flower order, fpa_build again where the
//                 staged move's inputs have changed; the log and the epoch row.
//
// fpa_build: the trial, j, k, epsilon and |levy| by every lane (the same instructions as one lane would take); flower i, and the
// inverse of the sequence's source (flower i for a global move, flower j for a local one) into LDS; swap_sequence(source, target)
// from its orbit form (swap_seq.h, shared with particle_swarm.hip); the prefix length; the prefix applied to flower i by one lane
// in order (the pairs have ascending i and q > i, but several may share a q); the edge lengths in parallel and their sum by one
// lane.
//
//   LDS of a workgroup: 768 bytes of header, wave counts and the commit's "accepted" bits | pairs[n] u32 (the sequence; the edge
//   lengths afterwards) | cur[n], inv[n], pi[n] u16  (10 n bytes).
#include "swarm_tour.h"
#include "fpa_spec.h"
#include "swap_seq.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr size_t kFpaFixedBytes = 768;  // header (16 words), the wave counts (2 parities x 16 waves), then one bit per flower (128 words) from byte 256

__host__ __device__ __forceinline__ size_t fpa_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

struct FpaLds {
    uint32_t *hdr, *wsum, *accepted, *pairs;
    float *E;
    uint16_t *cur, *inv, *pi;
    __device__ FpaLds(unsigned char *smem, uint32_t n)
    {
        hdr = reinterpret_cast<uint32_t *>(smem);
        wsum = hdr + 16;
        accepted = hdr + 64;
        const size_t wd = fpa_up16((size_t)n * 4), sh = fpa_up16((size_t)n * 2);
        unsigned char *p = smem + kFpaFixedBytes;
        pairs = reinterpret_cast<uint32_t *>(p);
        E = reinterpret_cast<float *>(p);
        cur = reinterpret_cast<uint16_t *>(p + wd);
        inv = reinterpret_cast<uint16_t *>(p + wd + sh);
        pi = reinterpret_cast<uint16_t *>(p + wd + 2 * sh);
    }
};

// `flower` into L.cur, the inverse of `source` into L.inv, swap_sequence(source, target) into L.pairs: its length, to every lane.
// Ends behind a barrier.
__device__ uint32_t fpa_sequence(const FpaLds &L, uint32_t n, const uint16_t *flower, const uint16_t *source, const uint16_t *target)
{
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) {
        L.cur[p] = flower[p];
        L.inv[source[p]] = (uint16_t)p;
    }
    TL_SYNC();
    return swap_sequence_orbit(target, n, L, L.pairs);
}

// apply_swaps (route.rs:137-143) of L.pairs[0 .. m) to L.cur by one lane, in order — swaps may share positions.  Begins behind a
// barrier, ends behind one.
__device__ void fpa_apply(const FpaLds &L, uint32_t n, uint32_t m)
{
    if (threadIdx.x == 0) {
        for (uint32_t t = 0; t < m; ++t) {
            const uint32_t s = L.pairs[t], a = s & 0xFFFFu, b = s >> 16;
            if (a < n && b < n) {
                const uint16_t x = L.cur[a];
                L.cur[a] = L.cur[b];
                L.cur[b] = x;
            }
        }
    }
    TL_SYNC();
}

// One move (flower_pollination.rs:12-51,119-125) by the whole workgroup: from flower i, gbest and the flowers j and k as they
// stand to stage[i], scost[i], slen[i].  Ends behind a barrier.
template <bool DM>
__device__ void fpa_build(const FpaArgs &A, const FpaLds &L, const CityDist<DM> &D, uint32_t run, uint32_t i, uint64_t key)
{
    const uint32_t n = A.n, N = A.flowers;
    const size_t row = (size_t)run * N;
    const uint64_t ev = fpa_event(A.epoch, N, i);
    const bool global = fpa_is_global(key, ev, A.switch_prob);
    uint32_t j = 0, k = 0;
    fpa_partners(key, ev, i, N, &j, &k);
    const uint16_t *fi = A.flower + (row + i) * n;
    const uint16_t *source = global ? fi : A.flower + (row + j) * n;
    const uint16_t *target = global ? A.gbest + (size_t)run * n : A.flower + (row + k) * n;
    const uint32_t len = fpa_sequence(L, n, fi, source, target);
    uint32_t m = 0;
    if (len) m = global ? fpa_global_swaps(fpa_levy(key, ev), len) : fpa_local_swaps(fpa_epsilon(key, ev), len);  // (the same on every lane)
    fpa_apply(L, n, m);
    write_and_cost<DM>(L.cur, L.E, D, n, A.stage + (row + i) * n, A.scost + row + i);
    if (threadIdx.x == 0) A.slen[row + i] = fpa_length_word(len, m);
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_fpa_init(FpaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, ind = blockIdx.x, run = blockIdx.y;
    const FpaLds L(smem, n);
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
    const size_t idx = (size_t)run * A.flowers + ind;
    write_and_cost<DM>(L.cur, L.E, D, n, A.flower + idx * n, A.cost + idx);
}

// gbest of the start: a copy of the FIRST minimum flower (min_by keeps the first of equals)
__global__ __launch_bounds__(256) void k_fpa_first(FpaArgs A)
{
    __shared__ uint32_t pick;
    const uint32_t n = A.n, N = A.flowers, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
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
    const uint16_t *src = A.flower + ((size_t)run * N + b) * n;
    for (uint32_t k = tid; k < n; k += nt) {
        A.gbest[(size_t)run * n + k] = src[k];
        if (A.last) A.out_pos[(size_t)run * n + k] = src[k];
    }
    if (run == 0u) log_improvement(A, 0u, 0xFFFFFFFFu, b, pc[b], src);
}

template <bool DM>
__global__ __launch_bounds__(256) void k_fpa_move(FpaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FpaLds L(smem, A.n);
    const CityDist<DM> D{A.xy, A.dm_full, A.n};
    fpa_build<DM>(A, L, D, blockIdx.y, blockIdx.x, sa_chain_key(A.seed, (uint64_t)A.first_run + blockIdx.y));
}

template <bool DM>
__global__ __launch_bounds__(256) void k_fpa_commit(FpaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, N = A.flowers, tid = threadIdx.x, nt = blockDim.x, run = blockIdx.x;
    const FpaLds L(smem, n);
    const CityDist<DM> D{A.xy, A.dm_full, n};
    const uint64_t key = sa_chain_key(A.seed, (uint64_t)A.first_run + run);
    uint32_t *state = A.state + 8u * (size_t)run;
    float g = __builtin_bit_cast(float, state[0]);
    uint32_t improved = state[1];
    bool changed = false;  // gbest has changed in this epoch
    uint16_t *gbest = A.gbest + (size_t)run * n;
    float *cost = A.cost + (size_t)run * N;
    const float *scost = A.scost + (size_t)run * N;
    uint32_t *erow = A.epoch_log && run == 0u && A.epoch < A.epoch_cap ? A.epoch_log + (size_t)A.epoch * 4u * N : nullptr;
    for (uint32_t w = tid; w < (kFpaMaxFlowers >> 5); w += nt) L.accepted[w] = 0u;
    TL_SYNC();
    for (uint32_t i = 0; i < N; ++i) {  // (every condition below is the same on every lane: the barriers are met by all)
        const uint64_t ev = fpa_event(A.epoch, N, i);
        const bool global = fpa_is_global(key, ev, A.switch_prob);
        uint32_t j = 0, k = 0;
        fpa_partners(key, ev, i, N, &j, &k);
        const bool moved = ((L.accepted[j >> 5] >> (j & 31u)) | (L.accepted[k >> 5] >> (k & 31u))) & 1u;  // (only flowers below i can be marked)
        const bool again = global ? changed : moved;  // the staged move read something that has since changed
        if (again) fpa_build<DM>(A, L, D, run, i, key);
        const float c = scost[i];
        const bool acc = c < cost[i];  // strict: an unchanged flower is never accepted
        if (erow && tid == 0) {
            erow[N + i] = fpa_kind_word(global, j, k);
            erow[3u * N + i] = (acc ? 1u : 0u) | (again ? 2u : 0u);
        }
        if (acc) {
            const uint16_t *src = A.stage + ((size_t)run * N + i) * n;
            uint16_t *dst = A.flower + ((size_t)run * N + i) * n;
            for (uint32_t p = tid; p < n; p += nt) dst[p] = src[p];
            if (c < g) {
                for (uint32_t p = tid; p < n; p += nt) gbest[p] = src[p];
                ++improved;
                if (run == 0u) log_improvement(A, improved, A.epoch, i, c, src);
                g = c;
                changed = true;
            }
            TL_SYNC();  // every lane has read cost[i] and the bits; flower i and gbest are whole before a later build reads them
            if (tid == 0) {
                cost[i] = c;
                L.accepted[i >> 5] |= 1u << (i & 31u);
            }
            TL_SYNC();
        }
    }
    TL_SYNC();
    if (tid == 0) {
        state[0] = __builtin_bit_cast(uint32_t, g);
        state[1] = improved;
        if (A.last) A.out_cost[run] = g;
    }
    if (erow) {
        for (uint32_t i = tid; i < N; i += nt) {
            erow[i] = __builtin_bit_cast(uint32_t, cost[i]);
            erow[2u * N + i] = A.slen[(size_t)run * N + i];
        }
    }
    if (A.last) {
        for (uint32_t p = tid; p < n; p += nt) A.out_pos[(size_t)run * n + p] = gbest[p];
    }
}

// the device's move on given (flower, source, target, prefix length) tuples (tl_fpa_selftest_pollinate): one workgroup per tuple;
// the prefix is cut to the sequence's length
__global__ __launch_bounds__(256) void k_fpa_selftest_pollinate(const uint16_t *flower, const uint16_t *source, const uint16_t *target, const uint32_t *prefix,
                                                                uint32_t n, uint16_t *out, uint32_t *out_len)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FpaLds L(smem, n);
    const size_t at = (size_t)blockIdx.x * n;
    const uint32_t len = fpa_sequence(L, n, flower + at, source + at, target + at);
    fpa_apply(L, n, prefix[blockIdx.x] < len ? prefix[blockIdx.x] : len);
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) out[at + p] = L.cur[p];
    if (threadIdx.x == 0) out_len[blockIdx.x] = len;
}

size_t flower_pollination_lds_bytes(uint32_t n) { return kFpaFixedBytes + fpa_up16((size_t)n * 4) + 3 * fpa_up16((size_t)n * 2); }

uint32_t flower_pollination_max_n(int lds_budget)
{
    if (lds_budget <= 0) return 0u;
    uint64_t m = (uint64_t)lds_budget / 10u;
    if (m > 0xFFFFu) m = 0xFFFFu;  // (cities and the positions of a pair are 16 bits wide)
    while (m > 0u && flower_pollination_lds_bytes((uint32_t)m) > (size_t)lds_budget) --m;
    return (uint32_t)m;
}

int flower_pollination_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 64u ? 64 : t > 256u ? 256 : (int)t;
}

hipError_t launch_fpa_init(const FpaArgs &A, uint32_t runs, hipStream_t s)
{
    hipError_t e = launch_max_lds(A.dm_full ? k_fpa_init<true> : k_fpa_init<false>, dim3(A.flowers, runs), flower_pollination_threads(A.n),
                              flower_pollination_lds_bytes(A.n), s, A);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fpa_first, dim3(runs), dim3(flower_pollination_threads(A.n)), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_fpa_move(const FpaArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_fpa_move<true> : k_fpa_move<false>, dim3(A.flowers, runs), flower_pollination_threads(A.n), flower_pollination_lds_bytes(A.n), s,
                      A);
}

hipError_t launch_fpa_commit(const FpaArgs &A, uint32_t runs, hipStream_t s)
{
    return launch_max_lds(A.dm_full ? k_fpa_commit<true> : k_fpa_commit<false>, dim3(runs), flower_pollination_threads(A.n), flower_pollination_lds_bytes(A.n), s, A);
}

hipError_t launch_fpa_selftest_pollinate(const uint16_t *flower, const uint16_t *source, const uint16_t *target, const uint32_t *prefix, uint32_t n, uint32_t count,
                                         uint16_t *out, uint32_t *out_len, hipStream_t s)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_fpa_selftest_pollinate));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fpa_selftest_pollinate, dim3(count), dim3(flower_pollination_threads(n)), flower_pollination_lds_bytes(n), s, flower, source, target, prefix,
                       n, out, out_len);
    return hipGetLastError();
}

}  // namespace tl
