// lk_ils.h — k_lk_ils, the whole ILS of a SMALL instance (a part of lk.hip; round 5): ONE persistent workgroup,
// every array the search touches in this CU's LDS as 16-bit city ids (coordinates, candidate lists, tour, scratch tour, rank,
// successor, predecessor, scan order, best tour: n (22 + 2k) bytes), no kernel boundary per round — at berlin52's size a round of
// the chip-wide form is 23.6 us of launch latency around a scan of 52 x 2 x 3 candidates.
//
// What made the round-2 single-workgroup form (k_lk_solve<NT, true>) slow was one LANE walking a pair's whole depth-first search
// (up to k + k^2 + ... + k^depth nodes, three dependent look-ups each).  Here find_lk_move (:345-389) runs LEVEL BY LEVEL over a
// chunk of consecutive (t1, orientation) pairs: a lane is (live node, candidate q) — one branch of find_lk_chain's loop (:290-337)
// — and files the child it creates, after the child's own closing test (:280-283), in the next level's queue.  A node's place in
// the reference's depth-first order is its PATH (q0, q1, ...): as a key of `bits` per level, digit q + 1, most significant first,
// zeros behind a node that closes — so a closing node sorts before its own descendants and after everything under an earlier
// sibling, exactly as the recursion meets them.  The pair's first chain is the minimum key that closed (ds_min_u64 per pair), and
// nodes behind an already posted key are not expanded.  Exactness of dropping the `break` at g1 <= EPS (:292-295): see lk_subsearch.
// Then, as in the reference (:373-381): only that first chain of a pair is checked for a single cycle; the lowest pair with a
// valid one wins; its wave builds the move's segment table; the workgroup copies the arcs.  Chunks grow geometrically from the
// front (hits of a running pass sit near the front), a queue overflow halves the chunk and repeats it (the plan guarantees that a
// chunk of one pair fits: k^(max_depth-1) <= queue capacity).
//
// The ILS state machine (first pass, kick, accept / plateau: :61-97) runs in the same workgroup; a launch is a SLICE of at most
// LkArgs::ils_slice scans — the state lives in LkState + the global tour / best / city_ids between slices — so that the host can
// drain progress snapshots (tl_lk_live) and a run of minutes is no single launch.
//
// k_lk_ils is ONE body built from lambdas (rebuild, tour_distance, snapshot, expand, scan, apply_move, kick_from_best, then the two
// drivers: mode 2 and the slice loop).  As named force-inlined functions over a struct of the LDS pointers and one of the launch's
// scalars it did not compile to the same instructions (NOTEBOOK.md, the entry of lk_chain.h): it stays one body until it does.
#pragma once

namespace {
__device__ __forceinline__ uint32_t readlane_u32(uint32_t v, uint32_t l)  // l: wave-uniform
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)l));
}
constexpr int kIlsNT = 1024;
#ifndef TL_ILS_SMALL_N
#define TL_ILS_SMALL_N 200u
#endif
constexpr uint32_t kIlsSmallN = TL_ILS_SMALL_N;  // up to here k_lk_ils runs on 4 waves
constexpr uint32_t kIlsHdr = 4u;  // record words in front of the chain: key lo, key hi, gain, pair (chunk-local)

__host__ __device__ __forceinline__ uint32_t ils_bits(uint32_t k)
{
    uint32_t b = 1u;
    while ((1u << b) < k + 1u) ++b;
    return b;
}
__host__ __device__ __forceinline__ size_t ils_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }
// LDS image: xy | cand | dcand (the candidates' distances) | dnext (every city's tour edge to its successor) | 7 x u16[n] |
// pairmin u64[kIlsNT] | two queues of qcap records of (kIlsHdr + max_depth) words
__host__ __device__ __forceinline__ size_t ils_fixed_bytes(uint32_t n, uint32_t k)
{
    return ils_up16((size_t)n * 8) + ils_up16((size_t)n * k * 2) + ils_up16((size_t)n * k * 4) + ils_up16((size_t)n * 4) + 7u * ils_up16((size_t)n * 2) +
           (size_t)kIlsNT * 8;
}
// the kernel's static __shared__: per-wave segment tables + words
constexpr size_t kIlsStatic = (size_t)(kIlsNT / 64) * kLkMaxSeg * 16 + 1024;

}  // namespace

// the form applies iff this returns a queue capacity (records per level) > 0
uint32_t lk_ils_qcap(uint32_t n, uint32_t k, uint32_t max_depth, size_t lds_budget)
{
    if (n < 4 || n > 65535u || k == 0 || k > 16u || max_depth == 0 || max_depth > (uint32_t)kLkMaxDepth) return 0u;  // (k <= 16: the task -> (node, candidate) split of a level)
    if (ils_bits(k) * max_depth > 64u) return 0u;
    const size_t fixed = ils_fixed_bytes(n, k) + kIlsStatic;
    if (fixed >= lds_budget) return 0u;
    const size_t rec = (size_t)(kIlsHdr + max_depth) * 4;
    size_t qcap = (lds_budget - fixed) / (2 * rec);
    // a chunk of ONE pair must fit: its widest queued level holds k^(max_depth-1) nodes; the queues also serve as the n floats of
    // the ordered cost sum
    uint64_t need = 1;
    for (uint32_t d = 1; d < max_depth; ++d) {
        need *= k;
        if (need > qcap) return 0u;
    }
    // no more than the search uses: a level of a chunk of <= 1024 pairs rarely holds more than a few hundred nodes (an overflow
    // only halves the chunk), and a small image lets two epochs share a CU
    size_t cap = need > 512 ? need : 512;
    if ((size_t)n * 4 > 2 * cap * rec) cap = ((size_t)n * 4 + 2 * rec - 1) / (2 * rec);
    if (cap > 2048) cap = 2048;
    if (qcap > cap) qcap = cap;
    if (qcap < 64 || 2 * qcap * rec < (size_t)n * 4) return 0u;
    return (uint32_t)qcap;
}

size_t lk_ils_lds_bytes(uint32_t n, uint32_t k, uint32_t max_depth, uint32_t qcap)
{
    return ils_fixed_bytes(n, k) + 2 * (size_t)qcap * (kIlsHdr + max_depth) * 4 + kIlsStatic;
}

// the workgroup width launch_lk_ils and launch_lk_ils_pop choose by n
uint32_t lk_ils_threads(uint32_t n) { return n <= kIlsSmallN ? 256u : (uint32_t)kIlsNT; }

namespace {

// The profile build (-DTL_PROFILE_ILS, scripts/lk_ils_profile.py): cycles per phase of a slice in iq[0..6], the levels run in iq[7]
#ifdef TL_PROFILE_ILS
#define TL_IPROFILE_BEGIN() uint64_t iq[8] = {0, 0, 0, 0, 0, 0, 0, 0}, it = __builtin_amdgcn_s_memtime()
#define TL_ISTAMP(k) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); iq[k] += t_ - it; it = t_; } while (0)
#define TL_ICOUNT(k) do { iq[k] += 1; } while (0)
#define TL_IPROFILE_END(n, scans) do { if (threadIdx.x == 0) ils_profile_print(iq, n, (unsigned long)(scans), (unsigned long)(scans) + 1ul); } while (0)
__device__ void ils_profile_print(const uint64_t (&iq)[8], uint32_t n, unsigned long scans, unsigned long per)
{
    printf("k_lk_ils n=%u: scans %lu; cycles per scan: chunk init %lu, level 0 %lu, deeper levels %lu (%lu levels per 100 scans), validation %lu, segment table %lu, apply + rebuild %lu, pass end %lu\n",
           n, scans, iq[0] / per, iq[1] / per, iq[2] / per, iq[7] * 100 / per, iq[3] / per, iq[4] / per, iq[5] / per, iq[6] / per);
}
#else
#define TL_IPROFILE_BEGIN() do { } while (0)
#define TL_ISTAMP(k) do { } while (0)
#define TL_ICOUNT(k) do { } while (0)
#define TL_IPROFILE_END(n, scans) do { } while (0)
#endif

// Pop: the POPULATION launch (tl_lk_population) — workgroup b is seeded run b of the call and executes what mode 0
// executes, on its own LkState, tour, best, city_ids and seed; xy, the candidate lists and their distances (ils_dcand, filled once
// by k_lk_pop_prepare) are shared.  A run that has finished (or whose pass cycles: finished == 2) returns at once; no workgroup waits
// for another.
// (The body is lk_ils_body.h, included into both kernels: as a function of its own, force-inlined into the two, k_lk_ils<NT> did not keep
//  its instructions — NOTEBOOK.md, "Lin-Kernighan for seeded runs".)
template <int NT>
__global__ __launch_bounds__(NT) void k_lk_ils(LkArgs G)
{
    constexpr bool Pop = false;
#include "lk_ils_body.h"
}
template <int NT>
__global__ __launch_bounds__(NT) void k_lk_ils_pop(LkArgs G)
{
    constexpr bool Pop = true;
#include "lk_ils_body.h"
}

// The verdict over a batch of speculative epochs (k_lk_ils mode 2), in epoch order, exactly as the sequential loop gives it
// (lin_kernighan.rs:75-97): an epoch's counters count; shorter than the best -> it becomes the best (PathUpdate), the plateau
// count restarts, and the batch ends here — the later epochs of the batch were kicked from a tour that is no longer the best and
// are run again; not shorter -> the plateau count grows and may end the search.
__global__ __launch_bounds__(256) void k_lk_ils_commit(LkArgs G)
{
    __shared__ uint32_t s_acc;
    __shared__ float s_d;
    LkState *S = G.state;
    if (S->finished) return;
    const uint32_t tid = threadIdx.x, n = G.n;
    const uint32_t width = S->applied < G.ils_P ? S->applied : G.ils_P;
    const uint32_t left = G.epochs - S->epoch, P = width < left ? width : left;
    if (tid == 0) {
        uint32_t epoch = S->epoch, platoo = S->platoo, acc = 0xFFFFFFFFu;
        float best_dist = S->best_dist;
        uint64_t scans = S->scans, searches = S->searches, moves = S->moves, exchanged = S->exchanged;
        bool fin = false;
        uint32_t window = S->window;
        for (uint32_t j = 0; j < P; ++j) {
            const uint64_t *cn = G.ils_ep_cnt + (size_t)j * 4;
            if (cn[0] == ~0ull) {  // out of its scan budget: the verdict stops in front of it; if it is the next epoch it runs again, longer
                if (j == 0u) {  // the next epoch: again with 8 x the budget — or, if that was lk_pass_cap already, it does not terminate
                    const uint32_t lvl = window < 6u ? window : 6u;
                    if (((uint64_t)G.ils_slice << (3u * lvl)) >= lk_pass_cap(n)) S->key = 0xDEAD0001u;
                    ++window;
                }
                break;
            }
            if (j == 0u) window = 0u;
            scans += cn[0];
            searches += cn[1];
            moves += cn[2];
            exchanged += cn[3];
            const float d = G.ils_ep_dist[j];
            bool stop = false;
            if (d < best_dist) {      // :86
                best_dist = d;
                platoo = 0u;
                acc = j;
            } else if (++platoo >= G.platoo_epochs) {  // :92-95
                stop = true;
            }
            ++epoch;
            fin = stop || epoch >= G.epochs;
            if (fin || acc != 0xFFFFFFFFu) break;
        }
        S->epoch = epoch;
        S->platoo = platoo;
        S->best_dist = best_dist;
        S->draws = n >= 8u ? 3ull * epoch : 0ull;
        S->scans = scans;
        S->searches = searches;
        S->moves = moves;
        S->exchanged = exchanged;
        S->finished = fin ? 1u : (S->key == 0xDEAD0001u ? 2u : 0u);
        S->window = window;
        // the next batch's width: decided at epoch j -> a few times j; a batch that was rejected throughout -> four times as wide
        {
            uint32_t w2 = acc != 0xFFFFFFFFu ? 4u * (acc + 1u) + 8u : 4u * width;
            w2 = w2 < 16u ? 16u : w2;
            S->applied = w2 > G.ils_P ? G.ils_P : w2;
        }
        s_acc = acc;
        s_d = best_dist;
    }
    TL_SYNC();
    const uint32_t acc = s_acc;
    if (acc == 0xFFFFFFFFu) return;
    const uint32_t *src = G.ils_ep_tour + (size_t)acc * n;
    const uint32_t sidx = S->snaps;
    const bool keep = G.snap && (G.snap_ring || sidx < G.snap_cap);
    const uint32_t at = G.snap_ring ? sidx % (G.snap_cap ? G.snap_cap : 1u) : sidx;
    for (uint32_t r = tid; r < n; r += 256u) {
        const uint32_t c = src[r];
        G.best[r] = c;
        if (keep) G.snap[(size_t)at * n + r] = c;  // :90 send_progress(best_tour, best_dist)
    }
    TL_SYNC();
    if (tid == 0) {
        if (keep) G.snap_dist[at] = s_d;
        S->snaps = sidx + 1u;
    }
}

// Before a population's first slice: the candidates' distances once for every run (what a workgroup of mode 0 computes for itself,
// the same dist), and, where the runs share one start tour, row 0 of the tours copied into the rows behind it.
__global__ __launch_bounds__(256) void k_lk_pop_prepare(LkArgs G, uint32_t count, uint32_t share_start)
{
    const size_t gid = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t e = gid; e < (size_t)G.n * G.k; e += step) G.ils_dcand[e] = dist(G.xy[e / G.k], G.xy[G.cand[e]]);
    if (share_start)
        for (size_t e = gid + G.n; e < (size_t)count * G.n; e += step) G.tour[e] = G.tour[e % G.n];
}
}  // namespace

hipError_t launch_lk_pop_prepare(const LkArgs &G, uint32_t count, bool share_start, hipStream_t s)
{
    const size_t work = (size_t)G.n * (share_start ? (count > G.k ? count : G.k) : G.k);
    const size_t blocks = (work + 255) / 256;
    hipLaunchKernelGGL(k_lk_pop_prepare, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(256), 0, s, G, count, share_start ? 1u : 0u);
    return hipGetLastError();
}

// one slice of every unfinished run of a population: workgroup b works on G.state[b], row b of G.tour / best / city_ids, the seed G.counters[b]
hipError_t launch_lk_ils_pop(const LkArgs &G, uint32_t count, hipStream_t s)
{
    const size_t lds = ils_fixed_bytes(G.n, G.k) + 2 * (size_t)G.ils_qcap * (kIlsHdr + G.max_depth) * 4;
    auto go = [&](auto kern, int nt) -> hipError_t {
        hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(count), dim3(nt), lds, s, G);
        return hipGetLastError();
    };
    if (G.n <= kIlsSmallN) return go(k_lk_ils_pop<256>, 256);
    return go(k_lk_ils_pop<kIlsNT>, kIlsNT);
}

hipError_t launch_lk_ils_commit(const LkArgs &G, hipStream_t s)
{
    hipLaunchKernelGGL(k_lk_ils_commit, dim3(1), dim3(256), 0, s, G);
    return hipGetLastError();
}

hipError_t launch_lk_ils(const LkArgs &G, hipStream_t s)
{
    const size_t lds = ils_fixed_bytes(G.n, G.k) + 2 * (size_t)G.ils_qcap * (kIlsHdr + G.max_depth) * 4;
    auto go = [&](auto kern, int nt) -> hipError_t {
        hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(G.ils_mode == 2u ? G.ils_P : 1u), dim3(nt), lds, s, G);
        return hipGetLastError();
    };
    // a level of a small instance is a few hundred lanes: four waves meet at a barrier faster than sixteen
    const uint32_t nt = G.ils_threads ? G.ils_threads : (G.n <= kIlsSmallN ? 256u : 1024u);
    if (nt == 256u) return go(k_lk_ils<256>, 256);
    if (nt == 512u) return go(k_lk_ils<512>, 512);
    return go(k_lk_ils<kIlsNT>, kIlsNT);
}
