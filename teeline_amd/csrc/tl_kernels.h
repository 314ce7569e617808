// tl_kernels.h — kernel argument blocks and launch entry points (internal to libteeline_gpu).
#pragma once
#include "tl_device.h"

#ifndef TL_TWO_OPT_NT
#define TL_TWO_OPT_NT 1024  // threads per descent workgroup (16 waves, 4 per SIMD)
#endif

#include <mutex>
#include <set>
#include <utility>

namespace tl {

// MaxDynamicSharedMemorySize is an attribute of the FUNCTION (per device), not of a launch or a stream: setting it per launch
// to the size of that launch lets two host threads solving different n race (set 110 KB, set 30 KB, launch with 110 KB ->
// invalid configuration).  Every launcher therefore raises it ONCE per (kernel, device) to all the LDS the device has left
// beside the kernel's static allocation, and passes its real size only as the launch parameter.
inline hipError_t allow_max_lds(const void *kern)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({kern, dev})) return hipSuccess;
    int maxlds = 0;
    if ((e = hipDeviceGetAttribute(&maxlds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev)) != hipSuccess) return e;
    hipFuncAttributes fa;
    if ((e = hipFuncGetAttributes(&fa, kern)) != hipSuccess) return e;
    const int dyn = maxlds - (int)fa.sharedSizeBytes;
    if ((e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, dyn)) != hipSuccess) return e;
    done.insert({kern, dev});
    return hipSuccess;
}

// u64 words per descent in out_stats: sweeps, moves, reversed, status, steps, then profile words
#define TL_STATS_STRIDE 16

enum : uint32_t { TL_INIT_IDENTITY = 0, TL_INIT_ARRAY = 1, TL_INIT_SEEDED = 2 };

// Neighbour lists of an instance (two_opt_nl.hip): what the late sweeps of the LDS descent read instead of walking tiles.
// One 128-byte record of 64 u16 per city, so that a row (a, b) is ONE wave-wide load of two cache lines — lane l reads word l of
// a's record (l < kNlRecB0, except the count) or of b's:
//   [0]       high half of the bits of the KA-th smallest squared distance from the city (i.e. rounded down)
//   [2]       1 if more than kNlRB cities have this one among their KB nearest (the list below is then incomplete), else 0
//   [4 .. 20) its KA nearest cities
//   [20 .. 56) the cities that have it among their KB nearest (the first kNlRB of them), 0xFFFF = empty slot
//   [56 .. 64) unused here: those lanes of a row's pass take the chunk's long cities
constexpr int kNlKA = 16;        // nearest cities kept per city for "c closer to a than b" (rows with a longer (a, b) take the tile path)
constexpr int kNlKB = 24;        // nearest cities per city behind the reverse lists ("b closer to e than c")
constexpr int kNlRecA0 = 4, kNlRecB0 = 20, kNlRB = 36, kNlSurv0 = 56, kNlSurvSlots = 8;
constexpr int kNlLongCap = 128;  // cities with a tour edge beyond their KB-th distance a descent can hold (more: tile path for the sweep)
struct TwoOptNl {
    const uint16_t *rec;     // [n][64] records; nullptr = no lists (tile path only)
    const uint32_t *dkb2;    // [n] bits of the KB-th smallest squared distance
    const uint16_t *knn_b;   // [n][kNlKB] the KB nearest cities of each city (the forward form of the reverse lists; diagnostics)
    const uint32_t *rcnt;    // [n] reverse counts (diagnostics)
    uint32_t sweep_min;      // first sweep of a descent that may run in the late phase (neighbour-list rows) ...
    uint32_t moves_max;      // ... once a sweep has applied fewer moves than this (in the late phase every move is a whole step)
};
size_t two_opt_nl_ws_bytes(uint32_t n);
hipError_t launch_two_opt_nl_build(const float2 *xy, uint32_t n, void *ws, bool fresh, TwoOptNl *out, hipStream_t s, int form = 0);  // form 1: the workgroup-per-city kernel (cross-check)

// two_opt_dm.hip — the matrix form's lists for its late sweeps: per city the 16 nearest by its matrix row and the
// reverse relation, cut from the full matrix once per call and shared by every descent of the batch
constexpr int kDmK = 16;     // nearest cities per city (the c side of a row: D[a][c] < D[a][b])
constexpr int kDmInv = 48;   // reverse-list slots per city (the e side: D[b][e] < D[c][e]; lanes 16..63 of a row's pass)
#ifndef TL_DM_LONG_CAP
#define TL_DM_LONG_CAP 1024  // (256 / 512 / 1024 measured: n = 1 002 alike, n = 5 000 population 148 / 134 / 131 ms)
#endif
// cities with a tour edge beyond their kDmK-th distance a descent's list (LDS) can hold in its late sweeps.  ONE constant for the kernel
// (two_opt_dm.hip) and for the host's threshold (tl_api_two_opt.hip: TL_DM_LONG_MAX <= this, by static_assert; the kernel clamps too)
constexpr uint32_t kDmLongCap = TL_DM_LONG_CAP;
struct DmLists {
    const uint16_t *id;       // [n][kDmK] nearest cities in (distance, id) order, the city itself excluded; nullptr = no lists
    const float *d;           // [n][kDmK] their distances
    const float *dk;          // [n] the kDmK-th of them (NaN where the row holds a NaN: never listed)
    const uint16_t *inv_id;   // [n][kDmInv] the cities that hold this one among their kDmK (0xFFFF: empty slot)
    const float *inv_d;       // [n][kDmInv] D[that city][this one]
    const uint32_t *inv_cnt;  // [n] entries offered (beyond kDmInv: the list is incomplete, the row walks the matrix row)
    uint32_t long_max;        // a sweep runs on the lists while at most this many cities have a tour edge beyond their dk (<= kDmLongCap)
    uint32_t moves_max;       // ... and the sweep before it applied at most this many moves
};
size_t dm_lists_ws_bytes(uint32_t n);
bool two_opt_ref_dm_late_fits(uint32_t n, int lds_budget);  // the late sweeps' state fits the LDS beside the tour
size_t two_opt_ref_dm_late_work_bytes(uint32_t n, uint32_t count);  // ... and the descents' per-city records in HBM (TwoOptBatchArgs::work)
hipError_t launch_dm_lists_build(const float *full, uint32_t n, void *ws, DmLists *out, hipStream_t s);

struct TwoOptBatchArgs {
    const float2 *xy;        // n cities, city order
    const float *dm;         // packed lower triangle (matrix kernels) or nullptr
    const float *dm_full;    // the same matrix expanded to row-major n x n (k_dm_expand_full), matrix kernels only
    const uint32_t *init;    // [count][n] when init_mode == TL_INIT_ARRAY
    uint32_t *out_pos;       // [count][n]
    float *out_cost;         // [count]
    uint64_t *out_stats;     // [count][TL_STATS_STRIDE] = sweeps, moves, reversed, status(0 ok, 1 sweep cap), steps, ...
    uint64_t seed;
    uint32_t first;          // restart index of descent 0 (seeded init)
    uint32_t n;
    uint32_t n_pad;
    uint32_t max_sweeps;
    uint32_t init_mode;
    uint32_t *work;          // per-descent global workspace (global-memory variants)
    uint32_t *move_log;      // LDS kernel, optional: [count][log_cap] words — (row << 16 | column) of every applied move in the reference's
    uint32_t log_cap;        // order (two_opt.rs:50), 0xFFFFFFFF where a new sweep begins — what a caller replays the reference's per-move
                             // progress messages from; NULL = off
    const uint2 *fx_xy;      // LDS kernel, grid-coordinate form: per city {x (20 bits) | y low 12 bits << 20, y high 8 bits} (k_fx_encode)
    double fx_inv;           // ... fl64(1 / S) of its decimal grid, 0 = plain float2 form
    TwoOptNl nl;             // LDS kernel, 16-wave float2 form: neighbour lists for the late sweeps (rec == nullptr: off)
    DmLists dml;             // matrix kernel: lists for its late sweeps (id == nullptr: off)
};

// two_opt_ref.hip
size_t two_opt_ref_lds_bytes(uint32_t n, uint32_t *n_pad_out);
size_t two_opt_ref_nl_lds_bytes(uint32_t n);  // ... with the neighbour-list state (city -> position table, long list) beside the tour
// would a batch of `count` descents run in the form that reads neighbour lists (16 waves, float2 points, lists + tour fit the LDS)?
bool two_opt_ref_nl_applies(uint32_t n, uint32_t count, int cus, int lds_budget, int force_nt);
int two_opt_ref_pick_nt(uint32_t n, uint32_t count, int cus, int lds_budget, int force_nt);   // threads per descent of such a batch
bool two_opt_ref_nl_form(uint32_t n, uint32_t count, int cus, int lds_budget, int force_nt);  // ... and whether that form reads the lists
hipError_t launch_two_opt_ref_lds(const TwoOptBatchArgs &A, uint32_t count, bool prune, hipStream_t s, bool count_work, int cus, int lds_budget,
                                  int force_nt);
// grid-coordinate form (A.fx_xy / A.fx_inv set): would it let two tours share a CU where the float2 form cannot?
bool two_opt_ref_fx_pays(uint32_t n, uint32_t count, int cus, int lds_budget);
size_t two_opt_ref_fx_lds_bytes(uint32_t n);
// encode xy on the grid 1/scale: out[c] = packed grid coordinates, *bad += cities that do not decode back bit for bit
hipError_t launch_fx_encode(const float2 *xy, uint32_t n, double scale, uint2 *out, uint32_t *bad, hipStream_t s);

// two_opt_dm.hip — same algorithm, distances gathered from the packed matrix in HBM/L2
size_t two_opt_ref_dm_lds_bytes(uint32_t n);
hipError_t launch_two_opt_ref_dm(const TwoOptBatchArgs &A, uint32_t count, int lds_budget, hipStream_t s);
hipError_t launch_dm_expand_full(const float *packed, uint32_t n, float *full, hipStream_t s);

// two_opt_best.hip — BEST_SWEEP mode (whole chip per sweep)
struct BestSweepArgs {
    const float2 *xy;
    uint32_t *perm;                // [n] in/out (device)
    float2 *P;                     // [n_pad + 1] tour-ordered coordinates
    float4 *tbox;                  // [ntile_cap] L0 boxes
    float *tmsq;                   // [ntile_cap]
    unsigned long long *partials;  // one packed key per scan workgroup
    unsigned long long *rowkey;    // [n] every row's best candidate as of the last sweep that decided it (kNoKey64: none)
    uint32_t *move;                // {a move has been applied, its row is, its column js}: what the next sweep must decide again
    uint64_t *counters;            // sweeps, moves, done, reversed
    uint32_t n, n_pad, ntile_cap, phase;
};
hipError_t launch_best_sweep_init(const BestSweepArgs &A, hipStream_t s);
hipError_t launch_best_sweep_round(const BestSweepArgs &A, hipStream_t s);
uint32_t best_sweep_scan_blocks(uint32_t n);

// two_opt_best_lds.hip — BEST_SWEEP for a batch: one workgroup per descent, the whole state in its LDS
struct BestLdsArgs {
    const float2 *xy;      // n cities, city order
    const uint32_t *init;  // [count][n] when init_mode == TL_INIT_ARRAY
    uint32_t *out_pos;     // [count][n]
    float *out_cost;       // [count]
    uint64_t *out_stats;   // [count][TL_STATS_STRIDE] = sweeps, moves, reversed, status (0 ok, 1 sweep cap, 2 init position >= n), 0 ...
    uint64_t seed;
    uint32_t first;        // restart index of descent 0 (TL_INIT_SEEDED)
    uint32_t n;
    uint32_t max_sweeps;
    uint32_t init_mode;    // TL_INIT_ARRAY or TL_INIT_SEEDED
};
size_t two_opt_best_lds_bytes(uint32_t n);            // LDS of one descent's workgroup
uint32_t two_opt_best_lds_max_n(int lds_budget);      // largest n whose state fits (0: none)
int two_opt_best_lds_threads(uint32_t n, uint32_t count, int cus, int lds_budget);
hipError_t launch_two_opt_best_lds(const BestLdsArgs &A, uint32_t count, int threads, hipStream_t s);

// two_opt_large.hip — REF_ORDER for tours beyond one CU's LDS
struct LargeTwoOptState {
    unsigned long long key;  // (row << 32) | column of the lexicographically first improving candidate of the round; ~0 = none
    uint32_t i0, j0, rows, improved, sweeps, done, status, pad_;
    uint64_t moves, reversed;
};
struct LargeTwoOptArgs {
    const float2 *xy;
    uint32_t *perm;     // [n] in/out
    float2 *P;          // [n_pad + 1]
    float4 *tbox;       // [ntile_cap]
    float *tmsq;        // [ntile_cap]
    LargeTwoOptState *state;
    uint32_t n, n_pad, ntile_cap, max_sweeps;
};
hipError_t launch_large_two_opt_init(const LargeTwoOptArgs &A, hipStream_t s);
hipError_t launch_large_two_opt_round(const LargeTwoOptArgs &A, hipStream_t s);

// A best-improvement descent (3-opt, Or-opt) runs as batches of passes enqueued back to back: the pick kernel of a pass that finds
// no move sets `done`, every kernel of a later pass of the batch returns at once, and the host polls this block once per batch
// instead of once per pass (round 4: the per-pass read-back was 40 % of an Or-opt descent at n = 5 000).
struct ScanRunState {
    uint32_t done;     // a pass found no improving move: the descent is over
    uint32_t passes;   // find_best_move calls so far (the last one finds nothing)
    uint32_t moves;    // moves applied; also the number of log entries offered
    uint32_t log_cap;  // entries (4 words each) the move log holds
};
// What one thread of a pick kernel does with its pass (three_opt.rs:36-45, or_opt.rs:45 `while let Some(best) = find_best_move(..)`):
// count the pass, file the move's four words or end the descent.  run == nullptr: a single find_best_move, nothing to file.
__device__ __forceinline__ void scan_file_pass(ScanRunState *run, uint32_t *log, bool found, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    if (!run) return;
    run->passes += 1u;
    if (!found) {
        run->done = 1u;
        return;
    }
    const uint32_t m = run->moves;
    if (m < run->log_cap) {
        log[4u * m + 0u] = w0;
        log[4u * m + 1u] = w1;
        log[4u * m + 2u] = w2;
        log[4u * m + 3u] = w3;
    }
    run->moves = m + 1u;
}

// three_opt.hip
struct ThreeOptBest {
    float sav;
    uint32_t ij;     // i << 16 | j
    uint32_t kc;     // k << 3 | case (1..7); 0xFFFFFFFF = none
    uint32_t found;
};
struct ThreeOptArgs {
    const float2 *xy;
    const float *dm;             // packed matrix or nullptr
    uint32_t *perm;              // [n] tour positions, updated in place by k_three_opt_pick
    float2 *Pt;                  // [n+1] tour-ordered coordinates (coordinate form)
    float *E;                    // [n] tour-edge lengths, E[n-1] = closing edge
    float *Dt;                   // [n][n+1] distances between tour POSITIONS, column n == column 0 (rebuilt every pass)
    const uint32_t *chunk_prefix;  // [n-1]: chunks of rows < i
    ThreeOptBest *partials;      // one per scan workgroup
    ThreeOptBest *best;          // result of the pass
    uint64_t *counters;          // passes, moves
    uint32_t *scratch;           // [n] the move's two segments in k_three_opt_pick where they do not fit the LDS
    ScanRunState *run;           // a descent's batch state (nullptr: a single find_best_move)
    uint32_t *log;               // [run->log_cap][4] applied moves: i, j, k, case
    uint32_t n;
    uint32_t jc;                 // j values per scan workgroup
};
size_t three_opt_scan_lds_bytes(uint32_t n);
hipError_t launch_three_opt_pass(const ThreeOptArgs &A, uint32_t nblocks, bool dm, int apply, hipStream_t s, int lds_budget);

// A population of tours, one persistent workgroup per tour running the whole descent without a launch per move: what
// three_opt_pop.hip and or_opt_lds.hip share
struct PopArgs {
    const float2 *xy;      // n cities, city order (coordinate form)
    const float *dm;       // packed matrix or nullptr
    const uint32_t *init;  // [count][n] start tours of this launch (permutations: the host checks)
    uint32_t *out_pos;     // [count][n]
    float *out_cost;       // [count] tour_length of the result
    uint32_t *out_run;     // [count][4] moves, passes, status (1: pass cap reached), 0
    float *Dt;             // 3-opt: [count][n][n+1] each tour's distances between tour positions (workspace); Or-opt: nullptr
    uint32_t n;
    uint32_t max_passes;   // a descent stops (status 1) when it has run this many passes and still finds a move
};
// The end of a tour's descent, by the whole workgroup: the tour out, its length from the tour edges E and the run words
__device__ __forceinline__ void pop_finish(const PopArgs &A, const uint32_t *perm, const float *E, uint32_t moves, uint32_t passes, uint32_t status)
{
    const uint32_t n = A.n, tour = blockIdx.x;
    uint32_t *out = A.out_pos + (size_t)tour * n;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) out[k] = perm[k];
    if (threadIdx.x == 0) {
        // tour_length (distance_matrix.rs:235-245): the closing edge first, then the n - 1 edges in order, sequential f32
        float total = E[n - 1u];
        for (uint32_t k = 0; k + 1u < n; ++k) total += E[k];
        A.out_cost[tour] = total;
        A.out_run[4u * tour + 0u] = moves;
        A.out_run[4u * tour + 1u] = passes;
        A.out_run[4u * tour + 2u] = status;
        A.out_run[4u * tour + 3u] = 0u;
    }
}
// Threads per tour.  A pass has `units` wave-sized units of work (the caller may stop counting at 16), so a tour cannot use more
// waves than that; beyond it the widest workgroup of which the CU still holds its share of the batch (count / cus tours, 32 waves,
// the LDS at tour_lds bytes a tour) at once.
inline int pop_threads(uint64_t units, size_t tour_lds, uint32_t count, int cus, int lds_budget)
{
    const uint32_t per_cu = cus > 0 ? (count + (uint32_t)cus - 1u) / (uint32_t)cus : 1u;
    const size_t fit = (size_t)(lds_budget > 0 ? lds_budget : 0) / tour_lds;  // tours whose state one CU's LDS holds
    uint32_t share = per_cu < fit ? per_cu : (uint32_t)fit;
    if (share < 1u) share = 1u;
    int nt = 1024;
    while (nt > 64 && ((uint64_t)nt / 64u > units || (uint32_t)nt * share > 2048u)) nt >>= 1;
    return nt;
}
// one workgroup of `threads` per tour with tour_lds bytes of LDS; k_dm / k_xy: the kernel's matrix and coordinate forms
inline hipError_t launch_pop(void (*k_dm)(PopArgs), void (*k_xy)(PopArgs), const PopArgs &A, uint32_t count, int threads, size_t tour_lds, hipStream_t s)
{
    void (*const kern)(PopArgs) = A.dm ? k_dm : k_xy;
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(count), dim3(threads), tour_lds, s, A);
    return hipGetLastError();
}

// three_opt_pop.hip
size_t three_opt_pop_lds_bytes(uint32_t n);          // LDS of one tour's workgroup (either form)
uint32_t three_opt_pop_max_n(int lds_budget);        // largest n whose state fits
int three_opt_pop_threads(uint32_t n, uint32_t count, int cus, int lds_budget);
hipError_t launch_three_opt_pop(const PopArgs &A, uint32_t count, int threads, hipStream_t s);

// or_opt.hip
struct OrOptBest {
    uint32_t found, delta_bits, i, j, seg_len, reversed;
};
struct OrOptArgs {
    const float2 *xy;
    const float *dm;               // packed matrix or nullptr
    uint32_t *perm;                // [n] tour positions, updated in place by k_or_pick
    float2 *Pt;                    // [n] tour-ordered coordinates
    float *E;                      // [n] tour-edge lengths, E[n-1] = closing edge
    unsigned long long *partials;  // one packed key (two words: ~delta bits, loop-order index) per scan workgroup
    OrOptBest *best;
    uint32_t *scratch;             // [n] the pre-move tour of k_or_pick where it does not fit the LDS
    ScanRunState *run;             // a descent's batch state (nullptr: a single find_best_move)
    uint32_t *log;                 // [run->log_cap][4] applied moves: i, j, seg_len, reversed
    uint32_t n;
};
hipError_t launch_or_opt_pass(const OrOptArgs &A, bool dm, int apply, hipStream_t s, int lds_budget);
uint32_t or_opt_scan_blocks(uint32_t n);

// or_opt_lds.hip — a population of tours (PopArgs, Dt unused), the whole descent in LDS
size_t or_opt_lds_bytes(uint32_t n, bool dm);             // LDS of one tour's workgroup
uint32_t or_opt_lds_max_n(int lds_budget, bool dm);       // largest n whose state fits
int or_opt_lds_threads(uint32_t n, uint32_t count, int cus, int lds_budget, bool dm);
hipError_t launch_or_opt_lds(const PopArgs &A, uint32_t count, int threads, hipStream_t s);

// sim_anneal.hip — simulated annealing, one workgroup per chain
struct SaArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // chain b of the launch starts from init + b * init_stride (0: every chain from the same tour)
    uint32_t *out_pos;      // [count][n] the chains' last states
    float *out_cost;        // [count] their tour_length
    uint32_t *out_run;      // [count][4] accepted epochs, elements moved (64 bits), unused: added to by every launch of a schedule
    const float *temps;     // [e_end - e_begin] the temperatures of this launch's epochs
    uint32_t *log;          // optional: [log_cap][4] epoch, from, to, cost bits of every accepted epoch of the launch's chain 0
    uint64_t seed;
    uint32_t log_cap;
    uint32_t first_chain;   // stream id of the launch's chain 0
    uint32_t n;
    uint32_t init_stride;
    uint32_t e_begin, e_end;  // the epochs this launch runs
    uint32_t window;        // epochs evaluated at once (1 .. threads)
};
size_t sim_anneal_lds_bytes(uint32_t n);     // LDS of one chain's workgroup (either form)
uint32_t sim_anneal_lds_max_n(int lds_budget);
hipError_t launch_sim_anneal(const SaArgs &A, uint32_t count, int threads, hipStream_t s);
hipError_t launch_sa_selftest(const float *T, const float *oldc, const float *newc, const float *p, uint32_t count, uint32_t *out_accept,
                              float *out_criteria, hipStream_t s);

// tabu_search.hip — tabu search, one workgroup per chain
struct TabuArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // chain b of the launch starts from init + b * init_stride (0: every chain from the same tour)
    uint32_t *out_pos;      // [count][n] the chains' best routes
    float *out_cost;        // [count] their tour_length
    uint32_t *out_run;      // [count][8] new bests, candidates (64 bits), elements moved (64 bits), unused
    uint16_t *ring;         // [count][ring_stride] the tabu lists: n routes of n positions each
    uint32_t *hashes;       // [count][n] one hash per listed route
    uint32_t *log;          // optional: [log_cap][4] taken attempt, from, to, cost bits of every epoch of the launch's chain 0
    uint64_t seed;
    uint64_t ring_stride;   // elements between two chains' rings (>= n * n)
    uint32_t log_cap;
    uint32_t first_chain;   // stream id of the launch's chain 0
    uint32_t n;
    uint32_t init_stride;
    uint32_t epochs;        // the epochs to run (the reference's `epochs` + 1)
    uint32_t full_compare;  // every membership test compares whole routes (TL_FLAG_TABU_FULL_COMPARE)
};
size_t tabu_search_lds_bytes(uint32_t n);    // LDS of one chain's workgroup (either form)
uint32_t tabu_search_lds_max_n(int lds_budget);
hipError_t launch_tabu_search(const TabuArgs &A, uint32_t count, int threads, hipStream_t s);

// hill_climb.hip — the stochastic hill climb, one workgroup per chain
struct HillArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // chain b of the launch starts from init + b * init_stride (0: every chain from the same tour)
    uint32_t *out_pos;      // [count][n] the chains' best routes
    float *out_cost;        // [count] their tour_length
    uint32_t *out_run;      // [count][4] acceptances, elements moved (64 bits), restarts
    uint32_t *log;          // optional: [log_cap][4] the events of the launch's chain 0 in order: epoch, from, to, cost bits of an
                            // acceptance; epoch, 0xFFFFFFFF, 0, 0 of a restart
    uint64_t seed;
    uint32_t log_cap;
    uint32_t first_chain;   // stream id of the launch's chain 0
    uint32_t n;
    uint32_t init_stride;
    uint32_t epochs;        // the epochs to run (the reference's `epochs` + 1)
    uint32_t platoo;        // platoo_epochs (0: never a restart)
    uint32_t window;        // epochs evaluated at once (1 .. threads)
};
size_t hill_climb_lds_bytes(uint32_t n);     // LDS of one chain's workgroup (either form)
uint32_t hill_climb_lds_max_n(int lds_budget);
hipError_t launch_hill_climb(const HillArgs &A, uint32_t count, int threads, hipStream_t s);

// genetic.hip — the genetic algorithm, the run a grid dimension, two launches per generation
struct GaArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // the initial tour (from_cities_seeded), or nullptr (from_cities)
    uint16_t *pop[2];       // [runs][pop_stride] the populations, current and next: up to n routes of n cities each
    float *fit[2];          // [runs][n] their fitness values
    uint32_t *order;        // [runs][n] the individuals of the current population, sorted (stable, fitness descending)
    float *prefix;          // [runs][n + 1] the roulette's running sum over the sorted population
    uint32_t *state;        // [runs][8] best fitness bits, improved generations, mutations, status, best index
    uint32_t *out_pos;      // [runs][n] the best route of the last population
    float *out_cost;        // [runs] its tour_length
    uint32_t *log;          // optional: [log_cap][4] best index, fitness bits, tour_length bits, population length per generation of run 0
    uint32_t *route_log;    // optional: [route_cap][n] the best route of the first generations of run 0
    uint64_t seed;
    uint64_t pop_stride;    // elements between two runs' populations (>= n * n)
    uint32_t log_cap, route_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, n_elite;
    float p_mut;
    uint32_t generation;    // breed: the generation being bred; rank: the generations bred so far
    uint32_t len;           // the length of the current population
    uint32_t src;           // which of pop / fit is the current one
    uint32_t last;          // rank: no generation follows — write the result
};
size_t genetic_lds_bytes(uint32_t n);        // LDS of one workgroup (either form)
uint32_t genetic_max_n(int lds_budget);
int genetic_threads(uint32_t n);
hipError_t launch_ga_init(const GaArgs &A, uint32_t runs, hipStream_t s);
hipError_t launch_ga_rank(const GaArgs &A, uint32_t runs, hipStream_t s);
hipError_t launch_ga_breed(const GaArgs &A, uint32_t runs, uint32_t next_len, hipStream_t s);
hipError_t launch_ga_selftest_crossover(const uint16_t *p1, const uint16_t *p2, uint32_t n, uint32_t from, uint32_t to, uint16_t *out1, uint16_t *out2,
                                        hipStream_t s);

// ant_colony.hip — the ant colony solver, the run (colony) a grid dimension, three launches per epoch
struct AcoArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // the initial tour(s), or nullptr (a shuffle)
    uint32_t init_stride;   // 0: one tour for every run, n: one per run
    float *tau, *eta, *w;   // [runs][mat_stride] pheromone, eta^beta, tau^alpha eta^beta
    uint16_t *tour, *succ, *pred;  // [runs][num_ants][n] every ant's tour by position, and its successor / predecessor by city
    float *cost;            // [runs][num_ants] the ants' tour lengths
    uint32_t *start, *fb;   // [runs][num_ants] their start cities and their counts of fallback selections
    uint32_t *state;        // [runs][8] best cost bits, improvements, fallback selections (lo), tau0 bits, tau_min bits, fallbacks (hi)
    uint32_t *out_pos;      // [runs][n] the best tour so far
    float *out_cost;        // [runs] its cost
    uint32_t *log;          // optional: [log_cap][3 num_ants] cost bits, start cities, fallback counts per epoch of run 0
    uint32_t *route_log;    // optional: [route_cap][n + 3] epoch, ant, cost bits, tour: the start tour, then every improving ant of run 0
    uint64_t seed;
    uint64_t mat_stride;    // elements between two runs' matrices (>= n * n)
    uint32_t log_cap, route_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, num_ants;
    uint32_t epoch;
    uint32_t pre;           // update: the deposit of the initial tour before epoch 0 (no evaporation; one "ant", or none)
    float alpha, beta, rate;
};
size_t ant_colony_lds_bytes(uint32_t n);     // LDS of a construct workgroup
uint32_t ant_colony_max_n(int lds_budget);
int ant_colony_threads();
hipError_t launch_aco_init(const AcoArgs &A, uint32_t runs, hipStream_t s);    // start tour, its cost, tau0; then tau and eta
hipError_t launch_aco_construct(const AcoArgs &A, uint32_t runs, hipStream_t s);
hipError_t launch_aco_best(const AcoArgs &A, uint32_t runs, hipStream_t s);
hipError_t launch_aco_update(const AcoArgs &A, uint32_t runs, int lds_budget, hipStream_t s);
hipError_t launch_aco_selftest_select(const float *weights, const float *eta, const uint32_t *visited, uint32_t n, float r1, float r2, uint32_t *out,
                                      hipStream_t s);

// particle_swarm.hip — the particle swarm solver, the run (swarm) a grid dimension, two launches per epoch
struct PsoArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // the initial tour(s) of particle 0, or nullptr (a shuffle)
    uint32_t init_stride;   // 0: one tour for every run, n: one per run
    uint16_t *pos[2];       // [runs][particles][n] the positions before and after the epoch's moves (pos[src], pos[src ^ 1])
    uint16_t *pbest;        // [runs][particles][n]
    uint16_t *gbest;        // [runs][n]
    uint32_t *vel[2];       // [runs][particles][vmax] the velocities, a swap (i, j) as i | j << 16
    uint32_t *vlen[2];      // [runs][particles] their lengths
    float *cost;            // [runs][particles] tour_length of the moved positions
    float *pcost;           // [runs][particles] pbest_cost
    uint32_t *state;        // [runs][8] gbest cost bits, gbest improvements
    uint32_t *out_pos;      // [runs][n] gbest after the last epoch
    float *out_cost;        // [runs] its cost
    uint32_t *log;          // optional: [log_cap][4] epoch, particle, cost bits, route index: the start gbest, then every improvement of run 0
    uint32_t *route_log;    // optional: [route_cap][n] their routes
    uint32_t *epoch_log;    // optional: [epoch_cap][2 particles] every particle's cost bits, then every particle's velocity length, of run 0
    uint64_t seed;
    uint32_t log_cap, route_cap, epoch_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, particles, vmax;
    uint32_t epoch, epochs;
    uint32_t src;           // which of pos / vel / vlen holds the state before the epoch
    uint32_t last;          // commit: no epoch follows — write the result
};
size_t particle_swarm_lds_bytes(uint32_t n);  // LDS of one workgroup (every kernel)
uint32_t particle_swarm_max_n(int lds_budget);
int particle_swarm_threads(uint32_t n);
hipError_t launch_pso_init(const PsoArgs &A, uint32_t runs, hipStream_t s);    // start positions and costs, then the first minimum
hipError_t launch_pso_move(const PsoArgs &A, uint32_t runs, hipStream_t s);    // every particle against the epoch-start gbest
hipError_t launch_pso_commit(const PsoArgs &A, uint32_t runs, hipStream_t s);  // the particles in index order; after an improvement the later ones again
hipError_t launch_pso_selftest_swap_sequence(const uint16_t *from, const uint16_t *to, uint32_t n, uint32_t count, uint32_t *out_pairs, uint32_t *out_len,
                                             hipStream_t s);

// cuckoo_search.hip — the cuckoo search solver, the run a grid dimension, two launches per epoch
struct CsArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // the initial tour(s) of nest 0, or nullptr (a shuffle)
    uint32_t init_stride;   // 0: one tour for every run, n: one per run
    uint16_t *nest;         // [runs][nests][n]
    uint16_t *fly;          // [runs][nests][n] cuckoo c's flight, staged
    uint16_t *repl;         // [runs][nests][n] nest c's replacement, staged where its abandonment trial succeeds
    uint16_t *best;         // [runs][n]
    float *cost;            // [runs][nests] the nests' costs
    float *fcost;           // [runs][nests] the staged flights' costs
    float *rcost;           // [runs][nests] the staged replacements' costs
    uint32_t *fk;           // [runs][nests] the flights' lengths k
    uint32_t *state;        // [runs][8] best cost bits, best improvements
    uint32_t *out_pos;      // [runs][n] best after the last epoch
    float *out_cost;        // [runs] its cost
    uint32_t *log;          // optional: [log_cap][4] epoch, source, cost bits, route index: the start best, then every improvement of run 0
    uint32_t *route_log;    // optional: [route_cap][n] their routes
    uint32_t *epoch_log;    // optional: [epoch_cap][4 nests] of run 0: nest cost bits | k | target (bit 31 accepted, bit 30 flown again) | abandoned
    uint64_t seed;
    double pa;
    uint32_t log_cap, route_cap, epoch_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, nests;
    uint32_t epoch;
    uint32_t last;          // commit: no epoch follows — write the result
};
size_t cuckoo_search_lds_bytes(uint32_t n);  // LDS of one workgroup (every kernel)
uint32_t cuckoo_search_max_n(int lds_budget);
int cuckoo_search_threads(uint32_t n);
hipError_t launch_cs_init(const CsArgs &A, uint32_t runs, hipStream_t s);    // start nests and costs, then the first minimum
hipError_t launch_cs_fly(const CsArgs &A, uint32_t runs, hipStream_t s);     // every flight from the epoch-start nests, every replacement
hipError_t launch_cs_commit(const CsArgs &A, uint32_t runs, hipStream_t s);  // the cuckoos in order (a flight from an overwritten nest again), then the abandonments
hipError_t launch_cs_selftest_levy(const uint64_t *words, uint32_t count, uint32_t n, uint64_t *out_bits, uint32_t *out_k, uint32_t *out_resamples, hipStream_t s);
hipError_t launch_cs_selftest_reversals(const uint16_t *tours, const uint32_t *pairs, const uint32_t *lens, uint32_t n, uint32_t kcap, uint32_t count,
                                        uint16_t *out, hipStream_t s);

// flower_pollination.hip — the flower pollination solver, the run a grid dimension, two launches per epoch
struct FpaArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // the initial tour(s) of flower 0, or nullptr (a shuffle)
    uint32_t init_stride;   // 0: one tour for every run, n: one per run
    uint16_t *flower;       // [runs][flowers][n]
    uint16_t *stage;        // [runs][flowers][n] flower i's move, staged
    uint16_t *gbest;        // [runs][n]
    float *cost;            // [runs][flowers] the flowers' costs
    float *scost;           // [runs][flowers] the staged moves' costs
    uint32_t *slen;         // [runs][flowers] the staged moves' sequence length | prefix length << 16
    uint32_t *state;        // [runs][8] gbest cost bits, gbest improvements
    uint32_t *out_pos;      // [runs][n] gbest after the last epoch
    float *out_cost;        // [runs] its cost
    uint32_t *log;          // optional: [log_cap][4] epoch, flower, cost bits, route index: the start gbest, then every improvement of run 0
    uint32_t *route_log;    // optional: [route_cap][n] their routes
    uint32_t *epoch_log;    // optional: [epoch_cap][4 flowers] of run 0: cost bits | kind, j, k | lengths | accepted, built again
    uint64_t seed;
    double switch_prob;
    uint32_t log_cap, route_cap, epoch_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, flowers;
    uint32_t epoch;
    uint32_t last;          // commit: no epoch follows — write the result
};
size_t flower_pollination_lds_bytes(uint32_t n);  // LDS of one workgroup (every kernel)
uint32_t flower_pollination_max_n(int lds_budget);
int flower_pollination_threads(uint32_t n);
hipError_t launch_fpa_init(const FpaArgs &A, uint32_t runs, hipStream_t s);    // start flowers and costs, then the first minimum
hipError_t launch_fpa_move(const FpaArgs &A, uint32_t runs, hipStream_t s);    // every flower's move against the epoch-start state
hipError_t launch_fpa_commit(const FpaArgs &A, uint32_t runs, hipStream_t s);  // the flowers in order (a move whose inputs have changed is built again)
hipError_t launch_fpa_selftest_pollinate(const uint16_t *flower, const uint16_t *source, const uint16_t *target, const uint32_t *prefix, uint32_t n, uint32_t count,
                                         uint16_t *out, uint32_t *out_len, hipStream_t s);

// gravitational_search.hip — the gravitational search solver, the run a grid dimension, a span of epochs per launch
struct GsaArgs {
    const float2 *xy;       // n cities, city order (coordinate form)
    const float *dm_full;   // the matrix expanded to row-major n x n, or nullptr
    const uint32_t *init;   // the initial tour(s) of agent 0, or nullptr (a shuffle)
    uint32_t init_stride;   // 0: one tour for every run, n: one per run
    uint16_t *pos;          // [runs][agents][n] the positions
    uint16_t *gbest;        // [runs][n]
    float *cost;            // [runs][agents] the agents' costs
    double *mass;           // [runs][agents] the masses of the epoch being walked
    uint16_t *kbest;        // [runs][agents] the agents by rank; the first ceil(agents / 2) are read
    uint32_t *state;        // [runs][8] gbest cost bits, gbest improvements, 1 where the reference would have panicked
    uint32_t *out_pos;      // [runs][n] gbest after the last epoch
    float *out_cost;        // [runs] its cost
    uint32_t *log;          // optional: [log_cap][4] epoch, agent, cost bits, route index: the start gbest, then every improvement of run 0
    uint32_t *route_log;    // optional: [route_cap][n] their routes
    uint32_t *epoch_log;    // optional: [epoch_cap][3 agents + 2] of run 0: cost bits | velocity length | live pulls | g's bits, low word first
    uint64_t seed;
    uint32_t log_cap, route_cap, epoch_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, agents, vmax;
    uint32_t e0, e1, epochs;  // the span [e0, e1) of the schedule of `epochs` epochs
    uint32_t last;          // no launch follows — write the result
};
size_t gravitational_search_lds_bytes(uint32_t n);  // LDS of one workgroup (every kernel)
uint32_t gravitational_search_max_n(int lds_budget);
int gravitational_search_threads(uint32_t n);
hipError_t launch_gsa_init(const GsaArgs &A, uint32_t runs, hipStream_t s);    // start positions and costs, then the first minimum
hipError_t launch_gsa_epochs(const GsaArgs &A, uint32_t runs, hipStream_t s);  // the epochs [e0, e1): one workgroup per run, the agents in order
hipError_t launch_gsa_selftest_pull(const uint16_t *from, const uint16_t *to, const uint32_t *want, uint32_t n, uint32_t count, uint32_t *out_pairs,
                                    uint32_t *out_len, hipStream_t s);

// kohonen_som.hip — the Kohonen self-organising map solver, the run a grid dimension, a span of epochs per launch
struct SomEpoch;  // som_spec.h
struct SomArgs {
    const double *cities;   // the normalised cities: x[n] | y[n]
    const double *ring0;    // the start ring x[M] | y[M], the same for every run
    double *ring;           // [runs][2 M] a run's ring, x[M] | y[M]: loaded at a span's start, stored at its end
    const SomEpoch *sched;  // [epochs] the schedule, epoch t at t - 1
    uint32_t *log;          // optional: [log_cap][2] (city, bmu) of epoch t at row t - 1, run 0 of the launch
    const float2 *xy;       // the extraction's cost: n cities (coordinate form)
    const float *dm_full;   // or the matrix expanded to row-major n x n
    uint32_t *bmu;          // [runs][n] the extraction's first-minimum neuron of every city
    double *bdist;          // [runs][n] and its distance
    float *edge;            // [runs][n] the tour's edge lengths
    uint32_t *out_pos;      // [runs][n] the extracted tour
    float *out_cost;        // [runs] its cost
    uint64_t seed;
    uint32_t log_cap;
    uint32_t first_run;     // stream id of the launch's run 0
    uint32_t n, M;
    uint32_t t0, t1;        // the span [t0, t1) of the epochs 1 .. epochs
    uint32_t fresh;         // the span begins the run: the ring is ring0
};
constexpr size_t kSomLdsFixedBytes = 512;  // the reduction's double-buffered slots of up to 16 waves
inline size_t kohonen_som_lds_bytes(uint32_t M, bool lds_form) { return kSomLdsFixedBytes + (lds_form ? 16 * (size_t)M : 0); }
int kohonen_som_threads(uint32_t M);
hipError_t launch_som_train(const SomArgs &A, uint32_t runs, bool lds_form, hipStream_t s);  // the epochs [t0, t1): one workgroup per run
hipError_t launch_som_extract(const SomArgs &A, uint32_t runs, hipStream_t s);               // every run's tour and cost from its ring
hipError_t launch_som_selftest_bmu(const SomArgs &A, int threads, bool lds_form, hipStream_t s);  // the training's BMU of cities 0 .. n - 1 into A.bmu, on A.ring as it is

// fourier_curve.hip — the Fourier-curve solver, the job (an option set) a grid dimension, a span of gradient steps per launch
struct FourierJob {          // one option set of a batch
    double lambda, lambda_decay, lr_over_n;
    uint32_t k_max, m, epochs;
    uint32_t total;          // k_max epochs: the job's steps
    uint32_t off_c;          // where the job's 2 (2 k_max + 1) coefficient doubles begin in FourierArgs::coeffs
    uint32_t off_m;          // where its m samples begin in FourierArgs::basis (pairs of f64) and ::g32 (pairs of f32)
};
struct FourierArgs {
    const FourierJob *jobs;  // [J]
    const float2 *cities;    // n cities as the solver reads them
    double *coeffs;          // every job's coefficients (re, im pairs): loaded at a span's start, stored at its end
    double *basis;           // every job's table E: the workspace form's (and the decode's) copy
    float2 *g32;             // every job's curve as f32: the decode's (and the self-test's) samples
    uint32_t *sidx;          // [J][n] every city's nearest sample: the workspace form's array, the decode's in either form
    const float2 *xy;        // the decode's cost: n cities (coordinate form)
    const float *dm_full;    // or the matrix expanded to row-major n x n
    float *edge;             // [J][n] the tour's edge lengths
    uint32_t *out_pos;       // [J][n] the decoded tour
    float *out_cost;         // [J] its cost
    uint32_t *log;           // optional: [log_cap][n] every city's sample index at step t, job 0 of the launch
    double *stage_c;         // optional: [k_max][2 L] job 0's coefficients at the end of every stage
    const double *gamma_in;  // the self-test's curve: m pairs
    uint32_t log_cap;
    uint32_t n;
    uint32_t s0, s1;         // the span [s0, s1) of the steps; a job runs what of it lies below its total
    uint32_t chunk;          // cities whose gradient terms are formed at once
    uint32_t max_l, max_m;   // the largest 2 k_max + 1 and m of the launch: the LDS layout
};
size_t fourier_curve_lds_bytes(uint32_t n, uint32_t max_l, uint32_t max_m, uint32_t chunk, bool lds_form);
int fourier_curve_threads(uint32_t n, uint32_t m);  // about 32 (city, sample) pairs a lane in whole waves, 256 .. 1024
hipError_t launch_fourier_steps(const FourierArgs &A, uint32_t jobs, int threads, bool lds_form, hipStream_t s);  // the steps [s0, s1): one workgroup per job
hipError_t launch_fourier_decode(const FourierArgs &A, uint32_t jobs, hipStream_t s);                                // every job's tour and cost from its coefficients
hipError_t launch_fourier_selftest_search(const FourierArgs &A, int threads, hipStream_t s);  // the steps' search alone on A.gamma_in (m = max_m) into A.sidx

// one_tree_bound.hip — the Held-Karp lower bound, the job (an option set) a grid dimension, a span of ascent iterations per launch
struct OneTreeJob;    // one_tree_spec.h
struct OneTreeState;  // one_tree_spec.h
struct OneTreeArgs {
    const OneTreeJob *jobs;  // [J]
    OneTreeState *state;     // [J] the ascent between two launches
    const float2 *xy;        // coordinate form
    const float *dm_full;    // matrix form: the expanded n x n matrix (then xy is not read)
    double *pi, *best_pi;    // [J][n] the penalties between two launches; those of the best 1-tree
    uint32_t *best_par;      // [J][n] the best 1-tree's parents
    uint32_t *tour_par;      // [J][n] the parents of the 1-tree that was a tour
    double *log;             // [J][log_cap][3] (L_k, sum of g^2, lambda) or nullptr
    uint32_t log_cap;
    uint32_t n;
    uint32_t span;           // iterations of this launch
};
size_t one_tree_lds_bytes(uint32_t n);     // key, pi, parent, degree: 24 n bytes
uint32_t one_tree_max_n(int lds_bytes);    // the largest n whose state fits
int one_tree_threads(uint32_t n);          // n in whole waves, 64 .. 1024
hipError_t launch_one_tree_ascent(const OneTreeArgs &A, uint32_t jobs, int threads, hipStream_t s);  // one workgroup per job

// alpha_candidates.hip — alpha-nearness under given penalties, one workgroup per source city, its beta / alpha row in LDS
struct AlphaNode;  // alpha_spec.h
struct AlphaArgs {
    const float2 *xy;           // coordinate form
    const float *dm_full;       // matrix form: the expanded n x n matrix (then xy is not read)
    const double *pi;           // [n]
    const AlphaNode *by_pos;    // [n] the 1-tree's positions: parent, w(v, parent)
    const AlphaNode *by_level;  // [n - 1] the same in level order from Prim's start
    const uint32_t *level_at;   // [levels + 1] where a level begins in by_level
    uint32_t *out_cand;         // [n][kk]
    double *out_alpha;          // [n][kk] or nullptr
    uint32_t n, kk, levels;
    uint32_t root, nb0, nb1;    // the special position and its two neighbours in the order chosen
};
size_t alpha_rows_lds_bytes(uint32_t n);    // w and beta / alpha of a row: 16 n bytes
uint32_t alpha_rows_max_n(int lds_bytes);   // the largest n whose row fits
int alpha_rows_threads(uint32_t n);         // n in whole waves, 64 .. 256
hipError_t launch_alpha_rows(const AlphaArgs &A, int threads, hipStream_t s);  // one workgroup per source

// lk.hip
struct LkState {          // device-side state machine of the multi-CU LK variant
    uint32_t key;            // min pair index with a valid chain in the current scan (0xFFFFFFFF: none)
    uint32_t finished;
    uint32_t stage;          // 0: initial lk_pass, 1: ILS epochs
    uint32_t epoch, platoo;
    float best_dist;
    uint64_t draws;
    uint64_t scans, searches, moves, exchanged;
    uint32_t window;         // pairs [0, window) the next scan looks at (a prefix: the lowest pair index wins anyway)
    uint32_t applied;        // k_lk_control applied a move into `alt`: k_lk_rebuild copies it back and rebuilds pos / next / prev
    uint32_t key2[2];        // chip-wide step: the scan's key, double-buffered by round parity
    uint32_t flip, flip_next;  // chip-wide step: which tour buffer is current (0: tour, 1: alt); handed over by the next scan
    uint32_t snaps;          // best tours recorded so far (LkArgs::snap; counted on beyond snap_cap)
    uint32_t pass_moves;     // moves of the lk_pass in progress (finished = 2 beyond lk_pass_cap: the pass is cycling)
};
struct LkArgs {
    const float2 *xy;
    const uint32_t *cand;   // [n][k] candidate lists, ascending distance
    uint32_t *tour;         // [n] working tour (in: initial tour)
    uint32_t *alt;          // [n] scratch for chain application
    uint32_t *pos;          // [n] rank of city
    uint32_t *next;         // [n]
    uint32_t *prev;         // [n]
    uint32_t *city_ids;     // [n] scan order snapshot of a pass
    uint32_t *best;         // [n] out: best tour
    uint64_t *counters;     // scans, searches, moves, exchanged edges
    LkState *state;         // multi-CU variant
    uint32_t *chains;       // multi-CU variant: [2n][kLkMaxChain + 2] chain slots
    uint32_t *pairmin;      // split scan: [2n] minimum sub-search index with a chain (0xFFFFFFFF: none); nullptr = unsplit scan
    uint32_t *subchains;    // split scan: [2n * k(k+1)][16] the chain each successful sub-search found (len, cities), or nullptr:
                            // k_lk_scan_pick then reads the winner's chain instead of walking it again
    uint64_t seed;
    uint32_t n, k, max_depth, epochs, platoo_epochs;
    uint32_t lds_budget;    // LDS bytes a scan workgroup may use for its xy/next copies
    uint32_t split_levels;  // split scan: 2 = k(k+1) sub-searches per pair, 3 = k(k+1)^2
    uint32_t chip_step;     // fused scan at n >= 1500: k_lk_control<true> (state machine + move application, chip-wide) replaces
                            // k_lk_control<false> + k_lk_rebuild
    uint32_t parity;        // round & 1 (set per launch)
    uint32_t fused_pick;    // split scan, one workgroup per pair: the workgroup picks its first chain and validates it itself
                            // (no k_lk_scan_pick launch, no pairmin / subchains traffic)
    uint32_t *snap;         // optional [snap_cap][n]: every best tour the search settles on, in order — what the reference sends as
    float *snap_dist;       // PathUpdate(best_tour, best_dist) (lin_kernighan.rs:71,90) — and its best_dist; nullptr = not recorded
    uint32_t snap_cap;
    uint32_t snap_ring;      // snap is a ring of snap_cap slots (tl_lk_live) instead of a list of the first snap_cap
    uint32_t persist_blocks; // fused three-level scan: workgroups of the persistent grid (k_lk_scan_persist); 0 = one workgroup per pair
    // k_lk_ils (the LDS-resident single-workgroup ILS of a small instance): records per level queue (lk_ils_qcap), scans per launch,
    // and how many snapshots of the ring the host has taken so far (a slice ends when the ring is full of undelivered ones)
    // the packed view of the chip-wide scan (lk.hip LkViewPk): candidate ids with their distances, successor records; nullptr = classic view
    uint2 *candd;
    float4 *nx;
    uint32_t ils_qcap, ils_slice, snap_delivered;
    uint32_t ils_threads;    // 0: by n (256 up to n = 200, else 1024); tuning: 256 / 512 / 1024
    // speculative epochs (k_lk_ils mode 2 + k_lk_ils_commit): ils_P workgroups = ils_P consecutive epochs kicked from the same best tour
    uint32_t ils_mode, ils_P;
    float *ils_dcand;        // [n][k] the candidates' distances (written by the first-pass launch, read by the epoch launches)
    uint32_t *ils_ep_tour;   // [ils_P][n] the tour each epoch ends on
    float *ils_ep_dist;      // [ils_P] its tour_distance
    uint64_t *ils_ep_cnt;    // [ils_P][4] scans, searches, moves, exchanged edges of the epoch
    // the population launch (k_lk_ils_pop<NT>): state, tour, best and city_ids are arrays of `count` rows and `counters` holds the runs'
    // seeds, run b's in counters[b] (no field of its own: a longer LkArgs moves the hidden kernel arguments of the chip-wide kernels)
};
// form: 0 = default (16 lanes per city up to n = 32 K, 4 beyond), 4 = four lanes per city, 1 = one lane per city
hipError_t launch_knn(const float2 *xy, uint32_t n, uint32_t k, uint32_t *cand, hipStream_t s, int form = 0);
hipError_t launch_nn_seed(const float2 *xy, uint32_t n, const uint32_t *cand, uint32_t k, uint32_t *path, int lds_bytes, hipStream_t s);
hipError_t launch_nn_seed_dm(const float *dm, uint32_t n, uint32_t *path, int lds_bytes, hipStream_t s);
// small: the LDS-resident form (n (36 + 4k) bytes of LDS, lk_small_lds_bytes) with `threads` in {64, 256, 1024}
hipError_t launch_lk_solve(const LkArgs &G, hipStream_t s, bool small = false, int threads = 1024);
size_t lk_small_lds_bytes(uint32_t n, uint32_t k);
hipError_t launch_lk_begin(const LkArgs &G, hipStream_t s);
hipError_t launch_lk_round(const LkArgs &G, hipStream_t s, uint32_t round);
uint32_t lk_ils_qcap(uint32_t n, uint32_t k, uint32_t max_depth, size_t lds_budget);  // > 0: k_lk_ils applies (records per level queue)
size_t lk_ils_lds_bytes(uint32_t n, uint32_t k, uint32_t max_depth, uint32_t qcap);   // LDS of one k_lk_ils workgroup
hipError_t launch_lk_ils(const LkArgs &G, hipStream_t s);                             // mode 0 / 1: one slice of G.ils_slice scans; mode 2: ils_P epochs
hipError_t launch_lk_ils_commit(const LkArgs &G, hipStream_t s);                      // the verdict over a batch of epochs
uint32_t lk_ils_threads(uint32_t n);                                                   // its width by n: 256 up to TL_ILS_SMALL_N, else 1024
hipError_t launch_lk_pop_prepare(const LkArgs &G, uint32_t count, bool share_start, hipStream_t s);  // a population's ils_dcand, and its shared start tour into every row
hipError_t launch_lk_ils_pop(const LkArgs &G, uint32_t count, hipStream_t s);         // one slice of G.ils_slice scans of every unfinished run, a workgroup per run
size_t lk_chain_slot_words();
size_t lk_sub_slot_words();
uint32_t lk_max_depth();  // the build's compile-time recursion bound (6)

}  // namespace tl
// lk_deep.hip — lk.hip compiled with chains of up to 16 exchanges (max_depth 7..16)
namespace tl_lk_deep {
hipError_t launch_lk_solve(const tl::LkArgs &G, hipStream_t s, bool small = false, int threads = 1024);
size_t lk_small_lds_bytes(uint32_t n, uint32_t k);
hipError_t launch_lk_begin(const tl::LkArgs &G, hipStream_t s);
hipError_t launch_lk_round(const tl::LkArgs &G, hipStream_t s, uint32_t round);
uint32_t lk_ils_qcap(uint32_t n, uint32_t k, uint32_t max_depth, size_t lds_budget);
size_t lk_ils_lds_bytes(uint32_t n, uint32_t k, uint32_t max_depth, uint32_t qcap);
hipError_t launch_lk_ils(const tl::LkArgs &G, hipStream_t s);
hipError_t launch_lk_ils_commit(const tl::LkArgs &G, hipStream_t s);
uint32_t lk_ils_threads(uint32_t n);
hipError_t launch_lk_pop_prepare(const tl::LkArgs &G, uint32_t count, bool share_start, hipStream_t s);
hipError_t launch_lk_ils_pop(const tl::LkArgs &G, uint32_t count, hipStream_t s);
size_t lk_chain_slot_words();
size_t lk_sub_slot_words();
uint32_t lk_max_depth();
}  // namespace tl_lk_deep
namespace tl {

// kdtree.hip — build_candidates through the reference's kd-tree (kdtree.rs)
struct KdNode {
    float x, y;           // the node's point
    int32_t left, right;  // node indices, -1 = None
    uint32_t pos;         // its position in the city array (= KDPoint.id of build_candidates' cities)
    uint32_t coord;       // depth % 2
};
size_t kdtree_build_ws_bytes(uint32_t n, size_t *cub_bytes_out);
hipError_t kdtree_build_dev(const float2 *xy, uint32_t n, void *ws, KdNode *nodes, hipStream_t s);  // root = node n / 2
hipError_t launch_knn_kdtree(const KdNode *nodes, const float2 *xy, uint32_t n, uint32_t k, uint32_t *cand, hipStream_t s);

// dm_build.hip
hipError_t launch_dm_build(const float2 *xy, uint32_t n, int dist, int layout, float *out, hipStream_t s);
hipError_t launch_dm_compare(const float2 *xy, uint32_t n, const float *dm, uint32_t *differs, hipStream_t s);
hipError_t launch_selftest_sqrt(uint32_t first_bits, uint64_t count, unsigned long long *mismatches, uint32_t *first_bad, hipStream_t s);
hipError_t launch_tour_length(const float2 *xy, const float *dm, uint32_t n, const uint32_t *perm,
                              float *out_cost, hipStream_t s);

// greedy_edge.hip — greedy-edge and savings construction, and Christofides' greedy matching, in bands of at most `cap` sorted
// keys
enum GreedyKey : int {
    kGeKeyLength = 0,    // greedy-edge: f32::total_cmp of the edge length
    kGeKeySavings = 1,   // savings: descending total_cmp of the saving against w.dh
    kGeKeyMatching = 2,  // Christofides' matching: partial_cmp of the length (-0.0 = +0.0), NaN above +inf; capacity 1, no cycle test
};
struct GreedyWs {
    uint64_t *keys;       // [cap] the band's keys
    uint32_t *hist;       // [4096] digit histogram
    uint32_t *state;      // accepted edges, edges examined (u64), keys in the band, free cities
    uint16_t *end;        // [n] fragment-end table between bands
    uint16_t *free;       // [n] the free cities (degree < 2), position order
    uint32_t *slots;      // [n][2] both neighbours of a city in acceptance order
    uint32_t *succ[2];    // [2n] list ranking of the directed arcs (double-buffered)
    uint32_t *dte[2];
    float *dh;            // [n] savings only: d(hub, k), +0.0 at the hub (after every greedy-edge field: those keep their offsets)
    uint32_t cap;
};
uint32_t greedy_band_cap(int lds_bytes);  // keys per band: a power of two whose keys fit one workgroup's LDS (16 384 on 160 KB)
size_t greedy_ws_bytes(uint32_t n, uint32_t cap);
GreedyWs greedy_ws_layout(void *ws, uint32_t n, uint32_t cap);
hipError_t launch_greedy_init(const GreedyWs &w, uint32_t n, hipStream_t s);
// savings: w.dh[k] = d(hub, k) — dist() in coordinate form (the matrix builder's bits), a packed-triangle gather in matrix form
hipError_t launch_savings_dh(const GreedyWs &w, const float2 *xy, const float *dm, uint32_t n, uint32_t hub, hipStream_t s);
hipError_t launch_greedy_hist(const GreedyWs &w, const float2 *xy, const float *dm, uint32_t f, uint64_t t_prev, uint64_t prefix,
                              uint32_t shift, uint32_t width, int blocks, GreedyKey key, hipStream_t s);
// compact the keys in (t_lo, t_hi], sort them, walk them.  target: kGeKeyMatching only — the walk stops at that many pairs and
// lists them in w.slots (pair a at [2a], [2a + 1]); the other two stop at n edges.
hipError_t launch_greedy_band(const GreedyWs &w, const float2 *xy, const float *dm, uint32_t n, uint32_t f, uint64_t t_lo, uint64_t t_hi,
                              int blocks, GreedyKey key, uint32_t target, hipStream_t s);
hipError_t launch_greedy_path(const GreedyWs &w, uint32_t n, uint32_t *out_pos, hipStream_t s);

// christofides.hip — Prim's tree and the odd vertices of Christofides.  The fields alias the list-ranking part
// of a GreedyWs (succ / dte: Christofides ranks no list) and the words of its state block behind the band state.
struct ChrWs {
    float *key;        // [n] Prim's keys where they do not fit LDS
    uint16_t *par;     // [n] ... and the tentative parents
    uint16_t *parent;  // [n] out: parent[v], 0xFFFF = none (position 0, or a vertex no finite distance reaches)
    uint16_t *order;   // [n] out: order[r] = the vertex that joined in round r
    uint32_t *status;  // [0] != 0: a vertex other than 0 joined without a parent, [1] the first such position
};
ChrWs chr_ws_layout(const GreedyWs &w, uint32_t n);
// The whole tree in one launch of one workgroup (prim_mst, christofides.rs:75-114)
hipError_t launch_chr_prim(const ChrWs &cw, const float2 *xy, const float *dm, uint32_t n, int lds_bytes, hipStream_t s);
// Degrees from cw.parent: the odd vertices go to w.free in position order, w.end holds c for them and "full" for every other
// city, w.state is reset with state[4] = their number
hipError_t launch_chr_odd(const GreedyWs &w, const ChrWs &cw, uint32_t n, hipStream_t s);

// bellman_karp.hip — the Bellman-Held-Karp exact solver, 1 <= n <= TL_BHK_MAX_N
struct BhkWs {
    float *dsq;       // [32][32] d(a, b) of the instance, +0.0 on the diagonal and outside it
    uint32_t *binom;  // [32][32] C(a, b), uploaded by the host
    float *out_f;     // [0] tour_length of the route, [1] the optimum
    uint32_t *out_u;  // [0] 1 if the route is a permutation
    float *opt;       // [2^(n-1)][32] the table, mask-major
};
size_t bhk_ws_bytes(uint32_t n);
BhkWs bhk_ws_layout(void *ws, uint32_t n);
void bhk_binomials(uint32_t *out);  // host: the [32][32] table w.binom holds
hipError_t launch_bhk_init(const BhkWs &w, const float2 *xy, const float *dm, uint32_t n, hipStream_t s);
// layer p (2 <= p <= n - 1): every opt[S][c] with |S| = p from the layer below; count = C(n - 1, p)
hipError_t launch_bhk_layer(const BhkWs &w, uint32_t n, uint32_t p, uint32_t count, int cus, hipStream_t s);
hipError_t launch_bhk_walk(const BhkWs &w, uint32_t n, bool exact, uint32_t *out_pos, hipStream_t s);

// branch_and_bound.hip — the depth-first branch and bound, 4 <= n <= TL_BNB_MAX_N: a wave per subtree, a lane per
// city and per level of the search, a bounded number of nodes per launch.  The host (tl_api_bnb.hip) owns the queue and the splits.
constexpr int kBnbThreads = 256;                   // 4 waves share a workgroup's copy of the matrix
constexpr uint32_t kBnbWavesPerGroup = kBnbThreads / 64;
struct BnbItem {        // a subtree: the prefix path[0..depth-1], 1 <= depth <= n - 1
    uint8_t path[64];
    uint32_t depth, pad;
};
struct BnbWaveHdr {     // a wave's search between launches
    uint32_t active;    // 0: no subtree
    uint32_t k;         // the level whose untried children are next: the prefix path[0..k-1] stands
    uint32_t base;      // the depth of the subtree's root: the subtree is done when level `base` has no child left
    uint32_t rec_has, rec_bits;  // the wave's record: a leaf was kept, the bits of its length
    uint32_t pad[3];
};
struct BnbCtrl {
    uint32_t ub_bits;   // the shared upper bound: the bits of a non-negative f32, lowered with atomicMin
    uint32_t ticket;    // the next queue item
    uint32_t queue_len, pad;
    unsigned long long nodes, leaves, idle;  // summed over every launch; idle: waves that ended a launch with no subtree and no item
};
struct BnbWs {
    float *D;           // [64][64] the distances, +0.0 on the diagonal and outside the instance
    uint64_t *nk;       // [64] the candidate masks N_K(c) (every position where K does not restrict)
    BnbCtrl *ctrl;
    BnbItem *queue;     // [queue_cap]
    BnbWaveHdr *hdr;    // [waves]
    // per wave and lane l: level l of the search
    uint32_t *path;     // [waves][64] the position placed at level l
    uint64_t *untried;  // [waves][64] the children of the prefix path[0..l-1] not yet tried
    double *cost;       // [waves][64] the f64 sum of the edges of path[0..l]
    double *mst;        // [waves][64] the spanning tree's weight at the prefix path[0..l-1]
    uint32_t *rec;      // [waves][64] the recorded tour
};
size_t bnb_ws_bytes(uint32_t waves, uint32_t queue_cap);
BnbWs bnb_ws_layout(void *ws, uint32_t waves, uint32_t queue_cap);
// one launch: every wave takes at most `slice` nodes and leaves, then stores its search.  factor: the prune's 1 + (n + 1) 2^-23
hipError_t launch_bnb(const BnbWs &w, uint32_t n, uint32_t start, uint32_t slice, uint32_t workgroups, uint32_t ub0_bits, bool has_start,
                      double factor, hipStream_t s);

}  // namespace tl
