/*
 * teeline_gpu.h — C ABI of libteeline_gpu.so: the MI355X (gfx950) local-search engine that slots in
 * behind the solver entry points of the `teeline` Rust crate (timgluz/teeline).
 *
 * The reference has NO FFI and no Solver trait; its plug-in boundary is three free
 * functions of identical shape selected by a `match`:
 *     two_opt::solve / three_opt::solve / lin_kernighan::solve
 *         (&TspProblem, &Options, Option<&Sender<ProgressMessage>>, Option<&[usize]>) -> Solution
 *     reference: src/tsp/two_opt.rs:7-12, src/tsp/three_opt.rs:16-21, src/tsp/lin_kernighan.rs:35-40,
 *                dispatch src/tsp/mod.rs:1690-1694,1718,1719.
 * Each entry point below is what a Rust `extern "C"` block binds to replace the body
 * of one of those functions or of a helper they call.  Plain pointers and sizes only.
 *
 * Conventions
 *  - Tours are POSITIONS: indices 0..n-1 into the caller's city array (the reference maps
 *    id<->position with HashMaps at every distance lookup, distance_matrix.rs:197-212; the shim does
 *    that once at the boundary).  u32 is enough: n <= 2^32-1.
 *  - `xy` is n x 2 f32 row-major in city order (KDPoint.coords, kdtree.rs:248-252).
 *  - `dm_packed` (optional) is the reference's packed strict-lower-triangle matrix, n(n-1)/2 f32,
 *    idx(i>j) = i(i-1)/2 + j (distance_matrix.rs:122-153,186).  Pass it for EXPLICIT / GEO problems;
 *    NULL means EUC_2D computed on the fly from xy with the reference's exact f32 arithmetic
 *    (sqrtf(dx*dx+dy*dy), no FMA; kdtree.rs:291-295).
 *  - All host pointers are borrowed for the duration of the call only.  A tl_ctx is single-threaded;
 *    distinct contexts are independent (own HIP stream, event pair and workspace; the library's only
 *    shared mutable state is a mutex-guarded set) — the reference calls solvers from arbitrary threads
 *    (teeline-api tsp_service.rs:295,328, teeline-qt solver_engine.rs:412-432), so create one context per
 *    thread; any number of threads may be inside the library at once, each with its own context
 *    (tests/test_gpu_threads.py).  Two threads on ONE context do not race: the second to arrive gets
 *    TL_ERR_BUSY back at once from every entry point that takes the context.  (tl_destroy on a context
 *    another thread is using is undefined, as free() of a buffer in use is.)
 *  - Return value: TL_OK (0) or a negative tl_status; tl_last_error(ctx) has the message.
 *  - There is NO CPU fallback: every compute entry point fails with TL_ERR_NO_DEVICE / TL_ERR_HIP when
 *    no gfx950 device is usable.
 */
#ifndef TEELINE_GPU_H
#define TEELINE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TL_ABI_VERSION 5 /* bumped when an existing entry point, struct or code changes meaning; additions (round 5: tl_multistart_shard,
                            tl_two_opt_last_counters, new tl_create flags, k <= 64; later: tl_or_opt_population, tl_or_opt_lds_max_n,
                            TL_FLAG_OR_OPT_FORCE_SCAN, tl_three_opt_population and its three companions, TL_FLAG_3OPT_POP_*, tl_sim_anneal and its companions,
                            TL_FLAG_SA_NO_SPECULATION, tl_tabu_search and its companions,
                            TL_FLAG_TABU_FULL_COMPARE, TL_MODE_BEST_SWEEP in the 2-opt batch entries, tl_two_opt_best_population and its three
                            companions) leave it — a caller built against 5 runs unchanged */

typedef struct tl_ctx tl_ctx;

typedef enum tl_status {
    TL_OK = 0,
    TL_ERR_BADARG = -1,      /* NULL pointer, n out of range, init tour not a permutation, ...        */
    TL_ERR_REF_PANICS = -2,  /* input on which the reference itself panics (e.g. 2-opt with n < 3,     */
                             /* two_opt.rs:17,29 usize underflow); the shim turns this into panic!()   */
    TL_ERR_NO_DEVICE = -3,   /* no HIP device / not gfx950                                             */
    TL_ERR_HIP = -4,         /* a HIP runtime call failed                                              */
    TL_ERR_NOMEM = -5,       /* device or host allocation failed                                       */
    TL_ERR_UNSUPPORTED = -6, /* size/mode combination this build cannot run                            */
    TL_ERR_NO_CONVERGE = -7, /* safety cap on sweeps hit (the reference would still be looping)        */
    TL_ERR_BUSY = -8         /* another host thread is inside an entry point with this context (ABI v5);  */
                             /* nothing was touched, tl_last_error(ctx) is NOT updated (it is that thread's) */
} tl_status;

/* 2-opt evaluation order */
typedef enum tl_mode {
    /* The reference's algorithm: first-improvement, in place, lexicographic (i,j), open path
     * (two_opt.rs:26-61).  Tours are bit-identical to the reference's.  Default. */
    TL_MODE_REF_ORDER = 0,
    /* This build's own throughput mode: per sweep evaluate every (i,j), apply the single best
     * improving move (lowest f32 delta, lowest linear index on ties), repeat.  NOT the reference's
     * algorithm; parity-checked against oracle/tlo_two_opt_best. */
    TL_MODE_BEST_SWEEP = 1
} tl_mode;

/* tl_create flags */
#define TL_FLAG_NONE 0u
/* Evaluate every candidate with two fresh correctly-rounded sqrt distances instead of the exact
 * squared-distance pre-test (see DESIGN.md "Exact pruning").  Results are identical; only speed
 * changes.  Used by bench.py to report the un-pruned rate next to the default one. */
#define TL_FLAG_NO_PRUNE 1u
/* Alternative forms of a kernel, kept as cross-checks of each other (the parity tests run every form against the oracle):
 * results are identical, only speed changes.  The library never reads the environment. */
#define TL_FLAG_2OPT_FORCE_HBM (1u << 1)   /* tl_two_opt: the HBM-resident REF_ORDER variant (n > LDS limit) at every n; also sends
                                              tl_two_opt_multistart, tl_two_opt_multistart_devices (the flag of ctxs[0] decides) and the
                                              coordinate form of tl_two_opt_population through their beyond-the-LDS branch at every n >= 4 */
#define TL_FLAG_LK_ONE_WORKGROUP (1u << 2) /* tl_lk: the whole ILS in one persistent workgroup instead of chip-wide scans  */
#define TL_FLAG_KNN_BRUTE (1u << 10)       /* candidate lists: brute-force scan (sixteen lanes per city) in (distance, position)
                                              order instead of the kd-tree walk — the same lists unless two candidates of a city
                                              are at the same f32 distance (then the reference's order is the tree's visiting order) */
#define TL_FLAG_2OPT_NT512 (1u << 14)      /* LDS 2-opt: every descent on 8 waves (default: only when two descents share a CU)   */
#define TL_FLAG_2OPT_NT256 (1u << 15)      /* LDS 2-opt: every descent on 4 waves (default: only when four descents share a CU)  */
#define TL_FLAG_2OPT_FX (1u << 16)         /* LDS 2-opt: the grid-coordinate form (5 B per point) wherever the instance lies on a decimal grid */
#define TL_FLAG_2OPT_NO_NL (1u << 18)      /* LDS 2-opt: never read neighbour lists — every pruned row walks its tiles (default: rows of the
                                              late sweeps (once a sweep has applied fewer than n / 40 moves) of an instance with n >= 400 read the lists, csrc/two_opt_nl.hip).
                                              Matrix form (dm_packed): never cut lists from the matrix rows — every row walks its matrix rows (default: from
                                              n = 500, a sweep that follows one with at most n^2 / 4000 moves decides a row from a's 16 nearest cities, b's
                                              reverse list and the cities with a long tour edge, csrc/two_opt_dm.hip; same tours either way)                  */
#define TL_FLAG_2OPT_NL_ALWAYS (1u << 19)  /* LDS 2-opt: neighbour-list rows at every n they fit and from the second sweep on; matrix form: list
                                              rows at every n >= 8 and in every sweep that has at most 1024 cities with a long tour edge              */
#define TL_FLAG_LK_CHIP_WIDE (1u << 20)    /* tl_lk: chip-wide scans at every n (default: an instance whose search state fits one CU's LDS runs its
                                              lk_pass in ONE workgroup with all state in LDS, k_lk_ils in csrc/lk.hip — up to n = 700, and wherever
                                              it fits (n ~ 3000) with epochs and platoo_epochs >= 64)                                            */
#define TL_FLAG_LK_ILS_LDS (1u << 21)      /* tl_lk: that single-workgroup LDS form at every n it fits                                          */
#define TL_FLAG_MULTISTART_RCCL (1u << 24)  /* tl_two_opt_multistart(_devices), set on ctxs[0]: the winner is found by an RCCL min-all-reduce of the
                                              devices' packed (cost, restart) keys and its tour reaches every device by an RCCL broadcast from its
                                              owner (one process, ncclCommInitAll; librccl is loaded on first use) — the host minimum is computed
                                              all the same and must agree.  Default: the host minimum alone.                                      */
#define TL_FLAG_LK_CLASSIC_VIEW (1u << 23)  /* tl_lk, chip-wide scans at n >= 1500: the chain search reads cand -> xy -> next -> xy (default: the
                                              packed view — candidates with their distances, successor records with the successor's point and the
                                              tour edge's length: two dependent look-ups and one square root per branch instead of four and three) */
#define TL_FLAG_BHK_EXACT_WALK (1u << 25)   /* tl_bellman_karp: read the route back by exact f32 equality instead of the reference's 1e-4 tolerance walk, which
                                              can leave a result that is no tour — always a permutation while a finite tour exists; the same table and optimum */
#define TL_FLAG_OR_OPT_FORCE_SCAN (1u << 26) /* tl_or_opt_population: the tours one after the other through the chip-wide descent of tl_or_opt at every n
                                              (default: only beyond the LDS-resident size) */
#define TL_FLAG_3OPT_POP_FORCE_SCAN (1u << 27) /* tl_three_opt_population: the tours one after the other through the chip-wide descent of tl_three_opt
                                              (default: tl_three_opt_population_plan chooses); wins over TL_FLAG_3OPT_POP_FORCE_WG */
#define TL_FLAG_3OPT_POP_FORCE_WG (1u << 28) /* tl_three_opt_population: one workgroup per tour wherever a tour fits the LDS and its Dt the workspace limit */
#define TL_FLAG_LK_NO_SPECULATION (1u << 22) /* tl_lk, LDS form: the epochs one after the other in one workgroup (default: one workgroup per epoch,
                                              as many consecutive epochs at once as the chip holds, taken in order up to the first accepted one) */
#define TL_FLAG_SA_NO_SPECULATION (1u << 29) /* tl_sim_anneal*: the same kernel with a window of one epoch — the chain epoch after epoch (default: a window of
                                              consecutive epochs evaluated at once against the same tour, the first accepted one committed) */
#define TL_FLAG_TABU_FULL_COMPARE (1u << 30) /* tl_tabu_search*: every tabu-list membership test compares the candidate with every listed route element for
                                              element (default: only with the listed routes whose hash equals the candidate's).  Same results: the cross-check form */
/* TUNING BUILDS ONLY (libteeline_gpu_tune.so, -DTL_TUNE: `python -m teeline_amd.build --tune`).  Forms that were measured and
 * rejected and stay as cross-checks for development; the product library does not carry them and tl_create
 * returns TL_ERR_UNSUPPORTED if one of these bits is set. */
#define TL_FLAG_LK_NO_SPLIT (1u << 3)      /* tl_lk: one lane per (t1, orientation) pair, no sub-search split               */
#define TL_FLAG_LK_SPLIT2 (1u << 4)        /* tl_lk: two split levels (k(k+1) sub-searches per pair) instead of three       */
#define TL_FLAG_LK_NO_SUBCHAINS (1u << 5)  /* tl_lk: the pick step walks the winning chain again instead of reading it      */
#define TL_FLAG_KNN_4LANES (1u << 6)       /* candidate lists: brute force, four lanes per city                              */
#define TL_FLAG_KNN_1LANE (1u << 7)        /* candidate lists: brute force, one lane per city                                */
#define TL_FLAG_LK_SMALL (1u << 9)         /* tl_lk: the LDS-resident single-workgroup form at every n it fits               */
#define TL_FLAG_LK_SEPARATE_PICK (1u << 11) /* tl_lk: pick and validate the pairs' first chains in a kernel of their own (k_lk_scan_pick) */
#define TL_FLAG_LK_NO_GRAPH (1u << 12)      /* tl_lk: enqueue every round's kernels separately instead of replaying 64 rounds as one hipGraph */
#define TL_FLAG_LK_SEPARATE_STEP (1u << 13) /* tl_lk: state machine (one workgroup) and tour rebuild as two kernels at every n */
#define TL_FLAG_LK_SCAN_PERSIST (1u << 17)  /* tl_lk: the fused scan as a persistent grid striding over the window's pairs (round 4, VERDICT r03
                                               item 3: measured 60.6 us per round against 47.0 for one workgroup per pair at n = 13 509) */
#define TL_TUNE_ONLY_FLAGS                                                                                                        \
    (TL_FLAG_LK_NO_SPLIT | TL_FLAG_LK_SPLIT2 | TL_FLAG_LK_NO_SUBCHAINS | TL_FLAG_KNN_4LANES | TL_FLAG_KNN_1LANE | TL_FLAG_LK_SMALL | \
     TL_FLAG_LK_SEPARATE_PICK | TL_FLAG_LK_NO_GRAPH | TL_FLAG_LK_SEPARATE_STEP | TL_FLAG_LK_SCAN_PERSIST)
/* The LDS-resident 2-opt kernel also counts the work its exact decision cascade really does (d_out_stats words 5..8: tile
 * bounds, candidates into L1 / L2 / L3).  Same results; slower (the counters are live scalar registers), so bench.py uses it for one
 * untimed launch only.  Counted: the form of one descent per CU (16 waves, float2 points); the narrower and the
 * grid-coordinate forms run uncounted (words 5..8 stay 0). */
#define TL_FLAG_COUNT_WORK (1u << 8)

/* matrix layouts for tl_dm_build */
#define TL_DM_PACKED_LOWER 0 /* reference layout, n(n-1)/2 floats (distance_matrix.rs:122-153) */
#define TL_DM_FULL 1         /* n x n row-major, zero diagonal (coalesced row gathers)           */
/* TL_DM_FULL entry (i, j) is bit for bit the packed entry at (max(i, j), min(i, j)), i.e. d(xy[max], xy[min]) — for GEO too —
 * and the diagonal is +0.0 whatever the coordinates (a NaN point included). */

/* distance function for tl_dm_build */
#define TL_DIST_EUC2D 0 /* kdtree.rs:291-295            */
#define TL_DIST_GEO 1   /* distance_matrix.rs:59-75     */

/* u64 words per descent written by tl_two_opt_batch_dev into d_out_stats */
#define TL_DEV_STATS_STRIDE 16

typedef struct tl_stats {
    uint64_t sweeps;     /* 2-opt: `while improved` iterations; 3-opt: passes; LK: lk_pass scans      */
    uint64_t candidates; /* candidates whose delta test was decided, counted as the reference's loop  */
                         /* visits them: 2-opt REF_ORDER/BEST_SWEEP = sweeps * (n-3)(n-2)/2            */
    uint64_t moves;      /* improving moves applied                                                    */
    uint64_t reversed;   /* tour elements moved by segment reversals                                   */
    double kernel_ms;    /* device time of the solver kernel(s), HIP events on the context's stream   */
    double total_ms;     /* wall time of the whole call incl. transfers                                */
} tl_stats;

typedef struct tl_lk_opts { /* LKOptions, src/tsp/mod.rs:1249-1267 */
    uint32_t epochs;        /* default 100 (10000 from the CLI, mod.rs:596-613,1321-1325) */
    uint32_t platoo_epochs; /* default 10                                                   */
    uint32_t n_nearest;     /* default 5                                                    */
    uint32_t max_depth;     /* default 5                                                    */
} tl_lk_opts;

/* ---- context ------------------------------------------------------------------------------- */
int tl_abi_version(void);
const char *tl_version(void);
/* device: HIP ordinal (one process per GPU: pass LOCAL_RANK). */
int tl_create(int device, uint32_t flags, tl_ctx **out);
void tl_destroy(tl_ctx *ctx);
const char *tl_last_error(const tl_ctx *ctx); /* ctx may be NULL: last tl_create failure */
/* CU count, LDS bytes per workgroup and arch name of the context's device. */
int tl_device_info(const tl_ctx *ctx, int *cus, int *lds_bytes, char *arch, size_t arch_len);
/* Largest n the LDS-resident REF_ORDER 2-opt kernel takes (tour + coordinates live in one CU's LDS).  tl_two_opt
 * handles larger n with the HBM-resident variant, and so (one descent after the other) do the multi-start and population entries;
 * the device-resident tl_two_opt_batch_dev and the trace entry are LDS-only. */
uint32_t tl_two_opt_lds_max_n(const tl_ctx *ctx);

/* ---- numerics self-test -------------------------------------------------------------------------- */
/* Every kernel's correctly rounded sqrt (the reference's f32::sqrt, kdtree.rs:294) is a short v_sqrt_f32 + FMA
 * fix-up; this compares it on the device with the compiler's full expansion for the `count` f32 bit patterns
 * starting at `first_bits`.  *mismatches must come back 0. */
int tl_selftest_sqrt(tl_ctx *ctx, uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint32_t *first_bad_bits);

/* ---- diagnostics: the neighbour lists of the LDS 2-opt descent's late sweeps ---------------------------------- */
/* Once a sweep has applied fewer than n / 40 moves (random restarts at n = 10^4: from the sixth sweep on), a descent of an instance with n >= 400 (one descent per CU, or two / four of n <= 5568 / 2176; TL_FLAG_2OPT_NO_NL: never) decides a
 * row (a, b) from per-city lists instead of walking every tile (csrc/two_opt_nl.hip: improving => c is strictly closer to a than
 * b, or b strictly closer to e than c).  This builds the lists for xy as a call would and copies them out, for tests:
 * rec [n][64] u16 — per city: [0] high half of the bits of its KA-th smallest squared distance, [2] 1 if its reverse list is
 * incomplete, [4, 4+KA) its KA nearest cities, [20, 20+RB) the cities that count it among their KB nearest (0xFFFF: empty);
 * dkb2 [n] — bits of the KB-th smallest squared distance; knn_b [n][KB] — the KB nearest cities; rcnt [n] — reverse counts.
 * KA, KB, RB come back in *ka, *kb, *rb.  form 0: the kernel the library runs (a wave per city); 1: its cross-check (a workgroup per
 * city, radix select) — the same lists.  TL_ERR_UNSUPPORTED where the lists do not apply (n <= KB + 1). */
int tl_two_opt_neighbour_lists(tl_ctx *ctx, const float *xy, uint32_t n, int form, uint16_t *rec, uint32_t *dkb2, uint16_t *knn_b, uint32_t *rcnt,
                               uint32_t *ka, uint32_t *kb, uint32_t *rb);

/* Which form of the LDS 2-opt descent a batch of `count` descents of n cities runs on a device with `cus` compute units and
 * `lds_bytes` of LDS per workgroup (tl_device_info), float2 points (the grid-coordinate form is decided per instance, on the device):
 * *threads per descent (1024 / 512 / 256 = one / two / four descents per CU; 0: n exceeds the LDS-resident limit) and whether that
 * form has the late phase on neighbour lists.  A host-only query (no context, no device): the library's own selection rule. */
int tl_two_opt_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint32_t flags, int *threads, int *late_phase);

/* ---- distance matrix: replaces DistanceMatrix::build (distance_matrix.rs:122-153) ----------- */
/* out_host may be NULL (matrix stays on the device for later calls on this context). */
int tl_dm_build(tl_ctx *ctx, const float *xy, uint32_t n, int dist, int layout, float *out_host,
                double *kernel_ms);

/* Does dm_packed hold exactly (bit for bit) the EUC_2D distances of xy?  The reference's DistanceMatrix does not keep its
 * DistanceType (distance_matrix.rs:86-93); a shim that only has `problem.distances.distances()` asks here once and then
 * passes dm_packed = NULL (coordinate kernels, same results) when *is_euc2d comes back 1.  Costs one upload of the matrix.
 * The comparison is on bit patterns, with one exception: a NaN entry matches a computed NaN whatever the payloads.  So -0.0 where
 * the computed distance is +0.0 reads as not EUC_2D (the conservative answer: the matrix kernels then run on it). */
int tl_dm_is_euc2d(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, int *is_euc2d);

/* ---- tour cost: replaces DistanceMatrix::tour_length_by_pos (distance_matrix.rs:235-245) ---- */
/* total = d(last,first), then += d(w0,w1) in tour order (sequential f32, bit-exact). */
int tl_tour_length(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n,
                   const uint32_t *perm, float *out_cost);

/* ---- 2-opt: replaces two_opt::solve (two_opt.rs:7-67) ---------------------------------------- */
/* init_pos NULL = city order (two_opt.rs:18-20).  out_pos: n entries.  out_cost = tour_length(out_pos)
 * as Solution::from_parts computes it (mod.rs:1776-1789).  With dm_packed (EXPLICIT / GEO, "matrix in HBM") every
 * distance is read from the matrix, which is expanded on the device to a full row-major n x n copy (4 n^2 bytes of
 * HBM) and the tour plus its edge lengths live in LDS: n <= ~19 900 on 160 KB (TL_ERR_UNSUPPORTED beyond). */
int tl_two_opt(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed,
               const uint32_t *init_pos, int mode, uint32_t *out_pos, float *out_cost,
               tl_stats *stats);

/* ---- 3-opt: replaces three_opt::solve (three_opt.rs:16-51) ---------------------------------- */
int tl_three_opt(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed,
                 const uint32_t *init_pos, uint32_t *out_pos, float *out_cost, tl_stats *stats);
/* One find_best_move scan (three_opt.rs:58-131).  *found = 0/1; (i,j,k,case,savings) as the reference. */
int tl_three_opt_find_best_move(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed,
                                const uint32_t *path, int *found, uint32_t *i, uint32_t *j,
                                uint32_t *k, int *kase, float *savings);

/* ---- Lin–Kernighan: replaces lin_kernighan::solve (lin_kernighan.rs:35-100) ----------------- */
/* seed drives the double-bridge kicks (the reference uses an unseeded thread RNG, :73).
 * The search itself is always Euclidean over xy: the reference rebuilds its own matrix from the city coordinates
 * (lin_kernighan.rs:41) whatever problem.distances holds.  dm_packed (optional; pass problem.distances for GEO / EXPLICIT
 * problems) is used exactly where the reference uses problem.distances: the nearest-neighbour seed when init_pos is NULL
 * (:47-55) and the reported total (:99 Solution::new -> tour_length). */
int tl_lk(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
          const tl_lk_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats);

/* ---- Or-opt: replaces or_opt::solve (or_opt.rs:18-74) — SURVEY.md §8(f) "next" row ------------ */
/* Best-improvement relocation of 1/2/3-city segments (forward and, for 2/3, reversed), threshold -1e-3 (:86). */
int tl_or_opt(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
              uint32_t *out_pos, float *out_cost, tl_stats *stats);
/* One find_best_move scan (or_opt.rs:80-164): (delta, seg_start i, insert_after j, seg_len, reversed). */
int tl_or_opt_find_best_move(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *path,
                             int *found, float *delta, uint32_t *i, uint32_t *j, uint32_t *seg_len, int *reversed);

/* ---- the solvers with what their progress channel carries listed (ABI v4; tl_lk_live: v5) ------- */
/* The reference's solve() functions take Option<&Sender<ProgressMessage>> (two_opt.rs:10, three_opt.rs:19, lin_kernighan.rs:38;
 * only teeline-qt passes one).  A descent here is one kernel launch (or a device-side state machine), so nothing can be sent
 * while it runs; the *_trace entries return, beside the plain entry's results, the record from which the caller replays the
 * reference's exact message sequence after the fact (the Python mirror under teeline_amd/host, teeline_gpu.hpp and integration/teeline-gpu/gpu.rs do).
 * (nearest_neighbor::solve needs no such entry: its messages — the growing path prefix and the current city per step,
 * nearest_neighbor.rs:32-34,40-42,67-69,72-74 — follow from the finished tour.)
 *
 * tl_two_opt_trace — two_opt.rs:22-24,30-32,53-56,63-65 sends PathUpdate(start), CityChange(path[i]) per outer i of every sweep,
 * PathUpdate(path, new_distance) per improving move and Done.  move_log[m] = (i << 16) | j for swap_2opt(path, i+1, j) in the
 * order the reference applies them, and the word TL_TRACE_SWEEP (0xFFFFFFFF) where a new sweep begins (a row can hold moves of
 * two consecutive sweeps back to back); new_distance = d(p[i],p[j]) + d(p[i+1],p[j+1]) on the path before the move.
 * *log_len = words = stats->moves + stats->sweeps - 1; if it exceeds log_cap the log holds the first log_cap words.  REF_ORDER;
 * coordinates (dm_packed NULL; n beyond tl_two_opt_lds_max_n or > 65535: TL_ERR_UNSUPPORTED) or the matrix form (dm_packed,
 * as tl_two_opt). */
#define TL_TRACE_SWEEP 0xFFFFFFFFu
int tl_two_opt_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                     uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap,
                     uint32_t *log_len);
/* tl_three_opt_trace — three_opt.rs:34,42,47-49 sends PathUpdate(path, 0.0) for the start path and after every apply_3opt, then
 * Done.  move_log holds 4 words per applied move, in order: i, j, k, case (three_opt.rs:36-45, apply_3opt :186-218);
 * *log_len = moves (= stats->moves); the log holds the first log_cap of them. */
int tl_three_opt_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                       uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap,
                       uint32_t *log_len);
/* tl_or_opt_trace — or_opt.rs:40-42,62-67,70-72 sends PathUpdate(path, 0.0) for the start path, PathUpdate(path,
 * distances.tour_length(path)) after every apply_relocation, then Done.  move_log holds 4 words per applied move, in order:
 * i (segment start), j (insert after), seg_len, reversed (or_opt.rs:45-51, apply_relocation :172-184); *log_len = moves. */
int tl_or_opt_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                    uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap,
                    uint32_t *log_len);
/* tl_lk_trace — lin_kernighan.rs:71,90 sends PathUpdate(best_tour, best_dist) after the first lk_pass and after every epoch that
 * improves on it (no Done).  snap_pos holds those tours (snap_cap x n positions, in order), snap_dist their best_dist (the
 * Euclidean tour_distance of :118-122, whatever problem.distances holds); *snap_len counts them all, the buffers hold the first
 * snap_cap.  n < 4: none (:57-59).  With TL_FLAG_LK_ONE_WORKGROUP (a cross-check form that keeps no snapshots on the device) the
 * list is the reference's LAST message alone: the final best tour and its best_dist (*snap_len = 1). */
int tl_lk_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                const tl_lk_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats,
                uint32_t *snap_pos, float *snap_dist, uint32_t snap_cap, uint32_t *snap_len);

/* tl_lk_live (ABI v5) — the same messages WHILE the search runs: `progress` is called on the calling thread, between two polls of
 * the device-side search (every 64 rounds: a few milliseconds at n = 13 509), once per best tour the ILS settles on, in order,
 * with the tour (n positions, valid during the call only) and its best_dist — what teeline-qt's channel shows of a multi-second
 * run (teeline-qt/src/solver_engine.rs:412-434).  A call into the SAME context from inside the callback is refused with
 * TL_ERR_BUSY (the running search owns the context's stream and workspace; other contexts are free to use); the callback should
 * return quickly — the GPU idles while it runs.  With TL_FLAG_LK_ONE_WORKGROUP: one call, the
 * final tour.  (The 2-opt / 3-opt / Or-opt descents are single launches of milliseconds: their messages are replayed, above.) */
typedef void (*tl_lk_progress_fn)(void *user, const uint32_t *best_pos, uint32_t n, float best_dist);
int tl_lk_live(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_lk_opts *opts,
               uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats, tl_lk_progress_fn progress, void *user);

/* ---- Lin–Kernighan for seeded runs (additive entries, ABI v5) ---------------------------------------------------
 * LK's result depends on its kick stream; the usual way to use it is several runs with different seeds, keeping the best.
 * THE RUN SEED: run r of seed S is the search tl_lk performs with seed tl_lk_run_seed(S, r) — run 0: S itself; run r >= 1: output
 * 2^63 + r of the splitmix64 stream of S (the kicks draw outputs below 2^35 of their stream, so run 1 of seed 1 is not run 0 of seed
 * 2, as it would be with S + r).  Nothing else of LK changes: candidate lists, first lk_pass, accept / plateau rule, the cap of
 * 64 n + 4096 moves per pass.  tl_lk_run_seed is host-only.
 * tl_lk_population runs the runs first_run .. first_run + count - 1; run r of any call equals first_run = r, count = 1, and run 0
 * equals tl_lk(seed): tour, cost bits and counters.  init_count: 0 (init_pos NULL) — the nearest-neighbour seed tl_lk would build,
 * computed once; 1 — one start tour for all runs; count — row i starts run first_run + i; anything else TL_ERR_BADARG.  A row that is
 * not a permutation: TL_ERR_BADARG, the message names the row; nothing is launched or written.  dm_packed as in tl_lk (the NN seed
 * and the reported totals).  out_pos: count x n positions.  out_costs (optional, count floats): what tl_lk reports.  out_counters
 * (optional, count x 4): the run's sweeps, candidates, moves, reversed as tl_lk's tl_stats counts them.  *best_index (optional): the
 * row of minimum tl_pack_cost_key(cost, i) — equal costs go to the lowest run.  stats (optional): sums over the runs.
 * count == 0: TL_OK, nothing written.  n < 4: every run returns its start tour untouched.  Options as tl_lk checks them (n_nearest
 * 1..64, max_depth 1..16).  A run whose lk_pass hits the cap: TL_ERR_NO_CONVERGE, the message names the run.
 * TWO FORMS, the same results.  Form 1: one workgroup per run with the whole ILS of that run in its CU's LDS (csrc/lk_ils.h,
 * k_lk_ils_pop<NT>), all runs at once (256 threads up to n = 200, two such workgroups per CU where two LDS images fit; 1024 threads beyond, one per CU: the kernel's 110 registers allow 16 waves on a CU); possible where the LDS form of tl_lk fits
 * (tl_lk_population_max_n: the largest such n for these options; 0 for a NULL context or where none fits).  Form 0: the runs one after
 * the other, each in whatever form tl_lk takes (stats->kernel_ms: the sum of the runs' device times).
 * tl_lk_population_plan (host-only, no context): the rule the entry follows for `count` runs of n cities on a device with `cus`
 * compute units and lds_bytes of LDS per workgroup — force_form -1: the plan's choice (form 1 wherever it fits from the measured
 * crossover count on: 64 runs where epochs and plateau are both >= 64, the speculative epochs of a single tl_lk filling the chip, else 2), 0 / 1: forced (1 where it does not fit still gives 0).  Outputs, each optional: *form; *threads (256 up to
 * n = 200, else 1024; 0 in form 0); *per_cu (workgroups that share a CU: 2 where *threads is 256 and two LDS images fit, else 1; 0 in form 0).  TL_ERR_BADARG for cus < 1,
 * lds_bytes < 0, a force_form outside -1..1 and options out of range.
 * tl_lk_population_setting: a setting of the context, not a tl_create flag (all 31 assigned flag bits are taken; bit 31 stays the one
 * no flag has) — the force_form of this context's later populations, and slice_scans, the scans a run advances per launch of form 1
 * (0: the default of 8192; small values let tests reach the slice boundaries).  The cross-check knob of the two forms. */
uint64_t tl_lk_run_seed(uint64_t seed, uint32_t run);
uint32_t tl_lk_population_max_n(const tl_ctx *ctx, const tl_lk_opts *opts);
int tl_lk_population_plan(uint32_t n, const tl_lk_opts *opts, uint32_t count, int cus, int lds_bytes, int force_form, int *form,
                          int *threads, uint32_t *per_cu);
int tl_lk_population_setting(tl_ctx *ctx, int force_form, uint32_t slice_scans);
int tl_lk_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                     uint32_t first_run, uint32_t count, const tl_lk_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                     uint64_t *out_counters, uint32_t *best_index, tl_stats *stats);

/* ---- LK candidate lists: replaces lin_kernighan::build_candidates (lin_kernighan.rs:12-27) -- */
/* out: n x min(k, n-1) u32 — the k-NN buffer of the reference's kd-tree query per city (kdtree.rs:193-212, mod.rs:1839-1889):
 * ascending f32 distance, equal distances in the tree's visiting order.  The tree is the reference's wherever its median
 * selection is unambiguous (no points comparing Equal around a pivot, kdtree.rs:63,301-317); elsewhere the reference's tree is
 * implementation-defined and the (coordinate value, position) order decides.  k <= 64. */
int tl_build_candidates(tl_ctx *ctx, const float *xy, uint32_t n, uint32_t k, uint32_t *out);

/* ---- NN seed: replaces nearest_neighbor::solve (nearest_neighbor.rs:8-76) ---------------------- */
/* First unvisited among the n_nearest closest (stable ties, mod.rs:1848-1855), else the globally
 * nearest unvisited (tie -> lowest position; the reference iterates a HashSet there).  The walk's visited flags
 * live in one CU's LDS (n bytes): n <= ~160 000 (TL_ERR_UNSUPPORTED beyond); n_nearest <= 64.
 * dm_packed NULL: EUC_2D from xy; otherwise every distance is read from the packed matrix (GEO / EXPLICIT problems,
 * distance_matrix.rs:259-297) and xy may be NULL. */
int tl_nearest_neighbor(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, uint32_t n_nearest,
                        uint32_t *out_pos, float *out_cost);

/* ---- greedy-edge construction: replaces greedy_edge::solve (greedy_edge.rs:21-65, graph.rs:54-196) ---- */
/* Every edge i < j in ascending f32::total_cmp order of its length (ties: (i, j) ascending — the reference's unstable sort leaves
 * that order open), accepted unless an endpoint has degree 2 or it closes a cycle before n - 1 edges are in, until n edges are in;
 * the cycle is walked from position 0 along its earlier-accepted edge.  *out_cost is tour_length of that path (the closing edge
 * first, sequential f32).  n <= 2: the identity.  Argument convention of tl_nearest_neighbor (dm_packed NULL: EUC_2D from xy).
 * n <= 65 535 (positions are 16-bit in the sort keys; TL_ERR_UNSUPPORTED beyond).  stats (optional): sweeps = bands of sorted edges,
 * candidates = edges the selection examined, moves = n. */
int tl_greedy_edge(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos, float *out_cost,
                   tl_stats *stats);

/* ---- savings construction: replaces savings::solve (savings.rs:34-163 over graph.rs:98-196) ---- */
/* tl_greedy_edge's selection and path under another order: every edge i < j by its saving s = (dh[i] + dh[j]) - d(i, j) — two f32
 * operations in that order, dh[k] = d(hub, k), dh[hub] = +0.0 — DESCENDING under f32::total_cmp (-0.0 below +0.0, subnormals kept).
 * Two orders the reference leaves open are fixed here:
 *   ties  equal savings go in (i, j) ascending order (the reference's unstable sort leaves that order open);
 *   NaN   a NaN saving of any sign or payload (inf - inf is -NaN on x86, +NaN on AArch64 and on the GPU, and total_cmp puts those
 *         at opposite ends) is ONE value that ranks below every number, after -inf, ties by (i, j): such an edge is taken only
 *         when nothing else is left.
 * Hub (tl_savings_hub, savings.rs:94-117): the position nearest the centroid of xy, all in f32 — sequential left-to-right sums of
 * x and of y, each divided by (float)n, d2 = dx*dx + dy*dy unfused, the first position with d2 < best from best = 0, d2 = FLT_MAX;
 * NaN or inf coordinates therefore give 0, and so does n = 0.  It is host code, O(n), and always reads the coordinates, also where
 * the distances are a GEO or EXPLICIT matrix.
 * tl_savings: hub = TL_SAVINGS_HUB_AUTO computes tl_savings_hub(xy); any other hub >= n is TL_ERR_BADARG.  xy is required when the
 * hub is AUTO or dm_packed is NULL (dm_packed NULL: EUC_2D from xy; otherwise every distance is read from the packed matrix).
 * *out_hub (optional) receives the hub used.  n <= 2: the identity.  *out_cost is tour_length of the path.  n <= 65 535 (positions
 * are 16-bit in the sort keys; TL_ERR_UNSUPPORTED beyond).  stats (optional) as tl_greedy_edge's: sweeps = bands of sorted edges,
 * candidates = edges the selection examined, moves = n. */
#define TL_SAVINGS_HUB_AUTO 0xFFFFFFFFu
int tl_savings_hub(const float *xy, uint32_t n, uint32_t *out_hub);
int tl_savings(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, uint32_t hub, uint32_t *out_pos, float *out_cost,
               uint32_t *out_hub, tl_stats *stats);

/* ---- Christofides construction: replaces christofides::solve (christofides.rs:12-241) ---------- */
/* The reference's six steps on positions: Prim's tree from position 0, its odd-degree vertices, a GREEDY matching of them (all
 * pairs by length, a pair taken when both ends are unmatched — not a blossom matching), the multigraph of tree and matching, its
 * Euler circuit from position 0 (Hierholzer) and the shortcut to first occurrences.  Tree and matching run on the GPU, the O(n)
 * walk of steps 4 to 6 on the host inside the call.  Orders fixed here:
 *   Prim      each round takes the non-tree vertex of smallest key, the FIRST in position order among equals; -0.0 equals +0.0;
 *             key[v] falls to d(u, v) only where d(u, v) < key[v] strictly (keys start at f32::MAX, 0.0 at position 0);
 *   matching  ascending length, -0.0 equal to +0.0, equal lengths in (i, j) ascending order (the reference's stable sort);
 *   NaN       a NaN length between two odd vertices makes the reference's comparator inconsistent and its order unspecified:
 *             here every NaN ranks after +inf, ties by (i, j);
 *   tree      a vertex other than 0 that joins without a parent (every distance to it NaN or >= f32::MAX) leaves the reference
 *             with a result that is no tour: TL_ERR_UNSUPPORTED, the message names the position.
 * dm_packed NULL: EUC_2D from xy; otherwise every distance is read from the packed matrix and xy may be NULL.  n < 4: the
 * identity.  *out_cost is tour_length of the route.  n <= 65 535 (positions are 16-bit in the sort keys; TL_ERR_UNSUPPORTED
 * beyond).  stats (optional): sweeps = bands of sorted pairs, candidates = pairs the matching examined, moves = n, kernel_ms =
 * tree + odd vertices + matching, reversed = the tree's launch alone in nanoseconds, total_ms includes the host walk. */
int tl_christofides(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos, float *out_cost,
                    tl_stats *stats);

/* ---- Bellman-Held-Karp exact solver: replaces bellman_karp::solve (bellman_karp.rs:24-165) ---------- */
/* The dynamic program over subsets on positions, k = n - 1, last = k: opt[c][S] = the f32 minimum over i in S \ c of
 * opt[i][S \ c] + d(i, c), started at f32::MAX and replaced under a strict `<` (a NaN term, or one that rounds to f32::MAX or inf,
 * is never taken), opt[i][{i}] = d(i, last); one kernel launch per subset size, the table (2^k rows of 128 bytes) stays in the
 * context's workspace.  *out_optimal (optional) = the f32::min fold from f32::MAX over i of opt[i][all] + d(i, last), terms with
 * both operands < f32::MAX only (f32::MAX itself: no finite tour, or n = 1).  Every table value is the reference's up to the sign of
 * a zero, which neither the route nor the cost can show.
 * out_pos: n positions exactly as the reference's walk (read_optimal_route, :122-156) leaves them, out_pos[0] = n - 1: per step the
 * FIRST j not yet read with |left - (opt[j][unread] + d(j, prev))| <= max(|left|, |that|, 1) * 1e-4, then left -= d(j, prev); the
 * walk ends once left <= 0.0, and a step that finds no j leaves 0 in its place.  SO THE RESULT NEED NOT BE A TOUR, as in the
 * reference (seeded random instances of 4..12 cities: 1 in 200): the status is TL_OK all the same, *out_is_tour (optional) is 0
 * and a pipeline's validate_tour rejects it.  With TL_FLAG_BHK_EXACT_WALK on the context the route is read back by exact equality
 * instead — the first j not yet read with opt[j][unread] + d(j, prev) == rem, then rem = opt[j][unread], from rem = optimal —
 * which cannot fail: always a permutation while optimal < f32::MAX (otherwise the tolerance walk's result, unchanged).
 * *out_cost = tour_length of out_pos as given, a permutation or not: d(out_pos[n-1], out_pos[0]) first, then the n - 1 edges in
 * order (sequential f32), d(p, p) = 0.  It is NOT *out_optimal: the two sums differ in their last bits.
 * dm_packed NULL: EUC_2D from xy; otherwise every distance is read from the packed matrix and xy may be NULL.  n = 1: [0], cost 0,
 * optimal f32::MAX; n = 0: TL_OK, nothing written, cost 0 (the reference underflows).  n > TL_BHK_MAX_N: TL_ERR_UNSUPPORTED
 * before anything is allocated (n = 26 holds 4 GiB of workspace).  stats (optional): sweeps = layers launched (n - 2),
 * candidates = k(k-1) 2^(k-2) terms, moves = n, kernel_ms = init + layers + optimum + walk, reversed = the layers alone in
 * nanoseconds. */
#define TL_BHK_MAX_N 26u
int tl_bellman_karp(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, uint32_t *out_pos, float *out_cost,
                    float *out_optimal, uint32_t *out_is_tour, tl_stats *stats);

/* ---- branch and bound: the second exact solver, to 64 cities --------------------- */
/* A depth-first branch and bound with the bound of branch_bound.rs:240-268 — the running cost, the next edge, a minimum spanning
 * tree over the start and the unvisited cities — under a specification of this project's own; the reference's search order (a
 * HashSet's iteration order) is not reproduced, and the name `branch_bound` stays refused.
 * D(a, b): the distance of positions a, b in either input form, with tl_bellman_karp's bits, D(a, a) = +0.0.  L(p): tl_tour_length's
 * sum (the closing edge first, then the n - 1 edges in order, sequential f32).  S: every permutation p of 0..n-1 with p[0] =
 * opts->start; with n_nearest = K, 0 < K < n, p[k] must also lie in N_K(p[k-1]) wherever N_K(p[k-1]) holds an unvisited position
 * (any unvisited position where it holds none, branch_bound.rs:231-235).  N_K(c) is c itself and the K - 1 positions j != c with the
 * smallest (D(c, j), j).  K = 0 or K >= n: no restriction, the exact solver.
 * The result R is the argmin over S of (L(p), p), p compared as a sequence of positions.  init_pos NULL: R is returned, *out_improved
 * = 1.  init_pos given (a permutation, else TL_ERR_BADARG): R if L(R) < L(init_pos as given), else init_pos as given with
 * *out_improved = 0 (branch_bound.rs:84-90).  *out_cost = L(out_pos).  With *out_proved = 1 the result is exactly that, whatever
 * the launch parameters, the device and the run.  max_nodes / time_limit_ms (0: none) are checked between launches; when either
 * ends the search the status is TL_OK, *out_proved = 0 and the result the best tour found so far (or init_pos, or start followed by
 * the other positions in order): a valid tour, never longer than init_pos, otherwise unspecified.
 * A child is cut only if running cost + next edge + MST, summed in f64, exceeds (double)bound x (1 + (n + 1) 2^-23): no tour of
 * length <= bound is ever cut, equal lengths included (DESIGN.md §4.27 has the proof).
 * n > TL_BNB_MAX_N: TL_ERR_UNSUPPORTED before anything is allocated.  A distance between two of the n positions that is NaN, has its
 * sign bit set (-0.0 included) or is >= f32::MAX: TL_ERR_UNSUPPORTED; so is an instance none of whose tours has a length <=
 * f32::MAX.  opts->start >= n (n >= 1): TL_ERR_BADARG.  n = 0 and n = 1 as tl_bellman_karp.  opts NULL: all zero.
 * tl_branch_and_bound_host is the sequential restatement on the CPU (no context, no device): the same contract, the frontier
 * builder of the device entry, the tests' oracle for large cases and the timing baseline; its budgets are checked at every node.
 * tl_branch_and_bound_plan: the launch parameters the device entry takes for n on a device of `cus` compute units and `lds_bytes`
 * of LDS per workgroup (each output optional; cus < 1 or lds_bytes < 0: TL_ERR_BADARG; n > TL_BNB_MAX_N: TL_ERR_UNSUPPORTED). */
#define TL_BNB_MAX_N 64u
typedef struct tl_bnb_opts {
    uint32_t start;            /* p[0]; the mirrors pass the position of the smallest id (route.sort(), branch_bound.rs:35)  */
    uint32_t n_nearest;        /* K; 0 or >= n: exact                                                                        */
    uint64_t max_nodes;        /* 0: no limit                                                                                */
    uint32_t time_limit_ms;    /* 0: no limit                                                                                */
    uint32_t nodes_per_launch; /* nodes and leaves a wave takes per launch (0: the plan's)                                   */
    uint32_t frontier_depth;   /* positions behind start that the host places before the device takes over (0: the plan's)  */
    uint32_t workgroups;       /* 0: the plan's                                                                              */
} tl_bnb_opts;
typedef struct tl_bnb_stats {
    uint64_t nodes;              /* prefixes whose bound was computed, host frontier included                                */
    uint64_t leaves;             /* complete tours whose length was computed                                                 */
    uint64_t launches;
    uint64_t queue_start;        /* subtrees the host's frontier queued                                                      */
    uint64_t queue_end;          /* ... plus those split off unfinished subtrees at launch boundaries                        */
    uint64_t wave_launches;      /* launches x waves                                                                         */
    uint64_t idle_wave_launches; /* of those, the ones that ended with no subtree and an empty queue                         */
    double kernel_ms;            /* the launches, HIP events                                                                 */
    double max_launch_ms;        /* the longest launch-and-poll interval seen by the host                                    */
    double total_ms;
} tl_bnb_stats;
int tl_branch_and_bound(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, const uint32_t *init_pos, const tl_bnb_opts *opts,
                        uint32_t *out_pos, float *out_cost, uint32_t *out_proved, uint32_t *out_improved, tl_bnb_stats *stats);
int tl_branch_and_bound_host(const float *xy, const float *dm_packed, uint32_t n, const uint32_t *init_pos, const tl_bnb_opts *opts,
                             uint32_t *out_pos, float *out_cost, uint32_t *out_proved, uint32_t *out_improved, tl_bnb_stats *stats);
int tl_branch_and_bound_plan(uint32_t n, int cus, int lds_bytes, int *threads, int *workgroups, uint32_t *frontier_depth,
                             uint32_t *nodes_per_launch);

/* ---- multi-start 2-opt (north-star config 4; no counterpart in the reference) ---------------- */
/* Runs restarts [first, first+count) — restart r starts from the Fisher–Yates permutation drawn
 * from splitmix64(seed + r) (specification: DESIGN.md / oracle tlo_restart_perm) — one descent per
 * workgroup, all concurrently.  Returns the best tour of this shard; out_costs (count floats,
 * optional) gets every restart's final cost.  Ranks shard [0,R) between themselves and min-reduce
 * tl_pack_cost_key(best_cost, best_restart) with RCCL.
 * Beyond tl_two_opt_lds_max_n (or with TL_FLAG_2OPT_FORCE_HBM) the restarts run ONE AFTER THE OTHER through the HBM form:
 * the same tours, costs and counters; stats->kernel_ms is then the sum of the descents' device times.
 * mode == TL_MODE_BEST_SWEEP (coordinates, n <= 65535 as in tl_two_opt): every restart is a whole best-sweep descent in ONE workgroup
 * with the tour, the tile metadata and the row-key cache in that CU's LDS (csrc/two_opt_best_lds.hip), no launch between sweeps;
 * restart r's tour, cost and counters are what tl_two_opt(..., TL_MODE_BEST_SWEEP, ...) gives from the same start.  Beyond
 * tl_two_opt_best_lds_max_n, or after tl_two_opt_best_force_scan(ctx, 1), the restarts run one after the other through that chip-wide form
 * (kernel_ms: the sum of the descents' device times; over several devices the slowest shard's sum, as above).  stats->candidates is
 * the sum over the descents of sweeps * (n-3)(n-2)/2.  tl_two_opt_last_counters has nothing to report after a call in this mode. */
int tl_two_opt_multistart(tl_ctx *ctx, const float *xy, uint32_t n, uint64_t seed, uint32_t first,
                          uint32_t count, int mode, uint32_t *out_best_pos, float *out_best_cost,
                          uint32_t *out_best_restart, float *out_costs, tl_stats *stats);
/* The same job over several devices of one node from ONE process (the reference is single-process; SURVEY.md §8(b)
 * proposed tl_multistart_two_opt(..., n_gpus, ...)): ctxs holds one context per device, each from tl_create(device, ...).
 * Restarts [first, first+count) are dealt in contiguous blocks (the first count % n_ctxs contexts take one more), all
 * shards run concurrently, the winner is the minimum packed key over the shards (equal costs: the lower restart) — results
 * do not depend on n_ctxs.  Errors are reported on ctxs[0].  stats->kernel_ms is the slowest shard's device time.
 * Beyond tl_two_opt_lds_max_n (or with TL_FLAG_2OPT_FORCE_HBM on ctxs[0]) the shards do NOT run concurrently: every descent goes
 * through the HBM form and is polled on the calling thread, shard after shard, restart after restart.  Results are the same;
 * stats->kernel_ms is still the slowest shard's — the largest of the shards' summed device times — while total_ms covers all
 * of them, so several devices give no speed-up on this path.
 * tl_multistart_shard: that deal as a host-only query (no context) — block `part` of `parts`; the ranks of a multi-process job
 * (bench.py, teeline_amd/host/multistart.py shard_total) use the same map. */
int tl_multistart_shard(uint32_t first, uint32_t count, int parts, int part, uint32_t *shard_first, uint32_t *shard_count);
int tl_two_opt_multistart_devices(tl_ctx *const *ctxs, int n_ctxs, const float *xy, uint32_t n, uint64_t seed,
                                  uint32_t first, uint32_t count, int mode, uint32_t *out_best_pos, float *out_best_cost,
                                  uint32_t *out_best_restart, float *out_costs, tl_stats *stats);
/* (float_bits(cost) << 32) | restart: order-preserving for cost >= 0, ties -> lowest restart. */
uint64_t tl_pack_cost_key(float cost, uint32_t restart);
/* A population of `count` explicit tours (init_pos: count x n positions), each refined by its own
 * REF_ORDER descent, one workgroup per tour, all concurrently; tour r of out_pos / out_costs equals what
 * tl_two_opt returns for it alone (two_opt.rs:7-67 with init_tour = Some(tour r)).  The reference has no
 * batch form: its callers loop over two_opt::solve (the north-star's GA refinement would, too).
 * dm_packed as in tl_two_opt.  Beyond tl_two_opt_lds_max_n, or with TL_FLAG_2OPT_FORCE_HBM (coordinates only), the tours run one after
 * the other through the HBM form; stats->kernel_ms is then the sum of the descents' device times. */
int tl_two_opt_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed,
                          const uint32_t *init_pos, uint32_t count, uint32_t *out_pos, float *out_costs,
                          tl_stats *stats);
/* The same for TL_MODE_BEST_SWEEP (EUC_2D coordinates, 3 <= n <= 65535): each of the `count` tours by its own best-sweep descent, one
 * workgroup per tour with the whole state in that CU's LDS (csrc/two_opt_best_lds.hip), all concurrently.  Tour r of out_pos /
 * out_costs / out_moves (optional, count entries: the moves that descent applied) is exactly what the single-tour entry in mode
 * TL_MODE_BEST_SWEEP returns for init_pos + r * n alone: the route element for element, the cost bit for bit.
 * count == 0: TL_OK, nothing written.  A row of init_pos that is not a permutation of 0..n-1: TL_ERR_BADARG, the message names the
 * tour; nothing is launched or written.  A descent at the sweep cap: TL_ERR_NO_CONVERGE, the message names the tour.
 * tl_two_opt_best_lds_max_n: the largest n of the LDS-resident form (0 for a NULL context) — 18 bytes per position of the padded
 * tour (point, row key, 16-bit position) and 20 per tile of the padded tile table: 8 768 on 160 KB.  Beyond it, or
 * after tl_two_opt_best_force_scan(ctx, 1), the tours run one after the other through the chip-wide descent: the same results;
 * stats->kernel_ms is then the sum of the descents' device times.
 * tl_two_opt_best_force_scan: a setting of the context (on != 0: every later best-sweep multi-start / population call of this context
 * takes the loop at every n; for tl_two_opt_multistart_devices the setting of ctxs[0] decides; 0 restores the default) — the cross-check
 * of the two forms.  It is a setting and not a tl_create flag because all 31 assigned flag bits are taken and bit 31 stays the one bit
 * no flag has, which the seeded solvers refuse.  TL_ERR_BADARG for a NULL context.
 * tl_two_opt_best_plan (host-only, no context): which form a batch of `count` descents of n cities takes on a device with `cus`
 * compute units and lds_bytes of LDS per workgroup, with the context's force-scan setting as `force_scan` — *form 0: one workgroup per
 * descent, *threads wide; *form 1: the loop over the chip-wide descent (*threads 0).  TL_ERR_BADARG on a NULL output. */
uint32_t tl_two_opt_best_lds_max_n(const tl_ctx *ctx);
int tl_two_opt_best_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, int force_scan, int *form, int *threads);
int tl_two_opt_best_force_scan(tl_ctx *ctx, int on);
int tl_two_opt_best_population(tl_ctx *ctx, const float *xy, uint32_t n, const uint32_t *init_pos, uint32_t count, uint32_t *out_pos,
                               float *out_costs, uint32_t *out_moves, tl_stats *stats);

/* Or-opt over a population of `count` explicit tours (init_pos: count x n positions), each by its own or_opt::solve descent
 * (or_opt.rs:18-74), one workgroup per tour with the tour in that CU's LDS (csrc/or_opt_lds.hip), all concurrently.  Tour r of
 * out_pos / out_costs / out_moves (optional, count entries: the moves that descent applied) is exactly what tl_or_opt returns for
 * init_pos + r * n alone: the route element for element, the cost bit for bit.  The reference has no batch form.
 * n < 4: every output tour is the identity and init_pos is ignored (or_opt.rs:31-34).  count == 0: TL_OK, nothing written.  A row
 * of init_pos that is not a permutation of 0..n-1: TL_ERR_BADARG, the message names the tour; nothing is launched or written.  A
 * descent still finding moves after 64 n + 1024 passes: TL_ERR_NO_CONVERGE, the message names the tour.
 * tl_or_opt_lds_max_n: the largest n of the LDS-resident coordinate form (16 bytes per city: position, point, tour edge; 10 224
 * on 160 KB); the matrix form (dm_packed; distances read from the packed matrix in HBM) keeps 8 bytes per city and takes twice
 * that n.  Beyond it, or with TL_FLAG_OR_OPT_FORCE_SCAN, the tours run one after the other through tl_or_opt's chip-wide descent:
 * the same results; stats->kernel_ms is then the sum of the descents' device times.
 * stats (optional): moves and sweeps (passes, each descent's last one finds nothing) summed over the tours, candidates = the
 * placements those passes examined, counted as tl_or_opt counts them. */
uint32_t tl_or_opt_lds_max_n(const tl_ctx *ctx);
int tl_or_opt_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t count,
                         uint32_t *out_pos, float *out_costs, uint32_t *out_moves, tl_stats *stats);

/* 3-opt over a population of `count` explicit tours (init_pos: count x n positions), each by its own three_opt::solve descent
 * (three_opt.rs:16-51).  Tour r of out_pos / out_costs / out_moves (optional, count entries: the moves that descent applied) is
 * exactly what tl_three_opt returns for init_pos + r * n alone: the route element for element, the cost bit for bit.  The reference
 * has no batch form.
 * n < 4: every output tour is the identity and init_pos is ignored (three_opt.rs:25-28).  count == 0: TL_OK, nothing written.  A row
 * of init_pos that is not a permutation of 0..n-1: TL_ERR_BADARG, the message names the tour; nothing is launched or written.  A
 * descent still finding moves after 64 n + 1024 passes (looked at every 16 passes, as tl_three_opt looks: a descent fails here exactly
 * when tl_three_opt fails on it): TL_ERR_NO_CONVERGE, the message names the tour.
 * Two forms.  form 1: one persistent workgroup per tour (csrc/three_opt_pop.hip) with the tour, its edges and the move's staging in
 * that CU's LDS (20 bytes per city) and the tour's own n x (n+1) f32 matrix of distances between tour positions in the context's
 * workspace, all tours of a batch concurrently; `batch` tours' matrices fit the workspace limit (default 8 GiB,
 * tl_three_opt_population_work_limit; 0 restores the default), and the entry runs batch after batch.  form 0: the tours one after
 * the other through tl_three_opt's chip-wide descent.  The results are the same; in form 0 stats->kernel_ms is the sum of the
 * descents' device times.
 * tl_three_opt_population_plan (pure: no device, no context) is the rule the entry follows with the context's CU count, LDS and
 * workspace limit: form 0 where n exceeds the LDS fit (tl_three_opt_pop_max_n; 0 for NULL), where not even one matrix fits
 * work_bytes (batch 0) or with TL_FLAG_3OPT_POP_FORCE_SCAN; form 1 with TL_FLAG_3OPT_POP_FORCE_WG; otherwise the form its cost model
 *  estimates faster — few large tours leave most CUs idle in form 1, many small ones pay four launches per move in
 * form 0.  threads (form 1: a multiple of 64 in 64..1024; form 0: 0) and batch (the matrices that fit, at most count) are outputs,
 * each optional.  TL_ERR_BADARG for cus < 1 or lds_bytes < 0.
 * stats (optional): moves and sweeps (passes, each descent's last one finds nothing) summed over the tours, candidates =
 * sweeps x (C(n,3) - (n-2)), as tl_three_opt counts them. */
uint32_t tl_three_opt_pop_max_n(const tl_ctx *ctx);
int tl_three_opt_population_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint64_t work_bytes, uint32_t flags, int *form,
                                 int *threads, uint32_t *batch);
int tl_three_opt_population_work_limit(tl_ctx *ctx, uint64_t bytes);
int tl_three_opt_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t count,
                            uint32_t *out_pos, float *out_costs, uint32_t *out_moves, tl_stats *stats);

/* ---- simulated annealing: replaces simulated_annealing::solve (simulated_annealing.rs:10-83) ---------- */
/* The reference's chain with its quirks kept: "best_route" is the current state and the LAST state is returned; the schedule is
 * `while epoch < epochs || temperature > min_temperature`, T <- T - cooling_rate * T (f32, two roundings: 138 149 epochs with the
 * defaults); an epoch reverses positions from..=to of the open path (route.rs:48-113; after 10 redraws the last pair is used even
 * when equal or adjacent), costs the whole candidate with tour_length (closing edge first, sequential f32) and accepts it when it
 * is shorter, never when |new - old| < FLT_EPSILON, else when p < exp(-(new - old) / T).
 * TWO THINGS ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_sa_oracle.py is the statement):
 *   draws   the reference's unseeded thread RNG cannot be reproduced.  Here u(seed, chain, epoch, slot) =
 *           mix(mix(seed + G (chain + 1)) + G (32 epoch + slot + 1)), mix = splitmix64's output function, G = 0x9E3779B97F4A7C15
 *           (tl_sa_draw); pair attempt a uses slots 2a, 2a + 1, a position is ((u >> 32) n) >> 32, p = float(u >> 40) 2^-24 from
 *           slot 22.  A draw never depends on an earlier one;
 *   exp     a fixed f64 operation sequence without FMA instead of the platform's exp: 0 for x < -87, else k = rint(x log2 e),
 *           r = (x - k ln2_hi) - k ln2_lo, the Horner sum of r^i / i! up to i = 13, (float) ldexp(q, k).
 * One workgroup per chain with the chain in that CU's LDS (12 bytes per city; csrc/sim_anneal.hip), a window of consecutive
 * epochs evaluated at once; with TL_FLAG_SA_NO_SPECULATION the window is one epoch.  Same tours, costs and accepted epochs.
 * opts NULL: the defaults (10 000 / 1e-4 / 1e-3 / 1000; mod.rs:598-608, 697-705).  Options that SAOptions::validate (mod.rs:707-741)
 * refuses are TL_ERR_BADARG — except where the schedule is empty (epochs = 0 and not max_temperature > min_temperature): solve itself
 * never validates, and the reference's own test runs epochs 0, max 0, min 1e6 and gets its start tour back; so does this.  A schedule
 * of more than 2^32 - 1 epochs (or one that never ends: T stops falling above min_temperature): TL_ERR_UNSUPPORTED.  n < 2 with a
 * non-empty schedule: TL_ERR_REF_PANICS (route.rs:87-89).  n > tl_sim_anneal_lds_max_n: TL_ERR_UNSUPPORTED, before anything of size
 * n is read or allocated.  init_pos NULL: city order; not a permutation: TL_ERR_BADARG.  dm_packed as in tl_two_opt (expanded on
 * the device to a row-major n x n copy; the matrix must be what the packed triangle is: symmetric).
 * tl_sim_anneal runs chain 0.  stats (optional): sweeps = candidates = epochs run, moves = accepted epochs, reversed = elements
 * moved by their reversals.
 * tl_sim_anneal_trace: the same plus the accepted epochs in order, 4 words each: epoch, from, to, the bits of the new cost — what
 * a caller replays the reference's PathUpdate messages from.  *log_len counts them all; the log holds the first log_cap.
 * tl_sim_anneal_trace_chain: the same for chain `chain` of the seed (what a caller replays the best chain of a population from).
 * tl_sim_anneal_population: chains first_chain .. first_chain + count - 1, each its own stream of draws, all concurrently (more
 * chains than the device holds at once — tl_sim_anneal_plan's per_launch — run in further launches).  init_count 0: every chain
 * from city order (init_pos ignored); 1: every chain from init_pos; count: chain r from init_pos + r * n; anything else
 * TL_ERR_BADARG.  out_pos count x n, out_costs / out_moves (optional) count entries, *best_index (optional) the chain (0-based
 * within the call) of minimum tl_pack_cost_key(cost, index): equal costs go to the lower chain.  Chain c of any population equals
 * first_chain = c, count = 1.  count == 0: TL_OK, nothing written.  stats: sums over the chains.
 * Host-only queries (no context, no device): tl_sa_draw — the u64 above; tl_sa_schedule_epochs — the length of the schedule
 * (TL_ERR_UNSUPPORTED as above; the options are not validated); tl_sim_anneal_plan — the window (epochs at once), the threads of a
 * chain's workgroup and the chains one launch holds, for n cities and count chains on a device with cus compute units and lds_bytes
 * of LDS per workgroup (outputs optional; window and threads 0 where n exceeds the LDS-resident limit).
 * tl_sa_selftest_accept: the acceptance rule evaluated on the device for count given (T, old, new, p): out_accept 0 / 1,
 * out_criteria the criterion's value (computed for every entry, also where the rule does not consult it). */
typedef struct tl_sa_opts { /* SAOptions, src/tsp/mod.rs:689-706 */
    uint32_t epochs;        /* default 10 000 */
    float cooling_rate;     /* default 1e-4   */
    float min_temperature;  /* default 1e-3   */
    float max_temperature;  /* default 1000   */
} tl_sa_opts;
uint32_t tl_sim_anneal_lds_max_n(const tl_ctx *ctx);
int tl_sim_anneal(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_sa_opts *opts,
                  uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_sim_anneal_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_sa_opts *opts,
                        uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap,
                        uint32_t *log_len);
int tl_sim_anneal_trace_chain(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_sa_opts *opts,
                              uint64_t seed, uint32_t chain, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap,
                              uint32_t *log_len);
int tl_sim_anneal_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                             uint32_t first_chain, uint32_t count, const tl_sa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                             uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_sa_draw(uint64_t seed, uint32_t chain, uint32_t epoch, uint32_t slot);
int tl_sa_schedule_epochs(const tl_sa_opts *opts, uint64_t *epochs);
int tl_sim_anneal_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint32_t flags, uint32_t *window, int *threads, uint32_t *per_launch);
int tl_sa_selftest_accept(tl_ctx *ctx, const float *T, const float *old_cost, const float *new_cost, const float *p, uint32_t count,
                          uint32_t *out_accept, float *out_criteria);

/* ---- tabu search: replaces tabu_search::solve (tabu_search.rs:9-110) ---------------------------------- */
/* The reference's chain with its quirks kept: best = u = the start tour, which the list (capacity n routes, FIFO: a full list drops
 * its oldest) receives.  Epoch e = 0, 1, ...: up to n + 1 candidates of u are drawn, each u with positions from..=to of the open path
 * reversed (route.rs:48-113; after 10 redraws the last pair is used even when equal or adjacent) and costed with tour_length of the
 * whole candidate (closing edge first, sequential f32).  The first of candidates 0 .. n-1 that is shorter than u AND equal to no
 * listed route is taken; failing that, candidate n is taken with no check at all (it may be longer, equal to u, or listed).  A taken
 * candidate shorter than the best so far becomes the best; the OLD u goes into the list (so the start tour is listed twice after
 * epoch 0); u <- the taken candidate.  The loop ends when `epoch > epochs` after the increment: epochs + 1 epochs run.  The BEST
 * route is returned.
 * THE RANDOM STREAM IS THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_tabu_oracle.py is the
 * statement): tl_sim_anneal's stream indexed by a 64-bit event, event = epoch (n + 1) + attempt,
 *   u(seed, chain, event, slot) = mix(mix(seed + G (chain + 1)) + G (32 event + slot + 1))      (tl_tabu_draw)
 * pair attempt t uses slots 2t, 2t + 1, a position is ((u >> 32) n) >> 32.  No draw depends on an earlier one, so the candidates of
 * an epoch are evaluated at once, a round of `window` per step (csrc/tabu_search.hip: one workgroup per chain, the tour in that CU's
 * LDS, 12 bytes per city; the list a ring of n routes of 16-bit entries in the context's workspace, 2 n^2 bytes per chain, with one
 * hash per route — a hash match is always followed by an element-for-element comparison, and with TL_FLAG_TABU_FULL_COMPARE every
 * listed route is compared).
 * epochs = 0 (the reference never ends) and epochs = 2^32 - 1: TL_ERR_UNSUPPORTED.  n < 2: TL_ERR_REF_PANICS (route.rs:87-89).
 * n > tl_tabu_search_lds_max_n: TL_ERR_UNSUPPORTED, before anything of size n is read or allocated (no HBM form).  init_pos NULL:
 * city order; not a permutation: TL_ERR_BADARG.  A context whose flags hold a bit no flag has: TL_ERR_UNSUPPORTED.  dm_packed as in
 * tl_sim_anneal.
 * tl_tabu_search runs chain 0.  stats (optional): sweeps = epochs run, candidates = the candidates the reference would have drawn
 * (the sum of taken attempt + 1), moves = new bests, reversed = elements moved by the taken reversals.
 * tl_tabu_search_trace: the same plus EVERY epoch in order, 4 words each: taken attempt (n: the unchecked one), from, to, the bits
 * of the taken candidate's cost — what a caller replays the reference's PathUpdate messages from (one per new best).  *log_len
 * counts them all; the log holds the first log_cap.  tl_tabu_search_trace_chain: the same for chain `chain` of the seed.
 * tl_tabu_search_population: chains first_chain .. first_chain + count - 1, each its own stream of draws, concurrently (more
 * chains than the LDS and the workspace limit hold at once — tl_tabu_search_plan's per_launch — run in further launches).
 * init_count, out_pos / out_costs / out_moves (new bests per chain), *best_index and its tie rule, count == 0: as
 * tl_sim_anneal_population.  Chain c of any population equals first_chain = c, count = 1.
 * Host-only queries (no context, no device): tl_tabu_draw — the u64 above for candidate `attempt` of `epoch` on n cities;
 * tl_tabu_search_plan — the window (candidates per round), the threads of a chain's workgroup and the chains one launch holds, for
 * n cities and count chains on a device with cus compute units, lds_bytes of LDS per workgroup and workspace_bytes for the lists
 * (outputs optional; all 0 where n is outside 2 .. the LDS-resident limit; the entries plan with 8 GiB). */
uint32_t tl_tabu_search_lds_max_n(const tl_ctx *ctx);
int tl_tabu_search(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, uint64_t seed,
                   uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_tabu_search_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, uint64_t seed,
                         uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len);
int tl_tabu_search_trace_chain(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                               uint64_t seed, uint32_t chain, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log,
                               uint32_t log_cap, uint32_t *log_len);
int tl_tabu_search_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                              uint32_t first_chain, uint32_t count, uint32_t epochs, uint64_t seed, uint32_t *out_pos, float *out_costs,
                              uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_tabu_draw(uint64_t seed, uint32_t chain, uint32_t n, uint32_t epoch, uint32_t attempt, uint32_t slot);
int tl_tabu_search_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags, uint32_t *window, int *threads,
                        uint32_t *per_launch);

/* ---- the genetic algorithm (src/tsp/genetic_algorithm.rs:16-336) ------------------------------ */
/* The reference's algorithm with its quirks kept.  The population size is n.  fitness = 1 / tour_length in f32 (0 where the length
 * is 0), tour_length as everywhere here (closing edge first, sequential f32).  Start population: with init_pos, individual 0 is that
 * tour, individuals 1 .. max(n / 5, 1) - 1 are the tour after 2, 3 or 4 mutations, the rest are shuffles of city order; init_pos
 * NULL: n shuffles.  A generation: stable sort by fitness, descending; the first min(n_elite, length) individuals are copied; then
 * n / 2 - n_elite times two roulette selections over the SORTED population (r in [0, total), total and the running sum sequential
 * f32 sums; the first i with r < up_to + f_i, else the last), one ordered crossover (child 1 has PARENT 2's segment from..=to, the
 * other positions are filled from to + 1 on, wrapping, with parent 1's cities in the order met from to + 1; child 2 symmetrically),
 * and each child mutated with probability mutation_probability — a reversal of from..=to that does NOT recompute the fitness.  So the
 * population has n individuals in generation 0 and min(n_elite, length) + 2 max(0, n / 2 - n_elite) afterwards.  The result is the
 * individual of maximum fitness, the LAST of equals; *out_cost is tour_length of its route, recomputed (it can differ from
 * 1 / fitness after a mutation).  epochs = 0 returns the best of the start population.
 * THE RANDOM STREAM IS THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_ga_oracle.py is the
 * statement; csrc/ga_spec.h the text): tl_sim_anneal's stream indexed by a 64-bit event,
 *   u(seed, run, event, slot) = mix(mix(seed + G (run + 1)) + G (32 event + slot + 1))              (tl_ga_draw)
 * Pair p of generation g owns the events 4 (g n + p) + part: part 0 holds the crossover pair (slots 0 .. 21, attempt t on 2t,
 * 2t + 1), the two roulette draws (22, 23) and the two mutation trials (24, 25: p > float(u >> 40) 2^-24); parts 1 and 2 hold the
 * mutation pairs of child 1 and child 2.  Individual i of the start population owns the events 2^58 + i n + j: j = 0, slot 27 its
 * mutation count 2 + position(u, 3); j = 1 + m, slots 0 .. 21 its mutation m; slot 26 of event j step j = n - 1 .. 1 of its
 * Fisher-Yates pass, swap(a[j], a[position(u, j + 1)]).  No draw depends on an earlier one, so a generation's pairs are bred at once
 * (csrc/genetic.hip: a rank launch and a breed launch per generation, one workgroup per pair, the populations 16-bit in the
 * context's workspace, 4 n^2 bytes per run).
 * Small n, as the reference's code behaves: n = 0: TL_ERR_REF_PANICS (best() of an empty population).  n = 1: there is no pair, so
 * a generation keeps min(n_elite, 1) individuals — epochs = 0 or n_elite >= 1 return the one city at cost 0, epochs >= 1 with
 * n_elite = 0 is TL_ERR_REF_PANICS (the population empties).  n = 2 and n = 3 run as any n does (one pair; the population of n = 3
 * has 2 individuals after generation 0).  A population whose total fitness is not > 0 or not finite when a roulette is due (all
 * cities in one place): TL_ERR_REF_PANICS (random_range on an empty range).
 * n > tl_genetic_algorithm_max_n: TL_ERR_UNSUPPORTED, before anything of size n is read or allocated.  init_pos not a permutation:
 * TL_ERR_BADARG.  mutation_probability not finite or outside [0, 1]: TL_ERR_BADARG (GAOptions::validate).  A context whose flags
 * hold a bit no flag has: TL_ERR_UNSUPPORTED.  dm_packed as in tl_sim_anneal.
 * tl_genetic_algorithm runs run 0.  stats (optional): sweeps = generations, candidates = children bred, moves = generations whose
 * best fitness exceeds that of the population before, reversed = mutations applied.
 * tl_genetic_algorithm_trace: the same plus 4 words per generation: the best individual's index in the new population, its fitness
 * bits, the bits of its recomputed tour_length, the population's length.  *log_len counts the generations; the log holds the first
 * log_cap.  route_log (optional, route_cap x n): the best route of the first route_cap generations — what a caller replays the
 * reference's PathUpdate messages from (one per generation, then one more, then Done).  tl_genetic_algorithm_trace_run: the same
 * for run `run` of the seed.
 * tl_genetic_algorithm_population: runs first_run .. first_run + count - 1, each its own stream of draws, in one launch sequence
 * (more runs than the workspace limit holds — tl_genetic_algorithm_plan's per_launch — go in further sequences).  init_pos: NULL or
 * ONE tour, the initial tour of every run.  out_pos count x n, out_costs (optional) count entries, *best_index (optional) and its
 * tie rule, count == 0: as tl_tabu_search_population.  Run c of any batch equals first_run = c, count = 1.
 * Host-only queries (no context, no device): tl_ga_draw — the u64 above; tl_genetic_algorithm_plan — the runs one launch sequence
 * holds, the threads of a breeding workgroup and the workspace bytes of min(count, per_launch) runs, for n cities on a device with
 * cus compute units, lds_bytes of LDS per workgroup and workspace_bytes of workspace (outputs optional; all 0 where n is outside
 * 1 .. the limit; the entries plan with 8 GiB).  tl_genetic_algorithm_max_n: the largest n (the breeding workgroup keeps 14 bytes
 * per city in LDS).
 * tl_ga_selftest_crossover: the DEVICE's ordered crossover on two given parents (permutations of 0..n-1, 2 <= n <= the limit,
 * from <= to < n; else TL_ERR_BADARG): out1, out2 receive child 1 and child 2. */
uint32_t tl_genetic_algorithm_max_n(const tl_ctx *ctx);
int tl_genetic_algorithm(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                         float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_genetic_algorithm_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                               float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats,
                               uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap);
int tl_genetic_algorithm_trace_run(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs,
                                   float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost,
                                   tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap);
int tl_genetic_algorithm_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t first_run,
                                    uint32_t count, uint32_t epochs, float mutation_probability, uint32_t n_elite, uint64_t seed, uint32_t *out_pos,
                                    float *out_costs, uint32_t *best_index, tl_stats *stats);
uint64_t tl_ga_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot);
int tl_genetic_algorithm_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t *per_launch, int *threads,
                              uint64_t *workspace_needed);
int tl_ga_selftest_crossover(tl_ctx *ctx, const uint32_t *p1, const uint32_t *p2, uint32_t n, uint32_t from, uint32_t to, uint32_t *out1,
                             uint32_t *out2);

/* ---- the ant colony solver (src/tsp/ant_colony.rs:97-252) ------------------------------------- */
/* The reference's Ant System with its quirks kept, all arithmetic f32.  n <= 2: city order, no device.  With init_pos: best = that
 * tour, tau0 = (float)num_ants / best_cost where best_cost > 0 (else 1) and one deposit of the tour before epoch 0; without: best =
 * a shuffle of city order, tau0 = 1.  tau_min = tau0 1e-4f; eta_beta[u][v] = pow(1.0f / max(d(u, v), 1e-6f), beta), the diagonal 0;
 * per epoch tau_alpha = pow(tau, alpha); every ant, in ant order, draws a start city and makes n - 1 selections (select_next: the
 * weights tau_alpha eta over the unvisited cities in city order, their SEQUENTIAL f32 sum > 0 and finite, else eta only with r2, else
 * the first candidate; roulette_select's strict acc > r sum, the last candidate when the walk is exhausted); its cost is
 * tour_length_by_pos (closing edge first); cost < best_cost is strict and in ant order; then tau *= (1.0f - rate), floored at
 * tau_min, and every ant deposits 1.0f / cost on both cells of each of its edges, in ant order (nothing where cost <= 0).  The
 * result is the best tour and its cost.  epochs = 0 returns the start tour.
 * TWO THINGS ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_aco_oracle.py is the statement;
 * csrc/aco_spec.h the text).  The draws: tl_genetic_algorithm's stream, u(seed, run, event, slot) (tl_aco_draw = tl_ga_draw); ant a
 * of epoch g at step s owns the event (g num_ants + a) n + s: slot 0 of step 0 is the start city, ((u >> 32) n) >> 32; slots 1 and
 * 2 of steps 1 .. n - 1 are r1 and r2, float(u >> 40) 2^-24; the shuffle is the Fisher-Yates pass of the events 2^58 + j, slot 26.
 * The power: tl_aco_pow(x, a), a fixed f64 operation sequence without FMA or library calls, exact at a = 0, 1 and 2.
 * Errors (AcoOptions::validate, mod.rs:1115-1153): alpha not finite or < 0, beta outside [0, 6], evaporation_rate outside (0, 1),
 * num_ants = 0, init_pos not a permutation: TL_ERR_BADARG.  num_ants > 4096, n > tl_ant_colony_max_n, epochs x num_ants x n > 2^58,
 * a context whose flags hold a bit no flag has: TL_ERR_UNSUPPORTED, before anything of size n is read.  dm_packed as in tl_sim_anneal.
 * tl_ant_colony runs run 0.  stats (optional): sweeps = epochs, candidates = tours constructed, moves = improving ants, reversed =
 * selections that left the primary weights; tl_ant_colony_population's stats are these summed over its runs (sweeps = epochs x count).
 * tl_ant_colony_trace: the same plus 3 num_ants words per epoch: every ant's cost bits, then every ant's start city, then every
 * ant's count of fallback selections.  *log_len counts the epochs; the log holds the first log_cap.  route_log (optional, route_cap
 * rows of n + 3 words: epoch, ant, cost bits, the tour; row 0 is the start tour with epoch = ant = 0xFFFFFFFF): the improving ants
 * in the order they improved; *route_len (optional) counts the rows there are.  A caller replays the reference's messages from it:
 * PathUpdate(row 0), per epoch a PathUpdate per row of that epoch and EpochUpdate(epoch), then Done.  tl_ant_colony_trace_run: the
 * same for run `run` of the seed.
 * tl_ant_colony_population: runs first_run .. first_run + count - 1, each its own stream of draws, at once (more runs than the
 * workspace limit holds — tl_ant_colony_plan's per_launch — go in further sequences).  init_count: 0, 1 (one tour for every run) or
 * count.  out_pos, out_costs, *best_index, count == 0: as tl_tabu_search_population.  Run c of any batch equals first_run = c, count = 1.
 * Host-only queries: tl_aco_draw; tl_aco_pow; tl_ant_colony_plan — the runs one launch sequence holds, the threads of a construct
 * workgroup and the workspace bytes of min(count, per_launch) runs (outputs optional; all 0 where n is outside 3 .. the limit or
 * num_ants outside 1 .. 4096; the entries plan with 8 GiB); tl_ant_colony_max_n: the largest n (a construct workgroup keeps 12 bytes
 * per city in LDS beside its tiles; a run keeps 12 n^2 bytes of workspace).
 * tl_aco_selftest_select: the DEVICE's selection for one ant on a given row: weights and eta hold n f32 each, visited n words (non-zero:
 * not a candidate; at least one candidate, 1 <= n <= the limit, else TL_ERR_BADARG).  out[0] the chosen city, out[1] the path that
 * chose it (0 primary, 1 eta only, 2 first candidate), out[2] the primary total's bits, out[3] the eta total's bits (0 on path 0). */
uint32_t tl_ant_colony_max_n(const tl_ctx *ctx);
int tl_ant_colony(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, float alpha, float beta,
                  float evaporation_rate, uint32_t num_ants, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_ant_colony_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, float alpha, float beta,
                        float evaporation_rate, uint32_t num_ants, uint64_t seed, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log,
                        uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *route_len);
int tl_ant_colony_trace_run(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t epochs, float alpha,
                            float beta, float evaporation_rate, uint32_t num_ants, uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost,
                            tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len, uint32_t *route_log, uint32_t route_cap,
                            uint32_t *route_len);
int tl_ant_colony_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                             uint32_t first_run, uint32_t count, uint32_t epochs, float alpha, float beta, float evaporation_rate, uint32_t num_ants,
                             uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *best_index, tl_stats *stats);
uint64_t tl_aco_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot);
float tl_aco_pow(float x, float a);
int tl_ant_colony_plan(uint32_t n, uint32_t num_ants, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t *per_launch, int *threads,
                       uint64_t *workspace_needed);
int tl_aco_selftest_select(tl_ctx *ctx, const float *weights, const float *eta, const uint32_t *visited, uint32_t n, float r1, float r2, uint32_t *out);

/* ---- the particle swarm solver (src/tsp/particle_swarm.rs:22-129) ---------------------------- */
/* The reference's discrete particle swarm with its quirks kept.  P = max(n_nearest, 30) particles (the count rides on
 * HeuristicOptions::n_nearest), v_max = max(ceil(0.35 n), 1) in f64.  Particle 0 starts on init_pos if given, every other particle
 * (and particle 0 without init_pos) on a Fisher-Yates shuffle of city order; velocities start empty; pbest = the start positions,
 * their costs tour_length as everywhere here (closing edge first, sequential f32); gbest = the FIRST minimum.  Epoch e:
 * w = 0.9 - (0.9 - 0.4) (e / max(epochs, 1)) in f64; the particles IN INDEX ORDER: r1, r2 in [0, 1);
 * inertia_keep = round(w len(v)), cog_keep = round((1.5 r1) len(cog)), soc_keep = round((1.5 r2) len(soc)), round half away from
 * zero, a keep above its length clamped by `take`; cog = swap_sequence(pos, pbest) and soc = swap_sequence(pos, gbest), both from
 * the SAME pos, lists of position pairs (route.rs:118-134: for i = 0 .. n - 2, where pos[i] differs from the target, the pair (i, j)
 * with j > i the place of target[i], applied before i + 1 is looked at); new_vel = v[:inertia_keep] ++ cog[:cog_keep] ++
 * soc[:soc_keep] truncated to v_max; pos = the swaps applied in order; cost < pbest_cost updates pbest, cost < gbest_cost updates
 * gbest AT ONCE — the next particle of the same epoch sees it.  The result is gbest and its cost; epochs = 0 returns the start gbest.
 * TWO THINGS ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_pso_oracle.py is the statement;
 * csrc/pso_spec.h the text).  The draws: tl_genetic_algorithm's stream, u(seed, run, event, slot) (tl_pso_draw = tl_ga_draw);
 * particle i of epoch e owns the event e P + i, r1 on slot 0 and r2 on slot 1, each (u >> 11) 2^-53; start particle i owns the events
 * 2^58 + i n + j, slot 26: step j = n - 1 .. 1 of its pass, swap(a[j], a[position(u, j + 1)]).  The rounding: tl_pso_keep(x) =
 * t + (x - t >= 0.5) with t = trunc(x) for x >= 0 (0 for x < 0 or NaN), every f64 product left to right without FMA; tl_pso_weight
 * is w above.
 * On the device (csrc/particle_swarm.hip) every particle of an epoch is moved at once against the epoch-start gbest; a commit
 * launch then walks the particles in index order and, from the first one that improves gbest, moves the later ones again against
 * the new gbest, one after the other — the reference's order in two launches per epoch.  The swap sequences come from their orbit
 * form, one lane per position.
 * opts NULL: the defaults (10 000 epochs, n_nearest 3).  n = 0: TL_OK, nothing written, cost 0 (the reference returns the empty
 * route, as tl_ant_colony).  n = 1: the one city at cost 0, no device work.  init_pos not a permutation: TL_ERR_BADARG.
 * epochs = 2^32 - 1, more than 4096 particles, n > tl_particle_swarm_max_n, a context whose flags hold a bit no flag has:
 * TL_ERR_UNSUPPORTED, before anything of size n is read or allocated.  dm_packed as in tl_sim_anneal.
 * tl_particle_swarm runs run 0.  stats (optional): sweeps = epochs, candidates = particle steps (epochs x P), moves = gbest
 * improvements; tl_particle_swarm_population's stats are these summed over its runs.
 * tl_particle_swarm_trace: run `run` of the seed, the same result plus a log of 4 words per record: epoch, particle, cost bits,
 * the index of the record's route in route_log (0xFFFFFFFF beyond route_cap).  Record 0 is the start gbest (epoch 0xFFFFFFFF, the
 * particle it came from); every gbest improvement follows in the order it happened.  *log_len counts the records there are; the log
 * holds the first log_cap, route_log (optional, route_cap x n) the routes of the first route_cap.  epoch_log (optional, epoch_cap
 * rows of 2 P words): for the first epoch_cap epochs every particle's cost bits, then every particle's velocity length, as the
 * epoch leaves them.  A caller replays the reference's messages from the log: PathUpdate(record 0), per epoch a PathUpdate per record
 * of that epoch and EpochUpdate(epoch), then Done.  n <= 1: record 0 alone, every epoch row zero.
 * tl_particle_swarm_population: runs first_run .. first_run + count - 1, each its own stream of draws, at once (more runs than the
 * workspace limit holds — tl_particle_swarm_plan's per_launch — go in further launch sequences).  init_count: 0, 1 (one tour for
 * every run) or count.  out_pos, out_costs, out_moves (improvements per run), *best_index, count == 0: as tl_sim_anneal_population.
 * Run c of any batch equals first_run = c, count = 1.
 * Host-only queries: tl_pso_draw; tl_pso_weight; tl_pso_keep; tl_particle_swarm_plan — the particles, the threads of a particle's
 * workgroup and the runs one launch sequence holds (outputs optional; all 0 where n is outside 2 .. the limit or P > 4096; a flag bit
 * no flag has: TL_ERR_UNSUPPORTED; the entries plan with 8 GiB).  tl_particle_swarm_max_n: the largest n (a workgroup keeps
 * 14 n + 4 v_max bytes in LDS).
 * tl_pso_selftest_swap_sequence: the DEVICE's swap sequence on `count` given pairs of permutations of 0..n-1 (from, to: count x n;
 * 1 <= n <= the limit, 1 <= count <= 65535, else TL_ERR_BADARG): out_len[c] is the length of pair c's sequence, out_pairs
 * (count x n x 2) its pairs (i, j), 0xFFFFFFFF beyond the length. */
typedef struct tl_pso_opts { /* HeuristicOptions, src/tsp/mod.rs:596-611: what particle_swarm reads of it */
    uint32_t epochs;
    uint32_t n_nearest; /* P = max(n_nearest, 30) */
} tl_pso_opts;
uint32_t tl_particle_swarm_max_n(const tl_ctx *ctx);
int tl_particle_swarm(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_pso_opts *opts, uint64_t seed,
                      uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_particle_swarm_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_pso_opts *opts,
                            uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                            uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap);
int tl_particle_swarm_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                 uint32_t first_run, uint32_t count, const tl_pso_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                 uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_pso_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot);
double tl_pso_weight(uint32_t epoch, uint32_t epochs);
uint32_t tl_pso_keep(double x);
int tl_particle_swarm_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                           uint32_t *particles, int *threads, uint32_t *per_launch);
int tl_pso_selftest_swap_sequence(tl_ctx *ctx, const uint32_t *from, const uint32_t *to, uint32_t n, uint32_t count, uint32_t *out_pairs,
                                  uint32_t *out_len);

/* ---- the cuckoo search solver (src/tsp/cuckoo_search.rs:26-136) ------------------------------- */
/* The reference's cuckoo search with its quirks kept.  N = max(n_nearest, 25) nests, pa = clamp((f64) mutation_probability, 0.01,
 * 0.99) (tl_cs_pa; the default 0.001 gives 0.01).  Nest 0 starts on init_pos if given, every other nest (and nest 0 without
 * init_pos) on a Fisher-Yates shuffle of city order; costs are tour_length as everywhere here (closing edge first, sequential f32).
 * best is a COPY of the FIRST minimum nest and from then on no nest's property.  Epoch e, the cuckoos IN INDEX ORDER c = 0 .. N - 1:
 * k = clamp(ceil(|levy| (n 0.1)) as usize, 1, n / 2) (tl_cs_flight_length: NaN gives 1, +inf n / 2); k times i = range(0 .. n - 1),
 * j = range(i + 1 .. n), reverse [i ..= j] — from nest c AS IT STANDS, so a cuckoo whose nest an earlier flight of the epoch has
 * overwritten flies from the new tour; the target t = range(0 .. N) AFTER the flight (c = t is allowed); new_cost < costs[t]
 * (strict) replaces nest t, and if also < best_cost, best.  Then the nests in index order: r < pa replaces the nest UNCONDITIONALLY
 * by a fresh shuffle, with the same best rule.  The result is best and its cost; epochs = 0 returns the start best.
 * THE DRAWS AND THE LEVY STEP ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_cs_oracle.py
 * is the statement; csrc/cs_spec.h and csrc/levy_spec.h the text).  The draws: tl_genetic_algorithm's stream, u(seed, run, event,
 * slot) (tl_cs_draw = tl_ga_draw); cuckoo c and nest c of epoch e own the events B .. B + n, B = (e N + c)(n + 1): event B holds
 * the Levy words on slots 0-3, v's four resample pairs on slots 4-11, the target on slot 12 (position(u, N)) and the abandonment
 * trial on slot 13 ((u >> 11) 2^-53 < pa); event B + 1 + r, slots 0 / 1, reversal r: i = position(u, n - 1),
 * j = i + 1 + position(u', n - 1 - i); event B + 1 + j, slot 2, step j = n - 1 .. 1 of the replacement's shuffle; start nest i owns
 * the events 2^58 + i n + j, slot 26.  epochs N (n + 1) > 2^58: TL_ERR_UNSUPPORTED.  The Levy step (tl_levy_from_words: the 12
 * words in, the signed step out, *resamples (optional) the further pairs v took) is Mantegna's (probability.rs:8-22) in f64 with a
 * fixed sequence for log, cos(2 pi u) — an exact quadrant reduction — and the power, IEEE sqrt and /; v = 0 (u2 = 1/4 or 3/4) takes
 * the next pair, at most four times, and is 1.0 after the last.
 * On the device (csrc/cuckoo_search.hip) every flight of an epoch is built at once from the epoch-start nests — the k reversals as
 * a gather, each output position followed back through them — and every replacement whose trial succeeds; a commit launch walks
 * the cuckoos in order, flies a cuckoo again where its nest has been overwritten earlier in the epoch, and applies the abandonments.
 * opts NULL: the defaults (10 000 epochs, n_nearest 3, mutation_probability 0.001).  n <= 1 with epochs >= 1: TL_ERR_REF_PANICS
 * (clamp(1, n / 2) with min > max panics); with epochs = 0, n = 0: TL_OK, nothing written, cost 0; n = 1: the one city at cost 0.
 * init_pos not a permutation, mutation_probability not finite or outside [0, 1] (CSOptions::validate): TL_ERR_BADARG.
 * epochs = 2^32 - 1, more than 4096 nests, n > tl_cuckoo_search_max_n, a context whose flags hold a bit no flag has:
 * TL_ERR_UNSUPPORTED, before anything of size n is read or allocated.  dm_packed as in tl_sim_anneal.
 * tl_cuckoo_search runs run 0.  stats (optional): sweeps = epochs, candidates = flights (epochs x N), moves = best improvements;
 * tl_cuckoo_search_population's stats are these summed over its runs.
 * tl_cuckoo_search_trace: run `run` of the seed, the same result plus a log of 4 words per record: epoch, source, cost bits, the
 * index of the record's route in route_log (0xFFFFFFFF beyond route_cap).  source is the cuckoo for a flight, N + the nest for an
 * abandonment.  Record 0 is the start best (epoch 0xFFFFFFFF, the nest it was copied from); every best improvement follows in the
 * order it happened.  *log_len counts the records there are; the log holds the first log_cap, route_log (optional, route_cap x n)
 * the routes of the first route_cap.  epoch_log (optional, epoch_cap rows of 4 N words): for the first epoch_cap epochs every
 * nest's cost bits as the epoch leaves them; every cuckoo's k; every cuckoo's target, bit 31 set when accepted, bit 30 when its
 * source nest had been overwritten earlier in the epoch; every nest's abandoned flag.  A caller replays the reference's messages
 * from the log: PathUpdate(record 0), per epoch a PathUpdate per record of that epoch and EpochUpdate(epoch), then Done.
 * tl_cuckoo_search_population: as tl_particle_swarm_population.  Run c of any batch equals first_run = c, count = 1.
 * Host-only queries: tl_cs_draw; tl_levy_from_words; tl_cs_flight_length (0 for n < 2); tl_cs_pa; tl_cuckoo_search_plan — the
 * nests, the threads of a workgroup and the runs one launch sequence holds (outputs optional; all 0 where n is outside 2 .. the
 * limit or N > 4096; a flag bit no flag has: TL_ERR_UNSUPPORTED; the entries plan with 8 GiB).  tl_cuckoo_search_max_n: the
 * largest n (a workgroup keeps 10 n bytes in LDS).
 * tl_cs_selftest_levy: the DEVICE's Levy step on `count` given tuples of 12 words: its bits, tl_cs_flight_length(|step|, n) and
 * the resamples (n >= 2, 1 <= count <= 2^24, else TL_ERR_BADARG).  tl_cs_selftest_reversals: the DEVICE's gather on `count` given
 * rows of n elements (each <= 65535) and lists of lens[c] <= kcap <= n / 2 pairs (i, j), 0 <= i < j < n (pairs: count x kcap x 2):
 * out (count x n) is each row after its reversals in order. */
typedef struct tl_cs_opts { /* CSOptions, src/tsp/mod.rs:913-925: what cuckoo_search reads of it */
    uint32_t epochs;
    uint32_t n_nearest; /* N = max(n_nearest, 25) */
    float mutation_probability;
} tl_cs_opts;
uint32_t tl_cuckoo_search_max_n(const tl_ctx *ctx);
int tl_cuckoo_search(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_cs_opts *opts, uint64_t seed,
                     uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_cuckoo_search_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_cs_opts *opts,
                           uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                           uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap);
int tl_cuckoo_search_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                uint32_t first_run, uint32_t count, const tl_cs_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_cs_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot);
double tl_levy_from_words(const uint64_t *words, uint32_t *resamples);
uint32_t tl_cs_flight_length(double levy, uint32_t n);
double tl_cs_pa(float mutation_probability);
int tl_cuckoo_search_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                          uint32_t *nests, int *threads, uint32_t *per_launch);
int tl_cs_selftest_levy(tl_ctx *ctx, const uint64_t *words, uint32_t count, uint32_t n, uint64_t *out_bits, uint32_t *out_k, uint32_t *out_resamples);
int tl_cs_selftest_reversals(tl_ctx *ctx, const uint32_t *tours, const uint32_t *pairs, const uint32_t *lens, uint32_t n, uint32_t kcap, uint32_t count,
                             uint32_t *out);

/* ---- the flower pollination solver (src/tsp/flower_pollination.rs:53-151) --------------------- */
/* The reference's flower pollination with its quirks kept.  N = max(n_nearest, 25) flowers; switch_prob = 0.8 if
 * mutation_probability < 0.01 (compared in f32: the default 0.001 gives 0.8), else (f64) mutation_probability (tl_fpa_switch_prob).
 * Flower 0 starts on init_pos if given, every other flower (and flower 0 without init_pos) on a Fisher-Yates shuffle of city order;
 * costs are tour_length as everywhere here (closing edge first, sequential f32).  gbest is a COPY of the FIRST minimum flower.
 * Epoch e, the flowers IN INDEX ORDER i = 0 .. N - 1: u < switch_prob is a GLOBAL pollination — seq = swap_sequence(flower i, gbest);
 * empty: the flower comes back unchanged and nothing further is drawn; else the first clamp(ceil(|levy| len 0.5) as usize, 1, len)
 * swaps of it (tl_fpa_global_swaps: the product left to right, NaN gives 1, +inf len) are applied to flower i.  Otherwise a LOCAL
 * one: j among the flowers other than i, k among those other than i and j, seq = swap_sequence(flower j, flower k) from the
 * flowers AS THEY STAND; empty: unchanged; else its first clamp(ceil(epsilon len) as usize, 1, len) swaps (tl_fpa_local_swaps) are
 * applied to FLOWER i.  new_cost < costs[i] (strict: an unchanged flower is never accepted) replaces flower i, and if also
 * < gbest_cost, gbest AT ONCE — the next flower of the same epoch sees it.  The result is gbest and its cost; epochs = 0 returns
 * the start gbest.
 * THE DRAWS ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_fpa_oracle.py is the statement;
 * csrc/fpa_spec.h the text; the Levy step is tl_levy_from_words, unchanged).  tl_genetic_algorithm's stream, u(seed, run, event,
 * slot) (tl_fpa_draw = tl_ga_draw); flower i of epoch e owns the event e N + i: slot 0 the switch trial ((u >> 11) 2^-53 <
 * switch_prob), slots 1-12 the Levy words, slot 13 j = position(u, N - 1) stepped over i, slot 14 k = position(u, N - 2) stepped
 * over i and j in ascending order (tl_fpa_partners: the reference's rejection loop has the same distribution), slot 15 epsilon;
 * start flower i owns the events 2^58 + i n + j, slot 26, as the swarm's and the nests' do.  A draw the reference would not have
 * made is not read.
 * On the device (csrc/flower_pollination.hip) every move of an epoch is built at once against the epoch-start state; a commit
 * launch walks the flowers in order and builds a flower again where its staged move read something that has since changed (a
 * global move after gbest changed; a local move whose j or k was accepted earlier in the epoch).
 * opts NULL: the defaults (10 000 epochs, n_nearest 3, mutation_probability 0.001: FPAOptions::default).  n = 0 and n = 1: the
 * reference does not panic (every sequence is empty, nothing is accepted) — TL_OK, the empty route or the one city at cost 0.
 * init_pos not a permutation, mutation_probability not finite or outside [0, 1] (FPAOptions::validate): TL_ERR_BADARG.
 * What validate lets through and the port cannot run — epochs = 2^32 - 1, more than 4096 flowers, n > tl_flower_pollination_max_n —
 * and a context whose flags hold a bit no flag has: TL_ERR_UNSUPPORTED, before anything of size n is read or allocated.
 * dm_packed as in tl_sim_anneal.
 * tl_flower_pollination runs run 0.  stats (optional): sweeps = epochs, candidates = moves built (epochs x N), moves = gbest
 * improvements; tl_flower_pollination_population's stats are these summed over its runs.
 * tl_flower_pollination_trace: run `run` of the seed, the same result plus a log of 4 words per record: epoch, flower, cost bits,
 * the index of the record's route in route_log (0xFFFFFFFF beyond route_cap).  Record 0 is the start gbest (epoch 0xFFFFFFFF, the
 * flower it was copied from); every gbest improvement follows in the order it happened.  *log_len counts the records there are;
 * the log holds the first log_cap, route_log (optional, route_cap x n) the routes of the first route_cap.  epoch_log (optional,
 * epoch_cap rows of 4 N words): for the first epoch_cap epochs every flower's cost bits as the epoch leaves them; every flower's
 * move — bit 31 set: global, else j | k << 12; every move's sequence length | prefix length << 16 (0 for an empty sequence); bit 0
 * accepted, bit 1 built again by the commit.  A caller replays the reference's messages from the log: PathUpdate(record 0), per
 * epoch a PathUpdate per record of that epoch and EpochUpdate(epoch), then Done.
 * tl_flower_pollination_population: as tl_particle_swarm_population.  Run c of any batch equals first_run = c, count = 1.
 * Host-only queries: tl_fpa_draw; tl_fpa_switch_prob; tl_fpa_global_swaps and tl_fpa_local_swaps (0 for len = 0); tl_fpa_partners
 * (3 <= flowers <= 4096, i < flowers, else TL_ERR_BADARG); tl_flower_pollination_plan — the flowers, the threads of a workgroup
 * and the runs one launch sequence holds (outputs optional; all 0 where n is outside 2 .. the limit or N > 4096; a flag bit no
 * flag has: TL_ERR_UNSUPPORTED; the entries plan with 8 GiB, at most 65 535 runs a sequence).  tl_flower_pollination_max_n: the
 * largest n (a workgroup keeps 10 n bytes in LDS).
 * tl_fpa_selftest_pollinate: the DEVICE's move on `count` given tuples of three permutations of 0 .. n - 1 (count x n each) and a
 * prefix length: out_len[c] is the length of swap_sequence(source, target), out (count x n) flower c after the first
 * min(prefix[c], out_len[c]) swaps of it (1 <= n <= the limit, 1 <= count <= 65535, else TL_ERR_BADARG). */
typedef struct tl_fpa_opts { /* FPAOptions, src/tsp/mod.rs:998-1010: what flower_pollination reads of it */
    uint32_t epochs;
    uint32_t n_nearest; /* N = max(n_nearest, 25) */
    float mutation_probability;
} tl_fpa_opts;
uint32_t tl_flower_pollination_max_n(const tl_ctx *ctx);
int tl_flower_pollination(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_fpa_opts *opts, uint64_t seed,
                          uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_flower_pollination_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_fpa_opts *opts,
                                uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap);
int tl_flower_pollination_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                     uint32_t first_run, uint32_t count, const tl_fpa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                     uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_fpa_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot);
double tl_fpa_switch_prob(float mutation_probability);
uint32_t tl_fpa_global_swaps(double levy, uint32_t len);
uint32_t tl_fpa_local_swaps(double epsilon, uint32_t len);
int tl_fpa_partners(uint64_t seed, uint32_t run, uint32_t epoch, uint32_t i, uint32_t flowers, uint32_t *j, uint32_t *k);
int tl_flower_pollination_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                               uint32_t *flowers, int *threads, uint32_t *per_launch);
int tl_fpa_selftest_pollinate(tl_ctx *ctx, const uint32_t *flower, const uint32_t *source, const uint32_t *target, const uint32_t *prefix, uint32_t n,
                              uint32_t count, uint32_t *out, uint32_t *out_len);

/* ---- the gravitational search solver (src/tsp/gravitational_search.rs:23-145) ------------------ */
/* The reference's gravitational search with its quirks kept.  N = max(n_nearest, 25) agents; agent 0 starts on init_pos if given,
 * every other agent (and agent 0 without init_pos) on a Fisher-Yates shuffle of city order; costs are tour_length as everywhere
 * here (closing edge first, sequential f32).  gbest is a COPY of the FIRST minimum agent.
 * Epoch e, from the costs at its start: worst = the f32 maximum; sum_fitness = the f64 sum in agent order of (double)(worst - c),
 * the subtraction in f32; below f64::EPSILON every mass is 1 / N, else mass_a = (double)(worst - c_a) / sum_fitness.  kbest: the
 * first ceil(N / 2) agents by descending mass.  g = 20 exp(-(1.0 e) / max(epochs, 1)).  Then the agents IN INDEX ORDER: INERTIA_W
 * is 0, nothing of the old velocity is kept; for j in kbest order, j != i: n_swaps = round((r g) mass_j) (tl_gsa_pull_swaps: left
 * to right, half away from zero); if not 0, the first n_swaps pairs of swap_sequence(positions[i], positions[j]) — positions[j] AS
 * IT STANDS, an agent of a lower index has already moved in this epoch — are appended; the concatenation is cut to v_max =
 * max(ceil(0.35 n), 1) and applied in order; costs[i] = tour_length; costs[i] < gbest_cost (strict) replaces gbest AT ONCE.  The
 * masses and the ranking stay those of the epoch's start.  The result is gbest and its cost; epochs = 0 returns the start gbest.
 * THREE THINGS ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_gsa_oracle.py is the
 * statement; csrc/gsa_spec.h the text).  The draws: tl_genetic_algorithm's stream, u(seed, run, event, slot) (tl_gsa_draw =
 * tl_ga_draw); the pull of agent j on agent i in epoch e owns the event (e N + i) N + j — the agent index, not its rank — and r is
 * slot 0, (u >> 11) 2^-53; start agent i owns the events 2^58 + i n + j, slot 26, as the swarm's do; a draw the reference would
 * not have made (j == i, j outside kbest) is not read.  The order among EQUAL masses: the reference's sort_unstable_by leaves it
 * unspecified; here ties go in ASCENDING AGENT INDEX (tl_gsa_masses).  exp: the fixed f64 sequence of the Levy step
 * (tl_gsa_g), not libm's.  Since r < 1, g <= 20 and mass <= 1, n_swaps <= 20.
 * On the device (csrc/gravitational_search.hip) one workgroup per run walks the agents in order; the pulls of an agent are
 * computed at once, a wave each, and only the first n_swaps pairs of a sequence are looked for.  The schedule is one launch per
 * span of up to 4096 epochs, or of up to opts->span_epochs where that is not 0 (1: one launch per epoch).  Same results: the
 * cross-check form.  (It is an option and not a context flag because the 31 flag bits are all given out.)
 * opts NULL: the defaults (10 000 epochs, n_nearest 3: HeuristicOptions::default; span_epochs 0).  n = 0 and n = 1: the reference does not
 * panic — TL_OK, the empty route or the one city at cost 0.  A start cost that is NaN, or a mass that is NaN at an epoch's start
 * (a cost that is not finite: only the matrix form can produce one): TL_ERR_REF_PANICS (partial_cmp(..).unwrap()), found on the
 * device and reported after the launches; the outputs are then unspecified.  init_pos not a permutation: TL_ERR_BADARG.
 * epochs = 2^32 - 1, more than 4096 agents, n > tl_gravitational_search_max_n and a context whose flags hold a bit no flag has:
 * TL_ERR_UNSUPPORTED, before anything of size n is read or allocated.  dm_packed as in tl_sim_anneal.
 * tl_gravitational_search runs run 0.  stats (optional): sweeps = epochs, candidates = moves (epochs x N), moves = gbest
 * improvements; tl_gravitational_search_population's stats are these summed over its runs.
 * tl_gravitational_search_trace: run `run` of the seed, the same result plus a log of 4 words per record: epoch, agent, cost bits,
 * the index of the record's route in route_log (0xFFFFFFFF beyond route_cap).  Record 0 is the start gbest (epoch 0xFFFFFFFF, the
 * agent it was copied from); every gbest improvement follows in the order it happened.  *log_len counts the records there are;
 * the log holds the first log_cap, route_log (optional, route_cap x n) the routes of the first route_cap.  epoch_log (optional,
 * epoch_cap rows of 3 N + 2 words): for the first epoch_cap epochs every agent's cost bits after its move; every agent's
 * velocity length (after the cut to v_max); every agent's live pulls (the j of kbest other than i with n_swaps > 0, cut or not);
 * then the bits of g, low word first.  The reference's message sequence is PathUpdate(record 0), per epoch a PathUpdate per record
 * of that epoch and EpochUpdate(epoch), then Done.
 * tl_gravitational_search_population: as tl_particle_swarm_population.  Run c of any batch equals first_run = c, count = 1.
 * Host-only queries: tl_gsa_draw; tl_gsa_g; tl_gsa_pull_swaps; tl_gsa_masses — the masses of `agents` costs and out_rank, the
 * agents by rank (1 <= agents <= 4096, else TL_ERR_BADARG; a NaN mass: TL_ERR_REF_PANICS, the masses written, the ranks not);
 * tl_gravitational_search_plan — the agents, the threads of the epochs' workgroup and the runs one launch sequence holds (outputs
 * optional; all 0 where n is outside 2 .. the limit or N > 4096; a flag bit no flag has: TL_ERR_UNSUPPORTED; the entries plan
 * with 8 GiB, at most 65 535 runs a sequence).  tl_gravitational_search_max_n: the largest n (a workgroup keeps 8 n bytes in LDS).
 * tl_gsa_selftest_pull: the DEVICE's pull on `count` given pairs of permutations of 0 .. n - 1 (count x n each) and a prefix
 * length each (<= 20): out_len[c] = min(prefix[c], the length of swap_sequence(from, target)), out_pairs (count x 20 words) its
 * first out_len[c] pairs, i | j << 16, then 0xFFFFFFFF (1 <= n <= the limit, 1 <= count <= 65535, else TL_ERR_BADARG). */
typedef struct tl_gsa_opts { /* HeuristicOptions, src/tsp/mod.rs:596-611: what gravitational_search reads of it */
    uint32_t epochs;
    uint32_t n_nearest;
    uint32_t span_epochs; /* not the reference's: epochs of one launch at most; 0: the default, 4096.  The result does not depend on it */
} tl_gsa_opts;
uint32_t tl_gravitational_search_max_n(const tl_ctx *ctx);
int tl_gravitational_search(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_gsa_opts *opts, uint64_t seed,
                            uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_gravitational_search_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_gsa_opts *opts,
                                  uint64_t seed, uint32_t run, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                                  uint32_t *log_len, uint32_t *route_log, uint32_t route_cap, uint32_t *epoch_log, uint32_t epoch_cap);
int tl_gravitational_search_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                                       uint32_t first_run, uint32_t count, const tl_gsa_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                                       uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_gsa_draw(uint64_t seed, uint32_t run, uint64_t event, uint32_t slot);
double tl_gsa_g(uint32_t epoch, uint32_t epochs);
uint32_t tl_gsa_pull_swaps(double r, double g, double mass);
int tl_gsa_masses(const float *costs, uint32_t agents, double *out_masses, uint32_t *out_rank);
int tl_gravitational_search_plan(uint32_t n, uint32_t n_nearest, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                                 uint32_t *agents, int *threads, uint32_t *per_launch);
int tl_gsa_selftest_pull(tl_ctx *ctx, const uint32_t *from, const uint32_t *target, const uint32_t *prefix, uint32_t n, uint32_t count, uint32_t *out_pairs,
                         uint32_t *out_len);

/* ---- the Kohonen self-organising map solver (src/tsp/som.rs:12-186) ---------------------------- */
/* The reference's SOM with its quirks kept.  n < 2: the trivial route.  A start tour is ignored (the entries take none).  The
 * cities are normalised per axis in f64 with span max(max - min, 1e-9); the centroid is a sequential f64 sum in city order;
 * M = n neuron_multiplier neurons start on a circle of radius 0.1 around it.  For t = 1 .. epochs: eta = eta0 exp(-t / epochs),
 * sigma = max(sigma0 exp(-t / epochs), 1.0) with sigma0 = radius_fraction M; one city is drawn with replacement; the BMU is the
 * FIRST minimum of (nx - cx)^2 + (ny - cy)^2; every neuron at ring distance d = min(|i - bmu|, M - |i - bmu|) gets
 * h = exp(((-d) d) / (2 sigma^2)), is skipped when h < 1e-3, else neuron += (eta h) (city - neuron) per axis, in place.  The tour:
 * every city's first-minimum neuron, the cities sorted by (neuron, distance, city index).  The cost: the f32 sequential
 * tour_length (tl_tour_length), from dm_packed where one is given, else from xy.
 * THREE THINGS ARE THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_som_oracle.py is the
 * statement; csrc/som_spec.h the text) — the reference draws from an unseeded RNG and calls libm, so no run of it can be
 * reproduced.  The draw: the city of epoch t of run r is position(u(seed, r, event t, slot 0), n) on tl_genetic_algorithm's stream
 * (tl_som_draw).  exp: the fixed f64 sequence of the Levy step, for the schedule and for h; a neuron with
 * y = ((-d) d) / two_sigma_sq < -8.0 is skipped without an exp (exp(-8) = 3.4e-4 is below the cut) (tl_som_h, tl_som_schedule).
 * The start ring: cos and sin of 2 pi (i / M) from the Levy step's exact quadrant reduction and its two polynomials
 * (tl_som_ring_init).  All f64, no fused multiply-add.
 * The map trains on the COORDINATES: xy is required, dm_packed (optional) only prices the tour.  xy NULL, a coordinate that is
 * not finite, or options outside SOMOptions::validate (epochs >= 1, learning_rate and radius_fraction in (0, 1],
 * neuron_multiplier >= 1; also form > 2 or reserved != 0): TL_ERR_BADARG, before anything is launched.  epochs = 2^32 - 1, more than
 * 65 536 neurons, form = 1 with a ring that does not fit the LDS, and a context whose flags hold a bit no flag has:
 * TL_ERR_UNSUPPORTED.  opts NULL: the defaults (100 000 epochs, learning_rate 0.8, radius_fraction 0.1, neuron_multiplier 8).
 * On the device (csrc/kohonen_som.hip) one workgroup per run keeps the ring in LDS (form 1: 512 + 16 M bytes) or, where it does
 * not fit, in the run's workspace block (form 2) — the same kernel body and the same result; opts->form forces either.
 * tl_kohonen_som runs run 0.  stats (optional): sweeps = epochs, candidates = epochs x M, summed over the runs of a population.
 * tl_kohonen_som_trace: run `run` of the seed, the same result plus log (optional, log_cap rows of 2 words): (city, bmu) of epoch
 * t at row t - 1; out_ring (optional): the final ring, x[M] then y[M]; and one record per progress message pair of the reference
 * (som.rs:117-145), in its order: with checkpoint = max(epochs / 10, 1), for every t with t % checkpoint == 0 the record
 * (cp_epochs = t, the tour extracted then, its cost bits) — EpochUpdate(t) then PathUpdate —, and where epochs % checkpoint != 0
 * one last record with cp_epochs = 0xFFFFFFFF: the final PathUpdate.  Then Done.  *cp_len counts the records there are (at most
 * 19); cp_epochs, cp_tours (cp_cap x n) and cp_cost_bits hold the first cp_cap.
 * tl_kohonen_som_population: runs first_run .. first_run + count - 1 of the seed at once; out_pos count x n, out_costs and
 * best_index (lowest cost, then lowest index) optional.  Run c of any batch equals first_run = c, count = 1.
 * Host-only queries: tl_som_draw — the city of an epoch; tl_som_schedule — eta, sigma, two_sigma_sq and the update's radius of
 * epoch 1 <= t <= epochs for 1 <= M <= 65 536 (else TL_ERR_BADARG; outputs optional); tl_som_h — 1 and h where a neuron at ring
 * distance d is moved, 0 where it is skipped (h = 0 where no exp was taken); tl_som_ring_init — the start ring (x[M] then y[M]) and
 * optionally the normalised cities (x[n] then y[n]); tl_kohonen_som_plan — the neurons, the threads of the training workgroup
 * (about eight neurons a lane in whole waves: clamp(round_up(ceil(M / 8), 64), 64, 1024)), the form and the runs one launch
 * sequence holds (outputs optional; all 0 where n < 2, M > 65 536, form 1 does not fit or the workspace holds no run; the entries
 * plan with opts->work_bytes, 8 GiB where that is 0, at most 65 535 runs a sequence); tl_kohonen_som_max_n — the largest n for a
 * multiplier and a form (0 or 2: the cap on M; 1: the LDS).
 * tl_som_selftest_bmu: the DEVICE's BMU as the training finds it (out_bmu, n words: one reduction per given city, `threads` lanes,
 * 0: the plan's) and as the extraction finds it (out_extract_bmu, optional), and the extraction's tour (out_tour, optional), on a
 * ring (x[M] then y[M]) and normalised cities (x[n] then y[n]) given by the caller: how exact ties are planted. */
typedef struct tl_som_opts { /* SOMOptions, src/tsp/mod.rs:1465-1499 */
    uint32_t epochs;
    uint32_t neuron_multiplier;
    double learning_rate;
    double radius_fraction;
    uint32_t form;       /* not the reference's: 0 the plan decides, 1 the ring in LDS, 2 the ring in the workspace.  Same result */
    uint32_t reserved;   /* 0 */
    uint64_t work_bytes; /* not the reference's: the workspace one launch sequence plans with; 0: 8 GiB.  Same result */
} tl_som_opts;
uint32_t tl_kohonen_som_max_n(const tl_ctx *ctx, uint32_t neuron_multiplier, uint32_t form);
int tl_kohonen_som(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const tl_som_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_cost,
                   tl_stats *stats);
int tl_kohonen_som_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const tl_som_opts *opts, uint64_t seed, uint32_t run,
                         uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, double *out_ring, uint32_t *cp_epochs,
                         uint32_t *cp_tours, uint32_t *cp_cost_bits, uint32_t cp_cap, uint32_t *cp_len);
int tl_kohonen_som_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, uint32_t first_run, uint32_t count, const tl_som_opts *opts,
                              uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *best_index, tl_stats *stats);
uint32_t tl_som_draw(uint64_t seed, uint32_t run, uint32_t epoch, uint32_t n);
int tl_som_schedule(uint32_t epoch, uint32_t epochs, uint32_t neurons, double learning_rate, double radius_fraction, double *eta, double *sigma,
                    double *two_sigma_sq, uint32_t *radius);
int tl_som_h(double d, double two_sigma_sq, double *h);
int tl_som_ring_init(const float *xy, uint32_t n, uint32_t neuron_multiplier, double *out_ring, double *out_cities);
int tl_kohonen_som_plan(uint32_t n, uint32_t neuron_multiplier, uint32_t form, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes, uint32_t flags,
                        uint32_t *neurons, int *threads, uint32_t *form_out, uint32_t *per_launch);
int tl_som_selftest_bmu(tl_ctx *ctx, const double *ring, uint32_t neurons, const double *cities, uint32_t n, int threads, uint32_t form, uint32_t *out_bmu,
                        uint32_t *out_extract_bmu, uint32_t *out_tour);

/* ---- stochastic hill climb: replaces stochastic_hill::solve (stochastic_hill.rs:7-97) ------------------ */
/* The reference's chain, quirks kept: best = current = the start tour (init_pos, NULL: city order — the reference's own shuffle is
 * the caller's); every epoch draws one candidate of the CURRENT tour (positions from..=to of the open path reversed, the pair by
 * random_position_pair) and prices it with the full tour_length re-sum; the candidate is accepted iff its cost is below the BEST
 * cost (not the current tour's): then current = best = candidate and n_stale = 0, else n_stale += 1.  After the epoch counter's
 * increment, if platoo_epochs > 0 and n_stale > platoo_epochs the current tour is shuffled in place and n_stale = 0; the best stays
 * (after a restart a candidate of the random tour must still beat the best cost, so restarts rarely help: the reference's
 * behaviour).  The restart check precedes the end check, so a restart can fall on the last epoch.  epochs + 1 epochs run; the BEST
 * route is returned, *out_cost the bits of the best cost.
 * THE RANDOM STREAM IS THIS PROJECT'S SPECIFICATION, NOT THE REFERENCE'S (tests/_hill_oracle.py is the
 * statement, csrc/hill_spec.h the text): the reference draws from an unseeded thread RNG.  With
 *   u(seed, chain, event, slot) = mix(mix(seed + G (chain + 1)) + G (32 event + slot + 1))      (tl_hill_draw)
 * the pair of epoch e is tl_sim_anneal's (event e, slots 0 .. 21), and the restart after epoch e (the index before the increment)
 * is the Fisher-Yates pass j = n - 1 .. 1, swap(a[j], a[position(u, j + 1)]), u on slot 26 of the event 2^58 + e n + j.  No draw
 * depends on an earlier one, so `window` consecutive epochs are evaluated at once (csrc/hill_climb.hip: one workgroup per chain,
 * the tour in that CU's LDS); opts->window = 1 is the chain epoch after epoch, and every window gives the same result.
 * opts NULL: the defaults (10 000 epochs, platoo_epochs 500, the plan's window).  epochs = 0 (the reference never ends) and
 * epochs = 2^32 - 1: TL_ERR_UNSUPPORTED.  reserved != 0, window above the threads of the plan: TL_ERR_BADARG.  n < 2:
 * TL_ERR_REF_PANICS (route.rs:87-89); n = 2 and n = 3 run (the 11th pair is taken whatever it is).  n > tl_hill_climb_lds_max_n:
 * TL_ERR_UNSUPPORTED, before anything of size n is read or allocated (no HBM form).  init_pos not a permutation: TL_ERR_BADARG.  A
 * context whose flags hold a bit no flag has: TL_ERR_UNSUPPORTED.  dm_packed as in tl_sim_anneal.
 * tl_hill_climb runs chain 0.  stats (optional): sweeps = candidates = epochs run, moves = acceptances, reversed = elements moved,
 * summed over the chains of a population.
 * tl_hill_climb_trace: the same plus every event in order, 4 words each: an acceptance is (epoch, from, to, the bits of the new
 * best cost), a restart (epoch, 0xFFFFFFFF, 0, 0), epoch the index before the increment — what the reference's messages are
 * replayed from: PathUpdate(start, 0.0), PathUpdate(best, best cost) per acceptance, PathUpdate(shuffled current, 0.0) per restart,
 * Done.  *log_len counts all events; the log holds the first log_cap.  tl_hill_climb_trace_chain: the same for chain `chain`.
 * tl_hill_climb_population: chains first_chain .. first_chain + count - 1, each its own stream of draws, concurrently (more chains
 * than the LDS holds at once — tl_hill_climb_plan's per_launch — run in further launches).  init_count, out_pos, out_costs,
 * out_moves (acceptances), *best_index and its tie rule, count == 0: as tl_tabu_search_population.  Chain c of any population
 * equals first_chain = c, count = 1.
 * Host-only queries (no context, no device): tl_hill_draw — the u64 above; tl_hill_climb_plan — the window (window_request, or
 * where that is 0 the threads), the threads of a chain's workgroup (256 for a chain alone on its CU, 64 once there are more chains
 * than CUs) and the chains one launch holds (outputs optional; all 0 where n is outside 2 .. the limit; window_request above the
 * threads: TL_ERR_BADARG, as cus < 1 or lds_bytes < 0). */
typedef struct tl_hill_opts { /* HeuristicOptions, src/tsp/mod.rs:598-608 */
    uint32_t epochs;
    uint32_t platoo_epochs;
    uint32_t window;   /* not the reference's: 0 the plan's; 1 the chain epoch after epoch; up to the plan's threads.  Same result */
    uint32_t reserved; /* 0 */
} tl_hill_opts;
uint32_t tl_hill_climb_lds_max_n(const tl_ctx *ctx);
int tl_hill_climb(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_hill_opts *opts, uint64_t seed,
                  uint32_t *out_pos, float *out_cost, tl_stats *stats);
int tl_hill_climb_trace(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_hill_opts *opts, uint64_t seed,
                        uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, uint32_t *log_len);
int tl_hill_climb_trace_chain(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, const tl_hill_opts *opts,
                              uint64_t seed, uint32_t chain, uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                              uint32_t *log_len);
int tl_hill_climb_population(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t init_count,
                             uint32_t first_chain, uint32_t count, const tl_hill_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs,
                             uint32_t *out_moves, uint32_t *best_index, tl_stats *stats);
uint64_t tl_hill_draw(uint64_t seed, uint32_t chain, uint64_t event, uint32_t slot);
int tl_hill_climb_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint32_t window_request, uint32_t *window, int *threads, uint32_t *per_launch);

/* ---- Fourier curve: replaces fourier::solve (fourier.rs:10-312) ----------------------------------------- */
/* A closed curve gamma(s) = sum_k c_k e^{2 pi i k s}, |k| <= k_max, sampled at m points, descends towards the cities: k_max stages
 * (stage s frees the modes |k| <= s + 1) of `epochs` gradient steps, lambda multiplied by lambda_decay after each stage; the tour is
 * the cities in the order of their nearest sample (a stable sort: ties in city order), priced by tour_length.  The reference's
 * quirks are kept: n < 2 is the trivial tour; a start tour is ignored and no progress is sent; the centroid, the radius and every
 * coefficient's gradient are sequential f64 sums in city order; only the modes |k| <= k_active are updated.  xy is required (the
 * curve descends on the coordinates); dm_packed, where given, only prices the tour.
 * The solver draws nothing, so there is no seed: a batch is a list of option sets on one problem, one workgroup each.  Job j of a
 * batch equals the single call with opts[j] bit for bit; *best_index is the job of the lowest cost, the lowest index among equals.
 * This project's specification (csrc/fourier_spec.h) departs from the reference in five places: the basis is one
 * table E[(k j) mod m] from an exact quadrant reduction instead of libm's cos and sin of a rounded angle; |z| is sqrt(re re + im im)
 * instead of hypot; the nearest sample is the least f32 sqrt(dx dx + dy dy), the LOWEST index among equal roots (the reference:
 * whichever its kd-tree visits first); (2 pi k)^2 is t t with t = 6.283185307179586 k; lambda is the running product.
 * opts NULL (single call only): the defaults (k_max 4, m 200, lambda 0.05, lambda_decay 0.5, lr 0.05, epochs 400).  What
 * FourierOptions::validate refuses (k_max < 1, m < 2, lambda <= 0, lambda_decay outside (0, 1), lr <= 0, epochs < 1) is
 * TL_ERR_BADARG, as are a coordinate that is not finite, launch parameters that differ inside a batch and a coeff_stride below the
 * largest job's 2 (2 k_max + 1).  The limits are TL_ERR_UNSUPPORTED: k_max > 32, m > 4096, n > 65 536, k_max x epochs >= 2^32, more
 * than 65 535 jobs, a context whose flags hold a bit no flag has.
 * out_pos: jobs x n positions; out_costs (optional): jobs f32; out_coeffs (optional): job j's final coefficients, (re, im) pairs for
 * k = -k_max .. k_max, at out_coeffs + j coeff_stride doubles (the single call: 2 (2 k_max + 1) doubles), the rest zero.  Evidence
 * of job 0 (optional): log — log_cap x n words, every city's nearest sample at step t (of k_max x epochs) in row t; stage_coeffs —
 * k_max x 2 (2 k_max + 1) doubles, the coefficients at the end of every stage.  stats: sweeps = steps of all jobs, candidates =
 * (city, sample) pairs searched.
 * Host-only: tl_fourier_basis — the table E of m (2 m doubles); tl_fourier_init — the start coefficients; tl_fourier_nearest —
 * every city's nearest sample on a given curve (m pairs of f64) by the specification's rule; tl_fourier_curve_plan — the threads of
 * a workgroup, the form (1: everything in LDS, 2: basis, cities and sample indices in the workspace), the chunk and the span a call
 * would run with; tl_fourier_curve_work_bytes — the device workspace such a call takes (0 where it would be refused or n < 2).
 * tl_fourier_selftest_search: the DEVICE's search of the gradient step alone, on a curve given by the caller. */
typedef struct tl_fourier_opts { /* FourierOptions, src/tsp/mod.rs:1341-1384 */
    uint32_t k_max;
    uint32_t m;
    uint32_t epochs;
    uint32_t chunk;      /* not the reference's: cities whose gradient terms are formed at once; 0: 64.  Same result */
    double lambda;
    double lambda_decay;
    double lr;
    uint32_t span_steps; /* not the reference's: gradient steps of one launch; 0: 65 536.  Same result */
    uint32_t threads;    /* not the reference's: lanes of a workgroup, a multiple of 64 in 64 .. 1024, >= 2 (2 k_max + 1); 0: the plan's.  Same result */
} tl_fourier_opts;
int tl_fourier_curve(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const tl_fourier_opts *opts, uint32_t *out_pos, float *out_cost,
                     double *out_coeffs, tl_stats *stats);
int tl_fourier_curve_batch(tl_ctx *ctx, const float *xy, uint32_t n, const float *dm_packed, const tl_fourier_opts *opts, uint32_t jobs, uint32_t *out_pos,
                           float *out_costs, double *out_coeffs, uint32_t coeff_stride, uint32_t *best_index, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                           double *stage_coeffs);
uint64_t tl_fourier_curve_work_bytes(uint32_t n, const tl_fourier_opts *opts, uint32_t jobs, uint32_t log_cap);
int tl_fourier_curve_plan(uint32_t n, const tl_fourier_opts *opts, uint32_t jobs, int lds_bytes, int *threads, uint32_t *form, uint32_t *chunk,
                          uint32_t *span_steps);
int tl_fourier_basis(uint32_t m, double *out);
int tl_fourier_init(const float *xy, uint32_t n, uint32_t k_max, double *out_coeffs);
int tl_fourier_nearest(const double *gamma, uint32_t m, const float *xy, uint32_t n, uint32_t *out_idx);
int tl_fourier_selftest_search(tl_ctx *ctx, const double *gamma, uint32_t m, const float *xy, uint32_t n, int threads, uint32_t *out_idx);

/* ---- Held-Karp lower bound: the minimum 1-tree under node penalties, raised by subgradient ascent ----- */
/* Not a solver and not the reference's: this project's own specification (csrc/one_tree_spec.h,
 * tests/_one_tree_oracle.py).  The result is a LOWER bound on the length of every tour under the same f32 distances d (dist() of
 * the coordinates, or dm_packed), as a double: L = min 1-tree weight under w(i, j) = (double)d(i, j) + (pi_i + pi_j), minus 2 sum pi.
 * A 1-tree with special position `root`: Prim's tree over the other positions (the lowest of them first; the smallest key, the
 * first in position order among equals; a key is lowered only where w is STRICTLY smaller) plus the root's two smallest edges
 * (the lower position among equals).  The ascent starts at pi = 0, lambda = lambda0, and per iteration k: builds the 1-tree; a new
 * best L is kept with its pi and its tree, else after `patience` iterations without one lambda is halved; stops where the 1-tree
 * is a tour (every degree 2: the bound is then the optimum and the tour is written out from the root towards its first chosen
 * neighbour), where lambda < 2^-20, where upper - L_k <= 0; else pi_i += lambda (upper - L_k) / sum g^2 x (degree_i - 2).
 * A batch is a list of option sets on one problem, one workgroup each; job j equals the single call with opts[j] bit for bit, and
 * neither depends on iters_per_launch.  *best_index: the first job with the largest bound.
 * opts is required (upper has no default).  TL_ERR_BADARG: root >= n (n >= 1), iterations < 1, lambda0 not finite or <= 0,
 * patience < 1, upper not finite or <= 0, reserved != 0, more than 65 535 jobs.  TL_ERR_UNSUPPORTED: a coordinate that is not
 * finite or beyond 2^62 in size, a matrix entry that is not finite or is negative (-0.0 included), n > tl_one_tree_bound_max_n
 * (before anything of size n is read).  n <= 2 is answered without a launch: bound 0 (n <= 1) or 2 d(0, 1), is_tour 1, stop 0.
 * Outputs, each optional: results — jobs records; out_pi — jobs x n doubles, the best pi; out_parent — jobs x n, the best tree's
 * parents (TL_ONE_TREE_NONE for the root and for Prim's start); out_tour — jobs x n positions where is_tour, else untouched; log —
 * jobs x log_cap rows of 3 doubles (L_k, sum g^2, lambda after the iteration's halving), rows >= iterations_run untouched.
 * stats: sweeps = iterations of all jobs, candidates = Prim rounds; kernel_ms sums the launches between event pairs and leaves out the
 * host's look at the states after every 16th launch (tl_last_kernel_ms reports the last group of launches only).
 * tl_one_tree_bound_host: the sequential restatement on the CPU (no context, no device), the same contract for one job, any n.
 * tl_one_tree_bound_plan: threads of a workgroup and iterations of a launch for n; tl_one_tree_bound_max_n: the largest n whose
 * state (24 n bytes) fits lds_bytes; tl_one_tree_bound_work_bytes: the device workspace of such a call (0 for n <= 2). */
#define TL_ONE_TREE_NONE 0xFFFFFFFFu
#define TL_ONE_TREE_STOP_TOUR 1u
#define TL_ONE_TREE_STOP_LAMBDA 2u
#define TL_ONE_TREE_STOP_UPPER 3u
#define TL_ONE_TREE_STOP_ITERATIONS 4u
typedef struct tl_one_tree_opts {
    uint32_t root;             /* the 1-tree's special position */
    uint32_t iterations;       /* default of the mirrors: 1000 */
    uint32_t patience;         /* 10 */
    uint32_t iters_per_launch; /* 0: the plan's.  Same result */
    double lambda0;            /* 2.0 */
    double upper;              /* the length of any tour */
    uint64_t reserved;         /* 0 */
} tl_one_tree_opts;
typedef struct tl_one_tree_result {
    double bound;              /* the best L */
    double lambda;             /* at the end */
    uint32_t best_iter;
    uint32_t iterations_run;
    uint32_t stop;             /* TL_ONE_TREE_STOP_* */
    uint32_t is_tour;
    uint32_t root_nb[2];       /* the best tree's root neighbours in the order chosen */
    uint32_t tour_nb[2];       /* those of the 1-tree that was a tour */
} tl_one_tree_result;
int tl_one_tree_bound(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, tl_one_tree_result *result,
                      double *out_pi, uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap, tl_stats *stats);
int tl_one_tree_bound_batch(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, uint32_t jobs,
                            tl_one_tree_result *results, double *out_pi, uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap,
                            uint32_t *best_index, tl_stats *stats);
int tl_one_tree_bound_host(const float *xy, const float *dm_packed, uint32_t n, const tl_one_tree_opts *opts, tl_one_tree_result *result, double *out_pi,
                           uint32_t *out_parent, uint32_t *out_tour, double *log, uint32_t log_cap);
int tl_one_tree_bound_plan(uint32_t n, int lds_bytes, int *threads, uint32_t *iters_per_launch);
uint32_t tl_one_tree_bound_max_n(int lds_bytes);
uint64_t tl_one_tree_bound_work_bytes(uint32_t n, uint32_t jobs, uint32_t log_cap);

/* ---- alpha-nearness candidate lists under given penalties, and Lin-Kernighan on supplied lists ----- */
/* This project's own specification (csrc/alpha_spec.h, tests/_alpha_oracle.py): Helsgaun's alpha-nearness over the
 * two arrays tl_one_tree_bound hands back.  The 1-tree under pi (n doubles, NULL: all zero) with special position `root` is exactly
 * the one described above, w(i, j) = (double)d(i, j) + (pi_i + pi_j); the entry rebuilds it from pi, and for the out_pi of a
 * tl_one_tree_bound call the parents and root neighbours written here equal that call's out_parent and root_nb.
 *   i != j, both != root: beta(i, j) = the largest w on the tree path between i and j; alpha(i, j) = w(i, j) - beta(i, j).
 *   the root r with its neighbours a (chosen first) and b: alpha(r, a) = alpha(r, b) = 0, else alpha(r, j) = w(r, j) - w(r, b);
 *   alpha(j, r) = alpha(r, j).
 * beta is a maximum of doubles and therefore exact, alpha ONE defined subtraction per pair: device, host and numpy agree bit for
 * bit.  alpha >= +0.0 always.  Row i of out_cand (n x k', k' = min(k, n - 1)) holds the positions j != i smallest by
 * (alpha(i, j), w(i, j), j) — the doubles compared as numbers, the position last — in that order; out_alpha (optional, n x k')
 * their values; out_parent (optional, n) and out_root_nb (optional, 2) the tree.
 * TL_ERR_BADARG: root >= n (n >= 1), k == 0, threads neither 0 nor whole waves up to 1024.  TL_ERR_UNSUPPORTED: k > 64,
 * n > tl_alpha_candidates_max_n (both before anything of size n is read); a coordinate or matrix entry tl_one_tree_bound refuses, a
 * penalty that is not finite or beyond 2^1020.  n <= 2 is answered on the host (n == 2: each position's candidate is the other, alpha 0).
 * threads: the workgroup of a source city, 0: the plan's; a launch parameter, the same result.  stats: sweeps = the tree's levels
 * (a source's sweep takes one barrier fewer), candidates = alpha values formed, kernel_ms = the 1-tree's launch plus the rows' kernel.
 * tl_alpha_candidates_host: the sequential O(n^2) restatement on the CPU (no context, no device), the same contract, n <= 65 535.
 * tl_alpha_candidates_plan: the threads of a source's workgroup and the LDS of its row (16 n bytes); tl_alpha_candidates_max_n: the
 * largest n whose 1-tree state (24 n bytes) and row fit lds_bytes.
 *
 * tl_lk_candidates: a setting of the context, like tl_lk_population_setting (the flag bits are used up).  The call copies n x k
 * positions; every later tl_lk, tl_lk_trace, tl_lk_live and tl_lk_population on this context searches these lists instead of the
 * kd-tree's.  cand == NULL or k == 0 clears them, and every LK entry does again exactly what it does without the setting.
 * TL_ERR_BADARG, the message naming the row: a row that holds its own position, a repeat, or a position >= n; also k > 64 and
 * k > n - 1.  While lists are set: an LK call with another n returns TL_ERR_BADARG naming the setting; opts->n_nearest is ignored —
 * the list width is k wherever LK sizes by it (key bits, queue capacity, tl_lk_population_max_n; tl_lk_population_plan takes no
 * context: pass n_nearest = k); the nearest-neighbour seed of init_pos == NULL is untouched.
 * ALPHA CHOOSES THE SET, DISTANCE ORDERS IT: the kernels search a row in ascending f32 Euclidean distance, so at each LK call the
 * stored rows are put into ascending dist(xy_i, xy_j) order — stably: equal distances keep the supplied order — before anything
 * reads them.  The results equal the reference's lin_kernighan on the rows so ordered. */
int tl_alpha_candidates(tl_ctx *ctx, const float *xy, const float *dm_packed, uint32_t n, const double *pi, uint32_t root, uint32_t k,
                        uint32_t threads, uint32_t *out_cand, double *out_alpha, uint32_t *out_parent, uint32_t *out_root_nb, tl_stats *stats);
int tl_alpha_candidates_host(const float *xy, const float *dm_packed, uint32_t n, const double *pi, uint32_t root, uint32_t k, uint32_t *out_cand,
                             double *out_alpha, uint32_t *out_parent, uint32_t *out_root_nb);
int tl_alpha_candidates_plan(uint32_t n, uint32_t k, int lds_bytes, int *threads, uint32_t *lds_used);
uint32_t tl_alpha_candidates_max_n(int lds_bytes);
int tl_lk_candidates(tl_ctx *ctx, const uint32_t *cand, uint32_t n, uint32_t k);

/* ---- device-resident batch entry (bench / pipelines that keep data in HBM) ------------------- */
/* All d_* are DEVICE pointers on the context's device.  d_init: count x n u32 (NULL: seeded restarts
 * first..first+count as above; seed ignored otherwise).  d_out_pos: count x n u32, d_out_cost: count f32,
 * d_out_stats: count x TL_DEV_STATS_STRIDE u64 {sweeps, moves, reversed, status (0 ok, 1 sweep cap reached, 2 d_init holds a
 * position >= n: that descent is refused, its cost is NaN), steps, L0 tile bounds evaluated, candidates into L1, into L2,
 * into L3, shader clocks, 100 MHz ticks, reserved...}.  stream: the hipStream_t to enqueue on,
 * or NULL for the context's own stream — which is NON-BLOCKING, i.e. not ordered with the legacy default stream: a
 * caller that passes NULL must wait on tl_last_kernel_ms() (or a device synchronise) before touching the outputs.
 * Several asynchronous calls on one context may use different streams: the context's shared device workspace (the instance's
 * neighbour lists, grid coordinates) is handed from one kernel sequence to the next through an event, so a call on stream B waits
 * on the device for the previous call's descents on stream A before it rebuilds them (no host synchronisation).
 * Asynchronous: returns after enqueueing — except that a batch with more descents than the device has CUs at 7 100 < n <= 10 240
 * first asks the device whether the coordinates lie on a decimal grid (then two descents share a CU): one 4-byte read-back,
 * i.e. a synchronisation of `stream`, before the descents are enqueued.
 * mode == TL_MODE_BEST_SWEEP: one LDS-resident best-sweep descent per workgroup (csrc/two_opt_best_lds.hip); stats words 0-3 as above,
 * the rest 0; n beyond tl_two_opt_best_lds_max_n or 65535: TL_ERR_UNSUPPORTED (this entry has no loop form). */
int tl_two_opt_batch_dev(tl_ctx *ctx, const float *d_xy, uint32_t n, const uint32_t *d_init,
                         uint64_t seed, uint32_t first, uint32_t count, int mode, uint32_t *d_out_pos,
                         float *d_out_cost, uint64_t *d_out_stats, void *stream);
/* Device time (ms) between the start and end of the most recent *_dev / solver kernel sequence on
 * this context, from HIP events recorded on the launch stream.  Synchronises on the end event. */
int tl_last_kernel_ms(tl_ctx *ctx, double *ms);
int tl_dm_build_dev(tl_ctx *ctx, const float *d_xy, uint32_t n, int dist, int layout, float *d_out,
                    void *stream);
/* Diagnostics: the 16 kernel-side counters of descent 0 of the most recent tl_two_opt / tl_two_opt_trace / tl_two_opt_population /
 * tl_two_opt_multistart call of this context (host-buffer entries; words 0-4: sweeps, moves, reversed elements, status, steps; the
 * rest is per kernel — matrix form: 5 = steps of sweeps run on the lists, 6 = such sweeps, 7 = their rows that walked the matrix rows).
 * TL_ERR_BADARG (with a message) whenever the context does not hold such counters: no 2-opt call yet; the most recent one ran the
 * HBM form or TL_MODE_BEST_SWEEP (no kernel-side counters); or the buffer has been used since by tl_lk_trace / tl_lk_live (their
 * snapshot distances) or tl_two_opt_batch_dev (asynchronous, possibly still writing).
 * Not part of the reference's interface; tests and timing scripts read which form ran from it. */
int tl_two_opt_last_counters(tl_ctx *ctx, uint64_t out[16]);

#ifdef __cplusplus
}
#endif
#endif /* TEELINE_GPU_H */
