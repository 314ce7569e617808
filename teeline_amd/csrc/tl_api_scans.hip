// tl_api_scans.hip — C ABI, the best-improvement scans: tl_three_opt* (src/tsp/three_opt.rs:16-218) and tl_or_opt* (src/tsp/or_opt.rs:18-184),
// tl_or_opt_population and tl_three_opt_population included.
#include "tl_api_common.h"

using namespace tl;
using namespace tlapi;

static constexpr int kScanBatch = 16;  // passes of a 3-opt / Or-opt descent enqueued per host poll (later ones return at once when it ends)

// The descent 3-opt and Or-opt share (three_opt.rs:36-45, or_opt.rs:45: while find_best_move finds a move, apply it): batches of passes
// enqueued back to back (tl_kernels.h ScanRunState) — the pick kernel counts passes and moves, files every move and sets `done` when
// a pass finds none; the host looks once per batch.  who: "three_opt" / "or_opt", the name in the messages.  setup(A) uploads the
// inputs, lays out c->work and fills A; pass(A) enqueues one pass that applies its move; per_pass: the candidates a pass evaluates.
// move_log (optional): 4 words per applied move, in order, at most log_cap moves; *log_len = moves
template <class Args, class Setup, class Pass>
static int scan_descent(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t *out_pos,
                        float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len, uint64_t per_pass, Setup setup,
                        Pass pass)
{
    if (log_len) *log_len = 0;
    if (!c || (!xy && !dm_packed) || !out_pos) return fail(c, TL_ERR_BADARG, "tl_%s: NULL argument", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc;
    if (n < 4) {  // three_opt.rs:25-28, or_opt.rs:31-34: returns the cities order, init_tour ignored
        for (uint32_t i = 0; i < n; ++i) out_pos[i] = i;
        if (out_cost) {
            if (n < 2) *out_cost = 0.0f;
            else if ((rc = tl_tour_length(c, xy, dm_packed, n, out_pos, out_cost))) return rc;
        }
        return TL_OK;
    }
    if (init_pos && !is_permutation(init_pos, n)) return fail(c, TL_ERR_BADARG, "tl_%s: init tour is not a permutation of 0..n-1", who);
    HIPCHK(c, hipSetDevice(c->device));
    Args A{};
    if ((rc = setup(A))) return rc;
    const uint32_t dev_log_cap = move_log ? log_cap : 0u;
    if ((rc = ensure(c, c->misc, 256 + (size_t)(dev_log_cap ? dev_log_cap : 1u) * 16))) return rc;
    A.run = (ScanRunState *)c->misc.p;
    A.log = (uint32_t *)((unsigned char *)c->misc.p + 256);
    const ScanRunState hs0{0u, 0u, 0u, dev_log_cap};
    ScanRunState hs = hs0;
    HIPCHK(c, hipMemcpyAsync(A.run, &hs0, sizeof(hs0), hipMemcpyHostToDevice, c->stream));
    c->ev_valid = false;  // (an early return below must not leave this ev0 paired with an older sequence's ev1)
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    const uint64_t cap = 64ull * n + 1024;  // safety cap, far above any observed pass count
    for (;;) {
        for (int b = 0; b < kScanBatch; ++b) HIPCHK(c, pass(A));
        HIPCHK(c, hipMemcpyAsync(&hs, A.run, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (hs.done) break;
        if (hs.passes > cap) return fail(c, TL_ERR_NO_CONVERGE, "%s: pass cap reached", who);
    }
    const uint64_t passes = hs.passes, moves = hs.moves;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    HIPCHK(c, hipMemcpyAsync(out_pos, A.perm, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (move_log && moves && dev_log_cap)
        HIPCHK(c, hipMemcpyAsync(move_log, A.log, (size_t)(moves < dev_log_cap ? moves : dev_log_cap) * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (out_cost) {
        // Solution::from_parts -> tour_length (mod.rs:1776-1789)
        if ((rc = ensure(c, c->out_cost, 4))) return rc;
        HIPCHK(c, launch_tour_length(A.xy, A.dm, n, A.perm, (float *)c->out_cost.p, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_cost, c->out_cost.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (stats) {
        stats->sweeps = passes;
        stats->moves = moves;
        stats->candidates = passes * per_pass;
        stamp_times(c, stats, t0);
    }
    if (log_len) *log_len = (uint32_t)moves;
    return TL_OK;
}

// The descent of every tour of a population, which tl_or_opt_population and tl_three_opt_population share; tour r's result is the
// single-tour entry's for it alone.  who: "or_opt" / "three_opt", the name in the messages.  run1(init, out, &cost, &stats): the
// chip-wide descent of one tour (or_opt_run / three_opt_run).  plan(P) fills a PopPlan: resident — one workgroup per tour (`threads`
// wide), batch after batch of `batch` tours, each with tour_work bytes of c->work (0: none, and the batch is the whole population) —
// or else the tours one after the other through run1.  launch(A, cnt, threads) enqueues a batch's kernel.  per_pass: the candidates
// a pass evaluates; max_passes: a resident descent still moving after that many passes is TL_ERR_NO_CONVERGE.
struct PopPlan {
    bool resident;
    int threads;
    uint32_t batch;
    size_t tour_work;
};
template <class Run, class Plan, class Launch>
static int population_descent(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t count,
                              uint32_t *out_pos, float *out_costs, uint32_t *out_moves, tl_stats *stats, uint64_t per_pass, uint32_t max_passes, Run run1,
                              Plan plan, Launch launch)
{
    if (!c || (!xy && !dm_packed)) return fail(c, TL_ERR_BADARG, "tl_%s_population: NULL argument", who);
    if (count == 0) return TL_OK;
    if (!out_pos || (n >= 4 && !init_pos)) return fail(c, TL_ERR_BADARG, "tl_%s_population: NULL argument", who);
    if (n >= 4)
        for (uint32_t r = 0; r < count; ++r)
            if (!is_permutation(init_pos + (size_t)r * n, n))
                return fail(c, TL_ERR_BADARG, "tl_%s_population: tour %u is not a permutation of 0..n-1", who, r);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc;
    if (n < 4) {  // three_opt.rs:25-28, or_opt.rs:31-34: the cities' order, init_tour ignored
        float cst = 0.0f;
        for (uint32_t k = 0; k < n; ++k) out_pos[k] = k;
        if (out_costs && n >= 2 && (rc = tl_tour_length(c, xy, dm_packed, n, out_pos, &cst))) return rc;
        for (uint32_t r = 0; r < count; ++r) {
            for (uint32_t k = 0; k < n; ++k) out_pos[(size_t)r * n + k] = k;
            if (out_costs) out_costs[r] = cst;
            if (out_moves) out_moves[r] = 0u;
        }
        return TL_OK;
    }
    PopPlan P{};
    if ((rc = plan(P))) return rc;
    if (!P.resident) {
        tl_stats acc{};
        for (uint32_t r = 0; r < count; ++r) {
            float cst = 0.0f;
            tl_stats st1{};
            if ((rc = run1(init_pos + (size_t)r * n, out_pos + (size_t)r * n, &cst, &st1))) return rc;
            if (out_costs) out_costs[r] = cst;
            if (out_moves) out_moves[r] = (uint32_t)st1.moves;
            acc.sweeps += st1.sweeps;
            acc.moves += st1.moves;
            acc.candidates += st1.candidates;
            acc.kernel_ms += st1.kernel_ms;
        }
        if (stats) {
            *stats = acc;
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return TL_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t words = (size_t)count * n;
    if ((rc = ensure(c, c->init, words * 4)) || (rc = ensure(c, c->out_pos, words * 4)) || (rc = ensure(c, c->out_cost, (size_t)count * 4)) ||
        (rc = ensure(c, c->misc, (size_t)count * 16)) || (P.tour_work && (rc = ensure(c, c->work, (size_t)P.batch * P.tour_work))))
        return rc;
    PopArgs A{};
    if ((rc = upload_input(c, xy, dm_packed, n, &A.xy, &A.dm))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->init.p, init_pos, words * 4, hipMemcpyHostToDevice, c->stream));
    A.Dt = P.tour_work ? (float *)c->work.p : nullptr;
    A.n = n;
    A.max_passes = max_passes;
    c->ev_valid = false;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t first = 0; first < count; first += P.batch) {  // a batch's workgroups own the workspace; the stream orders the batches
        const uint32_t cnt = count - first < P.batch ? count - first : P.batch;
        A.init = (const uint32_t *)c->init.p + (size_t)first * n;
        A.out_pos = (uint32_t *)c->out_pos.p + (size_t)first * n;
        A.out_cost = (float *)c->out_cost.p + first;
        A.out_run = (uint32_t *)c->misc.p + 4u * (size_t)first;
        HIPCHK(c, launch(A, cnt, P.threads));
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<uint32_t> run((size_t)count * 4);
    std::vector<float> costs(count);
    HIPCHK(c, hipMemcpyAsync(run.data(), c->misc.p, (size_t)count * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(costs.data(), c->out_cost.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t r = 0; r < count; ++r)
        if (run[4u * r + 2u] != 0u) return fail(c, TL_ERR_NO_CONVERGE, "%s: pass cap reached in tour %u", who, r);
    HIPCHK(c, hipMemcpyAsync(out_pos, c->out_pos.p, words * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t moves = 0, passes = 0;
    for (uint32_t r = 0; r < count; ++r) {
        if (out_costs) out_costs[r] = costs[r];
        if (out_moves) out_moves[r] = run[4u * r];
        moves += run[4u * r];
        passes += run[4u * r + 1u];
    }
    if (stats) {
        stats->moves = moves;
        stats->sweeps = passes;
        stats->candidates = passes * per_pass;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

// ------------------------------------------------------------------------------------------------
// 3-opt
// ------------------------------------------------------------------------------------------------
// (i, j) and (k, case) travel as packed 16-bit fields; the workspace holds an n x (n+1) f32 matrix (17 GB at this limit: sized
// for 288 GB of HBM; k_three_opt_pick stages the move's segments in the workspace where they do not fit the LDS)
static constexpr uint32_t kThreeOptMaxN = 65535u;

// uploads inputs, lays out the workspace in c->work and fills the kernel argument block (A.xy or A.dm: the form); *nblocks: the scan's grid
static int three_opt_setup(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *path, ThreeOptArgs &A, uint32_t *nblocks)
{
    if (n > kThreeOptMaxN)
        return fail(c, TL_ERR_UNSUPPORTED, "three_opt: n=%u exceeds the limit %u of this build (packed 16-bit indices)", n, kThreeOptMaxN);
    int rc;
    const uint32_t jc = n <= 256 ? 4u : 16u;
    std::vector<uint32_t> prefix(n - 1);
    uint32_t acc = 0;
    for (uint32_t i = 0; i + 2 < n; ++i) {
        prefix[i] = acc;
        acc += ((n - 2u - i) + jc - 1u) / jc;  // j in [i+1, n-1)
    }
    prefix[n - 2] = acc;
    *nblocks = acc;
    if ((rc = upload_input(c, xy, dm_packed, n, &A.xy, &A.dm))) return rc;
    // workspace: perm | Pt | E | prefix | partials | best | counters
    const size_t o_perm = 0, o_pt = up256(o_perm + (size_t)n * 4), o_e = up256(o_pt + (size_t)(n + 1) * 8), o_pre = up256(o_e + (size_t)n * 4),
                 o_par = up256(o_pre + (size_t)(n - 1) * 4), o_best = up256(o_par + (size_t)acc * sizeof(ThreeOptBest)),
                 o_cnt = up256(o_best + sizeof(ThreeOptBest)), o_scr = up256(o_cnt + 16), o_dt = up256(o_scr + (size_t)n * 4),
                 total = up256(o_dt + (size_t)n * (n + 1) * 4);
    if ((rc = ensure(c, c->work, total))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    HIPCHK(c, hipMemcpyAsync(w + o_pre, prefix.data(), (size_t)(n - 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + o_cnt, 0, 16, c->stream));
    if ((rc = upload_start_sync(c, path, n, w + o_perm))) return rc;  // (prefix goes out of scope behind it)
    A.perm = (uint32_t *)(w + o_perm);
    A.Pt = (float2 *)(w + o_pt);
    A.E = (float *)(w + o_e);
    A.Dt = (float *)(w + o_dt);
    A.chunk_prefix = (const uint32_t *)(w + o_pre);
    A.partials = (ThreeOptBest *)(w + o_par);
    A.best = (ThreeOptBest *)(w + o_best);
    A.counters = (uint64_t *)(w + o_cnt);
    A.scratch = (uint32_t *)(w + o_scr);
    A.n = n;
    A.jc = jc;
    return TL_OK;
}

extern "C" int tl_three_opt_find_best_move(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *path,
                                           int *found, uint32_t *oi, uint32_t *oj, uint32_t *ok, int *kase, float *savings)
{
    TL_ENTER(c);
    if (!c || (!xy && !dm_packed) || !path || !found) return fail(c, TL_ERR_BADARG, "tl_three_opt_find_best_move: NULL argument");
    *found = 0;
    if (n < 4) return TL_OK;
    if (!is_permutation(path, n)) return fail(c, TL_ERR_BADARG, "tl_three_opt_find_best_move: path is not a permutation of 0..n-1");
    HIPCHK(c, hipSetDevice(c->device));
    ThreeOptArgs A{};
    uint32_t nblocks = 0;
    int rc;
    if ((rc = three_opt_setup(c, xy, n, dm_packed, path, A, &nblocks))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_three_opt_pass(A, nblocks, A.dm != nullptr, 0, c->stream, c->lds_bytes));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    ThreeOptBest b{};
    HIPCHK(c, hipMemcpyAsync(&b, A.best, sizeof(b), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (b.found) {
        *found = 1;
        if (oi) *oi = b.ij >> 16;
        if (oj) *oj = b.ij & 0xFFFFu;
        if (ok) *ok = b.kc >> 3;
        if (kase) *kase = (int)(b.kc & 7u);
        if (savings) *savings = b.sav;
    }
    return TL_OK;
}

static uint64_t three_opt_per_pass(uint32_t n)
{
    const uint64_t nn = n;
    return nn * (nn - 1) * (nn - 2) / 6 - (nn - 2);  // C(n,3) - (n-2) triples per pass
}

// the log's 4 words per move: i, j, k, case of three_opt.rs:36-45
static int three_opt_run(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                         uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    uint32_t nblocks = 0;
    return scan_descent<ThreeOptArgs>(
        c, "three_opt", xy, n, dm_packed, init_pos, out_pos, out_cost, stats, move_log, log_cap, log_len, three_opt_per_pass(n),
        [&](ThreeOptArgs &A) { return three_opt_setup(c, xy, n, dm_packed, init_pos, A, &nblocks); },
        [&](const ThreeOptArgs &A) { return launch_three_opt_pass(A, nblocks, A.dm != nullptr, 1, c->stream, c->lds_bytes); });
}

extern "C" int tl_three_opt(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                            uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return three_opt_run(c, xy, n, dm_packed, init_pos, out_pos, out_cost, stats, nullptr, 0, nullptr);
}

// three_opt::solve with its moves listed: the reference sends the path after every apply_3opt (three_opt.rs:34,42,47-49); the
// pick kernel files every move it applies, the list is read back once.
extern "C" int tl_three_opt_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                                  uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    TL_ENTER(c);
    if (!move_log || !log_len) return fail(c, TL_ERR_BADARG, "tl_three_opt_trace: NULL argument");
    return three_opt_run(c, xy, n, dm_packed, init_pos, out_pos, out_cost, stats, move_log, log_cap, log_len);
}

// ------------------------------------------------------------------------------------------------
// Or-opt (or_opt.rs)
// ------------------------------------------------------------------------------------------------
// (no size limit of its own: a 96-bit argmin key, and a workspace copy of the tour beyond the LDS)
static int or_opt_setup(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *path, OrOptArgs &A)
{
    int rc;
    if ((rc = upload_input(c, xy, dm_packed, n, &A.xy, &A.dm))) return rc;
    const uint32_t nblocks = or_opt_scan_blocks(n);
    const size_t o_perm = 0, o_pt = up256((size_t)n * 4), o_e = up256(o_pt + (size_t)n * 8), o_par = up256(o_e + (size_t)n * 4),
                 o_best = up256(o_par + (size_t)nblocks * 16), o_old = up256(o_best + 256), total = o_old + (size_t)n * 4 + 256;
    if ((rc = ensure(c, c->work, total))) return rc;
    unsigned char *w = (unsigned char *)c->work.p;
    if ((rc = upload_start_sync(c, path, n, w + o_perm))) return rc;
    A.perm = (uint32_t *)(w + o_perm);
    A.Pt = (float2 *)(w + o_pt);
    A.E = (float *)(w + o_e);
    A.partials = (unsigned long long *)(w + o_par);
    A.best = (OrOptBest *)(w + o_best);
    A.scratch = (uint32_t *)(w + o_old);
    A.n = n;
    return TL_OK;
}

extern "C" int tl_or_opt_find_best_move(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *path,
                                        int *found, float *delta, uint32_t *oi, uint32_t *oj, uint32_t *seg_len, int *reversed)
{
    TL_ENTER(c);
    if (!c || (!xy && !dm_packed) || !path || !found) return fail(c, TL_ERR_BADARG, "tl_or_opt_find_best_move: NULL argument");
    *found = 0;
    if (n < 4) return TL_OK;
    if (!is_permutation(path, n)) return fail(c, TL_ERR_BADARG, "tl_or_opt_find_best_move: path is not a permutation of 0..n-1");
    HIPCHK(c, hipSetDevice(c->device));
    OrOptArgs A{};
    int rc;
    if ((rc = or_opt_setup(c, xy, n, dm_packed, path, A))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, launch_or_opt_pass(A, A.dm != nullptr, 0, c->stream, c->lds_bytes));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    OrOptBest b{};
    HIPCHK(c, hipMemcpyAsync(&b, A.best, sizeof(b), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (b.found) {
        *found = 1;
        if (delta) memcpy(delta, &b.delta_bits, 4);
        if (oi) *oi = b.i;
        if (oj) *oj = b.j;
        if (seg_len) *seg_len = b.seg_len;
        if (reversed) *reversed = (int)b.reversed;
    }
    return TL_OK;
}

// deltas evaluated per pass: seg_len 1: n(n-2) forward; seg_len 2: (n-1)(n-3) x 2; seg_len 3: (n-2)(n-4) x 2
static uint64_t or_opt_per_pass(uint32_t n)
{
    const uint64_t nn = n;
    uint64_t per = 0;
    if (nn > 2) per += nn * (nn - 2);
    if (nn > 3) per += 2 * (nn - 1) * (nn - 3);
    if (nn > 4) per += 2 * (nn - 2) * (nn - 4);
    return per;
}

// the log's 4 words per move: i, j, seg_len, reversed of or_opt.rs:45-51
static int or_opt_run(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                      uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    return scan_descent<OrOptArgs>(
        c, "or_opt", xy, n, dm_packed, init_pos, out_pos, out_cost, stats, move_log, log_cap, log_len, or_opt_per_pass(n),
        [&](OrOptArgs &A) { return or_opt_setup(c, xy, n, dm_packed, init_pos, A); },
        [&](const OrOptArgs &A) { return launch_or_opt_pass(A, A.dm != nullptr, 1, c->stream, c->lds_bytes); });
}

extern "C" int tl_or_opt(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                         uint32_t *out_pos, float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return or_opt_run(c, xy, n, dm_packed, init_pos, out_pos, out_cost, stats, nullptr, 0, nullptr);
}

// or_opt::solve with its moves listed: the reference sends the path and its tour_length after every apply_relocation
// (or_opt.rs:40-42,62-67,70-72); the pick kernel files every move it applies.
extern "C" int tl_or_opt_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos,
                               uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *move_log, uint32_t log_cap, uint32_t *log_len)
{
    TL_ENTER(c);
    if (!move_log || !log_len) return fail(c, TL_ERR_BADARG, "tl_or_opt_trace: NULL argument");
    return or_opt_run(c, xy, n, dm_packed, init_pos, out_pos, out_cost, stats, move_log, log_cap, log_len);
}

// ------------------------------------------------------------------------------------------------
// Or-opt over a population of tours (or_opt_lds.hip)
// ------------------------------------------------------------------------------------------------
extern "C" uint32_t tl_or_opt_lds_max_n(const tl_ctx *c) { return c ? or_opt_lds_max_n(c->lds_bytes, false) : 0u; }

// Every tour refined by its own descent, one workgroup per tour with the tour in LDS; tour r's result is tl_or_opt's for it alone.
// Beyond the LDS-resident size, or with TL_FLAG_OR_OPT_FORCE_SCAN, the tours go one after the other through the chip-wide descent.
extern "C" int tl_or_opt_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t count,
                                    uint32_t *out_pos, float *out_costs, uint32_t *out_moves, tl_stats *stats)
{
    TL_ENTER(c);
    const bool dm = dm_packed != nullptr;
    return population_descent(
        c, "or_opt", xy, n, dm_packed, init_pos, count, out_pos, out_costs, out_moves, stats, or_opt_per_pass(n),
        64u * n + 1024u,  // scan_descent's cap as a count of passes.  (tl_three_opt_population rounds it up to scan_descent's next look,
                          // so the two differ; making them alike would change when a descent fails, and is left alone)
        [&](const uint32_t *init, uint32_t *out, float *cost, tl_stats *st) { return or_opt_run(c, xy, n, dm_packed, init, out, cost, st, nullptr, 0, nullptr); },
        [&](PopPlan &P) -> int {
            P.resident = !(c->flags & TL_FLAG_OR_OPT_FORCE_SCAN) && n <= or_opt_lds_max_n(c->lds_bytes, dm);
            if (P.resident) P.threads = or_opt_lds_threads(n, count, c->cus, c->lds_bytes, dm);
            P.batch = count;
            return TL_OK;
        },
        [&](const PopArgs &A, uint32_t cnt, int threads) { return launch_or_opt_lds(A, cnt, threads, c->stream); });
}

// ------------------------------------------------------------------------------------------------
// 3-opt over a population of tours (three_opt_pop.hip)
// ------------------------------------------------------------------------------------------------
// The cost model behind tl_three_opt_population_plan: a pass of one tour is triples(n) = C(n,3) - (n-2) triples, and both forms run
// the same passes, so the forms are compared per pass.
//   form 1: the tours of a batch run one per CU at kPopRcu triples a second each, in ceil(count / cus) rounds;
//   form 0: every tour's pass has the whole chip at kPopRchip triples a second plus kPopTpass of launches, the global reduction
//           and the host's share of a poll every 16 passes.
// Measured on one MI355X (256 CUs), 2026-10-19, scripts/timing_three_opt_population.py; NOTEBOOK.md, "3-opt for a population".
//   kPopRcu    the mean tour's triples over the kernel time of 256 random tours at n = 500 (2.02e9) — a round lasts as long as its
//              longest descent, so that wait is inside the figure.  The rate is not one number: a single tour runs at 2.6e9 at
//              n = 500 and 1.1e9 at n = 100 (barriers and the Dt rebuild weigh more the smaller n); the figure taken is the one
//              near the sizes where the two forms meet, which is where the choice matters.
//   kPopRchip, kPopTpass: least-squares fit of the loop's wall seconds per pass, t = triples / R + T, over n = 52 ... 1 002.
static constexpr double kPopRcu = 2.0e9;     // triples / s on one CU (form 1)
static constexpr double kPopRchip = 6.9e11;  // triples / s of the chip-wide scan (form 0)
static constexpr double kPopTpass = 23e-6;   // s of overhead per chip-wide pass (form 0)
static constexpr uint64_t kPopWorkDefault = 8ull << 30;  // the precedent of the matrix-form lists

extern "C" uint32_t tl_three_opt_pop_max_n(const tl_ctx *c) { return c ? three_opt_pop_max_n(c->lds_bytes) : 0u; }

extern "C" int tl_three_opt_population_plan(uint32_t n, uint32_t count, int cus, int lds_bytes, uint64_t work_bytes, uint32_t flags, int *form,
                                            int *threads, uint32_t *batch)
{
    if (cus < 1 || lds_bytes < 0) return TL_ERR_BADARG;
    const uint64_t dt_bytes = (uint64_t)n * ((uint64_t)n + 1u) * 4u;
    uint64_t b = dt_bytes ? work_bytes / dt_bytes : count;
    if (b > count) b = count;
    int f;
    if (n < 4 || count == 0 || b == 0 || n > three_opt_pop_max_n(lds_bytes) || (flags & TL_FLAG_3OPT_POP_FORCE_SCAN)) {
        f = 0;
    } else if (flags & TL_FLAG_3OPT_POP_FORCE_WG) {
        f = 1;
    } else {
        const double triples = (double)three_opt_per_pass(n);
        const double rounds = (double)((count + (uint32_t)cus - 1u) / (uint32_t)cus);
        const double est_wg = rounds * triples / kPopRcu, est_loop = (double)count * (triples / kPopRchip + kPopTpass);
        f = est_wg <= est_loop ? 1 : 0;
    }
    if (form) *form = f;
    if (threads) *threads = f ? three_opt_pop_threads(n, (uint32_t)b, cus, lds_bytes) : 0;
    if (batch) *batch = (uint32_t)b;
    return TL_OK;
}

extern "C" int tl_three_opt_population_work_limit(tl_ctx *c, uint64_t bytes)
{
    TL_ENTER(c);
    if (!c) return fail(c, TL_ERR_BADARG, "tl_three_opt_population_work_limit: NULL context");
    c->three_opt_pop_work = bytes;
    return TL_OK;
}

// Every tour refined by its own descent; tour r's result is tl_three_opt's for it alone.  Form 1 (tl_three_opt_population_plan): one
// workgroup per tour, batch after batch; form 0: the tours one after the other through the chip-wide descent.
extern "C" int tl_three_opt_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const uint32_t *init_pos, uint32_t count,
                                       uint32_t *out_pos, float *out_costs, uint32_t *out_moves, tl_stats *stats)
{
    TL_ENTER(c);
    return population_descent(
        c, "three_opt", xy, n, dm_packed, init_pos, count, out_pos, out_costs, out_moves, stats, three_opt_per_pass(n),
        // scan_descent's cap as scan_descent applies it: it looks once per kScanBatch passes and gives up when the descent is still moving at
        // the first look beyond 64 n + 1024 passes — so a descent fails here exactly when it fails there.  (tl_or_opt_population passes the
        // plain 64 n + 1024; making the two alike would change when a descent fails, and is left alone.)
        (64u * n + 1024u) / (uint32_t)kScanBatch * (uint32_t)kScanBatch + (uint32_t)kScanBatch,
        [&](const uint32_t *init, uint32_t *out, float *cost, tl_stats *st) { return three_opt_run(c, xy, n, dm_packed, init, out, cost, st, nullptr, 0, nullptr); },
        [&](PopPlan &P) -> int {
            int form = 0;
            const int rc = tl_three_opt_population_plan(n, count, c->cus, c->lds_bytes, c->three_opt_pop_work ? c->three_opt_pop_work : kPopWorkDefault,
                                                        c->flags, &form, &P.threads, &P.batch);
            if (rc) return fail(c, rc, "tl_three_opt_population: no plan for this device");
            P.resident = form != 0;
            P.tour_work = (size_t)n * ((size_t)n + 1u) * 4;  // a tour's Dt
            return TL_OK;
        },
        [&](const PopArgs &A, uint32_t cnt, int threads) { return launch_three_opt_pop(A, cnt, threads, c->stream); });
}
