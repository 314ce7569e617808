// tl_api_fourier.hip — C ABI, the Fourier-curve solver: tl_fourier_curve* (src/tsp/fourier.rs:10-312) over fourier_curve.hip, the
// host-only queries of its specification (tl_fourier_basis, tl_fourier_init, tl_fourier_nearest, tl_fourier_curve_plan,
// tl_fourier_curve_work_bytes) and the device self-test of the search.
//
// The solver draws nothing, so the grid dimension is a list of option sets on one problem.  What does not depend on the device is
// built once per call on the host with fourier_spec.h's text: every job's start coefficients.  n < 2: the trivial route, no launch.
#include "fourier_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kFourierUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static constexpr uint32_t kFourierMaxJobs = 65535u;            // the job is the grid's x
static constexpr uint32_t kFourierDefaultChunk = 64u;
static constexpr uint32_t kFourierDefaultSpan = 1u << 16;      // steps of one launch

// FourierOptions::validate (mod.rs:1341-1384); nullptr: valid
static const char *fourier_invalid(const tl_fourier_opts &o)
{
    if (o.k_max < 1u) return "k_max must be >= 1";
    if (o.m < 2u) return "m must be >= 2";
    if (!(o.lambda > 0.0)) return "lambda must be > 0";
    if (!(o.lambda_decay > 0.0 && o.lambda_decay < 1.0)) return "lambda_decay must be in (0, 1)";
    if (!(o.lr > 0.0)) return "lr must be > 0";
    if (o.epochs < 1u) return "epochs must be >= 1";
    return nullptr;
}

static const tl_fourier_opts kFourierDefaults{4u, 200u, 400u, 0u, 0.05, 0.5, 0.05, 0u, 0u};  // mod.rs:1341-1352

namespace {
struct FourierPlan {
    uint32_t max_l, max_m, chunk, span;
    int threads;
    bool lds_form;
    uint64_t sum_c, sum_m;  // doubles of all coefficients, samples of all jobs
};
struct FourierLayout {
    size_t jobs, cities, coeffs, basis, g32, sidx, edge, log, stage, total;
};
}  // namespace

// 0 or an error code with *why set.  The launch parameters (chunk, span_steps, threads) are those of opts[0]
static int fourier_plan(const tl_fourier_opts *opts, uint32_t J, uint32_t n, int lds_bytes, FourierPlan *P, const char **why)
{
    P->max_l = P->max_m = 0u;
    P->sum_c = P->sum_m = 0u;
    for (uint32_t j = 0; j < J; ++j) {
        const tl_fourier_opts &o = opts[j];
        if ((*why = fourier_invalid(o))) return TL_ERR_BADARG;
        if (o.chunk != opts[0].chunk || o.span_steps != opts[0].span_steps || o.threads != opts[0].threads) {
            *why = "chunk, span_steps and threads are launch parameters: the same for every job of a batch";
            return TL_ERR_BADARG;
        }
        if (o.k_max > kFourierMaxK) {
            *why = "k_max above 32";
            return TL_ERR_UNSUPPORTED;
        }
        if (o.m > kFourierMaxM) {
            *why = "m above 4096";
            return TL_ERR_UNSUPPORTED;
        }
        if ((uint64_t)o.k_max * o.epochs >= 0x100000000ull) {
            *why = "k_max x epochs reaches 2^32 steps";
            return TL_ERR_UNSUPPORTED;
        }
        const uint32_t L = 2u * o.k_max + 1u;
        if (L > P->max_l) P->max_l = L;
        if (o.m > P->max_m) P->max_m = o.m;
        P->sum_c += 2u * L;
        P->sum_m += o.m;
    }
    if (n > kFourierMaxN) {
        *why = "n above 65536";
        return TL_ERR_UNSUPPORTED;
    }
    const uint32_t t = opts[0].threads;
    if (t && (t < 64u || t > 1024u || t % 64u || t < 2u * P->max_l)) {
        *why = "threads is 0 (the plan's) or a multiple of 64 in 64 .. 1024 that is at least 2 (2 k_max + 1)";
        return TL_ERR_BADARG;
    }
    P->threads = t ? (int)t : fourier_curve_threads(n, P->max_m);
    P->span = opts[0].span_steps ? opts[0].span_steps : kFourierDefaultSpan;
    uint32_t chunk = opts[0].chunk ? opts[0].chunk : kFourierDefaultChunk;
    if (chunk > n) chunk = n ? n : 1u;
    const size_t lds = lds_bytes > 0 ? (size_t)lds_bytes : 0u;
    P->lds_form = fourier_curve_lds_bytes(n, P->max_l, P->max_m, chunk, true) <= lds;
    while (!P->lds_form && chunk > 1u && fourier_curve_lds_bytes(n, P->max_l, P->max_m, chunk, false) > lds) chunk = (chunk + 1u) / 2u;
    if (!P->lds_form && fourier_curve_lds_bytes(n, P->max_l, P->max_m, chunk, false) > lds) {
        *why = "the curve does not fit the LDS";
        return TL_ERR_UNSUPPORTED;
    }
    P->chunk = chunk;
    return TL_OK;
}

static FourierLayout fourier_layout(const FourierPlan &P, uint32_t J, uint32_t n, uint32_t log_cap, uint32_t stage_rows)
{
    FourierLayout W;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += up256(bytes ? bytes : 1u);
        return here;
    };
    W.jobs = take((size_t)J * sizeof(FourierJob));
    W.cities = take((size_t)n * 8);
    W.coeffs = take((size_t)P.sum_c * 8);
    W.basis = take((size_t)P.sum_m * 16);
    W.g32 = take((size_t)P.sum_m * 8);
    W.sidx = take((size_t)J * n * 4);
    W.edge = take((size_t)J * n * 4);
    W.log = take((size_t)log_cap * n * 4);
    W.stage = take((size_t)stage_rows * 2u * P.max_l * 8);
    W.total = at;
    return W;
}

extern "C" int tl_fourier_basis(uint32_t m, double *out)
{
    if (!out || m < 2u || m > kFourierMaxM) return TL_ERR_BADARG;
    for (uint32_t r = 0; r < m; ++r) {
        const FourierCx e = fourier_basis(r, m);
        out[2u * r] = e.re;
        out[2u * r + 1u] = e.im;
    }
    return TL_OK;
}

static bool fourier_finite(const float *xy, uint32_t n)
{
    for (size_t k = 0; k < 2 * (size_t)n; ++k)
        if (!std::isfinite(xy[k])) return false;
    return true;
}

extern "C" int tl_fourier_init(const float *xy, uint32_t n, uint32_t k_max, double *out_coeffs)
{
    if (!xy || !out_coeffs || n < 1u || n > kFourierMaxN || k_max < 1u || k_max > kFourierMaxK || !fourier_finite(xy, n)) return TL_ERR_BADARG;
    fourier_init(xy, n, k_max, out_coeffs);
    return TL_OK;
}

extern "C" int tl_fourier_nearest(const double *gamma, uint32_t m, const float *xy, uint32_t n, uint32_t *out_idx)
{
    if (!gamma || !xy || !out_idx || m < 1u || m > kFourierMaxM) return TL_ERR_BADARG;
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t best = ~0ull;
        for (uint32_t j = 0; j < m; ++j) {
            const uint64_t k = fourier_pair_key((float)gamma[2u * j], (float)gamma[2u * j + 1u], xy[2u * c], xy[2u * c + 1u], j);
            if (k < best) best = k;
        }
        out_idx[c] = (uint32_t)best;
    }
    return TL_OK;
}

extern "C" int tl_fourier_curve_plan(uint32_t n, const tl_fourier_opts *opts, uint32_t jobs, int lds_bytes, int *threads, uint32_t *form, uint32_t *chunk,
                                     uint32_t *span_steps)
{
    if (threads) *threads = 0;
    if (form) *form = 0u;
    if (chunk) *chunk = 0u;
    if (span_steps) *span_steps = 0u;
    if (lds_bytes < 0 || jobs > kFourierMaxJobs || (jobs && !opts)) return TL_ERR_BADARG;
    if (n < 2u || jobs == 0u) return TL_OK;
    FourierPlan P;
    const char *why = nullptr;
    const int rc = fourier_plan(opts, jobs, n, lds_bytes, &P, &why);
    if (rc) return rc;
    if (threads) *threads = P.threads;
    if (form) *form = P.lds_form ? 1u : 2u;
    if (chunk) *chunk = P.chunk;
    if (span_steps) *span_steps = P.span;
    return TL_OK;
}

extern "C" uint64_t tl_fourier_curve_work_bytes(uint32_t n, const tl_fourier_opts *opts, uint32_t jobs, uint32_t log_cap)
{
    if (n < 2u || jobs == 0u || jobs > kFourierMaxJobs) return 0u;
    const tl_fourier_opts *o = opts ? opts : &kFourierDefaults;
    if (!opts && jobs != 1u) return 0u;
    FourierPlan P;
    const char *why = nullptr;
    if (fourier_plan(o, jobs, n, 1 << 30, &P, &why)) return 0u;
    return fourier_layout(P, jobs, n, log_cap, log_cap ? o[0].k_max : 0u).total;
}

static int fourier_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, const tl_fourier_opts *opts, uint32_t J, uint32_t *out_pos,
                       float *out_costs, double *out_coeffs, uint32_t coeff_stride, uint32_t *best_index, tl_stats *stats, uint32_t *log, uint32_t log_cap,
                       double *stage_coeffs)
{
    if (!c) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (!xy) return fail(c, TL_ERR_BADARG, "%s: xy is NULL — the curve descends on the coordinates; a matrix only prices the tour", who);
    if (J == 0u) return TL_OK;
    if (!opts || !out_pos) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (J > kFourierMaxJobs) return fail(c, TL_ERR_UNSUPPORTED, "%s: more than %u jobs", who, kFourierMaxJobs);
    if (c->flags & kFourierUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    FourierPlan P;
    const char *why = nullptr;
    int rc = fourier_plan(opts, J, n, c->lds_bytes, &P, &why);
    if (rc) return fail(c, rc, "%s: %s", who, why);
    if (out_coeffs && coeff_stride < 2u * P.max_l)
        return fail(c, TL_ERR_BADARG, "%s: coeff_stride %u is below 2 (2 k_max + 1) = %u doubles", who, coeff_stride, 2u * P.max_l);
    if (!fourier_finite(xy, n)) return fail(c, TL_ERR_BADARG, "%s: a coordinate is not finite", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    if (out_coeffs) memset(out_coeffs, 0, (size_t)J * coeff_stride * 8);
    if (n < 2u) {  // fourier.rs:18-21: the trivial tour, no curve
        for (uint32_t j = 0; j < J; ++j) {
            if (n) out_pos[j] = 0u;
            if (out_costs) out_costs[j] = 0.0f;
        }
        c->ev_valid = false;
        stamp_times(c, stats, t0);
        return TL_OK;
    }
    std::vector<FourierJob> jobs(J);
    std::vector<double> coeffs(P.sum_c);
    uint32_t max_total = 0;
    uint64_t steps_sum = 0, pairs_sum = 0;
    {
        uint32_t off_c = 0, off_m = 0;
        for (uint32_t j = 0; j < J; ++j) {
            const tl_fourier_opts &o = opts[j];
            FourierJob &q = jobs[j];
            q.lambda = o.lambda;
            q.lambda_decay = o.lambda_decay;
            q.lr_over_n = o.lr / (double)n;
            q.k_max = o.k_max;
            q.m = o.m;
            q.epochs = o.epochs;
            q.total = o.k_max * o.epochs;
            q.off_c = off_c;
            q.off_m = off_m;
            fourier_init(xy, n, o.k_max, coeffs.data() + off_c);
            off_c += 2u * (2u * o.k_max + 1u);
            off_m += o.m;
            if (q.total > max_total) max_total = q.total;
            steps_sum += q.total;
            pairs_sum += (uint64_t)q.total * o.m;
        }
    }
    const uint32_t dev_log = log ? (log_cap < jobs[0].total ? log_cap : jobs[0].total) : 0u;
    const uint32_t stage_rows = stage_coeffs ? jobs[0].k_max : 0u;
    const FourierLayout W = fourier_layout(P, J, n, dev_log, stage_rows);

    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->out_pos, (size_t)J * n * 4)) || (rc = ensure(c, c->out_cost, (size_t)J * 4)) || (rc = ensure(c, c->work, W.total))) return rc;
    FourierArgs A{};
    {  // the cost is priced by the matrix where one is given, else by the f32 coordinates
        const float2 *dxy = nullptr;
        const float *dfull = nullptr;
        if ((rc = upload_instance_full(c, xy, dm_packed, n, &dxy, &dfull))) return rc;
        A.xy = dxy;
        A.dm_full = dfull;
    }
    unsigned char *w = (unsigned char *)c->work.p;
    HIPCHK(c, hipMemcpyAsync(w + W.jobs, jobs.data(), (size_t)J * sizeof(FourierJob), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + W.cities, xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + W.coeffs, coeffs.data(), coeffs.size() * 8, hipMemcpyHostToDevice, c->stream));
    A.jobs = (const FourierJob *)(w + W.jobs);
    A.cities = (const float2 *)(w + W.cities);
    A.coeffs = (double *)(w + W.coeffs);
    A.basis = (double *)(w + W.basis);
    A.g32 = (float2 *)(w + W.g32);
    A.sidx = (uint32_t *)(w + W.sidx);
    A.edge = (float *)(w + W.edge);
    A.log = dev_log ? (uint32_t *)(w + W.log) : nullptr;
    A.stage_c = stage_rows ? (double *)(w + W.stage) : nullptr;
    A.log_cap = dev_log;
    A.n = n;
    A.chunk = P.chunk;
    A.max_l = P.max_l;
    A.max_m = P.max_m;
    A.out_pos = (uint32_t *)c->out_pos.p;
    A.out_cost = (float *)c->out_cost.p;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint64_t s = 0; s < max_total; s += P.span) {  // a span carries its state in the workspace: the coefficients
        A.s0 = (uint32_t)s;
        A.s1 = (uint32_t)(s + P.span < max_total ? s + P.span : max_total);
        HIPCHK(c, launch_fourier_steps(A, J, P.threads, P.lds_form, c->stream));
    }
    HIPCHK(c, launch_fourier_decode(A, J, c->stream));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<float> costs(J);
    HIPCHK(c, hipMemcpyAsync(costs.data(), c->out_cost.p, (size_t)J * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_pos, c->out_pos.p, (size_t)J * n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_coeffs) HIPCHK(c, hipMemcpyAsync(coeffs.data(), A.coeffs, coeffs.size() * 8, hipMemcpyDeviceToHost, c->stream));
    if (dev_log) HIPCHK(c, hipMemcpyAsync(log, A.log, (size_t)dev_log * n * 4, hipMemcpyDeviceToHost, c->stream));
    if (stage_rows) HIPCHK(c, hipMemcpyAsync(stage_coeffs, A.stage_c, (size_t)stage_rows * 2u * (2u * jobs[0].k_max + 1u) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < J; ++j) {
        if (out_costs) out_costs[j] = costs[j];
        if (out_coeffs) memcpy(out_coeffs + (size_t)j * coeff_stride, coeffs.data() + jobs[j].off_c, (size_t)2u * (2u * jobs[j].k_max + 1u) * 8);
    }
    if (best_index) *best_index = best_chain(costs, J);
    if (stats) {
        stats->sweeps = steps_sum;
        stats->candidates = pairs_sum * n;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_fourier_curve(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const tl_fourier_opts *opts, uint32_t *out_pos, float *out_cost,
                                double *out_coeffs, tl_stats *stats)
{
    TL_ENTER(c);
    const tl_fourier_opts *o = opts ? opts : &kFourierDefaults;
    return fourier_run(c, "tl_fourier_curve", xy, n, dm_packed, o, 1u, out_pos, out_cost, out_coeffs, 2u * (2u * o->k_max + 1u), nullptr, stats, nullptr, 0u,
                       nullptr);
}

extern "C" int tl_fourier_curve_batch(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const tl_fourier_opts *opts, uint32_t jobs, uint32_t *out_pos,
                                      float *out_costs, double *out_coeffs, uint32_t coeff_stride, uint32_t *best_index, tl_stats *stats, uint32_t *log,
                                      uint32_t log_cap, double *stage_coeffs)
{
    TL_ENTER(c);
    return fourier_run(c, "tl_fourier_curve_batch", xy, n, dm_packed, opts, jobs, out_pos, out_costs, out_coeffs, coeff_stride, best_index, stats, log, log_cap,
                       stage_coeffs);
}

extern "C" int tl_fourier_selftest_search(tl_ctx *c, const double *gamma, uint32_t m, const float *xy, uint32_t n, int threads, uint32_t *out_idx)
{
    TL_ENTER(c);
    if (!c || !gamma || !xy || !out_idx) return fail(c, TL_ERR_BADARG, "tl_fourier_selftest_search: NULL argument");
    if (m < 1u || m > kFourierMaxM || n < 1u || n > 8192u) return fail(c, TL_ERR_BADARG, "tl_fourier_selftest_search: m is 1 .. 4096, n 1 .. 8192");
    if (threads == 0) threads = fourier_curve_threads(n, m);
    if (threads < 64 || threads > 1024 || threads % 64) return fail(c, TL_ERR_BADARG, "tl_fourier_selftest_search: threads is a multiple of 64 in 64 .. 1024");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t b_g = up256((size_t)m * 16), b_c = up256((size_t)n * 8), b_s = up256((size_t)n * 4);
    if ((rc = ensure(c, c->work, b_g + b_c + b_s))) return rc;
    c->ev_valid = false;
    unsigned char *w = (unsigned char *)c->work.p;
    FourierArgs A{};
    A.gamma_in = (const double *)w;
    A.cities = (const float2 *)(w + b_g);
    A.sidx = (uint32_t *)(w + b_g + b_c);
    A.n = n;
    A.max_m = m;
    HIPCHK(c, hipMemcpyAsync(w, gamma, (size_t)m * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w + b_g, xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_fourier_selftest_search(A, threads, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_idx, A.sidx, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}
