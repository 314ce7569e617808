// tl_api_som.hip — C ABI, the Kohonen self-organising map solver: tl_kohonen_som* (src/tsp/som.rs:12-186) over kohonen_som.hip, the
// host-only queries of its specification (tl_som_draw, tl_som_schedule, tl_som_h, tl_som_ring_init, tl_kohonen_som_plan,
// tl_kohonen_som_max_n) and the device self-test of the BMU and the extraction.
//
// What does not depend on the run is built once per call on the host, with som_spec.h's text: the normalised cities, the start
// ring and the schedule (eta, two_sigma_sq and the radius of every epoch).  n < 2: the trivial route, without a launch.
#include "som_spec.h"
#include "tl_api_chains.h"

using namespace tl;
using namespace tlapi;

static constexpr uint32_t kSomUnassignedFlags = 1u << 31;  // the one bit no flag of include/teeline_gpu.h has
static constexpr uint64_t kSomWorkDefault = 8ull << 30;    // the runs of one launch sequence
static constexpr uint32_t kSomMaxRuns = 65535u;            // the run is the grid's x
static constexpr uint64_t kSomLayoutSlack = 5 * 256;       // the arrays of a sequence each start on a 256-byte boundary

// one run's share of the workspace: the ring (2 M f64) and the extraction's neuron, distance and edge length of every city
static inline uint64_t som_run_bytes(uint32_t n, uint32_t M) { return 16ull * M + 16ull * n; }

static inline bool som_fits_lds(uint32_t M, int lds_bytes) { return lds_bytes > 0 && kohonen_som_lds_bytes(M, true) <= (size_t)lds_bytes; }

extern "C" uint32_t tl_som_draw(uint64_t seed, uint32_t run, uint32_t epoch, uint32_t n) { return n ? som_city(sa_chain_key(seed, run), epoch, n) : 0u; }

extern "C" int tl_som_schedule(uint32_t epoch, uint32_t epochs, uint32_t neurons, double learning_rate, double radius_fraction, double *eta, double *sigma,
                               double *two_sigma_sq, uint32_t *radius)
{
    if (epochs < 1u || epoch < 1u || epoch > epochs || neurons < 1u || neurons > kSomMaxNeurons) return TL_ERR_BADARG;
    double sg;
    const SomEpoch e = som_schedule(epoch, epochs, neurons, learning_rate, radius_fraction, &sg);
    if (eta) *eta = e.eta;
    if (sigma) *sigma = sg;
    if (two_sigma_sq) *two_sigma_sq = e.two_sigma_sq;
    if (radius) *radius = e.radius;
    return TL_OK;
}

extern "C" int tl_som_h(double d, double two_sigma_sq, double *h)
{
    double v;
    const bool applied = som_h(d, two_sigma_sq, &v);
    if (h) *h = v;
    return applied ? 1 : 0;
}

static bool som_finite(const float *xy, uint32_t n)
{
    for (size_t k = 0; k < 2 * (size_t)n; ++k)
        if (!std::isfinite(xy[k])) return false;
    return true;
}

extern "C" int tl_som_ring_init(const float *xy, uint32_t n, uint32_t neuron_multiplier, double *out_ring, double *out_cities)
{
    if (!xy || !out_ring || n < 1u || neuron_multiplier < 1u || (uint64_t)n * neuron_multiplier > kSomMaxNeurons || !som_finite(xy, n)) return TL_ERR_BADARG;
    const uint32_t M = n * neuron_multiplier;
    std::vector<double> cities(2 * (size_t)n);
    double cx, cy;
    som_normalise(xy, n, cities.data(), cities.data() + n, &cx, &cy);
    for (uint32_t i = 0; i < M; ++i) som_ring_neuron(i, M, cx, cy, out_ring + i, out_ring + M + i);
    if (out_cities) memcpy(out_cities, cities.data(), cities.size() * 8);
    return TL_OK;
}

extern "C" int tl_kohonen_som_plan(uint32_t n, uint32_t neuron_multiplier, uint32_t form, uint32_t count, int cus, int lds_bytes, uint64_t workspace_bytes,
                                   uint32_t flags, uint32_t *neurons, int *threads, uint32_t *form_out, uint32_t *per_launch)
{
    if (neurons) *neurons = 0u;
    if (threads) *threads = 0;
    if (form_out) *form_out = 0u;
    if (per_launch) *per_launch = 0u;
    if (cus < 1 || lds_bytes < 0 || form > 2u) return TL_ERR_BADARG;
    if (flags & kSomUnassignedFlags) return TL_ERR_UNSUPPORTED;
    (void)count;
    const uint64_t M64 = (uint64_t)n * neuron_multiplier;
    if (n < 2u || neuron_multiplier < 1u || M64 > kSomMaxNeurons) return TL_OK;
    const uint32_t M = (uint32_t)M64;
    const bool fits = som_fits_lds(M, lds_bytes);
    if (form == 1u && !fits) return TL_OK;
    uint64_t per = workspace_bytes > kSomLayoutSlack ? (workspace_bytes - kSomLayoutSlack) / som_run_bytes(n, M) : 0u;
    if (per > kSomMaxRuns) per = kSomMaxRuns;
    if (per == 0u) return TL_OK;
    if (neurons) *neurons = M;
    if (threads) *threads = kohonen_som_threads(M);  // about eight neurons a lane, in whole waves (kohonen_som.hip)
    if (form_out) *form_out = form ? form : (fits ? 1u : 2u);
    if (per_launch) *per_launch = (uint32_t)per;
    return TL_OK;
}

extern "C" uint32_t tl_kohonen_som_max_n(const tl_ctx *c, uint32_t neuron_multiplier, uint32_t form)
{
    if (!c || neuron_multiplier < 1u || form > 2u) return 0u;
    uint64_t m = kSomMaxNeurons;
    if (form == 1u) {
        const uint64_t lds = c->lds_bytes > (int)kSomLdsFixedBytes ? ((uint64_t)c->lds_bytes - kSomLdsFixedBytes) / 16u : 0u;
        if (lds < m) m = lds;
    }
    return (uint32_t)(m / neuron_multiplier);
}

namespace {
struct SomTrace {
    uint32_t *log;
    uint32_t log_cap;
    double *out_ring;
    uint32_t *cp_epochs, *cp_tours, *cp_cost_bits;
    uint32_t cp_cap;
    uint32_t *cp_len;
};
}  // namespace

static int som_run(tl_ctx *c, const char *who, const float *xy, uint32_t n, const float *dm_packed, uint32_t first_run, uint32_t count, const tl_som_opts *opts,
                   uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *best_index, tl_stats *stats, const SomTrace *tr)
{
    if (tr && tr->cp_len) *tr->cp_len = 0;
    if (!c) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (!xy) return fail(c, TL_ERR_BADARG, "%s: xy is NULL — the map trains on the coordinates; a matrix only prices the tour", who);
    if (count == 0) return TL_OK;
    if (!out_pos) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if ((uint64_t)first_run + count > 0x100000000ull) return fail(c, TL_ERR_BADARG, "%s: run ids beyond 2^32 - 1", who);
    if (c->flags & kSomUnassignedFlags) return fail(c, TL_ERR_UNSUPPORTED, "%s: the context's flags 0x%x hold a bit no flag has", who, c->flags);
    // SOMOptions::default (mod.rs:1473-1482) and ::validate (mod.rs:1485-1499)
    const uint32_t epochs = opts ? opts->epochs : 100000u, mult = opts ? opts->neuron_multiplier : 8u, form = opts ? opts->form : 0u;
    const double eta0 = opts ? opts->learning_rate : 0.8, rf = opts ? opts->radius_fraction : 0.1;
    if (epochs < 1u) return fail(c, TL_ERR_BADARG, "%s: epochs must be >= 1", who);
    if (!(eta0 > 0.0 && eta0 <= 1.0)) return fail(c, TL_ERR_BADARG, "%s: learning_rate must be in (0, 1]", who);
    if (!(rf > 0.0 && rf <= 1.0)) return fail(c, TL_ERR_BADARG, "%s: radius_fraction must be in (0, 1]", who);
    if (mult < 1u) return fail(c, TL_ERR_BADARG, "%s: neuron_multiplier must be >= 1", who);
    if (form > 2u || (opts && opts->reserved)) return fail(c, TL_ERR_BADARG, "%s: form is 0 (the plan decides), 1 (LDS) or 2 (workspace); reserved is 0", who);
    if (epochs == 0xFFFFFFFFu) return fail(c, TL_ERR_UNSUPPORTED, "%s: epochs = 2^32 - 1 is not supported", who);
    if ((uint64_t)n * mult > kSomMaxNeurons)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u x neuron_multiplier=%u: more than %u neurons", who, n, mult, kSomMaxNeurons);
    if (!som_finite(xy, n)) return fail(c, TL_ERR_BADARG, "%s: a coordinate is not finite", who);
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (best_index) *best_index = 0u;
    const uint32_t cp = som_checkpoint(epochs);
    const uint32_t cp_records = epochs / cp + (epochs % cp ? 1u : 0u);
    if (n < 2u) {  // som.rs:21-24: the trivial route, nothing trained, no message but what the caller adds
        for (uint32_t r = 0; r < count; ++r) {
            if (n) out_pos[r] = 0u;
            if (out_costs) out_costs[r] = 0.0f;
        }
        c->ev_valid = false;
        stamp_times(c, stats, t0);
        return TL_OK;
    }
    const uint32_t M = n * mult;
    uint32_t per_launch = 0, use_form = 0;
    const uint64_t work = opts && opts->work_bytes ? opts->work_bytes : kSomWorkDefault;
    tl_kohonen_som_plan(n, mult, form, count, c->cus, c->lds_bytes, work, 0u, nullptr, nullptr, &use_form, &per_launch);
    if (form == 1u && !som_fits_lds(M, c->lds_bytes))
        return fail(c, TL_ERR_UNSUPPORTED, "%s: %u neurons do not fit the LDS form (%zu bytes of %d)", who, M, kohonen_som_lds_bytes(M, true), c->lds_bytes);
    if (per_launch == 0u)
        return fail(c, TL_ERR_UNSUPPORTED, "%s: n=%u, %u neurons: one run's block (%llu bytes) exceeds the workspace limit", who, n, M,
                    (unsigned long long)som_run_bytes(n, M));
    const bool lds_form = use_form == 1u;

    // what every run shares
    std::vector<double> cities, ring0;
    std::vector<SomEpoch> sched;
    try {
        cities.resize(2 * (size_t)n);
        ring0.resize(2 * (size_t)M);
        sched.resize(epochs);
    } catch (const std::bad_alloc &) {
        return fail(c, TL_ERR_NOMEM, "%s: no host memory for the schedule of %u epochs", who, epochs);
    }
    double cx, cy;
    som_normalise(xy, n, cities.data(), cities.data() + n, &cx, &cy);
    for (uint32_t i = 0; i < M; ++i) som_ring_neuron(i, M, cx, cy, ring0.data() + i, ring0.data() + M + i);
    for (uint32_t t = 1; t <= epochs; ++t) sched[t - 1u] = som_schedule(t, epochs, M, eta0, rf, nullptr);

    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const uint32_t held = count < per_launch ? count : per_launch;
    const bool traced = tr != nullptr;
    const uint32_t dev_log_cap = traced && tr->log ? (tr->log_cap < epochs ? tr->log_cap : epochs) : 0u;
    const uint32_t dev_cp = traced && tr->cp_tours ? (tr->cp_cap < cp_records ? tr->cp_cap : cp_records) : 0u;
    const size_t b_cities = up256(cities.size() * 8), b_ring0 = up256(ring0.size() * 8), b_sched = up256(sched.size() * sizeof(SomEpoch)),
                 b_log = up256((size_t)(dev_log_cap ? dev_log_cap : 1u) * 8), b_cpt = up256((size_t)(dev_cp ? dev_cp : 1u) * n * 4),
                 b_cpc = up256((size_t)(dev_cp ? dev_cp : 1u) * 4);
    const size_t b_ring = up256((size_t)held * M * 16), b_bd = up256((size_t)held * n * 8), b_bmu = up256((size_t)held * n * 4), b_edge = b_bmu;
    if ((rc = ensure(c, c->out_pos, (size_t)count * n * 4)) || (rc = ensure(c, c->out_cost, (size_t)count * 4)) ||
        (rc = ensure(c, c->work, b_cities + b_ring0 + b_sched + b_log + b_cpt + b_cpc + b_ring + b_bd + b_bmu + b_edge)))
        return rc;
    SomArgs A{};
    {  // the cost is priced by the matrix where one is given, else by the f32 coordinates
        const float2 *dxy = nullptr;
        const float *dfull = nullptr;
        if ((rc = upload_instance_full(c, xy, dm_packed, n, &dxy, &dfull))) return rc;
        A.xy = dxy;
        A.dm_full = dfull;
    }
    unsigned char *w = (unsigned char *)c->work.p;
    HIPCHK(c, hipMemcpyAsync(w, cities.data(), cities.size() * 8, hipMemcpyHostToDevice, c->stream));
    A.cities = (const double *)w;
    w += b_cities;
    HIPCHK(c, hipMemcpyAsync(w, ring0.data(), ring0.size() * 8, hipMemcpyHostToDevice, c->stream));
    A.ring0 = (const double *)w;
    w += b_ring0;
    HIPCHK(c, hipMemcpyAsync(w, sched.data(), sched.size() * sizeof(SomEpoch), hipMemcpyHostToDevice, c->stream));
    A.sched = (const SomEpoch *)w;
    w += b_sched;
    uint32_t *d_log = (uint32_t *)w;
    w += b_log;
    uint32_t *d_cpt = (uint32_t *)w;
    w += b_cpt;
    float *d_cpc = (float *)w;
    w += b_cpc;
    A.ring = (double *)w;
    w += b_ring;
    A.bdist = (double *)w;
    w += b_bd;
    A.bmu = (uint32_t *)w;
    w += b_bmu;
    A.edge = (float *)w;
    A.log = dev_log_cap ? d_log : nullptr;
    A.log_cap = dev_log_cap;
    A.seed = seed;
    A.n = n;
    A.M = M;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint32_t b0 = 0; b0 < count; b0 += per_launch) {  // sequences on one stream follow each other: the next takes over the blocks
        const uint32_t cnt = count - b0 < per_launch ? count - b0 : per_launch;
        SomArgs L = A;
        L.first_run = first_run + b0;
        uint32_t *res_pos = (uint32_t *)c->out_pos.p + (size_t)b0 * n;
        float *res_cost = (float *)c->out_cost.p + b0;
        // a plain call is one span; a traced call is one span per checkpoint, the extraction behind each (som.rs:117-131)
        uint32_t k = 0;
        for (uint32_t t = 1; t <= epochs;) {
            const uint64_t end = traced ? ((uint64_t)(t - 1u) / cp + 1u) * cp : epochs;  // the last epoch of the span
            L.t0 = t;
            L.t1 = (uint32_t)(end < epochs ? end : epochs) + 1u;
            L.fresh = t == 1u;
            HIPCHK(c, launch_som_train(L, cnt, lds_form, c->stream));
            if (traced && end <= epochs && k < dev_cp) {
                L.out_pos = d_cpt + (size_t)k * n;
                L.out_cost = d_cpc + k;
                HIPCHK(c, launch_som_extract(L, cnt, c->stream));
                ++k;
            }
            t = L.t1;
        }
        L.out_pos = res_pos;
        L.out_cost = res_cost;
        HIPCHK(c, launch_som_extract(L, cnt, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    std::vector<float> costs(count);
    HIPCHK(c, hipMemcpyAsync(costs.data(), c->out_cost.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_pos, c->out_pos.p, (size_t)count * n * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<float> cp_costs(dev_cp ? dev_cp : 1u);
    if (traced) {
        if (dev_log_cap) HIPCHK(c, hipMemcpyAsync(tr->log, d_log, (size_t)dev_log_cap * 8, hipMemcpyDeviceToHost, c->stream));
        if (tr->out_ring) HIPCHK(c, hipMemcpyAsync(tr->out_ring, A.ring, (size_t)M * 16, hipMemcpyDeviceToHost, c->stream));
        if (dev_cp) {
            HIPCHK(c, hipMemcpyAsync(tr->cp_tours, d_cpt, (size_t)dev_cp * n * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(cp_costs.data(), d_cpc, (size_t)dev_cp * 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t r = 0; r < count; ++r)
        if (out_costs) out_costs[r] = costs[r];
    if (traced) {
        const uint32_t at_cp = epochs / cp;  // records that are checkpoints; one more where epochs % cp != 0: the final PathUpdate
        for (uint32_t k = 0; k < dev_cp; ++k) {
            if (k < at_cp) {
                if (tr->cp_epochs) tr->cp_epochs[k] = (k + 1u) * cp;
                if (tr->cp_cost_bits) tr->cp_cost_bits[k] = __builtin_bit_cast(uint32_t, cp_costs[k]);
            } else {  // the result itself
                if (tr->cp_epochs) tr->cp_epochs[k] = 0xFFFFFFFFu;
                if (tr->cp_cost_bits) tr->cp_cost_bits[k] = __builtin_bit_cast(uint32_t, costs[0]);
                memcpy(tr->cp_tours + (size_t)k * n, out_pos, (size_t)n * 4);
            }
        }
        if (tr->cp_len) *tr->cp_len = cp_records;
    }
    if (best_index) *best_index = best_chain(costs, count);
    if (stats) {
        stats->sweeps = (uint64_t)epochs * count;
        stats->candidates = (uint64_t)epochs * count * M;
        stamp_times(c, stats, t0);
    }
    return TL_OK;
}

extern "C" int tl_kohonen_som(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const tl_som_opts *opts, uint64_t seed, uint32_t *out_pos,
                              float *out_cost, tl_stats *stats)
{
    TL_ENTER(c);
    return som_run(c, "tl_kohonen_som", xy, n, dm_packed, 0u, 1u, opts, seed, out_pos, out_cost, nullptr, stats, nullptr);
}

extern "C" int tl_kohonen_som_trace(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, const tl_som_opts *opts, uint64_t seed, uint32_t run,
                                    uint32_t *out_pos, float *out_cost, tl_stats *stats, uint32_t *log, uint32_t log_cap, double *out_ring, uint32_t *cp_epochs,
                                    uint32_t *cp_tours, uint32_t *cp_cost_bits, uint32_t cp_cap, uint32_t *cp_len)
{
    TL_ENTER(c);
    if (!cp_len) return fail(c, TL_ERR_BADARG, "tl_kohonen_som_trace: NULL argument");
    const SomTrace tr{log, log_cap, out_ring, cp_epochs, cp_tours, cp_cost_bits, cp_tours ? cp_cap : 0u, cp_len};
    return som_run(c, "tl_kohonen_som_trace", xy, n, dm_packed, run, 1u, opts, seed, out_pos, out_cost, nullptr, stats, &tr);
}

extern "C" int tl_kohonen_som_population(tl_ctx *c, const float *xy, uint32_t n, const float *dm_packed, uint32_t first_run, uint32_t count,
                                         const tl_som_opts *opts, uint64_t seed, uint32_t *out_pos, float *out_costs, uint32_t *best_index, tl_stats *stats)
{
    TL_ENTER(c);
    return som_run(c, "tl_kohonen_som_population", xy, n, dm_packed, first_run, count, opts, seed, out_pos, out_costs, best_index, stats, nullptr);
}

extern "C" int tl_som_selftest_bmu(tl_ctx *c, const double *ring, uint32_t neurons, const double *cities, uint32_t n, int threads, uint32_t form,
                                   uint32_t *out_bmu, uint32_t *out_extract_bmu, uint32_t *out_tour)
{
    TL_ENTER(c);
    if (!c || !ring || !cities || !out_bmu) return fail(c, TL_ERR_BADARG, "tl_som_selftest_bmu: NULL argument");
    if (neurons < 1u || neurons > kSomMaxNeurons || n < 2u || n > kSomMaxNeurons || form > 2u)
        return fail(c, TL_ERR_BADARG, "tl_som_selftest_bmu: neurons, n or form out of range");
    if (threads == 0) threads = kohonen_som_threads(neurons);
    if (threads < 64 || threads > 1024 || threads % 64) return fail(c, TL_ERR_BADARG, "tl_som_selftest_bmu: threads is a multiple of 64 in 64 .. 1024");
    const bool fits = som_fits_lds(neurons, c->lds_bytes);
    if (form == 1u && !fits) return fail(c, TL_ERR_UNSUPPORTED, "tl_som_selftest_bmu: %u neurons do not fit the LDS form", neurons);
    const bool lds_form = form == 1u || (form == 0u && fits);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const uint32_t M = neurons;
    const size_t b_cities = up256((size_t)n * 16), b_ring = up256((size_t)M * 16), b_bd = up256((size_t)n * 8), b4 = up256((size_t)n * 4);
    if ((rc = ensure(c, c->work, b_cities + b_ring + b_bd + 4 * b4 + 256)) || (rc = ensure(c, c->xy, (size_t)n * 8))) return rc;
    c->ev_valid = false;
    unsigned char *w = (unsigned char *)c->work.p;
    SomArgs A{};
    A.cities = (const double *)w;
    A.ring = (double *)(w + b_cities);
    A.bdist = (double *)(w + b_cities + b_ring);
    uint32_t *d_train = (uint32_t *)(w + b_cities + b_ring + b_bd);
    uint32_t *d_ext = d_train + b4 / 4;
    A.edge = (float *)(d_ext + b4 / 4);
    A.out_pos = (uint32_t *)(d_ext + 2 * (b4 / 4));
    A.out_cost = (float *)(d_ext + 3 * (b4 / 4));  // (the cost of the planted tour is of no interest: priced on zeroed coordinates)
    A.xy = (const float2 *)c->xy.p;
    A.n = n;
    A.M = M;
    HIPCHK(c, hipMemsetAsync(c->xy.p, 0, (size_t)n * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync((void *)A.cities, cities, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(A.ring, ring, (size_t)M * 16, hipMemcpyHostToDevice, c->stream));
    A.bmu = d_train;
    HIPCHK(c, launch_som_selftest_bmu(A, threads, lds_form, c->stream));
    A.bmu = d_ext;
    HIPCHK(c, launch_som_extract(A, 1u, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_bmu, d_train, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_extract_bmu) HIPCHK(c, hipMemcpyAsync(out_extract_bmu, d_ext, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_tour) HIPCHK(c, hipMemcpyAsync(out_tour, A.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TL_OK;
}
