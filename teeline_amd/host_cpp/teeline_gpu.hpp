// teeline_gpu.hpp — C++ host-side mirror of the reference's solver interface for the 2-opt / 3-opt / LK path,
// over the C ABI of libteeline_gpu.so (include/teeline_gpu.h).  Header-only; no torch, no Python.
//
// The reference is Rust and no Rust toolchain exists in the build image, so this is the compiled-language mirror of
//   src/tsp/kdtree.rs:248-252        KDPoint
//   src/tsp/distance_matrix.rs       DistanceMatrix (packed strict lower triangle)
//   src/tsp/mod.rs:1731-1814         TspProblem, Solution
//   src/tsp/mod.rs:596-613,1249-1267 HeuristicOptions, LKOptions
//   src/tsp/tsplib.rs:101-255        tsplib::read_from_file
//   src/tsp/{two_opt,three_opt,or_opt,lin_kernighan,nearest_neighbor,greedy_edge,savings,christofides,bellman_karp}.rs  solve(problem, opts, progress, init_tour)
//   src/tsp/pipeline.rs:53-80        run_pipeline_stages (warm start + validate_tour)
// Same names, argument meaning and error behaviour: dispatcher-level failures throw std::runtime_error (the
// reference returns Err(String), mod.rs:1661), inputs on which the reference panics throw teeline::ReferencePanic.
#pragma once
#include <teeline_gpu.h>

#include <algorithm>
#include <cctype>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace teeline {

struct ReferencePanic : std::runtime_error {
    using std::runtime_error::runtime_error;
};

class Context {  // one tl_ctx per thread (teeline-api calls solvers from spawn_blocking, tsp_service.rs:295)
  public:
    explicit Context(int device = 0, uint32_t flags = TL_FLAG_NONE)
    {
        if (tl_create(device, flags, &h_) != TL_OK) throw std::runtime_error(tl_last_error(nullptr));
    }
    ~Context() { tl_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    tl_ctx *get() const { return h_; }
    void check(int rc) const
    {
        if (rc == TL_OK) return;
        if (rc == TL_ERR_BUSY) throw std::runtime_error("teeline-gpu: the context is in use by another thread (one Context per thread)");
        if (rc == TL_ERR_REF_PANICS) throw ReferencePanic(tl_last_error(h_));
        throw std::runtime_error(std::string("teeline-gpu: ") + tl_last_error(h_));
    }

  private:
    tl_ctx *h_ = nullptr;
};

namespace tsp {

struct KDPoint {  // kdtree.rs:248-252
    size_t id;
    float coords[2];
};

enum class DistanceType { Euc2D, Geo, Explicit };  // mod.rs DistanceType

class DistanceMatrix {  // distance_matrix.rs:82-212
  public:
    DistanceMatrix() = default;
    DistanceMatrix(size_t n, std::vector<float> items, const std::vector<KDPoint> &cities, DistanceType kind)
        : n_(n), items_(std::move(items)), kind_(kind)
    {
        if (items_.size() != n * (n - 1) / 2) throw std::runtime_error("distances length != n*(n-1)/2");  // :100-107
        for (size_t p = 0; p < cities.size(); ++p) city_idx_[cities[p].id] = p;
        if (city_idx_.size() != n) throw std::runtime_error("city_idx size differs from n cities");  // :99
    }
    // DistanceMatrix::build (:122-153) on the GPU
    static DistanceMatrix build(Context &ctx, const std::vector<KDPoint> &cities, DistanceType dt)
    {
        if (cities.size() < 2) throw std::runtime_error("distance matrix requires at least 2 points");
        if (dt == DistanceType::Explicit)
            throw std::runtime_error("cannot build distance matrix from coordinates for EXPLICIT type — use DistanceMatrix::new() with precomputed distances");
        std::vector<float> xy;
        for (auto &c : cities) { xy.push_back(c.coords[0]); xy.push_back(c.coords[1]); }
        const size_t n = cities.size();
        std::vector<float> items(n * (n - 1) / 2);
        ctx.check(tl_dm_build(ctx.get(), xy.data(), (uint32_t)n, dt == DistanceType::Geo ? TL_DIST_GEO : TL_DIST_EUC2D,
                              TL_DM_PACKED_LOWER, items.data(), nullptr));
        return DistanceMatrix(n, std::move(items), cities, dt);
    }
    size_t num_cities() const { return n_; }
    const std::vector<float> &distances() const { return items_; }
    DistanceType kind() const { return kind_; }
    float distance_by_pos(size_t p, size_t q) const  // :177-191
    {
        if (p == q) return 0.0f;
        if (p >= n_ || q >= n_) throw std::out_of_range("position out of range");
        const size_t from = std::max(p, q), to = std::min(p, q);
        return items_.at(from * (from - 1) / 2 + to);
    }
    float distance_between(size_t id1, size_t id2) const  // :197-212
    {
        if (id1 == id2) return 0.0f;
        return distance_by_pos(city_idx_.at(id1), city_idx_.at(id2));
    }
    bool city_id2pos(size_t id, size_t &pos) const
    {
        auto it = city_idx_.find(id);
        if (it == city_idx_.end()) return false;
        pos = it->second;
        return true;
    }

  private:
    size_t n_ = 0;
    std::vector<float> items_;
    DistanceType kind_ = DistanceType::Euc2D;
    std::unordered_map<size_t, size_t> city_idx_;
};

struct TspProblem {  // mod.rs:1731-1741
    std::vector<KDPoint> cities;
    DistanceMatrix distances;  // may be empty for plain EUC_2D: the kernels compute the identical f32 values on the fly
    DistanceType distance_type = DistanceType::Euc2D;

    std::vector<float> xy() const
    {
        std::vector<float> v;
        v.reserve(cities.size() * 2);
        for (auto &c : cities) { v.push_back(c.coords[0]); v.push_back(c.coords[1]); }
        return v;
    }
    const float *explicit_packed() const { return distance_type == DistanceType::Euc2D ? nullptr : distances.distances().data(); }
    std::vector<uint32_t> positions_of(const std::vector<size_t> &tour) const
    {
        std::unordered_map<size_t, uint32_t> idx;
        for (size_t p = 0; p < cities.size(); ++p) idx[cities[p].id] = (uint32_t)p;
        std::vector<uint32_t> out;
        for (size_t id : tour) {
            auto it = idx.find(id);
            if (it == idx.end()) throw ReferencePanic("two_opt: invalid city pair");  // two_opt.rs:37-47 .expect(...)
            out.push_back(it->second);
        }
        // a tour crosses the C ABI as n u32 values: a shorter one would be read past its end by the library
        if (out.size() != cities.size()) throw std::runtime_error("tour length differs from the number of cities");
        return out;
    }
};

struct HeuristicOptions {  // mod.rs:596-613
    size_t epochs = 10000, platoo_epochs = 500, n_nearest = 3;
    bool verbose = false;
};
struct LKOptions {  // mod.rs:1249-1267
    HeuristicOptions heuristic{100, 10, 5, false};
    size_t max_depth = 5;
};

struct Solution {  // mod.rs:1753-1814
    float total = 0.0f;
    std::vector<size_t> route_;
    tl_stats stats{};
    const std::vector<size_t> &route() const { return route_; }
};

enum class ProgressKind { PathUpdate, CityChange, Done, EpochUpdate };  // EpochUpdate(epoch): the epoch is the one entry of the id list
using ProgressFn = std::function<void(ProgressKind, const std::vector<size_t> &, float)>;  // progress.rs ProgressMessage

inline bool validate_tour(const std::vector<size_t> &tour, const std::vector<KDPoint> &cities)  // mod.rs:1620-1634
{
    if (tour.size() != cities.size()) return false;
    std::vector<size_t> a(tour), b;
    for (auto &c : cities) b.push_back(c.id);
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    return a == b;
}

namespace detail {  // what the solves share; the seeded solvers' frame reads side by side with host/_chains.py
inline bool live(const ProgressFn *tx) { return tx && *tx; }

inline Solution finish(const TspProblem &p, const std::vector<uint32_t> &pos, float cost, const tl_stats &st, const ProgressFn *tx)
{
    Solution s;
    s.total = cost;
    s.stats = st;
    for (uint32_t q : pos) s.route_.push_back(p.cities[q].id);
    if (live(tx)) {
        (*tx)(ProgressKind::PathUpdate, s.route_, cost);
        (*tx)(ProgressKind::Done, s.route_, cost);
    }
    return s;
}

// The prologue of a solve: the instance as the C ABI takes it, the start tour as positions (ip == nullptr: city order) and where
// the result lands
struct Call {
    std::vector<float> xy;
    uint32_t n;
    const float *packed;
    std::vector<uint32_t> init, out;
    const uint32_t *ip = nullptr;
    float cost = 0.f;
    tl_stats st{};

    Call(const TspProblem &problem, const std::vector<size_t> *init_tour)
        : xy(problem.xy()), n((uint32_t)problem.cities.size()), packed(problem.explicit_packed()), out(n)
    {
        if (!init_tour) return;
        init = problem.positions_of(*init_tour);
        ip = init.data();
    }
    Call(const Call &) = delete;
    Call &operator=(const Call &) = delete;
    std::vector<uint32_t> start_tour() const  // the tour a descent or a chain starts from: the given positions, or city order
    {
        std::vector<uint32_t> pos(n);
        for (uint32_t q = 0; q < n; ++q) pos[q] = ip ? init[q] : q;
        return pos;
    }
};

// the result of a call that has sent its own PathUpdates, and Done
inline Solution finish_done(const TspProblem &p, const Call &c, const ProgressFn *tx, bool done = true)
{
    Solution s = finish(p, c.out, c.cost, c.st, nullptr);
    if (done) (*tx)(ProgressKind::Done, s.route_, c.cost);
    return s;
}

// call(cap, &len) runs a trace entry with room for cap records; where it had more (len > cap) it runs again with room for all:
// every solver is deterministic, so the second run has the same records.  Returns len.
template <class F> uint32_t grow_trace(uint32_t cap, F &&call)
{
    uint32_t len = 0;
    for (;;) {
        call(cap, &len);
        if (len <= cap) break;
        cap = len;
    }
    return len;
}

inline float bits_to_f32(uint32_t bits)  // the f32 a trace record carries as a u32
{
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}

// send(pos, d): n positions -> city ids -> PathUpdate(route, d)
inline auto route_sender(const TspProblem &problem, const ProgressFn *tx)
{
    return [&problem, tx, route = std::vector<size_t>(problem.cities.size())](const uint32_t *pos, float d) mutable {
        for (size_t q = 0; q < route.size(); ++q) route[q] = problem.cities[pos[q]].id;
        (*tx)(ProgressKind::PathUpdate, route, d);
    };
}

// KDPoint::distance (kdtree.rs:291-295) of the cities at positions p and q: separate roundings, correctly rounded sqrt.  The
// volatile intermediates are the rounding specification: no product may be fused into the sum.
inline float dist_f32(const std::vector<float> &xy, uint32_t p, uint32_t q)
{
    if (p == q) return 0.0f;
    const volatile float dx = xy[2 * p] - xy[2 * q], dy = xy[2 * p + 1] - xy[2 * q + 1];
    const volatile float sx = dx * dx, sy = dy * dy;
    const volatile float ss = sx + sy;
    return std::sqrt((float)ss);
}

// A population of tours, each refined by its own descent: population(c, init, count, out, costs, moves, &st) is the entry of
// 2-opt, 3-opt or Or-opt; element k equals that solver's solve(ctx, problem, {}, nullptr, &init_tours[k]).
template <class P>
std::vector<Solution> solve_population(const TspProblem &problem, const std::vector<std::vector<size_t>> &init_tours, std::vector<uint32_t> *moves, P &&population)
{
    Call c(problem, nullptr);
    const uint32_t n = c.n, count = (uint32_t)init_tours.size();
    std::vector<uint32_t> init((size_t)count * n), out((size_t)count * n), mv(count);
    for (uint32_t k = 0; k < count; ++k) {
        const auto pos = problem.positions_of(init_tours[k]);
        std::copy(pos.begin(), pos.end(), init.begin() + (size_t)k * n);
    }
    std::vector<float> costs(count);
    population(c, init.data(), count, out.data(), costs.data(), mv.data(), &c.st);
    std::vector<Solution> res;
    for (uint32_t k = 0; k < count; ++k) {
        std::vector<uint32_t> one(out.begin() + (size_t)k * n, out.begin() + (size_t)(k + 1) * n);
        res.push_back(finish(problem, one, costs[k], c.st, nullptr));
    }
    if (moves) *moves = mv;
    return res;
}

// What greedy edge, savings and Christofides send: fewer than min_n cities, Done alone; otherwise the identity (cities in file
// order) with 0.0 before the selection, then the route with its length, then Done
inline void construction_messages(const TspProblem &problem, const Solution &s, const ProgressFn *tx, uint32_t min_n)
{
    if (!live(tx)) return;
    if (problem.cities.size() >= min_n) {
        std::vector<size_t> identity;
        for (auto &c : problem.cities) identity.push_back(c.id);
        (*tx)(ProgressKind::PathUpdate, identity, 0.0f);
        (*tx)(ProgressKind::PathUpdate, s.route_, s.total);
    }
    (*tx)(ProgressKind::Done, s.route_, s.total);
}

// _chains.solve_chains.  count > 1: population(count, outs, costs, moves, &best) runs the chains (or runs) at once into c.st and the
// best one (lowest cost, then lowest index) is kept, st.moves its own where the entry has a moves array (has_moves; else moves is
// nullptr); with a channel that one runs once more, alone, for its trace.  Else single(), or with a channel the trace of chain 0.
// trace_and_replay(chain) runs the trace entry into c.out / c.cost / c.st and sends the reference's messages short of Done, which
// follows here unless done is false.
template <class P, class S, class T>
Solution solve_chains(const TspProblem &problem, Call &c, const ProgressFn *tx, uint32_t count, bool has_moves, P &&population, S &&single, T &&trace_and_replay,
                      bool done = true)
{
    uint32_t best = 0;
    if (count > 1) {
        std::vector<uint32_t> outs((size_t)count * c.n), moves(count);
        std::vector<float> costs(count);
        population(count, outs.data(), costs.data(), has_moves ? moves.data() : nullptr, &best);
        std::copy(outs.begin() + (size_t)best * c.n, outs.begin() + (size_t)(best + 1) * c.n, c.out.begin());
        c.cost = costs[best];
        if (has_moves) c.st.moves = moves[best];
        if (!live(tx)) return finish(problem, c.out, c.cost, c.st, nullptr);
    } else if (!live(tx)) {
        single();
        return finish(problem, c.out, c.cost, c.st, nullptr);
    }
    trace_and_replay(best);
    return finish_done(problem, c, tx, done);
}

// _chains.solve_swarm: solve_chains over the three entries of one population solver (particle_swarm, cuckoo_search,
// flower_pollination, gravitational_search), `o` its opts struct.  The trace's log (epoch, who, cost bits, route index) and routes
// grow until they hold every improvement; the replay is the reference's: PathUpdate(start best), per epoch its improvements in order
// and EpochUpdate(epoch), then Done.
template <class Opts>
Solution solve_swarm(Context &ctx, const TspProblem &problem, const ProgressFn *tx, const std::vector<size_t> *init_tour, uint64_t seed, uint32_t runs, const Opts &o,
                     int (*single_fn)(tl_ctx *, const float *, uint32_t, const float *, const uint32_t *, const Opts *, uint64_t, uint32_t *, float *, tl_stats *),
                     int (*trace_fn)(tl_ctx *, const float *, uint32_t, const float *, const uint32_t *, const Opts *, uint64_t, uint32_t, uint32_t *, float *, tl_stats *,
                                     uint32_t *, uint32_t, uint32_t *, uint32_t *, uint32_t, uint32_t *, uint32_t),
                     int (*population_fn)(tl_ctx *, const float *, uint32_t, const float *, const uint32_t *, uint32_t, uint32_t, uint32_t, const Opts *, uint64_t,
                                          uint32_t *, float *, uint32_t *, uint32_t *, tl_stats *))
{
    Call c(problem, init_tour);
    const uint32_t n = c.n;
    return solve_chains(
        problem, c, tx, runs, false,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *moves, uint32_t *best) {
            ctx.check(population_fn(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.ip ? 1u : 0u, 0u, count, &o, seed, outs, costs, moves, best, &c.st));
        },
        [&] { ctx.check(single_fn(ctx.get(), c.xy.data(), n, c.packed, c.ip, &o, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t run) {
            std::vector<uint32_t> log, routes;
            const uint32_t rows = grow_trace(64u, [&](uint32_t cap, uint32_t *got) {  // the improvements are few but not known in advance
                log.assign((size_t)cap * 4, 0u);
                routes.assign((size_t)cap * std::max(n, 1u), 0u);
                ctx.check(trace_fn(ctx.get(), c.xy.data(), n, c.packed, c.ip, &o, seed, run, c.out.data(), &c.cost, &c.st, log.data(), cap, got, routes.data(), cap,
                                   nullptr, 0u));
            });
            auto send = route_sender(problem, tx);
            const auto path_update = [&](uint32_t k) { send(routes.data() + (size_t)k * n, bits_to_f32(log[(size_t)k * 4 + 2])); };
            if (rows == 0) return;
            path_update(0);
            uint32_t k = 1;
            for (uint32_t e = 0; e < o.epochs; ++e) {
                for (; k < rows && log[(size_t)k * 4] == e; ++k) path_update(k);
                (*tx)(ProgressKind::EpochUpdate, std::vector<size_t>{e}, 0.0f);
            }
        });
}
}  // namespace detail

namespace two_opt {  // two_opt.rs:7-67
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions & /*_opts*/, const ProgressFn *progress_tx,
                      const std::vector<size_t> *init_tour, int mode = TL_MODE_REF_ORDER)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n;
    // With a progress callback the descent also lists its moves (tl_two_opt_trace) and the reference's exact message sequence —
    // CityChange(path[i]) per outer i of every sweep, PathUpdate(path, new_distance) per move (two_opt.rs:30-32,53-56) — is
    // replayed from them once the kernel is back (coordinates within the LDS-resident descent, or problem.distances of a GEO /
    // EXPLICIT problem); otherwise the final PathUpdate (detail::finish).
    if (detail::live(progress_tx) && mode == TL_MODE_REF_ORDER && n >= 3 && n <= 65535u && (c.packed || n <= tl_two_opt_lds_max_n(ctx.get()))) {
        auto send = detail::route_sender(problem, progress_tx);
        std::vector<uint32_t> pos = c.start_tour(), log;
        send(pos.data(), 0.0f);  // :22-24
        const uint32_t len = detail::grow_trace(std::max<uint32_t>(64u, 16u * n), [&](uint32_t cap, uint32_t *got) {
            log.assign(cap, 0u);
            ctx.check(tl_two_opt_trace(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.out.data(), &c.cost, &c.st, log.data(), cap, got));
        });
        auto d = [&](uint32_t p, uint32_t q) { return c.packed ? problem.distances.distance_by_pos(p, q) : detail::dist_f32(c.xy, p, q); };
        size_t k = 0;
        std::vector<size_t> one(1);
        for (uint64_t sw = 0; sw < c.st.sweeps; ++sw, k += (k < len && log[k] == TL_TRACE_SWEEP) ? 1 : 0)
            for (uint32_t i = 0; i + 3 < n; ++i) {
                one[0] = problem.cities[pos[i]].id;
                (*progress_tx)(ProgressKind::CityChange, one, 0.0f);
                while (k < len && log[k] != TL_TRACE_SWEEP && (log[k] >> 16) == i) {
                    const uint32_t j = log[k] & 0xFFFFu;
                    const float new_distance = d(pos[i], pos[j]) + d(pos[i + 1], pos[j + 1]);
                    std::reverse(pos.begin() + i + 1, pos.begin() + j + 1);
                    send(pos.data(), new_distance);
                    ++k;
                }
            }
        return detail::finish_done(problem, c, progress_tx);
    }
    ctx.check(tl_two_opt(ctx.get(), c.xy.data(), n, c.packed, c.ip, mode, c.out.data(), &c.cost, &c.st));
    return detail::finish(problem, c.out, c.cost, c.st, progress_tx);
}

// A population of tours, each refined by its own descent, all concurrently (tl_two_opt_population; mode TL_MODE_BEST_SWEEP:
// tl_two_opt_best_population, coordinates only); element k equals solve(ctx, problem, {}, nullptr, &init_tours[k], mode).
// moves (optional, best-sweep only): the moves each descent applied.
inline std::vector<Solution> solve_population(Context &ctx, const TspProblem &problem, const std::vector<std::vector<size_t>> &init_tours,
                                              int mode = TL_MODE_REF_ORDER, std::vector<uint32_t> *moves = nullptr)
{
    return detail::solve_population(problem, init_tours, mode == TL_MODE_BEST_SWEEP ? moves : nullptr,
                                    [&](const detail::Call &c, const uint32_t *init, uint32_t count, uint32_t *out, float *costs, uint32_t *mv, tl_stats *st) {
                                        if (mode == TL_MODE_BEST_SWEEP) {
                                            if (c.packed) throw std::runtime_error("TL_MODE_BEST_SWEEP needs EUC_2D coordinates");
                                            ctx.check(tl_two_opt_best_population(ctx.get(), c.xy.data(), c.n, init, count, out, costs, mv, st));
                                        } else {
                                            ctx.check(tl_two_opt_population(ctx.get(), c.xy.data(), c.n, c.packed, init, count, out, costs, st));
                                        }
                                    });
}

// Multi-start 2-opt (tl_two_opt_multistart; no counterpart in the reference): restarts [first, first + restarts) from seeded
// Fisher-Yates permutations, all at once; the best tour, *best_restart (optional) the restart it came from.
inline Solution multistart(Context &ctx, const TspProblem &problem, uint32_t restarts, uint64_t seed = 0, uint32_t first = 0, int mode = TL_MODE_REF_ORDER,
                           uint32_t *best_restart = nullptr)
{
    detail::Call c(problem, nullptr);
    uint32_t br = 0;
    ctx.check(tl_two_opt_multistart(ctx.get(), c.xy.data(), c.n, seed, first, restarts, mode, c.out.data(), &c.cost, &br, nullptr, &c.st));
    if (best_restart) *best_restart = br;
    return detail::finish(problem, c.out, c.cost, c.st, nullptr);
}
}  // namespace two_opt

namespace three_opt {  // three_opt.rs:16-51
// three_opt.rs:186-218 apply_3opt: cases 1-3 reverse segments in place, 4-7 swap path[i+1..=j] and path[j+1..=k] with either reversed
inline void apply_3opt(std::vector<uint32_t> &path, uint32_t i, uint32_t j, uint32_t k, uint32_t kase)
{
    auto b1 = path.begin() + i + 1, e1 = path.begin() + j + 1, e2 = path.begin() + k + 1;
    switch (kase) {
    case 1: std::reverse(b1, e1); break;
    case 2: std::reverse(e1, e2); break;
    case 3: std::reverse(b1, e1); std::reverse(e1, e2); break;
    case 4: case 5: case 6: case 7: {
        std::vector<uint32_t> s1(b1, e1), s2(e1, e2);
        if (kase == 5 || kase == 7) std::reverse(s1.begin(), s1.end());
        if (kase == 6 || kase == 7) std::reverse(s2.begin(), s2.end());
        std::copy(s2.begin(), s2.end(), b1);
        std::copy(s1.begin(), s1.end(), b1 + (std::ptrdiff_t)s2.size());
        break;
    }
    default: throw std::runtime_error("apply_3opt: case must be 1-7");
    }
}

inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &, const ProgressFn *progress_tx,
                      const std::vector<size_t> *init_tour)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n;
    if (!detail::live(progress_tx) || n < 4) {  // (n < 4: the reference returns before its first message, three_opt.rs:25-28)
        ctx.check(tl_three_opt(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.out.data(), &c.cost, &c.st));
        return detail::finish(problem, c.out, c.cost, c.st, nullptr);
    }
    // With a progress callback the solve also lists its moves (tl_three_opt_trace) and the reference's message sequence — the
    // start path, the path after every apply_3opt (each with 0.0), Done (three_opt.rs:34,42,47-49) — is replayed from them.
    std::vector<uint32_t> log;
    const uint32_t len = detail::grow_trace(std::max<uint32_t>(64u, 4u * n), [&](uint32_t cap, uint32_t *got) {
        log.assign((size_t)cap * 4, 0u);
        ctx.check(tl_three_opt_trace(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.out.data(), &c.cost, &c.st, log.data(), cap, got));
    });
    auto send = detail::route_sender(problem, progress_tx);
    std::vector<uint32_t> pos = c.start_tour();
    send(pos.data(), 0.0f);
    for (uint32_t m = 0; m < len; ++m) {
        apply_3opt(pos, log[4 * m], log[4 * m + 1], log[4 * m + 2], log[4 * m + 3]);
        send(pos.data(), 0.0f);
    }
    return detail::finish_done(problem, c, progress_tx);
}

// A population of tours, each refined by its own descent (tl_three_opt_population: one workgroup per tour or tour after tour, the
// library picks); element k equals solve(ctx, problem, {}, nullptr, &init_tours[k]).  moves (optional): the moves each descent applied.
inline std::vector<Solution> solve_population(Context &ctx, const TspProblem &problem, const std::vector<std::vector<size_t>> &init_tours,
                                              std::vector<uint32_t> *moves = nullptr)
{
    return detail::solve_population(problem, init_tours, moves,
                                    [&](const detail::Call &c, const uint32_t *init, uint32_t count, uint32_t *out, float *costs, uint32_t *mv, tl_stats *st) {
                                        ctx.check(tl_three_opt_population(ctx.get(), c.xy.data(), c.n, c.packed, init, count, out, costs, mv, st));
                                    });
}
}  // namespace three_opt

namespace or_opt {  // or_opt.rs:18-74
// or_opt.rs:172-184 apply_relocation: drain the segment, insert it after the old index j, forward or reversed
inline void apply_relocation(std::vector<uint32_t> &tour, size_t i, size_t seg_len, size_t j, bool reversed)
{
    std::vector<uint32_t> seg(tour.begin() + i, tour.begin() + i + seg_len);
    tour.erase(tour.begin() + i, tour.begin() + i + seg_len);
    const size_t at = j >= i + seg_len ? j - seg_len + 1 : j + 1;
    if (reversed) std::reverse(seg.begin(), seg.end());
    tour.insert(tour.begin() + at, seg.begin(), seg.end());
}

// DistanceMatrix::tour_length (distance_matrix.rs:235-245) on positions, on the host, in the reference's f32 order: the closing
// edge first, then every window — through problem.distances where the problem has a matrix, else KDPoint::distance
inline float tour_length_f32(const TspProblem &problem, const std::vector<float> &xy, const std::vector<uint32_t> &pos)
{
    if (pos.size() < 2) return 0.0f;
    const bool have_dm = problem.distances.num_cities() == pos.size();
    auto d = [&](uint32_t p, uint32_t q) { return have_dm ? problem.distances.distance_by_pos(p, q) : detail::dist_f32(xy, p, q); };
    volatile float total = d(pos.back(), pos.front());
    for (size_t k = 0; k + 1 < pos.size(); ++k) total = total + d(pos[k], pos[k + 1]);
    return total;
}

inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &, const ProgressFn *progress_tx,
                      const std::vector<size_t> *init_tour)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n;
    if (!detail::live(progress_tx) || n < 4) {  // (n < 4: the reference returns before its first message, or_opt.rs:31-34)
        ctx.check(tl_or_opt(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.out.data(), &c.cost, &c.st));
        return detail::finish(problem, c.out, c.cost, c.st, nullptr);
    }
    // With a progress callback the solve also lists its moves (tl_or_opt_trace) and the reference's message sequence — the start
    // path (0.0), the path and its tour_length after every apply_relocation, Done (or_opt.rs:40-42,62-67,70-72) — is replayed.
    std::vector<uint32_t> log;
    const uint32_t len = detail::grow_trace(std::max<uint32_t>(64u, 4u * n), [&](uint32_t cap, uint32_t *got) {
        log.assign((size_t)cap * 4, 0u);
        ctx.check(tl_or_opt_trace(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.out.data(), &c.cost, &c.st, log.data(), cap, got));
    });
    auto send = detail::route_sender(problem, progress_tx);
    std::vector<uint32_t> pos = c.start_tour();
    send(pos.data(), 0.0f);
    for (uint32_t m = 0; m < len; ++m) {
        apply_relocation(pos, log[4 * m], log[4 * m + 2], log[4 * m + 1], log[4 * m + 3] != 0u);
        send(pos.data(), tour_length_f32(problem, c.xy, pos));
    }
    return detail::finish_done(problem, c, progress_tx);
}

// A population of tours, each refined by its own descent, all concurrently (tl_or_opt_population);
// element k equals solve(ctx, problem, {}, nullptr, &init_tours[k]).  moves (optional): the moves each descent applied.
inline std::vector<Solution> solve_population(Context &ctx, const TspProblem &problem, const std::vector<std::vector<size_t>> &init_tours,
                                              std::vector<uint32_t> *moves = nullptr)
{
    return detail::solve_population(problem, init_tours, moves,
                                    [&](const detail::Call &c, const uint32_t *init, uint32_t count, uint32_t *out, float *costs, uint32_t *mv, tl_stats *st) {
                                        ctx.check(tl_or_opt_population(ctx.get(), c.xy.data(), c.n, c.packed, init, count, out, costs, mv, st));
                                    });
}
}  // namespace or_opt

namespace nearest_neighbor {  // nearest_neighbor.rs:8-76
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &opts, const ProgressFn *progress_tx,
                      const std::vector<size_t> * /*_init_tour*/)
{
    if (opts.n_nearest == 0) throw std::runtime_error("n_nearest must be >= 1");  // mod.rs:677-682
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size();
    std::vector<uint32_t> out(n);
    float cost = 0.f;
    // GEO / EXPLICIT: the walk reads problem.distances (distance_matrix.rs:259-297)
    ctx.check(tl_nearest_neighbor(ctx.get(), xy.data(), problem.explicit_packed(), n, (uint32_t)opts.n_nearest, out.data(), &cost));
    Solution s = detail::finish(problem, out, cost, tl_stats{}, nullptr);
    if (progress_tx && *progress_tx && n > 0) {
        // the reference's messages follow from the finished walk (nearest_neighbor.rs:32-34,40-42,67-69,72-74): the start city,
        // then per step CityChange(current city) and the path so far, then Done
        std::vector<size_t> path{s.route_[0]}, one(1);
        (*progress_tx)(ProgressKind::PathUpdate, path, 0.0f);
        for (uint32_t t = 1; t < n; ++t) {
            one[0] = s.route_[t - 1];
            (*progress_tx)(ProgressKind::CityChange, one, 0.0f);
            path.push_back(s.route_[t]);
            (*progress_tx)(ProgressKind::PathUpdate, path, 0.0f);
        }
        (*progress_tx)(ProgressKind::Done, s.route_, cost);
    }
    return s;
}
}  // namespace nearest_neighbor

namespace greedy_edge {  // greedy_edge.rs:21-65 over graph.rs:54-196
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions & /*_opts*/, const ProgressFn *progress_tx,
                      const std::vector<size_t> * /*_init_tour*/)
{
    detail::Call c(problem, nullptr);
    // GEO / EXPLICIT: the edges are the packed matrix's (distance_by_pos, graph.rs:62-68)
    ctx.check(tl_greedy_edge(ctx.get(), c.xy.data(), c.packed, c.n, c.out.data(), &c.cost, &c.st));
    Solution s = detail::finish(problem, c.out, c.cost, c.st, nullptr);
    detail::construction_messages(problem, s, progress_tx, 3);  // greedy_edge.rs:33-62: n <= 2 sends Done alone
    return s;
}
}  // namespace greedy_edge

namespace savings {  // savings.rs:34-82 over graph.rs:98-196
// hub (optional): receives the position nearest the coordinates' centroid that ranked the edges (tl_savings_hub)
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions & /*_opts*/, const ProgressFn *progress_tx,
                      const std::vector<size_t> * /*_init_tour*/, uint32_t *hub = nullptr)
{
    detail::Call c(problem, nullptr);
    // GEO / EXPLICIT: the edges are the packed matrix's (distance_by_pos, savings.rs:144-152); the hub is the coordinates' all the same
    ctx.check(tl_savings(ctx.get(), c.xy.data(), c.packed, c.n, TL_SAVINGS_HUB_AUTO, c.out.data(), &c.cost, hub, &c.st));
    Solution s = detail::finish(problem, c.out, c.cost, c.st, nullptr);
    detail::construction_messages(problem, s, progress_tx, 3);  // savings.rs:46-79: n <= 2 sends Done alone
    return s;
}
}  // namespace savings

namespace christofides {  // christofides.rs:12-68
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions & /*_opts*/, const ProgressFn *progress_tx,
                      const std::vector<size_t> * /*_init_tour*/)
{
    detail::Call c(problem, nullptr);
    // GEO / EXPLICIT: every distance is the packed matrix's (distance_by_pos, christofides.rs:102-104, :147-149)
    ctx.check(tl_christofides(ctx.get(), c.xy.data(), c.packed, c.n, c.out.data(), &c.cost, &c.st));
    Solution s = detail::finish(problem, c.out, c.cost, c.st, nullptr);
    detail::construction_messages(problem, s, progress_tx, 4);  // christofides.rs:24-65: n < 4 sends Done alone; the identity goes out once the tree is built
    return s;
}
}  // namespace christofides

namespace bellman_karp {  // bellman_karp.rs:24-87, the exact solver (n <= TL_BHK_MAX_N)
// The route is what the reference's tolerance walk leaves (:122-156), which need not be a tour: *is_tour (optional) tells, and
// run_pipeline_stages' validate_tour rejects it as the reference's does.  A Context created with TL_FLAG_BHK_EXACT_WALK reads the
// route back by exact equality instead: always a tour while a finite one exists.  optimal (optional): the DP's optimum, which
// differs from Solution::total (tour_length of the route) in its last bits.
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions & /*opts: only `verbose` is read, to print the table*/,
                      const ProgressFn *progress_tx, const std::vector<size_t> * /*_init_tour*/, float *optimal = nullptr, bool *is_tour = nullptr)
{
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size();
    std::vector<uint32_t> out(n);
    float cost = 0.f, opt = 0.f;
    uint32_t ok = 0;
    tl_stats st{};
    ctx.check(tl_bellman_karp(ctx.get(), xy.data(), problem.explicit_packed(), n, out.data(), &cost, &opt, &ok, &st));
    if (optimal) *optimal = opt;
    if (is_tour) *is_tour = ok != 0;
    Solution s = detail::finish(problem, out, cost, st, nullptr);
    if (progress_tx && *progress_tx) {
        // :48-52, :81-84: CityChange per city of the subsets in position order, the route with 0.0, Done
        for (uint32_t k = 0; k + 1 < n; ++k) (*progress_tx)(ProgressKind::CityChange, std::vector<size_t>{problem.cities[k].id}, 0.0f);
        (*progress_tx)(ProgressKind::PathUpdate, s.route_, 0.0f);
        (*progress_tx)(ProgressKind::Done, s.route_, cost);
    }
    return s;
}
}  // namespace bellman_karp

namespace lin_kernighan {  // lin_kernighan.rs:35-100
inline Solution solve(Context &ctx, const TspProblem &problem, const LKOptions &opts, const ProgressFn *progress_tx,
                      const std::vector<size_t> *init_tour, uint64_t seed = 1)
{
    if (opts.heuristic.n_nearest == 0) throw std::runtime_error("n_nearest must be >= 1");  // mod.rs:677-682
    if (opts.max_depth == 0) throw std::runtime_error("max_depth must be >= 1");            // mod.rs:1270-1276
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size();
    std::vector<uint32_t> init, out(n);
    if (init_tour) init = problem.positions_of(*init_tour);
    tl_lk_opts o{(uint32_t)opts.heuristic.epochs, (uint32_t)opts.heuristic.platoo_epochs, (uint32_t)opts.heuristic.n_nearest, (uint32_t)opts.max_depth};
    float cost = 0.f;
    tl_stats st{};
    // problem.distances (GEO / EXPLICIT) feeds the NN seed and the reported total only; the search is Euclidean (lin_kernighan.rs:41,47-55,99)
    if (!(progress_tx && *progress_tx) || n < 4) {  // (n < 4: the reference returns before its first message, lin_kernighan.rs:57-59)
        ctx.check(tl_lk(ctx.get(), xy.data(), n, problem.explicit_packed(), init_tour ? init.data() : nullptr, &o, seed, out.data(), &cost, &st));
        return detail::finish(problem, out, cost, st, nullptr);
    }
    // With a progress callback: the best tours the search settles on, in order, handed on WHILE the search runs (tl_lk_live) as the
    // reference sends them — PathUpdate(best_tour, best_dist) after the first lk_pass and per improving epoch, no Done
    // (lin_kernighan.rs:71,90).
    struct Live {
        const TspProblem *problem;
        const ProgressFn *tx;
        std::vector<size_t> route;
        std::exception_ptr err;
    } live{&problem, progress_tx, std::vector<size_t>(n), nullptr};
    auto on_best = [](void *user, const uint32_t *pos, uint32_t nn, float best_dist) {
        Live *L = static_cast<Live *>(user);
        if (L->err) return;
        try {  // an exception must not unwind through the C frames of the library
            for (uint32_t q = 0; q < nn; ++q) L->route[q] = L->problem->cities[pos[q]].id;
            (*L->tx)(ProgressKind::PathUpdate, L->route, best_dist);
        } catch (...) {
            L->err = std::current_exception();
        }
    };
    ctx.check(tl_lk_live(ctx.get(), xy.data(), n, problem.explicit_packed(), init_tour ? init.data() : nullptr, &o, seed, out.data(), &cost, &st,
                         +on_best, &live));
    if (live.err) std::rethrow_exception(live.err);
    return detail::finish(problem, out, cost, st, nullptr);
}

inline uint64_t run_seed(uint64_t seed, uint32_t run) { return tl_lk_run_seed(seed, run); }

// Seeded runs first_run .. first_run + runs - 1 at once (tl_lk_population): run r is solve(..., seed = run_seed(seed, r)), run 0 the plain
// seed's.  init_tours: none (the NN seed solve would build), one start for all runs, or one per run.  One Solution per run, each with the
// run's own counters in its stats (the times are the call's); *best (optional): the cheapest, equal totals going to the lowest run.
inline std::vector<Solution> solve_population(Context &ctx, const TspProblem &problem, const LKOptions &opts, const std::vector<std::vector<size_t>> *init_tours,
                                              uint64_t seed, uint32_t runs, uint32_t first_run = 0, uint32_t *best = nullptr)
{
    if (opts.heuristic.n_nearest == 0) throw std::runtime_error("n_nearest must be >= 1");
    if (opts.max_depth == 0) throw std::runtime_error("max_depth must be >= 1");
    if (runs == 0) throw std::runtime_error("lin_kernighan::solve_population: runs == 0");
    const size_t given = init_tours ? init_tours->size() : 0;
    if (init_tours && given != 1 && given != runs) throw std::runtime_error("lin_kernighan::solve_population: one start tour, or one per run");
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size();
    std::vector<uint32_t> init, out((size_t)runs * n);
    for (size_t k = 0; k < given; ++k) {
        const std::vector<uint32_t> row = problem.positions_of((*init_tours)[k]);
        init.insert(init.end(), row.begin(), row.end());
    }
    tl_lk_opts o{(uint32_t)opts.heuristic.epochs, (uint32_t)opts.heuristic.platoo_epochs, (uint32_t)opts.heuristic.n_nearest, (uint32_t)opts.max_depth};
    std::vector<float> costs(runs);
    std::vector<uint64_t> cnt((size_t)runs * 4);
    uint32_t bi = 0;
    tl_stats st{};
    ctx.check(tl_lk_population(ctx.get(), xy.data(), n, problem.explicit_packed(), given ? init.data() : nullptr, (uint32_t)given, first_run, runs, &o, seed,
                               out.data(), costs.data(), cnt.data(), &bi, &st));
    std::vector<Solution> sols;
    for (uint32_t r = 0; r < runs; ++r) {
        tl_stats sr = st;
        sr.sweeps = cnt[(size_t)r * 4];
        sr.candidates = cnt[(size_t)r * 4 + 1];
        sr.moves = cnt[(size_t)r * 4 + 2];
        sr.reversed = cnt[(size_t)r * 4 + 3];
        sols.push_back(detail::finish(problem, std::vector<uint32_t>(out.begin() + (size_t)r * n, out.begin() + (size_t)(r + 1) * n), costs[r], sr, nullptr));
    }
    if (best) *best = bi;
    return sols;
}
}  // namespace lin_kernighan

namespace tsplib {  // tsplib.rs:142-255

struct TspLibData {
    std::string name, comment;
    std::vector<KDPoint> cities;
    size_t dimension = 0;
    std::vector<float> raw_distances;
    bool has_raw = false;
    DistanceType distance_type = DistanceType::Euc2D;

    TspProblem problem(Context &ctx) const  // TspLibData::distance_matrix (:84-98) + TspProblem::new
    {
        TspProblem p;
        p.cities = cities;
        if (has_raw) {
            p.distances = DistanceMatrix(cities.size(), raw_distances, cities, DistanceType::Explicit);
            p.distance_type = DistanceType::Explicit;
        } else if (distance_type == DistanceType::Geo) {
            p.distances = DistanceMatrix::build(ctx, cities, DistanceType::Geo);
            p.distance_type = DistanceType::Geo;
        }
        return p;
    }
};

inline bool parse_f32(const std::string &t, float &v)
{
    char *end = nullptr;
    v = std::strtof(t.c_str(), &end);  // f32::from_str: parse straight to f32, not strtod + cast
    return end && *end == '\0' && end != t.c_str();
}

inline TspLibData read_from_string(const std::string &text)
{
    std::map<std::string, std::string> meta;
    TspLibData d;
    std::vector<float> weights;
    enum { Start, In, Out, End } state = Start;
    std::string section, raw;
    std::istringstream in(text);
    size_t line_no = 1;
    auto is_section = [](const std::string &l) {
        if (l.empty() || !(std::isupper((unsigned char)l[0]) || l[0] == '_')) return false;
        for (char ch : l)
            if (!(std::isalnum((unsigned char)ch) || ch == '_')) return false;
        return true;
    };
    while (std::getline(in, raw)) {
        size_t b = raw.find_first_not_of(" \t\r\n"), e = raw.find_last_not_of(" \t\r\n");
        std::string line = b == std::string::npos ? "" : raw.substr(b, e - b + 1);
        for (auto &ch : line) ch = (char)std::toupper((unsigned char)ch);
        ++line_no;
        if (state == End) break;
        if (is_section(line)) {
            if (line == "EOF") state = End;
            else { state = In; section = line; }
            continue;
        }
        std::istringstream ls(line);
        std::vector<std::string> tok;
        for (std::string t; ls >> t;) tok.push_back(t);
        if (state == Start) {
            size_t c = line.find(':');
            if (c == std::string::npos) throw std::runtime_error("Failed to extract meta data on line." + std::to_string(line_no));
            auto trim = [](std::string s) {
                size_t b2 = s.find_first_not_of(" \t"), e2 = s.find_last_not_of(" \t");
                return b2 == std::string::npos ? std::string() : s.substr(b2, e2 - b2 + 1);
            };
            meta[trim(line.substr(0, c))] = trim(line.substr(c + 1));
        } else if (state == In && (section == "NODE_COORD_SECTION" || section == "DISPLAY_DATA_SECTION")) {
            float f;
            if (tok.empty() || !parse_f32(tok[0], f)) throw std::runtime_error("Failed to extract coordinates on line." + std::to_string(line_no));
            if (tok.size() < 3) throw std::runtime_error("KDPoint requires at least 2 coordinates");
            KDPoint p{};
            p.id = (size_t)std::stoull(tok[0]);
            if (!parse_f32(tok[1], p.coords[0]) || !parse_f32(tok[2], p.coords[1]))
                throw std::runtime_error("Error on line." + std::to_string(line_no) + " - invalid number");
            d.cities.push_back(p);
        } else if (state == In && section == "EDGE_WEIGHT_SECTION") {
            for (auto &t : tok) {
                float f;
                if (parse_f32(t, f)) weights.push_back(f);
            }
        }
    }
    if (meta.count("TYPE") && meta["TYPE"] == "ATSP") throw std::runtime_error("ATSP (asymmetric TSP) is not supported");
    const std::string ewt = meta.count("EDGE_WEIGHT_TYPE") ? meta["EDGE_WEIGHT_TYPE"] : "";
    d.distance_type = ewt == "GEO" ? DistanceType::Geo : (ewt == "EXPLICIT" ? DistanceType::Explicit : DistanceType::Euc2D);  // unknown -> EUC_2D (:199-202)
    d.dimension = meta.count("DIMENSION") ? (size_t)std::strtoull(meta["DIMENSION"].c_str(), nullptr, 10) : 0;
    if (!weights.empty()) {
        const size_t n = d.dimension;
        const std::string fmt = meta.count("EDGE_WEIGHT_FORMAT") ? meta["EDGE_WEIGHT_FORMAT"] : "";
        std::vector<float> full(n * n, 0.0f);
        if (fmt == "FULL_MATRIX") {
            if (weights.size() != n * n) throw std::runtime_error("FULL_MATRIX: expected " + std::to_string(n * n) + " tokens, got " + std::to_string(weights.size()));
            full = weights;
        } else if (fmt == "UPPER_ROW") {
            if (weights.size() != n * (n - 1) / 2) throw std::runtime_error("UPPER_ROW: wrong token count");
            size_t k = 0;
            for (size_t i = 0; i + 1 < n; ++i)
                for (size_t j = i + 1; j < n; ++j) full[i * n + j] = full[j * n + i] = weights[k++];
        } else if (fmt == "LOWER_DIAG_ROW") {
            if (weights.size() != n * (n + 1) / 2) throw std::runtime_error("LOWER_DIAG_ROW: wrong token count");
            size_t k = 0;
            for (size_t i = 0; i < n; ++i)
                for (size_t j = 0; j <= i; ++j) full[i * n + j] = weights[k++];
        } else {
            throw std::runtime_error("Unsupported EDGE_WEIGHT_FORMAT: " + fmt);
        }
        for (size_t i = 1; i < n; ++i)
            for (size_t j = 0; j < i; ++j) d.raw_distances.push_back(full[i * n + j]);
        d.has_raw = true;
    }
    if (d.cities.empty() && d.has_raw) {  // grid placeholder coordinates (:246-258)
        const size_t cols = (size_t)std::ceil(std::sqrt((double)d.dimension));
        for (size_t i = 0; i < d.dimension; ++i) d.cities.push_back(KDPoint{i + 1, {(float)(i % cols), (float)(i / cols)}});
    }
    if (d.cities.empty()) throw std::runtime_error("Found no valid city coordinates");
    auto lower = [](std::string s) { for (auto &ch : s) ch = (char)std::tolower((unsigned char)ch); return s; };
    d.name = lower(meta.count("NAME") ? meta["NAME"] : "unspecified");
    d.comment = lower(meta.count("COMMENT") ? meta["COMMENT"] : "unspecified");
    return d;
}

inline TspLibData read_from_file(const std::string &path)
{
    std::ifstream f(path);
    if (!f) throw std::runtime_error("tsplib: failed to read file");
    std::stringstream ss;
    ss << f.rdbuf();
    return read_from_string(ss.str());
}

}  // namespace tsplib

namespace opt_tour {  // opt_tour.rs:12-107
struct OptTour {
    std::string name, comment;
    size_t dimension = 0;
    std::vector<size_t> route;
};

inline OptTour read_from_string(const std::string &text)
{
    std::map<std::string, std::string> meta;
    OptTour t;
    enum { Header, TourSection, End } state = Header;
    std::istringstream in(text);
    std::string raw;
    while (std::getline(in, raw)) {
        size_t b = raw.find_first_not_of(" \t\r\n"), e = raw.find_last_not_of(" \t\r\n");
        std::string line = b == std::string::npos ? "" : raw.substr(b, e - b + 1);
        for (auto &ch : line) ch = (char)std::toupper((unsigned char)ch);
        if (line == "EOF" || state == End) break;
        if (state == Header) {
            if (line == "TOUR_SECTION") {
                state = TourSection;
                continue;
            }
            // ^(\w+)\s*:\s*(.+)$
            size_t k = 0;
            while (k < line.size() && (std::isalnum((unsigned char)line[k]) || line[k] == '_')) ++k;
            size_t c = k;
            while (c < line.size() && std::isspace((unsigned char)line[c])) ++c;
            if (k == 0 || c >= line.size() || line[c] != ':') continue;
            size_t v = c + 1;
            while (v < line.size() && std::isspace((unsigned char)line[v])) ++v;
            if (v >= line.size()) continue;
            meta[line.substr(0, k)] = line.substr(v);
        } else {
            std::istringstream ls(line);
            for (std::string tok; ls >> tok;) {
                char *end = nullptr;
                const long long id = std::strtoll(tok.c_str(), &end, 10);
                if (!end || *end != '\0' || end == tok.c_str()) continue;  // isize::from_str failed: ignored
                if (id == -1) {
                    state = End;
                    break;
                }
                if (id > 0) t.route.push_back((size_t)id);
            }
        }
    }
    const std::string ty = meta.count("TYPE") ? meta["TYPE"] : "";
    if (ty != "TOUR") throw std::runtime_error("opt_tour: expected TYPE : TOUR, found TYPE : " + ty);
    t.dimension = 0;
    if (meta.count("DIMENSION")) {
        char *end = nullptr;
        const unsigned long long d = std::strtoull(meta["DIMENSION"].c_str(), &end, 10);
        if (end && *end == '\0' && end != meta["DIMENSION"].c_str()) t.dimension = (size_t)d;
    }
    if (t.route.size() != t.dimension)
        throw std::runtime_error("opt_tour: dimension mismatch — DIMENSION=" + std::to_string(t.dimension) + " but parsed " +
                                 std::to_string(t.route.size()) + " cities");
    t.name = meta.count("NAME") ? meta["NAME"] : "unknown";
    t.comment = meta.count("COMMENT") ? meta["COMMENT"] : "";
    return t;
}

inline OptTour read_from_file(const std::string &path)
{
    std::ifstream f(path);
    if (!f) throw std::runtime_error("opt_tour: cannot open file: " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return read_from_string(ss.str());
}
}  // namespace opt_tour

namespace random_shuffle {  // random_shuffle.rs:12-27, seeded (the reference draws from an unseeded thread RNG, :20)
// Fisher-Yates `for i in (1..n).rev(): j = rng % (i+1); swap` driven by splitmix64 seeded with `seed` — the same stream the
// device draws restart 0 of `seed` from (two_opt_ref.hip, oracle tlo_restart_perm), so a `shuffle` stage and a multi-start
// restart agree.
inline Solution solve(Context &ctx, const TspProblem &problem, uint64_t seed)
{
    const uint32_t n = (uint32_t)problem.cities.size();
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    uint64_t st = seed;
    for (uint32_t i = n; i-- > 1;) {
        uint64_t z = (st += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        std::swap(perm[i], perm[(uint32_t)(z % ((uint64_t)i + 1))]);
    }
    float cost = 0.f;
    if (n >= 2) {
        const auto xy = problem.xy();
        ctx.check(tl_tour_length(ctx.get(), problem.explicit_packed() ? nullptr : xy.data(), problem.explicit_packed(), n, perm.data(), &cost));
    }
    return detail::finish(problem, perm, cost, tl_stats{}, nullptr);
}
}  // namespace random_shuffle

namespace simulated_annealing {  // simulated_annealing.rs:10-83
struct SAOptions {  // mod.rs:689-706
    HeuristicOptions heuristic;
    float cooling_rate = 0.0001f, min_temperature = 0.001f, max_temperature = 1000.0f;
    // SAOptions::validate (mod.rs:708-742): the message, or empty
    std::string validate() const
    {
        char b[128] = "";
        if (heuristic.n_nearest == 0) return "n_nearest must be >= 1";
        if (cooling_rate <= 0.0f) std::snprintf(b, sizeof b, "cooling_rate must be > 0 (got %g)", cooling_rate);
        else if (cooling_rate >= 1.0f) std::snprintf(b, sizeof b, "cooling_rate must be < 1 (got %g)", cooling_rate);
        else if (max_temperature <= 0.0f) std::snprintf(b, sizeof b, "max_temperature must be > 0 (got %g)", max_temperature);
        else if (min_temperature < 0.0f) std::snprintf(b, sizeof b, "min_temperature must be >= 0 (got %g)", min_temperature);
        else if (min_temperature >= max_temperature)
            std::snprintf(b, sizeof b, "min_temperature (%g) must be < max_temperature (%g)", min_temperature, max_temperature);
        return b;
    }
};

// The chain is the reference's; its random draws (a pure function of seed, chain, epoch and slot) and the evaluation of exp are this
// project's specification (include/teeline_gpu.h).  chains > 1: chains 0 .. chains-1 of the seed at once, the best one returned
// (lowest cost, then lowest chain).  With a progress callback the reference's messages — PathUpdate(route, distance) for the start
// route and after every accepted epoch, then Done (simulated_annealing.rs:33-38,49-54,63-65) — are replayed from the accepted
// epochs of that chain (tl_sim_anneal_trace_chain).
inline Solution solve(Context &ctx, const TspProblem &problem, const SAOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t chains = 1)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n;
    const tl_sa_opts o{(uint32_t)opts.heuristic.epochs, opts.cooling_rate, opts.min_temperature, opts.max_temperature};
    return detail::solve_chains(
        problem, c, progress_tx, chains, true,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *moves, uint32_t *best) {
            ctx.check(tl_sim_anneal_population(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.ip ? 1u : 0u, 0u, count, &o, seed, outs, costs, moves, best, &c.st));
        },
        [&] { ctx.check(tl_sim_anneal(ctx.get(), c.xy.data(), n, c.packed, c.ip, &o, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t chain) {
            std::vector<uint32_t> log;
            const uint32_t len = detail::grow_trace(1u << 14, [&](uint32_t cap, uint32_t *got) {  // room for every accepted epoch
                log.assign((size_t)cap * 4, 0u);
                ctx.check(tl_sim_anneal_trace_chain(ctx.get(), c.xy.data(), n, c.packed, c.ip, &o, seed, chain, c.out.data(), &c.cost, &c.st, log.data(), cap, got));
            });
            auto send = detail::route_sender(problem, progress_tx);
            std::vector<uint32_t> pos = c.start_tour();
            send(pos.data(), or_opt::tour_length_f32(problem, c.xy, pos));
            for (uint32_t m = 0; m < len; ++m) {
                std::reverse(pos.begin() + log[4 * m + 1], pos.begin() + log[4 * m + 2] + 1);  // swap_cities (route.rs:102-113)
                send(pos.data(), detail::bits_to_f32(log[4 * m + 3]));
            }
        });
}
}  // namespace simulated_annealing

namespace tabu_search {  // tabu_search.rs:9-110
// The chain is the reference's; its random draws (a pure function of seed, chain, epoch, attempt and slot) are this project's
// specification (include/teeline_gpu.h).  chains > 1: chains 0 .. chains-1 of the seed at once, the best one returned (lowest cost,
// then lowest chain).  With a progress callback the reference's messages — PathUpdate(start route, 0.0), PathUpdate(route, distance)
// per new best, then Done (tabu_search.rs:28-30,42-47,59-61) — are replayed from the epochs of that chain (tl_tabu_search_trace_chain).
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t chains = 1)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n, epochs = (uint32_t)opts.epochs;
    return detail::solve_chains(
        problem, c, progress_tx, chains, true,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *moves, uint32_t *best) {
            ctx.check(tl_tabu_search_population(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.ip ? 1u : 0u, 0u, count, epochs, seed, outs, costs, moves, best, &c.st));
        },
        [&] { ctx.check(tl_tabu_search(ctx.get(), c.xy.data(), n, c.packed, c.ip, epochs, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t chain) {
            // One record per epoch and epochs + 1 epochs run, so the log's length is known and nothing grows: the entry reports
            // len = epochs + 1 = cap on every call that succeeds, and refuses the epochs (0, 2^32 - 1) at which cap would not be that.
            const uint32_t cap = epochs + 1u;
            uint32_t len = 0;
            std::vector<uint32_t> log((size_t)cap * 4, 0u);
            ctx.check(tl_tabu_search_trace_chain(ctx.get(), c.xy.data(), n, c.packed, c.ip, epochs, seed, chain, c.out.data(), &c.cost, &c.st, log.data(), cap, &len));
            auto send = detail::route_sender(problem, progress_tx);
            std::vector<uint32_t> pos = c.start_tour();
            float best = or_opt::tour_length_f32(problem, c.xy, pos);
            send(pos.data(), 0.0f);
            for (uint32_t m = 0; m < len; ++m) {
                std::reverse(pos.begin() + log[4 * m + 1], pos.begin() + log[4 * m + 2] + 1);  // swap_cities (route.rs:102-113)
                const float d = detail::bits_to_f32(log[4 * m + 3]);
                if (d < best) {
                    best = d;
                    send(pos.data(), d);
                }
            }
        });
}
}  // namespace tabu_search

namespace genetic_algorithm {  // genetic_algorithm.rs:16-336
struct GAOptions {  // mod.rs:815-846
    HeuristicOptions heuristic;
    float mutation_probability = 0.001f;
    size_t n_elite = 3;
    std::string validate() const
    {
        if (!std::isfinite(mutation_probability) || mutation_probability < 0.0f || mutation_probability > 1.0f)
            return "mutation_probability must be in [0, 1] (got " + std::to_string(mutation_probability) + ")";
        return "";
    }
};
// The algorithm is the reference's; its random draws (a pure function of seed, run, generation, pair or individual, and role) are
// this project's specification (include/teeline_gpu.h).  runs > 1: runs 0 .. runs-1 of the seed at once, the best one returned
// (lowest cost, then lowest run).  With a progress callback the reference's messages — one PathUpdate(best route, its tour_length)
// per generation, one more, then Done (genetic_algorithm.rs:33-40,91-98) — are replayed from that run's trace and route log.
inline Solution solve(Context &ctx, const TspProblem &problem, const GAOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n, epochs = (uint32_t)opts.heuristic.epochs, e = (uint32_t)std::min<size_t>(opts.n_elite, 0xFFFFFFFFu);
    const float p = opts.mutation_probability;
    return detail::solve_chains(
        problem, c, progress_tx, runs, false,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *, uint32_t *best) {
            ctx.check(tl_genetic_algorithm_population(ctx.get(), c.xy.data(), n, c.packed, c.ip, 0u, count, epochs, p, e, seed, outs, costs, best, &c.st));
        },
        [&] { ctx.check(tl_genetic_algorithm(ctx.get(), c.xy.data(), n, c.packed, c.ip, epochs, p, e, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t run) {
            uint32_t len = 0;
            std::vector<uint32_t> log((size_t)std::max(epochs, 1u) * 4, 0u), routes((size_t)std::max(epochs, 1u) * n, 0u);
            ctx.check(tl_genetic_algorithm_trace_run(ctx.get(), c.xy.data(), n, c.packed, c.ip, epochs, p, e, seed, run, c.out.data(), &c.cost, &c.st, log.data(), epochs,
                                                     &len, routes.data(), epochs));
            auto send = detail::route_sender(problem, progress_tx);
            for (uint32_t g = 0; g < len && g < epochs; ++g) send(routes.data() + (size_t)g * n, detail::bits_to_f32(log[4 * (size_t)g + 2]));
            send(c.out.data(), c.cost);  // the one more: the result itself
        });
}
}  // namespace genetic_algorithm

namespace ant_colony {  // ant_colony.rs:97-252
struct AcoOptions {  // mod.rs:1082-1153
    HeuristicOptions heuristic;
    float alpha = 1.0f, beta = 2.0f, evaporation_rate = 0.5f;
    size_t num_ants = 25;
    AcoOptions() { heuristic.epochs = 150; }
    std::string validate() const
    {
        if (!std::isfinite(alpha) || alpha < 0.0f) return "alpha must be >= 0 (got " + std::to_string(alpha) + ")";
        if (!(beta >= 0.0f && beta <= 6.0f)) return "beta must be in [0, 6] (got " + std::to_string(beta) + ")";
        if (!std::isfinite(evaporation_rate) || evaporation_rate <= 0.0f || evaporation_rate >= 1.0f)
            return "evaporation_rate must be in (0, 1) (got " + std::to_string(evaporation_rate) + ")";
        if (num_ants == 0) return "num_ants must be >= 1";
        return "";
    }
};
// The algorithm is the reference's; its random draws and its power function are this project's specification
// (include/teeline_gpu.h).  runs > 1: runs 0 .. runs-1 of the seed at once, the best one returned (lowest cost, then lowest run).
// With a progress callback the reference's messages — PathUpdate(start tour), per epoch a PathUpdate per improving ant in ant order
// and EpochUpdate(epoch), then Done (ant_colony.rs:141-147,225-231,241-248) — are replayed from that run's route log.
inline Solution solve(Context &ctx, const TspProblem &problem, const AcoOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n, epochs = (uint32_t)opts.heuristic.epochs, ants = (uint32_t)std::min<size_t>(opts.num_ants, 0xFFFFFFFFu);
    const float a = opts.alpha, b = opts.beta, r = opts.evaporation_rate;
    return detail::solve_chains(
        problem, c, progress_tx, runs, false,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *, uint32_t *best) {
            ctx.check(tl_ant_colony_population(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.ip ? 1u : 0u, 0u, count, epochs, a, b, r, ants, seed, outs, costs, best, &c.st));
        },
        [&] { ctx.check(tl_ant_colony(ctx.get(), c.xy.data(), n, c.packed, c.ip, epochs, a, b, r, ants, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t run) {
            // the trace is the colony's own: one epoch-log row, and a route log of rows (epoch, ant, cost bits, the n positions) that
            // holds every improving ant
            uint32_t len = 0;
            std::vector<uint32_t> log((size_t)3 * std::max(ants, 1u), 0u), routes;
            const uint32_t rows = detail::grow_trace(64u, [&](uint32_t cap, uint32_t *got) {
                routes.assign((size_t)cap * (n + 3), 0u);
                ctx.check(tl_ant_colony_trace_run(ctx.get(), c.xy.data(), n, c.packed, c.ip, epochs, a, b, r, ants, seed, run, c.out.data(), &c.cost, &c.st, log.data(), 1u,
                                                  &len, routes.data(), cap, got));
            });
            auto send = detail::route_sender(problem, progress_tx);
            const auto path_update = [&](uint32_t k) {
                const uint32_t *rec = routes.data() + (size_t)k * (n + 3);
                send(rec + 3, detail::bits_to_f32(rec[2]));
            };
            if (rows == 0) return;  // (n <= 2: no row, the reference sends Done alone)
            path_update(0);
            uint32_t k = 1;
            for (uint32_t g = 0; g < epochs; ++g) {
                for (; k < rows && routes[(size_t)k * (n + 3)] == g; ++k) path_update(k);
                (*progress_tx)(ProgressKind::EpochUpdate, std::vector<size_t>{g}, 0.0f);
            }
        });
}
}  // namespace ant_colony

namespace particle_swarm {  // particle_swarm.rs:22-129
// The algorithm is the reference's; its random draws and its rounding are this project's specification (include/teeline_gpu.h).
// The particle count is max(opts.n_nearest, 30).  runs > 1: runs 0 .. runs-1 of the seed at once, the best one returned (lowest
// cost, then lowest run).  With a progress callback the reference's messages — PathUpdate(start gbest), per epoch a PathUpdate per
// gbest improvement in particle order and EpochUpdate(epoch), then Done (particle_swarm.rs:72-74,114-127) — are replayed from that
// run's improvement log.
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    const tl_pso_opts o{(uint32_t)opts.epochs, (uint32_t)std::min<size_t>(opts.n_nearest, 0xFFFFFFFFu)};
    return detail::solve_swarm(ctx, problem, progress_tx, init_tour, seed, runs, o, tl_particle_swarm, tl_particle_swarm_trace, tl_particle_swarm_population);
}
}  // namespace particle_swarm

namespace cuckoo_search {  // cuckoo_search.rs:26-136
// The algorithm is the reference's; its random draws and its Levy step are this project's specification (include/teeline_gpu.h).
// The nest count is max(opts.heuristic.n_nearest, 25).  runs > 1: runs 0 .. runs-1 of the seed at once, the best one returned
// (lowest cost, then lowest run).  With a progress callback the reference's messages — PathUpdate(start best), per epoch a
// PathUpdate per best improvement in the order they happen and EpochUpdate(epoch), then Done (cuckoo_search.rs:73-75,98-100,120-134)
// — are replayed from that run's improvement log.
struct CSOptions {  // mod.rs:913-940
    HeuristicOptions heuristic;
    float mutation_probability = 0.001f;
    std::string validate() const
    {
        if (!std::isfinite(mutation_probability) || mutation_probability < 0.0f || mutation_probability > 1.0f)
            return "mutation_probability must be in [0, 1] (got " + std::to_string(mutation_probability) + ")";
        return "";
    }
};
inline Solution solve(Context &ctx, const TspProblem &problem, const CSOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    const tl_cs_opts o{(uint32_t)opts.heuristic.epochs, (uint32_t)std::min<size_t>(opts.heuristic.n_nearest, 0xFFFFFFFFu), opts.mutation_probability};
    return detail::solve_swarm(ctx, problem, progress_tx, init_tour, seed, runs, o, tl_cuckoo_search, tl_cuckoo_search_trace, tl_cuckoo_search_population);
}
}  // namespace cuckoo_search

namespace flower_pollination {  // flower_pollination.rs:53-151
// The algorithm is the reference's; its random draws and its Levy step are this project's specification (include/teeline_gpu.h).
// The flower count is max(opts.heuristic.n_nearest, 25).  runs > 1: runs 0 .. runs-1 of the seed at once, the best one returned
// (lowest cost, then lowest run).  With a progress callback the reference's messages — PathUpdate(start gbest), per epoch a
// PathUpdate per gbest improvement in the order they happen and EpochUpdate(epoch), then Done (flower_pollination.rs:113-115,133-136,142-149)
// — are replayed from that run's improvement log.
struct FPAOptions {  // mod.rs:998-1026
    HeuristicOptions heuristic;
    float mutation_probability = 0.001f;
    std::string validate() const
    {
        if (!std::isfinite(mutation_probability) || mutation_probability < 0.0f || mutation_probability > 1.0f)
            return "mutation_probability must be in [0, 1] (got " + std::to_string(mutation_probability) + ")";
        return "";
    }
};
inline Solution solve(Context &ctx, const TspProblem &problem, const FPAOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    const tl_fpa_opts o{(uint32_t)opts.heuristic.epochs, (uint32_t)std::min<size_t>(opts.heuristic.n_nearest, 0xFFFFFFFFu), opts.mutation_probability};
    return detail::solve_swarm(ctx, problem, progress_tx, init_tour, seed, runs, o, tl_flower_pollination, tl_flower_pollination_trace, tl_flower_pollination_population);
}
}  // namespace flower_pollination

namespace gravitational_search {  // gravitational_search.rs:23-145
// The algorithm is the reference's; its random draws, the order among equal masses and its exp are this project's specification
// (include/teeline_gpu.h).  The agent count is max(opts.n_nearest, 25).  runs > 1: runs 0 .. runs-1 of the seed at once, the best one returned (lowest
// cost, then lowest run).  With a progress callback the reference's messages — PathUpdate(start gbest), per epoch a PathUpdate per
// gbest improvement in agent order and EpochUpdate(epoch), then Done (gravitational_search.rs:72-74,127-143) — are replayed from that
// run's improvement log.
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    const tl_gsa_opts o{(uint32_t)opts.epochs, (uint32_t)std::min<size_t>(opts.n_nearest, 0xFFFFFFFFu), 0u};
    return detail::solve_swarm(ctx, problem, progress_tx, init_tour, seed, runs, o, tl_gravitational_search, tl_gravitational_search_trace,
                               tl_gravitational_search_population);
}
}  // namespace gravitational_search

namespace kohonen_som {  // som.rs:12-186
struct SOMOptions {  // mod.rs:1465-1482
    size_t epochs = 100000;
    double learning_rate = 0.8;
    double radius_fraction = 0.1;
    size_t neuron_multiplier = 8;
};
// The algorithm is the reference's; the city drawn in an epoch, exp (with a cut at -8 before it) and the start ring's cos and sin are
// this project's specification (include/teeline_gpu.h).  init_tour is ignored, as the reference ignores it.  runs > 1: runs
// 0 .. runs-1 of the seed at once, the best one returned (lowest cost, then lowest run).  With a progress callback the reference's
// messages — EpochUpdate(t) then PathUpdate(snapshot) at every t % max(epochs / 10, 1) == 0, a final PathUpdate only where
// epochs % checkpoint != 0, then Done (som.rs:117-145; nothing for n < 2) — are replayed from that run's checkpoint records.
inline Solution solve(Context &ctx, const TspProblem &problem, const SOMOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> * /*init_tour*/,
                      uint64_t seed = 1, uint32_t runs = 1)
{
    detail::Call c(problem, nullptr);
    const uint32_t n = c.n;
    const tl_som_opts o{(uint32_t)std::min<size_t>(opts.epochs, 0xFFFFFFFFu), (uint32_t)std::min<size_t>(opts.neuron_multiplier, 0xFFFFFFFFu), opts.learning_rate,
                        opts.radius_fraction, 0u, 0u, 0ull};
    return detail::solve_chains(
        problem, c, progress_tx, runs, false,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *, uint32_t *best) {
            ctx.check(tl_kohonen_som_population(ctx.get(), c.xy.data(), n, c.packed, 0u, count, &o, seed, outs, costs, best, &c.st));
        },
        [&] { ctx.check(tl_kohonen_som(ctx.get(), c.xy.data(), n, c.packed, &o, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t run) {
            const uint32_t cap = 20;
            uint32_t rows = 0;
            std::vector<uint32_t> ep(cap), tours((size_t)cap * std::max(n, 1u)), cb(cap);
            ctx.check(tl_kohonen_som_trace(ctx.get(), c.xy.data(), n, c.packed, &o, seed, run, c.out.data(), &c.cost, &c.st, nullptr, 0u, nullptr, ep.data(), tours.data(),
                                           cb.data(), cap, &rows));
            auto send = detail::route_sender(problem, progress_tx);
            for (uint32_t k = 0; k < rows && k < cap; ++k) {
                if (ep[k] != 0xFFFFFFFFu) (*progress_tx)(ProgressKind::EpochUpdate, std::vector<size_t>{ep[k]}, 0.0f);
                send(tours.data() + (size_t)k * n, detail::bits_to_f32(cb[k]));
            }
        },
        n >= 2);  // (n < 2: the reference sends nothing, Done included)
}
}  // namespace kohonen_som

namespace hill_climb {  // stochastic_hill.rs:7-97
// The chain is the reference's (a candidate is accepted iff it beats the BEST cost; a plateau shuffles the current tour and leaves the
// best alone; epochs + 1 epochs run); its random draws (a pure function of seed, chain, event and slot) are this project's
// specification (include/teeline_gpu.h), and the solver goes by the name `hill_climb`.  init_tour nullptr: city order (the
// reference's own shuffle is the pipeline's shuffle stage).  chains > 1: chains 0 .. chains-1 of the seed at once, the best one
// returned (lowest cost, then lowest chain).  With a progress callback the reference's messages — PathUpdate(start route, 0.0),
// PathUpdate(best, distance) per acceptance, PathUpdate(shuffled current route, 0.0) per restart, then Done
// (stochastic_hill.rs:29-31,51-56,75-77,93-95) — are replayed from the events of that chain (tl_hill_climb_trace_chain), the
// shuffles through tl_hill_draw.  window: epochs evaluated at once (0: the plan's, 1: epoch after epoch); the same result.
inline Solution solve(Context &ctx, const TspProblem &problem, const HeuristicOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      uint64_t seed = 1, uint32_t chains = 1, uint32_t window = 0)
{
    detail::Call c(problem, init_tour);
    const uint32_t n = c.n;
    const tl_hill_opts o{(uint32_t)opts.epochs, (uint32_t)opts.platoo_epochs, window, 0u};
    return detail::solve_chains(
        problem, c, progress_tx, chains, true,
        [&](uint32_t count, uint32_t *outs, float *costs, uint32_t *moves, uint32_t *best) {
            ctx.check(tl_hill_climb_population(ctx.get(), c.xy.data(), n, c.packed, c.ip, c.ip ? 1u : 0u, 0u, count, &o, seed, outs, costs, moves, best, &c.st));
        },
        [&] { ctx.check(tl_hill_climb(ctx.get(), c.xy.data(), n, c.packed, c.ip, &o, seed, c.out.data(), &c.cost, &c.st)); },
        [&](uint32_t chain) {
            std::vector<uint32_t> log;
            const uint32_t len = detail::grow_trace(1u << 14, [&](uint32_t cap, uint32_t *got) {  // room for every event
                log.assign((size_t)cap * 4, 0u);
                ctx.check(tl_hill_climb_trace_chain(ctx.get(), c.xy.data(), n, c.packed, c.ip, &o, seed, chain, c.out.data(), &c.cost, &c.st, log.data(), cap, got));
            });
            auto send = detail::route_sender(problem, progress_tx);
            std::vector<uint32_t> pos = c.start_tour();
            send(pos.data(), 0.0f);
            for (uint32_t m = 0; m < len; ++m) {
                if (log[4 * m + 1] == 0xFFFFFFFFu) {  // a restart: the Fisher-Yates pass of csrc/hill_spec.h on the current contents
                    for (uint32_t j = n - 1u; j >= 1u; --j) {
                        const uint64_t u = tl_hill_draw(seed, chain, (1ull << 58) + (uint64_t)log[4 * m] * n + j, 26u);
                        std::swap(pos[j], pos[(uint32_t)(((u >> 32) * (j + 1u)) >> 32)]);
                    }
                    send(pos.data(), 0.0f);
                } else {
                    std::reverse(pos.begin() + log[4 * m + 1], pos.begin() + log[4 * m + 2] + 1);  // swap_cities (route.rs:102-113)
                    send(pos.data(), detail::bits_to_f32(log[4 * m + 3]));
                }
            }
        });
}
}  // namespace hill_climb

namespace fourier_curve {  // fourier.rs:10-312
struct FourierOptions {  // mod.rs:1341-1352
    size_t k_max = 4;
    size_t m = 200;
    double lambda = 0.05;
    double lambda_decay = 0.5;
    double lr = 0.05;
    size_t epochs = 400;
};
inline tl_fourier_opts c_opts(const FourierOptions &o)
{
    return tl_fourier_opts{(uint32_t)std::min<size_t>(o.k_max, 0xFFFFFFFFu), (uint32_t)std::min<size_t>(o.m, 0xFFFFFFFFu), (uint32_t)std::min<size_t>(o.epochs, 0xFFFFFFFFu),
                           0u, o.lambda, o.lambda_decay, o.lr, 0u, 0u};
}
// The algorithm is the reference's; the basis table, sqrt for hypot, the lowest index among samples at one f32 distance, (2 pi k)^2
// as t t and lambda as the running product are this project's specification (include/teeline_gpu.h).  The solver draws nothing: a
// batch is a list of option sets, all at once, the best kept (lowest cost, then lowest index; *best_job names it).  progress_tx and
// init_tour are ignored, as the reference ignores them.
inline Solution solve_many(Context &ctx, const TspProblem &problem, const std::vector<FourierOptions> &jobs, uint32_t *best_job = nullptr)
{
    if (jobs.empty()) throw std::runtime_error("fourier_curve: no option set");
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size(), J = (uint32_t)jobs.size();
    std::vector<tl_fourier_opts> o;
    for (const FourierOptions &j : jobs) o.push_back(c_opts(j));
    std::vector<uint32_t> outs((size_t)J * std::max(n, 1u)), out(n);
    std::vector<float> costs(J);
    tl_stats st{};
    uint32_t best = 0;
    ctx.check(tl_fourier_curve_batch(ctx.get(), xy.data(), n, problem.explicit_packed(), o.data(), J, outs.data(), costs.data(), nullptr, 0u, &best, &st, nullptr, 0u,
                                     nullptr));
    std::copy(outs.begin() + (size_t)best * n, outs.begin() + (size_t)(best + 1) * n, out.begin());
    if (best_job) *best_job = best;
    return detail::finish(problem, out, costs[best], st, nullptr);
}
inline Solution solve(Context &ctx, const TspProblem &problem, const FourierOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour)
{
    (void)progress_tx;
    (void)init_tour;
    return solve_many(ctx, problem, std::vector<FourierOptions>{opts});
}
}  // namespace fourier_curve

namespace branch_and_bound {  // the depth-first branch and bound of DESIGN.md §4.27 (the bound of branch_bound.rs:240-268, a result of this project's specification)
struct BnbOptions {
    size_t n_nearest = 0;  // K; 0 or >= n: the exact solver.  0 < K < n restricts a city's successors to its K nearest (itself counted): a heuristic
    uint64_t max_nodes = 0;  // budgets, checked between launches (0: none)
    uint32_t time_limit_ms = 0;
    uint32_t nodes_per_launch = 0, frontier_depth = 0, workgroups = 0;  // 0: the plan's; a proved result does not depend on them
};
struct BnbOutcome {
    bool proved = false, improved = false;
    tl_bnb_stats stats{};
};
// The search starts at the smallest id (route.sort(), :35).  init_tour: the start tour, which comes back as given unless a strictly
// shorter tour exists (:84-90).  progress_tx gets the sorted route, the result and Done; the reference's per-move messages are not
// reproduced.  Solution::stats: sweeps = launches, candidates = nodes, moves = leaves.
inline Solution solve(Context &ctx, const TspProblem &problem, const BnbOptions &opts, const ProgressFn *progress_tx, const std::vector<size_t> *init_tour,
                      BnbOutcome *outcome = nullptr)
{
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size();
    std::vector<uint32_t> init, out(n);
    if (init_tour) init = problem.positions_of(*init_tour);
    uint32_t start = 0;
    for (uint32_t p = 1; p < n; ++p)
        if (problem.cities[p].id < problem.cities[start].id) start = p;
    const tl_bnb_opts o{start, (uint32_t)std::min<size_t>(opts.n_nearest, 0xFFFFFFFFu), opts.max_nodes, opts.time_limit_ms, opts.nodes_per_launch, opts.frontier_depth,
                        opts.workgroups};
    float cost = 0.f;
    uint32_t proved = 0, improved = 0;
    tl_bnb_stats bs{};
    ctx.check(tl_branch_and_bound(ctx.get(), xy.data(), problem.explicit_packed(), n, init_tour ? init.data() : nullptr, &o, out.data(), &cost, &proved, &improved, &bs));
    if (outcome) *outcome = BnbOutcome{proved != 0, improved != 0, bs};
    tl_stats st{};
    st.sweeps = bs.launches;
    st.candidates = bs.nodes;
    st.moves = bs.leaves;
    st.kernel_ms = bs.kernel_ms;
    st.total_ms = bs.total_ms;
    Solution s = detail::finish(problem, out, cost, st, nullptr);
    if (progress_tx && *progress_tx) {
        std::vector<size_t> sorted_ids;
        for (auto &c : problem.cities) sorted_ids.push_back(c.id);
        std::sort(sorted_ids.begin(), sorted_ids.end());
        (*progress_tx)(ProgressKind::PathUpdate, sorted_ids, 0.0f);
        (*progress_tx)(ProgressKind::PathUpdate, s.route_, cost);
        (*progress_tx)(ProgressKind::Done, s.route_, cost);
    }
    return s;
}
}  // namespace branch_and_bound

namespace one_tree_bound {  // the Held-Karp lower bound of DESIGN.md §4.29: not a solver and not the reference's (it computes no bound)
struct BoundOptions {
    size_t root = 0, iterations = 1000, patience = 10;
    double lambda0 = 2.0;
};
struct Bound {
    double bound = 0.0, upper = 0.0;
    bool is_tour = false;
    uint32_t job = 0;                   // of a batch: the first job with the largest bound
    std::vector<double> bounds;         // every job's
    std::vector<double> pi;             // the best penalties
    std::vector<size_t> route;          // city ids where the 1-tree was a tour (the bound is then the optimum), else empty
    tl_one_tree_result result{};
    tl_stats stats{};
    double gap_pct(double cost) const { return 100.0 * (cost - bound) / bound; }  // how far above the optimum a tour of this cost can be at most
};
// upper: the length of any tour (it scales the step).  One workgroup per option set, all at once; the best job's figures come back.
inline Bound bound_batch(Context &ctx, const TspProblem &problem, double upper, const std::vector<BoundOptions> &jobs)
{
    if (jobs.empty()) throw std::runtime_error("one_tree_bound: no option set");
    const auto xy = problem.xy();
    const uint32_t n = (uint32_t)problem.cities.size(), J = (uint32_t)jobs.size();
    std::vector<tl_one_tree_opts> o;
    for (const BoundOptions &j : jobs)
        o.push_back(tl_one_tree_opts{(uint32_t)std::min<size_t>(j.root, 0xFFFFFFFFu), (uint32_t)std::min<size_t>(j.iterations, 0xFFFFFFFFu),
                                     (uint32_t)std::min<size_t>(j.patience, 0xFFFFFFFFu), 0u, j.lambda0, upper, 0u});
    std::vector<tl_one_tree_result> res(J);
    std::vector<double> pi((size_t)J * std::max(n, 1u));
    std::vector<uint32_t> tour((size_t)J * std::max(n, 1u));
    Bound b;
    ctx.check(tl_one_tree_bound_batch(ctx.get(), xy.data(), problem.explicit_packed(), n, o.data(), J, res.data(), pi.data(), nullptr, tour.data(), nullptr, 0u, &b.job,
                                      &b.stats));
    b.result = res[b.job];
    b.bound = b.result.bound;
    b.upper = upper;
    b.is_tour = b.result.is_tour != 0u;
    for (const tl_one_tree_result &r : res) b.bounds.push_back(r.bound);
    b.pi.assign(pi.begin() + (size_t)b.job * n, pi.begin() + (size_t)(b.job + 1) * n);
    if (b.is_tour)
        for (uint32_t k = 0; k < n; ++k) b.route.push_back(problem.cities[tour[(size_t)b.job * n + k]].id);
    return b;
}
inline Bound bound(Context &ctx, const TspProblem &problem, double upper, const BoundOptions &opts = BoundOptions{})
{
    return bound_batch(ctx, problem, upper, std::vector<BoundOptions>{opts});
}
}  // namespace one_tree_bound

namespace alpha_candidates {  // alpha-nearness candidate lists of DESIGN.md §4.32 (this project's own specification) and LK on supplied lists
struct Lists {
    uint32_t n = 0, k = 0;            // k: min(asked, n - 1)
    std::vector<uint32_t> rows;       // n x k POSITIONS in (alpha, w, position) order
    std::vector<double> alpha;        // their values
    std::vector<uint32_t> parent;     // the 1-tree they come from
    uint32_t root_nb[2] = {TL_ONE_TREE_NONE, TL_ONE_TREE_NONE};
    tl_stats stats{};
};
// pi: n penalties (usually a one_tree_bound::Bound's) or empty for zero
inline Lists candidates(Context &ctx, const TspProblem &problem, uint32_t k, const std::vector<double> &pi = {}, uint32_t root = 0)
{
    const auto xy = problem.xy();
    Lists L;
    L.n = (uint32_t)problem.cities.size();
    if (!pi.empty() && pi.size() != L.n) throw std::runtime_error("alpha_candidates: pi must hold one penalty per city");
    L.k = std::min(k, L.n ? L.n - 1u : 0u);
    L.rows.resize(std::max<size_t>((size_t)L.n * std::min(L.k, 64u), 1u));
    L.alpha.resize(L.rows.size());
    L.parent.resize(std::max(L.n, 1u));
    ctx.check(tl_alpha_candidates(ctx.get(), xy.data(), problem.explicit_packed(), L.n, pi.empty() ? nullptr : pi.data(), root, k, 0u, L.rows.data(), L.alpha.data(),
                                  L.parent.data(), L.root_nb, &L.stats));
    L.rows.resize((size_t)L.n * L.k);
    L.alpha.resize((size_t)L.n * L.k);
    L.parent.resize(L.n);
    return L;
}
// Every later lin_kernighan call of this context searches these lists (alpha chooses the set, distance orders it: the library puts
// every row into ascending Euclidean distance, stably, before a search reads it); clear() restores the kd-tree's.
inline void set_lk_lists(Context &ctx, const Lists &L) { ctx.check(tl_lk_candidates(ctx.get(), L.rows.data(), L.n, L.k)); }
inline void clear_lk_lists(Context &ctx) { ctx.check(tl_lk_candidates(ctx.get(), nullptr, 0u, 0u)); }
}  // namespace alpha_candidates

// Solvers (mod.rs:47-72) this build accelerates, by the reference's names and aliases (FromStr, mod.rs:559-590)
enum class Solvers { NearestNeighbor, TwoOpt, ThreeOpt, OrOpt, LinKernighan, RandomShuffle, GreedyEdge, Savings, Christofides, BellmanKarp, SimulatedAnnealing, TabuSearch, GeneticAlgorithm, AntColony, ParticleSwarm, CuckooSearch, FlowerPollination, GravitationalSearch, KohonenSom, HillClimb, FourierCurve, BranchAndBound };

inline bool solver_from_str(std::string s, Solvers &out, std::string &why)
{
    for (auto &ch : s) ch = (char)std::tolower((unsigned char)ch);
    if (s == "nn" || s == "nearest_neighbor") out = Solvers::NearestNeighbor;
    else if (s == "2opt" || s == "two_opt") out = Solvers::TwoOpt;
    else if (s == "3opt" || s == "three_opt") out = Solvers::ThreeOpt;
    else if (s == "or_opt" || s == "or-opt" || s == "oropt") out = Solvers::OrOpt;
    else if (s == "lk" || s == "lin_kernighan") out = Solvers::LinKernighan;
    else if (s == "shuffle" || s == "random_shuffle") out = Solvers::RandomShuffle;
    else if (s == "gec" || s == "greedy_edge") out = Solvers::GreedyEdge;
    else if (s == "sav" || s == "savings") out = Solvers::Savings;
    else if (s == "chr" || s == "christofides") out = Solvers::Christofides;
    else if (s == "bhk" || s == "bellman_karp") out = Solvers::BellmanKarp;
    else if (s == "simulated_annealing") out = Solvers::SimulatedAnnealing;  // (the alias `sa` stays refused, below: this build's annealing is a
                                                                              // seeded chain of its own specification, asked for by its long name)
    else if (s == "tabu_search") out = Solvers::TabuSearch;  // (the alias `tabu` stays refused, below, as `sa` does)
    else if (s == "genetic_algorithm") out = Solvers::GeneticAlgorithm;  // (the alias `ga` likewise)
    else if (s == "ant_colony") out = Solvers::AntColony;  // (the alias `aco` likewise)
    else if (s == "particle_swarm") out = Solvers::ParticleSwarm;  // (the alias `pso` likewise)
    else if (s == "cuckoo_search") out = Solvers::CuckooSearch;  // (the alias `cs` likewise)
    else if (s == "flower_pollination") out = Solvers::FlowerPollination;  // (the alias `fpa` likewise)
    else if (s == "gravitational_search") out = Solvers::GravitationalSearch;  // (the alias `gsa` likewise)
    else if (s == "kohonen_som") out = Solvers::KohonenSom;  // (the aliases `som` and `kohonen` likewise)
    else if (s == "hill_climb") out = Solvers::HillClimb;  // (the reference's `stochastic_hill` stays refused, below; `hill` stays unknown)
    else if (s == "fourier_curve") out = Solvers::FourierCurve;  // (the reference's `fourier` stays refused, below)
    else if (s == "branch_and_bound") out = Solvers::BranchAndBound;  // (the reference's `branch_bound` stays refused, below: its result depends on a HashSet's order)
    else {
        static const char *cpu_only[] = {"aco", "branch_bound",
                                         "cs", "fpa", "fourier", "ga", "gsa",
                                         "pso", "sa",
                                         "som", "kohonen", "stochastic_hill", "tabu"};
        for (const char *c : cpu_only)
            if (s == c) {
                why = "solver `" + s + "` is not accelerated by this build (nn, gec, sav, chr, bhk, 2opt, 3opt, or_opt, lk, shuffle are, and simulated_annealing under its long name)";
                if (s == "tabu") why += "; the seeded tabu search of this build is `tabu_search`";
                if (s == "ga") why += "; the seeded genetic algorithm of this build is `genetic_algorithm`";
                if (s == "aco") why += "; the seeded ant colony of this build is `ant_colony`";
                if (s == "pso") why += "; the seeded particle swarm of this build is `particle_swarm`";
                if (s == "cs") why += "; the seeded cuckoo search of this build is `cuckoo_search`";
                if (s == "fpa") why += "; the seeded flower pollination of this build is `flower_pollination`";
                if (s == "gsa") why += "; the seeded gravitational search of this build is `gravitational_search`";
                if (s == "som" || s == "kohonen") why += "; the seeded Kohonen map of this build is `kohonen_som`";
                if (s == "stochastic_hill") why += "; the seeded hill climb of this build is `hill_climb`";
                if (s == "fourier") why += "; the Fourier-curve solver of this build is `fourier_curve`";
                return false;
            }
        why = "unknown solver";  // FromStr's Err (mod.rs:588)
        return false;
    }
    return true;
}

inline const char *solver_name(Solvers s)
{
    switch (s) {
        case Solvers::NearestNeighbor: return "nn";
        case Solvers::TwoOpt: return "2opt";
        case Solvers::ThreeOpt: return "3opt";
        case Solvers::OrOpt: return "or_opt";
        case Solvers::LinKernighan: return "lk";
        case Solvers::GreedyEdge: return "greedy_edge";
        case Solvers::Savings: return "savings";
        case Solvers::Christofides: return "christofides";
        case Solvers::BellmanKarp: return "bellman_karp";
        case Solvers::SimulatedAnnealing: return "simulated_annealing";
        case Solvers::TabuSearch: return "tabu_search";
        case Solvers::GeneticAlgorithm: return "genetic_algorithm";
        case Solvers::AntColony: return "ant_colony";
        case Solvers::ParticleSwarm: return "particle_swarm";
        case Solvers::CuckooSearch: return "cuckoo_search";
        case Solvers::FlowerPollination: return "flower_pollination";
        case Solvers::GravitationalSearch: return "gravitational_search";
        case Solvers::KohonenSom: return "kohonen_som";
        case Solvers::HillClimb: return "hill_climb";
        case Solvers::FourierCurve: return "fourier_curve";
        case Solvers::BranchAndBound: return "branch_and_bound";
        default: return "shuffle";
    }
}

namespace pipeline {  // pipeline.rs
struct StageOptions {
    HeuristicOptions heuristic;
    LKOptions lk;
    int two_opt_mode = TL_MODE_REF_ORDER;
    uint32_t two_opt_runs = 1;  // >= 2: a 2opt stage runs this many seeded restarts (seed) at once and keeps the best; its warm start is not used
    uint32_t lk_runs = 1;  // >= 2: an lk stage that is the LAST stage runs this many seeded runs (seed) at once from its warm start and keeps the best
    simulated_annealing::SAOptions sa;
    uint32_t sa_chains = 1;  // an sa stage runs this many chains and keeps the best
    uint32_t tabu_chains = 1;  // a tabu_search stage likewise
    genetic_algorithm::GAOptions ga;
    uint32_t ga_runs = 1;  // a genetic_algorithm stage breeds this many runs and keeps the best
    ant_colony::AcoOptions aco;
    uint32_t aco_runs = 1;  // an ant_colony stage runs this many colonies and keeps the best
    uint32_t pso_runs = 1;  // a particle_swarm stage runs this many swarms and keeps the best
    float cs_mutation_probability = 0.001f;  // CSOptions::mutation_probability (mod.rs:922)
    uint32_t cs_runs = 1;  // a cuckoo_search stage runs this many runs and keeps the best
    float fpa_mutation_probability = 0.001f;  // FPAOptions::mutation_probability (mod.rs:1007)
    uint32_t fpa_runs = 1;  // a flower_pollination stage runs this many runs and keeps the best
    uint32_t gsa_runs = 1;  // a gravitational_search stage runs this many runs and keeps the best
    kohonen_som::SOMOptions som;
    uint32_t som_runs = 1;  // a kohonen_som stage runs this many runs and keeps the best
    uint32_t hill_chains = 1;  // a hill_climb stage runs this many chains and keeps the best
    fourier_curve::FourierOptions fourier;
    std::vector<fourier_curve::FourierOptions> fourier_jobs;  // not empty: a fourier_curve stage runs these option sets at once and keeps the best
    branch_and_bound::BnbOptions bnb;  // a branch_and_bound stage: exact unless bnb.n_nearest restricts it
    uint64_t seed = 1;  // LK kicks, shuffle, SA, tabu and GA draws
    const ProgressFn *progress = nullptr;  // handed to every stage's solve() (the reference's CLI passes None; teeline-qt a sender)
};
struct StageOutcome {  // :11-14
    Solvers solver;
    Solution solution;
    uint64_t duration_ms = 0;
    double duration_us = 0.0;  // the same interval, finer (the CLI's --timing)
    int64_t best_restart = -1;  // a multi-start 2opt stage: the restart its tour came from
    int64_t best_run = -1;      // an lk stage of several seeded runs: the run its tour came from
};

// stage_warnings (:92-132), for the solvers this build knows
inline std::vector<std::string> stage_warnings(const std::vector<Solvers> &solvers)
{
    std::vector<std::string> w;
    for (size_t i = 0; i < solvers.size(); ++i) {
        if (i > 0) {
            if (solvers[i] == Solvers::NearestNeighbor)
                w.push_back("nn at stage " + std::to_string(i) + " discards the warm-start seed from the previous stage");
            else if (solvers[i] == Solvers::GreedyEdge)
                w.push_back("greedy_edge at stage " + std::to_string(i) +
                            " discards the warm-start seed from the previous stage (it always rebuilds from scratch)");
            else if (solvers[i] == Solvers::Savings)
                w.push_back("savings at stage " + std::to_string(i) +
                            " discards the warm-start seed from the previous stage (it always rebuilds from scratch)");
        }
        if (i + 1 != solvers.size() && solvers[i] == Solvers::BellmanKarp)  // :112-118: an exact stage that is not the last
            w.push_back("BellmanKarp at stage " + std::to_string(i) +
                        " ignores the warm-start seed entirely (the exact DP has no use for a partial/seed tour) and its optimal result will be "
                        "superseded by later stages");
    }
    return w;
}

// run_pipeline_stages (:53-80): stage k+1 is warm-started with stage k's tour; an invalid seed is dropped with a warning,
// an invalid stage result is a hard error
inline std::vector<StageOutcome> run_pipeline_stages(Context &ctx, const TspProblem &problem, const std::vector<Solvers> &stages,
                                                     const StageOptions &o)
{
    if (stages.empty()) throw std::runtime_error("pipeline has no stages");
    std::vector<StageOutcome> out;
    std::vector<size_t> seed;
    bool have_seed = false;
    size_t stage_index = 0;
    for (Solvers s : stages) {
        const bool last_stage = ++stage_index == stages.size();
        if (have_seed && !validate_tour(seed, problem.cities)) {
            std::fprintf(stderr, "warning: pipeline: invalid seed; using default seeding\n");
            have_seed = false;
        }
        const std::vector<size_t> *init = have_seed ? &seed : nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        Solution sol;
        uint32_t best_restart = 0, best_run = 0;
        const bool lk_population = s == Solvers::LinKernighan && last_stage && o.lk_runs >= 2;
        switch (s) {
            case Solvers::NearestNeighbor: sol = nearest_neighbor::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::TwoOpt:
                sol = o.two_opt_runs >= 2 ? two_opt::multistart(ctx, problem, o.two_opt_runs, o.seed, 0, o.two_opt_mode, &best_restart)
                                          : two_opt::solve(ctx, problem, o.heuristic, o.progress, init, o.two_opt_mode);
                break;
            case Solvers::ThreeOpt: sol = three_opt::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::OrOpt: sol = or_opt::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::LinKernighan:
                if (lk_population) {
                    std::vector<std::vector<size_t>> start;
                    if (init) start.push_back(*init);
                    sol = lin_kernighan::solve_population(ctx, problem, o.lk, init ? &start : nullptr, o.seed, o.lk_runs, 0, &best_run)[best_run];
                } else {
                    sol = lin_kernighan::solve(ctx, problem, o.lk, o.progress, init, o.seed);
                }
                break;
            case Solvers::RandomShuffle: sol = random_shuffle::solve(ctx, problem, o.seed); break;
            case Solvers::GreedyEdge: sol = greedy_edge::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::Savings: sol = savings::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::Christofides: sol = christofides::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::BellmanKarp: sol = bellman_karp::solve(ctx, problem, o.heuristic, o.progress, init); break;
            case Solvers::SimulatedAnnealing: sol = simulated_annealing::solve(ctx, problem, o.sa, o.progress, init, o.seed, o.sa_chains); break;
            case Solvers::TabuSearch: sol = tabu_search::solve(ctx, problem, o.heuristic, o.progress, init, o.seed, o.tabu_chains); break;
            case Solvers::GeneticAlgorithm: sol = genetic_algorithm::solve(ctx, problem, o.ga, o.progress, init, o.seed, o.ga_runs); break;
            case Solvers::AntColony: sol = ant_colony::solve(ctx, problem, o.aco, o.progress, init, o.seed, o.aco_runs); break;
            case Solvers::ParticleSwarm: sol = particle_swarm::solve(ctx, problem, o.heuristic, o.progress, init, o.seed, o.pso_runs); break;
            case Solvers::CuckooSearch: sol = cuckoo_search::solve(ctx, problem, cuckoo_search::CSOptions{o.heuristic, o.cs_mutation_probability}, o.progress, init, o.seed, o.cs_runs); break;
            case Solvers::FlowerPollination: sol = flower_pollination::solve(ctx, problem, flower_pollination::FPAOptions{o.heuristic, o.fpa_mutation_probability}, o.progress, init, o.seed, o.fpa_runs); break;
            case Solvers::GravitationalSearch: sol = gravitational_search::solve(ctx, problem, o.heuristic, o.progress, init, o.seed, o.gsa_runs); break;
            case Solvers::KohonenSom: sol = kohonen_som::solve(ctx, problem, o.som, o.progress, init, o.seed, o.som_runs); break;
            case Solvers::HillClimb: sol = hill_climb::solve(ctx, problem, o.heuristic, o.progress, init, o.seed, o.hill_chains); break;
            case Solvers::FourierCurve:
                sol = o.fourier_jobs.empty() ? fourier_curve::solve(ctx, problem, o.fourier, o.progress, init) : fourier_curve::solve_many(ctx, problem, o.fourier_jobs);
                break;
            case Solvers::BranchAndBound: {
                branch_and_bound::BnbOutcome bo;
                sol = branch_and_bound::solve(ctx, problem, o.bnb, o.progress, init, &bo);
                if (!bo.proved)
                    std::fprintf(stderr, "branch_and_bound: proved=0 (the budget ended the search after %llu nodes; the tour is the best found, not a proved optimum)\n",
                                 (unsigned long long)bo.stats.nodes);
                break;
            }
        }
        const auto t1 = std::chrono::steady_clock::now();
        const uint64_t ms = (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count();
        if (!validate_tour(sol.route(), problem.cities))
            throw std::runtime_error(std::string("stage ") + solver_name(s) + " invalid tour");  // :70-71
        seed = sol.route();
        have_seed = true;
        out.push_back(StageOutcome{s, std::move(sol), ms, std::chrono::duration<double, std::micro>(t1 - t0).count(),
                                   s == Solvers::TwoOpt && o.two_opt_runs >= 2 ? (int64_t)best_restart : -1, lk_population ? (int64_t)best_run : -1});
    }
    return out;
}
}  // namespace pipeline

namespace cli {  // teeline-cli/src/main.rs output helpers
// print_solution (main.rs:645-652): "{:.5} {flag}\n", then every id followed by ONE space, then "\n"
inline std::string format_solution(const Solution &tour, bool is_optimized)
{
    char head[64];
    std::snprintf(head, sizeof(head), "%.5f %d\n", tour.total, is_optimized ? 1 : 0);
    std::string s = head;
    for (size_t id : tour.route()) {
        s += std::to_string(id);
        s += ' ';
    }
    s += '\n';
    return s;
}

struct OptimalComparison {  // main.rs:654-658
    float optimal_cost = 0.f, gap_pct = 0.f;
    std::string opt_name;
};

// compute_optimal_comparison (main.rs:660-684): the optimal tour's cost through the same tour_length; false on a dimension mismatch
inline bool compute_optimal_comparison(Context &ctx, float solver_cost, const TspProblem &problem, const opt_tour::OptTour &ot,
                                       OptimalComparison &cmp)
{
    if (ot.dimension != problem.cities.size()) {
        std::fprintf(stderr, "--optimal-tour: dimension mismatch (%zu vs %zu); skipping comparison\n", ot.dimension, problem.cities.size());
        return false;
    }
    // DistanceMatrix::tour_length (distance_matrix.rs:221-233): 0.0 for fewer than 2 cities or an unknown id
    float optimal = 0.f;
    std::unordered_map<size_t, uint32_t> idx;
    for (size_t p = 0; p < problem.cities.size(); ++p) idx[problem.cities[p].id] = (uint32_t)p;
    std::vector<uint32_t> pos;
    bool known = ot.route.size() >= 2;
    for (size_t id : ot.route) {
        auto it = idx.find(id);
        if (it == idx.end()) {
            known = false;
            break;
        }
        pos.push_back(it->second);
    }
    if (known) {
        const auto xy = problem.xy();
        ctx.check(tl_tour_length(ctx.get(), problem.explicit_packed() ? nullptr : xy.data(), problem.explicit_packed(),
                                 (uint32_t)pos.size(), pos.data(), &optimal));
    }
    cmp.optimal_cost = optimal;
    cmp.gap_pct = optimal > 0.0f ? (solver_cost - optimal) / optimal * 100.0f : 0.0f;  // f32 arithmetic, as the reference
    cmp.opt_name = ot.name;
    return true;
}

// print_optimal_comparison (main.rs:686-698), to stderr
inline std::string format_optimal_comparison(float solver_cost, const OptimalComparison &cmp)
{
    char buf[256];
    std::string s = "--- Comparison ---\n";
    std::snprintf(buf, sizeof(buf), "Optimal  : %.5f  (from %s)\n", cmp.optimal_cost, cmp.opt_name.c_str());
    s += buf;
    std::snprintf(buf, sizeof(buf), "Solver   : %.5f\n", solver_cost);
    s += buf;
    if (std::fabs(cmp.gap_pct) < 0.001f) s += "Gap      : 0.00 % (matches optimal)\n";
    else {
        std::snprintf(buf, sizeof(buf), "Gap      : %+.2f %%\n", cmp.gap_pct);
        s += buf;
    }
    return s;
}

// serde_json's rendering of an f32 inside json!(): widened to f64, shortest round-trip decimal, always with a fraction or
// an exponent ("60.0", never "60")
inline std::string json_f32(float v)
{
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), (double)v);
    std::string s(buf, r.ptr);
    if (s.find_first_of(".eE") == std::string::npos) s += ".0";
    return s;
}

// print_solution_json (main.rs:700-712): serde_json::Value prints object keys sorted (BTreeMap: no preserve_order), compact
inline std::string json_f64(double v)
{
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), v);
    std::string s(buf, r.ptr);
    if (s.find_first_of(".eE") == std::string::npos) s += ".0";
    return s;
}

// --lower-bound (not the reference's): the Held-Karp bound and the gap of the tour's cost to it, in percent, as f64
inline std::string format_lower_bound(float solver_cost, const one_tree_bound::Bound &lb)
{
    char buf[160];
    std::snprintf(buf, sizeof(buf), "bound=%.17g\ngap_pct=%.4f\n", lb.bound, lb.gap_pct((double)solver_cost));
    return std::string(buf) + (lb.is_tour ? "proved=1\n" : "");
}

// lb (--lower-bound): adds "bound" and "gap_pct" (f64); beside an optimal comparison, whose "gap_pct" keeps its key, the bound's gap
// is "bound_gap_pct"
// best_run >= 0 (an lk stage of `runs` seeded runs): adds "best_run" and "runs"
inline std::string format_solution_json(const Solution &tour, bool is_optimized, const OptimalComparison *opt, const one_tree_bound::Bound *lb = nullptr,
                                        int64_t best_run = -1, uint32_t runs = 0)
{
    std::string s = "{";
    if (best_run >= 0) s += "\"best_run\":" + std::to_string(best_run) + ",";
    if (lb) s += "\"bound\":" + json_f64(lb->bound) + ",";
    if (lb && opt) s += "\"bound_gap_pct\":" + json_f64(lb->gap_pct((double)tour.total)) + ",";
    s += "\"cost\":" + json_f32(tour.total);
    if (lb && !opt) s += ",\"gap_pct\":" + json_f64(lb->gap_pct((double)tour.total));
    if (opt) s += ",\"gap_pct\":" + json_f32(opt->gap_pct) + ",\"optimal_cost\":" + json_f32(opt->optimal_cost);
    s += std::string(",\"optimized\":") + (is_optimized ? "true" : "false") + ",\"route\":[";
    for (size_t k = 0; k < tour.route().size(); ++k) {
        if (k) s += ',';
        s += std::to_string(tour.route()[k]);
    }
    s += "]";
    if (best_run >= 0) s += ",\"runs\":" + std::to_string(runs);
    s += "}\n";
    return s;
}
}  // namespace cli
}  // namespace tsp
}  // namespace teeline
