// aco_cpu_baseline.cpp — the project's ant colony solver restated for one CPU core, stand-alone (its own main, no library): the second
// oracle beside tests/_aco_oracle.py and the CPU baseline of scripts/timing_ant_colony.py.  It does what the reference does — the
// distance matrix up front, per step two compacted candidate lists, a sum and a roulette walk over them, per epoch a power per cell,
// evaporation and the deposits in ant order — with the project's seeded draws and power function, whose text
// (teeline_amd/csrc/aco_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/aco_cpu_baseline.cpp -o aco_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   aco_cpu_baseline FILE.tsp [--epochs E --seed S --run K --alpha A --beta B --evaporation-rate R --num-ants N --init FILE --trace]
//   aco_cpu_baseline x --draws [--seed S --run K]        u(seed, run, event, slot) for the events 0 .. 7 and 2^58 .. 2^58 + 7, slot < 28
//   aco_cpu_baseline x --pow XBITS ABITS [XBITS ABITS ..] the bits of aco_pow for pairs of f32 bit patterns
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: the initial tour, n positions separated by white space (default:
// none, a shuffle).  Prints "epochs tours improved fallbacks cost_bits seconds", the best tour, and with --trace one line per epoch
// (every ant's cost bits, then start cities, then fallback counts) followed by one "R epoch ant cost_bits tour.." line per route row.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "aco_spec.h"

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static float dist(const std::vector<float> &xy, uint32_t a, uint32_t b)
{
    const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
    volatile float xx = dx * dx, yy = dy * dy;
    return std::sqrt(xx + yy);
}

struct Dm {
    uint32_t n;
    std::vector<float> d;
    float operator()(uint32_t a, uint32_t b) const { return d[(size_t)a * n + b]; }
};

static float tour_length(const Dm &d, const std::vector<uint32_t> &t)
{
    const size_t n = t.size();
    if (n < 2) return 0.0f;
    float tot = d(t[n - 1], t[0]);
    for (size_t k = 0; k + 1 < n; ++k) tot += d(t[k], t[k + 1]);
    return tot;
}

typedef std::vector<std::pair<uint32_t, float>> Cands;

static uint32_t roulette_select(const Cands &w, float sum, float r)  // probability.rs:69-79
{
    const float target = r * sum;
    float acc = 0.0f;
    for (const auto &c : w) {
        acc += c.second;
        if (acc > target) return c.first;
    }
    return w.back().first;
}

static uint32_t select_next(const Cands &primary, const Cands &fallback, float r1, float r2, uint32_t *path)  // ant_colony.rs:65-78
{
    float s1 = 0.0f;
    for (const auto &c : primary) s1 += c.second;
    *path = 0;
    if (s1 > 0.0f && std::isfinite(s1)) return roulette_select(primary, s1, r1);
    float s2 = 0.0f;
    for (const auto &c : fallback) s2 += c.second;
    *path = 1;
    if (s2 > 0.0f && std::isfinite(s2)) return roulette_select(fallback, s2, r2);
    *path = 2;
    return fallback.front().first;
}

static void deposit_tour(std::vector<float> &tau, uint32_t n, const std::vector<uint32_t> &t, float cost)  // ant_colony.rs:43-53
{
    if (t.size() < 2 || cost <= 0.0f) return;
    const float amount = 1.0f / cost;
    auto edge = [&](uint32_t u, uint32_t v) {
        tau[(size_t)u * n + v] += amount;
        tau[(size_t)v * n + u] += amount;
    };
    edge(t.back(), t[0]);
    for (size_t k = 0; k + 1 < t.size(); ++k) edge(t[k], t[k + 1]);
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: aco_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 150, seed = 1, run = 0, num_ants = 25;
    float alpha = 1.0f, beta = 2.0f, rate = 0.5f;
    bool trace = false, draws = false;
    std::string init_path;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const char *v = a + 1 < argc ? argv[a + 1] : "";
        if (s == "--trace") trace = true;
        else if (s == "--draws") draws = true;
        else if (s == "--pow") {
            for (int k = a + 1; k + 1 < argc; k += 2)
                printf("%u\n", bits(tl::aco_pow(from_bits((uint32_t)strtoul(argv[k], nullptr, 10)), from_bits((uint32_t)strtoul(argv[k + 1], nullptr, 10)))));
            return 0;
        } else if (s == "--epochs") epochs = strtoull(v, nullptr, 10), ++a;
        else if (s == "--seed") seed = strtoull(v, nullptr, 10), ++a;
        else if (s == "--run") run = strtoull(v, nullptr, 10), ++a;
        else if (s == "--num-ants") num_ants = strtoull(v, nullptr, 10), ++a;
        else if (s == "--alpha") alpha = strtof(v, nullptr), ++a;
        else if (s == "--beta") beta = strtof(v, nullptr), ++a;
        else if (s == "--evaporation-rate") rate = strtof(v, nullptr), ++a;
        else if (s == "--init") init_path = v, ++a;
        else {
            fprintf(stderr, "unknown option %s\n", s.c_str());
            return 2;
        }
    }
    const uint64_t key = tl::sa_chain_key(seed, run);
    if (draws) {
        for (uint64_t base : {0ull, (unsigned long long)tl::kGaInitEvent})
            for (uint64_t e = 0; e < 8; ++e)
                for (uint32_t s = 0; s < 28; ++s) printf("%llu\n", (unsigned long long)tl::ga_draw_key(key, base + e, s));
        return 0;
    }
    std::vector<float> xy;
    {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            perror(argv[1]);
            return 1;
        }
        char line[512];
        bool on = false;
        while (fgets(line, sizeof line, f)) {
            if (!on) {
                on = strncmp(line, "NODE_COORD_SECTION", 18) == 0;
                continue;
            }
            int id;
            float x, y;
            if (sscanf(line, "%d %f %f", &id, &x, &y) != 3) break;
            xy.push_back(x);
            xy.push_back(y);
        }
        fclose(f);
    }
    const uint32_t n = (uint32_t)(xy.size() / 2), A = (uint32_t)num_ants;
    const auto t0 = std::chrono::steady_clock::now();
    Dm d{n, std::vector<float>((size_t)n * n)};
    for (uint32_t u = 0; u < n; ++u)
        for (uint32_t v = 0; v < n; ++v) d.d[(size_t)u * n + v] = dist(xy, u, v);
    std::vector<uint32_t> best(n);
    std::iota(best.begin(), best.end(), 0u);
    uint64_t improved = 0, fallbacks = 0, tours = 0;
    std::vector<std::string> lines;
    auto route_line = [&](long long g, long long a, float cost, const std::vector<uint32_t> &t) {
        std::string s = "R " + std::to_string(g) + " " + std::to_string(a) + " " + std::to_string(bits(cost));
        for (uint32_t c : t) s += " " + std::to_string(c);
        lines.push_back(s);
    };
    if (n > 2) {
        const bool seeded = !init_path.empty();
        if (seeded) {
            FILE *f = fopen(init_path.c_str(), "r");
            if (!f) {
                perror(init_path.c_str());
                return 1;
            }
            std::vector<bool> seen(n, false);
            for (uint32_t i = 0; i < n; ++i) {
                unsigned v;
                if (fscanf(f, "%u", &v) != 1 || v >= n || seen[v]) {
                    fprintf(stderr, "%s: not a permutation of 0..n-1\n", init_path.c_str());
                    fclose(f);
                    return 1;
                }
                seen[v] = true;
                best[i] = v;
            }
            fclose(f);
        } else {
            for (uint32_t j = n - 1; j >= 1; --j) std::swap(best[j], best[tl::sa_position(tl::ga_draw_key(key, tl::aco_shuffle_event(j), tl::kGaSlotShuffle), j + 1)]);
        }
        float best_cost = tour_length(d, best);
        if (trace) route_line(-1, -1, best_cost, best);
        const float tau0 = seeded && best_cost > 0.0f ? (float)A / best_cost : 1.0f;
        const float tau_min = tau0 * tl::kAcoTauMinRatio;
        std::vector<float> tau((size_t)n * n, tau0), eta((size_t)n * n, 0.0f), tau_alpha((size_t)n * n);
        for (uint32_t u = 0; u < n; ++u)
            for (uint32_t v = 0; v < n; ++v)
                if (u != v) eta[(size_t)u * n + v] = tl::aco_eta(d(u, v), beta);
        if (seeded) deposit_tour(tau, n, best, best_cost);
        std::vector<std::vector<uint32_t>> ant_tour(A);
        std::vector<float> ant_cost(A);
        std::vector<uint32_t> ant_start(A), ant_fb(A);
        Cands primary, fallback;
        for (uint64_t g = 0; g < epochs; ++g) {
            for (size_t i = 0; i < tau.size(); ++i) tau_alpha[i] = tl::aco_pow(tau[i], alpha);
            for (uint32_t a = 0; a < A; ++a) {
                const uint64_t ev0 = tl::aco_event((uint32_t)g, A, a, n, 0);
                uint32_t cur = tl::sa_position(tl::ga_draw_key(key, ev0, tl::kAcoSlotStart), n), fb = 0;
                std::vector<bool> visited(n, false);
                visited[cur] = true;
                std::vector<uint32_t> tour{cur};
                ant_start[a] = cur;
                for (uint32_t s = 1; s < n; ++s) {
                    primary.clear();
                    fallback.clear();
                    for (uint32_t v = 0; v < n; ++v) {
                        if (visited[v]) continue;
                        const float e = eta[(size_t)cur * n + v];
                        primary.push_back({v, tau_alpha[(size_t)cur * n + v] * e});
                        fallback.push_back({v, e});
                    }
                    const float r1 = tl::ga_uniform(tl::ga_draw_key(key, ev0 + s, tl::kAcoSlotR1)), r2 = tl::ga_uniform(tl::ga_draw_key(key, ev0 + s, tl::kAcoSlotR2));
                    uint32_t path;
                    const uint32_t next = select_next(primary, fallback, r1, r2, &path);
                    fb += path != 0;
                    visited[next] = true;
                    tour.push_back(next);
                    cur = next;
                }
                const float cost = tour_length(d, tour);
                if (cost < best_cost) {
                    best = tour;
                    best_cost = cost;
                    ++improved;
                    if (trace) route_line((long long)g, a, cost, tour);
                }
                ant_tour[a] = std::move(tour);
                ant_cost[a] = cost;
                ant_fb[a] = fb;
                fallbacks += fb;
                ++tours;
            }
            const float keep = 1.0f - rate;
            for (float &t : tau) {  // evaporate_and_floor
                t *= keep;
                if (t < tau_min) t = tau_min;
            }
            for (uint32_t a = 0; a < A; ++a) deposit_tour(tau, n, ant_tour[a], ant_cost[a]);
            if (trace) {
                std::string s = "E";
                for (uint32_t a = 0; a < A; ++a) s += " " + std::to_string(bits(ant_cost[a]));
                for (uint32_t a = 0; a < A; ++a) s += " " + std::to_string(ant_start[a]);
                for (uint32_t a = 0; a < A; ++a) s += " " + std::to_string(ant_fb[a]);
                lines.push_back(s);
            }
        }
    }
    const float cost = tour_length(d, best);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %llu %u %.6f\n", (unsigned long long)epochs, (unsigned long long)tours, (unsigned long long)improved, (unsigned long long)fallbacks,
           bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", best[i], i + 1 == n ? '\n' : ' ');
    if (n == 0) printf("\n");
    for (const auto &s : lines) printf("%s\n", s.c_str());
    return 0;
}
