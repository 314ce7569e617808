// ga_cpu_baseline.cpp — the project's genetic algorithm restated for one CPU core, stand-alone (its own main, no library): the second
// oracle beside tests/_ga_oracle.py and the CPU baseline of scripts/timing_genetic.py.  It does what the reference does per
// generation — a stable sort, a linear roulette walk per parent, a hash set per crossover segment, a full f32 re-sum per child —
// with the project's seeded draws, whose text (teeline_amd/csrc/ga_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/ga_cpu_baseline.cpp -o ga_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   ga_cpu_baseline FILE.tsp [--epochs E --seed S --run K --mutation-probability P --n-elite N --init FILE --trace --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: the initial tour, n positions separated by white space (default:
// none, n shuffles).  Prints "generations children mutations improved cost_bits seconds", the best tour, and with --trace one
// "best_index fitness_bits cost_bits length" line per generation.  --draws prints u(seed, run, event, slot) for the events
// 0 .. 7 and 2^58 .. 2^58 + 7, slot < 28, and exits.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_set>
#include <vector>

#include "ga_spec.h"

static float dist(const std::vector<float> &xy, uint32_t a, uint32_t b)
{
    const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
    volatile float xx = dx * dx, yy = dy * dy;
    return std::sqrt(xx + yy);
}

static float tour_length(const std::vector<float> &xy, const std::vector<uint32_t> &t)
{
    const size_t n = t.size();
    if (n < 2) return 0.0f;
    float tot = dist(xy, t[n - 1], t[0]);
    for (size_t k = 0; k + 1 < n; ++k) tot += dist(xy, t[k], t[k + 1]);
    return tot;
}

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

struct Genotype {
    float fitness;
    std::vector<uint32_t> route;
};

static float fitness_of(const std::vector<float> &xy, const std::vector<uint32_t> &r)
{
    const float len = tour_length(xy, r);
    return len == 0.0f ? 0.0f : 1.0f / len;
}

static void reverse(std::vector<uint32_t> &r, uint32_t from, uint32_t to)
{
    while (from < to) std::swap(r[from++], r[to--]);
}

static size_t best_of(const std::vector<Genotype> &pop)  // max_by: the last of equal maxima
{
    size_t b = 0;
    for (size_t i = 1; i < pop.size(); ++i)
        if (pop[i].fitness >= pop[b].fitness) b = i;
    return b;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: ga_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, seed = 1, run = 0, n_elite = 3;
    float p_mut = 0.001f;
    bool trace = false, draws = false;
    std::string init_path;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const char *v = a + 1 < argc ? argv[a + 1] : "";
        if (s == "--trace") trace = true;
        else if (s == "--draws") draws = true;
        else if (s == "--epochs") epochs = strtoull(v, nullptr, 10), ++a;
        else if (s == "--seed") seed = strtoull(v, nullptr, 10), ++a;
        else if (s == "--run") run = strtoull(v, nullptr, 10), ++a;
        else if (s == "--n-elite") n_elite = strtoull(v, nullptr, 10), ++a;
        else if (s == "--mutation-probability") p_mut = strtof(v, nullptr), ++a;
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
    const uint32_t n = (uint32_t)(xy.size() / 2);
    if (n == 0) {
        fprintf(stderr, "best() of an empty population\n");
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    // the start population (genetic_algorithm.rs:193-237)
    std::vector<Genotype> pop;
    uint32_t n_seeded = 0;
    if (!init_path.empty()) {
        FILE *f = fopen(init_path.c_str(), "r");
        if (!f) {
            perror(init_path.c_str());
            return 1;
        }
        std::vector<uint32_t> start(n);
        std::vector<bool> seen(n, false);
        for (uint32_t i = 0; i < n; ++i) {
            unsigned v;
            if (fscanf(f, "%u", &v) != 1 || v >= n || seen[v]) {
                fprintf(stderr, "%s: not a permutation of 0..n-1\n", init_path.c_str());
                fclose(f);
                return 1;
            }
            seen[v] = true;
            start[i] = v;
        }
        fclose(f);
        n_seeded = std::max(n / 5u, 1u);
        pop.push_back({fitness_of(xy, start), start});
        for (uint32_t i = 1; i < n_seeded; ++i) {
            std::vector<uint32_t> r = start;
            const uint32_t m_count = 2u + tl::sa_position(tl::ga_draw_key(key, tl::ga_init_event(n, i, 0), tl::kGaSlotCount), 3);
            for (uint32_t m = 0; m < m_count; ++m) {
                uint32_t from, to;
                tl::ga_pair(key, tl::ga_init_event(n, i, 1 + m), n, &from, &to);
                reverse(r, from, to);
            }
            pop.push_back({fitness_of(xy, r), r});
        }
    }
    for (uint32_t i = n_seeded; i < n; ++i) {
        std::vector<uint32_t> r(n);
        std::iota(r.begin(), r.end(), 0u);
        for (uint32_t j = n - 1; j >= 1; --j) std::swap(r[j], r[tl::sa_position(tl::ga_draw_key(key, tl::ga_init_event(n, i, j), tl::kGaSlotShuffle), j + 1)]);
        pop.push_back({fitness_of(xy, r), r});
    }

    uint64_t children = 0, mutations = 0, improved = 0;
    std::vector<uint32_t> log;
    const uint32_t pairs = tl::ga_pairs(n, (uint32_t)std::min<uint64_t>(n_elite, 0xFFFFFFFFu));
    for (uint64_t g = 0; g < epochs; ++g) {
        const float before = pop[best_of(pop)].fitness;
        std::stable_sort(pop.begin(), pop.end(), [](const Genotype &x, const Genotype &y) { return x.fitness > y.fitness; });
        std::vector<Genotype> next;
        next.reserve(n);
        for (size_t i = 0; i < pop.size() && i < n_elite; ++i) next.push_back(pop[i]);
        for (uint32_t p = 0; p < pairs; ++p) {
            float total = 0.0f;
            for (const auto &x : pop) total += x.fitness;
            if (!(total > 0.0f) || !std::isfinite(total)) {
                fprintf(stderr, "empty range in random_selection\n");
                return 1;
            }
            const uint64_t ev = tl::ga_pair_event((uint32_t)g, n, p, 0);
            const Genotype *parent[2];
            for (uint32_t k = 0; k < 2; ++k) {
                const float r = tl::ga_uniform(tl::ga_draw_key(key, ev, tl::kGaSlotSelect + k)) * total;
                float up_to = 0.0f;
                parent[k] = &pop.back();
                for (const auto &x : pop) {
                    if (r < up_to + x.fitness) {
                        parent[k] = &x;
                        break;
                    }
                    up_to += x.fitness;
                }
            }
            uint32_t from, to;
            tl::ga_pair(key, ev, n, &from, &to);
            const std::vector<uint32_t> &p1 = parent[0]->route, &p2 = parent[1]->route;
            std::vector<uint32_t> gene[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
            const std::unordered_set<uint32_t> range_a(p1.begin() + from, p1.begin() + to + 1), range_b(p2.begin() + from, p2.begin() + to + 1);
            std::copy(p2.begin() + from, p2.begin() + to + 1, gene[0].begin() + from);
            std::copy(p1.begin() + from, p1.begin() + to + 1, gene[1].begin() + from);
            uint32_t k = (to + 1) % n, j1 = k, j2 = k;
            for (uint32_t it = 0; it < n; ++it) {
                if (!range_b.count(p1[k])) {
                    gene[0][j1] = p1[k];
                    j1 = (j1 + 1) % n;
                }
                if (!range_a.count(p2[k])) {
                    gene[1][j2] = p2[k];
                    j2 = (j2 + 1) % n;
                }
                k = (k + 1) % n;
            }
            for (uint32_t c = 0; c < 2; ++c) {
                Genotype child{fitness_of(xy, gene[c]), std::move(gene[c])};
                if (p_mut > tl::ga_uniform(tl::ga_draw_key(key, ev, tl::kGaSlotMutate + c))) {  // the fitness stays as it was
                    uint32_t mf, mt;
                    tl::ga_pair(key, tl::ga_pair_event((uint32_t)g, n, p, 1 + c), n, &mf, &mt);
                    reverse(child.route, mf, mt);
                    ++mutations;
                }
                if (next.size() < n) next.push_back(std::move(child));
                ++children;
            }
        }
        if (next.empty()) {
            fprintf(stderr, "best() of an empty population\n");
            return 1;
        }
        pop.swap(next);
        const size_t b = best_of(pop);
        improved += pop[b].fitness > before;
        if (trace) {
            log.push_back((uint32_t)b);
            log.push_back(bits(pop[b].fitness));
            log.push_back(bits(tour_length(xy, pop[b].route)));
            log.push_back((uint32_t)pop.size());
        }
    }
    const size_t b = best_of(pop);
    const float cost = tour_length(xy, pop[b].route);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %llu %u %.6f\n", (unsigned long long)epochs, (unsigned long long)children, (unsigned long long)mutations, (unsigned long long)improved,
           bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", pop[b].route[i], i + 1 == n ? '\n' : ' ');
    for (size_t k = 0; k + 3 < log.size(); k += 4) printf("%u %u %u %u\n", log[k], log[k + 1], log[k + 2], log[k + 3]);
    return 0;
}
