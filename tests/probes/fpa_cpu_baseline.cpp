// fpa_cpu_baseline.cpp — the project's flower pollination solver restated for one CPU core, stand-alone (its own main, no
// library): the second oracle beside tests/_fpa_oracle.py and the CPU baseline of scripts/timing_flower_pollination.py.  It does
// what the reference does per move — swap_sequence with its linear search, the prefix applied in order, a full f32 re-sum — in
// the reference's order (every flower from the state as it stands), with the project's seeded draws and Lévy step, whose text
// (teeline_amd/csrc/fpa_spec.h, levy_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/fpa_cpu_baseline.cpp -o fpa_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   fpa_cpu_baseline FILE.tsp [--epochs E --seed S --run K --n-nearest N --mutation-probability P --init FILE --trace --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: flower 0's start, n positions separated by white space.
// Prints "epochs moves improved cost_bits seconds", the best tour, and with --trace one "I epoch flower cost_bits" line per log
// record (the start gbest first, epoch 4294967295) and one "E .." line per epoch: the 4 N words of tl_flower_pollination_trace's
// epoch row.  --draws prints u(seed, run, event, slot) for the events 0 .. 7 and 2^58 .. 2^58 + 7, slot < 28, then for the
// flowers of epoch 3 at N = 25, 26 and 64 their j and k, and exits.
#include <algorithm>
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

#include "fpa_spec.h"

typedef std::vector<uint32_t> Route;
typedef std::vector<std::pair<uint32_t, uint32_t>> Swaps;

static float dist(const std::vector<float> &xy, uint32_t a, uint32_t b)
{
    const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
    volatile float xx = dx * dx, yy = dy * dy;
    return std::sqrt(xx + yy);
}

static float tour_length(const std::vector<float> &xy, const Route &t)
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

static Route shuffled(uint64_t key, uint32_t n, uint32_t flower)
{
    Route r(n);
    std::iota(r.begin(), r.end(), 0u);
    for (uint32_t j = n - 1; j >= 1 && j < n; --j) std::swap(r[j], r[tl::sa_position(tl::ga_draw_key(key, tl::ga_init_event(n, flower, j), tl::kGaSlotShuffle), j + 1)]);
    return r;
}

// route.rs:118-134: a linear search from i + 1 on
static Swaps swap_sequence(const Route &from, const Route &to)
{
    Route tmp = from;
    Swaps seq;
    for (size_t i = 0; i + 1 < tmp.size(); ++i) {
        if (tmp[i] == to[i]) continue;
        size_t j = i + 1;
        while (j < tmp.size() && tmp[j] != to[i]) ++j;
        if (j == tmp.size()) {
            fprintf(stderr, "swap_sequence: not permutations of the same elements\n");
            exit(1);
        }
        seq.emplace_back((uint32_t)i, (uint32_t)j);
        std::swap(tmp[i], tmp[j]);
    }
    return seq;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: fpa_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, seed = 1, run = 0, n_nearest = 3;
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
        else if (s == "--n-nearest") n_nearest = strtoull(v, nullptr, 10), ++a;
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
        for (uint32_t N : {25u, 26u, 64u})
            for (uint32_t i = 0; i < N; ++i) {
                uint32_t j, k;
                tl::fpa_partners(key, tl::fpa_event(3, N, i), i, N, &j, &k);
                printf("%u %u\n", j, k);
            }
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
    const uint32_t N = tl::fpa_flowers((uint32_t)std::min<uint64_t>(n_nearest, 0xFFFFFFFFu));
    const double switch_prob = tl::fpa_switch_prob(p_mut);
    if (n > 0xFFFFu || N > tl::kFpaMaxFlowers || epochs >= 0xFFFFFFFFull || !(p_mut >= 0.0f && p_mut <= 1.0f)) {
        fprintf(stderr, "outside the specification's range\n");
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Route> flower(N);
    for (uint32_t i = 0; i < N; ++i) {
        if (i == 0 && !init_path.empty()) {
            FILE *f = fopen(init_path.c_str(), "r");
            if (!f) {
                perror(init_path.c_str());
                return 1;
            }
            Route r(n);
            std::vector<bool> seen(n, false);
            for (uint32_t k = 0; k < n; ++k) {
                unsigned v;
                if (fscanf(f, "%u", &v) != 1 || v >= n || seen[v]) {
                    fprintf(stderr, "%s: not a permutation of 0..n-1\n", init_path.c_str());
                    fclose(f);
                    return 1;
                }
                seen[v] = true;
                r[k] = v;
            }
            fclose(f);
            flower[i] = r;
            continue;
        }
        flower[i] = shuffled(key, n, i);
    }
    std::vector<float> costs(N);
    for (uint32_t i = 0; i < N; ++i) costs[i] = tour_length(xy, flower[i]);
    uint32_t b = 0;
    for (uint32_t i = 1; i < N; ++i)
        if (costs[i] < costs[b]) b = i;  // min_by: the first of equal minima
    Route gbest = flower[b];
    float gbest_cost = costs[b];
    uint64_t improved = 0;
    std::vector<uint32_t> log, elog;
    if (trace) log.insert(log.end(), {0xFFFFFFFFu, b, bits(gbest_cost)});
    std::vector<uint32_t> row(4 * (size_t)N);
    std::vector<char> accepted(N);
    for (uint64_t e = 0; e < epochs; ++e) {
        std::fill(accepted.begin(), accepted.end(), 0);
        bool changed = false;
        for (uint32_t i = 0; i < N; ++i) {
            const uint64_t ev = tl::fpa_event((uint32_t)e, N, i);
            const bool global = tl::fpa_is_global(key, ev, switch_prob);
            uint32_t j = 0, k = 0, m = 0;
            Swaps seq;
            bool again;
            if (global) {
                seq = swap_sequence(flower[i], gbest);
                if (!seq.empty()) m = tl::fpa_global_swaps(tl::fpa_levy(key, ev), (uint32_t)seq.size());
                again = changed;
            } else {
                tl::fpa_partners(key, ev, i, N, &j, &k);
                seq = swap_sequence(flower[j], flower[k]);
                if (!seq.empty()) m = tl::fpa_local_swaps(tl::fpa_epsilon(key, ev), (uint32_t)seq.size());
                again = accepted[j] || accepted[k];
            }
            Route nw = flower[i];
            for (uint32_t t = 0; t < m; ++t) std::swap(nw[seq[t].first], nw[seq[t].second]);
            const float cost = tour_length(xy, nw);
            const bool acc = cost < costs[i];
            row[N + i] = tl::fpa_kind_word(global, j, k);
            row[2 * (size_t)N + i] = tl::fpa_length_word((uint32_t)seq.size(), m);
            row[3 * (size_t)N + i] = (acc ? 1u : 0u) | (again ? 2u : 0u);
            if (acc) {
                flower[i] = nw;
                costs[i] = cost;
                accepted[i] = 1;
                if (cost < gbest_cost) {
                    gbest = flower[i];
                    gbest_cost = cost;
                    changed = true;
                    ++improved;
                    if (trace) log.insert(log.end(), {(uint32_t)e, i, bits(cost)});
                }
            }
        }
        if (trace) {
            for (uint32_t i = 0; i < N; ++i) row[i] = bits(costs[i]);
            elog.insert(elog.end(), row.begin(), row.end());
        }
    }
    const float cost = tour_length(xy, gbest);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %u %.6f\n", (unsigned long long)epochs, (unsigned long long)(epochs * N), (unsigned long long)improved, bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", gbest[i], i + 1 == n ? '\n' : ' ');
    if (n == 0) printf("\n");
    for (size_t k = 0; k + 2 < log.size(); k += 3) printf("I %u %u %u\n", log[k], log[k + 1], log[k + 2]);
    for (size_t k = 0; k < elog.size(); k += 4 * (size_t)N) {
        printf("E");
        for (size_t j = 0; j < 4 * (size_t)N; ++j) printf(" %u", elog[k + j]);
        printf("\n");
    }
    return 0;
}
