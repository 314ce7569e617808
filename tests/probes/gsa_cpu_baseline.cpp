// gsa_cpu_baseline.cpp — the project's gravitational search solver restated for one CPU core, stand-alone (its own main, no
// library): the second oracle beside tests/_gsa_oracle.py and the CPU baseline of scripts/timing_gravitational_search.py.  It does
// what the reference does per move — swap_sequence with its linear search, the full sequence then `take`, the velocity applied in
// order, a full f32 re-sum — in the reference's order (every agent from the state as it stands), with the project's seeded draws,
// stable ranking and fixed exp, whose text (teeline_amd/csrc/gsa_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/gsa_cpu_baseline.cpp -o gsa_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   gsa_cpu_baseline FILE.tsp [--epochs E --seed S --run K --n-nearest N --init FILE --trace --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: agent 0's start, n positions separated by white space.
// Prints "epochs moves improved cost_bits seconds", the best tour, and with --trace one "I epoch agent cost_bits" line per log
// record (the start gbest first, epoch 4294967295) and one "E .." line per epoch: the 3 N + 2 words of
// tl_gravitational_search_trace's epoch row.  --draws prints u(seed, run, event, slot 0) for the events (3 N + i) N + j of N = 25,
// i, j < 5, then the bits of g for the epochs 0 .. 7 of 8 and of 10 000, and exits.
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

#include "gsa_spec.h"

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

static uint64_t bits64(double f)
{
    uint64_t u;
    memcpy(&u, &f, 8);
    return u;
}

static Route shuffled(uint64_t key, uint32_t n, uint32_t agent)
{
    Route r(n);
    std::iota(r.begin(), r.end(), 0u);
    for (uint32_t j = n - 1; j >= 1 && j < n; --j) std::swap(r[j], r[tl::sa_position(tl::ga_draw_key(key, tl::ga_init_event(n, agent, j), tl::kGaSlotShuffle), j + 1)]);
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
        fprintf(stderr, "usage: gsa_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, seed = 1, run = 0, n_nearest = 3;
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
        else if (s == "--init") init_path = v, ++a;
        else {
            fprintf(stderr, "unknown option %s\n", s.c_str());
            return 2;
        }
    }
    const uint64_t key = tl::sa_chain_key(seed, run);
    if (draws) {
        for (uint32_t i = 0; i < 5; ++i)
            for (uint32_t j = 0; j < 5; ++j) printf("%llu\n", (unsigned long long)tl::ga_draw_key(key, tl::gsa_event(3, 25, i, j), tl::kGsaSlotR));
        for (uint32_t total : {8u, 10000u})
            for (uint32_t e = 0; e < 8; ++e) printf("%llu\n", (unsigned long long)bits64(tl::gsa_g(e, total)));
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
    const uint32_t N = tl::gsa_agents((uint32_t)std::min<uint64_t>(n_nearest, 0xFFFFFFFFu));
    if (n > 0xFFFFu || N > tl::kGsaMaxAgents || epochs >= 0xFFFFFFFFull) {
        fprintf(stderr, "outside the specification's range\n");
        return 1;
    }
    const uint32_t kb = tl::gsa_kbest(N), v_max = tl::pso_vmax(n);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Route> pos(N);
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
            pos[i] = r;
            continue;
        }
        pos[i] = shuffled(key, n, i);
    }
    std::vector<float> costs(N);
    for (uint32_t i = 0; i < N; ++i) costs[i] = tour_length(xy, pos[i]);
    uint32_t b = 0;
    for (uint32_t i = 1; i < N; ++i)
        if (costs[i] < costs[b]) b = i;  // min_by: the first of equal minima
    Route gbest = pos[b];
    float gbest_cost = costs[b];
    uint64_t improved = 0;
    std::vector<uint32_t> log, elog;
    if (trace) log.insert(log.end(), {0xFFFFFFFFu, b, bits(gbest_cost)});
    std::vector<uint32_t> row(3 * (size_t)N + 2), kbest(N);
    std::vector<double> mass(N);
    std::vector<size_t> vel_len(N, 0);  // the reference keeps the velocities; only their lengths are read, by the inertia term
    for (uint64_t e = 0; e < epochs; ++e) {
        const float worst = tl::gsa_worst(costs.data(), N);
        const double sum = tl::gsa_sum_fitness(costs.data(), N, worst);
        for (uint32_t a = 0; a < N; ++a) {
            mass[a] = tl::gsa_mass(costs[a], worst, sum, N);
            if (mass[a] != mass[a]) {
                fprintf(stderr, "a mass is NaN: the reference panics\n");
                return 3;
            }
        }
        for (uint32_t a = 0; a < N; ++a) kbest[tl::gsa_rank(mass.data(), N, a)] = a;
        const double g = tl::gsa_g((uint32_t)e, (uint32_t)epochs);
        row[3 * (size_t)N] = (uint32_t)bits64(g);
        row[3 * (size_t)N + 1] = (uint32_t)(bits64(g) >> 32);
        for (uint32_t i = 0; i < N; ++i) {
            Swaps vel;  // trim_velocity(old, round(INERTIA_W len)): nothing
            if (tl::gsa_inertia_keep((uint32_t)vel_len[i]) != 0u) return 4;
            uint32_t live = 0;
            for (uint32_t rk = 0; rk < kb; ++rk) {
                const uint32_t j = kbest[rk];
                if (j == i) continue;
                const uint32_t m = tl::gsa_pull_swaps(tl::gsa_r(key, (uint32_t)e, N, i, j), g, mass[j]);
                if (m == 0u) continue;
                ++live;
                const Swaps pull = swap_sequence(pos[i], pos[j]);  // the full sequence, then `take`
                vel.insert(vel.end(), pull.begin(), pull.begin() + std::min<size_t>(m, pull.size()));
            }
            if (vel.size() > v_max) vel.resize(v_max);
            for (const auto &s : vel) std::swap(pos[i][s.first], pos[i][s.second]);
            vel_len[i] = vel.size();
            costs[i] = tour_length(xy, pos[i]);
            row[i] = bits(costs[i]);
            row[N + i] = (uint32_t)vel.size();
            row[2 * (size_t)N + i] = live;
            if (costs[i] < gbest_cost) {
                gbest = pos[i];
                gbest_cost = costs[i];
                ++improved;
                if (trace) log.insert(log.end(), {(uint32_t)e, i, bits(gbest_cost)});
            }
        }
        if (trace) elog.insert(elog.end(), row.begin(), row.end());
    }
    const float cost = tour_length(xy, gbest);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %u %.6f\n", (unsigned long long)epochs, (unsigned long long)(epochs * N), (unsigned long long)improved, bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", gbest[i], i + 1 == n ? '\n' : ' ');
    if (n == 0) printf("\n");
    for (size_t k = 0; k + 2 < log.size(); k += 3) printf("I %u %u %u\n", log[k], log[k + 1], log[k + 2]);
    for (size_t k = 0; k < elog.size(); k += row.size()) {
        printf("E");
        for (size_t j = 0; j < row.size(); ++j) printf(" %u", elog[k + j]);
        printf("\n");
    }
    return 0;
}
