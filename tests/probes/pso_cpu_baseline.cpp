// pso_cpu_baseline.cpp — the project's particle swarm solver restated for one CPU core, stand-alone (its own main, no library): the
// second oracle beside tests/_pso_oracle.py and the CPU baseline of scripts/timing_particle_swarm.py.  It does what the reference
// does per particle step — two swap sequences, each finding its cities by a LINEAR search, the swaps applied in order, a full f32
// re-sum — with the project's seeded draws and rounding, whose text (teeline_amd/csrc/pso_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/pso_cpu_baseline.cpp -o pso_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   pso_cpu_baseline FILE.tsp [--epochs E --seed S --run K --n-nearest N --init FILE --trace --inverse-table --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: particle 0's start, n positions separated by white space.
// --inverse-table: the swap sequence with a table of where every city is instead of the search (the same pairs in O(n); NOT what
// the reference does — timed under its own label).  Prints "epochs steps improved cost_bits seconds", the best tour, and with
// --trace one "I epoch particle cost_bits" line per log record (the start gbest first, epoch 4294967295) and one "E .." line per
// epoch: every particle's cost bits, then every particle's velocity length.  --draws prints u(seed, run, event, slot) for the
// events 0 .. 7 and 2^58 .. 2^58 + 7, slot < 28, then tl_pso_keep and tl_pso_weight vectors, and exits.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "pso_spec.h"

typedef std::vector<uint32_t> Route;
typedef std::vector<std::pair<uint32_t, uint32_t>> Velocity;

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

// swap_sequence (route.rs:118-134): the position of to[i] by a linear search behind i
static Velocity swap_sequence(const Route &from, const Route &to)
{
    Route tmp = from;
    Velocity seq;
    for (size_t i = 0; i + 1 < tmp.size(); ++i) {
        if (tmp[i] != to[i]) {
            size_t j = i + 1;
            while (tmp[j] != to[i]) ++j;
            seq.push_back({(uint32_t)i, (uint32_t)j});
            std::swap(tmp[i], tmp[j]);
        }
    }
    return seq;
}

static Velocity swap_sequence_inverse(const Route &from, const Route &to)
{
    Route tmp = from, where(from.size());
    for (size_t k = 0; k < tmp.size(); ++k) where[tmp[k]] = (uint32_t)k;
    Velocity seq;
    for (size_t i = 0; i + 1 < tmp.size(); ++i) {
        if (tmp[i] != to[i]) {
            const uint32_t j = where[to[i]];
            seq.push_back({(uint32_t)i, j});
            where[tmp[i]] = j;
            where[to[i]] = (uint32_t)i;
            std::swap(tmp[i], tmp[j]);
        }
    }
    return seq;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: pso_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, seed = 1, run = 0, n_nearest = 3;
    bool trace = false, draws = false, inverse = false;
    std::string init_path;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const char *v = a + 1 < argc ? argv[a + 1] : "";
        if (s == "--trace") trace = true;
        else if (s == "--draws") draws = true;
        else if (s == "--inverse-table") inverse = true;
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
        for (uint64_t base : {0ull, (unsigned long long)tl::kGaInitEvent})
            for (uint64_t e = 0; e < 8; ++e)
                for (uint32_t s = 0; s < 28; ++s) printf("%llu\n", (unsigned long long)tl::ga_draw_key(key, base + e, s));
        for (double x : {0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 4.5, 0.9 * 5.0, 2.4999999999999996, 1e9 + 0.5, -1.0, 5e9})
            printf("%u\n", tl::pso_keep(x));
        for (uint32_t e : {0u, 1u, 7u, 9999u})
            for (uint32_t of : {0u, 1u, 8u, 10000u}) printf("%.17g\n", tl::pso_weight(e, of));
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
    const uint32_t P = tl::pso_particles((uint32_t)std::min<uint64_t>(n_nearest, 0xFFFFFFFFu)), vmax = tl::pso_vmax(n);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Route> pos(P, Route(n));
    for (uint32_t i = 0; i < P; ++i) {
        Route &r = pos[i];
        if (i == 0 && !init_path.empty()) {
            FILE *f = fopen(init_path.c_str(), "r");
            if (!f) {
                perror(init_path.c_str());
                return 1;
            }
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
            continue;
        }
        std::iota(r.begin(), r.end(), 0u);
        for (uint32_t j = n - 1; j >= 1 && j < n; --j) std::swap(r[j], r[tl::sa_position(tl::ga_draw_key(key, tl::ga_init_event(n, i, j), tl::kGaSlotShuffle), j + 1)]);
    }
    std::vector<Velocity> vel(P);
    std::vector<Route> pbest = pos;
    std::vector<float> pcost(P);
    for (uint32_t i = 0; i < P; ++i) pcost[i] = tour_length(xy, pbest[i]);
    uint32_t b = 0;
    for (uint32_t i = 1; i < P; ++i)
        if (pcost[i] < pcost[b]) b = i;  // min_by: the first of equal minima
    Route gbest = pbest[b];
    float gcost = pcost[b];
    uint64_t improved = 0;
    std::vector<uint32_t> log, elog;
    if (trace) log.insert(log.end(), {0xFFFFFFFFu, b, bits(gcost)});
    for (uint64_t e = 0; e < epochs; ++e) {
        const double w = tl::pso_weight((uint32_t)e, (uint32_t)epochs);
        std::vector<uint32_t> costs(P), lens(P);
        for (uint32_t i = 0; i < P; ++i) {
            const uint64_t ev = tl::pso_step_event((uint32_t)e, P, i);
            const double r1 = tl::pso_uniform(tl::ga_draw_key(key, ev, tl::kPsoSlotR1)), r2 = tl::pso_uniform(tl::ga_draw_key(key, ev, tl::kPsoSlotR2));
            const size_t ik = tl::pso_inertia_keep(w, (uint32_t)vel[i].size());
            const Velocity cog = inverse ? swap_sequence_inverse(pos[i], pbest[i]) : swap_sequence(pos[i], pbest[i]);
            const size_t ck = tl::pso_pull_keep(r1, (uint32_t)cog.size());
            const Velocity soc = inverse ? swap_sequence_inverse(pos[i], gbest) : swap_sequence(pos[i], gbest);
            const size_t sk = tl::pso_pull_keep(r2, (uint32_t)soc.size());
            Velocity nv(vel[i].begin(), vel[i].begin() + std::min(ik, vel[i].size()));
            nv.insert(nv.end(), cog.begin(), cog.begin() + std::min(ck, cog.size()));
            nv.insert(nv.end(), soc.begin(), soc.begin() + std::min(sk, soc.size()));
            if (nv.size() > vmax) nv.resize(vmax);
            for (const auto &s : nv) std::swap(pos[i][s.first], pos[i][s.second]);
            vel[i] = nv;
            const float cost = tour_length(xy, pos[i]);
            costs[i] = bits(cost);
            lens[i] = (uint32_t)nv.size();
            if (cost < pcost[i]) {
                pbest[i] = pos[i];
                pcost[i] = cost;
            }
            if (cost < gcost) {
                gbest = pos[i];
                gcost = cost;
                ++improved;
                if (trace) log.insert(log.end(), {(uint32_t)e, i, bits(cost)});
            }
        }
        if (trace) {
            elog.insert(elog.end(), costs.begin(), costs.end());
            elog.insert(elog.end(), lens.begin(), lens.end());
        }
    }
    const float cost = tour_length(xy, gbest);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %u %.6f\n", (unsigned long long)epochs, (unsigned long long)(epochs * P), (unsigned long long)improved, bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", gbest[i], i + 1 == n ? '\n' : ' ');
    if (n == 0) printf("\n");
    for (size_t k = 0; k + 2 < log.size(); k += 3) printf("I %u %u %u\n", log[k], log[k + 1], log[k + 2]);
    for (size_t k = 0; k < elog.size(); k += 2 * (size_t)P) {
        printf("E");
        for (size_t j = 0; j < 2 * (size_t)P; ++j) printf(" %u", elog[k + j]);
        printf("\n");
    }
    return 0;
}
