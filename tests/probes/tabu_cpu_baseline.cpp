// tabu_cpu_baseline.cpp — the project's tabu search restated for one CPU core, stand-alone (its own main, no library): the second
// oracle beside tests/_tabu_oracle.py and the CPU baseline of scripts/timing_tabu_search.py.  It does what the reference does per
// candidate — clone the route, reverse from..=to, re-sum the whole tour in f32, compare with every listed route — with the
// project's seeded draws, whose text (teeline_amd/csrc/tabu_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/tabu_cpu_baseline.cpp -o tabu_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   tabu_cpu_baseline FILE.tsp [--epochs E --seed S --chain K --init FILE --trace --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: the start tour, n positions separated by white space (default:
// city order).  Prints "epochs hits forced bests candidates cost_bits seconds", the best tour, and with --trace one
// "attempt from to cost_bits" line per epoch.  --draws prints u(seed, chain, n = 7, epoch, attempt, slot) for epoch < 2,
// attempt <= 7, slot < 22 and exits.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "tabu_spec.h"

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

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: tabu_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, seed = 1, chain = 0;
    bool trace = false, draws = false;
    std::string init_path;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const char *v = a + 1 < argc ? argv[a + 1] : "";
        if (s == "--trace") trace = true;
        else if (s == "--draws") draws = true;
        else if (s == "--epochs") epochs = strtoull(v, nullptr, 10), ++a;
        else if (s == "--seed") seed = strtoull(v, nullptr, 10), ++a;
        else if (s == "--chain") chain = strtoull(v, nullptr, 10), ++a;
        else if (s == "--init") init_path = v, ++a;
        else {
            fprintf(stderr, "unknown option %s\n", s.c_str());
            return 2;
        }
    }
    const uint64_t key = tl::sa_chain_key(seed, chain);
    if (draws) {
        for (uint32_t e = 0; e < 2; ++e)
            for (uint32_t a = 0; a <= 7; ++a)
                for (uint32_t s = 0; s < 22; ++s) printf("%llu\n", (unsigned long long)tl::tabu_draw_key(key, tl::tabu_event(e, 7, a), s));
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
    if (n < 2) {
        fprintf(stderr, "n_items must be bigger than 2\n");
        return 1;
    }
    if (epochs == 0) {
        fprintf(stderr, "epochs = 0 never ends\n");
        return 1;
    }
    std::vector<uint32_t> u(n), cand(n);
    for (uint32_t i = 0; i < n; ++i) u[i] = i;
    if (!init_path.empty()) {
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
            u[i] = v;
        }
        fclose(f);
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::deque<std::vector<uint32_t>> tabu;  // newest first (tabu_search.rs:87-110)
    auto add = [&](const std::vector<uint32_t> &r) {
        if (tabu.size() >= n) tabu.pop_back();
        tabu.push_front(r);
    };
    auto contains = [&](const std::vector<uint32_t> &r) {
        for (const auto &t : tabu)
            if (t == r) return true;
        return false;
    };
    std::vector<uint32_t> best = u;
    add(best);
    float best_distance = tour_length(xy, u);
    uint64_t hits = 0, forced = 0, bests = 0, candidates = 0;
    std::vector<uint32_t> log;
    for (uint64_t e = 0; e <= epochs; ++e) {
        const float local = tour_length(xy, u);
        uint32_t a = 0, from = 0, to = 0;
        float c = 0.0f;
        for (;; ++a) {  // select (tabu_search.rs:65-81)
            tl::tabu_pair(key, tl::tabu_event((uint32_t)e, n, a), n, &from, &to);
            cand = u;
            for (uint32_t i = 0; from + i <= to; ++i) cand[from + i] = u[to - i];
            c = tour_length(xy, cand);
            if (a == n) {
                ++forced;
                break;
            }
            if (c < local) {
                if (!contains(cand)) break;
                ++hits;
            }
        }
        if (c < best_distance) {
            best = cand;
            best_distance = c;
            ++bests;
        }
        add(u);
        u.swap(cand);
        candidates += a + 1;
        if (trace) {
            log.push_back(a);
            log.push_back(from);
            log.push_back(to);
            log.push_back(bits(c));
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %llu %llu %u %.6f\n", (unsigned long long)(epochs + 1), (unsigned long long)hits, (unsigned long long)forced, (unsigned long long)bests,
           (unsigned long long)candidates, bits(best_distance), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", best[i], i + 1 == n ? '\n' : ' ');
    for (size_t k = 0; k + 3 < log.size(); k += 4) printf("%u %u %u %u\n", log[k], log[k + 1], log[k + 2], log[k + 3]);
    return 0;
}
