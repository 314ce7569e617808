// cs_cpu_baseline.cpp — the project's cuckoo search solver restated for one CPU core, stand-alone (its own main, no library): the
// second oracle beside tests/_cs_oracle.py and the CPU baseline of scripts/timing_cuckoo_search.py.  It does what the reference
// does per flight — k literal segment reversals, a full f32 re-sum — with the project's seeded draws and Lévy step, whose text
// (teeline_amd/csrc/cs_spec.h, levy_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/cs_cpu_baseline.cpp -o cs_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   cs_cpu_baseline FILE.tsp [--epochs E --seed S --run K --n-nearest N --mutation-probability P --init FILE --trace --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  --init FILE: nest 0's start, n positions separated by white space.
// Prints "epochs flights improved cost_bits seconds", the best tour, and with --trace one "I epoch source cost_bits" line per log
// record (the start best first, epoch 4294967295) and one "E .." line per epoch: the 4 N words of tl_cuckoo_search_trace's epoch
// row.  --draws prints u(seed, run, event, slot) for the events 0 .. 7 and 2^58 .. 2^58 + 7, slot < 28, then for each of 64 word
// tuples taken from that stream the Lévy step's bits, its resamples and the flight lengths at n = 52, 280, 1002, and exits.
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

#include "cs_spec.h"

typedef std::vector<uint32_t> Route;

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

static Route shuffled(uint64_t key, uint32_t n, uint64_t event0, uint32_t slot)
{
    Route r(n);
    std::iota(r.begin(), r.end(), 0u);
    for (uint32_t j = n - 1; j >= 1 && j < n; --j) std::swap(r[j], r[tl::sa_position(tl::ga_draw_key(key, event0 + j, slot), j + 1)]);
    return r;
}

struct StreamWords {
    uint64_t key, event;
    uint64_t operator()(uint32_t i) const { return tl::ga_draw_key(key, event, i); }
};

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: cs_cpu_baseline FILE.tsp [options]\n");
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
        for (uint64_t e = 0; e < 64; ++e) {
            uint32_t tries = 0;
            const double v = tl::levy_step(StreamWords{key, e}, &tries);
            uint64_t b;
            memcpy(&b, &v, 8);
            printf("%llu %u %u %u %u\n", (unsigned long long)b, tries, tl::cs_flight_length(std::fabs(v), 52), tl::cs_flight_length(std::fabs(v), 280),
                   tl::cs_flight_length(std::fabs(v), 1002));
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
    const uint32_t N = tl::cs_nests((uint32_t)std::min<uint64_t>(n_nearest, 0xFFFFFFFFu));
    const double pa = tl::cs_pa(p_mut);
    if (n < 2 && epochs >= 1) {
        fprintf(stderr, "n=%u: the reference panics (clamp(1, n / 2) with min > max)\n", n);
        return 1;
    }
    if (n > 0xFFFFu || N > tl::kCsMaxNests || epochs >= 0xFFFFFFFFull || !tl::cs_events_fit((uint32_t)epochs, N, n)) {
        fprintf(stderr, "outside the specification's range\n");
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Route> nest(N);
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
            nest[i] = r;
            continue;
        }
        nest[i] = shuffled(key, n, tl::ga_init_event(n, i, 0), tl::kGaSlotShuffle);
    }
    std::vector<float> costs(N);
    for (uint32_t i = 0; i < N; ++i) costs[i] = tour_length(xy, nest[i]);
    uint32_t b = 0;
    for (uint32_t i = 1; i < N; ++i)
        if (costs[i] < costs[b]) b = i;  // min_by: the first of equal minima
    Route best = nest[b];
    float best_cost = costs[b];
    uint64_t improved = 0;
    std::vector<uint32_t> log, elog;
    if (trace) log.insert(log.end(), {0xFFFFFFFFu, b, bits(best_cost)});
    std::vector<uint32_t> row(4 * (size_t)N);
    std::vector<char> touched(N);
    for (uint64_t e = 0; e < epochs; ++e) {
        std::fill(touched.begin(), touched.end(), 0);
        for (uint32_t c = 0; c < N; ++c) {
            const uint64_t base = tl::cs_base((uint32_t)e, N, c, n);
            const uint32_t k = tl::cs_flight_length(tl::cs_levy(key, base), n);
            Route nw = nest[c];
            for (uint32_t r = 0; r < k; ++r) {
                uint32_t i, j;
                tl::cs_reversal(key, base, r, n, &i, &j);
                std::reverse(nw.begin() + i, nw.begin() + j + 1);
            }
            const float cost = tour_length(xy, nw);
            const uint32_t t = tl::cs_target(key, base, N);
            const bool acc = cost < costs[t];
            row[N + c] = k;
            row[2 * (size_t)N + c] = t | (acc ? 1u << 31 : 0u) | (touched[c] ? 1u << 30 : 0u);
            if (acc) {
                nest[t] = nw;
                costs[t] = cost;
                touched[t] = 1;
                if (cost < best_cost) {
                    best = nest[t];
                    best_cost = cost;
                    ++improved;
                    if (trace) log.insert(log.end(), {(uint32_t)e, c, bits(cost)});
                }
            }
        }
        for (uint32_t c = 0; c < N; ++c) {
            const uint64_t base = tl::cs_base((uint32_t)e, N, c, n);
            const bool ab = tl::cs_abandoned(key, base, pa);
            row[3 * (size_t)N + c] = ab ? 1u : 0u;
            if (!ab) continue;
            nest[c] = shuffled(key, n, base + 1, tl::kCsSlotReplace);
            costs[c] = tour_length(xy, nest[c]);
            if (costs[c] < best_cost) {
                best = nest[c];
                best_cost = costs[c];
                ++improved;
                if (trace) log.insert(log.end(), {(uint32_t)e, N + c, bits(best_cost)});
            }
        }
        if (trace) {
            for (uint32_t c = 0; c < N; ++c) row[c] = bits(costs[c]);
            elog.insert(elog.end(), row.begin(), row.end());
        }
    }
    const float cost = tour_length(xy, best);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %u %.6f\n", (unsigned long long)epochs, (unsigned long long)(epochs * N), (unsigned long long)improved, bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", best[i], i + 1 == n ? '\n' : ' ');
    if (n == 0) printf("\n");
    for (size_t k = 0; k + 2 < log.size(); k += 3) printf("I %u %u %u\n", log[k], log[k + 1], log[k + 2]);
    for (size_t k = 0; k < elog.size(); k += 4 * (size_t)N) {
        printf("E");
        for (size_t j = 0; j < 4 * (size_t)N; ++j) printf(" %u", elog[k + j]);
        printf("\n");
    }
    return 0;
}
