// hill_cpu_baseline.cpp — the project's stochastic hill climb restated for one CPU core, stand-alone (its own main, no library): the
// second oracle beside tests/_hill_oracle.py and the CPU baseline of scripts/timing_hill_climb.py.  It does what the reference does
// per epoch — clone the current route, reverse from..=to, re-sum the whole tour in f32, compare with the best cost — with the
// project's seeded draws, whose text (teeline_amd/csrc/hill_spec.h) it shares with the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/hill_cpu_baseline.cpp -o hill_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   hill_cpu_baseline CASE [--epochs E --platoo P --seed S --chain K --init FILE --trace --draws]
// CASE: a text file, "n xy" followed by n lines "x y", or "n dm" followed by the n x n distances row by row; a FILE.tsp with a
// NODE_COORD_SECTION (EUC_2D) is read too.  --init FILE: the start tour, n positions separated by white space (default: city
// order).  Prints "epochs accepts restarts reversed cost_bits seconds", the best tour, and with --trace one
// "epoch from to cost_bits" line per event (a restart: "epoch 4294967295 0 0").  --draws prints u(seed, chain, event, slot) for
// the pair slots of epochs 0 and 1 and for the shuffle events of epoch 3 on n = 7, and exits.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hill_spec.h"

struct Instance {
    uint32_t n = 0;
    std::vector<float> xy, dm;  // dm: n x n, or empty
    float d(uint32_t a, uint32_t b) const
    {
        if (!dm.empty()) return dm[(size_t)a * n + b];
        const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
        volatile float xx = dx * dx, yy = dy * dy;
        return std::sqrt(xx + yy);
    }
};

static float tour_length(const Instance &I, const std::vector<uint32_t> &t)
{
    const size_t n = t.size();
    if (n < 2) return 0.0f;
    float tot = I.d(t[n - 1], t[0]);
    for (size_t k = 0; k + 1 < n; ++k) tot += I.d(t[k], t[k + 1]);
    return tot;
}

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static bool read_case(const char *path, Instance &I)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        perror(path);
        return false;
    }
    char line[512], kind[16] = "";
    unsigned n = 0;
    if (fgets(line, sizeof line, f) && sscanf(line, "%u %15s", &n, kind) == 2 && (!strcmp(kind, "xy") || !strcmp(kind, "dm"))) {
        I.n = n;
        std::vector<float> &v = !strcmp(kind, "xy") ? I.xy : I.dm;
        const size_t want = !strcmp(kind, "xy") ? 2 * (size_t)n : (size_t)n * n;
        float x;
        while (v.size() < want && fscanf(f, "%f", &x) == 1) v.push_back(x);
        fclose(f);
        return v.size() == want;
    }
    bool on = strncmp(line, "NODE_COORD_SECTION", 18) == 0;
    while (fgets(line, sizeof line, f)) {
        if (!on) {
            on = strncmp(line, "NODE_COORD_SECTION", 18) == 0;
            continue;
        }
        int id;
        float x, y;
        if (sscanf(line, "%d %f %f", &id, &x, &y) != 3) break;
        I.xy.push_back(x);
        I.xy.push_back(y);
    }
    fclose(f);
    I.n = (uint32_t)(I.xy.size() / 2);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: hill_cpu_baseline CASE [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, platoo = 500, seed = 1, chain = 0;
    bool trace = false, draws = false;
    std::string init_path;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const char *v = a + 1 < argc ? argv[a + 1] : "";
        if (s == "--trace") trace = true;
        else if (s == "--draws") draws = true;
        else if (s == "--epochs") epochs = strtoull(v, nullptr, 10), ++a;
        else if (s == "--platoo") platoo = strtoull(v, nullptr, 10), ++a;
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
            for (uint32_t s = 0; s < 22; ++s) printf("%llu\n", (unsigned long long)tl::hill_draw_key(key, e, s));
        for (uint32_t j = 1; j < 7; ++j) printf("%llu\n", (unsigned long long)tl::hill_draw_key(key, tl::hill_shuffle_event(3, 7, j), tl::kGaSlotShuffle));
        return 0;
    }
    Instance I;
    if (!read_case(argv[1], I)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 1;
    }
    const uint32_t n = I.n;
    if (n < 2) {
        fprintf(stderr, "n_items must be bigger than 2\n");
        return 1;
    }
    if (epochs == 0 || epochs >= 0xFFFFFFFFull) {
        fprintf(stderr, "epochs = 0 never ends; epochs + 1 must fit 32 bits\n");
        return 1;
    }
    std::vector<uint32_t> cur(n), cand(n);
    for (uint32_t i = 0; i < n; ++i) cur[i] = i;
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
            cur[i] = v;
        }
        fclose(f);
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> best = cur;
    float best_distance = tour_length(I, best);
    uint64_t epoch = 0, n_stale = 0, accepts = 0, restarts = 0, reversed = 0;
    std::vector<uint32_t> log;
    for (;;) {  // stochastic_hill.rs:39-83
        uint32_t from = 0, to = 0;
        tl::sa_pair(key, (uint32_t)epoch, n, &from, &to);
        cand = cur;
        for (uint32_t i = 0; from + i <= to; ++i) cand[from + i] = cur[to - i];
        const float c = tour_length(I, cand);
        if (c < best_distance) {
            cur = cand;
            best = cand;
            best_distance = c;
            n_stale = 0;
            ++accepts;
            reversed += to - from + 1;
            if (trace) log.insert(log.end(), {(uint32_t)epoch, from, to, bits(c)});
        } else {
            ++n_stale;
        }
        ++epoch;
        if (n_stale > platoo && platoo > 0) {
            tl::hill_shuffle(key, (uint32_t)(epoch - 1), n, cur.data());
            n_stale = 0;
            ++restarts;
            if (trace) log.insert(log.end(), {(uint32_t)(epoch - 1), 0xFFFFFFFFu, 0u, 0u});
        }
        if (epoch > epochs) break;
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %llu %llu %u %.6f\n", (unsigned long long)epoch, (unsigned long long)accepts, (unsigned long long)restarts, (unsigned long long)reversed,
           bits(best_distance), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", best[i], i + 1 == n ? '\n' : ' ');
    for (size_t k = 0; k + 3 < log.size(); k += 4) printf("%u %u %u %u\n", log[k], log[k + 1], log[k + 2], log[k + 3]);
    return 0;
}
