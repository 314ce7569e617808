// sa_cpu_baseline.cpp — the project's simulated annealing restated for one CPU core, stand-alone (its own main, no library): the
// second oracle beside tests/_sa_oracle.py and the CPU baseline of scripts/timing_sim_anneal.py.  It does what the reference does
// per epoch — copy the route, reverse from..=to, re-sum the whole tour in f32 — with the project's seeded draws and its exp.
//
//   g++ -O2 -std=c++17 -ffp-contract=off tests/probes/sa_cpu_baseline.cpp -o sa_cpu_baseline
//   (host check: add -fsanitize=address,undefined)
//   sa_cpu_baseline FILE.tsp [--epochs E --cooling-rate C --min-temperature LO --max-temperature HI --seed S --chain K --trace --draws]
// FILE.tsp: NODE_COORD_SECTION instances (EUC_2D).  Prints "epochs accepted cost_bits seconds", the tour, and with --trace one
// "epoch from to cost_bits" line per accepted epoch.  --draws prints u(seed, chain, e, slot) for e < 2, slot < 23 and exits.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static const uint64_t G = 0x9E3779B97F4A7C15ULL;

static uint64_t mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static uint64_t draw(uint64_t key, uint64_t epoch, uint64_t slot) { return mix(key + G * (32 * epoch + slot + 1)); }

static float criteria(float x)
{
    if (x != x) return x;
    if (x < -87.0f) return 0.0f;
    if (x > 89.0f) return INFINITY;
    static const double fact[14] = {1, 1, 2, 6, 24, 120, 720, 5040, 40320, 362880, 3628800, 39916800, 479001600, 6227020800.0};
    const double xd = (double)x;
    const double k = std::rint(xd * 1.4426950408889634);
    volatile double t1 = k * 6.93147180369123816490e-01, t2 = k * 1.90821492927058770002e-10;  // (volatile: never an FMA)
    const double r = (xd - t1) - t2;
    double q = 1.0 / fact[13];
    for (int i = 12; i >= 0; --i) {
        volatile double m = q * r;
        q = m + 1.0 / fact[i];
    }
    return (float)std::ldexp(q, (int)k);
}

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
        fprintf(stderr, "usage: sa_cpu_baseline FILE.tsp [options]\n");
        return 2;
    }
    uint64_t epochs = 10000, seed = 1, chain = 0;
    float rate = 1e-4f, lo = 1e-3f, hi = 1000.0f;
    bool trace = false, draws = false;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const char *v = a + 1 < argc ? argv[a + 1] : "";
        if (s == "--trace") trace = true;
        else if (s == "--draws") draws = true;
        else if (s == "--epochs") epochs = strtoull(v, nullptr, 10), ++a;
        else if (s == "--seed") seed = strtoull(v, nullptr, 10), ++a;
        else if (s == "--chain") chain = strtoull(v, nullptr, 10), ++a;
        else if (s == "--cooling-rate") rate = strtof(v, nullptr), ++a;
        else if (s == "--min-temperature") lo = strtof(v, nullptr), ++a;
        else if (s == "--max-temperature") hi = strtof(v, nullptr), ++a;
        else {
            fprintf(stderr, "unknown option %s\n", s.c_str());
            return 2;
        }
    }
    const uint64_t key = mix(seed + G * (chain + 1));
    if (draws) {
        for (uint64_t e = 0; e < 2; ++e)
            for (uint64_t s = 0; s < 23; ++s) printf("%llu\n", (unsigned long long)draw(key, e, s));
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
    std::vector<uint32_t> tour(n), cand(n);
    for (uint32_t i = 0; i < n; ++i) tour[i] = i;
    const auto t0 = std::chrono::steady_clock::now();
    float cost = tour_length(xy, tour), T = hi;
    uint64_t e = 0, accepted = 0;
    std::vector<uint64_t> log;
    while (e < epochs || T > lo) {
        if (n < 2) {
            fprintf(stderr, "n_items must be bigger than 2\n");
            return 1;
        }
        uint32_t from = 0, to = 0;
        for (uint64_t a = 0; a < 11; ++a) {
            const uint32_t p1 = (uint32_t)(((draw(key, e, 2 * a) >> 32) * n) >> 32), p2 = (uint32_t)(((draw(key, e, 2 * a + 1) >> 32) * n) >> 32);
            from = p1 < p2 ? p1 : p2;
            to = p1 < p2 ? p2 : p1;
            if (to - from > 1) break;
        }
        cand = tour;
        for (uint32_t i = 0; from + i <= to; ++i) cand[from + i] = tour[to - i];
        const float c = tour_length(xy, cand);
        bool ok;
        if (c < cost) ok = true;
        else if (std::fabs(c - cost) < 1.1920929e-07f) ok = false;
        else ok = (float)(uint32_t)(draw(key, e, 22) >> 40) * 5.9604644775390625e-08f < criteria((-(c - cost)) / T);
        if (ok) {
            tour.swap(cand);
            cost = c;
            ++accepted;
            if (trace) {
                log.push_back(e);
                log.push_back(((uint64_t)from << 32) | to);
                log.push_back(bits(c));
            }
        }
        volatile float prod = rate * T;
        T = T - prod;
        ++e;
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %llu %u %.6f\n", (unsigned long long)e, (unsigned long long)accepted, bits(cost), sec);
    for (uint32_t i = 0; i < n; ++i) printf("%u%c", tour[i], i + 1 == n ? '\n' : ' ');
    for (size_t k = 0; k + 2 < log.size(); k += 3)
        printf("%llu %u %u %u\n", (unsigned long long)log[k], (uint32_t)(log[k + 1] >> 32), (uint32_t)log[k + 1], (uint32_t)log[k + 2]);
    return 0;
}
