// som_cpu_baseline.cpp — the Kohonen self-organising map solver of this project's specification (teeline_amd/csrc/som_spec.h) as a
// stand-alone CPU program: som_spec.h with a main.  It restates som.rs:12-186 in the reference's own loop order (every neuron of
// every epoch goes through the two tests, no radius), so it is also the one-core baseline of scripts/timing_kohonen_som.py.
//
//   som_cpu_baseline FILE [--epochs E] [--learning-rate X] [--radius-fraction X] [--neuron-multiplier K] [--seed S] [--run R] [--trace] [--time]
//   som_cpu_baseline x --queries
// FILE: the first token n, then n pairs "x y" (decimal f32).  Output: "cost_bits" / the tour; with --trace also "L city bmu" per
// epoch, "C epoch cost_bits tour.." per checkpoint record, "R xbits ybits" per neuron of the final ring (hex).  --time: the training's
// and the extraction's milliseconds instead.  --queries: draws, schedules, h values and small start rings for the tests.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "som_spec.h"

using namespace tl;

static uint64_t f64_bits(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
static uint32_t f32_bits(float x)
{
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

static float dist(const std::vector<float> &xy, uint32_t a, uint32_t b)
{
    const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
    return sqrtf(dx * dx + dy * dy);
}

// distance_matrix.rs:235-245: the closing edge first
static float tour_length(const std::vector<float> &xy, const std::vector<uint32_t> &tour)
{
    const size_t n = tour.size();
    if (n < 2) return 0.0f;
    float tot = dist(xy, tour[n - 1], tour[0]);
    for (size_t k = 0; k + 1 < n; ++k) tot += dist(xy, tour[k], tour[k + 1]);
    return tot;
}

static std::vector<uint32_t> extract(const std::vector<double> &cities, uint32_t n, const std::vector<double> &ring, uint32_t M)
{
    std::vector<uint32_t> bmu(n), tour(n);
    std::vector<double> bd(n);
    for (uint32_t c = 0; c < n; ++c) {
        double best = som_sq_dist(ring[0], ring[M], cities[c], cities[n + c]);
        uint32_t at = 0;
        for (uint32_t i = 1; i < M; ++i) {
            const double d = som_sq_dist(ring[i], ring[M + i], cities[c], cities[n + c]);
            if (d < best) {
                best = d;
                at = i;
            }
        }
        bmu[c] = at;
        bd[c] = best;
    }
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t rank = 0;
        for (uint32_t b = 0; b < n; ++b) rank += som_key_less(bmu[b], bd[b], b, bmu[c], bd[c], c) ? 1u : 0u;
        tour[rank] = c;
    }
    return tour;
}

static int queries()
{
    for (uint32_t t = 1; t <= 8; ++t) printf("%u\n", som_city(sa_chain_key(77, 5), t, 52));
    for (uint32_t epochs : {1u, 10u, 100000u})
        for (uint32_t t : {1u, epochs / 2u > 0u ? epochs / 2u : 1u, epochs}) {
            double sg;
            const SomEpoch e = som_schedule(t, epochs, 416, 0.8, 0.1, &sg);
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", f64_bits(e.eta), f64_bits(sg), f64_bits(e.two_sigma_sq), e.radius);
        }
    for (double d : {0.0, 1.0, 3.0, 4.0, 5.0, 6.0, 100.0}) {
        double h;
        const bool ok = som_h(d, 2.0, &h);
        printf("%d %" PRIu64 "\n", ok ? 1 : 0, f64_bits(h));
    }
    for (uint32_t M : {1u, 2u, 3u, 4u, 7u, 416u})
        for (uint32_t i = 0; i < M; ++i) {
            double x, y;
            som_ring_neuron(i, M, 0.5, 0.25, &x, &y);
            printf("%" PRIu64 " %" PRIu64 "\n", f64_bits(x), f64_bits(y));
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    uint32_t epochs = 100000, mult = 8, run = 0;
    uint64_t seed = 1;
    double eta0 = 0.8, rf = 0.1;
    bool trace = false, timing = false;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        auto val = [&]() { return a + 1 < argc ? argv[++a] : "0"; };
        if (s == "--queries") return queries();
        else if (s == "--epochs") epochs = (uint32_t)strtoul(val(), nullptr, 10);
        else if (s == "--learning-rate") eta0 = strtod(val(), nullptr);
        else if (s == "--radius-fraction") rf = strtod(val(), nullptr);
        else if (s == "--neuron-multiplier") mult = (uint32_t)strtoul(val(), nullptr, 10);
        else if (s == "--seed") seed = strtoull(val(), nullptr, 10);
        else if (s == "--run") run = (uint32_t)strtoul(val(), nullptr, 10);
        else if (s == "--trace") trace = true;
        else if (s == "--time") timing = true;
        else return 2;
    }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) return 2;
    uint32_t n = 0;
    if (fscanf(fh, "%u", &n) != 1 || n < 2 || epochs < 1 || mult < 1 || (uint64_t)n * mult > kSomMaxNeurons) return 2;
    std::vector<float> xy(2 * (size_t)n);
    for (size_t k = 0; k < xy.size(); ++k) {
        double v;
        if (fscanf(fh, "%lf", &v) != 1) return 2;
        xy[k] = (float)v;
    }
    fclose(fh);
    const uint32_t M = n * mult;
    std::vector<double> cities(2 * (size_t)n), ring(2 * (size_t)M);
    double cx, cy;
    som_normalise(xy.data(), n, cities.data(), cities.data() + n, &cx, &cy);
    for (uint32_t i = 0; i < M; ++i) som_ring_neuron(i, M, cx, cy, &ring[i], &ring[M + i]);
    const uint64_t key = sa_chain_key(seed, run);
    const uint32_t cp = som_checkpoint(epochs);
    std::string out;
    char buf[64];
    auto record = [&](uint32_t epoch, const std::vector<uint32_t> &tour, float cost) {
        snprintf(buf, sizeof buf, "C %u %u", epoch, f32_bits(cost));
        out += buf;
        for (uint32_t v : tour) {
            snprintf(buf, sizeof buf, " %u", v);
            out += buf;
        }
        out += "\n";
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t t = 1; t <= epochs; ++t) {
        const SomEpoch E = som_schedule(t, epochs, M, eta0, rf, nullptr);
        const uint32_t c = som_city(key, t, n);
        const double px = cities[c], py = cities[n + c];
        double best = som_sq_dist(ring[0], ring[M], px, py);
        uint32_t bmu = 0;
        for (uint32_t i = 1; i < M; ++i) {
            const double d = som_sq_dist(ring[i], ring[M + i], px, py);
            if (d < best) {
                best = d;
                bmu = i;
            }
        }
        for (uint32_t i = 0; i < M; ++i) {
            double h;
            if (!som_h((double)som_ring_distance(i, bmu, M), E.two_sigma_sq, &h)) continue;
            ring[i] = som_pull(ring[i], px, E.eta, h);
            ring[M + i] = som_pull(ring[M + i], py, E.eta, h);
        }
        if (trace) {
            snprintf(buf, sizeof buf, "L %u %u\n", c, bmu);
            out += buf;
            if (t % cp == 0) {
                const std::vector<uint32_t> snap = extract(cities, n, ring, M);
                record(t, snap, tour_length(xy, snap));
            }
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    const std::vector<uint32_t> tour = extract(cities, n, ring, M);
    const float cost = tour_length(xy, tour);
    const auto t2 = std::chrono::steady_clock::now();
    if (timing) {
        printf("%.3f %.3f\n", std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
        return 0;
    }
    if (trace && epochs % cp != 0) record(0xFFFFFFFFu, tour, cost);
    printf("%u\n", f32_bits(cost));
    for (uint32_t v : tour) printf("%u ", v);
    printf("\n");
    if (trace) {
        fputs(out.c_str(), stdout);
        for (uint32_t i = 0; i < M; ++i) printf("R %" PRIx64 " %" PRIx64 "\n", f64_bits(ring[i]), f64_bits(ring[M + i]));
    }
    return 0;
}
