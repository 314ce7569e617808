// one_tree_cpu_baseline.cpp — the Held-Karp ascent of DESIGN.md §4.29 on ONE core, with csrc/one_tree_spec.h's text for the
// scalar part: what scripts/timing_one_tree_bound.py holds the device against.  Unlike tl_one_tree_bound_host it reads the
// distances from an n x n f32 matrix built once before the clock starts, as a CPU program would.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/one_tree_cpu_baseline.cpp -o one_tree_cpu_baseline
//   one_tree_cpu_baseline FILE UPPER ROOT ITERATIONS LAMBDA0 PATIENCE     FILE: n, then n lines "x y"
// prints: bound (hex f64), best_iter, iterations run, stop, ms of the ascent
#include "one_tree_spec.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace tl;

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n = 0;
    if (fscanf(f, "%u", &n) != 1 || n < 3) return 2;
    std::vector<float> xy(2 * (size_t)n);
    for (size_t k = 0; k < xy.size(); ++k)
        if (fscanf(f, "%f", &xy[k]) != 1) return 2;
    fclose(f);
    const OneTreeJob J{atof(argv[5]), atof(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[6]), 0u};
    if (J.root >= n || J.iterations < 1 || J.patience < 1) return 2;
    std::vector<float> D((size_t)n * n, 0.0f);
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
            const float sx = dx * dx, sy = dy * dy;
            D[(size_t)a * n + b] = sqrtf(sx + sy);
        }
    const auto t0 = std::chrono::steady_clock::now();
    OneTreeState S;
    one_tree_start(S, J);
    const uint32_t s = J.root, start = s == 0u ? 1u : 0u;
    const double inf = __builtin_huge_val();
    std::vector<double> pi(n, 0.0), key(n);
    std::vector<uint32_t> par(n);
    std::vector<int> deg(n);
    std::vector<char> in(n);
    while (S.stop == kOneTreeStopNone) {
        for (uint32_t v = 0; v < n; ++v) {
            key[v] = v == start ? 0.0 : inf;
            par[v] = kOneTreeNone;
            deg[v] = 0;
            in[v] = v == s;
        }
        double sum = 0.0;
        uint32_t u = start;
        for (uint32_t r = 0; r + 1u < n; ++r) {  // the update pass and the next argmin are one sweep, as on the device
            in[u] = 1;
            sum = sum + key[u];
            if (par[u] != kOneTreeNone) {
                ++deg[u];
                ++deg[par[u]];
            }
            const float *row = &D[(size_t)u * n];
            const double pu = pi[u];
            uint32_t next = kOneTreeNone;
            double best = inf;
            for (uint32_t v = 0; v < n; ++v) {
                if (in[v]) continue;
                const double w = (double)row[v] + (pu + pi[v]);
                if (w < key[v]) {
                    key[v] = w;
                    par[v] = u;
                }
                if (next == kOneTreeNone || key[v] < best) {
                    best = key[v];
                    next = v;
                }
            }
            u = next;
        }
        uint32_t nb[2] = {kOneTreeNone, kOneTreeNone};
        for (int e = 0; e < 2; ++e) {
            double bw = 0.0;
            for (uint32_t v = 0; v < n; ++v) {
                if (v == s || v == nb[0]) continue;
                const double w = (double)D[(size_t)s * n + v] + (pi[s] + pi[v]);
                if (nb[e] == kOneTreeNone || w < bw) {
                    bw = w;
                    nb[e] = v;
                }
            }
            sum = sum + bw;
            ++deg[nb[e]];
        }
        deg[s] = 2;
        double P = 0.0;
        for (uint32_t v = 0; v < n; ++v) P = P + pi[v];
        uint32_t g2 = 0;
        for (uint32_t v = 0; v < n; ++v) g2 += (uint32_t)((deg[v] - 2) * (deg[v] - 2));
        double t;
        one_tree_decide(S, J, sum - 2.0 * P, g2, &t);
        if (S.stop == kOneTreeStopNone)
            for (uint32_t v = 0; v < n; ++v) pi[v] = pi[v] + t * (double)(deg[v] - 2);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%a %u %u %u %.3f\n", S.best, S.best_iter, S.k, S.stop, ms);
    return 0;
}
