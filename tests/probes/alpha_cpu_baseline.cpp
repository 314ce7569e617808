// alpha_cpu_baseline.cpp — the alpha-nearness candidate lists of DESIGN.md §4.32 on ONE core, with csrc/alpha_spec.h's text: what
// scripts/timing_alpha_candidates.py holds the device against.  Unlike tl_alpha_candidates_host it reads the distances from an
// n x n f32 matrix built once before the clock starts, as a CPU program would.  Penalties are zero unless a file of n doubles is given.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I teeline_amd/csrc tests/probes/alpha_cpu_baseline.cpp -o alpha_cpu_baseline
//   alpha_cpu_baseline FILE ROOT K [PIFILE]      FILE: n, then n lines "x y";  PIFILE: n numbers
//   alpha_cpu_baseline --self LO HI              synthetic instances of n = LO .. HI (every root's parity, k = 1, 5, n - 1): checks
//                                                every row against a walk along every tree path; prints "ok" (the sanitizer run)
// prints: an FNV-1a hash of the rows, the sum of the output alphas (hex f64), ms of the lists
#include "alpha_spec.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace tl;

namespace {

struct MatrixDist {
    const float *D;
    uint32_t n;
    float operator()(uint32_t a, uint32_t b) const { return D[(size_t)a * n + b]; }
};

std::vector<float> matrix_of(const std::vector<float> &xy, uint32_t n)
{
    std::vector<float> D((size_t)n * n, 0.0f);
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            const float dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
            const float sx = dx * dx, sy = dy * dy;
            D[(size_t)a * n + b] = sqrtf(sx + sy);
        }
    return D;
}

// every row again, beta by a walk from the source over the tree's adjacency: 0 where the lists agree
int self_check(uint32_t n, uint32_t root, uint32_t k, uint64_t seed)
{
    std::vector<float> xy(2 * (size_t)n);
    for (float &v : xy) {  // a small integer grid: many equal weights
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        v = (float)((seed >> 33) % 23u);
    }
    const std::vector<float> D = matrix_of(xy, n);
    const MatrixDist d{D.data(), n};
    std::vector<double> pi(n);
    for (uint32_t v = 0; v < n; ++v) pi[v] = (double)((v * 7u) % 5u) * 0.25 - 0.5;
    const uint32_t kk = k > n - 1u ? n - 1u : k;
    std::vector<uint32_t> cand((size_t)n * kk), par(n);
    std::vector<double> alpha((size_t)n * kk);
    uint32_t nb[2];
    if (!alpha_candidates_seq(d, pi.data(), n, root, kk, cand.data(), alpha.data(), par.data(), nb)) return 1;
    std::vector<std::vector<uint32_t>> adj(n);
    for (uint32_t v = 0; v < n; ++v)
        if (v != root && par[v] != kOneTreeNone) {
            adj[v].push_back(par[v]);
            adj[par[v]].push_back(v);
        }
    const double w_rb = alpha_weight(d(root, nb[1]), pi[root], pi[nb[1]]);
    std::vector<double> val(n), wrow(n), beta(n);
    std::vector<uint32_t> todo, want(kk);
    std::vector<double> want_alpha(kk);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t v = 0; v < n; ++v) wrow[v] = v == i ? 0.0 : alpha_weight(d(i, v), pi[i], pi[v]);
        if (i == root) {
            for (uint32_t v = 0; v < n; ++v) val[v] = alpha_of_root(wrow[v], w_rb, v == nb[0] || v == nb[1]);
        } else {
            std::vector<char> seen(n, 0);
            beta[i] = -__builtin_huge_val();
            seen[i] = 1;
            todo.assign(1, i);
            while (!todo.empty()) {
                const uint32_t u = todo.back();
                todo.pop_back();
                for (uint32_t v : adj[u])
                    if (!seen[v]) {
                        seen[v] = 1;
                        beta[v] = alpha_max(beta[u], alpha_weight(d(u, v), pi[u], pi[v]));
                        todo.push_back(v);
                    }
            }
            for (uint32_t v = 0; v < n; ++v)
                if (v != i) val[v] = v == root ? alpha_of_root(wrow[root], w_rb, i == nb[0] || i == nb[1]) : wrow[v] - beta[v];
        }
        alpha_select_host(val.data(), wrow.data(), n, i, kk, want.data(), want_alpha.data());
        if (memcmp(want.data(), &cand[(size_t)i * kk], (size_t)kk * 4) || memcmp(want_alpha.data(), &alpha[(size_t)i * kk], (size_t)kk * 8)) return 2;
        for (uint32_t q = 0; q < kk; ++q)
            if (std::signbit(want_alpha[q]) || want_alpha[q] != want_alpha[q]) return 3;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "--self")) {
        const uint32_t lo = (uint32_t)atoi(argv[2]), hi = (uint32_t)atoi(argv[3]);
        if (lo < 3 || hi < lo) return 2;
        for (uint32_t n = lo; n <= hi; ++n)
            for (uint32_t k : {1u, 5u, n - 1u}) {
                const uint32_t root = n % 3u == 0u ? 0u : n % 3u == 1u ? n - 1u : n / 2u;
                if (const int bad = self_check(n, root, k, 1000u * n + k)) {
                    printf("n = %u k = %u root = %u: check %d failed\n", n, k, root, bad);
                    return 1;
                }
            }
        printf("ok\n");
        return 0;
    }
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n = 0;
    if (fscanf(f, "%u", &n) != 1 || n < 3 || n > 65535) return 2;
    std::vector<float> xy(2 * (size_t)n);
    for (size_t q = 0; q < xy.size(); ++q)
        if (fscanf(f, "%f", &xy[q]) != 1) return 2;
    fclose(f);
    const uint32_t root = (uint32_t)atoi(argv[2]), k = (uint32_t)atoi(argv[3]);
    if (root >= n || k < 1 || k > kAlphaMaxK) return 2;
    std::vector<double> pi(n, 0.0);
    if (argc > 4) {
        FILE *g = fopen(argv[4], "r");
        if (!g) return 2;
        for (uint32_t v = 0; v < n; ++v)
            if (fscanf(g, "%lf", &pi[v]) != 1) return 2;
        fclose(g);
    }
    const std::vector<float> D = matrix_of(xy, n);
    const uint32_t kk = k > n - 1u ? n - 1u : k;
    std::vector<uint32_t> cand((size_t)n * kk);
    std::vector<double> alpha((size_t)n * kk);
    const auto t0 = std::chrono::steady_clock::now();
    if (!alpha_candidates_seq(MatrixDist{D.data(), n}, pi.data(), n, root, kk, cand.data(), alpha.data(), nullptr, nullptr)) return 1;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t c : cand)
        for (int b = 0; b < 4; ++b) h = (h ^ ((c >> (8 * b)) & 0xFFu)) * 0x100000001B3ull;
    double sum = 0.0;
    for (double a : alpha) sum = sum + a;
    printf("%016llx %a %.3f\n", (unsigned long long)h, sum, ms);
    return 0;
}
