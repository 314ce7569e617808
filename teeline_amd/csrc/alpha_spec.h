// alpha_spec.h — Helsgaun's alpha-nearness as this project specifies it: the values, the order of a row's
// candidates and the tree's level order.  One text for the device (alpha_candidates.hip), the host (tl_api_alpha.hip: the sequential
// restatement tl_alpha_candidates_host and the device entry's preparation) and the stand-alone one-core probe
// (tests/probes/alpha_cpu_baseline.cpp); tests/_alpha_oracle.py states the same in numpy and is the statement of record.  All f64,
// contraction off, as in one_tree_spec.h.
//
// The 1-tree under penalties pi with special position r is exactly §4.29's (one_tree_spec.h), w(i, j) = (double)d(i, j) + (pi_i + pi_j).
//   i != j, both != r:  beta(i, j) = the largest w on the tree path between i and j;  alpha(i, j) = w(i, j) - beta(i, j)
//   the root r with its neighbours a (chosen first) and b:  alpha(r, a) = alpha(r, b) = 0, else alpha(r, j) = w(r, j) - w(r, b);
//   alpha(j, r) = alpha(r, j)
// beta is a maximum of doubles and therefore exact: no evaluation order can change a bit of it, and alpha is ONE defined subtraction
// per pair.  That is what makes device, host and numpy agree bit for bit whatever the kernel's shape.  (w is never -0.0: d is +0.0 or
// positive, and x + y is -0.0 only where both are.)  alpha >= +0.0 always: Prim compares exactly these w, so the tree is minimal
// under the same comparisons, every path edge is <= the edge that closes its cycle, and x - x is +0.0.
//
// Row i: the k' = min(k, n - 1) positions j != i smallest by (alpha(i, j), w(i, j), j) — the doubles as numbers through
// one_tree_ordered, the position last (ties in alpha are the common case: every tree neighbour has alpha 0) — in that order.
//
// alpha chooses the set, distance orders it: Lin-Kernighan on supplied lists (tl_lk_candidates) searches every row in ascending
// f32 Euclidean distance, whatever order the rows were supplied in.
#pragma once
#include "one_tree_spec.h"

#include <algorithm>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace tl {

constexpr uint32_t kAlphaMaxK = 64u;

struct AlphaNode {  // a tree position: its parent and w(v, parent).  Prim's start: par = kOneTreeNone, wpar unused
    double wpar;
    uint32_t par, v;
};

struct AlphaKey {  // a candidate's place in its row
    uint64_t a, w;  // one_tree_ordered(alpha), one_tree_ordered(w)
    uint32_t j;
};

__host__ __device__ inline double alpha_weight(float d, double pi_i, double pi_j) { return (double)d + (pi_i + pi_j); }
__host__ __device__ inline double alpha_max(double a, double b) { return a < b ? b : a; }
// alpha(r, j) = alpha(j, r) from w(r, j), w(r, b) and whether j is one of the root's two neighbours
__host__ __device__ inline double alpha_of_root(double w_rj, double w_rb, bool is_nb) { return is_nb ? 0.0 : w_rj - w_rb; }
__host__ __device__ inline bool alpha_key_less(const AlphaKey &x, const AlphaKey &y)
{
    return x.a < y.a || (x.a == y.a && (x.w < y.w || (x.w == y.w && x.j < y.j)));
}

// ---- the sequential statement (host functions): D is float(uint32_t a, uint32_t b), a != b ----

// §4.29's 1-tree under pi, n >= 3: parents (kOneTreeNone for Prim's start and the root) and the root's neighbours in the order chosen
template <class D>
inline void alpha_tree_host(D d_of, const double *pi, uint32_t n, uint32_t s, uint32_t *par, uint32_t nb[2])
{
    const uint32_t start = s == 0u ? 1u : 0u;
    const double inf = __builtin_huge_val();
    std::vector<double> key(n, inf);
    std::vector<char> in(n, 0);
    for (uint32_t v = 0; v < n; ++v) par[v] = kOneTreeNone;
    key[start] = 0.0;
    in[s] = 1;
    for (uint32_t r = 0; r + 1u < n; ++r) {
        uint32_t u = kOneTreeNone;
        for (uint32_t v = 0; v < n; ++v)
            if (!in[v] && (u == kOneTreeNone || key[v] < key[u])) u = v;
        in[u] = 1;
        for (uint32_t v = 0; v < n; ++v) {
            if (in[v]) continue;
            const double w = alpha_weight(d_of(u, v), pi[u], pi[v]);
            if (w < key[v]) {
                key[v] = w;
                par[v] = u;
            }
        }
    }
    nb[0] = nb[1] = kOneTreeNone;
    for (int e = 0; e < 2; ++e) {
        double bw = 0.0;
        for (uint32_t v = 0; v < n; ++v) {
            if (v == s || v == nb[0]) continue;
            const double w = alpha_weight(d_of(s, v), pi[s], pi[v]);
            if (nb[e] == kOneTreeNone || w < bw) {
                bw = w;
                nb[e] = v;
            }
        }
    }
}

// The tree by position (by_pos[v]) and in level order (by_level: depth ascending from Prim's start, position order within a level;
// level L is by_level[level_at[L] .. level_at[L + 1])).  false: par is no tree over the positions other than s.
template <class D>
inline bool alpha_levels_host(D d_of, const double *pi, const uint32_t *par, uint32_t n, uint32_t s, std::vector<AlphaNode> &by_pos,
                              std::vector<AlphaNode> &by_level, std::vector<uint32_t> &level_at)
{
    const uint32_t start = s == 0u ? 1u : 0u, unknown = 0xFFFFFFFFu;
    std::vector<uint32_t> depth(n, unknown), stack;
    depth[start] = 0u;
    uint32_t levels = 1u;
    for (uint32_t v = 0; v < n; ++v) {
        if (v == s) continue;
        uint32_t u = v;
        stack.clear();
        while (depth[u] == unknown) {
            stack.push_back(u);
            u = par[u];
            if (u >= n || u == s || stack.size() > n) return false;
        }
        while (!stack.empty()) {
            const uint32_t t = stack.back();
            stack.pop_back();
            depth[t] = depth[par[t]] + 1u;
            if (depth[t] + 1u > levels) levels = depth[t] + 1u;
        }
    }
    by_pos.assign(n, AlphaNode{0.0, kOneTreeNone, 0u});
    level_at.assign((size_t)levels + 1u, 0u);
    for (uint32_t v = 0; v < n; ++v) {
        by_pos[v].v = v;
        if (v == s) continue;
        ++level_at[depth[v] + 1u];
        if (v != start) {
            by_pos[v].par = par[v];
            by_pos[v].wpar = alpha_weight(d_of(v, par[v]), pi[v], pi[par[v]]);
        }
    }
    for (uint32_t L = 0; L < levels; ++L) level_at[L + 1u] += level_at[L];
    by_level.assign(n - 1u, AlphaNode{0.0, kOneTreeNone, 0u});
    std::vector<uint32_t> at(level_at.begin(), level_at.end() - 1);
    for (uint32_t v = 0; v < n; ++v)
        if (v != s) by_level[at[depth[v]]++] = by_pos[v];
    return true;
}

// Source i: w(i, .) into wrow and alpha(i, .) into val (both n doubles; entry i of either is not a candidate's).  The source climbs its
// own path to Prim's start, then the levels are swept, each position taking max(beta[parent], w(position, parent)).
template <class D>
inline void alpha_row_host(D d_of, const double *pi, uint32_t n, uint32_t s, const uint32_t nb[2], const std::vector<AlphaNode> &by_pos,
                           const std::vector<AlphaNode> &by_level, uint32_t i, double *val, double *wrow, char *set)
{
    for (uint32_t v = 0; v < n; ++v) {
        wrow[v] = v == i ? 0.0 : alpha_weight(d_of(i, v), pi[i], pi[v]);
        set[v] = 0;
    }
    if (i == s) {
        const double w_rb = wrow[nb[1]];
        for (uint32_t v = 0; v < n; ++v) val[v] = alpha_of_root(wrow[v], w_rb, v == nb[0] || v == nb[1]);
        return;
    }
    double b = -__builtin_huge_val();
    val[i] = b;
    set[i] = 1;
    for (uint32_t v = i; by_pos[v].par != kOneTreeNone;) {
        b = alpha_max(b, by_pos[v].wpar);
        v = by_pos[v].par;
        val[v] = b;
        set[v] = 1;
    }
    for (const AlphaNode &r : by_level)
        if (!set[r.v]) val[r.v] = alpha_max(val[r.par], r.wpar);  // (its parent is a level up: set)
    const double w_rb = alpha_weight(d_of(s, nb[1]), pi[s], pi[nb[1]]);
    for (uint32_t v = 0; v < n; ++v) {
        if (v == i) continue;
        val[v] = v == s ? alpha_of_root(wrow[s], w_rb, i == nb[0] || i == nb[1]) : wrow[v] - val[v];
    }
}

// the kk first of row i by (alpha, w, position)
inline void alpha_select_host(const double *val, const double *wrow, uint32_t n, uint32_t i, uint32_t kk, uint32_t *out_cand, double *out_alpha)
{
    std::vector<AlphaKey> keys;
    keys.reserve(n);
    for (uint32_t v = 0; v < n; ++v)
        if (v != i) keys.push_back(AlphaKey{one_tree_ordered(val[v]), one_tree_ordered(wrow[v]), v});
    std::partial_sort(keys.begin(), keys.begin() + kk, keys.end(), alpha_key_less);
    for (uint32_t r = 0; r < kk; ++r) {
        out_cand[r] = keys[r].j;
        if (out_alpha) out_alpha[r] = val[keys[r].j];
    }
}

// n >= 3, 1 <= kk <= n - 1: every row.  false: never (the tree built here is a tree)
template <class D>
inline bool alpha_candidates_seq(D d_of, const double *pi, uint32_t n, uint32_t s, uint32_t kk, uint32_t *out_cand, double *out_alpha,
                                 uint32_t *out_parent, uint32_t *out_root_nb)
{
    std::vector<uint32_t> par(n), level_at;
    std::vector<AlphaNode> by_pos, by_level;
    uint32_t nb[2];
    alpha_tree_host(d_of, pi, n, s, par.data(), nb);
    if (!alpha_levels_host(d_of, pi, par.data(), n, s, by_pos, by_level, level_at)) return false;
    std::vector<double> val(n), wrow(n);
    std::vector<char> set(n);
    for (uint32_t i = 0; i < n; ++i) {
        alpha_row_host(d_of, pi, n, s, nb, by_pos, by_level, i, val.data(), wrow.data(), set.data());
        alpha_select_host(val.data(), wrow.data(), n, i, kk, out_cand + (size_t)i * kk, out_alpha ? out_alpha + (size_t)i * kk : nullptr);
    }
    if (out_parent)
        for (uint32_t v = 0; v < n; ++v) out_parent[v] = par[v];
    if (out_root_nb) {
        out_root_nb[0] = nb[0];
        out_root_nb[1] = nb[1];
    }
    return true;
}
}  // namespace tl
