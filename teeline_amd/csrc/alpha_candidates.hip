// alpha_candidates.hip — alpha-nearness candidate lists (alpha_spec.h): one workgroup per source city i, its row
// resident in the CU's LDS; the n x n table never exists in memory.
//
//   k_alpha_rows  In LDS: w(i, .) and beta(i, .) — later alpha(i, .) — of every position, 16 n bytes.  The 1-tree (built by ONE
//                 iteration of k_one_tree_ascent under the given pi), its parent weights and its level order are prepared once per
//                 call and read through L2 by every workgroup.
//                   1. w(i, v) for every v; beta unset (NaN: no beta is one).
//                   2. the source climbs its own path to Prim's start (one lane: beta of an ancestor is the largest w below it on the
//                      path), then the workgroup sweeps the levels, each position not on the path taking max(beta[parent],
//                      w(position, parent)): one barrier a level, the tree's depth of them.
//                   3. alpha = w - beta in place; the root's column and the root's own row by alpha_of_root.
//                   4. the k' smallest (ordered alpha, ordered w, position) — a 160-bit compare — one workgroup argmin each: through
//                      the wave by shuffles, then one LDS slot per wave, double-buffered by the round's parity, so a round has ONE
//                      barrier.  Round r takes the least key above round r - 1's.
#include "alpha_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kAlMaxThreads = 1024;
constexpr int kAlMaxWaves = kAlMaxThreads / 64;

struct alignas(8) AlSlot {
    uint64_t a, w;
    uint32_t j, pad_;
};

__device__ __forceinline__ uint64_t al_shfl_xor(uint64_t v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(kAlMaxThreads) void k_alpha_rows(AlphaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char al_lds[];
    __shared__ AlSlot slot[2][kAlMaxWaves];
    const uint32_t i = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, waves = nt >> 6, n = A.n, s = A.root;
    if (i >= n) return;  // (the whole workgroup)
    double *val = reinterpret_cast<double *>(al_lds);
    double *wrow = val + n;
    const bool i_is_nb = i == A.nb0 || i == A.nb1;

    auto d_of = [&](uint32_t u, float2 xu, uint32_t v) -> float {
        if (DM) return A.dm_full[(size_t)u * n + v];
        return dist(xu, A.xy[v]);
    };

    // 1. the source's weights
    {
        const double pi_i = A.pi[i];
        float2 xi = make_float2(0.f, 0.f);
        if (!DM) xi = A.xy[i];
        const double unset = __builtin_nan("");
        for (uint32_t v = tid; v < n; v += nt) {
            wrow[v] = v == i ? 0.0 : alpha_weight(d_of(i, xi, v), pi_i, A.pi[v]);
            val[v] = unset;
        }
    }
    TL_SYNC();

    if (i == s) {
        const double w_rb = wrow[A.nb1];
        for (uint32_t v = tid; v < n; v += nt) val[v] = alpha_of_root(wrow[v], w_rb, v == A.nb0 || v == A.nb1);
    } else {
        // 2. beta: the source's path, then the levels
        if (tid == 0) {
            double b = -__builtin_huge_val();
            val[i] = b;
            AlphaNode r = A.by_pos[i];
            for (uint32_t step = 0; r.par < n && step < n; ++step) {  // (step < n: a tree's path ends; a broken table cannot spin)
                b = alpha_max(b, r.wpar);
                val[r.par] = b;
                r = A.by_pos[r.par];
            }
        }
        TL_SYNC();
        const uint32_t levels = A.levels;
        uint32_t lo = A.level_at[levels > 1u ? 1u : 0u], hi = A.level_at[levels > 1u ? 2u : 0u];
        for (uint32_t L = 1; L < levels; ++L) {
            const uint32_t nxt = A.level_at[L + 2u <= levels ? L + 2u : levels];  // (the next level's end, asked for before this level's barrier)
            for (uint32_t idx = lo + tid; idx < hi; idx += nt) {
                const AlphaNode r = A.by_level[idx];
                if (r.v < n && r.par < n && __builtin_isnan(val[r.v])) val[r.v] = alpha_max(val[r.par], r.wpar);
            }
            TL_SYNC();
            lo = hi;
            hi = nxt;
        }
        // 3. alpha in place
        double w_rb;
        {
            float2 xs = make_float2(0.f, 0.f);
            if (!DM) xs = A.xy[s];
            w_rb = alpha_weight(d_of(s, xs, A.nb1), A.pi[s], A.pi[A.nb1]);
        }
        for (uint32_t v = tid; v < n; v += nt) {
            if (v == i) continue;
            val[v] = v == s ? alpha_of_root(wrow[s], w_rb, i_is_nb) : wrow[v] - val[v];
        }
    }
    TL_SYNC();

    // 4. the k' first of the row
    AlphaKey prev{0ull, 0ull, 0u};
    for (uint32_t r = 0; r < A.kk; ++r) {
        AlphaKey best{~(uint64_t)0, ~(uint64_t)0, ~0u};
        for (uint32_t v = tid; v < n; v += nt) {
            if (v == i) continue;
            const AlphaKey k{one_tree_ordered(val[v]), one_tree_ordered(wrow[v]), v};
            if (r != 0u && !alpha_key_less(prev, k)) continue;
            if (alpha_key_less(k, best)) best = k;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const AlphaKey o{al_shfl_xor(best.a, off), al_shfl_xor(best.w, off), (uint32_t)__shfl_xor((int)best.j, off, 64)};
            if (alpha_key_less(o, best)) best = o;
        }
        if (lane == 0) slot[r & 1u][wave] = AlSlot{best.a, best.w, best.j, 0u};
        TL_SYNC();
        AlSlot m = slot[r & 1u][0];
        for (uint32_t w = 1; w < waves; ++w) {
            const AlSlot o = slot[r & 1u][w];
            if (alpha_key_less(AlphaKey{o.a, o.w, o.j}, AlphaKey{m.a, m.w, m.j})) m = o;
        }
        if (m.j >= n) break;  // (every lane the same slot values: fewer than kk candidates cannot happen for kk <= n - 1)
        if (tid == 0) {
            A.out_cand[(size_t)i * A.kk + r] = m.j;
            if (A.out_alpha) A.out_alpha[(size_t)i * A.kk + r] = val[m.j];
        }
        prev = AlphaKey{m.a, m.w, m.j};
    }
}

size_t alpha_rows_lds_bytes(uint32_t n) { return (((size_t)n * 16u) + 15u) & ~(size_t)15; }

uint32_t alpha_rows_max_n(int lds_bytes)
{
    if (lds_bytes <= 1024) return 0u;
    const size_t m = ((size_t)lds_bytes - 1024u) / 16u;  // 1024: the static slots
    return m > 65535u ? 65535u : (uint32_t)m;
}

int alpha_rows_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 64u ? 64 : t > 256u ? 256 : (int)t;
}

hipError_t launch_alpha_rows(const AlphaArgs &A, int threads, hipStream_t s)
{
    const void *k = A.dm_full ? (const void *)k_alpha_rows<true> : (const void *)k_alpha_rows<false>;
    hipError_t e = allow_max_lds(k);
    if (e != hipSuccess) return e;
    if (A.dm_full) hipLaunchKernelGGL(k_alpha_rows<true>, dim3(A.n), dim3(threads), alpha_rows_lds_bytes(A.n), s, A);
    else hipLaunchKernelGGL(k_alpha_rows<false>, dim3(A.n), dim3(threads), alpha_rows_lds_bytes(A.n), s, A);
    return hipGetLastError();
}

}  // namespace tl
