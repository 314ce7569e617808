// one_tree_bound.hip — the Held-Karp lower bound (one_tree_spec.h): J independent jobs (option sets on one
// problem: root, step factor, patience), the job a grid dimension, one workgroup per job, a span of ascent iterations per launch.
//
//   k_one_tree_ascent  the iterations [S.k, S.k + span) of a job.  In the CU's LDS: key (f64), pi (f64), parent and degree of every
//                      position, 24 n bytes.  An iteration is one 1-tree:
//                        1. the two root edges: two workgroup argmins over w(s, v).  pi is summed in position order by one lane
//                           of the last wave, ceil(n / (n - 2)) terms a Prim round beside its sweep, and published through LDS
//                           behind the last round's barrier: no serial O(n) chain anywhere.
//                        2. Prim over the other positions in k_chr_prim's shape: a thread owns the positions tid, tid + nt, ..;
//                           round r's update pass and round r + 1's argmin are ONE sweep over them; the least (ordered f64 key,
//                           position) — a 96-bit compare — goes through the wave by shuffles, then through one 16-byte LDS slot
//                           per wave, double-buffered by the argmin's parity, so a round has ONE barrier.  Every lane carries the
//                           running sum of the taken keys (the winner's key comes back out of the slot), so the sequential f64
//                           sum costs nothing extra.  The taken position's owner counts the tree edge into both degrees: one
//                           thread a round, a barrier between two rounds.
//                        3. g = degree - 2, the sum of squares through the wave and one LDS word; then one_tree_decide (every
//                           lane the same scalars), the best pi and parents to the workspace where L is a new best, the log row,
//                           pi_i += t g_i.
//                      pi, lambda, stall, best: loaded from the workspace at the launch's start, stored at its end.  A job that has
//                      stopped returns at once, so a finished job costs a launch nothing and disturbs nobody.
#include "one_tree_spec.h"
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kOtMaxThreads = 1024;
constexpr int kOtMaxWaves = kOtMaxThreads / 64;

struct alignas(16) OtSlot {
    uint64_t k;
    uint32_t p, pad_;
};

__device__ __forceinline__ bool ot_less(uint64_t ak, uint32_t ap, uint64_t bk, uint32_t bp) { return ak < bk || (ak == bk && ap < bp); }

__device__ __forceinline__ uint64_t ot_shfl_xor(uint64_t v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t ot_uniform(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// the workgroup's least (k, p), to every lane; ONE barrier.  Consecutive calls alternate `parity`.
__device__ __forceinline__ void ot_argmin(uint64_t &k, uint32_t &p, OtSlot (*slot)[kOtMaxWaves], uint32_t parity, uint32_t lane, uint32_t wave, uint32_t waves)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = ot_shfl_xor(k, off);
        const uint32_t op = (uint32_t)__shfl_xor((int)p, off, 64);
        if (ot_less(ok, op, k, p)) {
            k = ok;
            p = op;
        }
    }
    if (lane == 0) slot[parity][wave] = OtSlot{k, p, 0u};
    TL_SYNC();
    OtSlot m = slot[parity][0];
    for (uint32_t w = 1; w < waves; ++w) {
        const OtSlot o = slot[parity][w];
        if (ot_less(o.k, o.p, m.k, m.p)) m = o;
    }
    k = ot_uniform(m.k);
    p = (uint32_t)__builtin_amdgcn_readfirstlane((int)m.p);
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(kOtMaxThreads) void k_one_tree_ascent(OneTreeArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ot_lds[];
    __shared__ OtSlot slot[2][kOtMaxWaves];
    __shared__ uint32_t sh_g2[2];
    __shared__ double sh_P;
    const uint32_t job = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6, waves = nt >> 6, n = A.n;
    const OneTreeJob J = A.jobs[job];
    OneTreeState S = A.state[job];
    if (S.stop != kOneTreeStopNone) return;  // (the whole workgroup)
    double *key = reinterpret_cast<double *>(ot_lds);
    double *pi = key + n;
    uint32_t *par = reinterpret_cast<uint32_t *>(pi + n);
    uint32_t *deg = par + n;
    double *pi_g = A.pi + (size_t)job * n, *best_pi_g = A.best_pi + (size_t)job * n;
    uint32_t *best_par_g = A.best_par + (size_t)job * n, *tour_par_g = A.tour_par + (size_t)job * n;
    const uint32_t s = J.root, start = s == 0u ? 1u : 0u;
    const uint32_t k_end = J.iterations - S.k < A.span ? J.iterations : S.k + A.span;
    const double inf = __builtin_huge_val();
    uint32_t parity = 0u;
    for (uint32_t v = tid; v < n; v += nt) pi[v] = pi_g[v];
    TL_SYNC();

    auto d_of = [&](uint32_t u, float2 xu, uint32_t v) -> float {
        if (DM) return A.dm_full[(size_t)u * n + v];
        return dist(xu, A.xy[v]);
    };

    while (S.stop == kOneTreeStopNone && S.k < k_end) {
        const uint32_t it = S.k;
        uint64_t mine = 0;  // bit k: position tid + nt k is in the tree (or is the root)
        {
            uint32_t k = 0;
            for (uint32_t v = tid; v < n; v += nt, ++k) {
                key[v] = v == start ? 0.0 : inf;
                par[v] = kOneTreeNone;
                deg[v] = 0u;
                if (v == s) mine |= (uint64_t)1 << k;
            }
        }
        if (tid == 0) sh_g2[it & 1u] = 0u;

        // 1. the root's two edges, the lower position among equals; the second the same way from the rest
        const double pi_s = pi[s];
        float2 xs = make_float2(0.f, 0.f);
        if (!DM) xs = A.xy[s];
        uint32_t nb[2] = {kOneTreeNone, kOneTreeNone};
        double wnb[2];
        for (int e = 0; e < 2; ++e) {
            uint64_t bk = ~(uint64_t)0;
            uint32_t bp = ~0u;
            for (uint32_t v = tid; v < n; v += nt) {
                if (v == s || v == nb[0]) continue;
                const double w = (double)d_of(s, xs, v) + (pi_s + pi[v]);
                const uint64_t ok = one_tree_ordered(w);
                if (ot_less(ok, v, bk, bp)) {
                    bk = ok;
                    bp = v;
                }
            }
            ot_argmin(bk, bp, slot, parity, lane, wave, waves);
            parity ^= 1u;
            nb[e] = bp;
            wnb[e] = one_tree_unordered(bk);
        }
        // pi summed in position order by ONE lane, a few terms a round beside the sweep (pi does not change while the tree grows)
        double P = 0.0;
        uint32_t pv = 0;
        const uint32_t pchunk = (n + (n - 3u)) / (n - 2u);  // n - 2 rounds have a sweep: ceil(n / (n - 2)) terms each cover all n

        // 2. Prim over the positions other than s
        double sum = 0.0, ku = 0.0;
        uint32_t u = start;
        for (uint32_t r = 0;; ++r) {
            sum = sum + ku;
            if (u % nt == tid) {  // u's owner; the degrees have one writer a round, a barrier between two rounds
                mine |= (uint64_t)1 << (u / nt);
                const uint32_t p = par[u];
                if (p != kOneTreeNone) {
                    deg[u] += 1u;
                    deg[p] += 1u;
                }
            }
            if (r + 2u == n) break;
            if (tid == nt - 1u)
                for (uint32_t c = 0; c < pchunk && pv < n; ++c, ++pv) P = P + pi[pv];
            const double pu = pi[u];
            float2 xu = make_float2(0.f, 0.f);
            if (!DM) xu = A.xy[u];
            uint64_t bk = ~(uint64_t)0;
            uint32_t bp = ~0u, k = 0;
            for (uint32_t v = tid; v < n; v += nt, ++k) {
                if ((mine >> k) & 1u) continue;
                const double w = (double)d_of(u, xu, v) + (pu + pi[v]);
                double kv = key[v];
                if (w < kv) {
                    kv = w;
                    key[v] = w;
                    par[v] = u;
                }
                const uint64_t ok = one_tree_ordered(kv);
                if (ot_less(ok, v, bk, bp)) {
                    bk = ok;
                    bp = v;
                }
            }
            ot_argmin(bk, bp, slot, parity, lane, wave, waves);
            parity ^= 1u;
            u = bp;
            ku = one_tree_unordered(bk);
        }
        if (tid == nt - 1u) sh_P = P;
        TL_SYNC();

        // 3. the value, the subgradient, the step
        P = sh_P;
        const double L = ((sum + wnb[0]) + wnb[1]) - 2.0 * P;
        uint32_t g2 = 0u;
        for (uint32_t v = tid; v < n; v += nt) {
            int dg = (int)deg[v] + (v == nb[0] ? 1 : 0) + (v == nb[1] ? 1 : 0);
            if (v == s) dg = 2;
            const int g = dg - 2;
            deg[v] = (uint32_t)g;
            g2 += (uint32_t)(g * g);
        }
        for (int off = 32; off > 0; off >>= 1) g2 += (uint32_t)__shfl_xor((int)g2, off, 64);
        if (lane == 0 && g2) atomicAdd(&sh_g2[it & 1u], g2);
        TL_SYNC();
        g2 = sh_g2[it & 1u];
        double t;
        const bool improved = one_tree_decide(S, J, L, g2, &t);
        if (improved) {
            S.best_nb[0] = nb[0];
            S.best_nb[1] = nb[1];
        }
        if (S.is_tour) {
            S.tour_nb[0] = nb[0];
            S.tour_nb[1] = nb[1];
        }
        if (A.log && tid == 0 && it < A.log_cap) {
            double *row = A.log + ((size_t)job * A.log_cap + it) * 3u;
            row[0] = L;
            row[1] = (double)g2;
            row[2] = S.lambda;
        }
        for (uint32_t v = tid; v < n; v += nt) {
            const double p = pi[v];
            const uint32_t q = par[v];
            if (improved) {
                best_pi_g[v] = p;
                best_par_g[v] = q;
            }
            if (S.is_tour) tour_par_g[v] = q;
            if (S.stop == kOneTreeStopNone) pi[v] = p + t * (double)(int)deg[v];
        }
        TL_SYNC();
    }
    for (uint32_t v = tid; v < n; v += nt) pi_g[v] = pi[v];
    if (tid == 0) A.state[job] = S;
}

size_t one_tree_lds_bytes(uint32_t n) { return (((size_t)n * 24u) + 15u) & ~(size_t)15; }

uint32_t one_tree_max_n(int lds_bytes)
{
    if (lds_bytes <= 1024) return 0u;
    const size_t m = ((size_t)lds_bytes - 1024u) / 24u;  // 1024: the static slots, as k_chr_prim reserves them
    return m > 65535u ? 65535u : (uint32_t)m;
}

int one_tree_threads(uint32_t n)
{
    const uint32_t t = (n + 63u) & ~63u;
    return t < 64u ? 64 : t > (uint32_t)kOtMaxThreads ? kOtMaxThreads : (int)t;
}

hipError_t launch_one_tree_ascent(const OneTreeArgs &A, uint32_t jobs, int threads, hipStream_t s)
{
    const void *k = A.dm_full ? (const void *)k_one_tree_ascent<true> : (const void *)k_one_tree_ascent<false>;
    hipError_t e = allow_max_lds(k);
    if (e != hipSuccess) return e;
    if (A.dm_full) hipLaunchKernelGGL(k_one_tree_ascent<true>, dim3(jobs), dim3(threads), one_tree_lds_bytes(A.n), s, A);
    else hipLaunchKernelGGL(k_one_tree_ascent<false>, dim3(jobs), dim3(threads), one_tree_lds_bytes(A.n), s, A);
    return hipGetLastError();
}

}  // namespace tl
