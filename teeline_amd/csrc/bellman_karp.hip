// bellman_karp.hip — the Bellman-Held-Karp exact solver (reference: src/tsp/bellman_karp.rs:24-165), DESIGN.md §4.14.
// k = n - 1 cities are in the subsets, `last` = k is where every path starts.  The table is MASK-major: row S holds the 32 floats
// opt[S][0..31] (128 bytes, one coalesced read or write of half a wave), so that the row of R = S \ c, which every term of
// opt[S][c] reads, is ONE cache line; the reference's city-major opt[c][S] turns the same read into 2^k-strided gathers.
//   k_bhk_init    the (k + 1)^2 distances, once, as a 32 x 32 f32 square in the workspace (dist() of tl_device.h in coordinate form —
//                 the matrix builder's bits — or the packed triangle), and the rows of the empty set and of the k singletons
//                 (:39-47: f32::MAX everywhere, opt[1 << i][i] = d(i, last));
//   k_bhk_layer   one launch per subset size p = 2..k (:89-120; a layer reads only the layer below, so the launch boundary is the
//                 only synchronisation).  Half a wave owns a subset S at a time and writes its whole row, f32::MAX where c is not
//                 in S — so no pass over the table has to fill it first.  Per c in S: lane i loads opt[R][i], adds d(i, c), keeps
//                 f32::MAX unless i is in R and the term is < f32::MAX (a NaN term, one that rounds to MAX or inf: never taken,
//                 as under the reference's strict `<` from best = MAX), and five xor-exchanges leave min in every lane.  No
//                 partial minimum is ever NaN, so the tree's value is the sequential scan's — up to the SIGN of a zero, which
//                 neither the route nor the cost can show.  The subsets of a layer are walked in numeric order: a half-wave
//                 unranks the first of its chunk from the binomial table (combinadic) and steps with Gosper's successor.
//   k_bhk_walk    one wave: the optimum (:65-75), either walk (:122-156, or the exact walk of TL_FLAG_BHK_EXACT_WALK), tour_length
//                 of the route as it stands (closing edge first, sequential f32, d(p, p) = 0) and whether it is a permutation.
//                 Lanes over j, ballot, first set bit; the table never leaves the device.
// Every table index is 64-bit: at k = 25 a row's BYTE offset passes 4 GiB.
#include "tl_kernels.h"

#include <cfloat>

namespace tl {

namespace {

constexpr int kBhkLayerThreads = 256;  // 8 half-waves
constexpr uint32_t kBhkRow = 32;       // floats per table row

__device__ __forceinline__ float min_lt(float a, float b) { return a < b ? a : b; }

// min over the 32 lanes of this half of the wave (offsets < 32 never leave it)
__device__ __forceinline__ float half_wave_min(float v)
{
    v = min_lt(v, __shfl_xor(v, 16));
    v = min_lt(v, __shfl_xor(v, 8));
    v = min_lt(v, __shfl_xor(v, 4));
    v = min_lt(v, __shfl_xor(v, 2));
    v = min_lt(v, __shfl_xor(v, 1));
    return v;
}

__global__ __launch_bounds__(1024) void k_bhk_init(const float2 *__restrict__ xy, const float *__restrict__ dm, uint32_t n,
                                                   float *__restrict__ dsq, float *__restrict__ opt)
{
    __shared__ float D[kBhkRow * kBhkRow];
    const uint32_t tid = threadIdx.x, a = tid >> 5, b = tid & 31u, k = n - 1;
    float d = 0.0f;  // the diagonal (distance_by_pos of a position with itself) and everything outside the instance
    if (a < n && b < n && a != b) d = dm ? dm_lookup(dm, a, b) : (a > b ? dist(xy[a], xy[b]) : dist(xy[b], xy[a]));
    D[tid] = d;
    dsq[tid] = d;
    TL_SYNC();
    // rows 0 (the empty set) and 1 << i: thread (a, b) writes entry b of row a's set, a = 0 for the empty set, a = i + 1 otherwise
    if (a <= k) {
        const uint64_t S = a ? (uint64_t)1 << (a - 1) : 0;
        opt[S * kBhkRow + b] = (a && b == a - 1) ? D[b * kBhkRow + k] : FLT_MAX;
    }
}

// The rank-th p-subset of {0..k-1} in numeric (colexicographic) order: the largest element a with C(a, p) <= rank first.
__host__ __device__ inline uint32_t bhk_unrank(const uint32_t *binom, uint32_t k, uint32_t p, uint32_t rank)
{
    uint32_t S = 0, a = k;
    for (uint32_t b = p; b > 0; --b) {
        do --a;
        while (binom[a * kBhkRow + b] > rank);
        S |= 1u << a;
        rank -= binom[a * kBhkRow + b];
    }
    return S;
}

// Gosper: the next larger number with the same number of set bits (x != 0)
__host__ __device__ inline uint32_t bhk_next(uint32_t x)
{
    const uint32_t t = x | (x - 1u);
    return (t + 1u) | (((~t & (0u - ~t)) - 1u) >> (__builtin_ctz(x) + 1));
}

// binom: C(a, b) at [a * 32 + b], a, b < 32 (0 where b > a).  count = C(k, p) subsets, `per` of them per half-wave.
__global__ __launch_bounds__(kBhkLayerThreads) void k_bhk_layer(float *__restrict__ opt, const float *__restrict__ dsq,
                                                                const uint32_t *__restrict__ binom_g, uint32_t k, uint32_t p, uint32_t count,
                                                                uint32_t per)
{
    __shared__ float D[kBhkRow * kBhkRow];
    __shared__ uint32_t binom[kBhkRow * kBhkRow];
    for (uint32_t t = threadIdx.x; t < kBhkRow * kBhkRow; t += kBhkLayerThreads) {
        D[t] = dsq[t];
        binom[t] = binom_g[t];
    }
    TL_SYNC();
    const uint32_t lane = threadIdx.x & 31u;
    const uint64_t hw = (uint64_t)blockIdx.x * (kBhkLayerThreads / 32) + (threadIdx.x >> 5);
    const uint64_t r0 = hw * per;
    if (r0 >= count) return;  // a whole half of the wave leaves: the exchanges of the other half never read it
    const uint32_t r1 = (uint32_t)(r0 + per < count ? r0 + per : count);
    uint32_t S = bhk_unrank(binom, k, p, (uint32_t)r0);
    for (uint32_t r = (uint32_t)r0; r < r1; ++r) {
        float mine = FLT_MAX;  // opt[S][lane]
        for (uint32_t m = S; m; m &= m - 1u) {
            const uint32_t c = (uint32_t)__builtin_ctz(m), R = S ^ (1u << c);
            const float t = opt[(uint64_t)R * kBhkRow + lane] + D[c * kBhkRow + lane];
            const float v = half_wave_min((((R >> lane) & 1u) && t < FLT_MAX) ? t : FLT_MAX);
            if (lane == c) mine = v;
        }
        opt[(uint64_t)S * kBhkRow + lane] = mine;
        S = bhk_next(S);
    }
}

// :158-165, all in f32; a NaN on either side makes diff NaN and the answer false
__device__ __forceinline__ bool bhk_approx(float x1, float x2)
{
    const float diff = fabsf(x1 - x2);
    const float scale = fmaxf(fmaxf(fabsf(x1), fabsf(x2)), 1.0f);
    return diff <= scale * 1e-4f;
}

// out_pos[n]; out_f[0] = tour_length(out_pos), out_f[1] = optimal; out_u[0] = is_tour
__global__ __launch_bounds__(64) void k_bhk_walk(const float *__restrict__ opt, const float *__restrict__ dsq, uint32_t n, uint32_t exact,
                                                 uint32_t *__restrict__ out_pos, float *__restrict__ out_f, uint32_t *__restrict__ out_u)
{
    __shared__ float D[kBhkRow * kBhkRow];
    __shared__ uint32_t route[kBhkRow];
    const uint32_t j = threadIdx.x, k = n - 1;
    for (uint32_t t = j; t < kBhkRow * kBhkRow; t += 64) D[t] = dsq[t];
    if (j < kBhkRow) route[j] = 0u;
    TL_SYNC();
    const uint32_t full = (uint32_t)(((uint64_t)1 << k) - 1u);
    // the optimum: every admitted term is a number (both operands are < MAX, so no inf - inf), and min from MAX over numbers does
    // not depend on the order
    float term = FLT_MAX;
    if (j < k) {
        const float sub = opt[(uint64_t)full * kBhkRow + j], ret = D[j * kBhkRow + k];
        if (sub < FLT_MAX && ret < FLT_MAX) term = min_lt(sub + ret, FLT_MAX);
    }
    float optimal = half_wave_min(term);  // k <= 25: lanes 0..31 hold every term
    optimal = readlane_f(optimal, 0);
    uint32_t unread = full, prev = k;
    if (j == 0) route[0] = k;
    if (exact && optimal < FLT_MAX) {
        float rem = optimal;
        for (uint32_t i = 1; i < n; ++i) {
            bool hit = false;
            float sub = 0.0f;
            if (j < k && ((unread >> j) & 1u)) {
                sub = opt[(uint64_t)unread * kBhkRow + j];
                const float step = D[j * kBhkRow + prev];
                hit = (i > 1 || (sub < FLT_MAX && step < FLT_MAX)) && sub + step == rem;
            }
            const uint64_t b = __builtin_amdgcn_ballot_w64(hit);
            if (!b) break;  // cannot happen: rem is the minimum of exactly these terms
            const uint32_t w = (uint32_t)__builtin_ctzll(b);
            rem = readlane_f(sub, (int)w);
            if (j == 0) route[i] = w;
            unread &= ~(1u << w);
            prev = w;
        }
    } else {
        float left = optimal;
        for (uint32_t i = 1; i < n; ++i) {
            if (left <= 0.0f) break;  // :129
            bool hit = false;
            float step = 0.0f;
            if (j < k) {
                step = D[j * kBhkRow + prev];
                const float cur = opt[(uint64_t)unread * kBhkRow + j] + step;
                hit = ((unread >> j) & 1u) && bhk_approx(left, cur);
            }
            const uint64_t b = __builtin_amdgcn_ballot_w64(hit);
            if (!b) {  // route[i] stays 0, and is the next step's previous position (:135)
                prev = 0u;
                continue;
            }
            const uint32_t w = (uint32_t)__builtin_ctzll(b);
            left -= readlane_f(step, (int)w);
            if (j == 0) route[i] = w;
            unread &= ~(1u << w);
            prev = w;
        }
    }
    TL_SYNC();
    if (j == 0) {
        float total = D[route[n - 1] * kBhkRow + route[0]];
        uint32_t seen = 0;
        for (uint32_t a = 0; a < n; ++a) {
            if (a + 1 < n) total += D[route[a] * kBhkRow + route[a + 1]];
            seen |= 1u << route[a];
            out_pos[a] = route[a];
        }
        out_f[0] = total;
        out_f[1] = optimal;
        out_u[0] = seen == (uint32_t)(((uint64_t)1 << n) - 1u) ? 1u : 0u;
    }
}

}  // namespace

size_t bhk_table_bytes(uint32_t n) { return ((size_t)1 << (n - 1)) * kBhkRow * sizeof(float); }

BhkWs bhk_ws_layout(void *ws, uint32_t n)
{
    BhkWs w;
    unsigned char *p = (unsigned char *)ws;
    w.dsq = (float *)p;
    p += kBhkRow * kBhkRow * sizeof(float);
    w.binom = (uint32_t *)p;
    p += kBhkRow * kBhkRow * sizeof(uint32_t);
    w.out_f = (float *)p;
    w.out_u = (uint32_t *)(p + 8);
    p += 256;
    w.opt = (float *)p;
    (void)n;
    return w;
}

size_t bhk_ws_bytes(uint32_t n) { return 2 * kBhkRow * kBhkRow * 4 + 256 + bhk_table_bytes(n); }

void bhk_binomials(uint32_t *out)
{
    for (uint32_t a = 0; a < kBhkRow; ++a)
        for (uint32_t b = 0; b < kBhkRow; ++b)
            out[a * kBhkRow + b] = b == 0 ? 1u : (a == 0 ? 0u : out[(a - 1) * kBhkRow + b - 1] + out[(a - 1) * kBhkRow + b]);
}

hipError_t launch_bhk_init(const BhkWs &w, const float2 *xy, const float *dm, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_bhk_init, dim3(1), dim3(1024), 0, s, xy, dm, n, w.dsq, w.opt);
    return hipGetLastError();
}

hipError_t launch_bhk_layer(const BhkWs &w, uint32_t n, uint32_t p, uint32_t count, int cus, hipStream_t s)
{
    // enough half-waves to fill every CU several times over, and no more: a half-wave pays one unranking per chunk
    const uint64_t target = (uint64_t)(cus > 0 ? cus : 256) * 32 * 2 * 4;
    const uint32_t per = (uint32_t)((count + target - 1) / target);
    const uint32_t halves = (count + per - 1) / per;
    const uint32_t blocks = (halves + kBhkLayerThreads / 32 - 1) / (kBhkLayerThreads / 32);
    hipLaunchKernelGGL(k_bhk_layer, dim3(blocks), dim3(kBhkLayerThreads), 0, s, w.opt, w.dsq, w.binom, n - 1, p, count, per);
    return hipGetLastError();
}

hipError_t launch_bhk_walk(const BhkWs &w, uint32_t n, bool exact, uint32_t *out_pos, hipStream_t s)
{
    hipLaunchKernelGGL(k_bhk_walk, dim3(1), dim3(64), 0, s, w.opt, w.dsq, n, exact ? 1u : 0u, out_pos, w.out_f, w.out_u);
    return hipGetLastError();
}

}  // namespace tl
