// two_opt_best_lds.hip — TL_MODE_BEST_SWEEP for many tours at once: one persistent workgroup per descent runs every sweep of
// tlo_two_opt_best (oracle) with the whole state in its CU's LDS — no launch and no global reduction per move, which is all a
// small tour's chip-wide sweep (two_opt_best.hip: k_bs_scan + k_bs_apply, two dependent launches) consists of.
//
//   LDS: P[n_pad] tour-ordered points | rowkey[n_pad] every row's best key as of the last sweep that decided it | tbox[ntile_cap],
//        tmsq[ntile_cap] the L0 tile metadata (build_tile_meta) | one key slot per wave, one control word | perm[n_pad] (16-bit).
//        18 bytes per padded position and 20 per tile of the padded table: n <= 8 768 on 160 KB (two_opt_best_lds_max_n).
//   Sweep: the rows are strided over the waves (row i always belongs to wave i mod waves, so its cache entry has one writer);
//        each row goes through bs_row_decide (two_opt_best_scan.h), the body k_bs_scan runs.  Wave minimum of the packed key
//        (~delta bits << 32 | i << 16 | j), a slot per wave, barrier, every thread takes the minimum of the slots: the argmin of a
//        key does not depend on which wave found it, so the result is the same for every workgroup size.
//   Apply: swap_2opt(i+1, j) on P and perm by the whole workgroup (each thread swaps whole pairs: no thread reads what another
//        writes), barrier, the touched tiles ((lo-1) >> 6 .. hi >> 6) rebuilt one per wave, barrier.  Three barriers per sweep.
//   Counters live in registers: every thread follows the same keys.
#include "tl_kernels.h"
#include "two_opt_best_scan.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kBsLdsMaxWaves = 16;
constexpr size_t kBsLdsTailBytes = (size_t)kBsLdsMaxWaves * 8 + 16;  // the waves' key slots, the control word

struct BsLdsLayout {
    uint32_t n_pad, ntile_cap;
    size_t o_rk, o_box, o_msq, o_key, o_perm, bytes;
    __host__ __device__ explicit BsLdsLayout(uint32_t n)
        : n_pad(((n + 64u + 63u) / 64u) * 64u), ntile_cap((((n_pad >> 6) + 63u) / 64u) * 64u), o_rk((size_t)n_pad * 8), o_box(o_rk + (size_t)n_pad * 8),
          o_msq(o_box + (size_t)ntile_cap * 16), o_key(o_msq + (size_t)ntile_cap * 4), o_perm(o_key + kBsLdsTailBytes), bytes(o_perm + (size_t)n_pad * 2)
    {
    }
};

}  // namespace

__global__ __launch_bounds__(kBsLdsMaxWaves * 64) void k_bs_lds(BestLdsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, d = blockIdx.x;
    const int lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), nwaves = nt >> 6;
    const BsLdsLayout L(n);
    float2 *P = reinterpret_cast<float2 *>(smem);
    unsigned long long *rowkey = reinterpret_cast<unsigned long long *>(smem + L.o_rk);
    float4 *tbox = reinterpret_cast<float4 *>(smem + L.o_box);
    float *tmsq = reinterpret_cast<float *>(smem + L.o_msq);
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(smem + L.o_key);
    uint32_t *bad_init = reinterpret_cast<uint32_t *>(smem + L.o_key + (size_t)kBsLdsMaxWaves * 8);
    uint16_t *perm = reinterpret_cast<uint16_t *>(smem + L.o_perm);

    // ---------------------------------------------------------------- start tour
    if (A.init_mode == TL_INIT_ARRAY) {
        // a device-resident start tour has not been through the host's permutation check (tl_two_opt_batch_dev): an entry >= n
        // would index xy out of bounds, so the descent is refused (status 2, cost NaN, tour untouched), as in the REF_ORDER batch
        const uint32_t *__restrict__ src = A.init + (size_t)d * n;
        if (tid == 0) *bad_init = 0u;
        TL_SYNC();
        bool bad = false;
        for (uint32_t k = tid; k < n; k += nt) {
            const uint32_t v = src[k];
            bad |= v >= n;
            perm[k] = (uint16_t)v;
        }
        if (bad) *bad_init = 1u;
        TL_SYNC();
        if (*bad_init) {
            if (tid == 0) {
                A.out_cost[d] = __builtin_nanf("");
                uint64_t *st = A.out_stats + (size_t)d * TL_STATS_STRIDE;
                for (int q = 0; q < TL_STATS_STRIDE; ++q) st[q] = 0;
                st[3] = 2;
            }
            return;
        }
    } else {
        for (uint32_t k = tid; k < n; k += nt) perm[k] = (uint16_t)k;
        // (the draws go where the points will be: they are not live yet)
        seeded_start_perm(perm, reinterpret_cast<uint16_t *>(smem), n, A.seed + (uint64_t)(A.first + d), tid, nt);
    }
    for (uint32_t k = tid; k < L.ntile_cap; k += nt) {
        const float inf = __builtin_inff();
        tbox[k] = make_float4(inf, inf, -inf, -inf);  // empty box: never live
        tmsq[k] = -1.0f;
    }
    TL_SYNC();
    for (uint32_t k = tid; k < L.n_pad; k += nt) P[k] = k < n ? A.xy[perm[k]] : make_float2(0.f, 0.f);
    TL_SYNC();
    // (the tiles a candidate's column can lie in; a lane of the last one reads P[j + 1] with j + 1 <= n + 62 < n_pad)
    for (uint32_t t = wave; t <= ((n - 2u) >> 6); t += nwaves) build_tile_meta(P, n, t, lane, tbox, tmsq);
    TL_SYNC();

    // ---------------------------------------------------------------- descent
    const uint32_t nrows = n - 3u;  // rows i in [0, n-3); j in [i+2, n-2]
    uint32_t sweeps = 0, moves = 0, status = 0, mv = 0, is = 0, js = 0;
    uint64_t reversed = 0;
    for (;;) {
        unsigned long long best = kNoKey64;
        for (uint32_t i = wave; i < nrows; i += nwaves) {
            const unsigned long long k = bs_row_decide(P, tbox, tmsq, rowkey, n, i, mv, is, js, lane);
            best = k < best ? k : best;
        }
        if (lane == 0) s_key[wave] = best;
        TL_SYNC();
        best = s_key[0];
        for (uint32_t w = 1; w < nwaves; ++w) best = s_key[w] < best ? s_key[w] : best;
        ++sweeps;  // the last sweep finds nothing and counts
        if (best == kNoKey64) break;
        if (sweeps >= A.max_sweeps) {
            status = 1u;
            break;
        }
        is = (uint32_t)((best >> 16) & 0xFFFFu);
        js = (uint32_t)(best & 0xFFFFu);
        mv = 1u;
        const uint32_t lo = is + 1u, hi = js, half = (hi - lo + 1u) >> 1;
        for (uint32_t t = tid; t < half; t += nt) {  // swap_2opt(path, i+1, j)
            const float2 x = P[lo + t], y = P[hi - t];
            P[lo + t] = y;
            P[hi - t] = x;
            const uint16_t u = perm[lo + t], v = perm[hi - t];
            perm[lo + t] = v;
            perm[hi - t] = u;
        }
        TL_SYNC();  // (also: every wave has read the slots before the next sweep writes them)
        for (uint32_t t = ((lo - 1u) >> 6) + wave; t <= (hi >> 6); t += nwaves) build_tile_meta(P, n, t, lane, tbox, tmsq);
        ++moves;
        reversed += (uint64_t)(js - is);
        TL_SYNC();
    }

    // ---------------------------------------------------------------- results
    uint32_t *__restrict__ out = A.out_pos + (size_t)d * n;
    for (uint32_t k = tid; k < n; k += nt) out[k] = perm[k];
    // tour_length (distance_matrix.rs:235-245): sequential f32 sum, closing edge first.  Edge lengths in parallel into the row
    // cache's place (every wave has left its scan behind the barrier above), the sum by one lane in tour order.
    float *E = reinterpret_cast<float *>(rowkey);
    for (uint32_t k = tid; k + 1u < n; k += nt) E[k] = dist(P[k], P[k + 1u]);
    TL_SYNC();
    if (tid == 0) {
        float total = dist(P[n - 1u], P[0]);
        const float4 *e4 = reinterpret_cast<const float4 *>(E);
        uint32_t k = 0;
        for (; k + 4u <= n - 1u; k += 4u) {
            const float4 v = e4[k >> 2];
            total += v.x;
            total += v.y;
            total += v.z;
            total += v.w;
        }
        for (; k < n - 1u; ++k) total += E[k];
        A.out_cost[d] = total;
        uint64_t *st = A.out_stats + (size_t)d * TL_STATS_STRIDE;
        for (int q = 4; q < TL_STATS_STRIDE; ++q) st[q] = 0;
        st[0] = sweeps;
        st[1] = moves;
        st[2] = reversed;
        st[3] = status;
    }
}

size_t two_opt_best_lds_bytes(uint32_t n) { return BsLdsLayout(n).bytes; }

// the largest n whose state fits: bytes(n) = 18 n_pad + 20 ntile_cap + 144 grows with n_pad = 64 ceil((n + 64) / 64), so the
// answer is the last n of the largest n_pad that fits, and at most 65 535 (the packed (i, j) key)
uint32_t two_opt_best_lds_max_n(int lds_budget)
{
    uint32_t best = 0;
    for (uint32_t n_pad = 128u; n_pad <= 65600u; n_pad += 64u) {
        const uint32_t n = n_pad - 64u;  // the largest n with this n_pad
        if (two_opt_best_lds_bytes(n) > (size_t)(lds_budget > 0 ? lds_budget : 0)) break;
        best = n < 65535u ? n : 65535u;
    }
    return best >= 3u ? best : 0u;
}

// Threads per descent (pop_threads, tl_kernels.h): a sweep is n - 3 wave-sized units of work
int two_opt_best_lds_threads(uint32_t n, uint32_t count, int cus, int lds_budget)
{
    return pop_threads(n > 3u ? n - 3u : 1u, two_opt_best_lds_bytes(n), count, cus, lds_budget);
}

hipError_t launch_two_opt_best_lds(const BestLdsArgs &A, uint32_t count, int threads, hipStream_t s)
{
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_bs_lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bs_lds, dim3(count), dim3(threads), two_opt_best_lds_bytes(A.n), s, A);
    return hipGetLastError();
}

}  // namespace tl
