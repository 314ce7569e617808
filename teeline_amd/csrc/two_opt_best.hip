// two_opt_best.hip — TL_MODE_BEST_SWEEP: best-improvement 2-opt (this build's own throughput mode; NOT the
// reference's algorithm — the reference is first-improvement, src/tsp/two_opt.rs:26-61).  Specification =
// oracle/tlo_two_opt_best: per sweep every (i,j) of the same open-path candidate set is decided, the move with the
// lowest f32 delta (new - cur) < 0 wins, lowest (i,j) on ties; apply; repeat until a sweep finds none.
//
// Unlike REF_ORDER a sweep has no sequential dependency, so the whole chip works on it:
//   k_bs_init    tour-ordered coordinates P[k] = xy[perm[k]] and per-tile L0 metadata, in HBM (L2-resident)
//   k_bs_scan    one wave per row i (two_opt_best_scan.h).  L0 (lanes = tiles) -> live-tile mask, L1 (lanes = j) on live tiles, L2 hardware
//                sqrt to discard the clearly non-improving, exact delta for the rest.  Argmin by wavefront DPP/shuffle
//                reduction of a packed 64-bit key (~delta bits << 32 | i << 16 | j), then per workgroup.  Every row's best key is
//                cached; a sweep decides only the rows (and, for the rows in front of the move, the columns) the previous move touched.
//   k_bs_apply   one workgroup: reduces the per-workgroup keys, applies swap_2opt(path, i+1, j) on P and perm,
//                rebuilds the L0 metadata of the touched tiles, bumps the counters / sets the done flag, files the move for the scan.
// The host replays 64 sweeps (scan + apply) as one hipGraph per poll of the done flag.
#include "tl_kernels.h"
#include "two_opt_best_scan.h"

#pragma clang fp contract(off)

namespace tl {

__global__ __launch_bounds__(256) void k_bs_init(BestSweepArgs A)
{
    const uint32_t n = A.n, npad = A.n_pad, ntile = npad >> 6;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (A.phase == 0) {
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k <= npad; k += gridDim.x * 256u)
            A.P[k] = k < n ? A.xy[A.perm[k]] : make_float2(0.f, 0.f);
        return;
    }
    for (uint32_t t = blockIdx.x * 4u + wave; t < A.ntile_cap; t += gridDim.x * 4u) {
        if (t < ntile) build_tile_meta(A.P, n, t, (int)lane, A.tbox, A.tmsq);
        else if (lane == 0) {
            const float inf = __builtin_inff();
            A.tbox[t] = make_float4(inf, inf, -inf, -inf);
            A.tmsq[t] = -1.0f;
        }
    }
}

// One wave per row, decided through the row cache A.rowkey (bs_row_decide, two_opt_best_scan.h: the body the population's
// LDS-resident form shares).
// (Scan and apply as ONE launch — 256 workgroups of 16 waves, rows strided over all waves, the workgroup that draws the sweep's last
//  ticket applies the move — was built and measured: 19.0 us per sweep against 10.2 for the two launches at n = 10^4, NOTEBOOK r5.4.)
constexpr int kBsWaves = 4;  // rows per scan workgroup
__global__ __launch_bounds__(kBsWaves * 64) void k_bs_scan(BestSweepArgs A)
{
    __shared__ unsigned long long s_key[kBsWaves];
    const uint32_t n = A.n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t i = blockIdx.x * kBsWaves + (uint32_t)wave;  // row
    unsigned long long best = kNoKey64;
    if (A.counters[2] == 0 && i + 3u < n) {  // not done; rows i in [0, n-3)
        const uint32_t mv = A.move[0], is = A.move[1], js = A.move[2];
        best = bs_row_decide(A.P, A.tbox, A.tmsq, A.rowkey, n, i, mv, is, js, lane);
    }
    if (lane == 0) s_key[wave] = best;
    TL_SYNC();
    if (threadIdx.x == 0) {
        unsigned long long k = s_key[0];
        for (int w = 1; w < kBsWaves; ++w) k = s_key[w] < k ? s_key[w] : k;
        A.partials[blockIdx.x] = k;
    }
}

__global__ __launch_bounds__(1024) void k_bs_apply(BestSweepArgs A, uint32_t nblocks)
{
    __shared__ unsigned long long s_key[16];
    const uint32_t tid = threadIdx.x, n = A.n;
    const int lane = tid & 63, wave = tid >> 6;
    if (A.counters[2] != 0) return;  // done in an earlier sweep of this batch
    unsigned long long best = kNoKey64;
    for (uint32_t b = tid; b < nblocks; b += 1024u) {
        const unsigned long long k = A.partials[b];
        best = k < best ? k : best;
    }
    best = wave_min_u64(best);
    if (lane == 0) s_key[wave] = best;
    TL_SYNC();
    best = s_key[0];
    for (int w = 1; w < 16; ++w) best = s_key[w] < best ? s_key[w] : best;
    if (best == kNoKey64) {
        if (tid == 0) {
            A.counters[0] += 1;  // the final, move-less sweep
            A.counters[2] = 1;   // done
        }
        return;
    }
    const uint32_t is = (uint32_t)((best >> 16) & 0xFFFFu), js = (uint32_t)(best & 0xFFFFu);
    const uint32_t lo = is + 1u, hi = js, half = (hi - lo + 1u) >> 1;
    float2 *P = A.P;
    uint32_t *perm = A.perm;
    for (uint32_t t = tid; t < half; t += 1024u) {  // swap_2opt(path, i+1, j)
        const float2 x = P[lo + t], y = P[hi - t];
        P[lo + t] = y;
        P[hi - t] = x;
        const uint32_t u = perm[lo + t], v = perm[hi - t];
        perm[lo + t] = v;
        perm[hi - t] = u;
    }
    TL_SYNC();
    for (uint32_t t = ((lo - 1u) >> 6) + (uint32_t)wave; t <= (hi >> 6); t += 16u) build_tile_meta(P, n, t, lane, A.tbox, A.tmsq);
    if (tid == 0) {
        A.counters[0] += 1;                       // sweeps
        A.counters[1] += 1;                       // moves
        A.counters[3] += (uint64_t)(js - is);     // reversed elements
        A.move[1] = is;                           // what the next sweep's scan needs to know
        A.move[2] = js;
        A.move[0] = 1u;
    }
}

hipError_t launch_best_sweep_init(const BestSweepArgs &A, hipStream_t s)
{
    BestSweepArgs B = A;
    B.phase = 0;
    hipLaunchKernelGGL(k_bs_init, dim3((A.n_pad + 256u) / 256u), dim3(256), 0, s, B);
    B.phase = 1;
    hipLaunchKernelGGL(k_bs_init, dim3((A.ntile_cap + 3u) / 4u), dim3(256), 0, s, B);
    return hipGetLastError();
}

hipError_t launch_best_sweep_round(const BestSweepArgs &A, hipStream_t s)
{
    const uint32_t nblocks = best_sweep_scan_blocks(A.n);
    hipLaunchKernelGGL(k_bs_scan, dim3(nblocks), dim3(kBsWaves * 64), 0, s, A);
    hipLaunchKernelGGL(k_bs_apply, dim3(1), dim3(1024), 0, s, A, nblocks);
    return hipGetLastError();
}

uint32_t best_sweep_scan_blocks(uint32_t n) { return (n - 3u + kBsWaves - 1) / kBsWaves; }

}  // namespace tl
