// or_opt.hip — Or-opt: best-improvement relocation of 1-, 2- or 3-city segments (reference: src/tsp/or_opt.rs;
// SURVEY.md §8(f) "next" row 3).
//
//   find_best_move (or_opt.rs:80-164): for seg_len in 1..=3, i in 0..n (segments that wrap are skipped), j in 0..n
//   outside {prev, i..i+seg_len-1}:  fwd_delta = -remove_gain + d(x,first) + d(last,y) - d(x,y) and, for seg_len > 1,
//   rev_delta with first/last swapped; the move with the lowest delta below -1e-3 wins, first in loop order
//   (seg_len, i, j, forward-before-reversed) on ties (strict `<`, :141,153).  apply_relocation (:170-184).
//
// Best-improvement, so one pass is a whole-chip scan: a wave takes 8 consecutive segment starts x a slab of insertion
// points (lanes along j) and shares the distances between the five placement kinds and the 8 starts (k_or_scan), every
// f32 expression associated exactly as the reference writes it; argmin by a packed 96-bit key
// (~delta_bits << 64 | loop-order index; the index 6 n^2 needs more than 32 bits from n = 26 755 on — round 4) reduced per wave,
// per workgroup, then by k_or_pick, which also applies the relocation in place.  Exact distances (correctly rounded sqrt); roofline: VALU.
#include "or_opt_scan.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kOrWaves = 4;
constexpr uint32_t kOrTargetWaves = 4096;  // waves a scan should at least consist of: small tours take fewer 63-wide chunks of
                                           // insertion points per wave (or_opt_chunks)

static uint32_t or_opt_grid_x(uint32_t n) { return ((n + kOrIR - 1) / kOrIR + kOrWaves - 1) / kOrWaves; }
static uint32_t or_opt_chunks(uint32_t n)  // 63-wide chunks of insertion points per wave
{
    const uint32_t total = (n + 62u) / 63u, groups = (n + kOrIR - 1) / kOrIR;
    uint32_t slabs = (kOrTargetWaves + groups - 1u) / groups;
    if (slabs > total) slabs = total;
    if (slabs == 0u) slabs = 1u;
    return (total + slabs - 1u) / slabs;
}
static uint32_t or_opt_grid_y(uint32_t n) { return ((n + 62u) / 63u + or_opt_chunks(n) - 1u) / or_opt_chunks(n); }

}  // namespace

// One wave = kOrIR consecutive segment starts i0..i0+kOrIR-1 x a slab of insertion points (`chunks` chunks of 63): or_scan_rows, or_opt_scan.h
template <bool DM>
__global__ __launch_bounds__(kOrWaves * 64) void k_or_scan(OrOptArgs A, uint32_t chunks)
{
    __shared__ unsigned long long s_key[kOrWaves * 2];
    if (A.run && A.run->done) return;  // a later pass of a batch whose descent is over
    const uint32_t n = A.n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t i0 = (blockIdx.x * kOrWaves + (uint32_t)wave) * kOrIR;
    const uint32_t jlo = blockIdx.y * (chunks * 63u);
    key_t best = no_key();
    float bestd = __builtin_inff();
    if (i0 < n) {
        const Dist<DM> D{A.Pt, A.dm, A.perm};
        or_scan_rows(D, A.E, n, i0, jlo, chunks, lane, best, bestd);
    }
    const key_t k = block_min_key(best, s_key, lane, (uint32_t)wave, kOrWaves);
    if (threadIdx.x == 0) {
        unsigned long long *out = A.partials + 2u * (size_t)(blockIdx.y * gridDim.x + blockIdx.x);
        out[0] = (unsigned long long)(k >> 64);
        out[1] = (unsigned long long)k;
    }
}

template <bool DM>
__global__ __launch_bounds__(256) void k_or_prepare(OrOptArgs A)
{
    if (A.run && A.run->done) return;
    const uint32_t n = A.n;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        const uint32_t p = A.perm[k], q = A.perm[k + 1u == n ? 0u : k + 1u];
        if (!DM) A.Pt[k] = A.xy[p];
        A.E[k] = DM ? dm_lookup(A.dm, p, q) : dist(A.xy[p], A.xy[q]);
    }
}

// reduce, publish the move and (optionally) apply_relocation (or_opt.rs:170-184)
__global__ __launch_bounds__(1024) void k_or_pick(OrOptArgs A, uint32_t nblocks, int apply, int stage_lds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the pre-move tour: in LDS where n entries fit, else in the workspace (one workgroup: its own barrier orders the copy)
    uint32_t *old = stage_lds ? reinterpret_cast<uint32_t *>(smem) : A.scratch;
    __shared__ unsigned long long s_key[16 * 2];
    const uint32_t tid = threadIdx.x, n = A.n;
    const int lane = tid & 63, wave = tid >> 6;
    if (A.run && A.run->done) return;
    key_t best = no_key();
    for (uint32_t b = tid; b < nblocks; b += 1024u) {
        const key_t k = make_key(A.partials[2u * (size_t)b], A.partials[2u * (size_t)b + 1u]);
        best = k < best ? k : best;
    }
    best = block_min_key(best, s_key, lane, (uint32_t)wave, 16u);
    const bool found = best != no_key();
    const OrMove mv = or_decode(best, n);
    const uint32_t i = mv.i, j = mv.j, seg_len = mv.seg_len, reversed = mv.reversed;
    if (tid == 0) {
        A.best->found = found ? 1u : 0u;
        A.best->delta_bits = ~(uint32_t)(unsigned long long)(best >> 64);
        A.best->i = i;
        A.best->j = j;
        A.best->seg_len = seg_len;
        A.best->reversed = reversed;
        scan_file_pass(A.run, A.log, found, i, j, seg_len, reversed);  // or_opt.rs:45
    }
    if (!found || !apply) return;
    uint32_t *path = A.perm;
    for (uint32_t t = tid; t < n; t += 1024u) old[t] = path[t];
    TL_SYNC();
    const uint32_t insert_at = (j >= i + seg_len) ? (j - seg_len + 1u) : (j + 1u);  // index in the drained tour
    for (uint32_t t = tid; t < n; t += 1024u) {
        uint32_t src;
        if (t >= insert_at && t < insert_at + seg_len) {
            const uint32_t s = t - insert_at;
            src = i + (reversed ? (seg_len - 1u - s) : s);
        } else {
            const uint32_t u = t < insert_at ? t : t - seg_len;  // index in the drained tour
            src = u < i ? u : u + seg_len;
        }
        path[t] = old[src];
    }
}

hipError_t launch_or_opt_pass(const OrOptArgs &A, bool dm, int apply, hipStream_t s, int lds_budget)
{
    const uint32_t gx = or_opt_grid_x(A.n), gy = or_opt_grid_y(A.n), nblocks = gx * gy;
    const uint32_t pg = (A.n + 255u) / 256u;
    if (dm) {
        hipLaunchKernelGGL(k_or_prepare<true>, dim3(pg), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_or_scan<true>, dim3(gx, gy), dim3(kOrWaves * 64), 0, s, A, or_opt_chunks(A.n));
    } else {
        hipLaunchKernelGGL(k_or_prepare<false>, dim3(pg), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_or_scan<false>, dim3(gx, gy), dim3(kOrWaves * 64), 0, s, A, or_opt_chunks(A.n));
    }
    hipError_t e = allow_max_lds(reinterpret_cast<const void *>(k_or_pick));
    if (e != hipSuccess) return e;
    // LDS up to 256 cities, the workspace beyond: both forms run in the parity tests at sizes the oracle affords
    const bool stage_lds = A.n <= 256u && (size_t)A.n * 4 + 1024 <= (size_t)lds_budget;
    hipLaunchKernelGGL(k_or_pick, dim3(1), dim3(1024), stage_lds ? (size_t)A.n * 4 : 0, s, A, nblocks, apply, stage_lds ? 1 : 0);
    return hipGetLastError();
}

uint32_t or_opt_scan_blocks(uint32_t n) { return or_opt_grid_x(n) * or_opt_grid_y(n); }

}  // namespace tl
