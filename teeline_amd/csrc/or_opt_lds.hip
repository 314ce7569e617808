// or_opt_lds.hip — Or-opt for a population of tours: one persistent workgroup per tour runs the whole descent of or_opt::solve
// (or_opt.rs:44-68: while find_best_move finds a move, apply_relocation) with the tour in its CU's LDS — no launch and no global
// reduction per move, which is all a small tour's chip-wide pass (or_opt.hip) consists of.
//
//   LDS: Pt[n] tour-ordered coordinates (coordinate form only) | perm[n] | E[n] tour-edge lengths | one key slot per wave.
//   Scan: the waves deal the groups of kOrIR segment starts between themselves and run or_scan_rows (or_opt_scan.h), the wave
//   body of k_or_scan, over every insertion point; the packed key (~delta bits, loop-order index) makes the minimum the same
//   move however the work is dealt, so the result does not depend on the workgroup size.
//   Apply: only the positions between the segment and the insertion point move (by seg_len, towards the segment's old place);
//   they are copied in workgroup-sized runs, each read before a barrier and written behind it, starting at the segment's end
//   so that no run overwrites what a later one reads.  E moves with them; the edges that changed are computed anew with dist.
#include "or_opt_scan.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kOrLdsMaxWaves = 16;
constexpr size_t kOrLdsSlotBytes = (size_t)kOrLdsMaxWaves * 16;  // the waves' key slots

}  // namespace

template <bool DM>
__global__ __launch_bounds__(kOrLdsMaxWaves * 64) void k_or_lds(PopArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, tour = blockIdx.x;
    const int lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), nwaves = nt >> 6;
    float2 *Pt = reinterpret_cast<float2 *>(smem);
    uint32_t *perm = reinterpret_cast<uint32_t *>(smem + (DM ? 0 : (size_t)n * 8));
    float *E = reinterpret_cast<float *>(perm + n);
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(smem + (DM ? 0 : (size_t)n * 8) + (size_t)n * 8);
    const Dist<DM> D{Pt, A.dm, perm};  // Pt and perm in LDS, the packed matrix in HBM

    const uint32_t *init = A.init + (size_t)tour * n;
    for (uint32_t k = tid; k < n; k += nt) {
        const uint32_t p = init[k];
        perm[k] = p;
        if (!DM) Pt[k] = A.xy[p];
    }
    TL_SYNC();
    for (uint32_t k = tid; k < n; k += nt) E[k] = D(k, k + 1u == n ? 0u : k + 1u);
    TL_SYNC();

    const uint32_t groups = (n + kOrIR - 1) / kOrIR, chunks = (n + 62u) / 63u;
    uint32_t passes = 0, moves = 0, status = 0;
    for (;;) {
        key_t best = no_key();
        float bestd = __builtin_inff();
        for (uint32_t g = wave; g < groups; g += nwaves) or_scan_rows(D, E, n, g * kOrIR, 0u, chunks, lane, best, bestd);
        best = block_min_key(best, s_key, lane, wave, nwaves);
        ++passes;  // or_opt.rs:45 `while let Some(best) = find_best_move(..)`: the last pass finds nothing
        if (best == no_key()) break;
        if (passes >= A.max_passes) {
            status = 1u;
            break;
        }
        ++moves;
        // apply_relocation (or_opt.rs:172-184): drain [i, i + L), insert it after the old index j.  (Every wave has left its scan
        // and read the slots' minimum; the slots are written again only behind the barriers below.)
        const OrMove mv = or_decode(best, n);
        const uint32_t i = mv.i, j = mv.j, L = mv.seg_len;
        const bool right = j >= i + L;                            // the segment travels towards higher positions
        const uint32_t insert_at = right ? j - L + 1u : j + 1u;  // its new first position
        // the segment: what this thread will write of it (thread t < L writes its new position insert_at + t)
        const uint32_t sk = i + (tid < L ? (mv.reversed ? L - 1u - tid : tid) : 0u);
        const uint32_t seg_p = perm[sk];
        float2 seg_c = {0.0f, 0.0f};
        if (!DM) seg_c = Pt[sk];
        // positions [lo, hi) take the element L places further on (right) or back: run after run from the segment's end
        const uint32_t lo = right ? i : insert_at + L, hi = right ? insert_at : i + L, cnt = hi - lo;
        for (uint32_t base = 0; base < cnt; base += nt) {
            const uint32_t q = base + tid;
            const bool act = q < cnt;
            const uint32_t t = right ? lo + q : hi - 1u - q, src = right ? t + L : t - L;
            uint32_t p = 0;
            float2 c = {0.0f, 0.0f};
            float e = 0.0f;
            if (act) {
                p = perm[src];
                if (!DM) c = Pt[src];
                e = E[src];
            }
            TL_SYNC();
            if (act) {
                perm[t] = p;
                if (!DM) Pt[t] = c;
                E[t] = e;  // the edge to the next position moved along (the run's last edge is one of those computed anew below)
            }
        }
        if (tid < L) {
            perm[insert_at + tid] = seg_p;
            if (!DM) Pt[insert_at + tid] = seg_c;
        }
        TL_SYNC();
        // the edges that changed: into, inside and out of the segment (insert_at - 1 .. insert_at + L - 1) and the one that closes
        // the gap it left (the position before i, or the last shifted one)
        if (tid < L + 2u) {
            const uint32_t k = tid <= L ? insert_at - 1u + tid : right ? (i == 0u ? n - 1u : i - 1u) : i + L - 1u;
            E[k] = D(k, k + 1u == n ? 0u : k + 1u);
        }
        TL_SYNC();
    }

    pop_finish(A, perm, E, moves, passes, status);
}

size_t or_opt_lds_bytes(uint32_t n, bool dm) { return (size_t)n * (dm ? 8 : 16) + kOrLdsSlotBytes; }

uint32_t or_opt_lds_max_n(int lds_budget, bool dm)
{
    if ((size_t)lds_budget <= kOrLdsSlotBytes) return 0u;
    const size_t m = ((size_t)lds_budget - kOrLdsSlotBytes) / (dm ? 8 : 16);
    return m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m;
}

// Threads per tour (pop_threads, tl_kernels.h): a pass is (n / kOrIR) wave-sized units of work
int or_opt_lds_threads(uint32_t n, uint32_t count, int cus, int lds_budget, bool dm)
{
    return pop_threads((n + kOrIR - 1) / kOrIR, or_opt_lds_bytes(n, dm), count, cus, lds_budget);
}

hipError_t launch_or_opt_lds(const PopArgs &A, uint32_t count, int threads, hipStream_t s)
{
    return launch_pop(k_or_lds<true>, k_or_lds<false>, A, count, threads, or_opt_lds_bytes(A.n, A.dm != nullptr), s);
}

}  // namespace tl
