// three_opt_pop.hip — 3-opt for a population of tours: one persistent workgroup per tour runs the whole descent of three_opt::solve
// (three_opt.rs:16-51: while find_best_move finds a move, apply_3opt) — no launch and no global reduction per move, which is
// nearly all a small tour's chip-wide pass (three_opt.hip: four launches) consists of.
//
//   LDS, per tour: Pt[n+1] tour-ordered coordinates (Pt[n] = Pt[0]; unused in the matrix form, kept so that one size rule serves
//   both forms) | perm[n] | E[n] tour-edge lengths | tmp[n] the two segments of apply_3opt | 16 reduction slots (sav, ij, kc).
//   Workspace, per tour: Dt, the n x (n+1) f32 matrix of distances between tour POSITIONS exactly as k_three_opt_build_dt fills it
//   (column n == column 0).  The workgroup builds it before its first pass and rebuilds all of it after every applied move —
//   O(n^2) beside the pass's O(n^3).  It is written with plain stores and read with plain loads by the same workgroup across a
//   barrier: no __restrict__ on it in here, nothing non-temporal, nothing kept in registers across a move.
//
//   THE DIVISION OF A PASS (the tests plant on these seams):
//     unit      = (i, chunk of kPopJC = 8 consecutive j): j in [i+1+8c, min(i+1+8c+8, n-1)); row i has ceil((n-2-i)/8) chunks, so the
//                 first row gets a second chunk at n = 11 (n-2 = 9 values of j).
//     waves     : the units, numbered in (i, chunk) order, are dealt round-robin: wave w takes units w, w + nwaves, ...
//                 (nwaves = threads / 64, 1 ... 16: a second round of units begins at unit number nwaves).
//     lanes     : along k in strides of 64 from jlo+1: lane l takes k = jlo+1+l, jlo+1+l+64, ... < n, and walks the chunk's j in
//                 registers exactly as k_three_opt_scan's lane does (the row of C = path[j] rolls into the next j's).  A second
//                 stride begins where n - (jlo+1) > 64: n = 67 for the first unit.
//     apply / refresh: strided by the workgroup's thread count (64 ... 1 024) over the move's i+1..k and over 0..n; Dt rows are dealt
//                 to the waves, columns to the lanes.
//   The per-triple arithmetic is k_three_opt_scan's: the 7 reconnection sums associated (x + y) + z, the first minimum among the
//   costs < orig per triple, and between triples the total order better() over (savings, (i,j), (k,case)) == the reference's
//   strict `>` in loop order — so the move found does not depend on how the work is dealt or on the workgroup size.
#include "three_opt_scan.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr uint32_t kPopJC = 8;     // j values per unit
constexpr int kPopMaxWaves = 16;
constexpr size_t kPopSlotBytes = 256;  // 3 x 16 words of reduction slots, padded

__host__ __device__ __forceinline__ uint32_t pop_chunks(uint32_t n, uint32_t i) { return ((n - 2u - i) + kPopJC - 1u) / kPopJC; }

}  // namespace

template <bool DM>
__global__ __launch_bounds__(kPopMaxWaves * 64) void k_three_opt_pop(PopArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n = A.n, tid = threadIdx.x, nt = blockDim.x, tour = blockIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), nwaves = nt >> 6;
    float2 *Pt = reinterpret_cast<float2 *>(smem);
    uint32_t *perm = reinterpret_cast<uint32_t *>(smem + (size_t)(n + 1u) * 8);
    float *E = reinterpret_cast<float *>(perm + n);
    uint32_t *tmp = reinterpret_cast<uint32_t *>(E + n);
    float *r_s = reinterpret_cast<float *>(tmp + n);
    uint32_t *r_ij = reinterpret_cast<uint32_t *>(r_s + kPopMaxWaves), *r_kc = r_ij + kPopMaxWaves;
    const size_t rs = (size_t)n + 1u;  // row stride of Dt
    float *Dt = A.Dt + (size_t)tour * n * rs;

    const uint32_t *init = A.init + (size_t)tour * n;
    for (uint32_t k = tid; k < n; k += nt) perm[k] = init[k];
    TL_SYNC();

    uint32_t passes = 0, moves = 0, status = 0;
    for (;;) {
        // Pt, E and Dt of the tour as it stands (k_three_opt_prepare, k_three_opt_build_dt)
        if (!DM) {
            for (uint32_t k = tid; k <= n; k += nt) Pt[k] = A.xy[perm[k == n ? 0u : k]];
            TL_SYNC();
        }
        for (uint32_t k = tid; k < n; k += nt) {
            const uint32_t q = k + 1u == n ? 0u : k + 1u;
            E[k] = DM ? dm_lookup(A.dm, perm[k], perm[q]) : dist(Pt[k], Pt[q]);
        }
        for (uint32_t p = wave; p < n; p += nwaves) {
            float *row = Dt + p * rs;
            for (uint32_t q = lane; q <= n; q += 64u) {
                const uint32_t qq = q == n ? 0u : q;
                row[q] = DM ? dm_lookup(A.dm, perm[p], perm[qq]) : dist(Pt[p], Pt[qq]);
            }
        }
        TL_SYNC();

        // find_best_move (three_opt.rs:58-131)
        float bs = 0.0f;  // :61 best_savings = 0.0
        uint32_t bij = 0xFFFFFFFFu, bkc = 0xFFFFFFFFu;
        uint32_t i = 0, c = wave;  // this wave's unit: chunk c of row i
        for (;;) {
            while (i + 2u < n && c >= pop_chunks(n, i)) {
                c -= pop_chunks(n, i);
                ++i;
            }
            if (i + 2u >= n) break;  // i in [0, n-2)
            const uint32_t jlo = i + 1u + c * kPopJC;
            uint32_t jhi = jlo + kPopJC;
            if (jhi > n - 1u) jhi = n - 1u;  // j in [i+1, n-1)
            // k_three_opt_scan's lane loop (three_opt_scan.h), which claims nothing about Dt and E: this kernel writes both
            three_opt_scan_lane(Dt, rs, E, n, i, jlo, jhi, jlo + 1u + lane, 64u, bs, bij, bkc);
            c += nwaves;
        }
        wave_best(bs, bij, bkc);
        if (lane == 0u) { r_s[wave] = bs; r_ij[wave] = bij; r_kc[wave] = bkc; }
        TL_SYNC();
        // every thread reads the slots behind the barrier, so the whole workgroup takes the same way out of the loop (the slots
        // are written again only behind the barriers of the apply step and the refresh)
        bs = r_s[0]; bij = r_ij[0]; bkc = r_kc[0];
        for (uint32_t w = 1; w < nwaves; ++w)
            if (better(r_s[w], r_ij[w], r_kc[w], bs, bij, bkc)) { bs = r_s[w]; bij = r_ij[w]; bkc = r_kc[w]; }
        ++passes;  // three_opt.rs:36-45: the last pass finds nothing
        if (bkc == 0xFFFFFFFFu) break;  // savings > 0 was required to record a move
        if (passes >= A.max_passes) {
            status = 1u;
            break;
        }
        ++moves;
        // apply_3opt (three_opt.rs:186-218), as k_three_opt_pick: seg1 = path[i+1..=j], seg2 = path[j+1..=k]
        const uint32_t mi = bij >> 16, mj = bij & 0xFFFFu, mk = bkc >> 3, kase = bkc & 7u;
        const uint32_t l1 = mj - mi, l2 = mk - mj, L = l1 + l2;
        for (uint32_t t = tid; t < L; t += nt) tmp[t] = perm[mi + 1u + t];
        TL_SYNC();
        for (uint32_t t = tid; t < L; t += nt) perm[mi + 1u + t] = tmp[three_opt_src(kase, t, l1, l2)];
        TL_SYNC();
    }

    pop_finish(A, perm, E, moves, passes, status);
}

size_t three_opt_pop_lds_bytes(uint32_t n) { return (size_t)n * 20 + 8 + kPopSlotBytes; }

uint32_t three_opt_pop_max_n(int lds_budget)
{
    if ((size_t)lds_budget <= 8 + kPopSlotBytes) return 0u;
    const size_t m = ((size_t)lds_budget - 8 - kPopSlotBytes) / 20;
    return m > 65535u ? 65535u : (uint32_t)m;  // packed 16-bit (i, j), (k, case), as tl_three_opt
}

// Threads per tour (pop_threads, tl_kernels.h): a pass has sum_i ceil((n-2-i) / kPopJC) wave-sized units
int three_opt_pop_threads(uint32_t n, uint32_t count, int cus, int lds_budget)
{
    uint64_t units = 0;
    for (uint32_t i = 0; i + 2u < n && units < (uint64_t)kPopMaxWaves; ++i) units += pop_chunks(n, i);
    return pop_threads(units, three_opt_pop_lds_bytes(n), count, cus, lds_budget);
}

hipError_t launch_three_opt_pop(const PopArgs &A, uint32_t count, int threads, hipStream_t s)
{
    return launch_pop(k_three_opt_pop<true>, k_three_opt_pop<false>, A, count, threads, three_opt_pop_lds_bytes(A.n), s);
}

}  // namespace tl
