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
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr uint32_t kPopJC = 8;     // j values per unit
constexpr int kPopMaxWaves = 16;
constexpr size_t kPopSlotBytes = 256;  // 3 x 16 words of reduction slots, padded

__device__ __forceinline__ bool better(float sa, uint32_t ija, uint32_t kca, float sb, uint32_t ijb, uint32_t kcb)
{
    return sa > sb || (sa == sb && (ija < ijb || (ija == ijb && kca < kcb)));
}

__host__ __device__ __forceinline__ uint32_t pop_chunks(uint32_t n, uint32_t i) { return ((n - 2u - i) + kPopJC - 1u) / kPopJC; }

}  // namespace

template <bool DM>
__global__ __launch_bounds__(kPopMaxWaves * 64) void k_three_opt_pop(ThreeOptPopArgs A)
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
            const float *Ra = Dt + i * rs, *Rb = Ra + rs;  // rows of a = path[i], b = path[i+1]
            const float d_ab = E[i];
            // k_three_opt_scan's lane loop (three_opt.hip), copied: Dt is written by this kernel, so it cannot take that kernel's
            // __restrict__ read-only rows, and E lives in LDS.  The two copies change together.
            for (uint32_t k = jlo + 1u + lane; k < n; k += 64u) {
                if (i == 0u && k == n - 1u) continue;  // :81-83
                const float d_ef = E[k], d_ae = Ra[k], d_be = Rb[k], d_bf = Rb[k + 1u];
                const float *Rc = Dt + jlo * rs;
                float d_ce = Rc[k], d_cf = Rc[k + 1u];
                // the row of D = path[j+1] and the j terms of the NEXT iteration are in flight during this one
                float n_de = Rc[rs + k], n_dtf = Rc[rs + k + 1u];
                float n_c_dt = E[jlo], n_ac = Ra[jlo], n_a_dt = Ra[jlo + 1u], n_b_dt = Rb[jlo + 1u];
                for (uint32_t j = jlo; j < jhi; ++j) {  // j >= k is masked below
                    const float d_de = n_de, d_dt_f = n_dtf;
                    const float d_c_dt = n_c_dt, d_ac = n_ac, d_a_dt = n_a_dt, d_b_dt = n_b_dt;
                    {   // rows up to jhi <= n-1 exist; the last iteration reloads the same (unused) values
                        const uint32_t jn = j + 1u < jhi ? j + 1u : j;
                        const float *Rn = Dt + (jn + 1u) * rs;
                        n_de = Rn[k];
                        n_dtf = Rn[k + 1u];
                        n_c_dt = E[jn];
                        n_ac = Ra[jn];
                        n_a_dt = Ra[jn + 1u];
                        n_b_dt = Rb[jn + 1u];
                    }
                    const float orig = (d_ab + d_c_dt) + d_ef;
                    const float c0 = (d_ac + d_b_dt) + d_ef;   // case 1
                    const float c1 = (d_ab + d_ce) + d_dt_f;   // case 2
                    const float c2 = (d_ac + d_be) + d_dt_f;   // case 3
                    const float c3 = (d_a_dt + d_be) + d_cf;   // case 4
                    const float c4 = (d_a_dt + d_ce) + d_bf;   // case 5
                    const float c5 = (d_ae + d_b_dt) + d_cf;   // case 6
                    const float c6 = (d_ae + d_c_dt) + d_bf;   // case 7
                    // :113-117 leaves cmin = min(orig, c0..c6) (NaN costs never pass `c < cmin`; fminf drops them the same way)
                    const float cm = fminf(fminf(fminf(orig, c0), fminf(c1, c2)), fminf(fminf(c3, c4), fminf(c5, c6)));
                    const float sav = orig - cm;  // :120
                    if (__builtin_amdgcn_ballot_w64((sav >= bs) & (sav > 0.0f) & (j < k))) {
                        float cmin = orig;
                        int ci = -1;
                        if (c0 < cmin) { cmin = c0; ci = 0; }
                        if (c1 < cmin) { cmin = c1; ci = 1; }
                        if (c2 < cmin) { cmin = c2; ci = 2; }
                        if (c3 < cmin) { cmin = c3; ci = 3; }
                        if (c4 < cmin) { cmin = c4; ci = 4; }
                        if (c5 < cmin) { cmin = c5; ci = 5; }
                        if (c6 < cmin) { cmin = c6; ci = 6; }
                        // :119-125 strict `>` in (i, j, k) loop order; a lane meets its triples in another order, so order by key
                        if (ci >= 0 && j < k && better(orig - cmin, (i << 16) | j, (k << 3) | (uint32_t)(ci + 1), bs, bij, bkc)) {
                            bs = orig - cmin;
                            bij = (i << 16) | j;
                            bkc = (k << 3) | (uint32_t)(ci + 1);
                        }
                    }
                    d_ce = d_de;
                    d_cf = d_dt_f;
                }
            }
            c += nwaves;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_down(bs, off);
            const uint32_t oij = __shfl_down(bij, off), okc = __shfl_down(bkc, off);
            if (better(os, oij, okc, bs, bij, bkc)) { bs = os; bij = oij; bkc = okc; }
        }
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
        for (uint32_t t = tid; t < L; t += nt) {
            uint32_t src;  // index into tmp (0..l1-1 = seg1, l1.. = seg2)
            switch (kase) {
            case 1: src = t < l1 ? (l1 - 1u - t) : t; break;                                  // rev(s1) + s2
            case 2: src = t < l1 ? t : (l1 + (L - 1u - t)); break;                            // s1 + rev(s2)
            case 3: src = t < l1 ? (l1 - 1u - t) : (l1 + (L - 1u - t)); break;                // rev(s1) + rev(s2)
            case 4: src = t < l2 ? (l1 + t) : (t - l2); break;                                // s2 + s1
            case 5: src = t < l2 ? (l1 + t) : (l1 - 1u - (t - l2)); break;                    // s2 + rev(s1)
            case 6: src = t < l2 ? (l1 + (l2 - 1u - t)) : (t - l2); break;                    // rev(s2) + s1
            default: src = t < l2 ? (l1 + (l2 - 1u - t)) : (l1 - 1u - (t - l2)); break;       // 7: rev(s2) + rev(s1)
            }
            perm[mi + 1u + t] = tmp[src];
        }
        TL_SYNC();
    }

    uint32_t *out = A.out_pos + (size_t)tour * n;
    for (uint32_t k = tid; k < n; k += nt) out[k] = perm[k];
    if (tid == 0) {
        // tour_length (distance_matrix.rs:235-245): the closing edge first, then the n - 1 edges in order, sequential f32
        float total = E[n - 1u];
        for (uint32_t k = 0; k + 1u < n; ++k) total += E[k];
        A.out_cost[tour] = total;
        A.out_run[4u * tour + 0u] = moves;
        A.out_run[4u * tour + 1u] = passes;
        A.out_run[4u * tour + 2u] = status;
        A.out_run[4u * tour + 3u] = 0u;
    }
}

size_t three_opt_pop_lds_bytes(uint32_t n) { return (size_t)n * 20 + 8 + kPopSlotBytes; }

uint32_t three_opt_pop_max_n(int lds_budget)
{
    if ((size_t)lds_budget <= 8 + kPopSlotBytes) return 0u;
    const size_t m = ((size_t)lds_budget - 8 - kPopSlotBytes) / 20;
    return m > 65535u ? 65535u : (uint32_t)m;  // packed 16-bit (i, j), (k, case), as tl_three_opt
}

// Threads per tour.  A pass has sum_i ceil((n-2-i) / kPopJC) wave-sized units, so a tour cannot use more waves than that; beyond
// it the widest workgroup of which the CU still holds its share of the batch (count / cus tours, 32 waves, the LDS) at once.
int three_opt_pop_threads(uint32_t n, uint32_t count, int cus, int lds_budget)
{
    uint64_t units = 0;
    for (uint32_t i = 0; i + 2u < n && units < (uint64_t)kPopMaxWaves; ++i) units += pop_chunks(n, i);
    const uint32_t per_cu = cus > 0 ? (count + (uint32_t)cus - 1u) / (uint32_t)cus : 1u;
    const size_t fit = (size_t)(lds_budget > 0 ? lds_budget : 0) / three_opt_pop_lds_bytes(n);
    uint32_t share = per_cu < fit ? per_cu : (uint32_t)fit;
    if (share < 1u) share = 1u;
    int nt = kPopMaxWaves * 64;
    while (nt > 64 && ((uint64_t)nt / 64u > units || (uint32_t)nt * share > 2048u)) nt >>= 1;
    return nt;
}

hipError_t launch_three_opt_pop(const ThreeOptPopArgs &A, uint32_t count, int threads, hipStream_t s)
{
    const bool dm = A.dm != nullptr;
    const void *kern = dm ? reinterpret_cast<const void *>(k_three_opt_pop<true>) : reinterpret_cast<const void *>(k_three_opt_pop<false>);
    hipError_t e = allow_max_lds(kern);
    if (e != hipSuccess) return e;
    const size_t lds = three_opt_pop_lds_bytes(A.n);
    if (dm) hipLaunchKernelGGL(k_three_opt_pop<true>, dim3(count), dim3(threads), lds, s, A);
    else hipLaunchKernelGGL(k_three_opt_pop<false>, dim3(count), dim3(threads), lds, s, A);
    return hipGetLastError();
}

}  // namespace tl
