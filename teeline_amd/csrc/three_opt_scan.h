// three_opt_scan.h — what the two 3-opt kernels share (internal to libteeline_gpu): the order between moves, a lane's walk over the
// triples of one (i, chunk of j), the wave's reduction of a best triple and apply_3opt's index arithmetic.  three_opt.hip (chip-wide
// pass over a tour in HBM) and three_opt_pop.hip (one workgroup per tour, the whole descent) include it, so both find and apply the
// same move bit for bit.
#pragma once
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

// The total order between moves, (savings, (i << 16 | j), (k << 3 | case)): higher savings first, then the lower key == the
// reference's strict `>` in (i, j, k) loop order (three_opt.rs:119-125)
__device__ __forceinline__ bool better(float sa, uint32_t ija, uint32_t kca, float sb, uint32_t ijb, uint32_t kcb)
{
    return sa > sb || (sa == sb && (ija < ijb || (ija == ijb && kca < kcb)));
}

// One lane's triples of the unit (i, j in [jlo, jhi)): the columns k = k0, k0 + kstep, ... < n (k0 > jlo).  Dt: the n x (n+1) matrix
// of distances between tour POSITIONS, row stride rs = n + 1, column n == column 0 (F = path[(k+1) % n], three_opt.rs:85); E[k]:
// the tour edge (k, k+1).  i, jlo and jhi are wave-uniform, so the (i, j) terms are scalar loads where the rows are in HBM.
// The lane owns a column k and walks the chunk's j in registers: everything that depends on (i, k) only is loaded once, the row of
// C = path[j] rolls into the row of the next j (D = path[j+1] is the next j's C), so a triple costs two coalesced loads and the
// seven sums.  No LDS of its own, no barrier.  bs / bij / bkc: this lane's best move so far, carried from one call to the next.
// No __restrict__ and no read-only claim on Dt or E: the population kernel writes both between its passes.
__device__ __forceinline__ void three_opt_scan_lane(const float *Dt, size_t rs, const float *E, uint32_t n, uint32_t i, uint32_t jlo,
                                                    uint32_t jhi, uint32_t k0, uint32_t kstep, float &bs, uint32_t &bij, uint32_t &bkc)
{
    const float *Ra = Dt + i * rs, *Rb = Ra + rs;  // rows of a = path[i], b = path[i+1]
    const float d_ab = E[i];
    for (uint32_t k = k0; k < n; k += kstep) {
        if (i == 0u && k == n - 1u) continue;  // :81-83
        const float d_ef = E[k], d_ae = Ra[k], d_be = Rb[k], d_bf = Rb[k + 1u];
        const float *Rc = Dt + jlo * rs;
        float d_ce = Rc[k], d_cf = Rc[k + 1u];
        // software pipeline: the row of D = path[j+1] and the j terms of the NEXT iteration are in flight during this one
        float n_de = Rc[rs + k], n_dtf = Rc[rs + k + 1u];
        float n_c_dt = E[jlo], n_ac = Ra[jlo], n_a_dt = Ra[jlo + 1u], n_b_dt = Rb[jlo + 1u];
        for (uint32_t j = jlo; j < jhi; ++j) {  // wave-uniform trip count; j >= k is masked below
            const float d_de = n_de, d_dt_f = n_dtf;
            const float d_c_dt = n_c_dt, d_ac = n_ac, d_a_dt = n_a_dt, d_b_dt = n_b_dt;
            {   // rows up to jhi <= n-1 exist (row n-1 is the last), so j+2 needs a clamp at the very end
                const uint32_t jn = j + 1u < jhi ? j + 1u : j;  // last iteration: reload the same (unused) values
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
            // :113-117 leaves cmin = min(orig, c0..c6) (NaN costs never pass `c < cmin`; fminf drops them the same way),
            // and a triple matters only if it beats this lane's best so far — rare, so the case index is worked out
            // under a wave-uniform branch
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
                // :119-125 strict `>` in (i, j, k) loop order; a lane meets its triples k-major, so order by key
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
}

// the best move of a wave's 64 lanes, left in lane 0 (shuffles)
__device__ __forceinline__ void wave_best(float &bs, uint32_t &bij, uint32_t &bkc)
{
    for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_down(bs, off);
        const uint32_t oij = __shfl_down(bij, off), okc = __shfl_down(bkc, off);
        if (better(os, oij, okc, bs, bij, bkc)) { bs = os; bij = oij; bkc = okc; }
    }
}

// apply_3opt (three_opt.rs:186-218): seg1 = path[i+1..=j] (l1 entries) and seg2 = path[j+1..=k] (l2) are staged one behind the other;
// position i + 1 + t of the new path takes the staged entry returned here (0..l1-1 = seg1, l1.. = seg2)
__device__ __forceinline__ uint32_t three_opt_src(uint32_t kase, uint32_t t, uint32_t l1, uint32_t l2)
{
    const uint32_t L = l1 + l2;
    switch (kase) {
    case 1: return t < l1 ? (l1 - 1u - t) : t;                                  // rev(s1) + s2
    case 2: return t < l1 ? t : (l1 + (L - 1u - t));                            // s1 + rev(s2)
    case 3: return t < l1 ? (l1 - 1u - t) : (l1 + (L - 1u - t));                // rev(s1) + rev(s2)
    case 4: return t < l2 ? (l1 + t) : (t - l2);                                // s2 + s1
    case 5: return t < l2 ? (l1 + t) : (l1 - 1u - (t - l2));                    // s2 + rev(s1)
    case 6: return t < l2 ? (l1 + (l2 - 1u - t)) : (t - l2);                    // rev(s2) + s1
    default: return t < l2 ? (l1 + (l2 - 1u - t)) : (l1 - 1u - (t - l2));       // 7: rev(s2) + rev(s1)
    }
}

}  // namespace

}  // namespace tl
