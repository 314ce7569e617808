// three_opt.hip — best-improvement 3-opt (reference: src/tsp/three_opt.rs).
//
//   find_best_move (three_opt.rs:58-131): scan every i<j<k (i in [0,n-2), j in [i+1,n-1), k in [j+1,n),
//   skip i==0 && k==n-1, F = path[(k+1)%n] wraps), 7 reconnection costs (:170-180), per-triple first minimum
//   among the costs < orig (:113-117), global strict-max of savings = orig - cost in loop order (:119-125).
//   apply_3opt (:186-218), solve loop (:16-51): one move per pass.
//
// This one IS best-improvement in the reference, so the whole chip works on one pass:
//   k_three_opt_prepare   Pt[k] = xy[perm[k]] (tour order, Pt[n] = Pt[0]) and E[k] = d(path[k], path[(k+1)%n])
//   k_three_opt_build_dt  the n x n matrix of distances between tour POSITIONS (coordinates: one correctly rounded
//                         distance each; explicit matrices: one gather each), rebuilt every pass — O(n^2) next to
//                         the pass's O(n^3).
//   k_three_opt_scan      one workgroup per (i, chunk of JC consecutive j).  Distance ROWS are staged in LDS:
//                         Da[k] = d(a, path[k]), Db[k] (per i), and a rolling pair Dc / Dn with Dn(j) = Dc(j+1)
//                         because D = path[j+1] is the next j's C — so each (i,j) costs ONE new row of n-j
//                         coalesced loads from Dt.  Lanes run along k: 7 stride-1 LDS reads + ~25 VALU per triple;
//                         every f32 sum is associated exactly as the reference writes it, (x + y) + z.
//   k_three_opt_pick      reduces the per-workgroup bests (max savings, lowest (i,j,k) on ties == the reference's
//                         strict `>` in loop order) and applies the move (apply_3opt) in place.
// Roofline: VALU (one correctly rounded sqrt + 7 three-term sums per triple); algorithmic bytes in matrix form
// would be 48 B/triple — served here from LDS rows.
#include "three_opt_scan.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kT3 = 256;  // threads per scan workgroup

template <bool DM>
__device__ __forceinline__ float Dpos(const float2 *__restrict__ Pt, const float *__restrict__ dm,
                                      const uint32_t *__restrict__ perm, uint32_t kp, uint32_t kq, uint32_t n)
{
    // distance between tour positions kp and kq (kq may be n == wrap to 0)
    const uint32_t q = kq == n ? 0u : kq;
    if (DM) return dm_lookup(dm, perm[kp], perm[q]);
    return dist(Pt[kp], Pt[q]);
}

}  // namespace

template <bool DM>
__global__ __launch_bounds__(256) void k_three_opt_prepare(ThreeOptArgs A)
{
    if (A.run && A.run->done) return;  // a later pass of a batch whose descent is over
    const uint32_t n = A.n;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k <= n; k += gridDim.x * 256u) {
        const uint32_t kk = k == n ? 0u : k;
        if (!DM) A.Pt[k] = A.xy[A.perm[kk]];
    }
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        const uint32_t p = A.perm[k], q = A.perm[(k + 1u) == n ? 0u : (k + 1u)];
        A.E[k] = DM ? dm_lookup(A.dm, p, q) : dist(A.xy[p], A.xy[q]);
    }
}

template <bool DM>
__global__ __launch_bounds__(256) void k_three_opt_build_dt(ThreeOptArgs A)
{
    if (A.run && A.run->done) return;
    const uint32_t n = A.n, p = blockIdx.x, q = blockIdx.y * 256u + threadIdx.x;
    if (q > n) return;
    A.Dt[(size_t)p * (n + 1u) + q] = Dpos<DM>(A.Pt, A.dm, A.perm, p, q, n);
}

__global__ __launch_bounds__(kT3) void k_three_opt_scan(ThreeOptArgs A)
{
    if (A.run && A.run->done) return;
    const uint32_t n = A.n;
    __shared__ uint32_t s_i;
    __shared__ float r_s[kT3 / 64];
    __shared__ uint32_t r_ij[kT3 / 64], r_kc[kT3 / 64];
    const uint32_t tid = threadIdx.x;
    const size_t rs = (size_t)n + 1u;  // row stride of Dt; column n == column 0 (F = path[(k+1) % n], :85)

    // block -> (i, chunk): prefix[i] = number of chunks of rows < i
    if (tid == 0) {
        uint32_t lo = 0, hi = n - 2u;  // i in [0, n-2)
        const uint32_t b = blockIdx.x;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (A.chunk_prefix[mid] <= b) lo = mid;
            else hi = mid;
        }
        s_i = lo;
    }
    TL_SYNC();
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_i);  // provably wave-uniform: scalar loads for the (i, j) terms
    const uint32_t jlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i + 1u + (blockIdx.x - A.chunk_prefix[i]) * A.jc));
    uint32_t jhi = jlo + A.jc;
    if (jhi > n - 1u) jhi = n - 1u;  // j in [i+1, n-1)

    float bs = 0.0f;  // three_opt.rs:61 best_savings = 0.0
    uint32_t bij = 0xFFFFFFFFu, bkc = 0xFFFFFFFFu;
    three_opt_scan_lane(A.Dt, rs, A.E, n, i, jlo, jhi, jlo + 1u + tid, kT3, bs, bij, bkc);  // lanes along k (three_opt_scan.h)

    // workgroup reduction: wave (shuffles) then LDS
    wave_best(bs, bij, bkc);
    if ((tid & 63u) == 0u) { r_s[tid >> 6] = bs; r_ij[tid >> 6] = bij; r_kc[tid >> 6] = bkc; }
    TL_SYNC();
    if (tid == 0) {
        for (int w = 1; w < kT3 / 64; ++w)
            if (better(r_s[w], r_ij[w], r_kc[w], bs, bij, bkc)) { bs = r_s[w]; bij = r_ij[w]; bkc = r_kc[w]; }
        ThreeOptBest *o = A.partials + blockIdx.x;
        o->sav = bs;
        o->ij = bij;
        o->kc = bkc;
    }
}

// one workgroup: reduce the partials, publish the move, optionally apply it (apply_3opt, three_opt.rs:186-218)
__global__ __launch_bounds__(1024) void k_three_opt_pick(ThreeOptArgs A, uint32_t nblocks, int apply, int stage_lds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the two segments of the move: in LDS where n entries fit, else in the workspace (one workgroup: its own barrier orders the copy)
    uint32_t *tmp = stage_lds ? reinterpret_cast<uint32_t *>(smem) : A.scratch;
    __shared__ float r_s[16];
    __shared__ uint32_t r_ij[16], r_kc[16];
    const uint32_t tid = threadIdx.x;
    if (A.run && A.run->done) return;
    float bs = 0.0f;
    uint32_t bij = 0xFFFFFFFFu, bkc = 0xFFFFFFFFu;
    for (uint32_t b = tid; b < nblocks; b += 1024u) {
        const ThreeOptBest p = A.partials[b];
        if (better(p.sav, p.ij, p.kc, bs, bij, bkc)) { bs = p.sav; bij = p.ij; bkc = p.kc; }
    }
    wave_best(bs, bij, bkc);
    if ((tid & 63u) == 0u) { r_s[tid >> 6] = bs; r_ij[tid >> 6] = bij; r_kc[tid >> 6] = bkc; }
    TL_SYNC();
    bs = r_s[0]; bij = r_ij[0]; bkc = r_kc[0];
    for (int w = 1; w < 16; ++w)
        if (better(r_s[w], r_ij[w], r_kc[w], bs, bij, bkc)) { bs = r_s[w]; bij = r_ij[w]; bkc = r_kc[w]; }
    const bool found = bkc != 0xFFFFFFFFu;  // savings > 0 was required to record a move
    if (tid == 0) {
        A.best->sav = bs;
        A.best->ij = bij;
        A.best->kc = bkc;
        A.best->found = found ? 1u : 0u;
        if (apply) {
            A.counters[0] += 1;                  // passes
            if (found) A.counters[1] += 1;       // moves
        }
        scan_file_pass(A.run, A.log, found, bij >> 16, bij & 0xFFFFu, bkc >> 3, bkc & 7u);  // three_opt.rs:36-45
    }
    if (!found || !apply) return;
    const uint32_t i = bij >> 16, j = bij & 0xFFFFu, k = bkc >> 3, kase = bkc & 7u;
    uint32_t *path = A.perm;
    const uint32_t l1 = j - i, l2 = k - j, L = l1 + l2;  // seg1 = path[i+1..=j], seg2 = path[j+1..=k]
    for (uint32_t t = tid; t < L; t += 1024u) tmp[t] = path[i + 1u + t];
    TL_SYNC();
    for (uint32_t t = tid; t < L; t += 1024u) path[i + 1u + t] = tmp[three_opt_src(kase, t, l1, l2)];
}

size_t three_opt_scan_lds_bytes(uint32_t) { return 0; }  // the scan keeps its rows in registers

hipError_t launch_three_opt_pass(const ThreeOptArgs &A, uint32_t nblocks, bool dm, int apply, hipStream_t s, int lds_budget)
{
    const uint32_t pg = (A.n + 256u) / 256u;
    const size_t lds = three_opt_scan_lds_bytes(A.n);
    hipError_t e;
    const dim3 dg(A.n, (A.n + 1u + 255u) / 256u);
    if (dm) {
        hipLaunchKernelGGL(k_three_opt_prepare<true>, dim3(pg), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_three_opt_build_dt<true>, dg, dim3(256), 0, s, A);
    } else {
        hipLaunchKernelGGL(k_three_opt_prepare<false>, dim3(pg), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_three_opt_build_dt<false>, dg, dim3(256), 0, s, A);
    }
    e = allow_max_lds(reinterpret_cast<const void *>(k_three_opt_scan));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_three_opt_scan, dim3(nblocks), dim3(kT3), lds, s, A);
    e = allow_max_lds(reinterpret_cast<const void *>(k_three_opt_pick));
    if (e != hipSuccess) return e;
    // LDS up to 256 cities, the workspace beyond: both forms run in the parity tests at sizes the oracle affords (the copy is one
    // workgroup's and L2-resident either way; the scan is what a pass costs)
    const bool stage_lds = A.n <= 256u && (size_t)A.n * 4 + 2048 <= (size_t)lds_budget;
    hipLaunchKernelGGL(k_three_opt_pick, dim3(1), dim3(1024), stage_lds ? (size_t)A.n * 4 : 0, s, A, nblocks, apply, stage_lds ? 1 : 0);
    return hipGetLastError();
}

}  // namespace tl
