// or_opt_scan.h — what the two Or-opt kernels share (internal to libteeline_gpu): the packed argmin key and the wave's scan of
// kOrIR consecutive segment starts against a run of insertion points.  or_opt.hip (chip-wide pass over a tour in HBM) and
// or_opt_lds.hip (one workgroup per tour, the tour in LDS) include it, so both find the same move bit for bit.
#pragma once
#include "tl_kernels.h"

#pragma clang fp contract(off)

namespace tl {

namespace {

constexpr int kOrIR = 8;          // consecutive segment starts served from one set of distance registers
typedef unsigned __int128 key_t;  // (~delta bits) << 64 | loop-order index
constexpr unsigned long long kNoKey64 = ~0ULL;
__device__ __forceinline__ key_t make_key(unsigned long long hi, unsigned long long lo) { return ((key_t)hi << 64) | (key_t)lo; }
__device__ __forceinline__ key_t no_key() { return make_key(kNoKey64, kNoKey64); }

__device__ __forceinline__ key_t wave_min_key(key_t v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oh = __shfl_down((unsigned long long)(v >> 64), off), ol = __shfl_down((unsigned long long)v, off);
        const key_t o = make_key(oh, ol);
        v = o < v ? o : v;
    }
    return make_key(__shfl((unsigned long long)(v >> 64), 0), __shfl((unsigned long long)v, 0));
}

// every wave's minimum into its slot (two words per wave), a barrier, then the minimum of the nwaves slots — in every thread, so the
// whole workgroup goes the same way on it.  The caller's next write to the slots lies behind a barrier of its own.
__device__ __forceinline__ key_t block_min_key(key_t best, unsigned long long *slots, int lane, uint32_t wave, uint32_t nwaves)
{
    best = wave_min_key(best);
    if (lane == 0) {
        slots[2u * wave] = (unsigned long long)(best >> 64);
        slots[2u * wave + 1u] = (unsigned long long)best;
    }
    TL_SYNC();
    best = make_key(slots[0], slots[1]);
    for (uint32_t w = 1; w < nwaves; ++w) {
        const key_t o = make_key(slots[2u * w], slots[2u * w + 1u]);
        best = o < best ? o : best;
    }
    return best;
}

// The distance between two tour positions: tour-ordered coordinates Pt, or the packed matrix dm through the tour perm.  Pt and
// perm in HBM (or_opt.hip) or in LDS (or_opt_lds.hip).
template <bool DM>
struct Dist {
    const float2 *Pt;
    const float *dm;
    const uint32_t *perm;
    __device__ __forceinline__ float operator()(uint32_t kp, uint32_t kq) const  // tour positions
    {
        if (DM) return dm_lookup(dm, perm[kp], perm[kq]);
        return dist(Pt[kp], Pt[kq]);
    }
};

// One wave (all 64 lanes, converged) = kOrIR consecutive segment starts i0..i0+kOrIR-1 (i0 < n) x the insertion points of `chunks`
// chunks of 63 from jlo on.  D(kp, kq): the distance between two tour positions; E[k]: the tour edge (k, k+1).
// Every placement of the five kinds (len 1 fwd; len 2, 3 fwd and reversed) of a pair (i, j) is a sum of the row constant,
// the tour edge (x_j, y_j) and two distances out of { d(x_j, P[i+m]), d(y_j, P[i+m]) : m = 0, 1, 2 } — and y_j = x_{j+1}.
// So a chunk computes d(x_j, P[i0+m]) once for m = 0..kOrIR+1 (lane = j, lane 63 only supplies x of the next j),
// gets the y-distances from the neighbouring lane, and serves all kOrIR starts from those registers: 1.25 correctly
// rounded distances per (i, j) instead of the 10 a row-per-wave scan evaluates.  The f32 expressions keep the
// reference's association (or_opt.rs:136-139, :148-151); distances are symmetric bit for bit.
// best / bestd: this lane's lowest key so far and its delta, carried from one call to the next.
template <class DistF>
__device__ __forceinline__ void or_scan_rows(const DistF &D, const float *E, uint32_t n, uint32_t i0, uint32_t jlo, uint32_t chunks, int lane,
                                             key_t &best, float &bestd)
{
    // row constants: lane (len-1)*kOrIR + r holds -remove_gain of (seg_len, i0 + r) (:114-116), rowmask its validity (:90-92, :98-100)
    float nrg = 0.0f;
    bool rv = false;
    if (lane < 3 * kOrIR) {
        const uint32_t len = (uint32_t)lane / kOrIR + 1u, i = i0 + (uint32_t)lane % kOrIR;
        rv = i < n && n > len + 1u && i + len <= n;
        if (rv) {
            const uint32_t prev = i == 0u ? n - 1u : i - 1u, after = (i + len) % n, pl = i + len - 1u;
            const float remove_gain = D(prev, i) + D(pl, after) - D(prev, after);
            nrg = -remove_gain;
        }
    }
    const uint64_t rowmask = __builtin_amdgcn_ballot_w64(rv);
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t jb = jlo + c * 63u;
        if (jb >= n) break;
        const uint32_t j = jb + (uint32_t)lane;
        const bool real = lane < 63 && j < n;
        const uint32_t jj = j < n ? j : 0u;  // position of x_j; j == n is the wrap (y of j = n-1 is P[0]), lanes beyond are unused
        const float e = real ? E[j] : 0.0f;
        float dX[kOrIR + 2], dY[kOrIR + 2];
#pragma unroll
        for (int m = 0; m < kOrIR + 2; ++m) {
            const uint32_t pm = i0 + (uint32_t)m < n ? i0 + (uint32_t)m : n - 1u;  // beyond the tour: unused by any valid row
            dX[m] = D(jj, pm);
            // d(y_j, P[i0+m]) = d(x_{j+1}, P[i0+m]): the lane above, one DPP wave shift (lane 63, the helper lane, gets 0)
            dY[m] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, dX[m]), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
        }
#pragma unroll
        for (int r = 0; r < kOrIR; ++r) {
            const uint32_t i = i0 + (uint32_t)r;
            if (i >= n) break;
            const uint32_t prev = i == 0u ? n - 1u : i - 1u;
            // the five placements of (i, j); an invalid one (row or column excluded, :90-92, :98-100, :123-125) reads +inf.
            // Only when the smallest of them can still beat this lane's best are the 64-bit keys looked at.
            float val[5];
            const bool okj = real & (j != prev);
            const float inf = __builtin_inff();
#pragma unroll
            for (int len = 1; len <= 3; ++len) {
                const int rl = (len - 1) * kOrIR + r;
                const bool ok = okj & !((j - i) < (uint32_t)len) & (bool)((rowmask >> rl) & 1ull);
                const float nr = readlane_f(nrg, rl);
                const float fwd = nr + dX[r] + dY[r + len - 1] - e;  // :136-139  -rg + d(x,first) + d(last,y) - d(x,y)
                val[len == 1 ? 0 : 2 * len - 3] = ok ? fwd : inf;
                if (len > 1) {
                    const float rev = nr + dX[r + len - 1] + dY[r] - e;  // :148-151  -rg + d(x,last) + d(first,y) - d(x,y)
                    val[2 * len - 2] = ok ? rev : inf;
                }
            }
            const float vmin = fminf(fminf(fminf(val[0], val[1]), fminf(val[2], val[3])), val[4]);  // NaN deltas drop out like in `<`
            if (__builtin_amdgcn_ballot_w64((vmin < -1e-3f) & (vmin <= bestd))) {
#pragma unroll
                for (int q = 0; q < 5; ++q) {  // loop order within (i, j): len 1 fwd; len 2 fwd, rev; len 3 fwd, rev — the order index decides ties
                    const int len = q == 0 ? 1 : (q + 3) / 2;
                    const unsigned long long order = ((unsigned long long)((uint32_t)(len - 1) * n + i) * n + j) * 2ull + (unsigned long long)(q != 0 && (q & 1) == 0);
                    const float v = val[q];
                    if ((v < -1e-3f) & (v <= bestd)) {
                        const key_t key = make_key((unsigned long long)(~__builtin_bit_cast(uint32_t, v)), order);
                        if (key < best) {
                            best = key;
                            bestd = v;
                        }
                    }
                }
            }
        }
    }
}

// A found key's move (or_opt.rs:80-164): loop-order index = ((seg_len - 1) n + i) n + j, doubled, + reversed
struct OrMove {
    uint32_t i, j, seg_len, reversed;
};
__device__ __forceinline__ OrMove or_decode(key_t key, uint32_t n)
{
    const unsigned long long order = (unsigned long long)key;
    const unsigned long long row = (order >> 1) / n;
    return OrMove{(uint32_t)(row % n), (uint32_t)((order >> 1) % n), (uint32_t)(row / n) + 1u, (uint32_t)(order & 1ull)};
}

}  // namespace

}  // namespace tl
