// greedy_edge.hip — greedy-edge construction (reference: src/tsp/greedy_edge.rs:21-65 over graph.rs:54-196), DESIGN.md §4.11,
// savings construction (src/tsp/savings.rs:34-163: the same selection under another sort key), DESIGN.md §4.12, and the greedy
// matching of Christofides (src/tsp/christofides.rs:138-166: the same bands, capacity 1 instead of 2, no cycle test), §4.13.
//
// The reference sorts all n(n-1)/2 edges by f32::total_cmp of their length and walks them once (select_edges): an edge is skipped
// if an endpoint already has degree 2, or if it would close a cycle before n - 1 edges are in.  Both rejections are final (degrees
// never fall, fragments never split), so this build never materialises the O(n^2) list.  It walks the edges in BANDS of at most
// `cap` keys (greedy_band_cap: 16 384 on 160 KB of LDS), each band being every still-possible edge in a key interval (T_prev, T]:
//   k_ge_hist     histogram of one 12-bit digit of the keys of all pairs of still-free cities (degree < 2) above T_prev: the host
//                 picks T so that the band holds as many keys as fit one workgroup's LDS (refining into a digit when a bin is crowded)
//   k_ge_compact  those keys, unordered
//   k_ge_sort     bitonic sort in one workgroup's LDS
//   k_ge_walk     select_edges over the band in one wave, with the fragment-end table in LDS
// until n edges are accepted.  Then k_ge_arcs / k_ge_jump / k_ge_emit turn the two neighbour slots of every city into the path
// (hamiltonian_cycle_to_path) by list ranking over the 2n directed arcs.
//
// Key of the edge (i < j): (total-order key of d) << 32 | i << 16 | j — the reference's order with ties broken by (i, j) ascending
// (its sort_unstable_by leaves that order open).  Positions fit 16 bits: n <= 65 535 (tl_greedy_edge refuses more).
// Savings swaps the upper word for KeySavings' (below); nothing else of the band scheme depends on what the key orders by: both
// rejections are final, degrees never fall, fragments never split.
#include "tl_kernels.h"

namespace tl {

namespace {

constexpr int kGeRows = 16;     // rows (first cities) of a pair tile
constexpr int kGeCols = 256;    // columns (second cities) of a pair tile = threads of the enumeration kernels
constexpr uint16_t kGeFull = 0xFFFFu;  // end-table sentinel: degree 2

// f32::total_cmp as an unsigned order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN
__device__ __forceinline__ uint32_t total_key(float d)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Key policies: the upper 32 bits of an edge's sort key from its length d and its two endpoints (the lower 32 are i << 16 | j).
// greedy-edge: ascending f32::total_cmp of the length
struct KeyLength {
    __device__ __forceinline__ uint32_t operator()(float d, uint32_t, uint32_t) const { return total_key(d); }
};

constexpr uint32_t kSavNanKey = 0xFF800001u;  // one past -inf's inverted key (~total_key(-inf) = 0xFF800000)

// savings (savings.rs:136-163): s = (dh[i] + dh[j]) - d in two f32 operations in that order (the sum commutes bit for bit, so
// which endpoint is i does not matter), DESCENDING f32::total_cmp — the inverted total-order key — with -0.0 and +0.0 distinct
// and subnormals kept.  A NaN saving of any sign or payload (inf - inf is +NaN here and -NaN on x86; total_cmp would put them at
// opposite ends) is ONE value that ranks below every number, after -inf: tested explicitly, never this device's default NaN.
// What the host relies on (tl_api_greedy.hip) holds as for KeyLength: every key is > 0 (j >= 1 in the low bits), and no key is
// all-ones (the largest upper word is kSavNanKey — ~total_key(s) of a non-NaN s is at most 0xFF800000 — and i < j <= 65 534 keeps
// the low word below 0xFFFFFFFF too), so ~0 stays free as the sort's padding and as "every edge walked".
struct KeySavings {
    const float *__restrict__ dh;
    __device__ __forceinline__ uint32_t operator()(float d, uint32_t i, uint32_t j) const
    {
        const float s = (dh[i] + dh[j]) - d;
        return s != s ? kSavNanKey : ~total_key(s);
    }
};

constexpr uint32_t kMatchNanKey = 0xFF800001u;  // one past +inf's key (total_key(+inf) = 0xFF800000)

// Christofides' matching (christofides.rs:153): ascending partial_cmp of the length, so -0.0 and +0.0 are ONE value (zero is
// canonicalised before the total-order key is formed).  A NaN length makes the reference's comparator inconsistent and its order
// unspecified; here a NaN of any sign or payload is ONE value above +inf, ties by (i, j).  The host's invariants
// hold as for the other two: every key is > 0 (j >= 1), none is all-ones (the largest upper word is kMatchNanKey).
struct KeyMatching {
    __device__ __forceinline__ uint32_t operator()(float d, uint32_t, uint32_t) const
    {
        if (d != d) return kMatchNanKey;
        return total_key(d == 0.0f ? 0.0f : d);
    }
};

// Calls visit(key) for every pair a < b of the free list (positions free[a], free[b]), tile by tile over a grid-stride loop.
template <bool DM, class Key, class Visit>
__device__ __forceinline__ void for_each_pair(const float2 *__restrict__ xy, const float *__restrict__ dm, const uint16_t *__restrict__ free,
                                              uint32_t f, Key key32, Visit visit)
{
    const uint32_t nrt = (f + kGeRows - 1) / kGeRows, ncb = (f + kGeCols - 1) / kGeCols;
    const uint64_t tiles = (uint64_t)nrt * ncb;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t rt = (uint32_t)(t / ncb), cb = (uint32_t)(t % ncb);
        const uint32_t a0 = rt * kGeRows, b = cb * kGeCols + threadIdx.x;
        if (cb * kGeCols + kGeCols - 1 <= a0) continue;  // the whole tile lies on or below the diagonal (uniform)
        if (b >= f) continue;
        const uint32_t pb = free[b];
        float2 qb = make_float2(0.f, 0.f);
        if (!DM) qb = xy[pb];  // (the distance is symmetric bit for bit: (p - q)^2 == (q - p)^2)
        const uint32_t aend = a0 + kGeRows < f ? a0 + kGeRows : f;
        for (uint32_t a = a0; a < aend && a < b; ++a) {
            const uint32_t pa = free[a];
            const uint32_t i = pa < pb ? pa : pb, j = pa < pb ? pb : pa;
            float d;
            if (DM) d = dm[(uint64_t)j * (j - 1) / 2 + i];
            else d = dist(xy[pa], qb);
            visit(((uint64_t)key32(d, i, j) << 32) | ((uint64_t)i << 16) | (uint64_t)j);
        }
    }
}

constexpr int kGeDigitBits = 12;
constexpr int kGeBins = 1 << kGeDigitBits;

// Histogram of digit (key >> shift) & (2^width - 1) over the pairs with key > t_prev whose bits above shift + width equal `prefix`.
template <bool DM, class Key>
__global__ __launch_bounds__(kGeCols) void k_ge_hist(const float2 *__restrict__ xy, const float *__restrict__ dm,
                                                     const uint16_t *__restrict__ free, const uint32_t *__restrict__ state,
                                                     uint64_t t_prev, uint64_t prefix, uint32_t shift, uint32_t width,
                                                     uint32_t *__restrict__ hist, Key key32)
{
    __shared__ uint32_t lh[kGeBins];
    for (int k = threadIdx.x; k < kGeBins; k += kGeCols) lh[k] = 0;
    TL_SYNC();
    const uint32_t f = state[4];
    const uint32_t pshift = shift + width;
    const uint64_t mask = ((uint64_t)1 << width) - 1;
    for_each_pair<DM>(xy, dm, free, f, key32, [&](uint64_t key) {
        if (key > t_prev && (pshift >= 64 || (key >> pshift) == prefix)) atomicAdd(&lh[(key >> shift) & mask], 1u);
    });
    TL_SYNC();
    for (int k = threadIdx.x; k < kGeBins; k += kGeCols)
        if (lh[k]) atomicAdd(&hist[k], lh[k]);
}

// Every pair key in (t_lo, t_hi], unordered; state[3] counts them (the host has sized the band: never more than cap)
template <bool DM, class Key>
__global__ __launch_bounds__(kGeCols) void k_ge_compact(const float2 *__restrict__ xy, const float *__restrict__ dm,
                                                        const uint16_t *__restrict__ free, uint32_t *__restrict__ state,
                                                        uint64_t t_lo, uint64_t t_hi, uint64_t *__restrict__ keys, uint32_t cap, Key key32)
{
    const uint32_t f = state[4];
    for_each_pair<DM>(xy, dm, free, f, key32, [&](uint64_t key) {
        if (key > t_lo && key <= t_hi) {
            const uint32_t at = atomicAdd(&state[3], 1u);
            if (at < cap) keys[at] = key;
        }
    });
}

// Ascending bitonic sort of the band (count <= cap, a power of two whose keys fit LDS) in one workgroup
__global__ __launch_bounds__(1024) void k_ge_sort(uint64_t *__restrict__ keys, const uint32_t *__restrict__ state, uint32_t cap)
{
    extern __shared__ uint64_t sk[];
    const uint32_t count = state[3] < cap ? state[3] : cap;
    uint32_t np = 1;
    while (np < count) np <<= 1;
    for (uint32_t k = threadIdx.x; k < np; k += blockDim.x) sk[k] = k < count ? keys[k] : ~(uint64_t)0;
    TL_SYNC();
    for (uint32_t size = 2; size <= np; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t k = threadIdx.x; k < np; k += blockDim.x) {
                const uint32_t m = k ^ stride;
                if (m > k) {
                    const uint64_t x = sk[k], y = sk[m];
                    const bool up = (k & size) == 0;
                    if ((x > y) == up) {
                        sk[k] = y;
                        sk[m] = x;
                    }
                }
            }
            TL_SYNC();
        }
    }
    for (uint32_t k = threadIdx.x; k < count; k += blockDim.x) keys[k] = sk[k];
}

// state: [0] accepted edges, [1..2] edges examined (u64, lo / hi), [3] keys in the band, [4] free cities (the free list's length)
//
// select_edges (graph.rs:98-126) over one sorted band, one wave.  end[c] (LDS, u16): c itself at degree 0, the other end of c's
// path fragment at degree 1, kGeFull at degree 2 — so "u and v already connected" (both of degree < 2) is end[u] == v.
// Each chunk of 64 keys is first tested by all lanes against the state at the chunk's start: a degree-2 endpoint rejects for
// good, and so does end[u] == v while fewer than n - 1 edges can be in before that key.  Lane 0 then walks the survivors in order
// with the exact test.  An accepted edge (u, v) lands in the first free of the two neighbour slots of u and of v (slot 0 = the
// earlier edge: adj[c][0] of hamiltonian_cycle_to_path).  At the end the wave writes the table back and lists the free cities.
// MATCH (greedy_matching, christofides.rs:158-164): a city's capacity is 1 — the table holds c for an unmatched odd vertex and
// kGeFull for everything else — so a pair is taken iff neither end is full, both ends then are, there is no cycle test, and the
// pairs go to slots[2a], slots[2a + 1] in acceptance order (a = the pair's index) until `target` = k / 2 of them are in.
template <bool MATCH>
__global__ __launch_bounds__(64) void k_ge_walk(const uint64_t *__restrict__ keys, uint32_t *__restrict__ state, uint16_t *__restrict__ end_g,
                                                uint32_t *__restrict__ slots, uint16_t *__restrict__ free, uint32_t n, uint32_t cap,
                                                uint32_t target)
{
    const uint32_t goal = MATCH ? target : n;
    extern __shared__ uint16_t lend[];
    __shared__ uint32_t ch[64];
    __shared__ uint32_t sh_acc, sh_done;
    const uint32_t l = threadIdx.x;
    for (uint32_t k = l; k < n; k += 64) lend[k] = end_g[k];
    const uint32_t count = state[3] < cap ? state[3] : cap;
    uint32_t acc = state[0];
    uint64_t examined = 0;
    if (l == 0) sh_done = 0;
    TL_SYNC();
    for (uint32_t base = 0; base < count && acc < goal; base += 64) {
        const bool valid = base + l < count;
        uint32_t u = 0, v = 0;
        bool alive = false;
        if (valid) {
            const uint64_t key = keys[base + l];
            u = (uint32_t)(key >> 16) & 0xFFFFu;
            v = (uint32_t)key & 0xFFFFu;
            const uint32_t eu = lend[u], ev = lend[v];
            alive = eu != kGeFull && ev != kGeFull && (MATCH || !(eu == v && acc + 64 < n));
        }
        ch[l] = (u << 16) | v;
        uint64_t live = __builtin_amdgcn_ballot_w64(alive);
        TL_SYNC();
        if (l == 0) {
            uint32_t stop = 0;
            while (live) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(live);
                live &= live - 1;
                const uint32_t uu = ch[bit] >> 16, vv = ch[bit] & 0xFFFFu;
                const uint32_t eu = lend[uu], ev = lend[vv];
                if (eu == kGeFull || ev == kGeFull) continue;
                if constexpr (MATCH) {
                    slots[2 * acc] = uu;
                    slots[2 * acc + 1] = vv;
                    lend[uu] = kGeFull;
                    lend[vv] = kGeFull;
                } else {
                    if (eu == vv && acc != n - 1) continue;
                    const uint32_t du = eu != uu, dv = ev != vv;  // degree before this edge (0 / 1)
                    slots[2 * uu + du] = vv;
                    slots[2 * vv + dv] = uu;
                    lend[eu] = (uint16_t)ev;
                    lend[ev] = (uint16_t)eu;
                    if (du) lend[uu] = kGeFull;
                    if (dv) lend[vv] = kGeFull;
                }
                if (++acc == goal) {
                    stop = bit + 1;
                    break;
                }
            }
            sh_acc = acc;
            sh_done = stop;
        }
        TL_SYNC();
        acc = sh_acc;
        if (sh_done) {
            examined += sh_done;
            break;
        }
        examined += count - base < 64 ? count - base : 64;
    }
    // write back; list the free cities in position order (ballot compaction)
    uint32_t nf = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 64) {
        const uint32_t k = b0 + l;
        const uint16_t e = k < n ? lend[k] : kGeFull;
        if (k < n) end_g[k] = e;
        const uint64_t m = __builtin_amdgcn_ballot_w64(e != kGeFull);
        if (e != kGeFull) free[nf + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)k;
        nf += (uint32_t)__builtin_popcountll(m);
    }
    if (l == 0) {
        const uint64_t ex = ((uint64_t)state[2] << 32 | state[1]) + examined;
        state[0] = acc;
        state[1] = (uint32_t)ex;
        state[2] = (uint32_t)(ex >> 32);
        state[4] = nf;
    }
}

__global__ __launch_bounds__(256) void k_ge_init(uint16_t *__restrict__ end_g, uint16_t *__restrict__ free, uint32_t *__restrict__ state, uint32_t n)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) {
        end_g[k] = (uint16_t)k;
        free[k] = (uint16_t)k;
    }
    if (k < 8) state[k] = k == 4 ? n : 0u;
}

// savings: dh[k] = d(hub, k), +0.0 at the hub itself (distance_by_pos's diagonal rule, also where the coordinates are inf or NaN)
template <bool DM>
__global__ __launch_bounds__(256) void k_sav_dh(const float2 *__restrict__ xy, const float *__restrict__ dm, uint32_t n, uint32_t hub,
                                                float *__restrict__ dh)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    float d = 0.f;
    if (k != hub) {
        const uint32_t i = k < hub ? k : hub, j = k < hub ? hub : k;
        if (DM) d = dm[(uint64_t)j * (j - 1) / 2 + i];
        else d = dist(xy[hub], xy[k]);
    }
    dh[k] = d;
}

constexpr uint32_t kGeEnd = 0xFFFFFFFFu;

// Arc 2c + s runs from c to slots[2c + s]; its successor leaves that city by the other slot.  The arc whose successor would be
// arc 0 (from position 0 along its earlier-accepted edge) ends the list.
__global__ __launch_bounds__(256) void k_ge_arcs(const uint32_t *__restrict__ slots, uint32_t n, uint32_t *__restrict__ succ, uint32_t *__restrict__ dist_to_end)
{
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= 2 * n) return;
    const uint32_t c = a >> 1, w = slots[a];
    if (w >= n) {  // (cannot happen once n edges are in: every slot is written)
        succ[a] = kGeEnd;
        dist_to_end[a] = n;
        return;
    }
    const uint32_t t = slots[2 * w] == c ? 1u : 0u;
    const uint32_t s = 2 * w + t;
    succ[a] = s == 0 ? kGeEnd : s;
    dist_to_end[a] = s == 0 ? 0u : 1u;
}

// one round of pointer jumping (Wyllie)
__global__ __launch_bounds__(256) void k_ge_jump(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ dte, uint32_t *__restrict__ succ2,
                                                 uint32_t *__restrict__ dte2, uint32_t n)
{
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= 2 * n) return;
    const uint32_t s = succ[a];
    if (s == kGeEnd) {
        succ2[a] = kGeEnd;
        dte2[a] = dte[a];
    } else {
        succ2[a] = succ[s];
        dte2[a] = dte[a] + dte[s];
    }
}

// arcs that reached the end are the path's orientation: arc 0 is n - 1 arcs from it, so the source of an arc d from the end sits at n - 1 - d
__global__ __launch_bounds__(256) void k_ge_emit(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ dte, uint32_t n, uint32_t *__restrict__ out_pos)
{
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= 2 * n) return;
    if (succ[a] == kGeEnd && dte[a] < n) out_pos[n - 1 - dte[a]] = a >> 1;
}

}  // namespace

uint32_t greedy_band_cap(int lds_bytes)
{
    uint32_t cap = 16384;
    while (cap > 64 && (size_t)cap * 8 + 1024 > (size_t)lds_bytes) cap >>= 1;
    return cap;
}

size_t greedy_ws_bytes(uint32_t n, uint32_t cap)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    return up((size_t)cap * 8) + up((size_t)kGeBins * 4) + 256 + 2 * up((size_t)n * 2) + 5 * up((size_t)n * 8) + up((size_t)n * 4);
}

GreedyWs greedy_ws_layout(void *ws, uint32_t n, uint32_t cap)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    unsigned char *p = (unsigned char *)ws;
    GreedyWs w;
    w.keys = (uint64_t *)p, p += up((size_t)cap * 8);
    w.hist = (uint32_t *)p, p += up((size_t)kGeBins * 4);
    w.state = (uint32_t *)p, p += 256;
    w.end = (uint16_t *)p, p += up((size_t)n * 2);
    w.free = (uint16_t *)p, p += up((size_t)n * 2);
    w.slots = (uint32_t *)p, p += up((size_t)n * 8);
    w.succ[0] = (uint32_t *)p, p += up((size_t)n * 8);
    w.succ[1] = (uint32_t *)p, p += up((size_t)n * 8);
    w.dte[0] = (uint32_t *)p, p += up((size_t)n * 8);
    w.dte[1] = (uint32_t *)p, p += up((size_t)n * 8);
    w.dh = (float *)p;
    w.cap = cap;
    return w;
}

hipError_t launch_greedy_init(const GreedyWs &w, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_ge_init, dim3((n + 255) / 256), dim3(256), 0, s, w.end, w.free, w.state, n);
    return hipGetLastError();
}

hipError_t launch_savings_dh(const GreedyWs &w, const float2 *xy, const float *dm, uint32_t n, uint32_t hub, hipStream_t s)
{
    if (dm) hipLaunchKernelGGL(k_sav_dh<true>, dim3((n + 255) / 256), dim3(256), 0, s, xy, dm, n, hub, w.dh);
    else hipLaunchKernelGGL(k_sav_dh<false>, dim3((n + 255) / 256), dim3(256), 0, s, xy, dm, n, hub, w.dh);
    return hipGetLastError();
}

namespace {

// Calls f(policy) with the key policy `key` names
template <class F>
hipError_t with_key(GreedyKey key, const GreedyWs &w, F f)
{
    if (key == kGeKeySavings) return f(KeySavings{w.dh});
    if (key == kGeKeyMatching) return f(KeyMatching{});
    return f(KeyLength{});
}

int pair_grid(uint32_t f, int blocks)
{
    const uint64_t tiles = (uint64_t)((f + kGeRows - 1) / kGeRows) * ((f + kGeCols - 1) / kGeCols);
    return (int)(tiles < (uint64_t)blocks ? (tiles ? tiles : 1) : (uint64_t)blocks);
}

}  // namespace

hipError_t launch_greedy_hist(const GreedyWs &w, const float2 *xy, const float *dm, uint32_t f, uint64_t t_prev, uint64_t prefix,
                              uint32_t shift, uint32_t width, int blocks, GreedyKey key, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(w.hist, 0, (size_t)kGeBins * 4, s);
    if (e != hipSuccess) return e;
    const int g = pair_grid(f, blocks);
    return with_key(key, w, [&](auto k) {
        using K = decltype(k);
        if (dm) hipLaunchKernelGGL((k_ge_hist<true, K>), dim3(g), dim3(kGeCols), 0, s, xy, dm, w.free, w.state, t_prev, prefix, shift, width, w.hist, k);
        else hipLaunchKernelGGL((k_ge_hist<false, K>), dim3(g), dim3(kGeCols), 0, s, xy, dm, w.free, w.state, t_prev, prefix, shift, width, w.hist, k);
        return hipGetLastError();
    });
}

hipError_t launch_greedy_band(const GreedyWs &w, const float2 *xy, const float *dm, uint32_t n, uint32_t f, uint64_t t_lo, uint64_t t_hi,
                              int blocks, GreedyKey key, uint32_t target, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(w.state + 3, 0, 4, s);
    if (e != hipSuccess) return e;
    const int g = pair_grid(f, blocks);
    e = with_key(key, w, [&](auto k) {
        using K = decltype(k);
        if (dm) hipLaunchKernelGGL((k_ge_compact<true, K>), dim3(g), dim3(kGeCols), 0, s, xy, dm, w.free, w.state, t_lo, t_hi, w.keys, w.cap, k);
        else hipLaunchKernelGGL((k_ge_compact<false, K>), dim3(g), dim3(kGeCols), 0, s, xy, dm, w.free, w.state, t_lo, t_hi, w.keys, w.cap, k);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    if ((e = allow_max_lds((const void *)k_ge_sort)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ge_sort, dim3(1), dim3(1024), (size_t)w.cap * 8, s, w.keys, w.state, w.cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t lds = ((size_t)n * 2 + 15) & ~(size_t)15;
    if (key == kGeKeyMatching) {
        if ((e = allow_max_lds((const void *)k_ge_walk<true>)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_ge_walk<true>, dim3(1), dim3(64), lds, s, w.keys, w.state, w.end, w.slots, w.free, n, w.cap, target);
    } else {
        if ((e = allow_max_lds((const void *)k_ge_walk<false>)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_ge_walk<false>, dim3(1), dim3(64), lds, s, w.keys, w.state, w.end, w.slots, w.free, n, w.cap, n);
    }
    return hipGetLastError();
}

hipError_t launch_greedy_path(const GreedyWs &w, uint32_t n, uint32_t *out_pos, hipStream_t s)
{
    const dim3 g((2 * n + 255) / 256);
    hipLaunchKernelGGL(k_ge_arcs, g, dim3(256), 0, s, w.slots, n, w.succ[0], w.dte[0]);
    hipError_t e = hipGetLastError();
    int cur = 0;
    for (uint32_t span = 1; span < n && e == hipSuccess; span <<= 1, cur ^= 1) {
        hipLaunchKernelGGL(k_ge_jump, g, dim3(256), 0, s, w.succ[cur], w.dte[cur], w.succ[cur ^ 1], w.dte[cur ^ 1], n);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ge_emit, g, dim3(256), 0, s, w.succ[cur], w.dte[cur], n, out_pos);
    return hipGetLastError();
}

}  // namespace tl
