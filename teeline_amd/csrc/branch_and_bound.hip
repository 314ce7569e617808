// branch_and_bound.hip — the depth-first branch and bound of DESIGN.md §4.27 (the bound is branch_bound.rs:240-268's: the running
// cost, the next edge, a minimum spanning tree over the start and the unvisited cities; the search order and the result are this
// project's specification, include/teeline_gpu.h).
// One WAVE owns a subtree; a lane is a city and, at the same time, a level of the search:
//   lane v   in Prim's algorithm holds min_key[v]; a step is one wave-wide minimum (DPP), a ballot, one conflict-free LDS row read
//            and a select.  The next child of a level is found the same way: the least (D(prev, c), c) over the level's untried
//            mask — the children of a node share its tree, so ascending D is ascending bound, and the first child that is cut
//            ends the level;
//   lane l   keeps level l of the depth-first search in registers: the position placed there, the mask of its untried siblings,
//            the f64 cost of the prefix and the tree's weight at the prefix.  A level is read with v_readlane and written under
//            `lane == l`, so the whole search state is five registers a lane and storing or restoring it is one coalesced access each.
// Visited sets, depth and every decision are wave-uniform (scalar registers, no divergence).
// A launch is BOUNDED: a wave takes at most `slice` nodes and leaves, stores its state and ends; the host relaunches (and, while the
// queue is shorter than the waves, splits untried siblings off unfinished searches).  A wave without a subtree takes the next
// ticket of the queue.  The shared upper bound is one u32 lowered with atomicMin; a leaf with L <= bound goes into the wave's own
// record if it beats it by (L, p) — the result does not depend on how the waves interleave.
#include "tl_kernels.h"

namespace tl {

namespace {

template <int CTRL>
__device__ __forceinline__ uint32_t bnb_dpp_shr_keep(uint32_t v)
{
    // row_shr within rows of 16 lanes; lanes without a source keep their own value
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
// the minimum over the wave, as a scalar (nn_knn.hip's form; all 64 lanes are active wherever this is called)
__device__ __forceinline__ uint32_t bnb_wave_min(uint32_t v)
{
    uint32_t o;
    o = bnb_dpp_shr_keep<0x111>(v); v = o < v ? o : v;
    o = bnb_dpp_shr_keep<0x112>(v); v = o < v ? o : v;
    o = bnb_dpp_shr_keep<0x114>(v); v = o < v ? o : v;
    o = bnb_dpp_shr_keep<0x118>(v); v = o < v ? o : v;  // lane 15 of each row: min of the row
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 47), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, uint32_t l) { return ((uint64_t)rl((uint32_t)(v >> 32), l) << 32) | rl((uint32_t)v, l); }
__device__ __forceinline__ double rld(double v, uint32_t l) { return __builtin_bit_cast(double, rl64(__builtin_bit_cast(uint64_t, v), l)); }
__device__ __forceinline__ uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float bitsf(uint32_t u) { return __builtin_bit_cast(float, u); }

__global__ __launch_bounds__(kBnbThreads) void k_bnb(BnbWs w, uint32_t n, uint32_t start, uint32_t slice, uint32_t ub0_bits, uint32_t has_start,
                                                     double factor)
{
    __shared__ float D[64 * 64];
    __shared__ uint64_t NK[64];
    for (uint32_t t = threadIdx.x; t < 64u * 64u; t += kBnbThreads) D[t] = w.D[t];
    if (threadIdx.x < 64u) NK[threadIdx.x] = w.nk[threadIdx.x];
    TL_SYNC();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = blockIdx.x * kBnbWavesPerGroup + (threadIdx.x >> 6);
    const size_t at = (size_t)wv * 64u + lane;
    const uint64_t full = n >= 64u ? ~(uint64_t)0 : (((uint64_t)1 << n) - 1u);
    const uint32_t qlen = uni(w.ctrl->queue_len);

    uint32_t active = uni(w.hdr[wv].active), k = uni(w.hdr[wv].k), base = uni(w.hdr[wv].base);
    uint32_t rec_has = uni(w.hdr[wv].rec_has), rec_bits = uni(w.hdr[wv].rec_bits);
    uint32_t path = w.path[at], rec = w.rec[at];
    uint64_t untried = w.untried[at];
    double cost = w.cost[at], mst = w.mst[at];
    uint64_t V = 0;  // the positions of path[0..k-1]
    if (active)
        for (uint32_t i = 0; i < k; ++i) V |= (uint64_t)1 << rl(path, i);

    // the node of the prefix path[0..k-1] (k < n): the tree over start and the unvisited positions, and the node's children
    auto expand = [&]() {
        const uint64_t unv = full & ~V;
        uint32_t key = ((unv >> lane) & 1u) ? fbits(D[start * 64u + lane]) : 0xFFFFFFFFu;
        double total = 0.0;
        for (uint64_t left = unv; left;) {
            const uint32_t kb = ((left >> lane) & 1u) ? key : 0xFFFFFFFFu;
            const uint32_t mn = bnb_wave_min(kb);
            const uint32_t u = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(kb == mn));
            total += (double)bitsf(mn);
            left &= ~((uint64_t)1 << u);
            const uint32_t du = fbits(D[u * 64u + lane]);
            key = du < key ? du : key;
        }
        uint64_t cand = NK[rl(path, k - 1u)] & unv;
        if (!cand) cand = unv;
        if (lane == k) {
            mst = total;
            untried = cand;
        }
    };

    uint32_t budget = slice, idle = 0;
    unsigned long long nodes = 0, leaves = 0;
    while (budget) {
        if (!active) {
            uint32_t t = 0;
            if (lane == 0) t = atomicAdd(&w.ctrl->ticket, 1u);
            t = uni(t);
            if (t >= qlen) {
                idle = 1;
                break;
            }
            const BnbItem *it = &w.queue[t];
            const uint32_t d = uni(it->depth);
            path = lane < d ? (uint32_t)it->path[lane] : 0u;
            V = 0;
            double acc = 0.0;
            for (uint32_t i = 0; i < d; ++i) {
                const uint32_t c = rl(path, i);
                if (i) acc += (double)D[rl(path, i - 1u) * 64u + c];
                if (lane == i) cost = acc;
                V |= (uint64_t)1 << c;
            }
            k = base = d;
            active = 1;
            expand();
            ++nodes;
            --budget;
            continue;
        }
        const uint64_t U = rl64(untried, k);
        if (!U) {  // the level is exhausted: the subtree is done, or one level up
            if (k == base) {
                active = 0;
                continue;
            }
            --k;
            V &= ~((uint64_t)1 << rl(path, k));
            continue;
        }
        const uint32_t prev = rl(path, k - 1u);
        const uint32_t kb = ((U >> lane) & 1u) ? fbits(D[prev * 64u + lane]) : 0xFFFFFFFFu;
        const uint32_t mn = bnb_wave_min(kb);
        const uint32_t c = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(kb == mn));
        const double nc = rld(cost, k - 1u) + (double)bitsf(mn);
        const uint32_t ub = uni(__hip_atomic_load(&w.ctrl->ub_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (nc + rld(mst, k) > (double)bitsf(ub) * factor) {  // the safe cut; every later child of the level has a larger bound
            if (lane == k) untried = 0;
            continue;
        }
        if (lane == k) {
            untried = U & ~((uint64_t)1 << c);
            path = c;
            cost = nc;
        }
        if (k + 1u == n) {  // a leaf: L as tl_tour_length sums it, the closing edge first
            const uint32_t nxt = (uint32_t)__shfl((int)path, (int)(lane + 1u < n ? lane + 1u : 0u), 64);
            const float e = lane < n ? D[path * 64u + nxt] : 0.0f;
            float L = readlane_f(e, (int)(n - 1u));
            for (uint32_t i = 0; i + 1u < n; ++i) L += readlane_f(e, (int)i);
            ++leaves;
            --budget;
            const uint32_t Lb = fbits(L);
            uint32_t old = 0;
            if (lane == 0) old = atomicMin(&w.ctrl->ub_bits, Lb);
            old = uni(old);
            bool take = Lb <= old && (!has_start || Lb < ub0_bits);
            if (take && rec_has) {
                if (Lb > rec_bits) take = false;
                else if (Lb == rec_bits) {
                    const uint64_t diff = __builtin_amdgcn_ballot_w64(lane < n && path != rec);
                    if (!diff) take = false;
                    else {
                        const uint32_t f = (uint32_t)__builtin_ctzll(diff);
                        take = rl(path, f) < rl(rec, f);
                    }
                }
            }
            if (take) {
                rec = path;
                rec_bits = Lb;
                rec_has = 1;
            }
            continue;
        }
        V |= (uint64_t)1 << c;
        ++k;
        expand();
        ++nodes;
        --budget;
    }

    w.path[at] = path;
    w.rec[at] = rec;
    w.untried[at] = untried;
    w.cost[at] = cost;
    w.mst[at] = mst;
    if (lane == 0) {
        BnbWaveHdr h;
        h.active = active;
        h.k = k;
        h.base = base;
        h.rec_has = rec_has;
        h.rec_bits = rec_bits;
        h.pad[0] = h.pad[1] = h.pad[2] = 0;
        w.hdr[wv] = h;
        if (nodes) atomicAdd(&w.ctrl->nodes, nodes);
        if (leaves) atomicAdd(&w.ctrl->leaves, leaves);
        if (idle) atomicAdd(&w.ctrl->idle, 1ull);
    }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

BnbWs bnb_ws_layout(void *ws, uint32_t waves, uint32_t queue_cap)
{
    BnbWs w;
    unsigned char *p = (unsigned char *)ws;
    auto take = [&p](size_t bytes) {
        unsigned char *at = p;
        p += up256(bytes);
        return at;
    };
    w.D = (float *)take(64 * 64 * sizeof(float));
    w.nk = (uint64_t *)take(64 * sizeof(uint64_t));
    w.ctrl = (BnbCtrl *)take(sizeof(BnbCtrl));
    w.queue = (BnbItem *)take((size_t)queue_cap * sizeof(BnbItem));
    w.hdr = (BnbWaveHdr *)take((size_t)waves * sizeof(BnbWaveHdr));
    w.path = (uint32_t *)take((size_t)waves * 64 * sizeof(uint32_t));
    w.untried = (uint64_t *)take((size_t)waves * 64 * sizeof(uint64_t));
    w.cost = (double *)take((size_t)waves * 64 * sizeof(double));
    w.mst = (double *)take((size_t)waves * 64 * sizeof(double));
    w.rec = (uint32_t *)take((size_t)waves * 64 * sizeof(uint32_t));
    return w;
}

size_t bnb_ws_bytes(uint32_t waves, uint32_t queue_cap)
{
    unsigned char *const origin = (unsigned char *)(uintptr_t)4096;  // only offsets are taken
    const BnbWs w = bnb_ws_layout(origin, waves, queue_cap);
    return (size_t)((unsigned char *)w.rec - origin) + up256((size_t)waves * 64 * sizeof(uint32_t));
}

hipError_t launch_bnb(const BnbWs &w, uint32_t n, uint32_t start, uint32_t slice, uint32_t workgroups, uint32_t ub0_bits, bool has_start,
                      double factor, hipStream_t s)
{
    hipLaunchKernelGGL(k_bnb, dim3(workgroups), dim3(kBnbThreads), 0, s, w, n, start, slice, ub0_bits, has_start ? 1u : 0u, factor);
    return hipGetLastError();
}

}  // namespace tl
