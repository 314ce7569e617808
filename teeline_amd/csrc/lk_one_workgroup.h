// lk_one_workgroup.h — k_lk_solve: lin_kernighan::solve (lin_kernighan.rs:35-100) as ONE persistent workgroup (a part of lk.hip).
// lk_pass (:454-481) scans the (t1, orientation) pairs in the reference's order NT at a time — every lane runs the depth-limited
// sequential chain search find_lk_chain (:265-340) for its pair, checks the closed chain for a single Hamiltonian cycle, and the
// lowest pair index with a valid chain wins (ds_min) — then the group applies the chain (apply_lk_chain, :397-450) by copying tour
// arcs, and rescans from the start exactly like find_lk_move does.  The ILS loop (double_bridge kicks :485-499, accept-if-shorter,
// plateau stop :75-97) runs on-device too.
//
// SMALL: every array the search touches — coordinates, candidate lists, tour, scratch tour, rank, successor, predecessor, scan
// order, best tour — lives in this CU's LDS (n (36 + 4k) bytes), so a node of the chain search costs LDS latencies and a move
// costs no kernel boundary.  Built as the candidate for small instances and MEASURED SLOWER than the
// chip-wide scans at every size: berlin52 with the CLI's options (3 327 scans) 129 ms against 80 ms, a280 517 against 349 ms,
// n = 1 500 933 against 58 ms (scripts/timing_lk.py, 64 / 256 / 1024 threads) — what a scan costs here is the single-lane
// stretches (segment table of apply_lk_chain, the ordered cost sum), not memory latency.  Kept as TL_FLAG_LK_SMALL (tuning build
// only), a cross-check of the state machine.
// !SMALL: the same code on the global arrays (TL_FLAG_LK_ONE_WORKGROUP).
#pragma once

template <int NT, bool SMALL>
__global__ __launch_bounds__(NT) void k_lk_solve(LkArgs G)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lk_small_smem[];
    __shared__ uint32_t s_key, s_clen, s_nseg;
    __shared__ uint32_t s_chain[kLkMaxChain];
    __shared__ LkSeg s_seg[kLkMaxSeg];
    __shared__ float s_part[NT];
    const uint32_t tid = threadIdx.x, n = G.n;
    uint32_t *tour = G.tour, *alt = G.alt, *pos = G.pos, *next = G.next, *prev = G.prev;
    uint32_t *city_ids = G.city_ids, *best = G.best;
    const float2 *xy = G.xy;
    const uint32_t *cand = G.cand;
    if (SMALL) {
        float2 *lxy = reinterpret_cast<float2 *>(lk_small_smem);
        uint32_t *w = reinterpret_cast<uint32_t *>(lk_small_smem + (size_t)n * 8);
        uint32_t *lcand = w;
        w += (size_t)n * G.k;
        tour = w; alt = w + n; pos = w + 2 * (size_t)n; next = w + 3 * (size_t)n; prev = w + 4 * (size_t)n;
        city_ids = w + 5 * (size_t)n; best = w + 6 * (size_t)n;
        for (uint32_t r = tid; r < n; r += NT) {
            lxy[r] = G.xy[r];
            tour[r] = G.tour[r];
        }
        for (size_t e = tid; e < (size_t)n * G.k; e += NT) lcand[e] = G.cand[e];
        xy = lxy;
        cand = lcand;
        TL_SYNC();
    }
    uint64_t scans = 0, searches = 0, moves = 0, exchanged = 0;

    auto rebuild = [&](const uint32_t *t) {  // make_pos + flat_to_next_prev (:110-145)
        for (uint32_t r = tid; r < n; r += NT) {
            const uint32_t c = t[r];
            pos[c] = r;
            next[c] = t[r + 1u == n ? 0u : r + 1u];
            prev[c] = t[r == 0u ? n - 1u : r - 1u];
        }
        TL_SYNC();
    };

    // tour_distance (:118-122): (0..n).map(d(t[i], t[(i+1)%n])).sum() — sequential f32 from 0, closing edge last
    auto tour_distance = [&](const uint32_t *t) -> float {
        float total = 0.0f;
        for (uint32_t base = 0; base < n; base += NT) {
            const uint32_t r = base + tid;
            if (r < n) {
                const uint32_t a = t[r], b = t[r + 1u == n ? 0u : r + 1u];
                s_part[tid] = a == b ? 0.0f : dist(xy[a], xy[b]);
            }
            TL_SYNC();
            if (tid == 0) {
                const uint32_t cnt = (n - base) < (uint32_t)NT ? (n - base) : (uint32_t)NT;
                for (uint32_t q = 0; q < cnt; ++q) total += s_part[q];
            }
            TL_SYNC();
        }
        if (tid == 0) s_part[0] = total;
        TL_SYNC();
        const float r = s_part[0];
        TL_SYNC();
        return r;
    };

    // lk_pass (:454-481) on `tour` (which must be G.tour); returns nothing, leaves the improved tour in G.tour
    auto lk_pass = [&]() {
        for (uint32_t r = tid; r < n; r += NT) city_ids[r] = tour[r];  // :466 fixed for the whole pass
        TL_SYNC();
        while (true) {
            rebuild(tour);  // :470
            LkView V{xy, cand, next, G.k, G.max_depth};
            bool found_any = false;
            for (uint32_t base = 0; base < 2u * n; base += NT) {  // find_lk_move (:345-389) in its own order
                if (tid == 0) s_key = 0xFFFFFFFFu;
                TL_SYNC();
                const uint32_t idx = base + tid;
                uint32_t chain[kLkMaxChain];
                uint32_t clen = 0;
                bool ok = false;
                if (idx < 2u * n) {
                    const uint32_t t1 = city_ids[idx >> 1];
                    const uint32_t t2 = (idx & 1u) ? prev[t1] : next[t1];  // :359 [next[t1], prev[t1]]
                    const float2 p1 = xy[t1], p2 = xy[t2];
                    chain[0] = t1;
                    chain[1] = t2;
                    const float g0 = t1 == t2 ? 0.0f : dist(p1, p2);
                    if (lk_chain<0, LkView>(V, chain, clen, p1, t2, p2, g0)) ok = chain_valid(chain, clen, tour, pos, n);
                }
                if (ok) atomicMin(&s_key, idx);
                TL_SYNC();
                const uint32_t key = s_key;
                if (key != 0xFFFFFFFFu) {
                    if (idx == key) {
                        s_clen = clen;
                        for (uint32_t t = 0; t < clen; ++t) s_chain[t] = chain[t];
                    }
                    searches += (uint64_t)key + 1u;
                    found_any = true;
                    TL_SYNC();
                    break;
                }
                TL_SYNC();
            }
            ++scans;
            if (!found_any) {
                searches += 2ull * n;
                break;
            }
            // ---- apply_lk_chain (:397-450): arcs copied in walk order from tour[0]
            if (tid == 0) {
                uint32_t chain[kLkMaxChain];
                const uint32_t clen = s_clen;
                for (uint32_t t = 0; t < clen; ++t) chain[t] = s_chain[t];
                uint32_t cpos[kLkMaxChain];
                chain_positions(chain, clen, pos, cpos);
                s_nseg = lk_build_segments(cpos, clen, n, s_seg);
            }
            TL_SYNC();
            const uint32_t nseg = s_nseg;
            for (uint32_t sidx = 0; sidx < nseg; ++sidx) {
                const LkSeg sg = s_seg[sidx];
                for (uint32_t t = tid; t < sg.len; t += NT) alt[sg.dst + t] = tour[seg_pos(sg, t, n)];
            }
            TL_SYNC();
            for (uint32_t r = tid; r < n; r += NT) tour[r] = alt[r];
            ++moves;
            exchanged += (uint64_t)(s_clen / 2u);
            TL_SYNC();
        }
    };

    // ---- lin_kernighan::solve (:35-100)
    if (n >= 4) {
        lk_pass();                                                   // :61-68
        for (uint32_t r = tid; r < n; r += NT) best[r] = tour[r];
        TL_SYNC();
        float best_dist = tour_distance(best);                       // :70
        uint32_t platoo = 0;
        uint64_t draws = 0;
        for (uint32_t e = 0; e < G.epochs; ++e) {                    // :75
            if (n < 8) {                                             // double_bridge (:485-499)
                for (uint32_t r = tid; r < n; r += NT) tour[r] = best[r];
            } else {
                uint32_t p1, p2, p3;
                double_bridge_cuts(G.seed, draws, n, p1, p2, p3);
                draws += 3;
                for (uint32_t w = tid; w < n; w += NT) tour[w] = best[double_bridge_src(w, p1, p2, p3)];
            }
            TL_SYNC();
            lk_pass();
            const float dcur = tour_distance(tour);
            if (dcur < best_dist) {                                  // :86
                for (uint32_t r = tid; r < n; r += NT) best[r] = tour[r];
                TL_SYNC();
                best_dist = dcur;
                platoo = 0;
            } else {
                if (++platoo >= G.platoo_epochs) break;              // :92-95
            }
        }
    } else {
        for (uint32_t r = tid; r < n; r += NT) best[r] = tour[r];
    }
    TL_SYNC();
    if (SMALL)
        for (uint32_t r = tid; r < n; r += NT) G.best[r] = best[r];
    if (tid == 0) {
        G.counters[0] = scans;
        G.counters[1] = searches;
        G.counters[2] = moves;
        G.counters[3] = exchanged;
    }
}

size_t lk_small_lds_bytes(uint32_t n, uint32_t k) { return (size_t)n * (36u + 4u * (size_t)k) + 16u; }

hipError_t launch_lk_solve(const LkArgs &G, hipStream_t s, bool small, int threads)
{
    if (!small) {
        hipLaunchKernelGGL((k_lk_solve<kLkNT, false>), dim3(1), dim3(kLkNT), 0, s, G);
        return hipGetLastError();
    }
#ifndef TL_TUNE  // the LDS-resident form loses to the chip-wide scans at every size: tuning build only
    (void)threads;
    return hipErrorInvalidValue;
#else
    const size_t lds = lk_small_lds_bytes(G.n, G.k);
    auto go = [&](auto kern, int nt) -> hipError_t {
        hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(1), dim3(nt), lds, s, G);
        return hipGetLastError();
    };
    (void)threads;  // 64 / 256 / 1024 threads measured (scripts/timing_lk.py): 256 is the best of the three up to n ~ 300
    return go(k_lk_solve<256, true>, 256);
#endif
}
