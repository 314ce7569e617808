"""The specification of the project's ant colony solver, in numpy (TEST infrastructure, not product code).

ant_colony.rs:97-252 and probability.rs:69-79 with two deliberate differences, because the reference's unseeded thread RNG and the
platform's `powf` cannot be reproduced: the random draws are a pure function of (seed, run, event, slot) — the stream of
tests/_ga_oracle.py — and the power is a fixed f64 operation sequence (teeline_amd/csrc/aco_spec.h).  Everything else is the
reference's, quirks included: select_next's sequential f32 sums over the unvisited cities in city order and its two fallbacks,
roulette_select's strict `acc > r * sum` and its last-candidate fallback, the closing edge first in the cost, `cost < best_cost`
strict and in ant order, evaporation floored at tau_min, deposits of 1 / cost in ant order and none where cost <= 0.

np.cumsum(..., dtype=float32) adds in order with one rounding per term: the sequential sum of the reference's `.sum()` and walk.
"""
import numpy as np

from _ga_oracle import INIT_EVENT, SLOT_SHUFFLE, draw, draw_key, position, uniform
from _sa_oracle import chain_key, dist_fn, tour_length
from _swarm_oracle import cached

DEFAULTS = dict(epochs=150, alpha=1.0, beta=2.0, evaporation_rate=0.5, num_ants=25)  # mod.rs:1091-1112
TAU_MIN_RATIO = np.float32(1e-4)
MIN_DIST = np.float32(1e-6)
SLOT_START, SLOT_R1, SLOT_R2 = 0, 1, 2
EVENT_LIMIT = 1 << 58
F32_MAX = np.float32(3.4028234663852886e38)
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
INV_LN2 = 1.4426950408889634
SQRT_HALF = 0.70710678118654752440
LOG_COEF = [1.0 / (2 * i + 1) for i in range(12)]
EXP_COEF = [1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0,
            1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0]


def event(epoch, num_ants, ant, n, step):
    return (epoch * num_ants + ant) * n + step


def shuffle_event(j):
    return INIT_EVENT + j


def roles(n, num_ants, epochs, seeded):
    """every (event, slot) the run draws, with its role: for the test that no two roles share one"""
    out = []
    if not seeded:
        out += [(shuffle_event(j), SLOT_SHUFFLE, ("shuffle", j)) for j in range(n - 1, 0, -1)]
    for g in range(epochs):
        for a in range(num_ants):
            out.append((event(g, num_ants, a, n, 0), SLOT_START, ("start", g, a)))
            for s in range(1, n):
                out.append((event(g, num_ants, a, n, s), SLOT_R1, ("r1", g, a, s)))
                out.append((event(g, num_ants, a, n, s), SLOT_R2, ("r2", g, a, s)))
    return out


def aco_pow(x, a):
    """aco_spec.h's aco_pow on an array of f32 x >= 0 (or NaN), a finite f32 a >= 0"""
    x = np.asarray(x, dtype=np.float32)
    a = np.float32(a)
    if a == 0:
        return np.ones_like(x)
    if a == 1:
        return x.copy()
    if a == 2:
        with np.errstate(all="ignore"):
            return (x * x).astype(np.float32)
    with np.errstate(all="ignore"):
        special = np.isnan(x) | (x == 0) | np.isinf(x)
        xd = np.where(special, np.float32(1.0), x).astype(np.float64)
        b = xd.view(np.uint64)
        e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64).astype(np.float64) - 1022.0
        m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FE0000000000000)).view(np.float64)
        low = m < SQRT_HALF
        m = np.where(low, m * 2.0, m)
        e = np.where(low, e - 1.0, e)
        s = (m - 1.0) / (m + 1.0)
        s2 = s * s
        p = np.full_like(s, LOG_COEF[11])
        for i in range(10, -1, -1):
            p = p * s2 + LOG_COEF[i]
        lx = e * LN2_HI + ((2.0 * s) * p + e * LN2_LO)
        y = float(a) * lx
        yc = np.clip(y, -200.0, 200.0)
        k = np.rint(yc * INV_LN2)
        r = (yc - k * LN2_HI) - k * LN2_LO
        q = np.full_like(r, EXP_COEF[13])
        for i in range(12, -1, -1):
            q = q * r + EXP_COEF[i]
        out = np.ldexp(q, k.astype(np.int64)).astype(np.float32)
        out = np.where(y > 89.0, np.float32(np.inf), out)
        out = np.where(y < -104.0, np.float32(0.0), out)
        return np.where(special, x, out).astype(np.float32)


def pow_scalar(x, a):
    return aco_pow(np.array([x], dtype=np.float32), a)[0]


def usable(total):
    return bool(total > 0 and total <= F32_MAX)


def roulette_select(weights, total, r):
    """probability.rs:69-79 on a candidate list: the index in the list"""
    with np.errstate(all="ignore"):
        target = np.float32(r) * np.float32(total)
        acc = np.cumsum(np.asarray(weights, dtype=np.float32), dtype=np.float32)
    hit = np.flatnonzero(acc > target)
    return int(hit[0]) if len(hit) else len(weights) - 1


def select_next(primary, fallback, r1, r2):
    """ant_colony.rs:65-78 on the candidates' weights: (index in the list, path, primary total, eta total or 0)"""
    primary, fallback = np.asarray(primary, dtype=np.float32), np.asarray(fallback, dtype=np.float32)
    with np.errstate(all="ignore"):
        t1 = np.cumsum(primary, dtype=np.float32)[-1]
        if usable(t1):
            return roulette_select(primary, t1, r1), 0, t1, np.float32(0.0)
        t2 = np.cumsum(fallback, dtype=np.float32)[-1]
    if usable(t2):
        return roulette_select(fallback, t2, r2), 1, t1, t2
    return 0, 2, t1, t2


def select_compacted(weights, eta, visited, r1, r2):
    """the reference's form: the candidate lists are the unvisited cities in city order.  (city, path, total, eta total)"""
    cand = np.flatnonzero(~np.asarray(visited, dtype=bool))
    i, path, t1, t2 = select_next(np.asarray(weights, dtype=np.float32)[cand], np.asarray(eta, dtype=np.float32)[cand], r1, r2)
    return int(cand[i]), path, t1, t2


def select_masked(weights, eta, visited, r1, r2):
    """the device's form (aco_spec.h): a walk over all n cities, a visited city's weight forced to +0.0f; the exhausted walk
    falls back to the last UNVISITED city, the degenerate case to the first"""
    visited = np.asarray(visited, dtype=bool)
    cand = np.flatnonzero(~visited)

    def walk(row, r):
        with np.errstate(all="ignore"):
            acc = np.cumsum(np.where(visited, np.float32(0.0), np.asarray(row, dtype=np.float32)), dtype=np.float32)
            total = acc[-1]
            if not usable(total):
                return None, total
            hit = np.flatnonzero(acc > np.float32(r) * total)
        return (int(hit[0]) if len(hit) else int(cand[-1])), total

    c, t1 = walk(weights, r1)
    if c is not None:
        return c, 0, t1, np.float32(0.0)
    c, t2 = walk(eta, r2)
    if c is not None:
        return c, 1, t1, t2
    return int(cand[0]), 2, t1, t2


def evaporate_and_floor(tau, rate, tau_min):
    """ant_colony.rs:25-32, in place"""
    tau *= np.float32(1.0) - np.float32(rate)
    np.maximum(tau, np.float32(tau_min), out=tau)


def deposit_tour(tau, tour, cost):
    """ant_colony.rs:43-53 on the n x n array, in place: each cell of a tour's edges once (no edge repeats within a tour of n >= 3,
    so the fancy-indexed add is the loop)"""
    cost = np.float32(cost)
    if len(tour) < 2 or cost <= 0:
        return
    amount = np.float32(1.0) / cost
    t = np.asarray(tour, dtype=np.int64)
    u, v = np.concatenate(([t[-1]], t[:-1])), np.concatenate(([t[0]], t[1:]))
    if len(t) == 2:  # the one edge twice: the closing edge, then the window
        for a, b in zip(u, v):
            tau[a, b] += amount
            tau[b, a] += amount
        return
    tau[u, v] += amount
    tau[v, u] += amount


def start_tour(key, n):
    r = list(range(n))
    for j in range(n - 1, 0, -1):
        k = position(draw_key(key, shuffle_event(j), SLOT_SHUFFLE), j + 1)
        r[j], r[k] = r[k], r[j]
    return np.asarray(r, dtype=np.int64)


def solve(xy, packed, n, init=None, *, epochs=150, alpha=1.0, beta=2.0, evaporation_rate=0.5, num_ants=25, seed=1, run=0, keep=False):
    """One run.  Returns a dict: tour, cost; epochs = [dict(costs, starts, fallbacks, improving)] (per ant; improving: the ants whose
    cost went below the best, in order); routes = [(epoch, ant, cost, tour)], the start tour first with epoch = ant = -1; counters
    (improved, fallbacks, tours).  keep: also paths[epoch][ant] = [(path, primary total, eta total)] per selection."""
    d = dist_fn(xy, packed, n)
    if n <= 2:
        t = np.arange(n, dtype=np.uint32)
        return dict(tour=t, cost=np.float32(tour_length(d, t.astype(np.int64))), epochs=[], routes=[], counters=dict(improved=0, fallbacks=0, tours=0), paths=[])
    if epochs * num_ants * n > EVENT_LIMIT:
        raise ValueError("unsupported: epochs x num_ants x n exceeds 2^58 draw events")
    alpha, beta, rate = np.float32(alpha), np.float32(beta), np.float32(evaporation_rate)
    key = chain_key(seed, run)
    best = np.asarray(init, dtype=np.int64).copy() if init is not None else start_tour(key, n)
    best_cost = np.float32(tour_length(d, best))
    routes = [(-1, -1, best_cost, best.astype(np.uint32))]
    with np.errstate(all="ignore"):
        tau0 = np.float32(num_ants) / best_cost if init is not None and best_cost > 0 else np.float32(1.0)
        tau_min = np.float32(tau0 * TAU_MIN_RATIO)
        tau = np.full((n, n), tau0, dtype=np.float32)
        idx = np.arange(n)
        dm = d(idx[:, None], idx[None, :]).astype(np.float32)
        eta = aco_pow(np.float32(1.0) / np.maximum(dm, MIN_DIST), beta)
        eta[idx, idx] = 0
        if init is not None:
            deposit_tour(tau, best, best_cost)
        log, paths, cnt = [], [], dict(improved=0, fallbacks=0, tours=0)
        for g in range(epochs):
            w = (aco_pow(tau, alpha) * eta).astype(np.float32)
            ants, rec = [], dict(costs=[], starts=[], fallbacks=[], improving=[])
            epaths = []
            for a in range(num_ants):
                cur = position(draw_key(key, event(g, num_ants, a, n, 0), SLOT_START), n)
                visited = np.zeros(n, dtype=bool)
                visited[cur] = True
                tour, fb, apaths = [cur], 0, []
                rec["starts"].append(cur)
                for s in range(1, n):
                    ev = event(g, num_ants, a, n, s)
                    r1, r2 = uniform(draw_key(key, ev, SLOT_R1)), uniform(draw_key(key, ev, SLOT_R2))
                    cand = np.flatnonzero(~visited)
                    i, path, t1, t2 = select_next(w[cur, cand], eta[cur, cand], r1, r2)
                    nxt = int(cand[i])
                    fb += path != 0
                    if keep:
                        apaths.append((path, t1, t2))
                    visited[nxt] = True
                    tour.append(nxt)
                    cur = nxt
                tour = np.asarray(tour, dtype=np.int64)
                cost = np.float32(tour_length(d, tour))
                if cost < best_cost:
                    best, best_cost = tour.copy(), cost
                    rec["improving"].append(a)
                    routes.append((g, a, cost, tour.astype(np.uint32)))
                    cnt["improved"] += 1
                ants.append((tour, cost))
                rec["costs"].append(cost)
                rec["fallbacks"].append(fb)
                cnt["fallbacks"] += fb
                cnt["tours"] += 1
                epaths.append(apaths)
            evaporate_and_floor(tau, rate, tau_min)
            for tour, cost in ants:
                deposit_tour(tau, tour, cost)
            log.append(rec)
            paths.append(epaths)
    return dict(tour=best.astype(np.uint32), cost=np.float32(tour_length(d, best)), epochs=log, routes=routes, counters=cnt, paths=paths if keep else [])


def log_words(res, num_ants):
    """the trace as the library writes it: 3 num_ants u32 per epoch"""
    rows = [np.concatenate((np.asarray(e["costs"], dtype=np.float32).view(np.uint32), np.asarray(e["starts"], dtype=np.uint32),
                            np.asarray(e["fallbacks"], dtype=np.uint32))) for e in res["epochs"]]
    return np.array(rows, dtype=np.uint32).reshape(len(rows), 3 * num_ants)


def route_words(res, n):
    """the route log as the library writes it: n + 3 u32 per row"""
    rows = [np.concatenate((np.array([g & 0xFFFFFFFF, a & 0xFFFFFFFF], dtype=np.uint32), np.array([c], dtype=np.float32).view(np.uint32), t))
            for g, a, c, t in res["routes"]]
    return np.array(rows, dtype=np.uint32).reshape(len(rows), n + 3)


def messages(res, ids=None):
    """the reference's progress messages (ant_colony.rs:141-147,225-231,241-248)"""
    name = (lambda t: [int(v) for v in t]) if ids is None else (lambda t: [int(v) for v in ids[t]])
    out = []
    if not res["routes"]:
        return [("Done", None)]
    out.append(("PathUpdate", (name(res["routes"][0][3]), float(res["routes"][0][2]))))
    for g in range(len(res["epochs"])):
        out += [("PathUpdate", (name(t), float(c))) for e, _a, c, t in res["routes"] if e == g]
        out.append(("EpochUpdate", g))
    return out + [("Done", None)]


solve_cached = cached(solve)

