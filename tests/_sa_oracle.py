"""The specification of the project's simulated annealing, in numpy (TEST infrastructure, not product code).

simulated_annealing.rs:10-83, route.rs:48-113 and probability.rs:25-32 with two deliberate differences, because the reference's
unseeded thread RNG and the platform's `exp` cannot be reproduced: the random draws are a pure function of
(seed, chain, epoch, slot), and the Metropolis criterion is a fixed f64 operation sequence.  Everything else is the reference's,
quirks included: "best_route" is the current state and the last state is returned; the schedule loop is
`while epoch < epochs || temperature > min_temperature`; after 10 redraws the last pair is used even when equal or adjacent;
the reversal is of positions from..=to of the open path; every cost is tour_length (closing edge first, sequential f32) of the
whole candidate tour, never old + delta.
"""
import math

import numpy as np

from _swarm_oracle import cached, read_only

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
F32_EPS = np.float32(1.1920929e-07)
DEFAULTS = dict(epochs=10_000, cooling_rate=1e-4, min_temperature=1e-3, max_temperature=1000.0)  # mod.rs:598-608, 697-705


def mix(z):
    """splitmix64's output function"""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def chain_key(seed, chain):
    return mix(seed + G * (chain + 1))


def draw(seed, chain, epoch, slot):
    return mix(chain_key(seed, chain) + G * (32 * epoch + slot + 1))


def pair_from_key(key, epoch, n):
    """random_position_pair (route.rs:69-83): attempt a = 0..10 uses slots 2a, 2a + 1; the first pair with hi - lo > 1 among
    attempts 0..9, else attempt 10 whatever it is."""
    base = key + G * (32 * epoch + 1)
    lo = hi = 0
    for a in range(11):
        p1 = ((mix(base + G * (2 * a)) >> 32) * n) >> 32
        p2 = ((mix(base + G * (2 * a + 1)) >> 32) * n) >> 32
        lo, hi = (p1, p2) if p1 < p2 else (p2, p1)
        if hi - lo > 1:
            break
    return lo, hi


def pair(seed, chain, epoch, n):
    return pair_from_key(chain_key(seed, chain), epoch, n)


def p_from_key(key, epoch):
    return np.float32(mix(key + G * (32 * epoch + 22 + 1)) >> 40) * np.float32(2.0 ** -24)


LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
INV_LN2 = 1.4426950408889634
COEF = [1.0 / float(math.factorial(i)) for i in range(14)]


def criteria(x):
    """exp(x) for the f32 x = -(new - old) / T as the project evaluates it: f64, no FMA, no library exp.  (Outside the
    specification's range: a NaN x gives NaN, x > 89 gives +inf.)"""
    x = np.float32(x)
    if x != x:
        return np.float32(np.nan)
    if x < np.float32(-87.0):
        return np.float32(0.0)
    if x > np.float32(89.0):
        return np.float32(np.inf)
    xd = float(x)
    k = float(np.rint(xd * INV_LN2))
    r = (xd - k * LN2_HI) - k * LN2_LO
    q = COEF[13]
    for i in range(12, -1, -1):
        q = q * r + COEF[i]
    return np.float32(math.ldexp(q, int(k)))


def metropolis(T, old, new):
    with np.errstate(all="ignore"):
        return criteria(np.float32(-(np.float32(new) - np.float32(old))) / np.float32(T))


def is_acceptable(T, old, new, p):
    """simulated_annealing.rs:69-83 with p given"""
    old, new = np.float32(old), np.float32(new)
    if new < old:
        return True
    with np.errstate(all="ignore"):
        if abs(np.float32(new - old)) < F32_EPS:
            return False
    return bool(np.float32(p) < metropolis(T, old, new))


def validate(epochs, cooling_rate, min_temperature, max_temperature):
    """SAOptions::validate (mod.rs:707-741): the message, or None"""
    c, lo, hi = np.float32(cooling_rate), np.float32(min_temperature), np.float32(max_temperature)
    if c <= 0:
        return "cooling_rate must be > 0"
    if c >= 1:
        return "cooling_rate must be < 1"
    if hi <= 0:
        return "max_temperature must be > 0"
    if lo < 0:
        return "min_temperature must be >= 0"
    if lo >= hi:
        return "min_temperature must be < max_temperature"
    return None


def schedule(epochs=10_000, cooling_rate=1e-4, min_temperature=1e-3, max_temperature=1000.0, limit=1 << 24):
    """The temperatures of the epochs, in order (float32 array): T_{e+1} = T_e - rate * T_e, two roundings."""
    rate, lo, T = np.float32(cooling_rate), np.float32(min_temperature), np.float32(max_temperature)
    out = []
    e = 0
    while e < epochs or T > lo:
        out.append(T)
        T = np.float32(T - np.float32(rate * T))
        e += 1
        assert e <= limit, "schedule too long for the oracle"
    return np.asarray(out, dtype=np.float32)


def dist_fn(xy, packed, n):
    """d(a, b) on position arrays, f32: the packed matrix where given, else KDPoint::distance (kdtree.rs:291-295)"""
    if packed is not None:
        full = np.zeros((n, n), dtype=np.float32)
        il = np.tril_indices(n, -1)
        full[il] = packed
        full = full + full.T
        return lambda a, b: full[a, b]
    xy = np.asarray(xy, dtype=np.float32)

    def d(a, b):
        dx, dy = xy[a, 0] - xy[b, 0], xy[a, 1] - xy[b, 1]
        return np.sqrt((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32), dtype=np.float32)
    return d


def tour_length(d, tour):
    """distance_matrix.rs:235-245: the closing edge first, then the n - 1 edges in order; np.add.accumulate on float32 adds in
    order with one rounding per term"""
    n = len(tour)
    if n < 2:
        return np.float32(0.0)
    e = np.empty(n, dtype=np.float32)
    e[0] = d(tour[n - 1], tour[0])
    e[1:] = d(tour[:-1], tour[1:])
    return np.add.accumulate(e, dtype=np.float32)[-1]


def solve(xy, packed, n, init=None, *, seed=1, chain=0, temps=None, **opts):
    """One chain.  Returns (tour, cost, trace) with trace = [(epoch, from, to, cost)] of the accepted epochs."""
    if temps is None:
        temps = schedule(**dict(DEFAULTS, **opts))
    tour = np.arange(n, dtype=np.int64) if init is None else np.asarray(init, dtype=np.int64).copy()
    if len(temps) and n < 2:
        raise ValueError("reference panics: n_items must be bigger than 2")
    d = dist_fn(xy, packed, n)
    cost = tour_length(d, tour)
    key = chain_key(seed, chain)
    trace = []
    with np.errstate(all="ignore"):
        for e in range(len(temps)):
            lo, hi = pair_from_key(key, e, n)
            cand = tour.copy()
            cand[lo:hi + 1] = tour[lo:hi + 1][::-1]
            new = tour_length(d, cand)
            if new < cost:
                ok = True
            elif abs(np.float32(new - cost)) < F32_EPS:
                ok = False
            else:
                ok = bool(p_from_key(key, e) < criteria(np.float32(-(new - cost)) / temps[e]))
            if ok:
                tour, cost = cand, new
                trace.append((e, lo, hi, np.float32(new)))
    return tour.astype(np.uint32), np.float32(cost), trace


solve_cached = cached(solve, lambda out: (read_only(out[0]), out[1], tuple(out[2])))
