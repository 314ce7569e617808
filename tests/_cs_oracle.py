"""The specification of the project's cuckoo search solver, in numpy and literal loops (TEST infrastructure, not product code).

cuckoo_search.rs:26-136 with two deliberate differences, because the reference's unseeded thread RNG cannot be reproduced and libm's
log, cos and pow are the platform's: the random draws are a pure function of (seed, run, event, slot) — the stream of
tests/_ga_oracle.py, laid out as teeline_amd/csrc/cs_spec.h says — and the Lévy step is a fixed sequence of IEEE f64 operations
(teeline_amd/csrc/levy_spec.h).  Everything else is the reference's, quirks included: N = max(n_nearest, 25) nests;
pa = clamp(mutation_probability, 0.01, 0.99); nest 0 is the initial tour where one is given; best is a COPY of the FIRST minimum
nest; a flight starts from its nest AS IT STANDS (an earlier flight of the epoch may have overwritten it); the target is drawn after
the flight, c = t allowed; the test is strict; an abandonment replaces unconditionally.  Python floats are IEEE f64 and neither
Python nor numpy fuses a multiply with an add.
"""
import math

import numpy as np

from _ga_oracle import SLOT_SHUFFLE, draw, draw_key, init_event, position  # noqa: F401  (draw: re-exported)
from _sa_oracle import chain_key, dist_fn, tour_length
from _swarm_oracle import NONE, bits, cached, log_words, messages, route_words, uniform  # noqa: F401

SLOT_LEVY, SLOT_TARGET, SLOT_ABANDON = 0, 12, 13
SLOT_REV_I, SLOT_REV_J, SLOT_REPLACE = 0, 1, 2
RESAMPLES = 4
WORDS = 4 + 2 * RESAMPLES
DEFAULT_NESTS = 25
MAX_NESTS = 4096
EVENT_LIMIT = 1 << 58
DEFAULTS = dict(epochs=10_000, n_nearest=3, mutation_probability=0.001)  # mod.rs:604-611, 918-925
MIN_POSITIVE = 2.2250738585072014e-308
SIGMA_U = 0.6966
LN2_HI, LN2_LO, LOG2E, HALF_PI = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.4426950408889634, 1.5707963267948966
LOG_C = [1.0 / (2 * i + 1) for i in range(12)]
EXP_C = [1.0 / float(math.factorial(i)) for i in range(14)]
SIN_C = [(-1.0 if i % 2 else 1.0) / float(math.factorial(2 * i + 1)) for i in range(10)]
COS_C = [(-1.0 if i % 2 else 1.0) / float(math.factorial(2 * i)) for i in range(11)]


def nests(n_nearest):
    return max(int(n_nearest), DEFAULT_NESTS)


def pa_of(mutation_probability):
    p = float(np.float32(mutation_probability))
    return 0.01 if p < 0.01 else 0.99 if p > 0.99 else p


def base(epoch, N, c, n):
    return (epoch * N + c) * (n + 1)


def events_fit(epochs, N, n):
    return epochs * N * (n + 1) <= EVENT_LIMIT


# ---------------------------------------------------------------- the Lévy step, on arrays (one statement for one draw and for 10^6)
def _horner(c, x):
    p = np.full_like(x, c[-1])
    for k in range(len(c) - 2, -1, -1):
        p = p * x + c[k]
    return p


def log_spec(x):
    """log of positive normal f64s"""
    x = np.asarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64).astype(np.float64) - 1022.0
    m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FE0000000000000)).view(np.float64)
    small = m < 0.70710678118654752440
    m = np.where(small, m * 2.0, m)
    e = np.where(small, e - 1.0, e)
    s = (m - 1.0) / (m + 1.0)
    p = _horner(LOG_C, s * s)
    return e * LN2_HI + ((2.0 * s) * p + e * LN2_LO)


def exp_spec(y):
    y = np.asarray(y, dtype=np.float64)
    k = np.rint(y * LOG2E)
    r = (y - k * LN2_HI) - k * LN2_LO
    return np.ldexp(_horner(EXP_C, r), k.astype(np.int64))


def cos2pi_spec(u):
    """cos(2 pi u) for dyadic u in [0, 1): the quadrant reduction is exact"""
    u = np.asarray(u, dtype=np.float64)
    t = u * 4.0
    qf = np.floor(t)
    f = t - qf
    low = f <= 0.5
    g = np.where(low, f, 1.0 - f)
    x = g * HALF_PI
    x2 = x * x
    S = x * _horner(SIN_C, x2)
    Cc = _horner(COS_C, x2)
    c, s = np.where(low, Cc, S), np.where(low, S, Cc)
    q = qf.astype(np.int64)
    return np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))


def uniform_np(w):
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def normal_spec(w1, w2):
    u1 = np.maximum(uniform_np(w1), MIN_POSITIVE)
    return np.sqrt(-2.0 * log_spec(u1)) * cos2pi_spec(uniform_np(w2))


def levy_spec(words):
    """words: [m, WORDS] u64.  Returns (the signed steps, the resamples v took)"""
    words = np.asarray(words, dtype=np.uint64).reshape(-1, WORDS)
    with np.errstate(all="ignore"):
        u = normal_spec(words[:, 0], words[:, 1]) * SIGMA_U
        v = normal_spec(words[:, 2], words[:, 3])
        tries = np.zeros(len(words), dtype=np.uint32)
        for t in range(RESAMPLES):
            again = np.abs(v) < MIN_POSITIVE
            v = np.where(again, normal_spec(words[:, 4 + 2 * t], words[:, 5 + 2 * t]), v)
            tries += again
        v = np.where(np.abs(v) < MIN_POSITIVE, 1.0, v)
        return u / exp_spec((1.0 / 1.5) * log_spec(np.abs(v))), tries


def levy_libm(words):
    """the reference's formula (probability.rs:8-22) by numpy's libm, on the same words; rows whose first v is zero are resampled as
    the specification does"""
    words = np.asarray(words, dtype=np.uint64).reshape(-1, WORDS)

    def normal(w1, w2):
        return np.sqrt(-2.0 * np.log(np.maximum(uniform_np(w1), MIN_POSITIVE))) * np.cos(2.0 * np.pi * uniform_np(w2))
    with np.errstate(all="ignore"):
        u = normal(words[:, 0], words[:, 1]) * SIGMA_U
        v = normal(words[:, 2], words[:, 3])
        return u / np.power(np.abs(v), 1.0 / 1.5)


def levy_from_words(words):
    """one step: (the signed f64, the resamples)"""
    v, t = levy_spec(np.asarray(words, dtype=np.uint64).reshape(1, WORDS))
    return float(v[0]), int(t[0])


def flight_length(levy, n):
    """(ceil(levy (n 0.1)) as usize).clamp(1, n / 2), Rust's `as`: NaN and negatives give 0, +inf saturates"""
    x = levy * (n * 0.1)
    if x != x or not x > 0.0:
        return 1
    if x == math.inf:
        return n // 2
    return min(max(int(math.ceil(x)), 1), n // 2)


def flight_length_np(levy, n):
    with np.errstate(all="ignore"):
        x = np.ceil(np.asarray(levy, dtype=np.float64) * (n * 0.1))
    x = np.where(x > 1.0, np.minimum(x, float(n // 2)), 1.0)
    return x.astype(np.int64)


def word_of_uniform(m):
    """the word whose uniform is m 2^-53"""
    return int(m) << 11


# ---------------------------------------------------------------- reversals
def reverse_literal(tour, pairs):
    """apply_k_random_2opt's loop (cuckoo_search.rs:18-22) on given pairs"""
    r = list(tour)
    for i, j in pairs:
        r[i:j + 1] = r[i:j + 1][::-1]
    return r


def source_position(pairs, p):
    q = p
    for i, j in reversed(pairs):
        if i <= q <= j:
            q = i + j - q
    return q


def reverse_gather(tour, pairs):
    """the form the device computes: every output position followed back through the reversals, last to first"""
    return [tour[source_position(pairs, p)] for p in range(len(tour))]


def reverse_gather_np(tour, pairs):
    tour = np.asarray(tour)
    q = np.arange(len(tour))
    for i, j in reversed(pairs):
        q = np.where((i <= q) & (q <= j), i + j - q, q)
    return tour[q]


# ---------------------------------------------------------------- the run
def roles(n, N, epochs, seeded):
    """every (event, slot) a run may draw, with its role: for the test that no two roles share one"""
    out = []
    for i in range(N):
        if seeded and i == 0:
            continue
        out += [(init_event(n, i, j), SLOT_SHUFFLE, ("shuffle", i, j)) for j in range(n - 1, 0, -1)]
    for e in range(epochs):
        for c in range(N):
            B = base(e, N, c, n)
            out += [(B, SLOT_LEVY + s, ("levy", e, c, s)) for s in range(WORDS)]
            out += [(B, SLOT_TARGET, ("target", e, c)), (B, SLOT_ABANDON, ("abandon", e, c))]
            for r in range(n // 2):
                out += [(B + 1 + r, SLOT_REV_I, ("i", e, c, r)), (B + 1 + r, SLOT_REV_J, ("j", e, c, r))]
            out += [(B + 1 + j, SLOT_REPLACE, ("replace", e, c, j)) for j in range(n - 1, 0, -1)]
    return out


def shuffled(key, n, event0, slot):
    r = list(range(n))
    for j in range(n - 1, 0, -1):
        k = position(draw_key(key, event0 + j, slot), j + 1)
        r[j], r[k] = r[k], r[j]
    return r


def flight_draws(key, B, n):
    """k and the k pairs of the flight whose events begin at B"""
    levy, _ = levy_from_words([draw_key(key, B, SLOT_LEVY + s) for s in range(WORDS)])
    k = flight_length(abs(levy), n)
    pairs = []
    for r in range(k):
        i = position(draw_key(key, B + 1 + r, SLOT_REV_I), n - 1)
        pairs.append((i, i + 1 + position(draw_key(key, B + 1 + r, SLOT_REV_J), n - 1 - i)))
    return k, pairs


def solve(xy, packed, n, init=None, *, epochs, n_nearest=3, mutation_probability=0.001, seed=1, run=0, mutate=None):
    """One run.  Returns a dict: tour, cost, improvements [(epoch or NONE, source, cost, route)] — the start best first; source is
    the cuckoo of a flight, N + the nest of an abandonment —, epochs [dict(costs, ks, targets, accepted, again, abandoned, pairs,
    best_nest, orphaned)], counters, nests.  `again` is a fact of the sequential algorithm: cuckoo c's nest had been overwritten by an earlier
    flight of the epoch.  best_nest: (per epoch, after it) whether some nest still holds best's tour.
    mutate: a deliberately WRONG variant, for the tests that show the cases tell it apart: "epoch_start" (every flight starts from
    the epoch-start nest), "best_is_min" (best taken as the minimum over the nests after every change), "le" (the target test <=)."""
    N = nests(n_nearest)
    if n <= 1:
        if epochs >= 1:
            raise ValueError("the reference panics: clamp(1, n / 2) with min > max")
        zero = np.float32(0.0)
        return dict(tour=np.arange(n, dtype=np.uint32), cost=zero, improvements=[(NONE, 0, zero, list(range(n)))], epochs=[], counters=dict(flights=0, improved=0),
                    nests=N)
    assert events_fit(epochs, N, n)
    d = dist_fn(xy, packed, n)
    key = chain_key(seed, run)
    pa = pa_of(mutation_probability)
    length = lambda r: tour_length(d, np.asarray(r, dtype=np.int64))  # noqa: E731
    nest = [[int(v) for v in init] if (i == 0 and init is not None) else shuffled(key, n, init_event(n, i, 0), SLOT_SHUFFLE) for i in range(N)]
    costs = [length(t) for t in nest]
    b = 0
    for i in range(1, N):
        if costs[i] < costs[b]:  # min_by keeps the first of equals
            b = i
    best, best_cost = list(nest[b]), costs[b]
    improvements = [(NONE, b, best_cost, list(best))]
    eps = []
    for e in range(epochs):
        start = [list(t) for t in nest]  # (mutate == "epoch_start" only)
        touched = [False] * N
        ks, targets, accepted, again, all_pairs = [], [], [], [], []
        for c in range(N):
            B = base(e, N, c, n)
            k, pairs = flight_draws(key, B, n)
            new = reverse_literal(start[c] if mutate == "epoch_start" else nest[c], pairs)
            new_cost = length(new)
            t = position(draw_key(key, B, SLOT_TARGET), N)
            ok = new_cost <= costs[t] if mutate == "le" else new_cost < costs[t]
            ks.append(k)
            targets.append(t)
            accepted.append(bool(ok))
            again.append(touched[c])
            all_pairs.append(pairs)
            if ok:
                nest[t], costs[t] = new, new_cost
                touched[t] = True
                if new_cost < best_cost:
                    best, best_cost = list(new), new_cost
                    improvements.append((e, c, new_cost, list(best)))
                elif mutate == "best_is_min" and min(costs) != best_cost:
                    m = int(np.argmin(costs))
                    best, best_cost = list(nest[m]), costs[m]
        abandoned, orphaned = [], False
        for c in range(N):
            B = base(e, N, c, n)
            ab = uniform(draw_key(key, B, SLOT_ABANDON)) < pa
            abandoned.append(bool(ab))
            if ab:
                t = shuffled(key, n, B + 1, SLOT_REPLACE)
                cost = length(t)
                orphaned = orphaned or (nest[c] == best and cost > best_cost)  # best's own nest is lost to a worse tour; best stands
                nest[c], costs[c] = t, cost
                if cost < best_cost:
                    best, best_cost = list(t), cost
                    improvements.append((e, N + c, cost, list(best)))
                elif mutate == "best_is_min" and min(costs) != best_cost:
                    m = int(np.argmin(costs))
                    best, best_cost = list(nest[m]), costs[m]
        eps.append(dict(costs=list(costs), ks=ks, targets=targets, accepted=accepted, again=again, abandoned=abandoned, pairs=all_pairs,
                        best_nest=any(t == best for t in nest), orphaned=orphaned))
    return dict(tour=np.asarray(best, dtype=np.uint32), cost=np.float32(length(best)), improvements=improvements, epochs=eps,
                counters=dict(flights=epochs * N, improved=len(improvements) - 1), nests=N)


def f64_bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def epoch_words(res):
    """the per-epoch record: nest cost bits | k | target, bit 31 accepted, bit 30 source overwritten earlier | abandoned"""
    N = res["nests"]
    rows = [[bits(c) for c in ep["costs"]] + list(ep["ks"]) + [t | (a << 31) | (g << 30) for t, a, g in zip(ep["targets"], ep["accepted"], ep["again"])] +
            [int(a) for a in ep["abandoned"]] for ep in res["epochs"]]
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 4 * N)


solve_cached = cached(solve)
