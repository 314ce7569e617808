"""The specification of the project's genetic algorithm, in numpy and literal loops (TEST infrastructure, not product code).

genetic_algorithm.rs:16-336 with one deliberate difference, because the reference's unseeded thread RNG cannot be reproduced: the
random draws are a pure function of (seed, run, event, slot) — the stream of tests/_sa_oracle.py indexed by a 64-bit event
(teeline_amd/csrc/ga_spec.h).  Everything else is the reference's, quirks included: the population has n individuals only in
generation 0 (afterwards min(e, len) + 2 max(0, n // 2 - e)); roulette selection walks the SORTED population with a sequential f32
running sum and falls back to the last individual; the ordered crossover gives child 1 parent 2's segment; a mutation reverses
from..=to and does NOT recompute the fitness; best() is the last of equal maxima; the returned cost is tour_length recomputed.
"""
import numpy as np

from _sa_oracle import G, chain_key, dist_fn, mix, pair_from_key, tour_length
from _swarm_oracle import cached, read_only

INIT_EVENT = 1 << 58
SLOT_SELECT, SLOT_MUTATE, SLOT_SHUFFLE, SLOT_COUNT = 22, 24, 26, 27
DEFAULTS = dict(epochs=10_000, mutation_probability=0.001, n_elite=3)  # mod.rs:822-828
U24 = np.float32(2.0 ** -24)


def pair_event(generation, n, pair, part):
    return 4 * (generation * n + pair) + part


def init_event(n, individual, j):
    return INIT_EVENT + individual * n + j


def draw_key(key, event, slot):
    return mix(key + G * (32 * event + slot + 1))


def draw(seed, run, event, slot):
    return draw_key(chain_key(seed, run), event, slot)


def uniform(u):
    return np.float32(u >> 40) * U24


def position(u, n):
    return ((u >> 32) * n) >> 32


def roles(n, n_elite, generations, seeded):
    """every (event, slot) the run draws, with its role: for the test that no two roles share one"""
    out = []
    n_seeded = max(n // 5, 1) if seeded else 0
    for i in range(n):
        if seeded and i == 0:
            continue
        if i < n_seeded:
            out.append((init_event(n, i, 0), SLOT_COUNT, ("count", i)))
            out += [(init_event(n, i, 1 + m), s, ("init_mutation", i, m)) for m in range(4) for s in range(22)]
        else:
            out += [(init_event(n, i, j), SLOT_SHUFFLE, ("shuffle", i, j)) for j in range(n - 1, 0, -1)]
    for g in range(generations):
        for p in range(max(0, n // 2 - n_elite)):
            out += [(pair_event(g, n, p, 0), s, ("crossover", g, p)) for s in range(22)]
            out += [(pair_event(g, n, p, 0), SLOT_SELECT + k, ("select", g, p, k)) for k in range(2)]
            out += [(pair_event(g, n, p, 0), SLOT_MUTATE + k, ("trial", g, p, k)) for k in range(2)]
            out += [(pair_event(g, n, p, 1 + k), s, ("mutation", g, p, k)) for k in range(2) for s in range(22)]
    return out


def fitness_of(length):
    length = np.float32(length)
    return np.float32(0.0) if length == 0 else np.float32(1.0) / length


def reverse(route, lo, hi):
    """mutate (genetic_algorithm.rs:327-335)"""
    while lo < hi:
        route[lo], route[hi] = route[hi], route[lo]
        lo += 1
        hi -= 1


def crossover(p1, p2, lo, hi):
    """ordered_crossover_genes (genetic_algorithm.rs:140-177)"""
    n = len(p1)
    g1, g2 = [0] * n, [0] * n
    range_a, range_b = set(p1[lo:hi + 1]), set(p2[lo:hi + 1])
    g1[lo:hi + 1] = p2[lo:hi + 1]
    g2[lo:hi + 1] = p1[lo:hi + 1]
    k = (hi + 1) % n
    j1 = j2 = k
    for _ in range(n):
        if p1[k] not in range_b:
            g1[j1] = p1[k]
            j1 = (j1 + 1) % n
        if p2[k] not in range_a:
            g2[j2] = p2[k]
            j2 = (j2 + 1) % n
        k = (k + 1) % n
    return g1, g2


def prefix_of(fits):
    """prefix[0] = 0, prefix[i + 1] = prefix[i] + f_i, sequential f32"""
    p = np.zeros(len(fits) + 1, dtype=np.float32)
    for i, f in enumerate(fits):
        p[i + 1] = np.float32(p[i] + np.float32(f))
    return p


def select_linear(fits, r):
    """random_selection (genetic_algorithm.rs:273-290) with r given"""
    up_to = np.float32(0.0)
    for i, f in enumerate(fits):
        if r < np.float32(up_to + f):
            return i
        up_to = np.float32(up_to + f)
    return len(fits) - 1


def select_search(prefix, r):
    """the same by binary search over the prefix (ga_spec.h: ga_select)"""
    n = len(prefix) - 1
    lo, hi = 0, n
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if r < prefix[mid + 1]:
            hi = mid
        else:
            lo = mid + 1
    return lo if lo < n else n - 1


def start_population(d, key, n, init):
    """from_cities / from_cities_seeded (genetic_algorithm.rs:193-237): [(fitness, route)]"""
    pop = []
    n_seeded = 0
    if init is not None:
        n_seeded = max(n // 5, 1)
        seed_route = [int(v) for v in init]
        pop.append((fitness_of(tour_length(d, np.asarray(seed_route, dtype=np.int64))), seed_route))
        for i in range(1, n_seeded):
            r = list(seed_route)
            for m in range(2 + position(draw_key(key, init_event(n, i, 0), SLOT_COUNT), 3)):
                lo, hi = pair_from_key(key, init_event(n, i, 1 + m), n)
                reverse(r, lo, hi)
            pop.append((fitness_of(tour_length(d, np.asarray(r, dtype=np.int64))), r))
    for i in range(n_seeded, n):
        r = list(range(n))
        for j in range(n - 1, 0, -1):
            k = position(draw_key(key, init_event(n, i, j), SLOT_SHUFFLE), j + 1)
            r[j], r[k] = r[k], r[j]
        pop.append((fitness_of(tour_length(d, np.asarray(r, dtype=np.int64))), r))
    return pop


def best_of(pop):
    """best() (genetic_algorithm.rs:257-262): max_by keeps the last of equal maxima"""
    b = 0
    for i in range(1, len(pop)):
        if pop[i][0] >= pop[b][0]:
            b = i
    return b


def solve(xy, packed, n, init=None, *, epochs, mutation_probability=0.001, n_elite=3, seed=1, run=0, keep=False):
    """One run.  Returns (tour, cost, trace, counters[, populations]): trace = [(best index, fitness, tour_length of the best route,
    population length)] per generation; counters = children, mutations, improved (generations whose best fitness exceeds the
    population's before).  keep: also every population [(fitness, route)], the start population first."""
    if n == 0:
        raise ValueError("reference panics: best() of an empty population")
    d = dist_fn(xy, packed, n)
    key = chain_key(seed, run)
    p_mut = np.float32(mutation_probability)
    pop = start_population(d, key, n, init)
    pops = [list(pop)]
    trace, cnt = [], dict(children=0, mutations=0, improved=0)
    length = lambda r: tour_length(d, np.asarray(r, dtype=np.int64))  # noqa: E731
    with np.errstate(all="ignore"):
        for g in range(epochs):
            order = sorted(range(len(pop)), key=lambda i: -pop[i][0])  # stable, descending (fitness >= 0, never NaN here)
            cur = [pop[i] for i in order]
            new = [(f, list(r)) for f, r in cur[:n_elite]]
            fits = [f for f, _ in cur]
            prefix = prefix_of(fits)
            for p in range(max(0, n // 2 - n_elite)):
                total = prefix[-1]
                if not (total > 0 and np.isfinite(total)):
                    raise ValueError("reference panics: empty range in random_selection")
                ev = pair_event(g, n, p, 0)
                parents = []
                for k in range(2):
                    r = np.float32(uniform(draw_key(key, ev, SLOT_SELECT + k)) * total)
                    parents.append(cur[select_linear(fits, r)][1])
                lo, hi = pair_from_key(key, ev, n)
                for k, gene in enumerate(crossover(parents[0], parents[1], lo, hi)):
                    f = fitness_of(length(gene))
                    if p_mut > uniform(draw_key(key, ev, SLOT_MUTATE + k)):
                        mlo, mhi = pair_from_key(key, pair_event(g, n, p, 1 + k), n)
                        reverse(gene, mlo, mhi)
                        cnt["mutations"] += 1
                    if len(new) < n:
                        new.append((f, gene))
                    cnt["children"] += 1
            if not new:
                raise ValueError("reference panics: best() of an empty population")
            before = pop[best_of(pop)][0]
            pop = new
            b = best_of(pop)
            cnt["improved"] += bool(pop[b][0] > before)
            trace.append((b, pop[b][0], length(pop[b][1]), len(pop)))
            if keep:
                pops.append(list(pop))
    b = best_of(pop)
    out = (np.asarray(pop[b][1], dtype=np.uint32), np.float32(length(pop[b][1])), trace, cnt)
    return out + (pops,) if keep else out


solve_cached = cached(solve, lambda out: (read_only(out[0]), out[1], tuple(out[2]), dict(out[3])) + tuple(out[4:]))
