"""The specification of the project's tabu search, in numpy (TEST infrastructure, not product code).

tabu_search.rs:9-110 and route.rs:48-113 with one deliberate difference, because the reference's unseeded thread RNG cannot be
reproduced: the random draws are a pure function of (seed, chain, event, slot) with event = epoch (n + 1) + attempt — the stream of
tests/_sa_oracle.py indexed by a 64-bit event instead of an epoch.  Everything else is the reference's, quirks included: the list
holds n whole routes, FIFO, and receives the start tour before the first epoch and the OLD current tour after every epoch (so the
start tour is listed twice after epoch 0); an epoch takes the first of candidates 0 .. n-1 that is shorter than the current tour
and equal to no listed route, else candidate n with no check at all; every cost is tour_length (closing edge first, sequential
f32) of the whole candidate; `epochs + 1` epochs run; the best route seen is returned.
"""
from collections import deque

import numpy as np

from _sa_oracle import G, chain_key, dist_fn, mix, pair_from_key, tour_length
from _swarm_oracle import cached, read_only

CHUNK = 64  # candidates costed at once (any value gives the same chain: the first qualifying candidate in order is taken)


def event(epoch, n, attempt):
    return epoch * (n + 1) + attempt


def draw(seed, chain, n, epoch, attempt, slot):
    return mix(chain_key(seed, chain) + G * (32 * event(epoch, n, attempt) + slot + 1))


def pair(seed, chain, n, epoch, attempt):
    """random_position_pair (route.rs:69-83) of candidate `attempt` of `epoch`: _sa_oracle's rule on the event's slots"""
    return pair_from_key(chain_key(seed, chain), event(epoch, n, attempt), n)


def candidate_costs(d, tour, pairs):
    """tour_length of every candidate (tour with positions lo..=hi reversed) at once: a 2-D edge array summed along its rows in order,
    one rounding per term"""
    n = len(tour)
    c = np.tile(tour, (len(pairs), 1))
    for r, (lo, hi) in enumerate(pairs):
        c[r, lo:hi + 1] = tour[lo:hi + 1][::-1]
    e = np.empty((len(pairs), n), dtype=np.float32)
    e[:, 0] = d(c[:, n - 1], c[:, 0])
    e[:, 1:] = d(c[:, :-1], c[:, 1:])
    return c, np.add.accumulate(e, axis=1, dtype=np.float32)[:, -1]


class TabuList:
    """tabu_search.rs:87-110: capacity routes, newest first; a full list drops its oldest"""

    def __init__(self, capacity):
        self.capacity, self.items, self.added = capacity, deque(), 0

    def add(self, route):
        if len(self.items) >= self.capacity:
            self.items.pop()
        self.items.appendleft(np.asarray(route, dtype=np.int64).tobytes())
        self.added += 1

    def contains(self, route):
        return np.asarray(route, dtype=np.int64).tobytes() in self.items

    def ring_indices(self, route):
        """where the listed copies of `route` sit in a ring that writes its k-th route to slot k mod capacity (the device's layout),
        ascending; empty when the route is not listed"""
        b = np.asarray(route, dtype=np.int64).tobytes()
        return sorted((self.added - 1 - i) % self.capacity for i, r in enumerate(self.items) if r == b)


def solve(xy, packed, n, init=None, *, epochs, seed=1, chain=0, record=None):
    """One chain.  Returns (best tour, its cost, log, counters): log = [(taken attempt, from, to, cost)] of every epoch; counters =
    hits (improving candidates the list refused), forced (epochs that took attempt n), bests (new bests), candidates (the sum of
    taken attempt + 1), reversed (elements moved), deepest (the largest taken attempt).  record: a dict that receives what the
    list did — "refusals" = [(epoch, attempt, ring indices of the listed copies that matched)], "list_len" = the list's length at
    every epoch, "checked" = per epoch the improving candidates looked up in the list (refused ones included)."""
    if n < 2:
        raise ValueError("reference panics: n_items must be bigger than 2")
    if epochs == 0:
        raise ValueError("epochs = 0 never ends")
    u = np.arange(n, dtype=np.int64) if init is None else np.asarray(init, dtype=np.int64).copy()
    d = dist_fn(xy, packed, n)
    key = chain_key(seed, chain)
    tabu = TabuList(n)
    best = u.copy()
    tabu.add(best)
    best_distance = tour_length(d, u)
    log, cnt = [], dict(hits=0, forced=0, bests=0, candidates=0, reversed=0, deepest=0)
    refusals, list_len, checked = [], [], []
    with np.errstate(all="ignore"):
        for e in range(epochs + 1):
            local = tour_length(d, u)
            taken = None
            list_len.append(len(tabu.items))
            checked.append(0)
            for a0 in range(0, n, CHUNK):
                pairs = [pair_from_key(key, event(e, n, a), n) for a in range(a0, min(n, a0 + CHUNK))]
                cands, costs = candidate_costs(d, u, pairs)
                for r in np.flatnonzero(costs < local):
                    checked[-1] += 1
                    if tabu.contains(cands[r]):
                        cnt["hits"] += 1
                        refusals.append((e, a0 + int(r), tuple(tabu.ring_indices(cands[r]))))
                        continue
                    taken = (a0 + int(r), pairs[r], cands[r].copy(), costs[r])
                    break
                if taken is not None:
                    break
            if taken is None:  # candidate n, with no check at all
                p = pair_from_key(key, event(e, n, n), n)
                cands, costs = candidate_costs(d, u, [p])
                taken = (n, p, cands[0].copy(), costs[0])
                cnt["forced"] += 1
            a, (lo, hi), cand, cost = taken
            if cost < best_distance:
                best, best_distance = cand.copy(), cost
                cnt["bests"] += 1
            tabu.add(u)
            u = cand
            log.append((a, lo, hi, np.float32(cost)))
            cnt["candidates"] += a + 1
            cnt["reversed"] += hi - lo + 1
            cnt["deepest"] = max(cnt["deepest"], a)
    if record is not None:
        record.update(refusals=refusals, list_len=list_len, checked=checked)
    return best.astype(np.uint32), np.float32(best_distance), log, cnt


def _solve_recorded(*args, **kw):
    """solve()'s result and, last, its `record`"""
    rec = {}
    tour, cost, log, cnt = solve(*args, record=rec, **kw)
    return read_only(tour), cost, tuple(log), dict(cnt), rec


_recorded = cached(_solve_recorded, tuple)
solve_cached = lambda key, *args, **kw: _recorded(key, *args, **kw)[:4]  # noqa: E731


def record_of(key):
    """the list's record (solve's `record`) of a chain that solve_cached has computed under `key`"""
    return _recorded.cache[key][4]
