"""The specification of the project's gravitational search solver, in numpy and literal loops (TEST infrastructure, not product code).

gravitational_search.rs:23-145 with three deliberate differences (teeline_amd/csrc/gsa_spec.h).  The reference's
unseeded thread RNG cannot be reproduced: the random draws are a pure function of (seed, run, event, slot) — the stream of
tests/_ga_oracle.py; the pull of agent j on agent i in epoch e owns the event (e N + i) N + j, slot 0.  The reference ranks the
masses with sort_unstable_by, whose order among equal masses is unspecified: here ties go in ascending agent index.  exp is the
fixed f64 sequence of tests/_cs_oracle.py (exp_spec), not libm's.  Everything else is the reference's, quirks included: N =
max(n_nearest, 25) agents; agent 0 is the initial tour where one is given; gbest is a COPY of the FIRST minimum agent; the masses and
the ranking of an epoch come from the costs at its start; INERTIA_W is 0; a pull takes the first round((r g) mass_j) pairs of
swap_sequence(positions[i], positions[j]) with positions[j] AS IT STANDS; the concatenation is cut to v_max; gbest is updated at
once.  Python floats are IEEE f64 and Python never fuses a multiply with an add.
"""
import numpy as np

from _cs_oracle import exp_spec
from _ga_oracle import SLOT_SHUFFLE, draw, draw_key, init_event, position  # noqa: F401  (draw: re-exported)
from _pso_oracle import keep, vmax
from _sa_oracle import chain_key, dist_fn, tour_length
from _swarm_oracle import (NONE, apply_swaps, bits, cached, log_words, messages, route_words, shuffled, swap_sequence_inverse,  # noqa: F401
                           swap_sequence_literal, uniform)

SLOT_R = 0
DEFAULT_AGENTS = 25
MAX_AGENTS = 4096
MAX_PULL = 20
G0, ALPHA, INERTIA_W = 20.0, 1.0, 0.0
EPSILON = 2.220446049250313e-16
DEFAULTS = dict(epochs=10_000, n_nearest=3)  # mod.rs:604-611


class RefPanics(Exception):
    """where the reference panics: partial_cmp(..).unwrap() of a NaN"""


def agents(n_nearest):
    return max(int(n_nearest), DEFAULT_AGENTS)


def kbest_count(N):
    return (N + 1) // 2


def event(epoch, N, i, j):
    return (epoch * N + i) * N + j


def g_of(epoch, epochs):
    """gravitational_search.rs:101 with the fixed exp"""
    return G0 * float(exp_spec(np.float64(-((ALPHA * float(epoch)) / float(max(epochs, 1))))))


def pull_swaps(r, g, mass):
    """gravitational_search.rs:114: (r g) mass left to right, f64::round spelled out"""
    return keep((r * g) * mass)


def masses_of(costs):
    """(masses, the agents by rank) of f32 costs (gravitational_search.rs:79-97); RefPanics where a mass is NaN"""
    c = [np.float32(v) for v in costs]
    N = len(c)
    worst = np.float32(-np.inf)
    for v in c:
        if v > worst:  # f32::max ignores a NaN
            worst = v
    s = 0.0
    with np.errstate(invalid="ignore"):
        for v in c:
            s += float(np.float32(worst - v))
        if s < EPSILON:
            m = [1.0 / float(N)] * N
        else:
            m = [float(np.float64(np.float32(worst - v)) / np.float64(s)) for v in c]
    if any(x != x for x in m):
        raise RefPanics("a mass is NaN")
    rank = sorted(range(N), key=lambda a: (-m[a], a))  # descending mass, ties in ascending agent index
    return m, rank, s < EPSILON


def roles(n, N, epochs, seeded):
    """every (event, slot) a run may draw, with its role: for the test that no two roles share one"""
    out = []
    for i in range(N):
        if seeded and i == 0:
            continue
        out += [(init_event(n, i, j), SLOT_SHUFFLE, ("shuffle", i, j)) for j in range(n - 1, 0, -1)]
    for e in range(epochs):
        for i in range(N):
            out += [(event(e, N, i, j), SLOT_R, ("r", e, i, j)) for j in range(N)]
    return out


def pull(src, dst, m, seq=swap_sequence_literal):
    """the first m pairs of swap_sequence(src, dst)"""
    return seq(src, dst)[:m]


def solve(xy, packed, n, init=None, *, epochs, n_nearest=3, seed=1, run=0, seq=swap_sequence_literal, mutate=None):
    """One run.  Returns a dict: tour, cost, improvements [(epoch or NONE, agent, cost, route)] — the start gbest first —, epochs
    [dict(costs, g, masses, kbest, uniform, moves)], moves being one record per agent: pulls [dict(j, n_swaps, moved, pairs)] — the
    live pulls in kbest order, moved: j < i and positions[j] is no longer what it was at the epoch's start —, wanted (the length of
    the concatenation before the cut), velocity (the swaps applied), unchanged (the position came back as it was), cost; counters;
    agents.  RefPanics where the reference panics.
    seq: which statement of swap_sequence to use (tested equal; the literal search is O(n^2)).
    mutate: a deliberately WRONG variant, for the tests that show the cases tell it apart: "epoch_start" (every pull reads the
    epoch-start positions), "by_rank" (r keyed by the rank instead of the agent), "unstable" (ties in descending index), "no_cut"
    (no cut to v_max)."""
    N = agents(n_nearest)
    kb = kbest_count(N)
    key = chain_key(seed, run)
    vm = vmax(n)
    d = dist_fn(xy, packed, n) if n >= 2 else None
    length = (lambda r: tour_length(d, np.asarray(r, dtype=np.int64))) if n >= 2 else (lambda r: np.float32(0.0))  # noqa: E731
    pos = [[int(v) for v in init] if (i == 0 and init is not None) else shuffled(key, n, i) for i in range(N)]
    costs = [length(t) for t in pos]
    if any(c != c for c in costs):
        raise RefPanics("a start cost is NaN")
    b = 0
    for i in range(1, N):
        if costs[i] < costs[b]:  # min_by keeps the first of equals
            b = i
    gbest, gcost = list(pos[b]), costs[b]
    improvements = [(NONE, b, gcost, list(gbest))]
    eps = []
    for e in range(epochs):
        m, rank, is_uniform = masses_of(costs)
        if mutate == "unstable":
            rank = sorted(range(N), key=lambda a: (-m[a], -a))
        kbest = rank[:kb]
        g = g_of(e, epochs)
        start = [list(t) for t in pos]
        moves = []
        for i in range(N):
            inertia_keep = keep(INERTIA_W * 0.0)  # nothing of the old velocity is kept
            vel, pulls = [], []
            assert inertia_keep == 0
            for rk, j in enumerate(kbest):
                if j == i:
                    continue
                r = uniform(draw_key(key, event(e, N, i, rk if mutate == "by_rank" else j), SLOT_R))
                k = pull_swaps(r, g, m[j])
                if k == 0:
                    continue
                assert k <= MAX_PULL
                pairs = pull(pos[i], start[j] if mutate == "epoch_start" else pos[j], k, seq)
                pulls.append(dict(j=j, n_swaps=k, moved=bool(j < i and pos[j] != start[j]), pairs=pairs))
                vel += pairs
            wanted = len(vel)
            if mutate != "no_cut":
                vel = vel[:vm]
            new = apply_swaps(pos[i], vel)
            unchanged = new == pos[i]
            pos[i] = new
            costs[i] = length(new)
            if costs[i] < gcost:
                gbest, gcost = list(new), costs[i]
                improvements.append((e, i, gcost, list(gbest)))
            moves.append(dict(pulls=pulls, wanted=wanted, velocity=vel, unchanged=unchanged, cost=costs[i]))
        eps.append(dict(costs=list(costs), g=g, masses=m, kbest=kbest, rank=rank, uniform=is_uniform, moves=moves))
    return dict(tour=np.asarray(gbest, dtype=np.uint32), cost=np.float32(length(gbest)), improvements=improvements, epochs=eps,
                counters=dict(moves=epochs * N, improved=len(improvements) - 1), agents=N)


def f64_bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def epoch_words(res):
    """the per-epoch record: agent cost bits | velocity length | live pulls | g's bits, low word first"""
    N = res["agents"]
    rows = [[bits(c) for c in ep["costs"]] + [len(m["velocity"]) for m in ep["moves"]] + [len(m["pulls"]) for m in ep["moves"]] +
            [f64_bits(ep["g"]) & 0xFFFFFFFF, f64_bits(ep["g"]) >> 32] for ep in res["epochs"]]
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 3 * N + 2)


def pairs_words(pairs):
    return [i | (j << 16) for i, j in pairs]


def evidence(res):
    """the share of live pulls whose j had already moved in the epoch, and the mean number of live pulls per move"""
    pulls = [p for ep in res["epochs"] for m in ep["moves"] for p in m["pulls"]]
    moves = sum(len(ep["moves"]) for ep in res["epochs"])
    return dict(moved_share=(sum(p["moved"] for p in pulls) / len(pulls)) if pulls else 0.0, live_per_move=len(pulls) / max(moves, 1))


solve_cached = cached(solve)
