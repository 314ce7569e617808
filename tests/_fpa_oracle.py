"""The specification of the project's flower pollination solver, in numpy and literal loops (TEST infrastructure, not product code).

flower_pollination.rs:53-151 with one deliberate difference, because the reference's unseeded thread RNG cannot be reproduced: the
random draws are a pure function of (seed, run, event, slot) — the stream of tests/_ga_oracle.py, laid out as
teeline_amd/csrc/fpa_spec.h says; the Lévy step is tests/_cs_oracle.py's (teeline_amd/csrc/levy_spec.h), unchanged.  Everything else
is the reference's, quirks included: N = max(n_nearest, 25) flowers; switch_prob = 0.8 where the f32 mutation_probability is below
0.01; flower 0 is the initial tour where one is given; gbest is a COPY of the FIRST minimum flower; a global move takes a prefix of
swap_sequence(flower i, gbest), a local one a prefix of swap_sequence(flower j, flower k) — from the flowers AS THEY STAND — and
applies it to flower i; an empty sequence leaves the flower unchanged and draws nothing further; the test is strict; gbest is
updated at once, so the next flower of the same epoch sees it.  Python floats are IEEE f64 and Python never fuses a multiply with
an add.
"""
import math

import numpy as np

from _cs_oracle import WORDS, levy_from_words
from _ga_oracle import SLOT_SHUFFLE, draw, draw_key, init_event, position  # noqa: F401  (draw: re-exported)
from _sa_oracle import chain_key, dist_fn, tour_length
from _swarm_oracle import (NONE, apply_swaps, bits, cached, log_words, messages, route_words, shuffled, swap_sequence_inverse,  # noqa: F401
                           swap_sequence_literal, uniform)

SLOT_SWITCH, SLOT_LEVY, SLOT_J, SLOT_K, SLOT_EPSILON = 0, 1, 13, 14, 15
DEFAULT_FLOWERS = 25
MAX_FLOWERS = 4096
DEFAULTS = dict(epochs=10_000, n_nearest=3, mutation_probability=0.001)  # mod.rs:604-611, 1003-1010
GLOBAL_BIT = 1 << 31


def flowers(n_nearest):
    return max(int(n_nearest), DEFAULT_FLOWERS)


def switch_prob(mutation_probability):
    """flower_pollination.rs:65-69: the comparison is in f32"""
    p = np.float32(mutation_probability)
    return 0.8 if p < np.float32(0.01) else float(p)


def event(epoch, N, i):
    return epoch * N + i


def clamped_ceil(x, length):
    """`(x.ceil() as usize).clamp(1, len)`, Rust's `as`: NaN gives 0, +inf saturates"""
    if x != x or not x > 0.0:
        return 1
    if x == math.inf:
        return length
    return min(max(int(math.ceil(x)), 1), length)


def global_swaps(levy, length):
    """flower_pollination.rs:23: (levy len) 0.5, left to right"""
    return clamped_ceil(levy * float(length) * 0.5, length) if length else 0


def local_swaps(epsilon, length):
    """flower_pollination.rs:49"""
    return clamped_ceil(epsilon * float(length), length) if length else 0


def step_over(r, excluded):
    """r counts the allowed indices in ascending order: the index it names"""
    for x in sorted(excluded):
        if r >= x:
            r += 1
    return r


def partners(key, ev, i, N):
    j = step_over(position(draw_key(key, ev, SLOT_J), N - 1), [i])
    k = step_over(position(draw_key(key, ev, SLOT_K), N - 2), [i, j])
    return j, k


def roles(n, N, epochs, seeded):
    """every (event, slot) a run may draw, with its role: for the test that no two roles share one"""
    out = []
    for i in range(N):
        if seeded and i == 0:
            continue
        out += [(init_event(n, i, j), SLOT_SHUFFLE, ("shuffle", i, j)) for j in range(n - 1, 0, -1)]
    for e in range(epochs):
        for i in range(N):
            ev = event(e, N, i)
            out.append((ev, SLOT_SWITCH, ("switch", e, i)))
            out += [(ev, SLOT_LEVY + s, ("levy", e, i, s)) for s in range(WORDS)]
            out += [(ev, SLOT_J, ("j", e, i)), (ev, SLOT_K, ("k", e, i)), (ev, SLOT_EPSILON, ("epsilon", e, i))]
    return out


def pollinate(flower, source, target, prefix, seq=swap_sequence_literal):
    """the move on given tours: (the sequence's length, flower after the first min(prefix, length) swaps of it)"""
    s = seq(source, target)
    return len(s), apply_swaps(flower, s[:min(prefix, len(s))])


def move(key, ev, i, N, sp, flower_i, gbest, flower_of, seq, half=0.5):
    """one move: dict(kind, j, k, len, prefix, levy or epsilon, new)"""
    if uniform(draw_key(key, ev, SLOT_SWITCH)) < sp:
        s = seq(flower_i, gbest)
        rec = dict(glob=True, j=0, k=0, len=len(s), prefix=0, levy=None, new=list(flower_i))
        if s:
            levy, _ = levy_from_words([draw_key(key, ev, SLOT_LEVY + w) for w in range(WORDS)])
            rec["levy"] = abs(levy)
            rec["prefix"] = clamped_ceil(abs(levy) * float(len(s)) * half, len(s))
            rec["new"] = apply_swaps(flower_i, s[:rec["prefix"]])
        return rec
    j, k = partners(key, ev, i, N)
    s = seq(flower_of(j), flower_of(k))
    rec = dict(glob=False, j=j, k=k, len=len(s), prefix=0, epsilon=None, new=list(flower_i))
    if s:
        rec["epsilon"] = uniform(draw_key(key, ev, SLOT_EPSILON))
        rec["prefix"] = local_swaps(rec["epsilon"], len(s))
        rec["new"] = apply_swaps(flower_i, s[:rec["prefix"]])
    return rec


def solve(xy, packed, n, init=None, *, epochs, n_nearest=3, mutation_probability=0.001, seed=1, run=0, seq=swap_sequence_literal, mutate=None):
    """One run.  Returns a dict: tour, cost, improvements [(epoch or NONE, flower, cost, route)] — the start gbest first —, epochs
    [dict(costs, moves)], moves being one record per flower: glob, j, k, len, prefix, levy / epsilon, accepted, again, cost, and
    for a flower with `again` set, differs: whether the move built against the epoch-start state gives another tour; counters;
    flowers.  `again` is a fact of the sequential algorithm: the move read gbest after it changed in this epoch (global), or a
    flower j or k accepted earlier in this epoch (local).
    seq: which statement of swap_sequence to use (tested equal; the literal search is O(n^2)).
    mutate: a deliberately WRONG variant, for the tests that show the cases tell it apart: "epoch_start" (the second build dropped:
    every flower moves against the epoch-start state), "le" (acceptance with <=), "no_half" (the global length without the 0.5)."""
    N = flowers(n_nearest)
    sp = switch_prob(mutation_probability)
    key = chain_key(seed, run)
    d = dist_fn(xy, packed, n) if n >= 2 else None
    length = (lambda r: tour_length(d, np.asarray(r, dtype=np.int64))) if n >= 2 else (lambda r: np.float32(0.0))  # noqa: E731
    fl = [[int(v) for v in init] if (i == 0 and init is not None) else shuffled(key, n, i) for i in range(N)]
    costs = [length(t) for t in fl]
    b = 0
    for i in range(1, N):
        if costs[i] < costs[b]:  # min_by keeps the first of equals
            b = i
    gbest, gcost = list(fl[b]), costs[b]
    improvements = [(NONE, b, gcost, list(gbest))]
    half = 1.0 if mutate == "no_half" else 0.5
    eps = []
    for e in range(epochs):
        start, gstart = [list(t) for t in fl], list(gbest)
        accepted, changed, moves = [False] * N, False, []
        for i in range(N):
            ev = event(e, N, i)
            rec = move(key, ev, i, N, sp, fl[i], gbest, lambda q: fl[q], seq, half)  # the reference: from the state as it stands
            again = changed if rec["glob"] else (accepted[rec["j"]] or accepted[rec["k"]])
            differs = False
            if again or mutate == "epoch_start":
                staged = move(key, ev, i, N, sp, start[i], gstart, lambda q: start[q], seq, half)
                differs = bool(again and rec["new"] != staged["new"])
                if mutate == "epoch_start":
                    rec = staged
            rec["again"], rec["differs"] = bool(again), differs
            cost = length(rec["new"])
            ok = cost <= costs[i] if mutate == "le" else cost < costs[i]
            rec["cost"], rec["accepted"] = cost, bool(ok)
            if ok:
                fl[i], costs[i] = rec["new"], cost
                accepted[i] = True
                if cost < gcost:
                    gbest, gcost = list(rec["new"]), cost
                    changed = True
                    improvements.append((e, i, cost, list(gbest)))
            moves.append(rec)
        eps.append(dict(costs=list(costs), moves=moves))
    return dict(tour=np.asarray(gbest, dtype=np.uint32), cost=np.float32(length(gbest)), improvements=improvements, epochs=eps,
                counters=dict(moves=epochs * N, improved=len(improvements) - 1), flowers=N)


def epoch_words(res):
    """the per-epoch record: flower cost bits | bit 31 global, else j | k << 12 | sequence length | prefix << 16 | bit 0 accepted, bit 1 built again"""
    N = res["flowers"]
    rows = [[bits(c) for c in ep["costs"]] + [GLOBAL_BIT if m["glob"] else m["j"] | (m["k"] << 12) for m in ep["moves"]] +
            [m["len"] | (m["prefix"] << 16) for m in ep["moves"]] + [int(m["accepted"]) | (int(m["again"]) << 1) for m in ep["moves"]] for ep in res["epochs"]]
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 4 * N)


solve_cached = cached(solve)
