"""The specification of the project's particle swarm solver, in numpy and literal loops (TEST infrastructure, not product code).

particle_swarm.rs:22-129 with two deliberate differences, because the reference's unseeded thread RNG cannot be reproduced and
`f64::round` must be the same operations everywhere: the random draws are a pure function of (seed, run, event, slot) — the stream
of tests/_ga_oracle.py (teeline_amd/csrc/pso_spec.h) — and the rounding is spelled out as t = trunc(x), t + (x - t >= 0.5).
Everything else is the reference's, quirks included: P = max(n_nearest, 30); v_max = max(ceil(0.35 n), 1); particle 0 is the
initial tour where one is given; gbest is the FIRST minimum; both swap sequences are taken from the same position and are lists of
position pairs; a keep may exceed its list (`take` clamps); truncation comes after concatenation; gbest is updated at once, so the
next particle of the same epoch already sees it.  Python floats are IEEE f64 and Python never fuses a multiply with an add.
"""
import math

import numpy as np

from _ga_oracle import SLOT_SHUFFLE, draw, draw_key, init_event, position  # noqa: F401  (draw: re-exported)
from _sa_oracle import chain_key, dist_fn, tour_length
from _swarm_oracle import (NONE, apply_swaps, bits, cached, log_words, orbits, route_words, shuffled, swap_sequence_inverse,  # noqa: F401
                           swap_sequence_literal, swap_sequence_orbit, uniform)

SLOT_R1, SLOT_R2 = 0, 1
DEFAULT_PARTICLES = 30
MAX_PARTICLES = 4096
DEFAULTS = dict(epochs=10_000, n_nearest=3)  # mod.rs:604-611


def particles(n_nearest):
    return max(int(n_nearest), DEFAULT_PARTICLES)


def vmax(n):
    return max(int(math.ceil(n * 0.35)), 1)


def step_event(epoch, P, particle):
    return epoch * P + particle


def weight(epoch, epochs):
    return 0.9 - (0.9 - 0.4) * (epoch / max(epochs, 1))


def keep(x):
    """`x.round() as usize` for x >= 0: half away from zero, spelled out"""
    if not x > 0.0:
        return 0
    t = math.trunc(x)
    return t + 1 if x - t >= 0.5 else t


def roles(n, P, epochs, seeded):
    """every (event, slot) the run draws, with its role: for the test that no two roles share one"""
    out = []
    for i in range(P):
        if seeded and i == 0:
            continue
        out += [(init_event(n, i, j), SLOT_SHUFFLE, ("shuffle", i, j)) for j in range(n - 1, 0, -1)]
    for e in range(epochs):
        for i in range(P):
            out.append((step_event(e, P, i), SLOT_R1, ("r1", e, i)))
            out.append((step_event(e, P, i), SLOT_R2, ("r2", e, i)))
    return out


def solve(xy, packed, n, init=None, *, epochs, n_nearest=3, seed=1, run=0, seq=swap_sequence_literal, mutate=None):
    """One run.  Returns a dict: tour, cost, improvements [(epoch or NONE, particle, cost, route)] — the start gbest first —,
    epochs [dict(costs, vlens, steps)], steps being one record per particle step: the three products before rounding, the three keeps as rounded, the three list
    lengths, the clamped parts, where truncation cut (None, "cog" or "soc"), the new velocity's length, the cost; counters.
    seq: which statement of swap_sequence to use (they are tested equal; the literal search is O(n^2)).
    mutate: a deliberately WRONG variant, for the tests that show the cases tell it apart: "no_redo" (every particle of an epoch
    sees the epoch-start gbest), "half_even" (np.round), "truncate_first" (each part cut to v_max before concatenation)."""
    P, vm = particles(n_nearest), vmax(n)
    if n <= 1:  # nothing to swap, no edge: every particle stays where it is at cost 0
        zero = np.float32(0.0)
        eps = [dict(costs=[zero] * P, vlens=[0] * P, steps=[]) for _ in range(epochs)]
        return dict(tour=np.arange(n, dtype=np.uint32), cost=zero, improvements=[(NONE, 0, zero, list(range(n)))], epochs=eps,
                    counters=dict(steps=epochs * P, improved=0), particles=P, vmax=vm)
    d = dist_fn(xy, packed, n)
    key = chain_key(seed, run)
    length = lambda r: tour_length(d, np.asarray(r, dtype=np.int64))  # noqa: E731
    rnd = (lambda x: int(np.round(x))) if mutate == "half_even" else keep
    pos = [[int(v) for v in init] if (i == 0 and init is not None) else shuffled(key, n, i) for i in range(P)]
    vel = [[] for _ in range(P)]
    pbest = [list(p) for p in pos]
    pcost = [length(p) for p in pbest]
    b = 0
    for i in range(1, P):
        if pcost[i] < pcost[b]:  # min_by keeps the first of equals
            b = i
    gbest, gcost = list(pbest[b]), pcost[b]
    improvements = [(NONE, b, gcost, list(gbest))]
    eps = []
    for e in range(epochs):
        w = weight(e, epochs)
        steps = []
        seen = list(gbest)  # (mutate == "no_redo" only)
        for i in range(P):
            ev = step_event(e, P, i)
            r1, r2 = uniform(draw_key(key, ev, SLOT_R1)), uniform(draw_key(key, ev, SLOT_R2))
            cog = seq(pos[i], pbest[i])
            soc = seq(pos[i], seen if mutate == "no_redo" else gbest)
            xs = (w * len(vel[i]), (1.5 * r1) * len(cog), (1.5 * r2) * len(soc))
            ik, ck, sk = rnd(xs[0]), rnd(xs[1]), rnd(xs[2])
            a, c, s = min(ik, len(vel[i])), min(ck, len(cog)), min(sk, len(soc))
            if mutate == "truncate_first":
                new = (vel[i][:ik][:vm] + cog[:ck][:vm] + soc[:sk][:vm])
            else:
                new = (vel[i][:ik] + cog[:ck] + soc[:sk])[:vm]
            cut = None if a + c + s <= vm else "cog" if a + c > vm else "soc"
            steps.append(dict(xs=xs, keeps=(ik, ck, sk), lens=(len(vel[i]), len(cog), len(soc)), parts=(a, c, s), cut=cut, vlen=len(new)))
            pos[i] = apply_swaps(pos[i], new)
            vel[i] = new
            cost = length(pos[i])
            steps[-1]["cost"] = cost
            if cost < pcost[i]:
                pbest[i], pcost[i] = list(pos[i]), cost
            if cost < gcost:
                gbest, gcost = list(pos[i]), cost
                improvements.append((e, i, cost, list(gbest)))
        eps.append(dict(costs=[s["cost"] for s in steps], vlens=[s["vlen"] for s in steps], steps=steps))
    return dict(tour=np.asarray(gbest, dtype=np.uint32), cost=np.float32(length(gbest)), improvements=improvements, epochs=eps,
                counters=dict(steps=epochs * P, improved=len(improvements) - 1), particles=P, vmax=vm)


def epoch_words(res):
    """the per-epoch record: every particle's cost bits, then every particle's velocity length"""
    P = res["particles"]
    return np.asarray([[bits(c) for c in ep["costs"]] + list(ep["vlens"]) for ep in res["epochs"]], dtype=np.uint32).reshape(-1, 2 * P)


def messages(res, ids=None):  # (not _swarm_oracle's: this one tolerates an empty improvement list, as the reference's `if let Some` does)
    """what the reference sends (particle_swarm.rs:72-74,114-116,120-122,125-127)"""
    name = (lambda r: [int(v) for v in r]) if ids is None else (lambda r: [int(v) for v in np.asarray(ids)[np.asarray(r, dtype=np.int64)]])
    imp = res["improvements"]
    out = []
    if imp:
        out.append(("PathUpdate", (name(imp[0][3]), float(imp[0][2]))))
        k = 1
        for e in range(len(res["epochs"])):
            while k < len(imp) and imp[k][0] == e:
                out.append(("PathUpdate", (name(imp[k][3]), float(imp[k][2]))))
                k += 1
            out.append(("EpochUpdate", e))
    out.append(("Done", None))
    return out


solve_cached = cached(solve)
