"""The specification of the project's Kohonen self-organising map solver, in numpy and literal loops (TEST infrastructure, not
product code).

som.rs:12-186 with three deliberate differences (teeline_amd/csrc/som_spec.h).  The reference's unseeded RNG cannot
be reproduced: the city of epoch t of run r is position(u(seed, r, event t, slot 0), n) on the stream of tests/_ga_oracle.py.  exp is
the fixed f64 sequence of tests/_cs_oracle.py (exp_spec), not libm's, and a neuron with y = ((-d) d) / two_sigma_sq < -8.0 is skipped
without it.  The start ring's cos and sin of 2 pi (i / M) come from the Lévy step's exact quadrant reduction and its two polynomials.
Everything else is the reference's, quirks included: a start tour is ignored; per-axis normalisation in f64 with span
max(max - min, 1e-9); the centroid a sequential sum in city order; sigma floored at 1; the FIRST minimum as the BMU; the 1e-3 cut;
in-place updates (eta h) (city - neuron); the tour by (neuron, distance, city index); the f32 sequential tour length.  Python floats
are IEEE f64 and neither Python nor numpy fuses a multiply with an add.
"""
import math

import numpy as np

from _cs_oracle import COS_C, HALF_PI, SIN_C, _horner, exp_spec
from _ga_oracle import draw, draw_key, position  # noqa: F401  (draw: re-exported)
from _sa_oracle import chain_key, dist_fn, tour_length
from _swarm_oracle import bits, cached, read_only  # noqa: F401  (bits: re-exported)

SLOT_CITY = 0
MAX_NEURONS = 65536
CUT_Y, CUT_H = -8.0, 1e-3
DEFAULTS = dict(epochs=100_000, learning_rate=0.8, radius_fraction=0.1, neuron_multiplier=8)  # mod.rs:1473-1482
NONE = 0xFFFFFFFF


def validate(epochs, learning_rate, radius_fraction, neuron_multiplier):
    """SOMOptions::validate (mod.rs:1485-1499)"""
    return epochs >= 1 and 0.0 < learning_rate <= 1.0 and 0.0 < radius_fraction <= 1.0 and neuron_multiplier >= 1


def city_of(key, t, n):
    return position(draw_key(key, t, SLOT_CITY), n)


def exp_libm(y):
    return np.exp(np.asarray(y, dtype=np.float64))


def schedule(t, epochs, M, eta0, rf, exp=exp_spec):
    """(eta, sigma, two_sigma_sq, radius) of epoch t = 1 .. epochs (som.rs:79-82)"""
    decay = float(exp(np.float64((-float(t)) / float(epochs))))
    sigma = (rf * float(M)) * decay
    if not sigma > 1.0:
        sigma = 1.0
    tss = (2.0 * sigma) * sigma
    radius = min(M, int(math.floor(math.sqrt(8.0 * tss))) + 2)
    return eta0 * decay, sigma, tss, radius


def h_of(d, tss, exp=exp_spec):
    """(moved, h) of a ring distance (som.rs:108-111 with the cut at -8 before the exp)"""
    y = ((-float(d)) * float(d)) / tss
    if y < CUT_Y:
        return False, 0.0
    h = float(exp(np.float64(y)))
    return not h < CUT_H, h


def cossin2pi(u):
    """(cos 2 pi u, sin 2 pi u) for f64 u in [0, 1): the quadrant reduction is exact for every such u"""
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
    return (np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s))),
            np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c))))


def cossin_libm(u):
    th = 2.0 * np.pi * np.asarray(u, dtype=np.float64)
    return np.cos(th), np.sin(th)


def normalise(xy):
    """(cities [n, 2] f64, cx, cy) (som.rs:27-50)"""
    xy = np.asarray(xy, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    n = len(xy)
    mn, mx = xy.min(axis=0), xy.max(axis=0)
    span = np.maximum(mx - mn, 1e-9)
    cities = (xy - mn) / span
    sx = sy = 0.0
    for c in range(n):  # a sequential sum in city order
        sx += float(cities[c, 0])
        sy += float(cities[c, 1])
    return cities, sx / float(n), sy / float(n)


def ring_init(cx, cy, M, cossin=cossin2pi):
    """[M, 2] f64 (som.rs:54-59)"""
    if cossin is cossin_libm:  # the reference's own order: 2 pi i / M
        th = 2.0 * np.pi * np.arange(M, dtype=np.float64) / float(M)
        c, s = np.cos(th), np.sin(th)
    else:
        c, s = cossin(np.arange(M, dtype=np.float64) / float(M))
    return np.stack([cx + 0.1 * c, cy + 0.1 * s], axis=1)


def first_min(ring, city):
    """(index, distance) of the FIRST minimum of sq_dist(neuron, city) (som.rs:8-10, 89-98)"""
    dx, dy = ring[:, 0] - city[0], ring[:, 1] - city[1]
    d = (dx * dx) + (dy * dy)
    i = int(np.argmin(d))  # the first occurrence
    return i, float(d[i])


def ring_distance(i, bmu, M):
    d = abs(i - bmu)
    return min(d, M - d)


def epoch_numpy(ring, city, bmu, eta, tss, exp=exp_spec):
    M = len(ring)
    i = np.arange(M, dtype=np.int64)
    d = np.abs(i - bmu)
    d = np.minimum(d, M - d).astype(np.float64)
    y = ((-d) * d) / tss
    near = np.nonzero(~(y < CUT_Y))[0]
    h = exp(y[near])
    keep = ~(h < CUT_H)
    at, h = near[keep], h[keep]
    for a in (0, 1):
        ring[at, a] = ring[at, a] + (eta * h) * (city[a] - ring[at, a])
    return len(at)


def epoch_literal(ring, city, bmu, eta, tss, exp=exp_spec):
    M = len(ring)
    moved = 0
    for i in range(M):
        ok, h = h_of(ring_distance(i, bmu, M), tss, exp)
        if not ok:
            continue
        moved += 1
        for a in (0, 1):
            ring[i, a] = float(ring[i, a]) + (eta * h) * (float(city[a]) - float(ring[i, a]))
    return moved


def extract(cities, ring):
    """extract_tour (som.rs:153-186): city indices"""
    bm = [first_min(ring, c) for c in cities]
    return sorted(range(len(cities)), key=lambda a: (bm[a][0], bm[a][1], a)), bm


def checkpoint_of(epochs):
    return max(epochs // 10, 1)


def solve(xy, packed, n, *, epochs, learning_rate=0.8, radius_fraction=0.1, neuron_multiplier=8, seed=1, run=0, literal=False, exp=exp_spec,
          cossin=cossin2pi):
    """One run.  Returns a dict: tour (city indices), cost, log [(city, bmu)] per epoch, moved [neurons updated] per epoch, ring
    [M, 2], checkpoints [(epoch or NONE, tour, cost)] in the reference's message order, schedule.  literal: the per-neuron loop
    instead of the numpy statement of an epoch (tested equal)."""
    assert validate(epochs, learning_rate, radius_fraction, neuron_multiplier)
    if n < 2:
        return dict(tour=np.arange(n, dtype=np.uint32), cost=np.float32(0.0), log=[], moved=[], ring=np.zeros((0, 2)), checkpoints=[], trivial=True)
    d = dist_fn(xy, packed, n)
    length = lambda r: tour_length(d, np.asarray(r, dtype=np.int64))  # noqa: E731
    cities, cx, cy = normalise(xy)
    M = n * neuron_multiplier
    assert M <= MAX_NEURONS
    ring = ring_init(cx, cy, M, cossin)
    key = chain_key(seed, run)
    cp = checkpoint_of(epochs)
    step = epoch_literal if literal else epoch_numpy
    log, moved, cps, sched = [], [], [], []
    for t in range(1, epochs + 1):
        eta, _sigma, tss, radius = schedule(t, epochs, M, learning_rate, radius_fraction, exp)
        c = city_of(key, t, n)
        bmu, _d = first_min(ring, cities[c])
        log.append((c, bmu))
        moved.append(step(ring, cities[c], bmu, eta, tss, exp))
        sched.append((eta, tss, radius))
        if t % cp == 0:
            tour, _bm = extract(cities, ring)
            cps.append((t, tour, length(tour)))
    tour, bm = extract(cities, ring)
    cost = length(tour)
    if epochs % cp != 0:
        cps.append((NONE, tour, cost))
    return dict(tour=np.asarray(tour, dtype=np.uint32), cost=np.float32(cost), log=log, moved=moved, ring=ring, checkpoints=cps, schedule=sched, bm=bm,
                trivial=False, neurons=M)


def f64_bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def log_words(res):
    return np.asarray(res["log"], dtype=np.uint32).reshape(-1, 2)


def ring_words(res):
    """the final ring as tl_kohonen_som_trace returns it: x[M] then y[M], as u64 bits"""
    return np.ascontiguousarray(res["ring"].T).reshape(-1).view(np.uint64)


def messages(res, ids=None):
    """what the reference sends (som.rs:117-145): nothing at all for n < 2"""
    if res["trivial"]:
        return []
    name = (lambda r: [int(v) for v in r]) if ids is None else (lambda r: [int(v) for v in np.asarray(ids)[np.asarray(r, dtype=np.int64)]])
    out = []
    for t, tour, cost in res["checkpoints"]:
        if t != NONE:
            out.append(("EpochUpdate", t))
        out.append(("PathUpdate", (name(tour), float(cost))))
    out.append(("Done", None))
    return out


solve_cached = cached(solve, lambda res: (read_only(res["tour"]), read_only(res["ring"]), res)[2])
