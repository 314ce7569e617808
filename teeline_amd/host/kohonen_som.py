"""som::solve — mirror of src/tsp/som.rs:12-186 over tl_kohonen_som.

The algorithm is the reference's Kohonen self-organising map, quirks included (a start tour is ignored, per-axis normalisation with
span max(max - min, 1e-9), a sequential centroid, M = n neuron_multiplier neurons on a circle of radius 0.1, sigma floored at 1, the
FIRST minimum as the BMU, the 1e-3 cut, in-place updates, the tour by (neuron, distance, city index)).  Three things are this
project's specification instead: the city of an epoch is a pure function of (seed, run, epoch) — the reference's RNG is unseeded —,
exp is a fixed f64 sequence with a cut at -8 before it, and the start ring's cos and sin are a fixed f64 sequence
(include/teeline_gpu.h).
"""
import ctypes as C

import numpy as np

from ._chains import bits_to_f32, solve_chains, vp

NONE = 0xFFFFFFFF


class SOMOptions:
    """src/tsp/mod.rs:1465-1499"""

    def __init__(self, epochs=100_000, learning_rate=0.8, radius_fraction=0.1, neuron_multiplier=8):
        self.epochs, self.learning_rate, self.radius_fraction, self.neuron_multiplier = epochs, learning_rate, radius_fraction, neuron_multiplier

    def validate(self):  # mod.rs:1485-1499
        if self.epochs == 0:
            raise ValueError("epochs must be >= 1")
        if self.learning_rate <= 0.0 or self.learning_rate > 1.0:
            raise ValueError("learning_rate must be in (0, 1]")
        if self.radius_fraction <= 0.0 or self.radius_fraction > 1.0:
            raise ValueError("radius_fraction must be in (0, 1]")
        if self.neuron_multiplier == 0:
            raise ValueError("neuron_multiplier must be >= 1")


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, runs=1, form=0):
    """opts: SOMOptions.  progress_tx: optional callable(kind, payload).  init_tour is ignored, as the reference ignores it.  With
    checkpoint = max(epochs / 10, 1) the reference sends EpochUpdate(t) then PathUpdate(snapshot, cost) at every t % checkpoint == 0,
    a final PathUpdate only when epochs % checkpoint != 0, then Done (som.rs:117-145; nothing at all for n < 2); with a channel the
    solve goes through tl_kohonen_som_trace and the sequence is replayed from its records.  runs > 1: runs 0 .. runs-1 of `seed` at
    once (tl_kohonen_som_population), the best one (lowest cost, then lowest run) returned; the replay is of that run."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or SOMOptions()
    n = len(problem)
    if problem.xy is None:
        raise ValueError("kohonen_som trains on the coordinates: the problem has none")
    o = _capi.TlSomOpts(int(opts.epochs), int(opts.neuron_multiplier), float(opts.learning_rate), float(opts.radius_fraction), int(form), 0, 0)
    packed = problem.explicit_packed()
    head = (ctx.handle, vp(problem.xy), n, vp(packed))

    def population(count, outs, costs, _moves, best, st):
        ctx.check(ctx.lib.tl_kohonen_som_population(*head, 0, count, C.byref(o), seed, vp(outs), vp(costs), C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(ctx.lib.tl_kohonen_som(*head, C.byref(o), seed, vp(out), C.byref(cost), C.byref(st)))

    def trace(run):
        out = np.empty(n, dtype=np.uint32)
        cost, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
        cap = 20
        ep, tours, bits = np.empty(cap, dtype=np.uint32), np.empty((cap, max(n, 1)), dtype=np.uint32), np.empty(cap, dtype=np.uint32)
        ctx.check(ctx.lib.tl_kohonen_som_trace(*head, C.byref(o), seed, run, vp(out), C.byref(cost), C.byref(st), None, 0, None, vp(ep), vp(tours), vp(bits), cap,
                                               C.byref(ln)))
        k = ln.value
        return out, cost.value, (ep[:k], tours[:k, :n], bits[:k]), dict(st.as_dict(), run=run)

    def replay(record):
        ep, tours, bits = record
        ids = problem.ids
        for k in range(len(ep)):
            if ep[k] != NONE:
                progress_tx("EpochUpdate", int(ep[k]))
            progress_tx("PathUpdate", ([int(v) for v in ids[tours[k]]], float(bits_to_f32(bits[k]))))
        if n >= 2:
            progress_tx("Done", None)

    sol = solve_chains(problem, progress_tx, runs, population, single, trace, replay)
    if "chain" in sol.stats:
        sol.stats["run"] = sol.stats.pop("chain")
    return sol
