"""genetic_algorithm::solve — mirror of src/tsp/genetic_algorithm.rs:16-336 over tl_genetic_algorithm.

The algorithm is the reference's, quirks included (a population of n only in generation 0; roulette over the sorted population with a
sequential f32 running sum; child 1 of the ordered crossover carries parent 2's segment; a mutation does not recompute the fitness;
the best is the last of equal maxima and its cost is recomputed).  One thing is this project's specification instead: the random
draws are a pure function of (seed, run, generation, pair or individual, role) — the reference's thread RNG is unseeded
(include/teeline_gpu.h).
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, vp


class GAOptions:
    """src/tsp/mod.rs:815-846"""

    def __init__(self, heuristic=None, mutation_probability=0.001, n_elite=3):
        self.heuristic = heuristic or HeuristicOptions()
        self.mutation_probability, self.n_elite = mutation_probability, n_elite

    @property
    def epochs(self):
        return self.heuristic.epochs

    def validate(self):
        self.heuristic.validate()
        p = float(self.mutation_probability)
        if not np.isfinite(p) or p < 0.0 or p > 1.0:
            raise ValueError(f"mutation_probability must be in [0, 1] (got {self.mutation_probability})")


def _options(opts):
    """GAOptions, or any options with `epochs` (HeuristicOptions: the GA's own defaults for the rest)"""
    if opts is None:
        return GAOptions()
    if isinstance(opts, GAOptions):
        return opts
    return GAOptions(heuristic=opts, mutation_probability=getattr(opts, "mutation_probability", 0.001), n_elite=getattr(opts, "n_elite", 3))


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, seed=1, runs=1, ctx=None):
    """progress_tx: optional callable(kind, payload).  The reference sends one PathUpdate(best route, its tour_length) per generation,
    then one more and Done (genetic_algorithm.rs:33-40,91-98); with a channel the solve goes through tl_genetic_algorithm_trace_run
    and the sequence is replayed from the per-generation trace and route log.  runs > 1: runs 0 .. runs-1 of `seed` are bred at once
    (tl_genetic_algorithm_population) and the best one (lowest cost, then lowest run) is returned; the replay is of that run."""
    from . import Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = _options(opts)
    opts.validate()
    n = len(problem)
    epochs, p, e = int(opts.epochs), float(opts.mutation_probability), int(opts.n_elite)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    st = _capi.TlStats()
    run, extra = 0, {}
    if runs > 1:
        outs = np.empty((runs, n), dtype=np.uint32)
        costs = np.empty(runs, dtype=np.float32)
        best = C.c_uint32()
        ctx.check(ctx.lib.tl_genetic_algorithm_population(ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos), 0, runs, epochs, p, e, seed, vp(outs),
                                                          vp(costs), C.byref(best), C.byref(st)))
        run = int(best.value)
        out, cost, extra = outs[run], float(costs[run]), {"run": run}
        if progress_tx is None:
            return Solution(cost, problem.ids[out], problem, dict(st.as_dict(), **extra))
    elif progress_tx is None:
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        ctx.check(ctx.lib.tl_genetic_algorithm(ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos), epochs, p, e, seed, vp(out), C.byref(cost), C.byref(st)))
        return Solution(cost.value, problem.ids[out], problem, st.as_dict())
    # the run once more (or for the first time), alone, with its generations
    out = np.empty(n, dtype=np.uint32)
    cost = C.c_float()
    st1 = _capi.TlStats()
    log = np.empty((max(epochs, 1), 4), dtype=np.uint32)
    routes = np.empty((max(epochs, 1), n), dtype=np.uint32)
    ln = C.c_uint32()
    ctx.check(ctx.lib.tl_genetic_algorithm_trace_run(ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos), epochs, p, e, seed, run, vp(out), C.byref(cost),
                                                     C.byref(st1), vp(log), epochs, C.byref(ln), vp(routes), epochs))
    ids = problem.ids
    for g in range(epochs):
        progress_tx("PathUpdate", ([int(v) for v in ids[routes[g]]], float(bits_to_f32(log[g, 2]))))
    progress_tx("PathUpdate", ([int(v) for v in ids[out]], float(cost.value)))
    progress_tx("Done", None)
    return Solution(cost.value, ids[out], problem, dict((st if runs > 1 else st1).as_dict(), **extra))
