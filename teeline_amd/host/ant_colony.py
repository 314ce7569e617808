"""ant_colony::solve — mirror of src/tsp/ant_colony.rs:97-252 over tl_ant_colony.

The algorithm is the reference's Ant System, quirks included (sequential f32 sums over the unvisited cities, the eta-only and
first-candidate fallbacks, the strict roulette test, `cost < best_cost` in ant order, the evaporation floor, no deposit where
cost <= 0).  Two things are this project's specification instead: the random draws are a pure function of (seed, run, epoch, ant,
step, role) — the reference's thread RNG is unseeded — and the power function is a fixed operation sequence
(include/teeline_gpu.h).
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, vp


class AcoOptions:
    """src/tsp/mod.rs:1082-1153: 150 epochs unless the heuristic options say otherwise"""

    def __init__(self, heuristic=None, alpha=1.0, beta=2.0, evaporation_rate=0.5, num_ants=25):
        self.heuristic = heuristic or HeuristicOptions(epochs=150)
        self.alpha, self.beta, self.evaporation_rate, self.num_ants = alpha, beta, evaporation_rate, num_ants

    @property
    def epochs(self):
        return self.heuristic.epochs

    def validate(self):
        # (not heuristic.validate(): the reference's AcoOptions::validate does not call it, mod.rs:1116-1119)
        a, b, r = float(self.alpha), float(self.beta), float(self.evaporation_rate)
        if not np.isfinite(a) or a < 0.0:
            raise ValueError(f"alpha must be >= 0 (got {self.alpha})")
        if not (0.0 <= b <= 6.0):
            raise ValueError(f"beta must be in [0, 6] (got {self.beta})")
        if not np.isfinite(r) or r <= 0.0 or r >= 1.0:
            raise ValueError(f"evaporation_rate must be in (0, 1) (got {self.evaporation_rate})")
        if int(self.num_ants) < 1:
            raise ValueError("num_ants must be >= 1")


def _options(opts):
    """AcoOptions, or any options with `epochs` (HeuristicOptions: the colony's own defaults for the rest)"""
    if opts is None:
        return AcoOptions()
    if isinstance(opts, AcoOptions):
        return opts
    return AcoOptions(heuristic=opts, alpha=getattr(opts, "alpha", 1.0), beta=getattr(opts, "beta", 2.0),
                      evaporation_rate=getattr(opts, "evaporation_rate", 0.5), num_ants=getattr(opts, "num_ants", 25))


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, seed=1, runs=1, ctx=None):
    """progress_tx: optional callable(kind, payload).  The reference sends PathUpdate(start tour, its cost), a PathUpdate per
    improving ant in ant order and EpochUpdate(epoch) per epoch, then Done (ant_colony.rs:141-147,225-231,241-248); with a channel the
    solve goes through tl_ant_colony_trace_run and the sequence is replayed from the route log.  runs > 1: runs 0 .. runs-1 of `seed`
    at once (tl_ant_colony_population), the best one (lowest cost, then lowest run) returned; the replay is of that run."""
    from . import Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = _options(opts)
    opts.validate()
    n = len(problem)
    epochs, ants = int(opts.epochs), int(opts.num_ants)
    par = (float(opts.alpha), float(opts.beta), float(opts.evaporation_rate), ants, seed)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    st = _capi.TlStats()
    run, extra = 0, {}
    if runs > 1:
        outs = np.empty((runs, n), dtype=np.uint32)
        costs = np.empty(runs, dtype=np.float32)
        best = C.c_uint32()
        ctx.check(ctx.lib.tl_ant_colony_population(ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos), 0 if init_pos is None else 1, 0, runs, epochs, *par,
                                                   vp(outs), vp(costs), C.byref(best), C.byref(st)))
        run = int(best.value)
        out, cost, extra = outs[run], float(costs[run]), {"run": run}
        if progress_tx is None:
            return Solution(cost, problem.ids[out], problem, dict(st.as_dict(), **extra))
    elif progress_tx is None:
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        ctx.check(ctx.lib.tl_ant_colony(ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos), epochs, *par, vp(out), C.byref(cost), C.byref(st)))
        return Solution(cost.value, problem.ids[out], problem, st.as_dict())
    # the run once more (or for the first time), alone, with its improving ants: at most epochs x num_ants of them, so read the count first
    out = np.empty(n, dtype=np.uint32)
    cost = C.c_float()
    st1 = _capi.TlStats()
    log = np.empty((1, 3 * ants), dtype=np.uint32)
    ln, rows = C.c_uint32(), C.c_uint32()
    cap = 64
    while True:
        routes = np.empty((cap, n + 3), dtype=np.uint32)
        ctx.check(ctx.lib.tl_ant_colony_trace_run(ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos), epochs, *par, run, vp(out), C.byref(cost), C.byref(st1),
                                                  vp(log), 1, C.byref(ln), vp(routes), cap, C.byref(rows)))
        if rows.value <= cap:
            break
        cap = rows.value
    ids = problem.ids
    routes = routes[:rows.value]
    if n > 2:
        progress_tx("PathUpdate", ([int(v) for v in ids[routes[0, 3:]]], float(bits_to_f32(routes[0, 2]))))
        k = 1
        for g in range(epochs):
            while k < len(routes) and routes[k, 0] == g:
                progress_tx("PathUpdate", ([int(v) for v in ids[routes[k, 3:]]], float(bits_to_f32(routes[k, 2]))))
                k += 1
            progress_tx("EpochUpdate", g)
    progress_tx("Done", None)
    return Solution(cost.value, ids[out], problem, dict((st if runs > 1 else st1).as_dict(), **extra))
