"""flower_pollination::solve — mirror of src/tsp/flower_pollination.rs:53-151 over tl_flower_pollination.

The algorithm is the reference's flower pollination, quirks included (max(n_nearest, 25) flowers, switch_prob 0.8 where
mutation_probability is below 0.01, gbest a copy of the first minimum flower, a global move along a prefix of the swap sequence to
gbest, a local one along a prefix of the sequence between two other flowers as they stand, strict acceptance, gbest updated at
once).  Two things are this project's specification instead: the random draws are a pure function of (seed, run, epoch, flower,
role) — the reference's thread RNG is unseeded — and the Lévy step is a fixed sequence of f64 operations (include/teeline_gpu.h,
DESIGN.md §4.22).
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, solve_chains, vp


class FPAOptions:
    """FPAOptions (src/tsp/mod.rs:998-1026)"""

    def __init__(self, heuristic=None, mutation_probability=0.001, **kw):
        self.heuristic = heuristic or HeuristicOptions(**kw)
        self.mutation_probability = float(mutation_probability)

    def validate(self):
        p = self.mutation_probability
        if not (np.isfinite(p) and 0.0 <= p <= 1.0):
            raise ValueError(f"mutation_probability must be in [0, 1] (got {p})")


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, runs=1):
    """opts: FPAOptions (or HeuristicOptions: the default mutation_probability).  progress_tx: optional callable(kind, payload).  The
    reference sends PathUpdate(start gbest, its cost), per epoch a PathUpdate per gbest improvement in the order they happen and
    EpochUpdate(epoch), then Done (flower_pollination.rs:113-115,133-136,142-149); with a channel the solve goes through
    tl_flower_pollination_trace and the sequence is replayed from its log.  runs > 1: runs 0 .. runs-1 of `seed` at once
    (tl_flower_pollination_population), the best one (lowest cost, then lowest run) returned; the replay is of that run."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or FPAOptions()
    if isinstance(opts, HeuristicOptions):
        opts = FPAOptions(opts)
    opts.validate()
    n = len(problem)
    epochs = int(opts.heuristic.epochs)
    o = _capi.TlFpaOpts(epochs, int(opts.heuristic.n_nearest), opts.mutation_probability)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    head = (ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos))

    def population(count, outs, costs, moves, best, st):
        ctx.check(ctx.lib.tl_flower_pollination_population(*head, 0 if init_pos is None else 1, 0, count, C.byref(o), seed, vp(outs), vp(costs), vp(moves),
                                                      C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(ctx.lib.tl_flower_pollination(*head, C.byref(o), seed, vp(out), C.byref(cost), C.byref(st)))

    def trace(run):
        # the improvements are few but not known in advance: read the count first
        out = np.empty(n, dtype=np.uint32)
        cost, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
        cap = 64
        while True:
            log = np.empty((cap, 4), dtype=np.uint32)
            routes = np.empty((cap, max(n, 1)), dtype=np.uint32)
            ctx.check(ctx.lib.tl_flower_pollination_trace(*head, C.byref(o), seed, run, vp(out), C.byref(cost), C.byref(st), vp(log), cap, C.byref(ln), vp(routes), cap,
                                                     None, 0))
            if ln.value <= cap:
                break
            cap = ln.value
        return out, cost.value, (log[:ln.value], routes[:ln.value, :n]), dict(st.as_dict(), run=run)

    def replay(record):
        log, routes = record
        ids = problem.ids
        send = lambda k: progress_tx("PathUpdate", ([int(v) for v in ids[routes[k]]], float(bits_to_f32(log[k, 2]))))  # noqa: E731
        if len(log):
            send(0)
        k = 1
        for e in range(epochs):
            while k < len(log) and log[k, 0] == e:
                send(k)
                k += 1
            progress_tx("EpochUpdate", e)
        progress_tx("Done", None)

    sol = solve_chains(problem, progress_tx, runs, population, single, trace, replay)
    if "chain" in sol.stats:
        sol.stats["run"] = sol.stats.pop("chain")
    return sol
