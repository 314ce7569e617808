"""gravitational_search::solve — mirror of src/tsp/gravitational_search.rs:23-145 over tl_gravitational_search.

The algorithm is the reference's gravitational search, quirks included (max(n_nearest, 25) agents, gbest the first minimum, the
masses and the ranking of an epoch from the costs at its start, no inertia, every pull from the positions as they stand, truncation
after concatenation, gbest updated at once within an epoch).  Three things are this project's specification instead: the random
draws are a pure function of (seed, run, epoch, agent, pulling agent) — the reference's thread RNG is unseeded —, equal masses
rank in ascending agent index — the reference's unstable sort leaves their order open — and exp is a fixed f64 sequence
(include/teeline_gpu.h).
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, solve_chains, vp


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, runs=1):
    """opts: HeuristicOptions (epochs, n_nearest).  progress_tx: optional callable(kind, payload).  The reference sends
    PathUpdate(start gbest, its cost), per epoch a PathUpdate per gbest improvement in agent order and EpochUpdate(epoch), then
    Done (gravitational_search.rs:72-74,127-143); with a channel the solve goes through tl_gravitational_search_trace and the sequence is
    replayed from its log.  runs > 1: runs 0 .. runs-1 of `seed` at once (tl_gravitational_search_population), the best one (lowest cost,
    then lowest run) returned; the replay is of that run."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or HeuristicOptions()
    n = len(problem)
    epochs = int(opts.epochs)
    o = _capi.TlGsaOpts(epochs, int(opts.n_nearest), 0)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    head = (ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos))

    def population(count, outs, costs, moves, best, st):
        ctx.check(ctx.lib.tl_gravitational_search_population(*head, 0 if init_pos is None else 1, 0, count, C.byref(o), seed, vp(outs), vp(costs), vp(moves),
                                                       C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(ctx.lib.tl_gravitational_search(*head, C.byref(o), seed, vp(out), C.byref(cost), C.byref(st)))

    def trace(run):
        # the improvements are few but not known in advance: read the count first
        out = np.empty(n, dtype=np.uint32)
        cost, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
        cap = 64
        while True:
            log = np.empty((cap, 4), dtype=np.uint32)
            routes = np.empty((cap, max(n, 1)), dtype=np.uint32)
            ctx.check(ctx.lib.tl_gravitational_search_trace(*head, C.byref(o), seed, run, vp(out), C.byref(cost), C.byref(st), vp(log), cap, C.byref(ln), vp(routes), cap,
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
