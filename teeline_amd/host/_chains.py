"""What the mirrors of the seeded chain solvers share (simulated_annealing, tabu_search; genetic_algorithm takes the small helpers):
the ctypes plumbing, the reversal and the solve skeleton population -> best chain -> optional re-trace / single / trace; and over
it solve_swarm, the whole solve of the population solvers with a 4-word improvement log (particle_swarm, cuckoo_search,
flower_pollination, gravitational_search)."""
import ctypes as C

import numpy as np


def vp(a):
    """a numpy array (or None) as a void pointer argument"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def swap_cities(tour, frm, to):
    """route.rs:102-113: positions from..=to of the open path reversed; returns the new tour"""
    t = np.array(tour, copy=True)
    t[frm:to + 1] = t[frm:to + 1][::-1]
    return t


def start_tour(problem, init_pos):
    """the tour a chain starts from: the given positions, or city order"""
    return np.arange(len(problem), dtype=np.uint32) if init_pos is None else np.array(init_pos, dtype=np.uint32)


def bits_to_f32(bits):
    """the f32 a trace record carries as a u32"""
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def solve_chains(problem, progress_tx, chains, population, single, trace, replay):
    """chains > 1: population(chains, outs, costs, moves, best, st) runs them at once and the best one (lowest cost, then lowest
    chain) is returned; with a channel that chain runs once more, alone, for its trace.  Else single(out, cost, st), or with a
    channel trace(0).  trace(chain) -> (out, cost, log, stats dict); replay(log) sends the reference's messages."""
    from . import Solution
    from .. import _capi
    n = len(problem)
    st = _capi.TlStats()
    if chains > 1:
        outs = np.empty((chains, n), dtype=np.uint32)
        costs = np.empty(chains, dtype=np.float32)
        moves = np.zeros(chains, dtype=np.uint32)
        best = C.c_uint32()
        population(chains, outs, costs, moves, best, st)
        chain = int(best.value)
        stats = dict(st.as_dict(), moves=int(moves[chain]), chain=chain)
        if progress_tx is not None:
            replay(trace(chain)[2])
        return Solution(float(costs[chain]), problem.ids[outs[chain]], problem, stats)
    if progress_tx is None:
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        single(out, cost, st)
        return Solution(cost.value, problem.ids[out], problem, st.as_dict())
    out, cost, log, stats = trace(0)
    replay(log)
    return Solution(cost, problem.ids[out], problem, stats)


def solve_swarm(problem, progress_tx, init_tour, ctx, seed, runs, epochs, o, single_fn, trace_fn, population_fn, trace_tail=(None, 0)):
    """solve_chains over the three entries of one population solver: single_fn, trace_fn, population_fn of the library, `o` its opts
    struct, trace_tail the arguments of trace_fn behind the route log (no epoch log).  The trace's log (epoch, who, cost bits,
    route index) and routes grow until they hold every improvement; the replay is the reference's: PathUpdate(start best), per
    epoch its improvements in order and EpochUpdate(epoch), then Done.  The stats name the run "run"."""
    from .. import _capi
    n = len(problem)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    head = (ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos))

    def population(count, outs, costs, moves, best, st):
        ctx.check(population_fn(*head, 0 if init_pos is None else 1, 0, count, C.byref(o), seed, vp(outs), vp(costs), vp(moves), C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(single_fn(*head, C.byref(o), seed, vp(out), C.byref(cost), C.byref(st)))

    def trace(run):
        # the improvements are few but not known in advance: read the count first
        out = np.empty(n, dtype=np.uint32)
        cost, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
        cap = 64
        while True:
            log = np.empty((cap, 4), dtype=np.uint32)
            routes = np.empty((cap, max(n, 1)), dtype=np.uint32)
            ctx.check(trace_fn(*head, C.byref(o), seed, run, vp(out), C.byref(cost), C.byref(st), vp(log), cap, C.byref(ln), vp(routes), cap, *trace_tail))
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
