"""tabu_search::solve — mirror of src/tsp/tabu_search.rs:9-110 over tl_tabu_search.

The chain is the reference's, quirks included (the list of n whole routes receives the start tour twice; candidate n of an epoch is
taken unchecked; `epochs + 1` epochs run; the best route seen is returned).  One thing is this project's specification instead: the
random draws are a pure function of (seed, chain, epoch, attempt, slot) — the reference's thread RNG is unseeded (include/teeline_gpu.h,
DESIGN.md §4.16).
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, solve_chains, start_tour, swap_cities, vp


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, seed=1, chains=1, ctx=None):
    """progress_tx: optional callable(kind, payload).  The reference sends PathUpdate(start route, 0.0), one PathUpdate(route, distance)
    per new best and Done (tabu_search.rs:28-30,42-47,59-61); with a channel the solve goes through tl_tabu_search_trace and the
    sequence is replayed from the per-epoch (attempt, from, to, cost) log.  chains > 1: chains 0 .. chains-1 of `seed` run at once
    (tl_tabu_search_population) and the best one (lowest cost, then lowest chain) is returned; the replay is of that chain."""
    from . import default_context
    ctx = ctx or default_context()
    opts = opts or HeuristicOptions()
    n = len(problem)
    epochs = int(opts.epochs)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    lib, inst = ctx.lib, (ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos))

    def population(chains, outs, costs, moves, best, st):
        ctx.check(lib.tl_tabu_search_population(*inst, 0 if init_pos is None else 1, 0, chains, epochs, seed, vp(outs), vp(costs), vp(moves),
                                                C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(lib.tl_tabu_search(*inst, epochs, seed, vp(out), C.byref(cost), C.byref(st)))

    def trace(chain):
        """Chain `chain` of `seed` alone, with every epoch (tl_tabu_search_trace_chain; chain 0 is tl_tabu_search_trace)."""
        from .. import _capi
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        st = _capi.TlStats()
        cap = epochs + 1
        log = np.empty((cap, 4), dtype=np.uint32)
        ln = C.c_uint32()
        ctx.check(lib.tl_tabu_search_trace_chain(*inst, epochs, seed, chain, vp(out), C.byref(cost), C.byref(st), vp(log), cap, C.byref(ln)))
        return out, cost.value, log[:min(ln.value, cap)], st.as_dict()

    return solve_chains(problem, progress_tx, chains, population, single, trace, lambda log: replay_progress(problem, init_pos, log, progress_tx))


def replay_progress(problem, init_pos, log, progress_tx):
    """The reference's message stream (tabu_search.rs:28-61) from the epochs of tl_tabu_search_trace: every epoch's reversal is applied,
    and an epoch whose cost is below every earlier one (the start tour's included) is a new best."""
    from .or_opt import tour_length_f32
    tour = start_tour(problem, init_pos)
    ids = problem.ids
    progress_tx("PathUpdate", ([int(v) for v in ids[tour]], 0.0))
    best = np.float32(tour_length_f32(problem, tour))
    for _attempt, frm, to, bits in np.asarray(log, dtype=np.uint32).reshape(-1, 4):
        tour = swap_cities(tour, int(frm), int(to))
        cost = bits_to_f32(bits)
        if cost < best:
            best = cost
            progress_tx("PathUpdate", ([int(v) for v in ids[tour]], float(cost)))
    progress_tx("Done", None)
