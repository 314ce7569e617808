"""stochastic_hill::solve — mirror of src/tsp/stochastic_hill.rs:7-97 over tl_hill_climb.

The chain is the reference's, quirks included (a candidate of the current tour is accepted iff it beats the BEST cost; the plateau
restart shuffles the current tour and leaves the best alone, so a restart rarely helps; `epochs + 1` epochs run; the best route is
returned).  One thing is this project's specification instead: the random draws are a pure function of (seed, chain, event, slot) —
the reference's thread RNG is unseeded (include/teeline_gpu.h).  The solver goes by the name `hill_climb`.
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, solve_chains, start_tour, swap_cities, vp

RESTART = 0xFFFFFFFF      # the `from` word of a restart's trace record
SHUFFLE_EVENT = 1 << 58   # csrc/hill_spec.h: the restart after epoch e draws on the events 2^58 + e n + j, slot 26
SHUFFLE_SLOT = 26


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, seed=1, chains=1, window=0, ctx=None):
    """progress_tx: optional callable(kind, payload).  The reference sends PathUpdate(start route, 0.0), PathUpdate(best, distance) per
    acceptance, PathUpdate(shuffled current route, 0.0) per restart and Done (stochastic_hill.rs:29-31,51-56,75-77,93-95); with a
    channel the solve goes through tl_hill_climb_trace and the sequence is replayed from the event log, the shuffles through
    tl_hill_draw.  init_tour None: city order (the reference's own shuffle is the pipeline's `shuffle` step).  chains > 1: chains
    0 .. chains-1 of `seed` run at once (tl_hill_climb_population) and the best one (lowest cost, then lowest chain) is returned; the
    replay is of that chain.  window: epochs evaluated at once (0: the plan's; 1: epoch after epoch) — the same result."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or HeuristicOptions()
    n = len(problem)
    o = _capi.TlHillOpts(int(opts.epochs), int(opts.platoo_epochs), int(window), 0)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    lib, inst = ctx.lib, (ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos))

    def population(chains, outs, costs, moves, best, st):
        ctx.check(lib.tl_hill_climb_population(*inst, 0 if init_pos is None else 1, 0, chains, C.byref(o), seed, vp(outs), vp(costs), vp(moves),
                                               C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(lib.tl_hill_climb(*inst, C.byref(o), seed, vp(out), C.byref(cost), C.byref(st)))

    traced = []

    def trace(chain):
        """Chain `chain` of `seed` alone, with its events (tl_hill_climb_trace_chain; chain 0 is tl_hill_climb_trace)."""
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        st = _capi.TlStats()
        cap = 1 << 14
        while True:
            log = np.empty((cap, 4), dtype=np.uint32)
            ln = C.c_uint32()
            ctx.check(lib.tl_hill_climb_trace_chain(*inst, C.byref(o), seed, chain, vp(out), C.byref(cost), C.byref(st), vp(log), cap, C.byref(ln)))
            if ln.value <= cap:
                traced.append(chain)
                return out, cost.value, log[:ln.value], st.as_dict()
            cap = int(ln.value)  # deterministic: once more with room for every event

    return solve_chains(problem, progress_tx, chains, population, single, trace,
                        lambda log: replay_progress(problem, init_pos, log, progress_tx, seed=seed, chain=traced[-1], lib=lib))


def shuffle(lib, seed, chain, epoch, tour):
    """The restart after epoch `epoch` (csrc/hill_spec.h): Fisher-Yates on the current contents; returns the new tour"""
    t = np.array(tour, copy=True)
    n = len(t)
    for j in range(n - 1, 0, -1):
        u = lib.tl_hill_draw(seed, chain, SHUFFLE_EVENT + epoch * n + j, SHUFFLE_SLOT)
        p = ((u >> 32) * (j + 1)) >> 32
        t[j], t[p] = t[p], t[j]
    return t


def replay_progress(problem, init_pos, log, progress_tx, *, seed, chain, lib):
    """The reference's message stream (stochastic_hill.rs:29-95) from the events of tl_hill_climb_trace."""
    tour = start_tour(problem, init_pos)
    ids = problem.ids
    progress_tx("PathUpdate", ([int(v) for v in ids[tour]], 0.0))
    for epoch, frm, to, bits in np.asarray(log, dtype=np.uint32).reshape(-1, 4):
        if int(frm) == RESTART:
            tour = shuffle(lib, seed, chain, int(epoch), tour)
            progress_tx("PathUpdate", ([int(v) for v in ids[tour]], 0.0))
        else:
            tour = swap_cities(tour, int(frm), int(to))
            progress_tx("PathUpdate", ([int(v) for v in ids[tour]], float(bits_to_f32(bits))))
    progress_tx("Done", None)
    return tour
