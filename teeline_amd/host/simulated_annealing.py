"""simulated_annealing::solve — mirror of src/tsp/simulated_annealing.rs:10-83 over tl_sim_anneal.

The chain is the reference's, quirks included (the last state is returned, not the best one seen).  Two things are this project's
specification instead: the random draws are a pure function of (seed, chain, epoch, slot) — the reference's thread RNG is unseeded —
and the Metropolis criterion is a fixed f64 operation sequence instead of the platform's exp (include/teeline_gpu.h).
"""
import ctypes as C

import numpy as np

from . import HeuristicOptions
from ._chains import bits_to_f32, solve_chains, start_tour, swap_cities, vp


class SAOptions:
    """src/tsp/mod.rs:689-706"""

    def __init__(self, heuristic=None, cooling_rate=0.0001, min_temperature=0.001, max_temperature=1000.0):
        self.heuristic = heuristic or HeuristicOptions()
        self.cooling_rate, self.min_temperature, self.max_temperature = cooling_rate, min_temperature, max_temperature

    def validate(self):  # mod.rs:708-742
        self.heuristic.validate()
        c, lo, hi = (np.float32(v) for v in (self.cooling_rate, self.min_temperature, self.max_temperature))
        if c <= 0:
            raise ValueError(f"cooling_rate must be > 0 (got {c})")
        if c >= 1:
            raise ValueError(f"cooling_rate must be < 1 (got {c})")
        if hi <= 0:
            raise ValueError(f"max_temperature must be > 0 (got {hi})")
        if lo < 0:
            raise ValueError(f"min_temperature must be >= 0 (got {lo})")
        if lo >= hi:
            raise ValueError(f"min_temperature ({lo}) must be < max_temperature ({hi})")

    @classmethod
    def parse(cls, epochs=None, cooling_rate=None, min_temperature=None, max_temperature=None):
        """SAOptions::from_cli: the defaults with what was given, validated (the one place that refuses the reference's own test
        combination epochs 0 / max 0 / min 1e6, which solve() itself runs)."""
        o = cls()
        if epochs is not None:
            o.heuristic.epochs = int(epochs)
        for name, v in (("cooling_rate", cooling_rate), ("min_temperature", min_temperature), ("max_temperature", max_temperature)):
            if v is not None:
                setattr(o, name, float(v))
        o.validate()
        return o

    def as_c(self):
        from .. import _capi
        return _capi.TlSaOpts(int(self.heuristic.epochs), float(self.cooling_rate), float(self.min_temperature), float(self.max_temperature))


def schedule_epochs(opts=None):
    """The epochs `while epoch < epochs || temperature > min_temperature` runs (host only; 138 149 with the defaults)."""
    from .. import _capi
    lib = _capi.load()
    n = C.c_uint64()
    o = (opts or SAOptions()).as_c()
    rc = lib.tl_sa_schedule_epochs(C.byref(o), C.byref(n))
    if rc != _capi.TL_OK:
        raise _capi.TeelineGpuError(rc, "the schedule has more than 2^32 - 1 epochs (or never ends)")
    return int(n.value)


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, chains=1):
    """progress_tx: optional callable(kind, payload).  The reference sends PathUpdate(route, distance) for the start route, one per
    accepted epoch and Done (simulated_annealing.rs:33-38,49-54,63-65); with a channel the solve goes through tl_sim_anneal_trace and
    the sequence is replayed from the accepted (epoch, from, to, cost) list.  chains > 1: chains 0 .. chains-1 of `seed` run at once
    (tl_sim_anneal_population) and the best one (lowest cost, then lowest chain) is returned; the replay is of that chain."""
    from . import default_context
    ctx = ctx or default_context()
    opts = opts or SAOptions()
    n = len(problem)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    packed = problem.explicit_packed()
    o = opts.as_c()
    lib, inst = ctx.lib, (ctx.handle, vp(problem.xy), n, vp(packed), vp(init_pos))

    def population(chains, outs, costs, moves, best, st):
        ctx.check(lib.tl_sim_anneal_population(*inst, 0 if init_pos is None else 1, 0, chains, C.byref(o), seed, vp(outs), vp(costs), vp(moves),
                                               C.byref(best), C.byref(st)))

    def single(out, cost, st):
        ctx.check(lib.tl_sim_anneal(*inst, C.byref(o), seed, vp(out), C.byref(cost), C.byref(st)))

    def trace(chain):
        """Chain `chain` of `seed` alone, with its accepted epochs (tl_sim_anneal_trace_chain; chain 0 is tl_sim_anneal_trace)."""
        from .. import _capi
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        st = _capi.TlStats()
        cap = 1 << 14
        while True:
            log = np.empty((cap, 4), dtype=np.uint32)
            ln = C.c_uint32()
            ctx.check(lib.tl_sim_anneal_trace_chain(*inst, C.byref(o), seed, chain, vp(out), C.byref(cost), C.byref(st), vp(log), cap, C.byref(ln)))
            if ln.value <= cap:
                return out, cost.value, log[:ln.value], st.as_dict()
            cap = int(ln.value)  # deterministic: once more with room for every accepted epoch

    return solve_chains(problem, progress_tx, chains, population, single, trace, lambda log: replay_progress(problem, init_pos, log, progress_tx))


def replay_progress(problem, init_pos, log, progress_tx):
    """The reference's message stream (simulated_annealing.rs:33-65) from the accepted epochs of tl_sim_anneal_trace."""
    from .or_opt import tour_length_f32
    tour = start_tour(problem, init_pos)
    ids = problem.ids
    progress_tx("PathUpdate", ([int(v) for v in ids[tour]], float(tour_length_f32(problem, tour))))
    for _epoch, frm, to, bits in np.asarray(log, dtype=np.uint32).reshape(-1, 4):
        tour = swap_cities(tour, int(frm), int(to))
        progress_tx("PathUpdate", ([int(v) for v in ids[tour]], float(bits_to_f32(bits))))
    progress_tx("Done", None)
    return tour
