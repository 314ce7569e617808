"""cuckoo_search::solve — mirror of src/tsp/cuckoo_search.rs:26-136 over tl_cuckoo_search.

The algorithm is the reference's cuckoo search, quirks included (max(n_nearest, 25) nests, pa clamped to [0.01, 0.99], best a copy
of the first minimum nest, a flight from the nest as it stands, the target drawn after the flight, strict acceptance, unconditional
abandonment).  Two things are this project's specification instead: the random draws are a pure function of (seed, run, epoch,
cuckoo, role) — the reference's thread RNG is unseeded — and the Lévy step is a fixed sequence of f64 operations
(include/teeline_gpu.h).
"""
import numpy as np

from . import HeuristicOptions
from ._chains import solve_swarm


class CSOptions:
    """CSOptions (src/tsp/mod.rs:913-940)"""

    def __init__(self, heuristic=None, mutation_probability=0.001, **kw):
        self.heuristic = heuristic or HeuristicOptions(**kw)
        self.mutation_probability = float(mutation_probability)

    def validate(self):
        p = self.mutation_probability
        if not (np.isfinite(p) and 0.0 <= p <= 1.0):
            raise ValueError(f"mutation_probability must be in [0, 1] (got {p})")


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, runs=1):
    """opts: CSOptions (or HeuristicOptions: the default mutation_probability).  progress_tx: optional callable(kind, payload).  The
    reference sends PathUpdate(start best, its cost), per epoch a PathUpdate per best improvement in the order they happen and
    EpochUpdate(epoch), then Done (cuckoo_search.rs:73-75,98-100,120-134); with a channel the solve goes through
    tl_cuckoo_search_trace and the sequence is replayed from its log.  runs > 1: runs 0 .. runs-1 of `seed` at once
    (tl_cuckoo_search_population), the best one (lowest cost, then lowest run) returned; the replay is of that run."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or CSOptions()
    if isinstance(opts, HeuristicOptions):
        opts = CSOptions(opts)
    opts.validate()
    epochs = int(opts.heuristic.epochs)
    o = _capi.TlCsOpts(epochs, int(opts.heuristic.n_nearest), opts.mutation_probability)
    lib = ctx.lib
    return solve_swarm(problem, progress_tx, init_tour, ctx, seed, runs, epochs, o, lib.tl_cuckoo_search, lib.tl_cuckoo_search_trace, lib.tl_cuckoo_search_population, (None, 0))
