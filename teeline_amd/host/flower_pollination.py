"""flower_pollination::solve — mirror of src/tsp/flower_pollination.rs:53-151 over tl_flower_pollination.

The algorithm is the reference's flower pollination, quirks included (max(n_nearest, 25) flowers, switch_prob 0.8 where
mutation_probability is below 0.01, gbest a copy of the first minimum flower, a global move along a prefix of the swap sequence to
gbest, a local one along a prefix of the sequence between two other flowers as they stand, strict acceptance, gbest updated at
once).  Two things are this project's specification instead: the random draws are a pure function of (seed, run, epoch, flower,
role) — the reference's thread RNG is unseeded — and the Lévy step is a fixed sequence of f64 operations (include/teeline_gpu.h,
DESIGN.md §4.22).
"""
import numpy as np

from . import HeuristicOptions
from ._chains import solve_swarm


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
    epochs = int(opts.heuristic.epochs)
    o = _capi.TlFpaOpts(epochs, int(opts.heuristic.n_nearest), opts.mutation_probability)
    lib = ctx.lib
    return solve_swarm(problem, progress_tx, init_tour, ctx, seed, runs, epochs, o, lib.tl_flower_pollination, lib.tl_flower_pollination_trace, lib.tl_flower_pollination_population, (None, 0))
