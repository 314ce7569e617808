"""gravitational_search::solve — mirror of src/tsp/gravitational_search.rs:23-145 over tl_gravitational_search.

The algorithm is the reference's gravitational search, quirks included (max(n_nearest, 25) agents, gbest the first minimum, the
masses and the ranking of an epoch from the costs at its start, no inertia, every pull from the positions as they stand, truncation
after concatenation, gbest updated at once within an epoch).  Three things are this project's specification instead: the random
draws are a pure function of (seed, run, epoch, agent, pulling agent) — the reference's thread RNG is unseeded —, equal masses
rank in ascending agent index — the reference's unstable sort leaves their order open — and exp is a fixed f64 sequence
(include/teeline_gpu.h).
"""
from . import HeuristicOptions
from ._chains import solve_swarm


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
    epochs = int(opts.epochs)
    o = _capi.TlGsaOpts(epochs, int(opts.n_nearest), 0)
    lib = ctx.lib
    return solve_swarm(problem, progress_tx, init_tour, ctx, seed, runs, epochs, o, lib.tl_gravitational_search, lib.tl_gravitational_search_trace, lib.tl_gravitational_search_population, (None, 0))
