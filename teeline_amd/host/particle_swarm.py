"""particle_swarm::solve — mirror of src/tsp/particle_swarm.rs:22-129 over tl_particle_swarm.

The algorithm is the reference's discrete particle swarm, quirks included (max(n_nearest, 30) particles, gbest the first minimum,
both swap sequences from the same position, keeps clamped by `take`, truncation after concatenation, gbest updated at once within
an epoch).  Two things are this project's specification instead: the random draws are a pure function of (seed, run, epoch,
particle, role) — the reference's thread RNG is unseeded — and f64::round is spelled out (include/teeline_gpu.h).
"""
from . import HeuristicOptions
from ._chains import solve_swarm


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, runs=1):
    """opts: HeuristicOptions (epochs, n_nearest).  progress_tx: optional callable(kind, payload).  The reference sends
    PathUpdate(start gbest, its cost), per epoch a PathUpdate per gbest improvement in particle order and EpochUpdate(epoch), then
    Done (particle_swarm.rs:72-74,114-127); with a channel the solve goes through tl_particle_swarm_trace and the sequence is
    replayed from its log.  runs > 1: runs 0 .. runs-1 of `seed` at once (tl_particle_swarm_population), the best one (lowest cost,
    then lowest run) returned; the replay is of that run."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or HeuristicOptions()
    epochs = int(opts.epochs)
    o = _capi.TlPsoOpts(epochs, int(opts.n_nearest))
    lib = ctx.lib
    return solve_swarm(problem, progress_tx, init_tour, ctx, seed, runs, epochs, o, lib.tl_particle_swarm, lib.tl_particle_swarm_trace, lib.tl_particle_swarm_population, (None, 0))
