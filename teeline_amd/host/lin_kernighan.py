"""lin_kernighan::solve — mirror of src/tsp/lin_kernighan.rs:35-100 over tl_lk."""
import ctypes as C

import numpy as np


class _Lists:
    """`candidates=` of a solve: the context searches these rows for the length of the call, then has again the lists it was found
    with (those set through Context.lk_candidates, or none)."""

    def __init__(self, ctx, rows):
        self.ctx, self.rows, self.before = ctx, rows, None

    def __enter__(self):
        if self.rows is not None:
            self.before = self.ctx.lk_candidates_set()
            self.ctx.lk_candidates(self.rows)

    def __exit__(self, *exc):
        if self.rows is not None:
            self.ctx.lk_candidates(self.before)
        return False


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, seed=1, candidates=None):
    """candidates: n x k POSITIONS (e.g. alpha_candidates.candidates(problem, k, pi).rows) searched instead of the kd-tree's lists
    (tl_lk_candidates for the length of this call; opts.heuristic.n_nearest is then ignored, the width is k).
    progress_tx: optional callable(kind, payload) — the reference's mpsc::Sender<ProgressMessage>.  The reference sends
    PathUpdate(best_tour, best_dist) after the first lk_pass and after every epoch that improves on it, and no Done
    (lin_kernighan.rs:71,90; nothing when n < 4, :57-59).  With a channel the solve goes through tl_lk_live: the device-side state
    machine files exactly those tours and distances and the host hands them on while the search runs (tl_lk_trace lists the same
    ones after the fact)."""
    from . import LKOptions, Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    opts = opts or LKOptions()
    opts.validate()
    n = len(problem)
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    o = _capi.TlLkOpts(opts.heuristic.epochs, opts.heuristic.platoo_epochs, opts.heuristic.n_nearest, opts.max_depth)
    out = np.empty(n, dtype=np.uint32)
    cost = C.c_float()
    st = _capi.TlStats()
    # GEO / EXPLICIT problems: the search is Euclidean over the city coordinates (lin_kernighan.rs:41 rebuilds its own
    # matrix), but the NN seed (:47-55) and the reported total (:99) go through problem.distances
    packed = problem.explicit_packed()
    args = (ctx.handle, problem.xy.ctypes.data_as(C.c_void_p), n,
            None if packed is None else packed.ctypes.data_as(C.c_void_p),
            None if init_pos is None else init_pos.ctypes.data_as(C.c_void_p), C.byref(o), int(seed),
            out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(st))
    if progress_tx is None or n < 4:
        with _Lists(ctx, candidates):
            ctx.check(ctx.lib.tl_lk(*args))
    else:
        # with a channel: tl_lk_live calls back WHILE the device-side search runs (between two polls of its state machine), once
        # per best tour the ILS settles on, in order — the messages arrive as the reference's would, not after the solve
        err = []

        def on_best(_user, pos, nn, best_dist):
            try:
                progress_tx("PathUpdate", ([int(v) for v in problem.ids[np.ctypeslib.as_array(pos, shape=(nn,))]], float(best_dist)))
            except BaseException as exc:  # an exception must not unwind through the C frames
                err.append(exc)

        cb = _capi.LK_PROGRESS_FN(on_best)
        with _Lists(ctx, candidates):
            ctx.check(ctx.lib.tl_lk_live(*args, cb, None))
        if err:
            raise err[0]
    return Solution(cost.value, problem.ids[out], problem, st.as_dict())


def build_candidates(problem, k, *, ctx=None):
    """lin_kernighan::build_candidates (lin_kernighan.rs:12-27) in POSITIONS: n x min(k, n-1) array."""
    from . import default_context
    ctx = ctx or default_context()
    n = len(problem)
    kk = min(int(k), n - 1)
    out = np.empty((n, max(kk, 1)), dtype=np.uint32)
    ctx.check(ctx.lib.tl_build_candidates(ctx.handle, problem.xy.ctypes.data_as(C.c_void_p), n, int(k),
                                          out.ctypes.data_as(C.c_void_p)))
    return out[:, :kk]


def _lk_opts(opts):
    from .. import _capi
    return _capi.TlLkOpts(opts.heuristic.epochs, opts.heuristic.platoo_epochs, opts.heuristic.n_nearest, opts.max_depth)


def run_seed(seed, run):
    """tl_lk_run_seed: the seed of run `run` of a population seeded `seed` — run 0 the seed itself, run r >= 1 output 2^63 + r of the
    seed's splitmix64 stream (the kicks of a search draw below 2^35 of theirs)."""
    from .. import _capi
    return int(_capi.load().tl_lk_run_seed(int(seed) & (2**64 - 1), int(run)))


def population_plan(n, opts=None, runs=2, *, cus=256, lds_bytes=163840, force_form=-1):
    """tl_lk_population_plan (host-only): {"form": 1 one workgroup per run / 0 the loop over tl_lk, "threads", "per_cu"} for `runs` runs
    of n cities on a device with `cus` compute units and `lds_bytes` of LDS per workgroup."""
    from . import TeelineGpuError
    from .. import _capi
    f, t, p = C.c_int(), C.c_int(), C.c_uint32()
    rc = _capi.load().tl_lk_population_plan(int(n), None if opts is None else C.byref(_lk_opts(opts)), int(runs), int(cus), int(lds_bytes),
                                            int(force_form), C.byref(f), C.byref(t), C.byref(p))
    if rc:
        raise TeelineGpuError(rc, "tl_lk_population_plan: cus < 1, lds_bytes < 0, force_form outside -1..1 or options out of range")
    return {"form": f.value, "threads": t.value, "per_cu": p.value}


def solve_population(problem, opts=None, init_tours=None, *, seed, runs, first_run=0, ctx=None, candidates=None):
    """candidates: as in solve — the lists every run searches.
    Seeded runs first_run .. first_run + runs - 1 of lin_kernighan::solve at once (tl_lk_population): run r is solve(...,
    seed=run_seed(seed, r)), run 0 the plain seed's.  init_tours: None (the NN seed solve would build), one tour of city ids for all
    runs, or `runs` of them.  Returns (solutions, best): one Solution per run with that run's own counters in its stats (the call's
    times), and the index of the cheapest (equal totals: the lowest run)."""
    from . import LKOptions, Solution, TeelineGpuError, default_context
    from .. import _capi
    runs = int(runs)
    if runs < 1:
        raise TeelineGpuError(_capi.TL_ERR_BADARG, f"lin_kernighan.solve_population: runs={runs} < 1")
    if init_tours is not None and len(init_tours) not in (1, runs):
        raise TeelineGpuError(_capi.TL_ERR_BADARG, f"lin_kernighan.solve_population: {len(init_tours)} start tours for {runs} runs (one, or one per run)")
    n = len(problem)
    for k, tour in enumerate(init_tours or ()):  # the library reads rows of n u32 values: checked before any pointer is taken
        if len(tour) != n:
            raise TeelineGpuError(_capi.TL_ERR_BADARG, f"tour {k} has {len(tour)} cities, the problem {n}")
    opts = opts or LKOptions()
    opts.validate()
    ctx = ctx or default_context()
    init = None if init_tours is None else np.ascontiguousarray([problem.positions_of(t) for t in init_tours], dtype=np.uint32)
    o = _lk_opts(opts)
    out = np.empty((runs, n), dtype=np.uint32)
    costs = np.empty(runs, dtype=np.float32)
    cnt = np.zeros((runs, 4), dtype=np.uint64)
    best = C.c_uint32()
    st = _capi.TlStats()
    packed = problem.explicit_packed()
    with _Lists(ctx, candidates):
        ctx.check(ctx.lib.tl_lk_population(ctx.handle, problem.xy.ctypes.data_as(C.c_void_p), n,
                                           None if packed is None else packed.ctypes.data_as(C.c_void_p),
                                           None if init is None else init.ctypes.data_as(C.c_void_p), 0 if init is None else len(init),
                                           int(first_run), runs, C.byref(o), int(seed) & (2**64 - 1), out.ctypes.data_as(C.c_void_p),
                                           costs.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(best), C.byref(st)))
    stats = st.as_dict()
    sols = [Solution(float(costs[r]), problem.ids[out[r]], problem,
                     dict(stats, sweeps=int(cnt[r, 0]), candidates=int(cnt[r, 1]), moves=int(cnt[r, 2]), reversed=int(cnt[r, 3]))) for r in range(runs)]
    return sols, int(best.value)
