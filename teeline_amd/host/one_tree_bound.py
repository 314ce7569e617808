"""The Held-Karp lower bound over tl_one_tree_bound: the minimum 1-tree under node penalties, raised by subgradient ascent.

Not a solver and not the reference's (the reference computes no bound): this project's own specification, DESIGN.md §4.29.  The
result bounds the length of EVERY tour from below under the same f32 distances, so `gap_pct(cost)` says how far a tour can be from
the optimum at most.  Where the 1-tree is itself a tour the bound is the optimum and `route` is that tour.

    bound(problem, upper)                one job
    bound_batch(problem, upper, sets)    one job per option set (dicts of root / iterations / lambda0 / patience), all at once
    bound_host(problem, upper)           the sequential restatement on the CPU: no context, no device
"""
import ctypes as C

import numpy as np

from ._chains import vp

STOP_NAMES = {0: "trivial", 1: "tour", 2: "lambda", 3: "upper", 4: "iterations"}


def gap_pct_of(cost, bound):
    """100 (cost - bound) / bound: how far above the optimum a tour of this cost can be at most, in percent."""
    return 100.0 * (float(cost) - float(bound)) / float(bound)


class Bound:
    """bound (f64), pi (the best penalties), is_tour, route (city ids where the 1-tree was a tour, else None), stats, log (rows of
    L_k, sum g^2, lambda), upper (the tour length the ascent aimed at) and upper_route (the tour it came from, where the mirror made it)."""

    def __init__(self, bound, pi, is_tour, route, stats, log, upper, upper_route=None, parent=None):
        self.bound, self.pi, self.is_tour, self.route, self.stats, self.log = float(bound), pi, bool(is_tour), route, stats, log
        self.upper, self.upper_route, self.parent = float(upper), upper_route, parent

    def gap_pct(self, cost):
        return gap_pct_of(cost, self.bound)


def _c_opts(upper, root=0, iterations=1000, lambda0=2.0, patience=10, iters_per_launch=0):
    from .. import _capi
    return _capi.TlOneTreeOpts(int(root), int(iterations), int(patience), int(iters_per_launch), float(lambda0), float(upper), 0)


def upper_from_solvers(problem, ctx=None):
    """A tour by the existing nearest_neighbor -> two_opt solvers: (its f32 cost as a float, its route)."""
    from . import nearest_neighbor, two_opt
    seed = nearest_neighbor.solve(problem, ctx=ctx)
    if len(problem) < 4:
        return float(seed.total), seed.route()
    sol = two_opt.solve(problem, None, None, seed.route(), ctx=ctx)
    return float(sol.total), sol.route()


def _results(problem, n, J, res, pi, par, tour, log, log_cap, upper, upper_route, st=None):
    out = []
    for j in range(J):
        r = res[j].as_dict()
        stats = dict(st.as_dict() if st is not None else {}, job=j, stop_name=STOP_NAMES.get(r["stop"], "?"), **r)
        rows = [tuple(float(v) for v in log[j, k]) for k in range(min(r["iterations_run"], log_cap))]
        route = [int(v) for v in problem.ids[tour[j, :n]]] if r["is_tour"] else None
        out.append(Bound(r["bound"], pi[j, :n].copy(), r["is_tour"], route, stats, rows, upper, upper_route, par[j, :n].copy()))
    return out


def bound_batch(problem, upper, option_sets, *, ctx=None, iters_per_launch=0, log_cap=0, return_all=False):
    """option_sets: dicts with any of root, iterations, lambda0, patience; one workgroup each (tl_one_tree_bound_batch).  Returns the
    Bound of the first job with the largest bound (stats["job"] names it, stats["bounds"] lists every job's); return_all: every job's."""
    from . import default_context
    from .. import _capi
    ctx = ctx or default_context()
    option_sets = list(option_sets)
    if not option_sets:
        raise ValueError("one_tree_bound: no option set")
    upper_route = None
    if upper is None:
        upper, upper_route = upper_from_solvers(problem, ctx)
    n, J = len(problem), len(option_sets)
    arr = (_capi.TlOneTreeOpts * J)(*[_c_opts(upper, iters_per_launch=iters_per_launch, **o) for o in option_sets])
    res = (_capi.TlOneTreeResult * J)()
    pi, par, tour = np.zeros((J, max(n, 1))), np.zeros((J, max(n, 1)), dtype=np.uint32), np.zeros((J, max(n, 1)), dtype=np.uint32)
    log = np.zeros((J, max(log_cap, 1), 3))
    best, st = C.c_uint32(), _capi.TlStats()
    ctx.check(ctx.lib.tl_one_tree_bound_batch(ctx.handle, vp(problem.xy), vp(problem.explicit_packed()), n, arr, J, res, vp(pi), vp(par), vp(tour),
                                              vp(log) if log_cap else None, int(log_cap), C.byref(best), C.byref(st)))
    out = _results(problem, n, J, res, pi, par, tour, log, log_cap, upper, upper_route, st)
    if return_all:
        return out
    b = out[int(best.value)]
    b.stats["bounds"] = [o.bound for o in out]
    return b


def bound(problem, upper=None, *, root=0, iterations=1000, lambda0=2.0, patience=10, ctx=None, iters_per_launch=0, log_cap=0):
    """upper: the length of any tour (it scales the step); None: the mirror takes a nearest_neighbor -> two_opt tour and reports it as
    upper_route."""
    return bound_batch(problem, upper, [dict(root=root, iterations=iterations, lambda0=lambda0, patience=patience)], ctx=ctx,
                       iters_per_launch=iters_per_launch, log_cap=log_cap)


def bound_host(problem, upper, *, root=0, iterations=1000, lambda0=2.0, patience=10, log_cap=0):
    """tl_one_tree_bound_host: the same contract on the CPU.  upper is required: no solver runs without a device."""
    from .. import _capi
    lib = _capi.load()
    n = len(problem)
    o = _c_opts(upper, root, iterations, lambda0, patience)
    res = (_capi.TlOneTreeResult * 1)()
    pi, par, tour = np.zeros((1, max(n, 1))), np.zeros((1, max(n, 1)), dtype=np.uint32), np.zeros((1, max(n, 1)), dtype=np.uint32)
    log = np.zeros((1, max(log_cap, 1), 3))
    rc = lib.tl_one_tree_bound_host(vp(problem.xy), vp(problem.explicit_packed()), n, C.byref(o), res, vp(pi), vp(par), vp(tour),
                                    vp(log) if log_cap else None, int(log_cap))
    if rc != _capi.TL_OK:
        raise _capi.TeelineGpuError(rc, lib.tl_last_error(None).decode())
    return _results(problem, n, 1, res, pi, par, tour, log, log_cap, upper, None)[0]
