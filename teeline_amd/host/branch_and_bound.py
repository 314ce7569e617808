"""branch_and_bound::solve — the depth-first branch and bound of DESIGN.md §4.27 on tl_branch_and_bound (exact, n <= 64).

The bound is the reference's (src/tsp/branch_bound.rs:240-268); the result is this project's specification — the least tour by
(tour_length, positions) among those that start at the smallest id — because the reference's own depends on a HashSet's iteration
order.  The reference's name `branch_bound` stays refused."""
import ctypes as C

import numpy as np


def _call(fn, head, problem, opts, init_tour, max_nodes, time_limit_ms, launch):
    from .. import _capi
    n = len(problem)
    packed = problem.explicit_packed()
    init_pos = problem.positions_of(init_tour) if init_tour is not None else None
    start = int(np.argmin(problem.ids)) if n else 0  # route.sort() (:35): the search starts at the smallest id
    o = _capi.TlBnbOpts(start, 0 if opts is None else int(opts.n_nearest), int(max_nodes), int(time_limit_ms),
                        int(launch.get("nodes_per_launch", 0)), int(launch.get("frontier_depth", 0)), int(launch.get("workgroups", 0)))
    out = np.empty(max(n, 1), dtype=np.uint32)
    cost, proved, improved = C.c_float(), C.c_uint32(), C.c_uint32()
    st = _capi.TlBnbStats()
    rc = fn(*head, problem.xy.ctypes.data_as(C.c_void_p), None if packed is None else packed.ctypes.data_as(C.c_void_p), n,
            None if init_pos is None else init_pos.ctypes.data_as(C.c_void_p), C.byref(o), out.ctypes.data_as(C.c_void_p), C.byref(cost),
            C.byref(proved), C.byref(improved), C.byref(st))
    stats = st.as_dict()
    stats["proved"], stats["improved"] = int(proved.value), int(improved.value)
    return rc, out[:n], cost.value, stats


def _finish(problem, out, cost, stats, progress_tx):
    from . import Solution
    route = problem.ids[out]
    if progress_tx is not None:  # (:36-38, :78-80; the per-move messages of the reference's search are not reproduced)
        progress_tx("PathUpdate", (sorted(int(v) for v in problem.ids), 0.0))
        progress_tx("PathUpdate", ([int(v) for v in route], float(np.float32(cost))))
        progress_tx("Done", None)
    return Solution(cost, route, problem, stats)


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, max_nodes=0, time_limit_ms=0, **launch):
    """opts None: the exact solver.  A HeuristicOptions passes its n_nearest = K as the reference reads it (:52-60): with 0 < K < n
    a city is followed by one of its K nearest (itself counted) wherever one is unvisited — a heuristic.  init_tour (city ids): the
    start tour; it comes back as given unless a strictly shorter tour exists (:84-90).  max_nodes / time_limit_ms: budgets (0:
    none), checked between launches; stats["proved"] is 0 when one of them ended the search.  launch: nodes_per_launch,
    frontier_depth, workgroups (0 or absent: the plan's) — a proved result does not depend on them.
    stats: proved, improved, nodes, leaves, launches, queue_start, queue_end, wave_launches, idle_wave_launches, kernel_ms, ..."""
    from . import default_context
    ctx = ctx or default_context()
    rc, out, cost, stats = _call(ctx.lib.tl_branch_and_bound, (ctx.handle,), problem, opts, init_tour, max_nodes, time_limit_ms, launch)
    ctx.check(rc)
    return _finish(problem, out, cost, stats, progress_tx)


def solve_host(problem, opts=None, progress_tx=None, init_tour=None, *, max_nodes=0, time_limit_ms=0):
    """The sequential restatement on the CPU (tl_branch_and_bound_host): the same contract, no device."""
    from .. import _capi
    lib = _capi.load()
    rc, out, cost, stats = _call(lib.tl_branch_and_bound_host, (), problem, opts, init_tour, max_nodes, time_limit_ms, {})
    if rc != _capi.TL_OK:
        raise _capi.TeelineGpuError(rc, lib.tl_last_error(None).decode())
    return _finish(problem, out, cost, stats, progress_tx)
