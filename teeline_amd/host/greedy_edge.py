"""greedy_edge::solve — mirror of src/tsp/greedy_edge.rs:21-65 (over graph.rs:54-196) on tl_greedy_edge."""
import ctypes as C

import numpy as np


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None):
    """opts and init_tour are ignored like the reference's `_opts` / `_init_tour` (greedy_edge.rs:23,25).  progress_tx: optional
    callable(kind, payload) receiving the reference's messages (replay_progress)."""
    from . import Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    packed = problem.explicit_packed()  # GEO / EXPLICIT: the edges are the packed matrix's (distance_by_pos, graph.rs:62-68)
    n = len(problem)
    out = np.empty(max(n, 1), dtype=np.uint32)
    cost = C.c_float()
    st = _capi.TlStats()
    ctx.check(ctx.lib.tl_greedy_edge(ctx.handle, problem.xy.ctypes.data_as(C.c_void_p),
                                     None if packed is None else packed.ctypes.data_as(C.c_void_p), n,
                                     out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(st)))
    route = problem.ids[out[:n]]
    if progress_tx is not None:
        replay_progress(problem.ids, route, np.float32(cost.value), progress_tx)
    return Solution(cost.value, route, problem, st.as_dict())


def replay_progress(ids, route, total, progress_tx):
    """greedy_edge.rs:33-62: n <= 2 sends Done alone; otherwise PathUpdate(identity, 0.0) before the selection — the city ids in
    file order — then PathUpdate(path, tour_length(path)) and Done."""
    path = [int(v) for v in route]
    if len(path) > 2:
        progress_tx("PathUpdate", ([int(v) for v in ids], 0.0))
        progress_tx("PathUpdate", (path, float(total)))
    progress_tx("Done", None)
