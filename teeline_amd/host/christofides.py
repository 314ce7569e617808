"""christofides::solve — mirror of src/tsp/christofides.rs:12-68 on tl_christofides."""
import ctypes as C

import numpy as np


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None):
    """opts and init_tour are ignored like the reference's `_opts` / `_init_tour` (christofides.rs:14,16).  progress_tx: optional
    callable(kind, payload) receiving the reference's messages (:24-65): n < 4 sends Done alone; otherwise PathUpdate(the city
    ids in file order, 0.0) — the placeholder after the tree — then PathUpdate(route, total) and Done.
    stats: sweeps = bands of sorted pairs, candidates = pairs the matching examined, prim_ms = the tree's launch."""
    from . import Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    packed = problem.explicit_packed()  # GEO / EXPLICIT: every distance is the packed matrix's (distance_by_pos, :102-104, :147-149)
    n = len(problem)
    out = np.empty(max(n, 1), dtype=np.uint32)
    cost = C.c_float()
    st = _capi.TlStats()
    ctx.check(ctx.lib.tl_christofides(ctx.handle, problem.xy.ctypes.data_as(C.c_void_p),
                                      None if packed is None else packed.ctypes.data_as(C.c_void_p), n,
                                      out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(st)))
    route = problem.ids[out[:n]]
    if progress_tx is not None:
        path = [int(v) for v in route]
        if n >= 4:
            progress_tx("PathUpdate", ([int(v) for v in problem.ids], 0.0))
            progress_tx("PathUpdate", (path, float(np.float32(cost.value))))
        progress_tx("Done", None)
    stats = st.as_dict()
    stats["prim_ms"] = stats.pop("reversed") / 1e6
    return Solution(cost.value, route, problem, stats)
