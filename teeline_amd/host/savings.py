"""savings::solve — mirror of src/tsp/savings.rs:34-82 (over graph.rs:98-196) on tl_savings."""
import ctypes as C

import numpy as np

from .greedy_edge import replay_progress


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None):
    """opts and init_tour are ignored like the reference's `_opts` / `_init_tour` (savings.rs:36,38).  progress_tx: optional
    callable(kind, payload) receiving the reference's messages (savings.rs:46-79: greedy_edge.replay_progress's three).  The hub is
    the position nearest the coordinates' centroid (tl_savings_hub), also for GEO / EXPLICIT problems; stats["hub"] reports it."""
    from . import Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    packed = problem.explicit_packed()  # GEO / EXPLICIT: the edges are the packed matrix's (distance_by_pos, savings.rs:144-152)
    n = len(problem)
    out = np.empty(max(n, 1), dtype=np.uint32)
    cost, hub = C.c_float(), C.c_uint32()
    st = _capi.TlStats()
    ctx.check(ctx.lib.tl_savings(ctx.handle, problem.xy.ctypes.data_as(C.c_void_p),
                                 None if packed is None else packed.ctypes.data_as(C.c_void_p), n, _capi.TL_SAVINGS_HUB_AUTO,
                                 out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(hub), C.byref(st)))
    route = problem.ids[out[:n]]
    if progress_tx is not None:
        replay_progress(problem.ids, route, np.float32(cost.value), progress_tx)
    return Solution(cost.value, route, problem, dict(st.as_dict(), hub=int(hub.value)))
