"""bellman_karp::solve — mirror of src/tsp/bellman_karp.rs:24-87 on tl_bellman_karp (the exact solver, n <= 26)."""
import ctypes as C

import numpy as np


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None, exact_walk=False):
    """opts and init_tour are ignored: the reference reads only opts.verbose (it prints the table, :61-63 — not reproduced) and
    never its `_init_tour` (:28).  progress_tx: optional callable(kind, payload) receiving the reference's messages (:48-52,
    :81-84): CityChange(id) for the n - 1 cities of the subsets in position order, PathUpdate(route, 0.0), Done.
    The route is what the reference's tolerance walk leaves (:122-156), which need NOT be a tour (stats["is_tour"] == 0; the
    pipeline's validate_tour rejects it, as the reference's does).  exact_walk=True reads the route back by exact f32 equality
    instead (TL_FLAG_BHK_EXACT_WALK, no counterpart in the reference): always a tour while a finite one exists.  The flag lives on
    the context; a context without it is replaced for this call by a temporary one on the same device.
    total is tour_length of the route; stats: optimal (the DP's optimum, which differs from total in its last bits), is_tour,
    sweeps = layers launched, candidates = terms, layers_ms = the DP layers' share of kernel_ms."""
    from . import Context, Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    own = None
    if exact_walk and not ctx.flags & _capi.TL_FLAG_BHK_EXACT_WALK:
        own = ctx = Context(ctx.device, ctx.flags | _capi.TL_FLAG_BHK_EXACT_WALK)
    try:
        packed = problem.explicit_packed()  # GEO / EXPLICIT: every distance is the packed matrix's (distance_by_pos, :45, :67, :110, :135)
        n = len(problem)
        out = np.empty(max(n, 1), dtype=np.uint32)
        cost, optimal, is_tour = C.c_float(), C.c_float(), C.c_uint32()
        st = _capi.TlStats()
        ctx.check(ctx.lib.tl_bellman_karp(ctx.handle, problem.xy.ctypes.data_as(C.c_void_p),
                                          None if packed is None else packed.ctypes.data_as(C.c_void_p), n,
                                          out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(optimal), C.byref(is_tour), C.byref(st)))
    finally:
        if own is not None:
            own.close()
    route = problem.ids[out[:n]]
    if progress_tx is not None:
        for v in problem.ids[:max(n - 1, 0)]:
            progress_tx("CityChange", int(v))
        progress_tx("PathUpdate", ([int(v) for v in route], 0.0))
        progress_tx("Done", None)
    stats = st.as_dict()
    stats["layers_ms"] = stats.pop("reversed") / 1e6
    stats["optimal"] = np.float32(optimal.value)
    stats["is_tour"] = int(is_tour.value)
    return Solution(cost.value, route, problem, stats)
