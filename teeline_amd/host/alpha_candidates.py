"""Alpha-nearness candidate lists over tl_alpha_candidates: Helsgaun's alpha(i, j) — how much the minimum 1-tree
under penalties pi grows when edge (i, j) is forced into it — and the k best candidates per city.  This project's own specification,
like the bound it builds on (one_tree_bound): pi is usually a Bound's best penalties.

    candidates(problem, k, pi=None, root=0)        on the device: an AlphaCandidates
    candidates_host(problem, k, pi=None, root=0)   the sequential restatement on the CPU: no context, no device
    from_ascent(problem, k, iterations=...)        the ascent as one_tree_bound.bound runs it, then its best pi's lists

The rows are POSITIONS in (alpha, w, position) order.  lin_kernighan.solve(..., candidates=rows) searches them: alpha chooses the set,
distance orders it (the library puts every row into ascending Euclidean distance before the search reads it).
"""
import ctypes as C

import numpy as np

from ._chains import vp


class AlphaCandidates:
    """rows (n x k' positions), alpha (n x k' f64), parent and root_nb (the 1-tree), pi (what it was built under, None: zero), stats."""

    def __init__(self, rows, alpha, parent, root_nb, pi, stats):
        self.rows, self.alpha, self.parent, self.root_nb, self.pi, self.stats = rows, alpha, parent, root_nb, pi, stats


def _call(lib, handle, problem, k, pi, root, threads):
    from .. import _capi
    n = len(problem)
    kk = max(min(int(k), n - 1), 0)
    rows = np.zeros((max(n, 1), max(kk, 1)), dtype=np.uint32)
    alpha = np.zeros((max(n, 1), max(kk, 1)))
    par = np.zeros(max(n, 1), dtype=np.uint32)
    nb = np.zeros(2, dtype=np.uint32)
    if pi is not None:
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        if pi.shape != (n,):
            raise ValueError(f"alpha_candidates: pi has shape {pi.shape}, the problem {n} cities")
    st = _capi.TlStats()
    if handle is None:
        rc = lib.tl_alpha_candidates_host(vp(problem.xy), vp(problem.explicit_packed()), n, vp(pi), int(root), int(k), vp(rows), vp(alpha), vp(par), vp(nb))
    else:
        rc = lib.tl_alpha_candidates(handle, vp(problem.xy), vp(problem.explicit_packed()), n, vp(pi), int(root), int(k), int(threads), vp(rows), vp(alpha),
                                     vp(par), vp(nb), C.byref(st))
    return rc, AlphaCandidates(rows[:n, :kk].copy(), alpha[:n, :kk].copy(), par[:n].copy(), (int(nb[0]), int(nb[1])), pi, st.as_dict())


def candidates(problem, k=5, pi=None, *, root=0, ctx=None, threads=0):
    """tl_alpha_candidates.  threads: the workgroup of a source city (0: the plan's); a launch parameter, the same result."""
    from . import default_context
    ctx = ctx or default_context()
    rc, out = _call(ctx.lib, ctx.handle, problem, k, pi, root, threads)
    ctx.check(rc)
    return out


def candidates_host(problem, k=5, pi=None, *, root=0):
    """tl_alpha_candidates_host: the same contract on the CPU."""
    from .. import _capi
    lib = _capi.load()
    rc, out = _call(lib, None, problem, k, pi, root, 0)
    if rc != _capi.TL_OK:
        raise _capi.TeelineGpuError(rc, lib.tl_last_error(None).decode())
    return out


def from_ascent(problem, k=5, *, root=0, iterations=1000, ctx=None):
    """The ascent as one_tree_bound.bound runs it (upper from nearest_neighbor -> two_opt), then the lists under its best pi.
    Returns (AlphaCandidates, Bound)."""
    from . import one_tree_bound
    b = one_tree_bound.bound(problem, None, root=root, iterations=iterations, ctx=ctx)
    return candidates(problem, k, b.pi, root=root, ctx=ctx), b


def plan(n, k=5, *, lds_bytes=163840):
    """tl_alpha_candidates_plan (host-only): {"threads", "lds_bytes"} of a source city's workgroup."""
    from .. import _capi
    t, used = C.c_int(), C.c_uint32()
    rc = _capi.load().tl_alpha_candidates_plan(int(n), int(k), int(lds_bytes), C.byref(t), C.byref(used))
    if rc:
        raise _capi.TeelineGpuError(rc, "tl_alpha_candidates_plan: k outside 1..64, lds_bytes < 0 or n beyond tl_alpha_candidates_max_n")
    return {"threads": t.value, "lds_bytes": used.value}
