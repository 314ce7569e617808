"""fourier::solve — mirror of src/tsp/fourier.rs:10-312 over tl_fourier_curve.

The algorithm is the reference's: a closed curve of 2 k_max + 1 Fourier coefficients descends towards the cities in k_max stages of
`epochs` gradient steps, and the tour is the cities in the order of their nearest curve sample.  Its quirks are kept (n < 2 is
trivial, a start tour is ignored, no progress is sent, sequential f64 sums in city order, only the modes |k| <= k_active move).
Five things are this project's specification instead (csrc/fourier_spec.h): the basis table with its exact
reduction, sqrt instead of hypot, the lowest index among samples at equal f32 distance, (2 pi k)^2 as t t, lambda as the running
product.  The solver draws nothing: a batch is a list of option sets on one problem (solve_many).
"""
import ctypes as C

import numpy as np

from ._chains import vp


class FourierOptions:
    """src/tsp/mod.rs:1341-1384 (the field `lambda` is spelled `lam`: a Python keyword)"""

    def __init__(self, k_max=4, m=200, lam=0.05, lambda_decay=0.5, lr=0.05, epochs=400):
        self.k_max, self.m, self.lam, self.lambda_decay, self.lr, self.epochs = k_max, m, lam, lambda_decay, lr, epochs

    def validate(self):  # mod.rs:1354-1384
        if self.k_max < 1:
            raise ValueError("k_max must be >= 1")
        if self.m < 2:
            raise ValueError("m must be >= 2")
        if not self.lam > 0.0:
            raise ValueError("lambda must be > 0")
        if not 0.0 < self.lambda_decay < 1.0:
            raise ValueError("lambda_decay must be in (0, 1)")
        if not self.lr > 0.0:
            raise ValueError("lr must be > 0")
        if self.epochs < 1:
            raise ValueError("epochs must be >= 1")


def _c_opts(o, chunk=0, span_steps=0, threads=0):
    from .. import _capi
    return _capi.TlFourierOpts(int(o.k_max), int(o.m), int(o.epochs), int(chunk), float(o.lam), float(o.lambda_decay), float(o.lr), int(span_steps), int(threads))


def solve_many(problem, options, *, ctx=None, chunk=0, span_steps=0, threads=0, return_all=False):
    """options: a list of FourierOptions, one job (one workgroup) each, all at once (tl_fourier_curve_batch).  Returns the best job's
    Solution (lowest cost, then lowest index; stats["job"] names it, stats["costs"] lists every job's cost); return_all: the list of
    every job's Solution instead, each with stats["coeffs"], its final coefficients as complex numbers for k = -k_max .. k_max."""
    from . import Solution, default_context
    from .. import _capi
    ctx = ctx or default_context()
    options = list(options)
    if not options:
        raise ValueError("fourier_curve: no option set")
    n = len(problem)
    if problem.xy is None:
        raise ValueError("fourier_curve descends on the coordinates: the problem has none")
    J = len(options)
    arr = (_capi.TlFourierOpts * J)(*[_c_opts(o, chunk, span_steps, threads) for o in options])
    stride = 2 * (2 * max(int(o.k_max) for o in options) + 1)
    outs = np.zeros((J, max(n, 1)), dtype=np.uint32)
    costs = np.zeros(J, dtype=np.float32)
    coeffs = np.zeros((J, stride))
    best, st = C.c_uint32(), _capi.TlStats()
    ctx.check(ctx.lib.tl_fourier_curve_batch(ctx.handle, vp(problem.xy), n, vp(problem.explicit_packed()), arr, J, vp(outs), vp(costs), vp(coeffs), stride,
                                             C.byref(best), C.byref(st), None, 0, None))

    def one(j):
        L = 2 * int(options[j].k_max) + 1
        stats = dict(st.as_dict(), job=j, coeffs=coeffs[j, :2 * L].view(np.complex128).copy(), costs=[float(v) for v in costs])
        return Solution(float(costs[j]), problem.ids[outs[j, :n]], problem, stats)

    return [one(j) for j in range(J)] if return_all else one(int(best.value))


def solve(problem, opts=None, progress_tx=None, init_tour=None, *, ctx=None):
    """opts: FourierOptions.  progress_tx and init_tour are ignored, as the reference ignores them (fourier.rs:13-14)."""
    return solve_many(problem, [opts or FourierOptions()], ctx=ctx)
