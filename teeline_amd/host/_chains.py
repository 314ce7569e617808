"""What the mirrors of the seeded chain solvers share (simulated_annealing, tabu_search; genetic_algorithm takes the small helpers):
the ctypes plumbing, the reversal and the solve skeleton population -> best chain -> optional re-trace / single / trace."""
import ctypes as C

import numpy as np


def vp(a):
    """a numpy array (or None) as a void pointer argument"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def swap_cities(tour, frm, to):
    """route.rs:102-113: positions from..=to of the open path reversed; returns the new tour"""
    t = np.array(tour, copy=True)
    t[frm:to + 1] = t[frm:to + 1][::-1]
    return t


def start_tour(problem, init_pos):
    """the tour a chain starts from: the given positions, or city order"""
    return np.arange(len(problem), dtype=np.uint32) if init_pos is None else np.array(init_pos, dtype=np.uint32)


def bits_to_f32(bits):
    """the f32 a trace record carries as a u32"""
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def solve_chains(problem, progress_tx, chains, population, single, trace, replay):
    """chains > 1: population(chains, outs, costs, moves, best, st) runs them at once and the best one (lowest cost, then lowest
    chain) is returned; with a channel that chain runs once more, alone, for its trace.  Else single(out, cost, st), or with a
    channel trace(0).  trace(chain) -> (out, cost, log, stats dict); replay(log) sends the reference's messages."""
    from . import Solution
    from .. import _capi
    n = len(problem)
    st = _capi.TlStats()
    if chains > 1:
        outs = np.empty((chains, n), dtype=np.uint32)
        costs = np.empty(chains, dtype=np.float32)
        moves = np.zeros(chains, dtype=np.uint32)
        best = C.c_uint32()
        population(chains, outs, costs, moves, best, st)
        chain = int(best.value)
        stats = dict(st.as_dict(), moves=int(moves[chain]), chain=chain)
        if progress_tx is not None:
            replay(trace(chain)[2])
        return Solution(float(costs[chain]), problem.ids[outs[chain]], problem, stats)
    if progress_tx is None:
        out = np.empty(n, dtype=np.uint32)
        cost = C.c_float()
        single(out, cost, st)
        return Solution(cost.value, problem.ids[out], problem, st.as_dict())
    out, cost, log, stats = trace(0)
    replay(log)
    return Solution(cost, problem.ids[out], problem, stats)
