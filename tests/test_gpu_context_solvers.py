"""The newer solvers on one grow-only context (-m gpu): savings, Christofides, Bellman-Held-Karp, branch and bound, Or-opt and 3-opt
for a population, simulated annealing, tabu search, the genetic algorithm, hill climb, ant colony, particle swarm, cuckoo search, flower
pollination, gravitational search, the Kohonen map and the Fourier curve all carve private tables out of c->work and share c->misc,
c->init, c->out_pos, c->out_cost, c->dm and c->dmfull with each other and with the older solvers; nothing clears those buffers between
calls.  The jobs are tests/_context_jobs.py's (one small job per family and two answered on the host), every expectation the pure
statement of the solver, every comparison exact.

1. The context is first filled by one large call of every family and by the older solvers' fillers; then the jobs run in three orders
   and each on a context of its own: no result depends on what ran before.
2. One job per host path (chains, genetic, Swarm4, ant colony, Kohonen map, Fourier curve, branch and bound, Bellman-Held-Karp,
   constructions, population scans) in a sequence in which every path follows every other directly: 91 calls.
3. tl_two_opt_last_counters behind every family: none of the newer host files touches out_stats, so the answer stays the descent's.

Measured on the MI355X: the 3 tests of this file take 0.8 s together (the fillers 0.54 s, the three orders and the 19 fresh contexts
0.20 s, the 91 calls of the pair sequence 0.03 s, the counters 0.02 s), 3 s with the imports and the job table; the oracle
expectations 0.4 s on the CPU.  Checked by sabotage on a scratch copy of the library: without the hipMemsetAsync of simulated
annealing's records in c->misc all three tests fail — the order test at its first job ("largest first", sim_anneal directly behind
the fillers), the pair sequence at call 0.
"""
import ctypes as C

import numpy as np
import pytest

import _bnb_cases as BK
import _context_jobs as CJ
import _oracle as O
import _sa_cases as K
import test_gpu_context_layer as L
from _context_jobs import vp

pytestmark = pytest.mark.gpu

_cache = {}


def table_and_expectations():
    """the job table and every oracle expectation, computed once for the module and left unchanged"""
    if not _cache:
        _cache["table"] = CJ.jobs()
        _cache["want"] = [j.oracle() for j in _cache["table"]]
    return _cache["table"], _cache["want"]


def _nn(xy):
    return O.nearest_neighbor(xy, None, len(xy), 3)[1].astype(np.uint32)


def _perms(n, count, seed):
    return np.ascontiguousarray(np.stack([O.restart_perm(n, seed, r) for r in range(count)]).astype(np.uint32))


def _fill_with_newer_solvers(c):
    """One large call of every newer family; results are not compared.  A call is large when its share of work, misc, init, out_pos,
    out_cost and dmfull is bigger than that of every small job: the small jobs have n <= 130 and at most 5 runs, so with
    n >= 300 (17 and 64 for the exact solvers, whose small jobs have 11 and 12) and 6 or 8 runs every size below — each is monotone
    in n and in the run count — exceeds the small jobs'.  The sizes are the host files' own (csrc/tl_api_*.hip)."""
    from teeline_amd import _capi
    lib, h = c.lib, c.handle
    info = c.device_info()
    WORK = 8 << 30
    st = _capi.TlStats()

    def population(fn, xy, pk, n, head, mid, count, moves=True):
        CJ._population(c, fn, xy, pk, n, head, mid, count, moves)

    # simulated annealing, hill climb: misc count x 16, init count x n x 4 (a start tour each), out_pos count x n x 4, out_cost count x 4;
    # work is the window table and the trace log only.  8 chains of n = 1500 (below tl_*_lds_max_n, asserted) against 5 x 130 and 3 x 64.
    n = 1500
    assert n <= lib.tl_sim_anneal_lds_max_n(h) and n <= lib.tl_hill_climb_lds_max_n(h)
    xy = K.synth(n, 801)
    o = _capi.TlSaOpts(3, 0.5, 400.0, 500.0)
    starts = _perms(n, 8, 801)
    population(lib.tl_sim_anneal_population, xy, None, n, (vp(starts), 8), (C.byref(o), 1), 8)
    o = _capi.TlHillOpts(3, 2, 0, 0)
    population(lib.tl_hill_climb_population, xy, None, n, (vp(starts), 8), (C.byref(o), 1), 8)
    # tabu: misc count x 32, work = log + held x (up256(2 n^2) + up256(4 n)); the plan says how many chains are held at once.  Matrix form:
    # dm n (n - 1) / 2 x 4, dmfull up256(4 n^2).  6 chains of n = 600: 4.3 MB of rings against 4 x 3.4 KB; dmfull 1.4 MB against 6.4 KB.
    n = 600
    assert n <= lib.tl_tabu_search_lds_max_n(h)
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    assert lib.tl_tabu_search_plan(n, 6, info["cus"], info["lds_bytes"], WORK, c.flags, C.byref(w), C.byref(t), C.byref(per)) == 0 and per.value >= 1
    xy = K.synth(n, 803)
    pk = O.dm_build_packed(xy)
    starts = _perms(n, 6, 803)
    population(lib.tl_tabu_search_population, xy, pk, n, (vp(starts), 6), (2, 1), 6)
    # genetic: misc count x 32, work = log + routes + held x (2 up256(2 n^2) + 4 up256(4 (n + 1))).  4 runs of n = 400, matrix form:
    # 2.6 MB of populations against 3 x 2.7 KB.
    n = 400
    assert n <= lib.tl_genetic_algorithm_max_n(h)
    xy = K.synth(n, 804)
    pk = O.dm_build_packed(xy)
    starts = _perms(n, 1, 804)
    population(lib.tl_genetic_algorithm_population, xy, pk, n, (vp(starts),), (1, 0.5, 3, 1), 4, moves=False)
    # Swarm4 (tl_api_swarm.h): misc count x 32, init, out_pos, out_cost as above; work = log + routes + epoch log, then held x run_bytes:
    # pso 6 P n + 2 n + 8 P vmax(n) + 16 P, cs 6 N n + 2 n + 16 N, fpa 4 N n + 2 n + 12 N, gsa 2 N n + 2 n + 14 N.  6 runs of n = 600 with
    # a start tour each against at most 4 runs of n <= 50.  The traced call last: 4096 routes of n = 600 (9.8 MB) in front of the tables,
    # against the small traced job's 91 routes of n = 33.
    n = 600
    for max_n in (lib.tl_particle_swarm_max_n, lib.tl_cuckoo_search_max_n, lib.tl_flower_pollination_max_n, lib.tl_gravitational_search_max_n):
        assert n <= max_n(h)
    xy = K.synth(n, 805)
    starts = _perms(n, 6, 805)
    o = _capi.TlCsOpts(1, 3, 0.25)
    population(lib.tl_cuckoo_search_population, xy, None, n, (vp(starts), 6), (C.byref(o), 1), 6)
    o = _capi.TlFpaOpts(1, 3, 0.001)
    population(lib.tl_flower_pollination_population, xy, None, n, (vp(starts), 6), (C.byref(o), 1), 6)
    o = _capi.TlGsaOpts(1, 3, 0)
    population(lib.tl_gravitational_search_population, xy, None, n, (vp(starts), 6), (C.byref(o), 1), 6)
    o = _capi.TlPsoOpts(2, 3)
    population(lib.tl_particle_swarm_population, xy, None, n, (vp(starts), 6), (C.byref(o), 1), 6)
    out, log, routes, elog = np.empty(n, np.uint32), np.empty((4096, 4), np.uint32), np.empty((4096, n), np.uint32), np.empty((2, 60), np.uint32)
    cost, ln = C.c_float(), C.c_uint32()
    c.check(lib.tl_particle_swarm_trace(h, vp(xy), n, None, vp(starts), C.byref(o), 1, 0, vp(out), C.byref(cost), C.byref(st), vp(log), 4096, C.byref(ln), vp(routes), 4096,
                                        vp(elog), 2))
    # ant colony: misc count x 32, work = trace + held x (3 up256(4 n^2) + 3 up256(2 ants n) + 3 up256(4 ants)).  4 runs of n = 400 with 25 ants,
    # matrix form: 7.7 MB against 3 x 5 KB.
    n = 400
    assert n <= lib.tl_ant_colony_max_n(h)
    xy = K.synth(n, 806)
    pk = O.dm_build_packed(xy)
    population(lib.tl_ant_colony_population, xy, pk, n, (None, 0), (1, 1.0, 2.0, 0.5, 25, 1), 4, moves=False)
    # Kohonen map: out_pos count x n x 4, work = cities, ring start, schedule, log, checkpoints, then 16 M + 16 n per run.  4 runs of n = 1500
    # (M = 12 000: past the LDS form, the rings themselves lie in c->work) against one of n = 21; then a traced call of n = 600, whose log
    # and checkpoint regions are in front.
    n = 1500
    assert n <= lib.tl_kohonen_som_max_n(h, 8, 0)
    xy = K.synth(n, 807)
    o = _capi.TlSomOpts(3, 8, 0.8, 0.1, 0, 0, 0)
    outs, costs, best = np.empty((4, n), np.uint32), np.empty(4, np.float32), C.c_uint32()
    c.check(lib.tl_kohonen_som_population(h, vp(xy), n, None, 0, 4, C.byref(o), 1, vp(outs), vp(costs), C.byref(best), C.byref(st)))
    n = 600
    o = _capi.TlSomOpts(40, 8, 0.8, 0.1, 0, 0, 0)
    out, log, ring = np.empty(n, np.uint32), np.empty((40, 2), np.uint32), np.empty(2 * 8 * n)
    ep, tours, cb = np.empty(20, np.uint32), np.empty((20, n), np.uint32), np.empty(20, np.uint32)
    xy6 = np.ascontiguousarray(xy[:n])
    c.check(lib.tl_kohonen_som_trace(h, vp(xy6), n, None, C.byref(o), 1, 0, vp(out), C.byref(cost), C.byref(st), vp(log), 40, vp(ring), vp(ep), vp(tours), vp(cb), 20,
                                     C.byref(ln)))
    # Fourier curve: out_pos J x n x 4, work = tl_fourier_curve_work_bytes(n, opts, J, ...).  4 jobs of n = 1500, k_max 4, m 200 against one of
    # n = 45, k_max 2, m 64 (asserted on the query).
    n = 1500
    arr = (_capi.TlFourierOpts * 4)(*[_capi.TlFourierOpts(4, 200, 1, 0, 0.05 + 0.01 * j, 0.5, 0.05, 0, 0) for j in range(4)])
    small = _capi.TlFourierOpts(2, 64, 5, 0, 0.05, 0.5, 0.05, 0, 0)
    assert lib.tl_fourier_curve_work_bytes(n, arr, 4, 0) > lib.tl_fourier_curve_work_bytes(45, C.byref(small), 1, 0) > 0
    outs, costs, coeffs = np.empty((4, n), np.uint32), np.empty(4, np.float32), np.empty((4, 18))
    c.check(lib.tl_fourier_curve_batch(h, vp(xy), n, None, arr, 4, vp(outs), vp(costs), vp(coeffs), 18, C.byref(best), C.byref(st), None, 0, None))
    # branch and bound: work = bnb_ws_bytes(waves, queue capacity), both of which grow with n and the frontier; n = 64 (the largest) on a circle,
    # from its 2-opt tour, ended by a node budget if the proof takes longer.  Bellman-Held-Karp: work = 2^(n - 1) rows of 128 bytes:
    # n = 17, matrix form, 8 MB against the small job's 128 KB.
    xy = BK.circle_xy(64, 0)
    r = BK.call(c, xy, None, 64, init=BK.seed_tour(xy, None, 64, 0), max_nodes=200000)
    assert r[0] == 0, r
    xy = K.synth(17, 808)
    pk = O.dm_build_packed(xy)
    out, optimal, ok = np.empty(17, np.uint32), C.c_float(), C.c_uint32()
    c.check(lib.tl_bellman_karp(h, vp(xy), vp(pk), 17, vp(out), C.byref(cost), C.byref(optimal), C.byref(ok), C.byref(st)))
    # constructions: out_pos n x 4, work = greedy_ws_bytes(n, cap), the sort's keys of n (n - 1) / 2 pairs; matrix form.  n = 1500 against 90 / 70.
    n = 1500
    xy = K.synth(n, 809)
    pk = O.dm_build_packed(xy)
    out, hub = np.empty(n, np.uint32), C.c_uint32()
    c.check(lib.tl_savings(h, vp(xy), vp(pk), n, _capi.TL_SAVINGS_HUB_AUTO, vp(out), C.byref(cost), C.byref(hub), C.byref(st)))
    c.check(lib.tl_christofides(h, vp(xy), vp(pk), n, vp(out), C.byref(cost), C.byref(st)))
    # population scans: misc count x 16, init and out_pos count x n x 4, work batch x tour_work (the per-tour matrices of the matrix form).
    # 8 tours of n = 1000 (Or-opt) and of n = 150 in matrix form (3-opt) against 4 x 60 and 3 x 30; from 2-opt'd tours, so a few moves each.
    n = 1000
    assert n <= c.or_opt_lds_max_n()
    xy = K.synth(n, 810)
    two = O.two_opt(xy, None, n, init=_nn(xy))[1].astype(np.uint32)
    tours = np.ascontiguousarray(np.stack([np.roll(two, 7 * r) for r in range(8)]))
    outs, costs, mv = np.empty((8, n), np.uint32), np.empty(8, np.float32), np.empty(8, np.uint32)
    c.check(lib.tl_or_opt_population(h, vp(xy), n, None, vp(tours), 8, vp(outs), vp(costs), vp(mv), C.byref(st)))
    n = 150
    assert n <= c.three_opt_pop_max_n()
    xy = K.synth(n, 811)
    pk = O.dm_build_packed(xy)
    two = O.two_opt(xy, None, n, init=_nn(xy))[1].astype(np.uint32)
    tours = np.ascontiguousarray(np.stack([np.roll(two, 7 * r) for r in range(8)]))
    outs = np.empty((8, n), np.uint32)
    c.check(lib.tl_three_opt_population(h, vp(xy), n, vp(pk), vp(tours), 8, vp(outs), vp(costs), vp(mv), C.byref(st)))


@pytest.fixture(scope="module")
def filled():
    """one context behind the large calls of the newer solvers and then of the older ones (2-opt in matrix form at n = 4000 with its
    neighbour lists behind the matrix in dmfull, LK, candidate lists, ...): both tests below run inside these buffers"""
    import teeline_amd as TA
    c = TA.Context(0)
    _fill_with_newer_solvers(c)
    L._fill_with_stale_data(c)
    yield c
    c.close()


def test_call_order_of_the_newer_solvers_does_not_show_in_any_result(filled):
    import teeline_amd as TA
    table, want = table_and_expectations()
    by_size = sorted(range(len(table)), key=lambda k: (-table[k].size, k))
    orders = {"largest first": by_size, "smallest first": by_size[::-1], "seeded shuffle": [int(v) for v in np.random.default_rng(8).permutation(len(table))]}
    before = "the fillers"
    for oname, order in orders.items():
        for k in order:
            got = table[k].run(filled)
            assert got == want[k], f"order '{oname}', job {k} ({table[k].name}) directly behind {before} differs from the oracle"
            before = f"job '{table[k].name}'"
    for k, j in enumerate(table):  # ... and each on a context of its own
        with TA.Context(0) as c:
            assert j.run(c) == want[k], f"fresh context, job {k} ({j.name}) differs from the oracle"


def test_every_host_path_directly_behind_every_other(filled):
    table, want = table_and_expectations()
    reps = CJ.representatives(table)
    g = len(reps)
    seq = CJ.euler_sequence(g)
    assert len(seq) == g * (g - 1) + 1 and {(a, b) for a, b in zip(seq, seq[1:])} == {(a, b) for a in range(g) for b in range(g) if a != b}
    before = "what the context held"
    for step, a in enumerate(seq):
        k = reps[a]
        got = table[k].run(filled)
        assert got == want[k], f"pair sequence, call {step}: job '{table[k].name}' directly behind {before} differs from the oracle"
        before = f"job '{table[k].name}'"


def test_last_counters_behind_every_newer_solver():
    """tl_two_opt_last_counters answers with the last 2-opt descent's counters or with TL_ERR_BADARG, never with another solver's data
    (tests/test_gpu_context_layer.py, section 2).  None of the newer host files touches out_stats or stats_valid, so today the
    answer behind each of them is the descent's own sixteen words."""
    import teeline_amd as TA
    table, want = table_and_expectations()
    n = 400
    xy = O.synth_xy(n, seed=12)
    with TA.Context(0) as c:
        before = L._descent_counters(c, xy, n, O.restart_perm(n, 1, 1))
        seen = {}
        for k, j in enumerate(table):
            assert j.run(c) == want[k], j.name
            try:
                seen[j.name] = "equal" if c.two_opt_last_counters() == before else "another solver's data"
            except TA.TeelineGpuError as e:
                seen[j.name] = "refused" if e.code == TA._capi.TL_ERR_BADARG else f"error {e.code}"
        assert not [s for s in seen.items() if s[1] not in ("equal", "refused")], seen  # the rule
        assert all(s == "equal" for s in seen.values()), seen                              # ... and what the code does today, family by family
        assert {j.family for j in table} == set(CJ.FAMILIES)
        L._descent_counters(c, xy, n, O.restart_perm(n, 1, 2))  # a following descent's counters are its own again
