"""The small jobs of the solvers added after the context and thread tests were written — savings, Christofides, Bellman-Held-Karp,
branch and bound, Or-opt and 3-opt for a population, simulated annealing, tabu search, the genetic algorithm, hill climb, ant colony,
particle swarm, cuckoo search, flower pollination, gravitational search, the Kohonen map, the Fourier curve — as one table:

    Job(name, family, group, size, run(ctx) -> outputs, oracle() -> the same outputs, matrix, init, count, record)

tests/test_gpu_context_solvers.py runs them in several orders on one grow-only context, tests/probes/thread_campaign.py on eight
threads, tests/test_context_jobs.py checks on the CPU that the table covers what it says.  Every comparison is exact: tours element
for element, costs (and every other f32 / f64) as bit patterns.  Every oracle is the pure-Python / numpy statement of its solver
(tests/_*_oracle.py; the C oracle of tests/_oracle.py for the two population scans).  Test infrastructure.

What the set covers (derived from the host files, csrc/tl_api_*.hip):
  matrix form (c->dm and c->dmfull rewritten)   christofides 70, three_opt_pop 30, tabu 40, genetic 24, cuckoo 20, ant_colony 18, bhk 11:
                                                in "largest first" each but the first runs behind a matrix job of a larger n
  start tours (c->init)                         sim_anneal (init_count == count == 5), tabu (one tour for 4 chains), genetic, particle_swarm,
                                                branch_and_bound, and the two population scans (a tour per descent)
  more than one chain or run                    16-byte records in c->misc: sim_anneal 5, hill_climb 3, or_opt_pop 4, three_opt_pop 3;
                                                32-byte records (8 words per run): tabu 4, genetic 3, cuckoo 4, gravitational 3, ant_colony 3
  a traced call                                 particle_swarm (the Swarm4 trace regions in front of its tables in c->work), kohonen_som
  answered on the host                          "particle_swarm n=1" and "ant_colony n=2": sizes 45 and 35, so between device jobs in every order

Measured: the 19 oracle expectations take 0.4 s together on one CPU core (the cuckoo search's four runs 0.2 s of them); building the
table (instances, packed matrices, start tours) 1.6 s.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import _aco_oracle as ACO
import _bhk_oracle as BHK
import _bnb_oracle as BNB
import _christofides_oracle as XO
import _cs_oracle as CSO
import _fourier_oracle as FO
import _fpa_oracle as FPO
import _ga_oracle as GAO
import _gsa_oracle as GSO
import _hill_oracle as HO
import _oracle as O
import _pso_oracle as PSO
import _sa_cases as K
import _sa_oracle as SAO
import _savings_oracle as SVO
import _som_oracle as SOMO
import _tabu_oracle as TO

Job = namedtuple("Job", "name family group size run oracle matrix init count record")

FAMILIES = ("savings", "christofides", "bellman_karp", "branch_and_bound", "or_opt_pop", "three_opt_pop", "sim_anneal", "tabu", "genetic", "hill_climb",
            "ant_colony", "particle_swarm", "cuckoo", "flower_pollination", "gravitational", "kohonen_som", "fourier")
# the host paths: tl_api_chains.h users with 4-word / 8-word records, tl_api_ga.hip, Swarm4 of tl_api_swarm.h, tl_api_aco.hip, ...
GROUPS = {"chains": ("sim_anneal", "tabu", "hill_climb"), "genetic": ("genetic",),
          "swarm4": ("particle_swarm", "cuckoo", "flower_pollination", "gravitational"), "ant_colony": ("ant_colony",), "kohonen_som": ("kohonen_som",),
          "fourier": ("fourier",), "branch_and_bound": ("branch_and_bound",), "bellman_karp": ("bellman_karp",), "constructions": ("savings", "christofides"),
          "pop_scans": ("or_opt_pop", "three_opt_pop")}
GROUP_OF = {f: g for g, fs in GROUPS.items() for f in fs}
# one job per host path for the pair sequence (the chains' is simulated annealing: its kernel adds to its record over the launches of a
# schedule, so it is the chain solver whose result hangs on the host path's zeroing)
REPRESENTATIVES = ("sim_anneal", "genetic", "cuckoo", "ant_colony", "kohonen_som", "fourier", "branch_and_bound", "bellman_karp", "christofides", "or_opt_pop")
NONE32 = 0xFFFFFFFF


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def f32bits(v):
    return int(np.float32(v).view(np.uint32))


def _best(cost_bits):
    """the run of the lowest cost, then the lowest index (tl_pack_cost_key)"""
    return int(np.argmin([(b << 32) | r for r, b in enumerate(cost_bits)]))


def _population(c, fn, xy, packed, n, head, mid, count, moves=True, host=False):
    """a *_population entry: fn(ctx, xy, n, packed, *head, first = 0, count, *mid, outs, costs[, moves], best, stats) ->
    (tours, cost bits, moves or None, best); every output array is pre-filled with a pattern the call has to overwrite.
    host: the call is answered without the device — two more words, the kernel time in its stats and the one the context reports
    behind it (tl_last_kernel_ms, which has no kernel sequence to report and may say so), both 0"""
    from teeline_amd import _capi
    outs = np.full((count, max(n, 1)), NONE32, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    mv = np.full(count, NONE32, dtype=np.uint32)
    best, st = C.c_uint32(NONE32), _capi.TlStats()
    tail = (vp(outs), vp(costs)) + ((vp(mv),) if moves else ()) + (C.byref(best), C.byref(st))
    c.check(fn(c.handle, vp(xy), n, vp(packed), *head, 0, count, *mid, *tail))
    got = (outs[:, :n].tolist(), costs.view(np.uint32).tolist(), mv.tolist() if moves else None, int(best.value))
    if host:
        ms = C.c_double(0.0)
        assert c.lib.tl_last_kernel_ms(c.handle, C.byref(ms)) in (_capi.TL_OK, _capi.TL_ERR_BADARG)
        got += (st.kernel_ms, ms.value)
    return got


def _want_population(rows, moves=True):
    """the same tuple from the oracle's (tour, cost, moves) per run"""
    cb = [f32bits(cost) for _t, cost, _m in rows]
    return ([[int(v) for v in t] for t, _c, _m in rows], cb, [int(m) for _t, _c, m in rows] if moves else None, _best(cb))


def euler_sequence(g):
    """A closed walk on the complete digraph of g vertices that takes every arc a -> b, a != b, exactly once: g (g - 1) + 1 vertices.
    Hierholzer's algorithm with the arcs of every vertex taken in ascending order: deterministic."""
    nxt = {a: [b for b in range(g) if b != a][::-1] for a in range(g)}
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def jobs():
    """The table.  Every instance has a seed of its own; K.synth gives coordinates on a 0.25 grid (exact in f32)."""
    from teeline_amd import _capi  # (the structs only: nothing is loaded before a job runs)
    out = []

    def add(name, family, size, run, oracle, matrix=False, init=False, count=1, record=0):
        out.append(Job(name, family, GROUP_OF[family], size, run, oracle, matrix, init, count, record))

    # ---- constructions (tl_api_greedy.hip): out_pos, out_cost, the sort workspace in c->work
    xy = K.synth(90, 901)

    def run_savings(c, xy=xy):
        o, cost, hub = np.full(90, NONE32, dtype=np.uint32), C.c_float(-1.0), C.c_uint32(NONE32)
        c.check(c.lib.tl_savings(c.handle, vp(xy), None, 90, _capi.TL_SAVINGS_HUB_AUTO, vp(o), C.byref(cost), C.byref(hub), C.byref(_capi.TlStats())))
        return (o.tolist(), f32bits(cost.value), int(hub.value))

    add("savings n=90", "savings", 90, run_savings, lambda xy=xy: (lambda r: (r[0].tolist(), f32bits(r[1]), int(r[2])))(SVO.savings(xy)))

    xy = K.synth(70, 902)
    pk = O.dm_build_packed(xy)

    def run_christofides(c, xy=xy, pk=pk):
        o, cost = np.full(70, NONE32, dtype=np.uint32), C.c_float(-1.0)
        c.check(c.lib.tl_christofides(c.handle, vp(xy), vp(pk), 70, vp(o), C.byref(cost), C.byref(_capi.TlStats())))
        return (o.tolist(), f32bits(cost.value))

    add("christofides matrix n=70", "christofides", 70, run_christofides,
        lambda xy=xy, pk=pk: (lambda r: (r[0].tolist(), f32bits(r[1])))(XO.christofides(xy, pk, 70)), matrix=True)

    # ---- the exact solvers: the DP table (tl_api_bhk.hip) and the wave headers and queue (tl_api_bnb.hip) in c->work
    xy = K.synth(11, 903)
    pk = O.dm_build_packed(xy)

    def run_bhk(c, xy=xy, pk=pk):
        o = np.full(11, NONE32, dtype=np.uint32)
        cost, optimal, ok = C.c_float(-1.0), C.c_float(-1.0), C.c_uint32(7)
        c.check(c.lib.tl_bellman_karp(c.handle, vp(xy), vp(pk), 11, vp(o), C.byref(cost), C.byref(optimal), C.byref(ok), C.byref(_capi.TlStats())))
        return (o.tolist(), f32bits(cost.value), f32bits(optimal.value), int(ok.value))

    add("bellman_karp matrix n=11", "bellman_karp", 11, run_bhk,
        lambda xy=xy, pk=pk: (lambda r: ([int(v) for v in r[0]], f32bits(r[1]), f32bits(r[2]), int(r[3])))(BHK.bellman_karp(xy, pk, 11)), matrix=True)

    xy = K.synth(12, 904)
    init = O.restart_perm(12, 904, 0)

    def run_bnb(c, xy=xy, init=init):
        o = np.full(12, NONE32, dtype=np.uint32)
        cost, proved, improved, opts = C.c_float(-1.0), C.c_uint32(7), C.c_uint32(7), _capi.TlBnbOpts(0, 0, 0, 0, 0, 0, 0)
        c.check(c.lib.tl_branch_and_bound(c.handle, vp(xy), None, 12, vp(init), C.byref(opts), vp(o), C.byref(cost), C.byref(proved), C.byref(improved), C.byref(_capi.TlBnbStats())))
        return (o.tolist(), f32bits(cost.value), int(proved.value), int(improved.value))

    add("branch_and_bound n=12", "branch_and_bound", 12, run_bnb,
        lambda xy=xy, init=init: (lambda r: ([int(v) for v in r[0]], f32bits(r[1]), 1, int(r[2])))(BNB.dfs(BNB.dist_matrix(xy), 0, 0, [int(v) for v in init])),
        init=True)

    # ---- population scans (tl_api_scans.hip): a start tour per descent in c->init, 4-word records in c->misc
    def scan_job(name, family, fn_name, oracle_fn, n, count, seed, matrix):
        xy = K.synth(n, seed)
        pk = O.dm_build_packed(xy) if matrix else None
        tours = np.stack([O.restart_perm(n, seed, r) for r in range(count)]).astype(np.uint32)

        def run(c):
            o, costs, mv = np.full((count, n), NONE32, dtype=np.uint32), np.full(count, -1.0, dtype=np.float32), np.full(count, NONE32, dtype=np.uint32)
            c.check(getattr(c.lib, fn_name)(c.handle, vp(xy), n, vp(pk), vp(tours), count, vp(o), vp(costs), vp(mv), C.byref(_capi.TlStats())))
            return (o.tolist(), costs.view(np.uint32).tolist(), mv.tolist())

        def oracle():
            rows = [oracle_fn(None if matrix else xy, pk, n, init=t) for t in tours]
            assert all(r[0] == 0 for r in rows)
            return ([r[1].tolist() for r in rows], [f32bits(r[2]) for r in rows], [r[3]["moves"] for r in rows])

        add(name, family, n, run, oracle, matrix=matrix, init=True, count=count, record=16)

    scan_job("or_opt_population 4 x n=60", "or_opt_pop", "tl_or_opt_population", O.or_opt, 60, 4, 905, False)
    scan_job("three_opt_population matrix 3 x n=30", "three_opt_pop", "tl_three_opt_population", O.three_opt, 30, 3, 906, True)

    # ---- the seeded chains (tl_api_chains.h): sim_anneal and hill_climb keep 4-word records, tabu 8-word ones and its rings in c->work
    xy = K.synth(130, 907)
    sa = dict(epochs=40, cooling_rate=0.5, min_temperature=400.0, max_temperature=500.0)
    inits = np.stack([O.restart_perm(130, 907, r) for r in range(5)]).astype(np.uint32)

    def run_sa(c, xy=xy, inits=inits):
        o = _capi.TlSaOpts(sa["epochs"], sa["cooling_rate"], sa["min_temperature"], sa["max_temperature"])
        return _population(c, c.lib.tl_sim_anneal_population, xy, None, 130, (vp(inits), 5), (C.byref(o), 31), 5)

    def want_sa(xy=xy, inits=inits):
        return _want_population([(lambda r: (r[0], r[1], len(r[2])))(SAO.solve(xy, None, 130, inits[r], seed=31, chain=r, **sa)) for r in range(5)])

    add("sim_anneal 5 x n=130, a start tour each", "sim_anneal", 130, run_sa, want_sa, init=True, count=5, record=16)

    xy = K.synth(40, 908)
    pk = O.dm_build_packed(xy)
    init = O.restart_perm(40, 908, 0)

    def run_tabu(c, xy=xy, pk=pk, init=init):
        return _population(c, c.lib.tl_tabu_search_population, xy, pk, 40, (vp(init), 1), (6, 32), 4)

    def want_tabu(pk=pk, init=init):
        return _want_population([(lambda r: (r[0], r[1], r[3]["bests"]))(TO.solve(None, pk, 40, init, epochs=6, seed=32, chain=r)) for r in range(4)])

    add("tabu matrix 4 x n=40, one start tour", "tabu", 40, run_tabu, want_tabu, matrix=True, init=True, count=4, record=32)

    xy = K.synth(64, 909)

    def run_hill(c, xy=xy):
        o = _capi.TlHillOpts(60, 7, 0, 0)
        return _population(c, c.lib.tl_hill_climb_population, xy, None, 64, (None, 0), (C.byref(o), 33), 3)

    def want_hill(xy=xy):
        return _want_population([(lambda r: (r["tour"], r["cost"], r["counters"]["accepts"]))(HO.solve(xy, None, 64, None, seed=33, chain=r, epochs=60, platoo_epochs=7))
                                 for r in range(3)])

    add("hill_climb 3 x n=64", "hill_climb", 64, run_hill, want_hill, count=3, record=16)

    # ---- the genetic algorithm (tl_api_ga.hip): 8-word records, two populations and four prefix rows per run in c->work
    xy = K.synth(24, 910)
    pk = O.dm_build_packed(xy)
    init = O.restart_perm(24, 910, 0)

    def run_ga(c, xy=xy, pk=pk, init=init):
        return _population(c, c.lib.tl_genetic_algorithm_population, xy, pk, 24, (vp(init),), (4, 0.5, 3, 34), 3, moves=False)

    def want_ga(pk=pk, init=init):
        return _want_population([GAO.solve(None, pk, 24, init, epochs=4, mutation_probability=0.5, n_elite=3, seed=34, run=r)[:2] + (0,) for r in range(3)], moves=False)

    add("genetic matrix 3 x n=24, a start tour", "genetic", 24, run_ga, want_ga, matrix=True, init=True, count=3, record=32)

    # ---- the population solvers over Swarm4 (tl_api_swarm.h): 8-word records; the trace regions lie in front of the tables in c->work
    xy = K.synth(33, 911)
    init = O.restart_perm(33, 911, 0)
    pso = dict(epochs=3, n_nearest=3, seed=35, run=0)

    def run_pso_trace(c, xy=xy, init=init):
        P = PSO.particles(3)
        cap = 1 + 3 * P
        o, log, routes, elog = (np.full(33, NONE32, dtype=np.uint32), np.full((cap, 4), NONE32, dtype=np.uint32), np.full((cap, 33), NONE32, dtype=np.uint32),
                                np.full((3, 2 * P), NONE32, dtype=np.uint32))
        cost, ln, po = C.c_float(-1.0), C.c_uint32(), _capi.TlPsoOpts(3, 3)
        c.check(c.lib.tl_particle_swarm_trace(c.handle, vp(xy), 33, None, vp(init), C.byref(po), 35, 0, vp(o), C.byref(cost), C.byref(_capi.TlStats()), vp(log), cap, C.byref(ln),
                                              vp(routes), cap, vp(elog), 3))
        k = min(int(ln.value), cap)
        return (o.tolist(), f32bits(cost.value), int(ln.value), log[:k].tolist(), routes[:k].tolist(), elog.tolist())

    def want_pso_trace(xy=xy, init=init):
        res = PSO.solve(xy, None, 33, init, **pso)
        return (res["tour"].tolist(), f32bits(res["cost"]), len(res["improvements"]), PSO.log_words(res).tolist(), PSO.route_words(res, 33).tolist(),
                PSO.epoch_words(res).tolist())

    add("particle_swarm traced n=33, a start tour", "particle_swarm", 33, run_pso_trace, want_pso_trace, init=True, record=32)

    xy = K.synth(20, 912)
    pk = O.dm_build_packed(xy)

    def run_cs(c, xy=xy, pk=pk):
        o = _capi.TlCsOpts(3, 3, 0.25)
        return _population(c, c.lib.tl_cuckoo_search_population, xy, pk, 20, (None, 0), (C.byref(o), 36), 4)

    def want_cs(pk=pk):
        return _want_population([(lambda r: (r["tour"], r["cost"], r["counters"]["improved"]))(
            CSO.solve(None, pk, 20, None, epochs=3, n_nearest=3, mutation_probability=0.25, seed=36, run=r)) for r in range(4)])

    add("cuckoo matrix 4 x n=20", "cuckoo", 20, run_cs, want_cs, matrix=True, count=4, record=32)

    xy = K.synth(50, 913)

    def run_fpa(c, xy=xy):
        o, cost, po = np.full(50, NONE32, dtype=np.uint32), C.c_float(-1.0), _capi.TlFpaOpts(3, 3, 0.001)
        c.check(c.lib.tl_flower_pollination(c.handle, vp(xy), 50, None, None, C.byref(po), 37, vp(o), C.byref(cost), C.byref(_capi.TlStats())))
        return (o.tolist(), f32bits(cost.value))

    add("flower_pollination n=50", "flower_pollination", 50, run_fpa,
        lambda xy=xy: (lambda r: (r["tour"].tolist(), f32bits(r["cost"])))(FPO.solve(xy, None, 50, None, epochs=3, n_nearest=3, mutation_probability=0.001, seed=37)),
        record=32)

    xy = K.synth(26, 914)

    def run_gsa(c, xy=xy):
        o = _capi.TlGsaOpts(3, 3, 0)
        return _population(c, c.lib.tl_gravitational_search_population, xy, None, 26, (None, 0), (C.byref(o), 38), 3)

    def want_gsa(xy=xy):
        return _want_population([(lambda r: (r["tour"], r["cost"], r["counters"]["improved"]))(GSO.solve(xy, None, 26, None, epochs=3, n_nearest=3, seed=38, run=r))
                                 for r in range(3)])

    add("gravitational 3 x n=26", "gravitational", 26, run_gsa, want_gsa, count=3, record=32)

    # answered on the host (Swarm4::kHostN = 1): nothing of the context is touched, and no kernel time is left behind
    xy1 = K.synth(1, 915)

    def run_pso_host(c, xy=xy1):
        o = _capi.TlPsoOpts(3, 3)
        return _population(c, c.lib.tl_particle_swarm_population, xy, None, 1, (None, 0), (C.byref(o), 39), 3, host=True)

    add("particle_swarm n=1 (host)", "particle_swarm", 45, run_pso_host,
        lambda xy=xy1: _want_population([(lambda r: (r["tour"], r["cost"], r["counters"]["improved"]))(PSO.solve(xy, None, 1, None, epochs=3, n_nearest=3, seed=39, run=r))
                                         for r in range(3)]) + (0.0, 0.0), count=3)

    # ---- the ant colony (tl_api_aco.hip over swarm_run): three n x n matrices and the ants' tables per run in c->work
    xy = K.synth(18, 916)
    pk = O.dm_build_packed(xy)
    aco = dict(epochs=3, alpha=1.0, beta=2.0, evaporation_rate=0.5, num_ants=6)

    def run_aco(c, xy=xy, pk=pk, n=18, seed=40, host=False):
        return _population(c, c.lib.tl_ant_colony_population, xy, pk, n, (None, 0), (3, 1.0, 2.0, 0.5, 6, seed), 3, moves=False, host=host)

    def want_aco(xy=xy, pk=pk, n=18, seed=40):
        return _want_population([(lambda r: (r["tour"], r["cost"], 0))(ACO.solve(xy, pk, n, None, seed=seed, run=r, **aco)) for r in range(3)], moves=False)

    add("ant_colony matrix 3 x n=18", "ant_colony", 18, run_aco, want_aco, matrix=True, count=3, record=32)
    xy2 = K.synth(2, 917)
    add("ant_colony n=2 (host)", "ant_colony", 35, lambda c: run_aco(c, xy2, None, 2, 41, host=True), lambda: want_aco(xy2, None, 2, 41) + (0.0, 0.0), count=3)

    # ---- the Kohonen map (tl_api_som.hip): cities, schedule, log and checkpoint regions in front of the ring blocks in c->work
    xy = K.synth(21, 918)
    som = dict(epochs=12, learning_rate=0.8, radius_fraction=0.1, neuron_multiplier=8, seed=42, run=0)

    def run_som_trace(c, xy=xy):
        M, cap = 21 * 8, 20
        o, log, ring = np.full(21, NONE32, dtype=np.uint32), np.full((12, 2), NONE32, dtype=np.uint32), np.full(2 * M, np.nan)
        ep, tours, cb = np.full(cap, 7, dtype=np.uint32), np.full((cap, 21), NONE32, dtype=np.uint32), np.full(cap, 7, dtype=np.uint32)
        cost, ln, po = C.c_float(-1.0), C.c_uint32(), _capi.TlSomOpts(12, 8, 0.8, 0.1, 0, 0, 0)
        c.check(c.lib.tl_kohonen_som_trace(c.handle, vp(xy), 21, None, C.byref(po), 42, 0, vp(o), C.byref(cost), C.byref(_capi.TlStats()), vp(log), 12, vp(ring), vp(ep), vp(tours), vp(cb),
                                           cap, C.byref(ln)))
        k = min(int(ln.value), cap)
        return (o.tolist(), f32bits(cost.value), log.tolist(), ring.view(np.uint64).tolist(), [(int(ep[i]), tours[i].tolist(), int(cb[i])) for i in range(k)])

    def want_som_trace(xy=xy):
        res = SOMO.solve(xy, None, 21, **som)
        return (res["tour"].tolist(), f32bits(res["cost"]), SOMO.log_words(res).tolist(), SOMO.ring_words(res).tolist(),
                [(int(t), [int(v) for v in tour], f32bits(cc)) for t, tour, cc in res["checkpoints"]])

    add("kohonen_som traced n=21", "kohonen_som", 21, run_som_trace, want_som_trace)

    # ---- the Fourier curve (tl_api_fourier.hip): basis table, coefficients and sums of every job in c->work
    xy = K.synth(45, 919)
    fo = dict(k_max=2, m=64, lam=0.05, lambda_decay=0.5, lr=0.05, epochs=5)

    def run_fourier(c, xy=xy):
        o, coeffs, cost = np.full(45, NONE32, dtype=np.uint32), np.full(2 * (2 * 2 + 1), np.nan), C.c_float(-1.0)
        po = _capi.TlFourierOpts(2, 64, 5, 0, 0.05, 0.5, 0.05, 0, 0)
        c.check(c.lib.tl_fourier_curve(c.handle, vp(xy), 45, None, C.byref(po), vp(o), C.byref(cost), vp(coeffs), C.byref(_capi.TlStats())))
        return (o.tolist(), f32bits(cost.value), coeffs.view(np.uint64).tolist())

    add("fourier n=45", "fourier", 45, run_fourier,
        lambda xy=xy: (lambda r: ([int(v) for v in r["tour"]], f32bits(r["cost"]), FO.f64_words(r["coeffs"]).tolist()))(FO.solve(xy, None, 45, **fo)))
    return out


def representatives(table):
    """one device job per host path, in the order of GROUPS"""
    by_family = {}
    for k, j in enumerate(table):
        if "(host)" not in j.name:
            by_family.setdefault(j.family, k)
    reps = [by_family[f] for f in REPRESENTATIVES]
    assert [table[k].group for k in reps] == list(GROUPS)
    return reps


def check_coverage(table):
    """the conditions the set as a whole has to meet; raises AssertionError naming the one that is not"""
    device = [j for j in table if "(host)" not in j.name]
    assert sorted(j.family for j in device) == sorted(FAMILIES), "one device job per family"
    assert sum(j.matrix for j in device) >= 5, "at least five matrix-form jobs"
    assert len({j.family for j in device if j.matrix}) >= 5
    assert sum(j.init for j in device) >= 4, "start tours on at least four jobs"
    assert any(j.family == "sim_anneal" and j.init and j.count > 1 for j in device), "init_count == count > 1"
    for rec in (16, 32):
        assert any(j.record == rec and 3 <= j.count <= 8 for j in device), f"several runs with {rec}-byte records"
    assert all(8 <= j.size <= 130 for j in device) and all(j.size <= 14 for j in device if j.family in ("bellman_karp", "branch_and_bound"))
    hosts = [j for j in table if "(host)" in j.name]
    sizes = sorted(j.size for j in device)
    assert hosts and all(sizes[0] < j.size < sizes[-1] for j in hosts), "a host-answered job between device jobs"
    seq = euler_sequence(len(GROUPS))
    g = len(GROUPS)
    assert len(seq) == g * (g - 1) + 1 and {(a, b) for a, b in zip(seq, seq[1:])} == {(a, b) for a in range(g) for b in range(g) if a != b}
    representatives(table)
