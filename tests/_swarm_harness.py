"""The GPU test harness of the solvers that share the `Swarm4` trace ABI (csrc/tl_api_swarm.h), written once (TEST infrastructure):
the device calls, the comparison of one run with the oracle's record, and the test bodies that are the same for every such solver.
A solver's test file states a `Swarm` — what differs between the solvers, as data — and its own tests."""
import ctypes as C
import dataclasses
import types
import typing

import numpy as np

import _cs_oracle
import _fpa_oracle
import _gsa_oracle
import _pso_oracle
import _sa_cases as K
from _raw_context import _vp, jitter_context
from _swarm_oracle import bits

WORK = 8 << 30  # the workspace the entries plan with (include/teeline_gpu.h)


@dataclasses.dataclass(frozen=True)
class Swarm:
    stem: str  # tl_<stem>, tl_<stem>_trace, tl_<stem>_population, tl_<stem>_plan
    oracle: types.ModuleType
    opts: typing.Callable  # opts(o, **launch): the entry's options struct
    size: typing.Callable  # the population size of n_nearest
    row: typing.Callable  # the words of an epoch's row, of the population size
    counter: str  # the oracle's counter that the stats' `candidates` equals
    routes: int = 1  # improvements an epoch can log per member: the route capacity a trace asks for
    launch: tuple = ()  # keywords that go to opts() and not to the oracle: how the work is launched

    def entry(self, ctx, suffix=""):
        return getattr(ctx.lib, f"tl_{self.stem}{suffix}")


def _pso_opts(o):
    from teeline_amd import _capi
    return _capi.TlPsoOpts(o["epochs"], o["n_nearest"])


def _cs_opts(o):
    from teeline_amd import _capi
    return _capi.TlCsOpts(o["epochs"], o["n_nearest"], o.get("mutation_probability", 0.001))


def _fpa_opts(o):
    from teeline_amd import _capi
    return _capi.TlFpaOpts(o["epochs"], o["n_nearest"], o.get("mutation_probability", 0.001))


def _gsa_opts(o, span=0):
    from teeline_amd import _capi
    return _capi.TlGsaOpts(o["epochs"], o["n_nearest"], span)


PSO = Swarm("particle_swarm", _pso_oracle, _pso_opts, _pso_oracle.particles, lambda P: 2 * P, "steps")
CS = Swarm("cuckoo_search", _cs_oracle, _cs_opts, _cs_oracle.nests, lambda N: 4 * N, "flights", routes=2)  # (a nest can improve best by a flight and by an abandonment)
FPA = Swarm("flower_pollination", _fpa_oracle, _fpa_opts, _fpa_oracle.flowers, lambda N: 4 * N, "moves")
GSA = Swarm("gravitational_search", _gsa_oracle, _gsa_opts, _gsa_oracle.agents, lambda N: 3 * N + 2, "moves", launch=("span",))
SWARMS = (PSO, CS, FPA, GSA)


def gpu_trace(desc, ctx, xy, packed, n, init, o, cap=4096, route_cap=None, epoch_cap=None, **launch):
    from teeline_amd import _capi
    N = desc.size(o["n_nearest"])
    route_cap = min(4096, 1 + desc.routes * min(o["epochs"], 4096) * N) if route_cap is None else route_cap
    epoch_cap = o["epochs"] if epoch_cap is None else epoch_cap
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.full((max(cap, 1), 4), 0xFFFFFFFF, dtype=np.uint32)
    routes = np.full((max(route_cap, 1), max(n, 1)), 0xFFFFFFFF, dtype=np.uint32)
    elog = np.full((max(epoch_cap, 1), desc.row(N)), 0xFFFFFFFF, dtype=np.uint32)
    cost, ln, st = C.c_float(-1.0), C.c_uint32(), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    po = desc.opts(o, **launch)
    rc = desc.entry(ctx, "_trace")(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), C.byref(po), o["seed"], o.get("run", 0), _vp(out), C.byref(cost), C.byref(st),
                                   _vp(log), cap, C.byref(ln), _vp(routes), route_cap, _vp(elog), epoch_cap)
    return rc, out[:n], np.float32(cost.value), log[:min(ln.value, cap)], ln.value, st.as_dict(), routes[:min(ln.value, route_cap), :n], elog[:min(epoch_cap, o["epochs"])]


def gpu_population(desc, ctx, xy, packed, n, init, init_count, first, count, o, **launch):
    from teeline_amd import _capi
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    moves = np.full(count, 0xFFFFFFFF, dtype=np.uint32)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    po = desc.opts(o, **launch)
    rc = desc.entry(ctx, "_population")(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), init_count, first, count, C.byref(po), o["seed"], _vp(out), _vp(costs),
                                        _vp(moves), C.byref(best), C.byref(st))
    return rc, out, costs, moves, best.value, st.as_dict()


def plan(desc, ctx, n, n_nearest=3, count=1, work=WORK, flags=0):
    info = ctx.device_info()
    N, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    rc = desc.entry(ctx, "_plan")(n, n_nearest, count, info["cus"], info["lds_bytes"], work, flags, C.byref(N), C.byref(t), C.byref(per))
    return rc, N.value, t.value, per.value


def okey(key, n, init, o):
    return (key, n, None if init is None else tuple(int(v) for v in init), tuple(sorted(o.items())))


def compare_run(desc, res, device_record, o, key):
    """a device record (gpu_trace's, after its rc) against the oracle's: every epoch row, every log record and route, tour, cost, stats"""
    out, gcost, glog, ln, st, routes, elog = device_record
    O = desc.oracle
    want = O.epoch_words(res)
    for e in range(o["epochs"]):
        assert elog[e].tolist() == want[e].tolist(), (key, "epoch", e)
    assert ln == len(res["improvements"]) and glog.tolist() == O.log_words(res).tolist(), key
    assert routes.tolist() == O.route_words(res, len(res["tour"])).tolist(), key
    assert out.tolist() == res["tour"].tolist(), key
    assert bits(gcost) == bits(res["cost"]), (key, gcost, res["cost"])
    c = res["counters"]
    assert (st["sweeps"], st["candidates"], st["moves"]) == (o["epochs"], c[desc.counter], c["improved"]), (key, st, c)


def check_run(desc, ctx, key, xy, packed, n, init, o, **kw):
    """one run against the oracle: tour, cost, every log record and route, every epoch row, stats.  Of kw, desc.launch goes to the
    device, the rest (seq) to the oracle."""
    launch = {k: kw.pop(k) for k in desc.launch if k in kw}
    res = desc.oracle.solve_cached(okey(key, n, init, o), xy, packed, n, init, **o, **kw)
    rc, *record = gpu_trace(desc, ctx, xy, packed, n, init, o, **launch)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    compare_run(desc, res, record, o, key)
    return res


def check_population(desc, ctx, xy, n, init, init_count, first, count, sample, o):
    rc, out, costs, moves, best, st = gpu_population(desc, ctx, xy, None, n, init, init_count, first, count, o)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        ini = None if init is None else np.asarray(init).reshape(-1, n)[r if init_count > 1 else 0]
        res = desc.oracle.solve_cached(okey("pop", n, ini, dict(o, run=first + r)), xy, None, n, ini, **dict(o, run=first + r))
        assert out[r].tolist() == res["tour"].tolist() and bits(costs[r]) == bits(res["cost"]) and moves[r] == res["counters"]["improved"], (count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == o["epochs"] * count and st["moves"] == int(moves.sum())
    return out, costs


# ---------------------------------------------------------------- test bodies that are the same for every solver
def plain_entry_defaults_and_truncated_trace(desc, ctx, golden):
    from teeline_amd import _capi
    O = desc.oracle
    xy, _packed_, n, init, o = golden["berlin52"]
    res = O.solve_cached(okey("berlin52", n, init, o), xy, None, n, init, **o)
    out, gcost, st = np.zeros(52, dtype=np.uint32), C.c_float(), _capi.TlStats()
    po = desc.opts(o)
    assert desc.entry(ctx)(ctx.handle, _vp(xy), 52, None, None, C.byref(po), o["seed"], _vp(out), C.byref(gcost), C.byref(st)) == 0
    assert out.tolist() == res["tour"].tolist() and bits(gcost.value) == bits(res["cost"])
    assert (st.sweeps, st.candidates, st.moves) == (o["epochs"], res["counters"][desc.counter], res["counters"]["improved"])
    rc, out2, _c, glog, ln, _st, routes, elog = gpu_trace(desc, ctx, xy, None, 52, None, o, cap=3, route_cap=2, epoch_cap=5)  # truncation is reported
    assert rc == 0 and ln == len(res["improvements"]) > 3 and len(glog) == 3 and len(routes) == 2 and len(elog) == 5 and out2.tolist() == res["tour"].tolist()
    assert glog.tolist() == O.log_words(res, route_cap=2)[:3].tolist() and routes.tolist() == O.route_words(res, 52)[:2].tolist()
    assert elog.tolist() == O.epoch_words(res)[:5].tolist()


def batches(desc, ctx, cases, pop):
    """cases: the solver's cases module (instance, start_tour); pop: the options of the batch"""
    n = 60
    xy = cases.instance(n)
    cus = ctx.device_info()["cus"]
    count = cus + 1
    out, costs = check_population(desc, ctx, xy, n, None, 0, 0, count, [0, 7, cus], pop)
    rc, o1, c1, _m, b1, _ = gpu_population(desc, ctx, xy, None, n, None, 0, 7, 1, pop)  # first_run = 7, count = 1 equals run 7 of the batch
    assert rc == 0 and b1 == 0 and o1[0].tolist() == out[7].tolist() and bits(c1[0]) == bits(costs[7])
    one = cases.start_tour(n, 3)
    check_population(desc, ctx, xy, n, one, 1, 100, 3, [0, 1, 2], pop)
    each = np.stack([cases.start_tour(n, 50 + r) for r in range(3)])
    check_population(desc, ctx, xy, n, each, 3, 5, 3, [0, 1, 2], pop)
    assert gpu_population(desc, ctx, xy, None, n, None, 0, 0, 0, pop)[0] == 0  # count == 0: TL_OK, nothing written


def more_runs_than_one_launch_sequence(desc, ctx, o, small_work):
    """small_work: the workspace in which two runs of n = 60 fit and three do not"""
    n = 3
    xy = K.small(3)
    per = plan(desc, ctx, n, 3, 10 ** 6)[3]
    assert per == 65535 and plan(desc, ctx, 60, 3, 10, small_work)[3] == 2  # a small workspace bounds it, too
    out, costs = check_population(desc, ctx, xy, n, None, 0, 0, per + 1, [0, per - 1, per], o)
    rc, o1, c1, _m, _b, _ = gpu_population(desc, ctx, xy, None, n, None, 0, per, 1, o)
    assert rc == 0 and o1[0].tolist() == out[per].tolist() and bits(c1[0]) == bits(costs[per])


def context_reuse(desc, runs):
    """runs: (key, xy, packed, n, init, o) in turn on one fresh context"""
    import teeline_amd as TA
    with TA.Context(0) as c:
        for key, xy, packed, n, init, o in runs:
            check_run(desc, c, key, xy, packed, n, init, o)


def common_errors(desc, ctx, members):
    """the refusals every entry shares; members: the population's name in the message"""
    import teeline_amd as TA
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    err = lambda: ctx.lib.tl_last_error(ctx.handle).decode()  # noqa: E731
    good = dict(epochs=2, n_nearest=3, seed=1)
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 52
    assert gpu_trace(desc, ctx, b["xy"], None, 52, bad, good)[0] == _capi.TL_ERR_BADARG and "permutation" in err()
    assert gpu_trace(desc, ctx, b["xy"], None, 52, None, dict(good, epochs=2 ** 32 - 1), epoch_cap=0)[0] == _capi.TL_ERR_UNSUPPORTED and "epochs" in err()
    assert gpu_trace(desc, ctx, b["xy"], None, 52, None, dict(good, n_nearest=4097), epoch_cap=0)[0] == _capi.TL_ERR_UNSUPPORTED and members in err()
    assert plan(desc, ctx, 52, 1024)[:3] == (0, 1024, 64) and plan(desc, ctx, 52, 1024)[3] >= 1 and plan(desc, ctx, 52, 4097) == (0, 0, 0, 0)
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = desc.opts(good)
    assert desc.entry(ctx)(ctx.handle, None, 52, None, None, C.byref(po), 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_BADARG
    assert err() == f"tl_{desc.stem}: NULL argument"
    assert gpu_population(desc, ctx, b["xy"], None, 52, None, 0, 2 ** 32 - 3, 6, good)[0] == _capi.TL_ERR_BADARG
    assert err() == f"tl_{desc.stem}_population: run ids beyond 2^32 - 1"
    assert gpu_population(desc, ctx, b["xy"], None, 52, np.arange(104, dtype=np.uint32) % 52, 2, 0, 6, good)[0] == _capi.TL_ERR_BADARG and "init_count" in err()
    ln = C.c_uint32()
    assert desc.entry(ctx, "_trace")(ctx.handle, _vp(b["xy"]), 52, None, None, C.byref(po), 1, 0, _vp(out), C.byref(cost), None, None, 4, C.byref(ln), None, 0,
                                     None, 0) == _capi.TL_ERR_BADARG
    assert plan(desc, ctx, 52, 3, 1, WORK, 1 << 31)[0] == _capi.TL_ERR_UNSUPPORTED
    with TA.Context(0, 1 << 31) as odd:  # a bit no flag has
        assert gpu_trace(desc, odd, b["xy"], None, 52, None, good)[0] == _capi.TL_ERR_UNSUPPORTED


def jitter(desc, more=None):
    """a context of the race-stress build with the solver's trace entry bound (and `more`: {entry: argtypes}); close() it"""
    from teeline_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    opts = type(desc.opts(dict(epochs=0, n_nearest=0)))
    trace = [vp, vp, u32, vp, vp, C.POINTER(opts), u64, u32, vp, C.POINTER(f32), C.POINTER(_capi.TlStats), vp, u32, C.POINTER(u32), vp, u32, vp, u32]
    return jitter_context({f"tl_{desc.stem}_trace": trace, **(more or {})})
