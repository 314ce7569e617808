"""Lin-Kernighan for seeded runs (tl_lk_population): what its CPU and GPU tests share (TEST infrastructure).

THE RUN SEED, restated: run r of seed S is the search tl_lk performs with seed run_seed(S, r) — run 0 is S itself, run r >= 1 is
output 2^63 + r of the splitmix64 stream of S.  The kicks of a search draw outputs below 2^35 of their stream, so the domains are
disjoint, and run 1 of seed 1 is not run 0 of seed 2 as it would be with S + r.

THE CASE TABLE (CASES): every listed run of every case is compared with the oracle, O.lin_kernighan_trace with seed = run_seed(S, r).
The reference's lk_pass can cycle and the oracle does not return from such a pass, so before a case went into
the table every run of it was computed by the oracle on the CPU under a time limit of 60 s; all of them returned, no base seed had to
be discarded.  (The same holds for the runs the GPU tests list outside this table: berlin52 seed 1 runs 0..7, n = 12 seed 9 runs
0..512, n = 40 seed 6 runs 0..9 from the NN seed and runs 0..3 from the random starts, n = 20 seed 1 runs 0..1, burma14 seed 3 runs
0..3.)

THE COMPARISON (check_population): tour, cost bits and the four counters of every run, as assert_same of tests/test_gpu_lk_ils.py.
"""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64_at(seed, k):
    """output k (0-based) of the splitmix64 stream started at `seed`"""
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def run_seed(seed, run):
    return seed & M64 if run == 0 else splitmix64_at(seed & M64, (1 << 63) + run)


def lattice(m, seed):
    g = np.stack(np.meshgrid(np.arange(m, dtype=np.float32), np.arange(m, dtype=np.float32)), -1).reshape(-1, 2)
    return np.ascontiguousarray(g[np.random.default_rng(seed).permutation(len(g))])


def _synth(n, seed):
    import _oracle as O
    return O.synth_xy(n, seed=seed)


def _kw(epochs=20, platoo_epochs=10, n_nearest=5, max_depth=5):
    return dict(epochs=epochs, platoo_epochs=platoo_epochs, n_nearest=n_nearest, max_depth=max_depth)


# name -> (xy, options, base seed S, runs, start tours: "nn" the NN seed | "one" a shared random start | "each" a random start per run)
CASES = {}
for _n in (4, 5, 7, 8, 9, 16):  # n < 8: double_bridge returns the tour as it is (lin_kernighan.rs:487-489)
    CASES[f"n{_n}"] = (lambda n=_n: _synth(n, n), _kw(12, 4, 3), 3, 3, "nn")
for _k in (1, 3, 5, 8):        # the key's digit width: 1, 2, 3, 4 bits
    CASES[f"n64_k{_k}"] = (lambda: _synth(64, 2), _kw(n_nearest=_k), 5, 3, "nn")
for _d in (1, 6):              # (depth 5: every other case)
    CASES[f"n64_depth{_d}"] = (lambda: _synth(64, 2), _kw(max_depth=_d), 5, 3, "each")
CASES["n200"] = (lambda: _synth(200, 4), _kw(10), 1, 3, "nn")       # the last size on 4 waves
CASES["n201"] = (lambda: _synth(201, 6), _kw(10), 2, 3, "each")     # the first on 16; random starts: the runs finish in different slices
CASES["depth8_k2"] = (lambda: _synth(150, 3), _kw(15, n_nearest=2, max_depth=8), 2, 2, "nn")  # the deep build
CASES["lattice10"] = (lambda: lattice(10, 2), _kw(20, 10), 11, 3, "one")                     # ties in every candidate list
CASES["no_epochs"] = (lambda: _synth(64, 2), _kw(0), 5, 2, "one")
CASES["one_epoch"] = (lambda: _synth(64, 2), _kw(1, 1), 5, 2, "nn")


def case_inputs(name):
    """(xy, options, S, runs, start tours as a list of position arrays or None)"""
    import _oracle as O
    make, kw, seed, runs, start = CASES[name]
    xy = make()
    n = len(xy)
    inits = None if start == "nn" else [O.restart_perm(n, 77, r) for r in range(1 if start == "one" else runs)]
    return xy, kw, seed, runs, inits


_oracle_cache = {}


def oracle_run(key, xy, init, seed, kw, packed=None, cap=64):
    """O.lin_kernighan_trace of one run, computed once per process under `key` and left unchanged: (route, cost bits, counters)"""
    import _oracle as O
    if key not in _oracle_cache:
        rc, route, cost, st = O.lin_kernighan_trace(xy, init=init, seed=seed, packed=packed, cap=cap, **kw)[:4]
        assert rc == 0, key
        route.setflags(write=False)
        _oracle_cache[key] = (route, np.float32(cost).tobytes(), (st["sweeps"], st["candidates"], st["moves"], st["reversed"]))
    return _oracle_cache[key]


def start_of(inits, i):
    return None if inits is None else inits[0 if len(inits) == 1 else i]


def check_population(got, key, xy, kw, seed, runs, first_run=0, inits=None, packed=None, cap=64):
    """got: [(route positions, total, stats)] per run of a population call over runs first_run .. first_run + runs - 1; inits as the
    call's (None, one, or one per run of the call).  Every run against the oracle with seed run_seed(seed, run)."""
    assert len(got) == runs
    for i, (route, cost, st) in enumerate(got):
        r = first_run + i
        init = start_of(inits, i)
        okey = (key, r, seed, None if init is None else bytes(np.asarray(init, dtype=np.uint32)))
        oroute, ocost, ocnt = oracle_run(okey, xy, init, run_seed(seed, r), kw, packed, cap)
        what = f"{key}: run {r}"
        assert list(route) == oroute.tolist(), f"{what}: tour differs from the oracle"
        assert np.float32(cost).tobytes() == ocost, what
        assert (st["sweeps"], st["candidates"], st["moves"], st["reversed"]) == ocnt, what
