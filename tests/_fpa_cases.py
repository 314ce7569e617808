"""Instances the flower pollination tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import numpy as np

import _sa_cases as K

THREADS = 256  # the widest workgroup (csrc/flower_pollination.hip: flower_pollination_threads): one pass of a strided loop


def start_tour(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def instance(n):
    return K.tsplib("berlin52")["xy"] if n == 52 else K.small(n) if n <= 8 else K.synth(n, 900 + n)


# name -> (xy, packed, n, init or None, dict(epochs, n_nearest, mutation_probability, seed, run)): what goldens_fpa.json freezes
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    return {
        "berlin52": (b["xy"], None, 52, None, dict(epochs=40, n_nearest=3, mutation_probability=0.001, seed=1, run=0)),
        "berlin52_init_run2": (b["xy"], None, 52, start_tour(52, 2), dict(epochs=30, n_nearest=3, mutation_probability=0.5, seed=2, run=2)),
        "gr17_matrix": (g["xy"], g["packed"], 17, None, dict(epochs=40, n_nearest=3, mutation_probability=0.25, seed=4, run=0)),
        "small5": (K.small(5), None, 5, None, dict(epochs=20, n_nearest=3, mutation_probability=0.5, seed=5, run=0)),
        "small8_init": (K.small(8), None, 8, start_tour(8, 8), dict(epochs=25, n_nearest=31, mutation_probability=0.01, seed=8, run=0)),
        "synth65": (K.synth(65, 65), None, 65, None, dict(epochs=8, n_nearest=65, mutation_probability=0.25, seed=65, run=0)),
    }


# The conditions the seeded cases are there for, each read off the oracle's record of a run
CONDITIONS = ("global_again_differs", "local_again_j", "local_again_k", "local_partners_above_accepted_later", "chain", "gbest_by_flower_0",
              "gbest_by_last_flower", "two_improvements_in_an_epoch", "global_empty_unchanged", "local_empty_unchanged", "prefix_one", "prefix_whole_levy_2",
              "prefix_above_256", "local_accepted", "global_accepted")


def conditions(res):
    """which of CONDITIONS the oracle's record of a run shows"""
    N, got = res["flowers"], set()
    for e, ep in enumerate(res["epochs"]):
        mv = ep["moves"]
        improvers = [i for ee, i, _c, _r in res["improvements"][1:] if ee == e]
        if 0 in improvers:
            got.add("gbest_by_flower_0")
        if N - 1 in improvers:
            got.add("gbest_by_last_flower")
        if len(improvers) >= 2:
            got.add("two_improvements_in_an_epoch")
        for i, m in enumerate(mv):
            earlier = lambda q: q < i and mv[q]["accepted"]  # noqa: E731
            assert m["again"] == (any(q < i for q in improvers) if m["glob"] else (earlier(m["j"]) or earlier(m["k"])))
            if m["accepted"]:
                got.add("global_accepted" if m["glob"] else "local_accepted")
            if m["len"] == 0:
                assert not m["accepted"] and m["prefix"] == 0
                got.add("global_empty_unchanged" if m["glob"] else "local_empty_unchanged")
            if m["glob"] and m["again"] and m["differs"]:
                got.add("global_again_differs")
            if not m["glob"] and earlier(m["j"]):
                got.add("local_again_j")
            if not m["glob"] and earlier(m["k"]):
                got.add("local_again_k")
            if not m["glob"] and m["j"] > i and m["k"] > i and mv[m["j"]]["accepted"] and mv[m["k"]]["accepted"]:
                assert not m["again"]
                got.add("local_partners_above_accepted_later")
            if m["again"] and m["accepted"]:  # a flower built again and accepted, which makes a later one be built again
                for q in range(i + 1, N):
                    if (mv[q]["glob"] and i in improvers) or (not mv[q]["glob"] and i in (mv[q]["j"], mv[q]["k"])):
                        assert mv[q]["again"]
                        got.add("chain")
            if m["len"] > 1 and m["prefix"] == 1:
                got.add("prefix_one")
            if m["glob"] and m["len"] > 1 and m["prefix"] == m["len"] and m["levy"] >= 2.0:
                got.add("prefix_whole_levy_2")
            if m["prefix"] > 256:
                got.add("prefix_above_256")
    return got


# name -> (n, init seed or None, opts, the conditions it is there for): picked on the CPU by scanning seeds from 1
_MOST = tuple(c for c in CONDITIONS if c not in ("prefix_above_256", "local_empty_unchanged"))
SEEDED = {
    "small8_every_condition": (8, None, dict(epochs=12, n_nearest=3, mutation_probability=0.5, seed=49, run=0), _MOST),
    "small6_init_every_condition": (6, 3, dict(epochs=12, n_nearest=3, mutation_probability=0.5, seed=17, run=0),
                                    tuple(c for c in _MOST if c != "gbest_by_last_flower")),
    "small3_empty_local": (3, None, dict(epochs=4, n_nearest=3, mutation_probability=0.5, seed=1, run=0), ("local_empty_unchanged", "global_empty_unchanged")),
    "berlin52_default": (52, None, dict(epochs=12, n_nearest=3, mutation_probability=0.001, seed=15, run=0), _MOST),
    "synth130_26_flowers": (130, 3, dict(epochs=6, n_nearest=26, mutation_probability=0.01, seed=1, run=0),
                            ("local_again_j", "local_again_k", "local_partners_above_accepted_later", "chain", "local_accepted")),
    "synth600_long_prefixes": (600, None, dict(epochs=2, n_nearest=3, mutation_probability=0.5, seed=2, run=0),
                               ("prefix_above_256", "global_again_differs", "local_again_j", "local_again_k", "global_accepted", "local_accepted")),
    "berlin52_all_global": (52, 5, dict(epochs=8, n_nearest=3, mutation_probability=1.0, seed=1, run=0),
                            ("global_again_differs", "global_empty_unchanged", "global_accepted", "prefix_whole_levy_2")),
}


def seeded_case(name):
    n, init_seed, o, want = SEEDED[name]
    return instance(n), None, n, None if init_seed is None else start_tour(n, init_seed), o, want


def check_conditions(name, n, res, opts):
    """what each golden case is there for, asserted on the oracle's record: no case passes vacuously"""
    N = res["flowers"]
    assert len(res["epochs"]) == opts["epochs"] and res["counters"]["moves"] == opts["epochs"] * N
    assert len(res["improvements"]) == 1 + res["counters"]["improved"], name
    assert sorted(res["tour"].tolist()) == list(range(n))
    assert any(m["accepted"] for ep in res["epochs"] for m in ep["moves"]), name
    assert any(m["again"] for ep in res["epochs"] for m in ep["moves"]), name
    kinds = {m["glob"] for ep in res["epochs"] for m in ep["moves"]}
    assert kinds == {True, False}, name
    if name == "synth65":
        assert N == 65  # the commit walks past one wave of flowers
