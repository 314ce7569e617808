"""Instances the cuckoo search tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import numpy as np

import _sa_cases as K

THREADS = 256  # the widest workgroup (csrc/cuckoo_search.hip: cuckoo_search_threads): one pass of a strided loop


def start_tour(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def instance(n):
    return K.tsplib("berlin52")["xy"] if n == 52 else K.small(n) if n <= 8 else K.synth(n, 700 + n)


# name -> (xy, packed, n, init or None, dict(epochs, n_nearest, mutation_probability, seed, run)): what goldens_cs.json freezes
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    return {
        "berlin52": (b["xy"], None, 52, None, dict(epochs=40, n_nearest=3, mutation_probability=0.001, seed=1, run=0)),
        "berlin52_init_run2": (b["xy"], None, 52, start_tour(52, 2), dict(epochs=30, n_nearest=3, mutation_probability=0.001, seed=2, run=2)),
        "gr17_matrix": (g["xy"], g["packed"], 17, None, dict(epochs=40, n_nearest=3, mutation_probability=0.5, seed=4, run=0)),
        "small5": (K.small(5), None, 5, None, dict(epochs=20, n_nearest=3, mutation_probability=0.5, seed=5, run=0)),
        "small8_init": (K.small(8), None, 8, start_tour(8, 8), dict(epochs=25, n_nearest=31, mutation_probability=0.001, seed=8, run=0)),
        "synth65": (K.synth(65, 65), None, 65, None, dict(epochs=8, n_nearest=65, mutation_probability=0.25, seed=65, run=0)),
    }


# The conditions the seeded cases are there for, each read off the oracle's record of a run
CONDITIONS = ("fly_again_accepted", "two_fly_again_accepted_in_an_epoch", "chain", "c_equals_t", "accepted_leaves_best", "accepted_improves_best",
              "best_improved_by_abandonment", "best_nest_abandoned_best_stands", "replaced_then_abandoned", "k_one", "k_half_n", "k_above_256",
              "whole_tour_reversal", "adjacent_reversal")


def conditions(res, n):
    """which of CONDITIONS the oracle's record of a run shows"""
    N, got = res["nests"], set()
    flights = {(e, s) for e, s, _c, _r in res["improvements"][1:] if s < N}
    if any(s >= N for _e, s, _c, _r in res["improvements"][1:]):
        got.add("best_improved_by_abandonment")
    for e, ep in enumerate(res["epochs"]):
        writer = {}  # nest -> the cuckoo whose accepted flight wrote it last (this epoch)
        chained = set()  # cuckoos that flew from a tour written by a cuckoo that had itself flown again
        hits = 0
        for c in range(N):
            t, acc, again = ep["targets"][c], ep["accepted"][c], ep["again"][c]
            assert again == (c in writer)
            if again and writer[c] < c and ep["again"][writer[c]]:
                chained.add(c)  # c' -> t -> t': nest c was written by a cuckoo that flew from a nest written in this epoch
            if again and acc and writer[c] < c:
                hits += 1  # a flight accepted into a higher-index nest whose cuckoo then flies from the new tour and is itself accepted
            if acc:
                writer[t] = c
                got.add("accepted_improves_best" if (e, c) in flights else "accepted_leaves_best")
                if t == c:
                    got.add("c_equals_t")
                if ep["abandoned"][t]:
                    got.add("replaced_then_abandoned")
            k = ep["ks"][c]
            if k == 1:
                got.add("k_one")
            if k == n // 2 and n // 2 > 1:
                got.add("k_half_n")
            if k > 256:
                got.add("k_above_256")
            if (0, n - 1) in ep["pairs"][c]:
                got.add("whole_tour_reversal")
            if any(j == i + 1 for i, j in ep["pairs"][c]):
                got.add("adjacent_reversal")
        if hits >= 1:
            got.add("fly_again_accepted")
        if hits >= 2:
            got.add("two_fly_again_accepted_in_an_epoch")
        if chained:
            got.add("chain")
        if ep["orphaned"]:
            got.add("best_nest_abandoned_best_stands")
    return got


# name -> (n, init seed or None, opts, the conditions it is there for): picked on the CPU by scanning seeds from 1
_FLY = ("fly_again_accepted", "two_fly_again_accepted_in_an_epoch", "chain", "c_equals_t", "accepted_leaves_best", "accepted_improves_best", "replaced_then_abandoned",
        "k_one", "k_half_n", "adjacent_reversal")
SEEDED = {
    "small8_every_condition": (8, None, dict(epochs=12, n_nearest=3, mutation_probability=0.5, seed=2, run=0), tuple(c for c in CONDITIONS if c != "k_above_256")),
    "small6_init_every_condition": (6, 3, dict(epochs=12, n_nearest=3, mutation_probability=0.25, seed=15, run=0),
                                    tuple(c for c in CONDITIONS if c != "k_above_256")),
    "berlin52_default_pa": (52, None, dict(epochs=12, n_nearest=3, mutation_probability=0.001, seed=26, run=0),
                            _FLY + ("best_nest_abandoned_best_stands", "whole_tour_reversal")),
    "synth130_26_nests": (130, 3, dict(epochs=6, n_nearest=26, mutation_probability=0.001, seed=1, run=0), _FLY),
    "synth600_long_flights": (600, None, dict(epochs=2, n_nearest=3, mutation_probability=0.001, seed=4, run=0), _FLY + ("k_above_256",)),
}


def seeded_case(name):
    n, init_seed, o, want = SEEDED[name]
    return instance(n), None, n, None if init_seed is None else start_tour(n, init_seed), o, want


def check_conditions(name, n, res, opts):
    """what each golden case is there for, asserted on the oracle's record: no case passes vacuously"""
    N = res["nests"]
    assert len(res["epochs"]) == opts["epochs"] and res["counters"]["flights"] == opts["epochs"] * N
    assert len(res["improvements"]) == 1 + res["counters"]["improved"], name
    assert sorted(res["tour"].tolist()) == list(range(n))
    assert any(any(ep["accepted"]) for ep in res["epochs"]), name
    if name in ("gr17_matrix", "small5", "synth65"):
        assert any(any(ep["abandoned"]) for ep in res["epochs"]), name
    if name == "synth65":
        assert N == 65  # the commit walks past one wave of nests
