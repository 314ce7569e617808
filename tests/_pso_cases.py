"""Instances the particle swarm tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import numpy as np

import _sa_cases as K

THREADS = 256  # the widest workgroup (csrc/particle_swarm.hip: particle_swarm_threads): one pass of a strided loop


def start_tour(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def instance(n):
    return K.tsplib("berlin52")["xy"] if n == 52 else K.small(n) if n <= 8 else K.synth(n, 700 + n)


# name -> (xy, packed, n, init or None, dict(epochs, n_nearest, seed, run)): what goldens_pso.json freezes
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    return {
        "berlin52": (b["xy"], None, 52, None, dict(epochs=40, n_nearest=3, seed=1, run=0)),
        "berlin52_init_run2": (b["xy"], None, 52, start_tour(52, 2), dict(epochs=30, n_nearest=3, seed=2, run=2)),
        "gr17_matrix": (g["xy"], g["packed"], 17, None, dict(epochs=40, n_nearest=3, seed=4, run=0)),
        "small5": (K.small(5), None, 5, None, dict(epochs=20, n_nearest=3, seed=5, run=0)),
        "small8_init": (K.small(8), None, 8, start_tour(8, 8), dict(epochs=25, n_nearest=31, seed=8, run=0)),
        "synth65": (K.synth(65, 65), None, 65, None, dict(epochs=8, n_nearest=65, seed=65, run=0)),
    }


# The conditions the issue names, each met by a seeded case below (chosen on the CPU with the oracle) and asserted from its record.
# "Truncation cutting inside the inertia part" is not among them because it cannot happen: inertia_keep is clamped to len(v), and
# len(v) <= v_max always (every velocity is the result of a truncation), so the inertia part never reaches past v_max.
CONDITIONS = ("two_improvements_in_an_epoch", "improvement_by_particle_0", "improvement_by_the_last_particle", "cut_in_cog", "cut_in_soc", "no_cut",
              "keep_zero", "keep_above_length", "later_particle_sees_new_gbest", "keep_exactly_half_above_even")


def conditions(res):
    """which of CONDITIONS the oracle's record of a run shows"""
    P, got = res["particles"], set()
    imp = res["improvements"][1:]
    per_epoch = {}
    for e, i, _c, _r in imp:
        per_epoch.setdefault(e, []).append(i)
        if i == 0:
            got.add("improvement_by_particle_0")
        if i == P - 1:
            got.add("improvement_by_the_last_particle")
    for e, who in per_epoch.items():
        if len(who) >= 2:
            got.add("two_improvements_in_an_epoch")
        if who[0] < P - 1:
            got.add("later_particle_sees_new_gbest")
    for ep in res["epochs"]:
        for s in ep["steps"]:
            got.add({None: "no_cut", "cog": "cut_in_cog", "soc": "cut_in_soc"}[s["cut"]])
            if any(k == 0 and ln > 0 for k, ln in zip(s["keeps"], s["lens"])):
                got.add("keep_zero")
            if any(k > ln for k, ln in zip(s["keeps"], s["lens"])):
                got.add("keep_above_length")
            if any(x - int(x) == 0.5 and int(x) % 2 == 0 for x in s["xs"]):  # where half-to-even rounding would differ
                got.add("keep_exactly_half_above_even")
            assert s["parts"][0] <= s["lens"][0] <= res["vmax"]  # (why a cut inside the inertia part cannot happen)
    return got


# name -> (n, init seed or None, opts, the conditions it is there for)
SEEDED = {
    "small8_every_condition": (8, 3, dict(epochs=12, n_nearest=30, seed=8, run=0), CONDITIONS[:-1]),
    "synth130_every_condition": (130, 3, dict(epochs=12, n_nearest=31, seed=6, run=0), CONDITIONS[:-1]),
    # 10 epochs: w = 0.9 - 0.5 (8 / 10) is exactly 0.5 in epoch 8, so every odd velocity length gives a product ending in .5
    "synth20_exact_halves": (20, None, dict(epochs=10, n_nearest=30, seed=1, run=0), ("keep_exactly_half_above_even",)),
    "berlin52_particle_0": (52, 3, dict(epochs=12, n_nearest=30, seed=8, run=0), ("improvement_by_particle_0", "two_improvements_in_an_epoch")),
    "berlin52_last_particle": (52, None, dict(epochs=12, n_nearest=30, seed=7, run=0), ("improvement_by_the_last_particle", "two_improvements_in_an_epoch")),
}


def seeded_case(name):
    n, init_seed, o, want = SEEDED[name]
    return instance(n), None, n, None if init_seed is None else start_tour(n, init_seed), o, want


def check_conditions(name, n, res, opts):
    """what each golden case is there for, asserted on the oracle's record: no case passes vacuously"""
    assert len(res["epochs"]) == opts["epochs"] and res["counters"]["steps"] == opts["epochs"] * res["particles"]
    assert len(res["improvements"]) == 1 + res["counters"]["improved"], name
    assert res["counters"]["improved"] >= 1 or name == "small5", name  # (30 shuffles of 5 cities: the start gbest is already a best tour)
    assert sorted(res["tour"].tolist()) == list(range(n))
    if name == "synth65":
        assert res["particles"] == 65  # the commit walks past one wave of particles
