"""Instances the gravitational search tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import numpy as np

import _sa_cases as K
from _gsa_oracle import vmax

THREADS = 256  # the workgroup of the epochs (csrc/gravitational_search.hip): one pass of a strided loop


def start_tour(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def triangle():
    """three cities whose every tour has the same cost, exactly: the masses are uniform in every epoch"""
    return np.ascontiguousarray(np.array([[0, 0], [3, 0], [0, 4]], dtype=np.float32))


def instance(n):
    return K.tsplib("berlin52")["xy"] if n == 52 else triangle() if n == 3 else K.small(n) if n <= 8 else K.synth(n, 900 + n)


# name -> (xy, packed, n, init or None, dict(epochs, n_nearest, seed, run)): what goldens_gsa.json freezes
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    return {
        "berlin52": (b["xy"], None, 52, None, dict(epochs=30, n_nearest=3, seed=1, run=0)),
        "berlin52_init_run2": (b["xy"], None, 52, start_tour(52, 2), dict(epochs=20, n_nearest=3, seed=2, run=2)),
        "gr17_matrix": (g["xy"], g["packed"], 17, None, dict(epochs=30, n_nearest=3, seed=4, run=0)),
        "gr17_matrix_init": (g["xy"], g["packed"], 17, start_tour(17, 17), dict(epochs=12, n_nearest=26, seed=6, run=1)),
        "small5": (K.small(5), None, 5, None, dict(epochs=20, n_nearest=3, seed=5, run=0)),
        "small8_init": (K.small(8), None, 8, start_tour(8, 8), dict(epochs=25, n_nearest=31, seed=8, run=0)),
        "synth65": (K.synth(65, 65), None, 65, None, dict(epochs=6, n_nearest=65, seed=65, run=0)),
    }


# The conditions the seeded cases are there for, each read off the oracle's record of a run.  prefix_past_64_positions is not among
# them: two agents that agree on their first 64 positions do not come up in a small seeded run, so the condition is reached through
# tl_gsa_selftest_pull's planted inputs (tests/test_gpu_gravitational_search.py: PLANTED).
CONDITIONS = ("pull_from_moved_lower_j", "pull_from_higher_j_unmoved", "no_live_pull_unchanged", "velocity_truncated_at_vmax", "two_pulls_share_a_position",
              "pulls_cancel", "uniform_mass_epoch", "tie_at_kbest_cut", "gbest_by_agent_0", "gbest_by_last_agent", "two_improvements_in_an_epoch")
PLANTED_ONLY = ("prefix_past_64_positions",)


def conditions(res):
    """which of CONDITIONS the oracle's record of a run shows"""
    N, got = res["agents"], set()
    kb = (N + 1) // 2
    for e, ep in enumerate(res["epochs"]):
        improvers = [i for ee, i, _c, _r in res["improvements"][1:] if ee == e]
        if 0 in improvers:
            got.add("gbest_by_agent_0")
        if N - 1 in improvers:
            got.add("gbest_by_last_agent")
        if len(improvers) >= 2:
            got.add("two_improvements_in_an_epoch")
        m, rank = ep["masses"], ep["rank"]
        assert ep["kbest"] == rank[:kb] and sorted(rank) == list(range(N))
        if ep["uniform"]:
            assert ep["kbest"] == list(range(kb))
            got.add("uniform_mass_epoch")
        elif m[rank[kb - 1]] == m[rank[kb]]:
            assert rank[kb - 1] < rank[kb]
            got.add("tie_at_kbest_cut")
        for i, mv in enumerate(ep["moves"]):
            assert len(mv["velocity"]) == min(mv["wanted"], vmax(len(res["tour"])))
            for p in mv["pulls"]:
                assert p["j"] != i and p["j"] in ep["kbest"] and 1 <= p["n_swaps"] <= 20 and len(p["pairs"]) <= p["n_swaps"]
                if p["moved"]:
                    got.add("pull_from_moved_lower_j")
                if p["j"] > i:
                    assert not p["moved"]
                    got.add("pull_from_higher_j_unmoved")
            if not mv["pulls"]:
                assert mv["unchanged"] and not mv["velocity"]
                got.add("no_live_pull_unchanged")
            if mv["wanted"] > len(mv["velocity"]):
                got.add("velocity_truncated_at_vmax")
            used = [set(q for pr in p["pairs"] for q in pr) for p in mv["pulls"]]
            if any(used[a] & used[b] for a in range(len(used)) for b in range(a + 1, len(used))):
                got.add("two_pulls_share_a_position")
            if mv["velocity"] and mv["unchanged"]:
                got.add("pulls_cancel")
    return got


# name -> (n, init seed or None, opts, the conditions it is there for): picked on the CPU by scanning seeds from 1
def _all_but(*missing):
    return tuple(c for c in CONDITIONS if c not in missing)


SEEDED = {
    "small8": (8, None, dict(epochs=12, n_nearest=3, seed=21, run=0), _all_but("tie_at_kbest_cut", "uniform_mass_epoch")),
    "small5_truncated": (5, None, dict(epochs=12, n_nearest=3, seed=10, run=0), _all_but("two_improvements_in_an_epoch", "uniform_mass_epoch")),  # v_max = 2
    "small6_init": (6, 3, dict(epochs=12, n_nearest=3, seed=10, run=0), _all_but("gbest_by_last_agent", "uniform_mass_epoch")),
    "triangle_uniform": (3, None, dict(epochs=4, n_nearest=3, seed=1, run=0),
                         _all_but("gbest_by_agent_0", "gbest_by_last_agent", "tie_at_kbest_cut", "two_improvements_in_an_epoch")),
    "berlin52_default": (52, None, dict(epochs=10, n_nearest=3, seed=5, run=0), _all_but("tie_at_kbest_cut", "uniform_mass_epoch", "velocity_truncated_at_vmax")),
    "synth130_26_agents": (130, 3, dict(epochs=5, n_nearest=26, seed=1, run=0),
                           ("pull_from_moved_lower_j", "pull_from_higher_j_unmoved", "no_live_pull_unchanged", "two_pulls_share_a_position", "gbest_by_agent_0")),
    "synth600": (600, None, dict(epochs=2, n_nearest=3, seed=1, run=0), ("pull_from_moved_lower_j", "pull_from_higher_j_unmoved", "two_pulls_share_a_position")),
}


def planted_pairs(n):
    """name -> (from, target, prefix length) for tl_gsa_selftest_pull, n >= 300: what a seeded run does not reach.  agree_K: the two
    agree on their first K positions and differ after (a random derangement-like shuffle of the rest), so the prefix starts in a
    later chunk of 64 positions and, for K = 255 and K = 60, crosses a chunk boundary."""
    rng = np.random.default_rng(n)
    base = rng.permutation(n).astype(np.uint32)
    out = {"identical": (base, base.copy(), 20)}
    for k in (60, 64, 70, 255, 256):
        dst = base.copy()
        dst[k:] = np.roll(base[k:], 1)  # one cycle over the rest: every position from k on but the last gives a pair
        out[f"agree_{k}"] = (base, dst, 20)
    out["one_n_cycle_up"] = (base, np.roll(base, -1), 20)   # pi(p) = p + 1: every walk ends at once
    out["one_n_cycle_down"] = (base, np.roll(base, 1), 20)  # pi(p) = p - 1: the walk from p runs down to 0 and wraps to n - 1
    one = base.copy()
    one[[5, n - 3]] = one[[n - 3, 5]]
    out["prefix_1"] = (base, rng.permutation(n).astype(np.uint32), 1)
    out["prefix_20"] = (base, rng.permutation(n).astype(np.uint32), 20)
    out["prefix_0"] = (base, rng.permutation(n).astype(np.uint32), 0)
    out["prefix_above_the_length"] = (base, one, 5)  # one transposition: a sequence of one pair
    sparse = base.copy()  # pairs at 10, 100 and 290 only: the prefix of 3 spans five chunks
    for a in (10, 100, 290):
        sparse[[a, a + 1]] = sparse[[a + 1, a]]
    out["sparse_pairs"] = (base, sparse, 3)
    return out


def seeded_case(name):
    n, init_seed, o, want = SEEDED[name]
    return instance(n), None, n, None if init_seed is None else start_tour(n, init_seed), o, want


def check_conditions(name, n, res, opts):
    """what each golden case is there for, asserted on the oracle's record: no case passes vacuously"""
    N = res["agents"]
    assert len(res["epochs"]) == opts["epochs"] and res["counters"]["moves"] == opts["epochs"] * N
    assert len(res["improvements"]) == 1 + res["counters"]["improved"], name
    assert sorted(res["tour"].tolist()) == list(range(n))
    got = conditions(res)
    assert {"pull_from_moved_lower_j", "pull_from_higher_j_unmoved"} <= got, name
    assert any(mv["velocity"] and not mv["unchanged"] for ep in res["epochs"] for mv in ep["moves"]), name
    if name == "synth65":
        assert N == 65 and len(res["epochs"][0]["kbest"]) == 33  # the ranking walks past one wave of agents; 32 pulls an agent are tried
        assert max(len(mv["pulls"]) for ep in res["epochs"] for mv in ep["moves"]) >= 2, name
