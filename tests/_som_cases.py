"""The cases of the Kohonen map solver (TEST infrastructure): what goldens_som.json freezes and what the GPU tests run, each with the
condition it is there for, checked on the oracle's record (tests/_som_oracle.py)."""
import hashlib

import numpy as np

import _sa_cases as K
import _som_oracle as SO

LDS_BYTES = 163840        # an MI355X workgroup's LDS
LDS_FIXED = 512           # the reduction's slots (csrc/tl_kernels.h)
LDS_MAX_NEURONS = (LDS_BYTES - LDS_FIXED) // 16


def threads_of(M):
    """the plan's rule: about eight neurons a lane, in whole waves"""
    return min(1024, max(64, (((M + 7) // 8 + 63) // 64) * 64))


def o(epochs, mult=1, lr=0.8, rf=0.1, seed=1, run=0):
    return dict(epochs=epochs, neuron_multiplier=mult, learning_rate=lr, radius_fraction=rf, seed=seed, run=run)


def line(n):
    """all cities on one vertical line: the x span is 1e-9"""
    xy = K.small(n).copy()
    xy[:, 0] = 250.0
    return xy


def duplicates(n):
    """every city twice (and one three times): extraction ties go by the city index"""
    a = K.small(n)
    return np.ascontiguousarray(np.concatenate([a, a, a[:1]]))


def circle(n, ids=None):
    """the reference's own unit-test instance (som.rs:194-204): f32 cos and sin"""
    i = np.arange(n, dtype=np.float32)
    th = np.float32(2.0) * np.float32(np.pi) * i / np.float32(n)
    return np.ascontiguousarray(np.stack([np.cos(th, dtype=np.float32), np.sin(th, dtype=np.float32)], axis=1))


# name -> (xy, packed, n, opts, conditions).  Every M below threads_of(M) * 8 etc. is pinned by test_cases_cover_the_sizes.
def cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    out = {}
    for n in (2, 3, 5, 7):
        out[f"n{n}_mult1"] = (K.small(n), None, n, o(25, seed=n), ("floor_from_epoch_1",))
    out["M63"] = (K.small(21), None, 21, o(25, 3, seed=63), ())
    out["M64"] = (K.small(8), None, 8, o(25, 8, seed=64), ())
    out["M65"] = (K.small(13), None, 13, o(25, 5, seed=65), ())
    out["M129"] = (K.small(43), None, 43, o(25, 3, seed=129), ())
    out["M513_two_waves"] = (K.small(171), None, 171, o(12, 3, seed=513), ())
    out["M1025_three_waves"] = (K.small(205), None, 205, o(12, 5, seed=1025), ())
    out["berlin52"] = (b["xy"], None, 52, o(40, 8, seed=1), ())
    out["M20_floor_crossed"] = (K.small(20), None, 20, o(25, seed=20), ("floor_crossed",))
    out["rf1_even"] = (K.small(20), None, 20, o(11, rf=1.0, seed=2), ("window_wider_than_ring", "opposite_neuron"))
    out["rf1_odd"] = (K.small(21), None, 21, o(11, rf=1.0, seed=3), ("window_wider_than_ring",))
    out["rf_small"] = (b["xy"], None, 52, o(20, 8, rf=0.005, seed=4), ("most_skipped_by_cut",))
    for e in (1, 9, 10, 11, 25):
        out[f"epochs{e}"] = (K.small(13), None, 13, o(e, 5, seed=100 + e), ("final_path_update" if e % max(e // 10, 1) else "no_final_path_update",))
    out["duplicates"] = (duplicates(6), None, 13, o(25, 4, seed=6), ("equal_neuron_and_distance",))
    out["vertical_line"] = (line(9), None, 9, o(25, 6, seed=9), ())
    out["gr17_matrix"] = (g["xy"], g["packed"], 17, o(25, 8, seed=17), ())
    out["run3"] = (K.small(13), None, 13, o(25, 5, seed=65, run=3), ())
    return out


GOLDEN = ("n2_mult1", "n7_mult1", "M65", "berlin52", "M20_floor_crossed", "rf1_even", "rf1_odd", "epochs11", "duplicates", "vertical_line", "gr17_matrix", "run3")


def check_conditions(name, res, opts, want):
    M = res["neurons"]
    sched = [SO.schedule(t, opts["epochs"], M, opts["learning_rate"], opts["radius_fraction"]) for t in range(1, opts["epochs"] + 1)]
    sig = [s[1] for s in sched]
    for w in want:
        if w == "floor_from_epoch_1":
            assert all(s == 1.0 for s in sig), name
        elif w == "floor_crossed":
            assert sig[0] > 1.0 and sig[-1] == 1.0, name
        elif w == "window_wider_than_ring":
            assert any(2 * s[3] + 1 > M for s in sched) and max(res["moved"]) == M, name
        elif w == "opposite_neuron":
            assert M % 2 == 0 and max(res["moved"]) == M, name  # the single neuron at distance M / 2 is moved, once
        elif w == "most_skipped_by_cut":
            assert max(res["moved"]) * 8 < M and all(s[3] * 4 < M for s in sched), name
        elif w == "final_path_update":
            assert res["checkpoints"][-1][0] == SO.NONE, name
        elif w == "no_final_path_update":
            assert res["checkpoints"][-1][0] == opts["epochs"], name
        elif w == "equal_neuron_and_distance":
            bm = res["bm"]
            assert any(bm[a] == bm[a + 6] for a in range(6)), name
        else:
            raise AssertionError(w)


def planted_ties(M, threads):
    """name -> (ring [M, 2], cities [k, 2]): exact ties of the minimum distance for tl_som_selftest_bmu.  Every neuron is far away
    (distance^2 = 2) but the planted ones, which sit at distance^2 = 0.25 of city 0 = (0.5, 0.5): (0.5, 0) and (0, 0.5) and (1, 0.5)
    are at EQUAL distance — different points, the same f64 — and -0.0 stands against +0.0 in a coordinate."""
    far = np.full((M, 2), 1.5)
    city = np.array([[0.5, 0.5]])
    spots = [(0.5, 0.0), (0.0, 0.5), (1.0, 0.5), (0.5, -0.0), (-0.0, 0.5)]
    out = {}

    def plant(name, idx):
        r = far.copy()
        for k, i in enumerate(idx):
            r[i] = spots[k % len(spots)]
        out[name] = (r, city, min(idx))

    plant("first_and_last", [M - 1, 0])
    if M > 2:
        plant("last_two", [M - 1, M - 2])
    if M > 64:
        plant("astride_a_wave", [64, 63])
    if M > 65:
        plant("lane_seam", [65, 1])                    # two lanes of different waves
    if M > threads:
        plant("ownership_seam", [threads, 0])          # the same lane's first and second neuron
    if M > threads + 1:
        plant("ownership_seam_2", [threads + 1, threads - 1, 1])
    if M > 2 * threads:
        plant("third_trip", [2 * threads, threads - 1])
    plant("all_equal", list(range(M)))
    return out


def ranking_ties():
    """(ring, cities): cities that share (neuron, distance) — mirror images about a neuron, duplicates, +0.0 / -0.0 — so that the
    extraction's order falls to the city index"""
    ring = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.5], [-0.0, 1.0]])
    cities = np.array([[0.75, 0.5], [0.25, 0.5], [0.5, 0.75], [0.5, 0.25], [0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [1.0, 1.0], [0.75, 0.5], [0.0, 1.0], [0.1, 0.9],
                       [0.1, 0.1], [0.9, 0.9]])
    return ring, cities


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=dtype)).astype(np.dtype(dtype).newbyteorder("<")).tobytes()).hexdigest()


def case_record(res):
    """what goldens_som.json freezes of a run"""
    return {"tour": [int(v) for v in res["tour"]], "cost_bits": SO.bits(res["cost"]), "log_sha256": sha(SO.log_words(res), np.uint32),
            "log_head": SO.log_words(res)[:4].tolist(), "ring_sha256": sha(SO.ring_words(res), np.uint64), "ring_head": [str(int(v)) for v in SO.ring_words(res)[:2]],
            "checkpoints": [[int(t), [int(v) for v in tour], SO.bits(c)] for t, tour, c in res["checkpoints"]], "moved": [int(v) for v in res["moved"]]}
