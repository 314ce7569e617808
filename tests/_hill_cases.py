"""The cases of the stochastic hill climb (TEST infrastructure): what goldens_hill.json freezes and what the GPU tests run, each with
the conditions it is there for, checked on the oracle's counters and on its window record (tests/_hill_oracle.py), so that no case
passes vacuously.  Seeds were picked on the CPU with the oracle until each condition held."""
import hashlib

import numpy as np

import _hill_oracle as HO
import _sa_cases as K
from _sa_oracle import chain_key, pair_from_key

WINDOWS = (64, 256)  # one wave per chain, and a chain alone on its CU


def start(n, s):
    """a shuffled start tour: the specification's own Fisher-Yates under a key of its own"""
    t = np.arange(n, dtype=np.int64)
    HO.shuffle(chain_key(s, 99), 0, n, t)
    return t.astype(np.uint32)


def o(epochs, platoo, seed, chain=0):
    return dict(epochs=epochs, platoo_epochs=platoo, seed=seed, chain=chain)


# name -> (xy, packed, n, init or None, opts, conditions)
def cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    bx = b["xy"]
    out = {}
    out["small2"] = (K.small(2), None, 2, None, o(200, 500, 2), ("never_accepted", "from_eq_to"))
    out["small3"] = (K.small(3), None, 3, start(3, 3), o(200, 500, 3), ("from_eq_to", "closing_pair"))
    out["small4"] = (K.small(4), None, 4, start(4, 4), o(200, 500, 1), ("from_eq_to", "closing_pair"))
    out["small5"] = (K.small(5), None, 5, start(5, 5), o(200, 500, 12), ("from_eq_to", "closing_pair"))
    out["small8"] = (K.small(8), None, 8, start(8, 8), o(200, 500, 8), ("closing_accept",))
    out["small5_p1"] = (K.small(5), None, 5, start(5, 5), o(200, 1, 1), ("accept_after_restart",))
    out["small5_p2"] = (K.small(5), None, 5, start(5, 5), o(200, 2, 1), ("accept_after_restart",))
    out["small8_p1"] = (K.small(8), None, 8, start(8, 8), o(200, 1, 1), ("accept_after_restart",))
    out["small8_p2"] = (K.small(8), None, 8, start(8, 8), o(200, 2, 1), ("accept_after_restart",))
    out["gr17_matrix"] = (g["xy"], g["packed"], 17, start(17, 17), o(300, 40, 17), ("restarts", "accepts"))
    out["berlin52_order"] = (bx, None, 52, None, o(600, 500, 1), ("two_accepts_in_256", "no_restart"))
    out["berlin52_p7"] = (bx, None, 52, start(52, 1), o(600, 7, 1), ("restart_before_accept", "accept_before_restart"))
    out["berlin52_p0"] = (bx, None, 52, start(52, 2), o(600, 0, 2), ("no_restart", "accepts"))
    out["berlin52_p300"] = (bx, None, 52, start(52, 3), o(3000, 300, 4), ("restarts", "stale_carried_into_restart", "stale_carried_into_accept"))
    out["berlin52_chain5"] = (bx, None, 52, start(52, 1), o(600, 7, 1, chain=5), ("restarts", "accepts"))
    for p in (63, 64, 255, 256):
        out[f"small4_p{p}"] = (K.small(4), None, 4, start(4, 4), o(1100, p, 4), (f"restart_at_last_lane:{p + 1}" if p in (63, 255) else f"restart_at_lane_0:{p}",))
    out["last_epoch_restart"] = (K.small(5), None, 5, start(5, 5), o(11, 4, 5), ("restart_on_last_epoch",))
    for e in (40, 63, 255, 300):
        out[f"berlin52_e{e}"] = (bx, None, 52, start(52, 1), o(e, 7, 1), ("restarts", "accepts") if e > 64 else ("accepts",))
    return out


def run(name, case=None):
    xy, packed, n, init, opts, _want = case or cases()[name]
    return HO.solve_cached((name,), xy, packed, n, init, **opts)


def window_record(name, W, case=None):
    xy, packed, n, init, opts, _want = case or cases()[name]
    res, rec = HO.windows(xy, packed, n, init, W=W, **opts)
    ref = run(name, case)
    assert res["log"] == ref["log"] and res["cost"] == ref["cost"] and np.array_equal(res["tour"], ref["tour"]), (name, W)
    return rec


def check_conditions(name, case=None):
    xy, packed, n, init, opts, want = case or cases()[name]
    res = run(name, case)
    c = res["counters"]
    key = chain_key(opts["seed"], opts["chain"])
    pairs = [pair_from_key(key, e, n) for e in range(opts["epochs"] + 1)]
    acc = [r for r in res["log"] if r[1] != HO.NONE]
    recs = {}

    def rec(W):
        if W not in recs:
            recs[W] = window_record(name, W, case)
        return recs[W]

    assert res["epochs_run"] == opts["epochs"] + 1, name
    for w in want:
        if w == "never_accepted":
            assert c["accepts"] == 0, name
        elif w == "accepts":
            assert c["accepts"] >= 2, name
        elif w == "restarts":
            assert c["restarts"] >= 1, name
        elif w == "no_restart":
            assert c["restarts"] == 0, name
        elif w == "from_eq_to":
            assert any(f == t for f, t in pairs), name
        elif w == "closing_pair":
            assert any(f == 0 for f, t in pairs) and any(t == n - 1 for f, t in pairs), name
        elif w == "closing_accept":
            assert any(f == 0 or t == n - 1 for _e, f, t, _c in acc) and any(f > 0 and t < n - 1 for _e, f, t, _c in acc), name
        elif w == "accept_after_restart":
            assert c["accepts_after_restart"] >= 1, name
        elif w == "two_accepts_in_256":
            assert c["max_accepts_in_256"] >= 2, name
        elif w == "restart_on_last_epoch":
            assert c["restart_on_last_epoch"] == 1 and res["log"][-1][:2] == (opts["epochs"], HO.NONE), name
        elif w == "restart_before_accept":  # a later lane of the window would have accepted: its verdict is thrown away
            for W in WINDOWS:
                assert any(out == "restart" and a is not None and a > r for _e0, _s, a, r, out in rec(W)), (name, W)
        elif w == "accept_before_restart":
            for W in WINDOWS:
                assert any(out == "accept" and r is not None and a < r for _e0, _s, a, r, out in rec(W)), (name, W)
                assert any(out == "accept" and a == r for _e0, _s, a, r, out in rec(W)), (name, W)  # the acceptance on the tripping lane wins
        elif w == "stale_carried_into_restart":
            for W in WINDOWS:
                assert any(out == "restart" and s > 0 for _e0, s, _a, _r, out in rec(W)), (name, W)
        elif w == "stale_carried_into_accept":
            for W in WINDOWS:
                assert any(out == "accept" and s > 0 for _e0, s, _a, _r, out in rec(W)), (name, W)
        elif w.startswith("restart_at_last_lane:"):
            W = int(w.split(":")[1])
            assert any(out == "restart" and r == W - 1 for _e0, _s, _a, r, out in rec(W)), name
        elif w.startswith("restart_at_lane_0:"):
            W = int(w.split(":")[1])
            assert any(out == "restart" and r == 0 and s == W for _e0, s, _a, r, out in rec(W)), name
        else:
            raise AssertionError(w)


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=dtype)).astype(np.dtype(dtype).newbyteorder("<")).tobytes()).hexdigest()


def case_record(res):
    """what goldens_hill.json freezes of a chain"""
    log = HO.log_words(res)
    return {"tour": [int(v) for v in res["tour"]], "cost_bits": HO.bits(res["cost"]), "counters": dict(res["counters"]), "log_len": int(len(log)),
            "log_sha256": sha(log, np.uint32), "log_head": log[:6].tolist(), "stale": [int(v) for v in res["stale"][:32]]}


def golden_draws():
    """draw values the goldens freeze: (seed, chain, event, slot)"""
    q = [(1, 0, e, s) for e in (0, 1, 599) for s in (0, 1, 21)]
    q += [(7, 3, HO.shuffle_event(e, n, j), HO.SLOT_SHUFFLE) for e, n, j in ((0, 5, 1), (0, 5, 4), (3, 7, 6), (600, 52, 51), (0xFFFFFFFE, 13650, 13649))]
    return q
