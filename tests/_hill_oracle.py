"""The specification of the project's stochastic hill climb, in numpy, one epoch at a time (TEST infrastructure, not product code).

stochastic_hill.rs:7-97 and route.rs:48-113 with one deliberate difference, because the reference's unseeded thread RNG cannot be
reproduced: the random draws are a pure function of (seed, chain, event, slot).  Everything else is the reference's, quirks included:
a candidate of the CURRENT tour is accepted iff its cost is below the BEST cost; the plateau check comes after the epoch counter's
increment and before the end check; a restart shuffles the current tour in place and leaves the best alone; `epochs + 1` epochs run;
the best route is returned; every cost is tour_length (closing edge first, sequential f32) of the whole candidate tour.
"""
import numpy as np

from _sa_oracle import G, M64, chain_key, dist_fn, mix, pair_from_key, tour_length
from _swarm_oracle import bits, cached  # noqa: F401  (bits: re-exported)

NONE = 0xFFFFFFFF
INIT_EVENT = 1 << 58
SLOT_SHUFFLE = 26
DEFAULTS = dict(epochs=10_000, platoo_epochs=500)  # mod.rs:598-608


def draw(seed, chain, event, slot):
    return mix(chain_key(seed, chain) + G * (32 * event + slot + 1))


def shuffle_event(epoch, n, j):
    return INIT_EVENT + epoch * n + j


def shuffle(key, epoch, n, tour):
    """the restart after epoch `epoch` (the index before the increment): Fisher-Yates on the current contents, in place"""
    for j in range(n - 1, 0, -1):
        u = mix(key + G * (32 * shuffle_event(epoch, n, j) + SLOT_SHUFFLE + 1))
        p = ((u >> 32) * (j + 1)) >> 32
        tour[j], tour[p] = tour[p], tour[j]


def roles(n, epochs):
    """every (event, slot) a chain on n cities reads in epochs 0 .. epochs - 1, with its role: what test_draw_roles_are_disjoint counts"""
    out = []
    for e in range(epochs):
        out += [((e, s), ("pair", e, s)) for s in range(22)]
        out += [((shuffle_event(e, n, j), SLOT_SHUFFLE), ("shuffle", e, j)) for j in range(1, n)]
    return out


def solve(xy, packed, n, init=None, *, seed=1, chain=0, epochs=10_000, platoo_epochs=500):
    """One chain.  Returns a dict: tour (the best), cost, log = [(epoch, from, to, cost bits) | (epoch, NONE, 0, 0)], stale = n_stale
    when each event fell (before it is cleared), shuffled = the current tour after each restart, and the counters."""
    if n < 2:
        raise ValueError("reference panics: n_items must be bigger than 2")
    if epochs == 0:
        raise ValueError("epochs = 0 never ends")
    cur = np.arange(n, dtype=np.int64) if init is None else np.asarray(init, dtype=np.int64).copy()
    d = dist_fn(xy, packed, n)
    key = chain_key(seed, chain)
    best, best_cost = cur.copy(), tour_length(d, cur)
    log, stale, shuffled, accept_epochs = [], [], [], []
    n_stale = accepts_after_restart = restart_on_last = reversed_ = 0
    cur_is_best = True
    epoch = 0
    while True:
        lo, hi = pair_from_key(key, epoch, n)
        cand = cur.copy()
        cand[lo:hi + 1] = cur[lo:hi + 1][::-1]
        c = tour_length(d, cand)
        if c < best_cost:
            stale.append(n_stale)
            accepts_after_restart += 0 if cur_is_best else 1
            cur, best, best_cost = cand, cand.copy(), c
            cur_is_best = True
            n_stale = 0
            reversed_ += hi - lo + 1
            accept_epochs.append(epoch)
            log.append((epoch, lo, hi, bits(c)))
        else:
            n_stale += 1
        epoch += 1
        if n_stale > platoo_epochs and platoo_epochs > 0:
            stale.append(n_stale)
            shuffle(key, epoch - 1, n, cur)
            shuffled.append(cur.copy())
            cur_is_best = False
            n_stale = 0
            log.append((epoch - 1, NONE, 0, 0))
            restart_on_last += 1 if epoch > epochs else 0
        if epoch > epochs:
            break
    a = np.asarray(accept_epochs, dtype=np.int64)
    in256 = max((int(np.searchsorted(a, e + 256) - k) for k, e in enumerate(a)), default=0)
    restarts = sum(1 for r in log if r[1] == NONE)
    return {"tour": best.astype(np.uint32), "cost": np.float32(best_cost), "log": log, "stale": stale, "shuffled": shuffled, "epochs_run": epoch,
            "counters": {"accepts": len(a), "restarts": restarts, "accepts_after_restart": accepts_after_restart, "restart_on_last_epoch": restart_on_last,
                         "max_accepts_in_256": in256, "reversed": int(reversed_)}}


def log_words(res):
    return np.asarray(res["log"], dtype=np.uint32).reshape(-1, 4)


def windows(xy, packed, n, init=None, *, W, seed=1, chain=0, epochs=10_000, platoo_epochs=500):
    """The same chain resolved a window of W epochs at a time, as the device does it: every lane of a window is priced against the
    window's start state.  Returns (result as solve()'s tour / cost / log, record) with one record row per window:
    (e0, n_stale at its start, a = the lowest accepting lane or None, r = the lane whose rejection trips the plateau or None (not a
    live lane), outcome 'accept' | 'restart' | 'none')."""
    cur = np.arange(n, dtype=np.int64) if init is None else np.asarray(init, dtype=np.int64).copy()
    d = dist_fn(xy, packed, n)
    key = chain_key(seed, chain)
    best, best_cost = cur.copy(), tour_length(d, cur)
    total = epochs + 1
    e0 = n_stale = 0
    log, rec = [], []
    while e0 < total:
        live = min(W, total - e0)
        a = None
        for lane in range(live):
            lo, hi = pair_from_key(key, e0 + lane, n)
            cand = cur.copy()
            cand[lo:hi + 1] = cur[lo:hi + 1][::-1]
            c = tour_length(d, cand)
            if c < best_cost:
                a = lane
                break
        r = platoo_epochs - n_stale if platoo_epochs > 0 and platoo_epochs - n_stale < live else None
        if a is not None and (r is None or a <= r):
            rec.append((e0, n_stale, a, r, "accept"))
            cur, best, best_cost = cand, cand.copy(), c
            log.append((e0 + a, lo, hi, bits(c)))
            n_stale = 0
            e0 += a + 1
        elif r is not None:
            if a is None:  # (the record wants to know whether a later lane would have accepted)
                for lane in range(r + 1, live):
                    lo, hi = pair_from_key(key, e0 + lane, n)
                    cand = cur.copy()
                    cand[lo:hi + 1] = cur[lo:hi + 1][::-1]
                    if tour_length(d, cand) < best_cost:
                        a = lane
                        break
            rec.append((e0, n_stale, a, r, "restart"))
            shuffle(key, e0 + r, n, cur)
            log.append((e0 + r, NONE, 0, 0))
            n_stale = 0
            e0 += r + 1
        else:
            rec.append((e0, n_stale, None, None, "none"))
            n_stale += live
            e0 += live
    return {"tour": best.astype(np.uint32), "cost": np.float32(best_cost), "log": log}, rec


def replay(ids, start, res):
    """The reference's message stream (stochastic_hill.rs:29-31,51-56,75-77,93-95) of a chain, from the oracle's own record"""
    out = [("PathUpdate", ([int(v) for v in ids[start]], 0.0))]
    tour = np.asarray(start, dtype=np.int64).copy()
    k = 0
    for epoch, frm, to, cb in res["log"]:
        if frm == NONE:
            tour = res["shuffled"][k].copy()
            k += 1
            out.append(("PathUpdate", ([int(v) for v in ids[tour]], 0.0)))
        else:
            tour[frm:to + 1] = tour[frm:to + 1][::-1].copy()
            out.append(("PathUpdate", ([int(v) for v in ids[tour]], float(np.array([cb], dtype=np.uint32).view(np.float32)[0]))))
    out.append(("Done", None))
    return out


solve_cached = cached(solve)
