"""What the oracles of the population solvers (tests/_pso_oracle.py, _cs_oracle.py, _fpa_oracle.py, _gsa_oracle.py) state in the same
words, written once (TEST infrastructure, not product code): the f64 uniform of a draw, a float's bits, the start shuffle, the swap
sequence of route.rs in its three tested-equal forms, the words of the `Swarm4` trace's improvement log and routes, the reference's
messages, and the per-module cache every oracle's solve_cached is made of.  Each oracle re-exports what it uses under the names it
always had; each solver's solve() stays in its own file.
"""
import numpy as np

NONE = 0xFFFFFFFF


def uniform(u):
    return (int(u) >> 11) * 2.0 ** -53


def bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def shuffled(key, n, member):
    """the start tour of population member `member`: Fisher-Yates from the top, on the member's init events"""
    from _ga_oracle import SLOT_SHUFFLE, draw_key, init_event, position  # (here: _ga_oracle takes cached() from this module)
    r = list(range(n))
    for j in range(n - 1, 0, -1):
        k = position(draw_key(key, init_event(n, member, j), SLOT_SHUFFLE), j + 1)
        r[j], r[k] = r[k], r[j]
    return r


def swap_sequence_literal(src, dst):
    """swap_sequence (route.rs:118-134) as written: a linear search from i + 1 on (list.index is one); saturating_sub for n = 0"""
    tmp = [int(v) for v in src]
    dst = [int(v) for v in dst]
    seq = []
    for i in range(max(len(tmp) - 1, 0)):
        if tmp[i] != dst[i]:
            j = tmp.index(dst[i], i + 1)
            seq.append((i, j))
            tmp[i], tmp[j] = tmp[j], tmp[i]
    return seq


def swap_sequence_inverse(src, dst):
    """the same walk with a table of where every city is instead of the search: O(n)"""
    tmp = [int(v) for v in src]
    where = [0] * len(tmp)
    for k, c in enumerate(tmp):
        where[c] = k
    seq = []
    for i in range(max(len(tmp) - 1, 0)):
        want = int(dst[i])
        if tmp[i] != want:
            j = where[want]
            seq.append((i, j))
            where[tmp[i]], where[want] = j, i
            tmp[i], tmp[j] = tmp[j], tmp[i]
    return seq


def orbits(src, dst):
    """pi(p) = src^-1[dst[p]] and the lengths of its cycles"""
    n = len(src)
    inv = [0] * n
    for k, c in enumerate(src):
        inv[int(c)] = k
    pi = [inv[int(dst[p])] for p in range(n)]
    seen, lens = [False] * n, []
    for s in range(n):
        if not seen[s]:
            k, p = 0, s
            while not seen[p]:
                seen[p] = True
                p = pi[p]
                k += 1
            lens.append(k)
    return pi, lens


def swap_sequence_orbit(src, dst):
    """the form the device computes (csrc/particle_swarm.hip): in ascending i, (i, q) for every i that is not the largest position
    of its pi-cycle, q the first of pi(i), pi^2(i), .. above i"""
    pi, _ = orbits(src, dst)
    seq = []
    for i in range(len(pi)):
        p = pi[i]
        while p < i:
            p = pi[p]
        if p > i:
            seq.append((i, p))
    return seq


def apply_swaps(pos, swaps):
    """apply_swaps (route.rs:137-143)"""
    out = list(pos)
    for i, j in swaps:
        out[i], out[j] = out[j], out[i]
    return out


def log_words(res, route_cap=None):
    """the improvement log of a tl_<solver>_trace: [epoch, member (cuckoo search: source), cost bits, route index]"""
    rows = [[e, i, bits(c), k if route_cap is None or k < route_cap else NONE] for k, (e, i, c, _r) in enumerate(res["improvements"])]
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 4)


def route_words(res, n):
    return np.asarray([r for _e, _i, _c, r in res["improvements"]], dtype=np.uint32).reshape(-1, n)


def messages(res, ids=None):
    """what the reference sends (cuckoo_search.rs:73-75,98-100,120-122,127-129,132-134; flower_pollination.rs:113-115,133-136,142-144,
    147-149; gravitational_search.rs:72-74,130-132,136-138,141-143): the start's PathUpdate, then per epoch its improvements' and
    an EpochUpdate, then Done"""
    name = (lambda r: [int(v) for v in r]) if ids is None else (lambda r: [int(v) for v in np.asarray(ids)[np.asarray(r, dtype=np.int64)]])
    imp = res["improvements"]
    out = [("PathUpdate", (name(imp[0][3]), float(imp[0][2])))]
    k = 1
    for e in range(len(res["epochs"])):
        while k < len(imp) and imp[k][0] == e:
            out.append(("PathUpdate", (name(imp[k][3]), float(imp[k][2]))))
            k += 1
        out.append(("EpochUpdate", e))
    out.append(("Done", None))
    return out


def read_only(a):
    a.setflags(write=False)
    return a


def _tour_read_only(res):
    read_only(res["tour"])
    return res


def cached(solve, share=_tour_read_only):
    """an oracle module's solve_cached: solve() once per process and key; the results are shared between tests and must not be
    written to.  One dict per call, so per module: the tests' keys ("epochs", "pop", ..) repeat across the solvers.
    share: what of a result is kept, read-only where it is an array (a dict's "tour" where nothing is given)"""
    cache = {}

    def solve_cached(key, *args, **kw):
        if key not in cache:
            cache[key] = share(solve(*args, **kw))
        return cache[key]
    solve_cached.cache = cache
    return solve_cached
