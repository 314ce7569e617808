"""The shared comparator of the swarm solvers' GPU tests (tests/_swarm_harness.py: compare_run) still bites: on the record a device
that is right would return it passes, and with any one field of that record changed — a word of the tour, the cost's low bit, a
word of a log record, the log's length, a route word, a word of an epoch row, each of the three stats — it fails.  No GPU: the
record is built from the oracle's result."""
import copy

import numpy as np
import pytest

import _cs_cases
import _fpa_cases
import _gsa_cases
import _pso_cases
import _swarm_harness as H

CASES = {"particle_swarm": (_pso_cases, "small8_every_condition"), "cuckoo_search": (_cs_cases, "small8_every_condition"),
         "flower_pollination": (_fpa_cases, "small8_every_condition"), "gravitational_search": (_gsa_cases, "small8")}


def implied_record(desc, res, n, o):
    """what gpu_trace returns after its rc where the device equals the oracle"""
    O, c = desc.oracle, res["counters"]
    stats = dict(sweeps=o["epochs"], candidates=c[desc.counter], moves=c["improved"])
    return [res["tour"].copy(), np.float32(res["cost"]), O.log_words(res), len(res["improvements"]), stats, O.route_words(res, n), O.epoch_words(res)]


def flips(record, epochs):
    """(what was changed, the record with it changed)"""
    def changed(field, at=None, stat=None):
        rec = copy.deepcopy(record)
        if stat is not None:
            rec[field][stat] += 1
        elif at is None:
            rec[field] = rec[field] + 1 if field == 3 else (rec[field].view(np.uint32) ^ np.uint32(1)).view(np.float32)
        else:
            rec[field][at] ^= 1
        return rec
    last = len(record[2]) - 1
    yield "tour word", changed(0, 0)
    yield "last tour word", changed(0, len(record[0]) - 1)
    yield "cost's low bit", changed(1)
    for col, name in enumerate(("epoch", "member", "cost bits", "route index")):
        yield f"log record's {name}", changed(2, (last, col))
    yield "first log record", changed(2, (0, 2))
    yield "log length", changed(3)
    yield "route word", changed(5, (last, 0))
    yield "first route's last word", changed(5, (0, record[5].shape[1] - 1))
    for e in (0, epochs - 1):
        for w in (0, record[6].shape[1] - 1):
            yield f"epoch {e}'s word {w}", changed(6, (e, w))
    for stat in ("sweeps", "candidates", "moves"):
        yield stat, changed(4, stat=stat)


@pytest.mark.parametrize("desc", H.SWARMS, ids=lambda d: d.stem)
def test_compare_run_passes_on_the_oracle_and_fails_on_every_flip(desc):
    cases, name = CASES[desc.stem]
    xy, packed, n, init, o, _want = cases.seeded_case(name)
    res = desc.oracle.solve_cached(H.okey(name, n, init, o), xy, packed, n, init, **o)
    assert len(res["improvements"]) >= 2 and o["epochs"] >= 2 and len(res["epochs"]) == o["epochs"]
    record = implied_record(desc, res, n, o)
    assert record[6].shape == (o["epochs"], desc.row(desc.size(o["n_nearest"])))
    H.compare_run(desc, res, record, o, name)
    seen = 0
    for what, rec in flips(record, o["epochs"]):
        with pytest.raises(AssertionError):
            H.compare_run(desc, res, rec, o, name)
            pytest.fail(f"compare_run passed with the {what} changed", pytrace=False)
        seen += 1
    assert seen == 18
    H.compare_run(desc, res, record, o, name)  # the flips were made on copies
