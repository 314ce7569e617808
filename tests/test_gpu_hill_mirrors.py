"""The hill climb's mirrors on the GPU: the Python mirror's message stream against the oracle's replay (one chain, and the best of 8),
the pipeline stage, and the C++ CLI against the Python mirror."""
import os
import subprocess

import numpy as np
import pytest

import _hill_cases as HC
import _hill_oracle as HO
import _sa_cases as K

pytestmark = pytest.mark.gpu

bits = HO.bits
TSP = os.path.join(K.TSPLIB, "berlin52.tsp")


def oracle(prob, init_pos, epochs, platoo, seed, chain=0):
    key = ("mirror", None if init_pos is None else tuple(int(v) for v in init_pos), epochs, platoo, seed, chain)
    return HO.solve_cached(key, prob.xy, None, len(prob), init_pos, epochs=epochs, platoo_epochs=platoo, seed=seed, chain=chain)


def same_messages(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, p), (_k, q) in zip(got, want):
        if k == "PathUpdate":
            assert p[0] == q[0] and bits(p[1]) == bits(q[1])


def test_python_mirror_messages_one_chain_and_best_of_eight(ctx):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(TSP).problem()
    start = HC.start(52, 1)
    opts = TA.HeuristicOptions(epochs=600, platoo_epochs=7)
    res = oracle(prob, start, 600, 7, 1)
    assert res["counters"]["restarts"] >= 1 and res["counters"]["accepts"] >= 2
    msgs = []
    sol = TA.hill_climb.solve(prob, opts, lambda k, p: msgs.append((k, p)), prob.ids[start].tolist(), ctx=ctx, seed=1)
    same_messages(msgs, HO.replay(prob.ids, start, res))
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    for window in (0, 1):
        plain = TA.hill_climb.solve(prob, opts, None, prob.ids[start].tolist(), ctx=ctx, seed=1, window=window)
        assert plain.route() == sol.route() and plain.stats["moves"] == res["counters"]["accepts"] and plain.stats["sweeps"] == 601
    # from city order (init_tour None), and the best of 8 chains with its own replay
    singles = [oracle(prob, None, 600, 7, 1, c) for c in range(8)]
    c = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    msgs2 = []
    best = TA.hill_climb.solve(prob, opts, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, chains=8)
    assert best.stats["chain"] == c and best.route() == prob.ids[singles[c]["tour"]].tolist() and bits(best.total) == bits(singles[c]["cost"])
    assert best.stats["moves"] == singles[c]["counters"]["accepts"]
    same_messages(msgs2, HO.replay(prob.ids, np.arange(52), singles[c]))


def test_pipeline_stage(ctx):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(TSP).problem()
    short = TA.HeuristicOptions(epochs=300, platoo_epochs=50)
    steps = TA.pipeline.steps_for_solve("hill_climb")
    assert steps == ["shuffle", "hill_climb"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"hill_climb": short}, ctx=ctx, lk_seed=3)
    assert [o.name for o in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = oracle(prob, prob.positions_of(outs[0].solution.route()), 300, 50, 3)
    assert outs[-1].solution.route() == prob.ids[seeded["tour"]].tolist() and bits(outs[-1].solution.total) == bits(seeded["cost"])
    outs2 = TA.pipeline.run_pipeline_stages(prob, steps, {"hill_climb": short}, ctx=ctx, lk_seed=3, hill_chains=3)
    assert outs2[-1].solution.total <= outs[-1].solution.total


def test_cli_equals_python_mirror(ctx):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    prob = TA.tsplib.read_from_file(TSP).problem()
    opts = TA.HeuristicOptions(epochs=300, platoo_epochs=50)
    args0 = ["--epochs", "300", "--platoo_epochs", "50", "--seed", "1"]
    for args, steps in ((["solve", "hill_climb"], ["shuffle", "hill_climb"]), (["pipeline", "--steps=nn,hill_climb"], ["nn", "hill_climb"]),
                        (["solve", "hill_climb", "--no-seed"], ["hill_climb"])):
        r = subprocess.run([cli] + args + ["-i", TSP] + args0, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs = TA.pipeline.run_pipeline_stages(prob, steps, {"hill_climb": opts, "nn": opts}, ctx=ctx, lk_seed=1)
        assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(outs[-1].solution).splitlines(), args
    r = subprocess.run([cli, "solve", "hill_climb", "-i", TSP, "--runs", "4"] + args0, capture_output=True, text=True, timeout=120)
    sh = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=1)[0].solution
    best = TA.hill_climb.solve(prob, opts, None, sh.route(), ctx=ctx, seed=1, chains=4)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(best).splitlines()


def test_cli_progress_digest_equals_python_messages(ctx):
    """the C++ mirror's replay (restarts shuffled through tl_hill_draw) ends on the same best route as the Python mirror's"""
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    r = subprocess.run([cli, "solve", "hill_climb", "--no-seed", "-i", TSP, "--epochs", "600", "--platoo_epochs", "7", "--seed", "1", "--progress-digest"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    prob = TA.tsplib.read_from_file(TSP).problem()
    msgs = []
    sol = TA.hill_climb.solve(prob, TA.HeuristicOptions(epochs=600, platoo_epochs=7), lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(sol).splitlines()
    h = 1469598103934665603  # the CLI's FNV-1a over (kind, ids as u64, f32 bits) per message; Done: the kind only

    def word(h, v, nbytes):
        for k in range(nbytes):
            h = ((h ^ ((v >> (8 * k)) & 0xFF)) * 1099511628211) & ((1 << 64) - 1)
        return h

    for kind, p in msgs:
        if kind == "Done":
            h = word(h, 2, 1)
            continue
        h = word(word(h, 0, 1), len(p[0]), 4)
        for v in p[0]:
            h = word(h, int(v), 8)
        h = word(h, bits(p[1]), 4)
    assert sum(1 for k, p in msgs if k == "PathUpdate" and p[1] == 0.0) >= 3  # the start route and restarts
    assert f"path_updates={len(msgs) - 1} " in r.stderr and f"digest={h:016x}" in r.stderr, r.stderr


def test_cpp_refusals_keep_their_wording():
    from teeline_amd import build
    cli = build.build_cli()
    r = subprocess.run([cli, "solve", "stochastic_hill", "-i", TSP], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the seeded hill climb of this build is `hill_climb`" in r.stderr
    r = subprocess.run([cli, "solve", "hill", "-i", TSP], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "unknown solver" in r.stderr
