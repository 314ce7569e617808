"""pipeline::run_pipeline_stages — mirror of src/tsp/pipeline.rs:53-80 for the GPU-accelerated solvers.

Stage k+1 is warm-started with stage k's tour; a seed that fails validate_tour is dropped with a warning (the stage then
uses its default seeding, :60-65); an invalid stage RESULT is a hard error (:70-71).  Each outcome carries the stage name,
its Solution and the wall time in ms (StageOutcome, :11-14).
"""
import time
import warnings

# Solvers::from_str (mod.rs:559-590), restricted to what this build accelerates
SOLVER_NAMES = {"nn": "nearest_neighbor", "nearest_neighbor": "nearest_neighbor", "2opt": "two_opt", "two_opt": "two_opt",
                "3opt": "three_opt", "three_opt": "three_opt", "oropt": "or_opt", "or_opt": "or_opt", "or-opt": "or_opt",
                "lk": "lin_kernighan", "lin_kernighan": "lin_kernighan", "shuffle": "random_shuffle",
                "random_shuffle": "random_shuffle", "greedy_edge": "greedy_edge", "gec": "greedy_edge", "savings": "savings", "sav": "savings",
                "christofides": "christofides", "chr": "christofides", "bhk": "bellman_karp", "bellman_karp": "bellman_karp",
                "simulated_annealing": "simulated_annealing", "tabu_search": "tabu_search",
                "genetic_algorithm": "genetic_algorithm", "ant_colony": "ant_colony", "particle_swarm": "particle_swarm", "cuckoo_search": "cuckoo_search",
                "flower_pollination": "flower_pollination", "gravitational_search": "gravitational_search", "kohonen_som": "kohonen_som",
                "hill_climb": "hill_climb", "fourier_curve": "fourier_curve", "branch_and_bound": "branch_and_bound"}  # (the branch and bound, DESIGN.md §4.27, goes by `branch_and_bound`: the reference's `branch_bound` stays unknown; the stochastic hill climb, DESIGN.md §4.25, goes by `hill_climb`: `stochastic_hill` and `hill` stay unknown; the aliases `sa`, `tabu`, `ga`, `aco`, `pso`, `cs`, `fpa`, `gsa`, `som` and `kohonen` stay refused: below)
PRESETS = {"fast": ["nn", "2opt"], "classic": ["nn", "2opt", "simulated_annealing"], "thorough": ["nn", "3opt", "simulated_annealing"]}  # resolve_preset (main.rs:354-369)
# The reference's short alias `sa` is NOT taken: callers of earlier versions rely on `sa` being refused (it named the reference's unseeded,
# unreproducible chain), and this build's annealing is a seeded chain of its own specification.  Ask for it by its long name.
# `tabu` likewise: tabu search goes by its long name only; so does the genetic algorithm (§4.17), `ga`, the ant colony (§4.19), `aco`, the particle swarm (§4.20), `pso`, the cuckoo search (§4.21), `cs`, the flower pollination (§4.22), `fpa`, and the gravitational search (§4.23), `gsa`.  The Kohonen map (§4.24) is `kohonen_som`; `som` and `kohonen` are refused.
REFUSED_ALIASES = {"sa": "simulated_annealing", "tabu": "tabu_search", "ga": "genetic_algorithm", "aco": "ant_colony", "pso": "particle_swarm", "cs": "cuckoo_search", "fpa": "flower_pollination", "gsa": "gravitational_search", "som": "kohonen_som", "kohonen": "kohonen_som",
                   "fourier": "fourier_curve"}  # (the Fourier-curve solver, DESIGN.md §4.26, goes by `fourier_curve`: the reference's `fourier` takes libm's cos, sin and hypot and its kd-tree's choice among tied samples; `branch_bound` stays unknown)
REFUSED_HINTS = {"sa": "the seeded annealing of this build is", "tabu": "the seeded tabu search of this build is",
                 "ga": "the seeded genetic algorithm of this build is", "aco": "the seeded ant colony of this build is",
                 "pso": "the seeded particle swarm of this build is", "cs": "the seeded cuckoo search of this build is",
                 "fpa": "the seeded flower pollination of this build is",
                 "gsa": "the seeded gravitational search of this build is",
                 "som": "the seeded Kohonen map of this build is", "kohonen": "the seeded Kohonen map of this build is",
                 "fourier": "the Fourier-curve solver of this build is"}
AUTO_EXPAND_WITH_SHUFFLE = {"simulated_annealing", "genetic_algorithm", "ant_colony", "particle_swarm", "cuckoo_search", "flower_pollination", "gravitational_search", "hill_climb"}  # mod.rs:144-157: `solve simulated_annealing` alone is shuffle -> simulated_annealing (ant_colony: mod.rs:2158, cuckoo_search: mod.rs:2154, flower_pollination: mod.rs:2155)
AUTO_EXPAND_WITH_NN = {"two_opt", "three_opt", "or_opt", "lin_kernighan", "tabu_search", "branch_and_bound"}  # mod.rs:127-139 (the branch and bound takes the seed's length as its first upper bound; greedy_edge, savings and christofides are seeds: `solve gec` / `solve sav` / `solve chr` run alone; so does the exact solver `solve bhk`, mod.rs:2137, and so does `solve kohonen_som`: the map is in neither list and ignores a start tour; `solve fourier_curve` likewise)


def _unknown(name):
    hint = f"; {REFUSED_HINTS[name.lower()]} `{REFUSED_ALIASES[name.lower()]}`" if name.lower() in REFUSED_ALIASES else ""
    return f"unknown solver `{name}` (this build accelerates {sorted(set(SOLVER_NAMES))}){hint}"


def steps_for_solve(solver, no_seed=False):
    """`teeline solve <solver>` -> pipeline steps (main.rs:371-398)."""
    s = solver.lower()
    if s in PRESETS:
        return list(PRESETS[s])
    if s not in SOLVER_NAMES:
        raise ValueError(_unknown(solver))
    if not no_seed and SOLVER_NAMES[s] in AUTO_EXPAND_WITH_NN:
        return ["nn", s]
    if not no_seed and SOLVER_NAMES[s] in AUTO_EXPAND_WITH_SHUFFLE:
        return ["shuffle", s]
    return [s]


def random_shuffle(problem, seed=1, *, ctx=None):
    """random_shuffle::solve (random_shuffle.rs:12-27), seeded: the Fisher-Yates stream of restart 0 of `seed` (synth.restart_perm,
    the device's multi-start generator); the reference draws from an unseeded thread RNG."""
    from . import Solution, synth
    import ctypes as C
    import numpy as np
    from . import default_context
    ctx = ctx or default_context()
    n = len(problem)
    perm = synth.restart_perm(n, seed, 0)
    cost = C.c_float(0.0)
    if n >= 2:
        packed = problem.explicit_packed()
        ctx.check(ctx.lib.tl_tour_length(ctx.handle, None if packed is not None else problem.xy.ctypes.data_as(C.c_void_p),
                                         None if packed is None else packed.ctypes.data_as(C.c_void_p), n,
                                         perm.ctypes.data_as(C.c_void_p), C.byref(cost)))
    return Solution(cost.value, problem.ids[perm], problem, {})


def format_solution(sol, is_optimized=False):
    """print_solution (main.rs:645-652): every id is followed by one space."""
    return f"{float(sol.total):.5f} {1 if is_optimized else 0}\n" + "".join(f"{v} " for v in sol.route()) + "\n"


def _json_f32(v):
    import numpy as np
    return repr(float(np.float32(v)))  # f32 widened to f64, shortest round-trip decimal, "60.0" for integers (serde_json)


def format_solution_json(sol, is_optimized=False, comparison=None):
    """print_solution_json (main.rs:700-712): keys sorted (serde_json's BTreeMap), compact."""
    s = '{"cost":' + _json_f32(sol.total)
    if comparison is not None:
        s += ',"gap_pct":' + _json_f32(comparison[1]) + ',"optimal_cost":' + _json_f32(comparison[0])
    s += ',"optimized":' + ("true" if is_optimized else "false") + ',"route":[' + ",".join(str(v) for v in sol.route()) + "]}\n"
    return s


class StageOutcome:
    def __init__(self, name, solution, duration_ms):
        self.name, self.solution, self.duration_ms = name, solution, duration_ms


def run_pipeline_stages(problem, steps, opts=None, *, ctx=None, lk_seed=1, exact_walk=False, init_tour=None, sa_chains=1, tabu_chains=1, ga_runs=1, aco_runs=1, pso_runs=1, cs_runs=1, fpa_runs=1, gsa_runs=1, som_runs=1, hill_chains=1, fourier_jobs=None, bnb_max_nodes=0, bnb_time_limit_ms=0):
    """steps: iterable of solver names ("nn", "gec", "sav", "chr", "bhk", "2opt", "3opt", "or_opt", "lk", "simulated_annealing", "tabu_search", "genetic_algorithm", "ant_colony", "particle_swarm", "cuckoo_search", "flower_pollination", "gravitational_search", "kohonen_som", "hill_climb", "fourier_curve", "branch_and_bound", "shuffle"); opts: {name: options} (optional).
    A `simulated_annealing` stage draws from the stream of lk_seed (the pipeline's one seed) and runs sa_chains chains, keeping the best;
    a `tabu_search` stage likewise, with tabu_chains chains, a `genetic_algorithm` stage with ga_runs runs an `ant_colony` stage with aco_runs runs a `particle_swarm` stage with pso_runs runs a `cuckoo_search` stage with cs_runs runs a `flower_pollination` stage with fpa_runs runs and a `gravitational_search` stage with gsa_runs runs.  A `kohonen_som` stage runs som_runs runs and ignores its seed tour.  A `hill_climb` stage runs hill_chains chains.  A `fourier_curve` stage ignores its seed tour too; fourier_jobs, a list of FourierOptions, makes it a batch of which the best is kept.
    A `branch_and_bound` stage takes the previous stage's tour as its start tour and is exact unless opts names a HeuristicOptions for it (then its n_nearest restricts the candidates); bnb_max_nodes / bnb_time_limit_ms are its budgets (0: none).
    exact_walk: a `bhk` stage reads its route back by exact equality (bellman_karp.solve) instead of the reference's tolerance walk,
    whose result can fail validate_tour below.  init_tour: the seed of the first stage (city ids; default: that stage's own seeding)."""
    from . import (HeuristicOptions, LKOptions, ant_colony, bellman_karp, branch_and_bound, christofides, cuckoo_search, flower_pollination, genetic_algorithm, gravitational_search, fourier_curve, greedy_edge, hill_climb, kohonen_som, lin_kernighan, nearest_neighbor, or_opt, particle_swarm, savings, simulated_annealing,
                   tabu_search, three_opt, two_opt, validate_tour)
    mods = {"nearest_neighbor": nearest_neighbor, "two_opt": two_opt, "three_opt": three_opt, "or_opt": or_opt,
            "lin_kernighan": lin_kernighan, "greedy_edge": greedy_edge, "savings": savings, "christofides": christofides,
            "bellman_karp": bellman_karp}
    opts = opts or {}
    outcomes, seed = [], (None if init_tour is None else list(init_tour))
    for step in steps:
        if step not in SOLVER_NAMES:
            raise ValueError(_unknown(step))
        name = SOLVER_NAMES[step]
        init = seed
        if init is not None and not validate_tour(init, problem):
            warnings.warn(f"pipeline: seed for stage `{step}` is not a valid tour; falling back to default seeding")
            init = None
        t0 = time.perf_counter()
        if name == "random_shuffle":
            sol = random_shuffle(problem, lk_seed, ctx=ctx)
        elif name == "lin_kernighan":
            sol = lin_kernighan.solve(problem, opts.get(step) or LKOptions(), None, init, ctx=ctx, seed=lk_seed)
        elif name == "simulated_annealing":
            sol = simulated_annealing.solve(problem, opts.get(step) or simulated_annealing.SAOptions(), None, init, ctx=ctx, seed=lk_seed, chains=sa_chains)
        elif name == "tabu_search":
            sol = tabu_search.solve(problem, opts.get(step) or HeuristicOptions(), None, init, ctx=ctx, seed=lk_seed, chains=tabu_chains)
        elif name == "genetic_algorithm":
            sol = genetic_algorithm.solve(problem, opts.get(step) or genetic_algorithm.GAOptions(), None, init, ctx=ctx, seed=lk_seed, runs=ga_runs)
        elif name == "ant_colony":
            sol = ant_colony.solve(problem, opts.get(step) or ant_colony.AcoOptions(), None, init, ctx=ctx, seed=lk_seed, runs=aco_runs)
        elif name == "particle_swarm":
            sol = particle_swarm.solve(problem, opts.get(step) or HeuristicOptions(), None, init, ctx=ctx, seed=lk_seed, runs=pso_runs)
        elif name == "cuckoo_search":
            sol = cuckoo_search.solve(problem, opts.get(step) or cuckoo_search.CSOptions(), None, init, ctx=ctx, seed=lk_seed, runs=cs_runs)
        elif name == "flower_pollination":
            sol = flower_pollination.solve(problem, opts.get(step) or flower_pollination.FPAOptions(), None, init, ctx=ctx, seed=lk_seed, runs=fpa_runs)
        elif name == "gravitational_search":
            sol = gravitational_search.solve(problem, opts.get(step) or HeuristicOptions(), None, init, ctx=ctx, seed=lk_seed, runs=gsa_runs)
        elif name == "kohonen_som":
            sol = kohonen_som.solve(problem, opts.get(step) or kohonen_som.SOMOptions(), None, init, ctx=ctx, seed=lk_seed, runs=som_runs)
        elif name == "hill_climb":
            sol = hill_climb.solve(problem, opts.get(step) or HeuristicOptions(), None, init, ctx=ctx, seed=lk_seed, chains=hill_chains)
        elif name == "fourier_curve":
            if fourier_jobs:
                sol = fourier_curve.solve_many(problem, list(fourier_jobs), ctx=ctx)
            else:
                sol = fourier_curve.solve(problem, opts.get(step) or fourier_curve.FourierOptions(), None, init, ctx=ctx)
        elif name == "branch_and_bound":
            sol = branch_and_bound.solve(problem, opts.get(step), None, init, ctx=ctx, max_nodes=bnb_max_nodes, time_limit_ms=bnb_time_limit_ms)
        elif name == "bellman_karp":
            sol = mods[name].solve(problem, opts.get(step) or HeuristicOptions(), None, init, ctx=ctx, exact_walk=exact_walk)
        else:
            sol = mods[name].solve(problem, opts.get(step) or HeuristicOptions(), None, init, ctx=ctx)
        ms = (time.perf_counter() - t0) * 1e3
        if not validate_tour(sol.route(), problem):
            raise RuntimeError(f"pipeline: stage `{step}` produced an invalid tour")
        outcomes.append(StageOutcome(step, sol, ms))
        seed = sol.route()
    return outcomes


POPULATION_SOLVERS = ("two_opt", "three_opt", "or_opt")  # the solvers with a population entry (tl_two_opt_population, tl_three_opt_population, tl_or_opt_population)


def run_population(problem, steps, init_tours, *, ctx=None):
    """run_pipeline_stages for a population of tours: every stage runs through its population entry (one descent per tour, all
    concurrently) and feeds the next.  steps: drawn from "2opt" / "3opt" / "or_opt" and their long names; any other step is a ValueError
    that names it, raised before anything runs.  Returns one list of StageOutcome per tour — entry k equals
    run_pipeline_stages(problem, steps) started from init_tours[k]; a stage's duration_ms is the whole population's."""
    from . import or_opt, three_opt, two_opt, validate_tour
    steps = list(steps)
    for step in steps:
        if SOLVER_NAMES.get(step) not in POPULATION_SOLVERS:
            raise ValueError(f"step `{step}` has no population form (population pipelines take {sorted(k for k, v in SOLVER_NAMES.items() if v in POPULATION_SOLVERS)})")
    mods = {"two_opt": two_opt, "three_opt": three_opt, "or_opt": or_opt}
    tours = [list(t) for t in init_tours]
    outcomes = [[] for _ in tours]
    for step in steps:
        t0 = time.perf_counter()
        sols = mods[SOLVER_NAMES[step]].solve_population(problem, tours, ctx=ctx)
        ms = (time.perf_counter() - t0) * 1e3
        for k, sol in enumerate(sols):
            if not validate_tour(sol.route(), problem):
                raise RuntimeError(f"pipeline: stage `{step}` produced an invalid tour for individual {k}")
            outcomes[k].append(StageOutcome(step, sol, ms))
        tours = [sol.route() for sol in sols]
    return outcomes
