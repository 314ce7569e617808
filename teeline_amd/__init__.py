"""teeline_amd — MI355X-native 2-opt / 3-opt / Lin–Kernighan local-search engine (with NN, greedy-edge, savings and Christofides seeds
and the Bellman–Held–Karp exact solver for n <= 26; simulated annealing closes the classic / thorough presets; tabu search runs as seeded chains, the genetic algorithm as seeded runs).

Host-side mirror of the solver entry points of the `teeline` Rust crate (timgluz/teeline):
    two_opt.solve / three_opt.solve / lin_kernighan.solve (problem, opts, progress_tx, init_tour)
    reference: src/tsp/two_opt.rs:7-12, src/tsp/three_opt.rs:16-21, src/tsp/lin_kernighan.rs:35-40
implemented as thin wrappers over the C ABI of libteeline_gpu.so (include/teeline_gpu.h), whose hot
paths are hand-written HIP kernels for gfx950.  There is no CPU fallback: without the built library
and a gfx950 device every solver call raises.
"""
from . import _capi
from ._capi import (TL_BHK_MAX_N, TL_FLAG_3OPT_POP_FORCE_SCAN, TL_FLAG_3OPT_POP_FORCE_WG, TL_FLAG_BHK_EXACT_WALK, TL_FLAG_2OPT_FORCE_HBM, TL_FLAG_2OPT_FX, TL_FLAG_2OPT_NL_ALWAYS, TL_FLAG_2OPT_NO_NL, TL_FLAG_2OPT_NT256, TL_FLAG_2OPT_NT512, TL_FLAG_COUNT_WORK, TL_FLAG_KNN_BRUTE, TL_FLAG_KNN_1LANE, TL_FLAG_KNN_4LANES, TL_FLAG_LK_NO_SPLIT,
                    TL_FLAG_LK_CHIP_WIDE, TL_FLAG_LK_CLASSIC_VIEW, TL_FLAG_LK_ILS_LDS, TL_FLAG_LK_NO_GRAPH, TL_FLAG_LK_NO_SPECULATION, TL_FLAG_LK_NO_SUBCHAINS, TL_FLAG_LK_ONE_WORKGROUP, TL_FLAG_LK_SCAN_PERSIST, TL_FLAG_LK_SEPARATE_PICK, TL_FLAG_LK_SEPARATE_STEP, TL_FLAG_LK_SMALL, TL_FLAG_LK_SPLIT2, TL_FLAG_MULTISTART_RCCL, TL_FLAG_NONE, TL_FLAG_NO_PRUNE, TL_FLAG_OR_OPT_FORCE_SCAN, TL_FLAG_SA_NO_SPECULATION, TL_FLAG_TABU_FULL_COMPARE,
                    TL_MODE_BEST_SWEEP, TL_MODE_REF_ORDER, ReferencePanics, TeelineGpuError)
from .host import (Context, HeuristicOptions, KDPoint, LKOptions, SAOptions, Solution, TspProblem, default_context,
                   alpha_candidates, ant_colony, bellman_karp, branch_and_bound, christofides, cuckoo_search, distance_matrix, flower_pollination, fourier_curve, genetic_algorithm, gravitational_search, greedy_edge, hill_climb, kohonen_som, lin_kernighan, multistart, nearest_neighbor, one_tree_bound, opt_tour, or_opt, particle_swarm, pipeline, savings, simulated_annealing, synth, tabu_search, three_opt, tsplib,
                   two_opt,
                   validate_tour)

__all__ = [
    "Context", "HeuristicOptions", "KDPoint", "LKOptions", "SAOptions", "Solution", "TspProblem", "default_context",
    "distance_matrix", "greedy_edge", "savings", "christofides", "bellman_karp", "branch_and_bound", "lin_kernighan", "simulated_annealing", "tabu_search", "genetic_algorithm", "ant_colony", "particle_swarm", "cuckoo_search", "flower_pollination", "gravitational_search", "kohonen_som", "hill_climb", "fourier_curve", "one_tree_bound", "alpha_candidates", "three_opt", "tsplib", "two_opt", "validate_tour",
    "TL_MODE_REF_ORDER", "TL_MODE_BEST_SWEEP", "TL_FLAG_NONE", "TL_FLAG_NO_PRUNE", "TL_FLAG_BHK_EXACT_WALK", "TL_BHK_MAX_N",
    "TeelineGpuError", "ReferencePanics",
]
