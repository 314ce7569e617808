"""ctypes loader for libteeline_gpu.so — the C ABI declared in include/teeline_gpu.h.

The library is the product; this module only binds it.  There is no CPU fallback anywhere in this
package: if the shared object is missing or no gfx950 device is usable, calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TEELINE_GPU_LIB: developer override to load a differently-built variant (tuning experiments)
LIB_PATH = os.environ.get("TEELINE_GPU_LIB") or os.path.join(_HERE, "libteeline_gpu.so")
TL_DEV_STATS_STRIDE = 16

TL_OK = 0
TL_ERR_BADARG, TL_ERR_REF_PANICS, TL_ERR_NO_DEVICE, TL_ERR_HIP = -1, -2, -3, -4
TL_ERR_NOMEM, TL_ERR_UNSUPPORTED, TL_ERR_NO_CONVERGE, TL_ERR_BUSY = -5, -6, -7, -8
TL_MODE_REF_ORDER, TL_MODE_BEST_SWEEP = 0, 1
TL_FLAG_NONE, TL_FLAG_NO_PRUNE = 0, 1
# alternative kernel forms (identical results; cross-checks of each other); _2OPT_FORCE_HBM also routes the multi-start / population entries
TL_FLAG_2OPT_FORCE_HBM, TL_FLAG_LK_ONE_WORKGROUP, TL_FLAG_LK_NO_SPLIT, TL_FLAG_LK_SPLIT2 = 1 << 1, 1 << 2, 1 << 3, 1 << 4
TL_FLAG_LK_NO_SUBCHAINS, TL_FLAG_KNN_4LANES, TL_FLAG_KNN_1LANE = 1 << 5, 1 << 6, 1 << 7
TL_FLAG_KNN_BRUTE = 1 << 10  # candidate lists by brute-force scan instead of the kd-tree walk
TL_FLAG_LK_SEPARATE_PICK = 1 << 11  # tl_lk: the pick / validate step as its own kernel (cross-check of the fused form)
TL_FLAG_LK_NO_GRAPH = 1 << 12  # tl_lk: no hipGraph replay of the round loop
TL_FLAG_LK_SEPARATE_STEP = 1 << 13  # tl_lk: k_lk_control + k_lk_rebuild instead of the chip-wide step kernel
TL_FLAG_2OPT_NT512, TL_FLAG_2OPT_NT256 = 1 << 14, 1 << 15  # LDS 2-opt: force the 8- / 4-wave form of a descent
TL_FLAG_2OPT_FX = 1 << 16  # LDS 2-opt: grid-coordinate form of the tour (two tours of n = 10^4 per CU) wherever it is exact
TL_FLAG_2OPT_NO_NL, TL_FLAG_2OPT_NL_ALWAYS = 1 << 18, 1 << 19  # LDS 2-opt: neighbour-list rows of the late sweeps off / wherever they fit
TL_FLAG_LK_SCAN_PERSIST = 1 << 17  # tl_lk (tuning build): the fused scan as a persistent grid striding over the window's pairs
TL_FLAG_LK_CHIP_WIDE = 1 << 20  # tl_lk: chip-wide scans at every n
TL_FLAG_LK_ILS_LDS = 1 << 21    # tl_lk: the single-workgroup LDS form (k_lk_ils) at every n it fits
TL_FLAG_MULTISTART_RCCL = 1 << 24  # multi-start over several devices of one process: RCCL min-all-reduce + broadcast inside the library
TL_FLAG_LK_CLASSIC_VIEW = 1 << 23  # tl_lk chip-wide: cand -> xy -> next -> xy look-ups instead of the packed records
TL_FLAG_LK_NO_SPECULATION = 1 << 22  # tl_lk, LDS form: epochs one after the other (default: a batch of consecutive epochs at once)
TL_FLAG_BHK_EXACT_WALK = 1 << 25  # tl_bellman_karp: the route by exact f32 equality instead of the reference's tolerance walk (always a tour)
TL_FLAG_OR_OPT_FORCE_SCAN = 1 << 26  # tl_or_opt_population: tour after tour through tl_or_opt's chip-wide descent at every n
TL_FLAG_3OPT_POP_FORCE_SCAN = 1 << 27  # tl_three_opt_population: tour after tour through tl_three_opt's chip-wide descent
TL_FLAG_3OPT_POP_FORCE_WG = 1 << 28  # tl_three_opt_population: one workgroup per tour wherever it fits
TL_FLAG_SA_NO_SPECULATION = 1 << 29  # tl_sim_anneal*: a window of one epoch (the chain epoch after epoch) instead of speculative windows
TL_FLAG_TABU_FULL_COMPARE = 1 << 30  # tl_tabu_search*: every tabu-list membership test compares whole routes (the cross-check form)
TL_BHK_MAX_N = 26  # tl_bellman_karp: largest n (a table of 2^(n-1) rows of 128 bytes: 4 GiB)
TL_BNB_MAX_N = 64  # tl_branch_and_bound: largest n (one wave's lanes, one 64-bit mask)
TL_FLAG_LK_SMALL = 1 << 9  # tl_lk: the LDS-resident single-workgroup form wherever it fits
TL_FLAG_COUNT_WORK = 1 << 8  # the LDS 2-opt kernel also counts the work of its cascade (stats words 5..8); ~8 % slower
TL_DM_PACKED_LOWER, TL_DM_FULL = 0, 1
TL_DIST_EUC2D, TL_DIST_GEO = 0, 1
TL_SAVINGS_HUB_AUTO = 0xFFFFFFFF  # tl_savings: the hub is tl_savings_hub(xy)

# every symbol include/teeline_gpu.h declares (tests/test_abi.py checks header <-> library <-> this list)
SYMBOLS = [
    "tl_abi_version", "tl_version", "tl_create", "tl_destroy", "tl_last_error", "tl_device_info",
    "tl_two_opt_lds_max_n", "tl_dm_build", "tl_tour_length", "tl_two_opt", "tl_three_opt",
    "tl_three_opt_find_best_move", "tl_lk", "tl_two_opt_multistart", "tl_pack_cost_key",
    "tl_two_opt_batch_dev", "tl_last_kernel_ms", "tl_dm_build_dev", "tl_build_candidates", "tl_nearest_neighbor",
    "tl_or_opt", "tl_or_opt_find_best_move", "tl_selftest_sqrt", "tl_two_opt_population", "tl_dm_is_euc2d",
    "tl_two_opt_multistart_devices", "tl_two_opt_trace", "tl_three_opt_trace", "tl_lk_trace", "tl_or_opt_trace",
    "tl_lk_live", "tl_two_opt_neighbour_lists", "tl_two_opt_plan", "tl_multistart_shard", "tl_two_opt_last_counters",
    "tl_greedy_edge", "tl_savings_hub", "tl_savings", "tl_christofides", "tl_bellman_karp",
    "tl_or_opt_population", "tl_or_opt_lds_max_n",
    "tl_two_opt_best_population", "tl_two_opt_best_lds_max_n", "tl_two_opt_best_plan", "tl_two_opt_best_force_scan",
    "tl_lk_run_seed", "tl_lk_population_max_n", "tl_lk_population_plan", "tl_lk_population_setting", "tl_lk_population",
    "tl_three_opt_population", "tl_three_opt_pop_max_n", "tl_three_opt_population_plan", "tl_three_opt_population_work_limit",
    "tl_sim_anneal", "tl_sim_anneal_trace", "tl_sim_anneal_trace_chain", "tl_sim_anneal_population", "tl_sim_anneal_lds_max_n", "tl_sim_anneal_plan",
    "tl_sa_draw", "tl_sa_schedule_epochs", "tl_sa_selftest_accept",
    "tl_tabu_search", "tl_tabu_search_trace", "tl_tabu_search_trace_chain", "tl_tabu_search_population", "tl_tabu_search_lds_max_n", "tl_tabu_search_plan",
    "tl_tabu_draw",
    "tl_genetic_algorithm", "tl_genetic_algorithm_trace", "tl_genetic_algorithm_trace_run", "tl_genetic_algorithm_population", "tl_genetic_algorithm_max_n",
    "tl_genetic_algorithm_plan", "tl_ga_draw", "tl_ga_selftest_crossover",
    "tl_ant_colony", "tl_ant_colony_trace", "tl_ant_colony_trace_run", "tl_ant_colony_population", "tl_ant_colony_max_n", "tl_ant_colony_plan",
    "tl_aco_draw", "tl_aco_pow", "tl_aco_selftest_select",
    "tl_particle_swarm", "tl_particle_swarm_trace", "tl_particle_swarm_population", "tl_particle_swarm_max_n", "tl_particle_swarm_plan",
    "tl_pso_draw", "tl_pso_weight", "tl_pso_keep", "tl_pso_selftest_swap_sequence",
    "tl_cuckoo_search", "tl_cuckoo_search_trace", "tl_cuckoo_search_population", "tl_cuckoo_search_max_n", "tl_cuckoo_search_plan",
    "tl_cs_draw", "tl_levy_from_words", "tl_cs_flight_length", "tl_cs_pa", "tl_cs_selftest_levy", "tl_cs_selftest_reversals",
    "tl_flower_pollination", "tl_flower_pollination_trace", "tl_flower_pollination_population", "tl_flower_pollination_max_n", "tl_flower_pollination_plan",
    "tl_fpa_draw", "tl_fpa_switch_prob", "tl_fpa_global_swaps", "tl_fpa_local_swaps", "tl_fpa_partners", "tl_fpa_selftest_pollinate",
    "tl_gravitational_search", "tl_gravitational_search_trace", "tl_gravitational_search_population", "tl_gravitational_search_max_n",
    "tl_gravitational_search_plan", "tl_gsa_draw", "tl_gsa_g", "tl_gsa_pull_swaps", "tl_gsa_masses", "tl_gsa_selftest_pull",
    "tl_kohonen_som", "tl_kohonen_som_trace", "tl_kohonen_som_population", "tl_kohonen_som_max_n", "tl_kohonen_som_plan",
    "tl_som_draw", "tl_som_schedule", "tl_som_h", "tl_som_ring_init", "tl_som_selftest_bmu",
    "tl_hill_climb", "tl_hill_climb_trace", "tl_hill_climb_trace_chain", "tl_hill_climb_population", "tl_hill_climb_lds_max_n", "tl_hill_climb_plan",
    "tl_hill_draw",
    "tl_fourier_curve", "tl_fourier_curve_batch", "tl_fourier_curve_work_bytes", "tl_fourier_curve_plan",
    "tl_fourier_basis", "tl_fourier_init", "tl_fourier_nearest", "tl_fourier_selftest_search",
    "tl_branch_and_bound", "tl_branch_and_bound_host", "tl_branch_and_bound_plan",
    "tl_one_tree_bound", "tl_one_tree_bound_batch", "tl_one_tree_bound_host", "tl_one_tree_bound_plan", "tl_one_tree_bound_max_n",
    "tl_one_tree_bound_work_bytes",
    "tl_alpha_candidates", "tl_alpha_candidates_host", "tl_alpha_candidates_plan", "tl_alpha_candidates_max_n", "tl_lk_candidates",
]


class TlStats(C.Structure):
    _fields_ = [("sweeps", C.c_uint64), ("candidates", C.c_uint64), ("moves", C.c_uint64),
                ("reversed", C.c_uint64), ("kernel_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TlLkOpts(C.Structure):
    _fields_ = [("epochs", C.c_uint32), ("platoo_epochs", C.c_uint32), ("n_nearest", C.c_uint32),
                ("max_depth", C.c_uint32)]


class TlSaOpts(C.Structure):
    """tl_sa_opts: SAOptions (src/tsp/mod.rs:689-706)"""
    _fields_ = [("epochs", C.c_uint32), ("cooling_rate", C.c_float), ("min_temperature", C.c_float), ("max_temperature", C.c_float)]


class TlPsoOpts(C.Structure):
    """tl_pso_opts: what particle_swarm reads of HeuristicOptions (src/tsp/mod.rs:596-611)"""
    _fields_ = [("epochs", C.c_uint32), ("n_nearest", C.c_uint32)]


class TlCsOpts(C.Structure):
    """tl_cs_opts: what cuckoo_search reads of CSOptions (src/tsp/mod.rs:913-925)"""
    _fields_ = [("epochs", C.c_uint32), ("n_nearest", C.c_uint32), ("mutation_probability", C.c_float)]


class TlFpaOpts(C.Structure):
    """tl_fpa_opts: what flower_pollination reads of FPAOptions (src/tsp/mod.rs:998-1010)"""
    _fields_ = [("epochs", C.c_uint32), ("n_nearest", C.c_uint32), ("mutation_probability", C.c_float)]


class TlGsaOpts(C.Structure):
    """tl_gsa_opts: what gravitational_search reads of HeuristicOptions (src/tsp/mod.rs:596-611), and the epochs of one launch (0: the default)"""
    _fields_ = [("epochs", C.c_uint32), ("n_nearest", C.c_uint32), ("span_epochs", C.c_uint32)]


class TlHillOpts(C.Structure):
    """tl_hill_opts: HeuristicOptions' epochs and platoo_epochs (src/tsp/mod.rs:598-608) and the window (0: the plan's, 1: the chain epoch
    after epoch)"""
    _fields_ = [("epochs", C.c_uint32), ("platoo_epochs", C.c_uint32), ("window", C.c_uint32), ("reserved", C.c_uint32)]


class TlSomOpts(C.Structure):
    """tl_som_opts: SOMOptions (src/tsp/mod.rs:1465-1499), the form of the ring (0: the plan decides, 1: LDS, 2: workspace) and the
    workspace one launch sequence plans with (0: the default)"""
    _fields_ = [("epochs", C.c_uint32), ("neuron_multiplier", C.c_uint32), ("learning_rate", C.c_double), ("radius_fraction", C.c_double),
                ("form", C.c_uint32), ("reserved", C.c_uint32), ("work_bytes", C.c_uint64)]


class TlFourierOpts(C.Structure):
    """tl_fourier_opts: FourierOptions (src/tsp/mod.rs:1341-1384) and the launch parameters (0: the plan's): the chunk of cities whose
    gradient terms are formed at once, the steps of one launch, the lanes of a workgroup"""
    _fields_ = [("k_max", C.c_uint32), ("m", C.c_uint32), ("epochs", C.c_uint32), ("chunk", C.c_uint32), ("lam", C.c_double),
                ("lambda_decay", C.c_double), ("lr", C.c_double), ("span_steps", C.c_uint32), ("threads", C.c_uint32)]


class TlBnbOpts(C.Structure):
    """tl_bnb_opts: the start position, K (0: exact), the budgets (0: none) and the launch parameters (0: the plan's)"""
    _fields_ = [("start", C.c_uint32), ("n_nearest", C.c_uint32), ("max_nodes", C.c_uint64), ("time_limit_ms", C.c_uint32),
                ("nodes_per_launch", C.c_uint32), ("frontier_depth", C.c_uint32), ("workgroups", C.c_uint32)]


class TlBnbStats(C.Structure):
    """tl_bnb_stats"""
    _fields_ = [("nodes", C.c_uint64), ("leaves", C.c_uint64), ("launches", C.c_uint64), ("queue_start", C.c_uint64), ("queue_end", C.c_uint64),
                ("wave_launches", C.c_uint64), ("idle_wave_launches", C.c_uint64), ("kernel_ms", C.c_double), ("max_launch_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TlOneTreeOpts(C.Structure):
    """tl_one_tree_opts: the 1-tree's special position, the ascent's options, the iterations of one launch (0: the plan's)"""
    _fields_ = [("root", C.c_uint32), ("iterations", C.c_uint32), ("patience", C.c_uint32), ("iters_per_launch", C.c_uint32),
                ("lambda0", C.c_double), ("upper", C.c_double), ("reserved", C.c_uint64)]


class TlOneTreeResult(C.Structure):
    """tl_one_tree_result"""
    _fields_ = [("bound", C.c_double), ("lam", C.c_double), ("best_iter", C.c_uint32), ("iterations_run", C.c_uint32), ("stop", C.c_uint32),
                ("is_tour", C.c_uint32), ("root_nb", C.c_uint32 * 2), ("tour_nb", C.c_uint32 * 2)]

    def as_dict(self):
        return dict(bound=self.bound, lam=self.lam, best_iter=self.best_iter, iterations_run=self.iterations_run, stop=self.stop,
                    is_tour=self.is_tour, root_nb=tuple(self.root_nb), tour_nb=tuple(self.tour_nb))


# tl_lk_progress_fn: void (*)(void *user, const uint32_t *best_pos, uint32_t n, float best_dist)
LK_PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_float)


class TeelineGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libteeline_gpu error {code}: {msg}")
        self.code = code


class ReferencePanics(TeelineGpuError):
    """Input on which the reference solver itself panics (e.g. two_opt with n < 3)."""


_lib = None


def load():
    """Load libteeline_gpu.so.  Raises if it has not been built — never falls back to a CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m teeline_amd.build` (hipcc, gfx950). "
            "teeline_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32, f32p = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_float)
    L.tl_abi_version.restype = i32
    L.tl_version.restype = C.c_char_p
    L.tl_create.argtypes = [i32, u32, C.POINTER(vp)]
    L.tl_destroy.argtypes = [vp]
    L.tl_destroy.restype = None
    L.tl_last_error.argtypes = [vp]
    L.tl_last_error.restype = C.c_char_p
    L.tl_device_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.c_char_p, C.c_size_t]
    L.tl_two_opt_lds_max_n.argtypes = [vp]
    L.tl_two_opt_lds_max_n.restype = u32
    L.tl_dm_build.argtypes = [vp, vp, u32, i32, i32, vp, C.POINTER(C.c_double)]
    L.tl_tour_length.argtypes = [vp, vp, vp, u32, vp, f32p]
    L.tl_dm_is_euc2d.argtypes = [vp, vp, vp, u32, C.POINTER(i32)]
    L.tl_two_opt.argtypes = [vp, vp, u32, vp, vp, i32, vp, f32p, C.POINTER(TlStats)]
    L.tl_three_opt.argtypes = [vp, vp, u32, vp, vp, vp, f32p, C.POINTER(TlStats)]
    L.tl_three_opt_find_best_move.argtypes = [vp, vp, u32, vp, vp, C.POINTER(i32), C.POINTER(u32),
                                              C.POINTER(u32), C.POINTER(u32), C.POINTER(i32), f32p]
    L.tl_lk.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlLkOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_two_opt_multistart.argtypes = [vp, vp, u32, u64, u32, u32, i32, vp, f32p, C.POINTER(u32), vp,
                                        C.POINTER(TlStats)]
    L.tl_two_opt_multistart_devices.argtypes = [C.POINTER(vp), i32, vp, u32, u64, u32, u32, i32, vp, f32p, C.POINTER(u32), vp,
                                                C.POINTER(TlStats)]
    L.tl_two_opt_population.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, C.POINTER(TlStats)]
    L.tl_two_opt_trace.argtypes = [vp, vp, u32, vp, vp, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_three_opt_trace.argtypes = [vp, vp, u32, vp, vp, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_or_opt_trace.argtypes = [vp, vp, u32, vp, vp, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_lk_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlLkOpts), u64, vp, f32p, C.POINTER(TlStats), vp, vp, u32, C.POINTER(u32)]
    L.tl_lk_live.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlLkOpts), u64, vp, f32p, C.POINTER(TlStats), LK_PROGRESS_FN, vp]
    L.tl_pack_cost_key.argtypes = [C.c_float, u32]
    L.tl_pack_cost_key.restype = u64
    L.tl_two_opt_batch_dev.argtypes = [vp, vp, u32, vp, u64, u32, u32, i32, vp, vp, vp, vp]
    L.tl_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.tl_two_opt_last_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.tl_dm_build_dev.argtypes = [vp, vp, u32, i32, i32, vp, vp]
    L.tl_build_candidates.argtypes = [vp, vp, u32, u32, vp]
    L.tl_nearest_neighbor.argtypes = [vp, vp, vp, u32, u32, vp, f32p]
    L.tl_greedy_edge.argtypes = [vp, vp, vp, u32, vp, f32p, C.POINTER(TlStats)]
    L.tl_christofides.argtypes = [vp, vp, vp, u32, vp, f32p, C.POINTER(TlStats)]
    L.tl_bellman_karp.argtypes = [vp, vp, vp, u32, vp, f32p, f32p, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_savings_hub.argtypes = [vp, u32, C.POINTER(u32)]
    L.tl_savings.argtypes = [vp, vp, vp, u32, u32, vp, f32p, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_selftest_sqrt.argtypes = [vp, u32, u64, C.POINTER(u64), C.POINTER(u32)]
    L.tl_two_opt_plan.argtypes = [u32, u32, i32, i32, u32, C.POINTER(i32), C.POINTER(i32)]
    L.tl_multistart_shard.argtypes = [u32, u32, i32, i32, C.POINTER(u32), C.POINTER(u32)]
    L.tl_two_opt_neighbour_lists.argtypes = [vp, vp, u32, i32, vp, vp, vp, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.tl_or_opt.argtypes = [vp, vp, u32, vp, vp, vp, f32p, C.POINTER(TlStats)]
    L.tl_or_opt_find_best_move.argtypes = [vp, vp, u32, vp, vp, C.POINTER(i32), f32p, C.POINTER(u32), C.POINTER(u32),
                                           C.POINTER(u32), C.POINTER(i32)]
    L.tl_or_opt_lds_max_n.argtypes = [vp]
    L.tl_or_opt_lds_max_n.restype = u32
    L.tl_or_opt_population.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, C.POINTER(TlStats)]
    L.tl_lk_run_seed.argtypes = [u64, u32]
    L.tl_lk_run_seed.restype = u64
    L.tl_lk_population_max_n.argtypes = [vp, C.POINTER(TlLkOpts)]
    L.tl_lk_population_max_n.restype = u32
    L.tl_lk_population_plan.argtypes = [u32, C.POINTER(TlLkOpts), u32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_lk_population_setting.argtypes = [vp, i32, u32]
    L.tl_lk_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlLkOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_two_opt_best_lds_max_n.argtypes = [vp]
    L.tl_two_opt_best_lds_max_n.restype = u32
    L.tl_two_opt_best_plan.argtypes = [u32, u32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.tl_two_opt_best_force_scan.argtypes = [vp, i32]
    L.tl_two_opt_best_population.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, C.POINTER(TlStats)]
    L.tl_three_opt_pop_max_n.argtypes = [vp]
    L.tl_three_opt_pop_max_n.restype = u32
    L.tl_three_opt_population.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, C.POINTER(TlStats)]
    L.tl_three_opt_population_plan.argtypes = [u32, u32, C.c_int, C.c_int, C.c_uint64, u32, C.POINTER(i32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_three_opt_population_work_limit.argtypes = [vp, C.c_uint64]
    L.tl_sim_anneal_lds_max_n.argtypes = [vp]
    L.tl_sim_anneal_lds_max_n.restype = u32
    L.tl_sim_anneal.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlSaOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_sim_anneal_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlSaOpts), u64, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_sim_anneal_trace_chain.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlSaOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_sim_anneal_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlSaOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_sa_draw.argtypes = [u64, u32, u32, u32]
    L.tl_sa_draw.restype = u64
    L.tl_sa_schedule_epochs.argtypes = [C.POINTER(TlSaOpts), C.POINTER(u64)]
    L.tl_sim_anneal_plan.argtypes = [u32, u32, i32, i32, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_sa_selftest_accept.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp]
    L.tl_tabu_search_lds_max_n.argtypes = [vp]
    L.tl_tabu_search_lds_max_n.restype = u32
    L.tl_tabu_search.argtypes = [vp, vp, u32, vp, vp, u32, u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_tabu_search_trace.argtypes = [vp, vp, u32, vp, vp, u32, u64, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_tabu_search_trace_chain.argtypes = [vp, vp, u32, vp, vp, u32, u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_tabu_search_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_tabu_draw.argtypes = [u64, u32, u32, u32, u32, u32]
    L.tl_tabu_draw.restype = u64
    L.tl_tabu_search_plan.argtypes = [u32, u32, i32, i32, u64, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_genetic_algorithm_max_n.argtypes = [vp]
    L.tl_genetic_algorithm_max_n.restype = u32
    L.tl_genetic_algorithm.argtypes = [vp, vp, u32, vp, vp, u32, C.c_float, u32, u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_genetic_algorithm_trace.argtypes = [vp, vp, u32, vp, vp, u32, C.c_float, u32, u64, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32]
    L.tl_genetic_algorithm_trace_run.argtypes = [vp, vp, u32, vp, vp, u32, C.c_float, u32, u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp,
                                                 u32]
    L.tl_genetic_algorithm_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.c_float, u32, u64, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_ga_draw.argtypes = [u64, u32, u64, u32]
    L.tl_ga_draw.restype = u64
    L.tl_genetic_algorithm_plan.argtypes = [u32, u32, i32, i32, u64, C.POINTER(u32), C.POINTER(i32), C.POINTER(u64)]
    L.tl_ga_selftest_crossover.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    f32 = C.c_float
    L.tl_ant_colony_max_n.argtypes = [vp]
    L.tl_ant_colony_max_n.restype = u32
    L.tl_ant_colony.argtypes = [vp, vp, u32, vp, vp, u32, f32, f32, f32, u32, u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_ant_colony_trace.argtypes = [vp, vp, u32, vp, vp, u32, f32, f32, f32, u32, u64, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32,
                                      C.POINTER(u32)]
    L.tl_ant_colony_trace_run.argtypes = [vp, vp, u32, vp, vp, u32, f32, f32, f32, u32, u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32,
                                          C.POINTER(u32)]
    L.tl_ant_colony_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, u32, f32, f32, f32, u32, u64, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_aco_draw.argtypes = [u64, u32, u64, u32]
    L.tl_aco_draw.restype = u64
    L.tl_aco_pow.argtypes = [f32, f32]
    L.tl_aco_pow.restype = f32
    L.tl_ant_colony_plan.argtypes = [u32, u32, u32, i32, i32, u64, C.POINTER(u32), C.POINTER(i32), C.POINTER(u64)]
    L.tl_aco_selftest_select.argtypes = [vp, vp, vp, vp, u32, f32, f32, vp]
    L.tl_particle_swarm_max_n.argtypes = [vp]
    L.tl_particle_swarm_max_n.restype = u32
    L.tl_particle_swarm.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlPsoOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_particle_swarm_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlPsoOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32, vp,
                                          u32]
    L.tl_particle_swarm_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlPsoOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_pso_draw.argtypes = [u64, u32, u64, u32]
    L.tl_pso_draw.restype = u64
    L.tl_pso_weight.argtypes = [u32, u32]
    L.tl_pso_weight.restype = C.c_double
    L.tl_pso_keep.argtypes = [C.c_double]
    L.tl_pso_keep.restype = u32
    L.tl_particle_swarm_plan.argtypes = [u32, u32, u32, i32, i32, u64, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_pso_selftest_swap_sequence.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.tl_cuckoo_search_max_n.argtypes = [vp]
    L.tl_cuckoo_search_max_n.restype = u32
    L.tl_cuckoo_search.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlCsOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_cuckoo_search_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlCsOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32, vp,
                                         u32]
    L.tl_cuckoo_search_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlCsOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_cs_draw.argtypes = [u64, u32, u64, u32]
    L.tl_cs_draw.restype = u64
    L.tl_levy_from_words.argtypes = [vp, C.POINTER(u32)]
    L.tl_levy_from_words.restype = C.c_double
    L.tl_cs_flight_length.argtypes = [C.c_double, u32]
    L.tl_cs_flight_length.restype = u32
    L.tl_cs_pa.argtypes = [f32]
    L.tl_cs_pa.restype = C.c_double
    L.tl_cuckoo_search_plan.argtypes = [u32, u32, u32, i32, i32, u64, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_cs_selftest_levy.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.tl_cs_selftest_reversals.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp]
    L.tl_flower_pollination_max_n.argtypes = [vp]
    L.tl_flower_pollination_max_n.restype = u32
    L.tl_flower_pollination.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlFpaOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_flower_pollination_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlFpaOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32,
                                              vp, u32]
    L.tl_flower_pollination_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlFpaOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_fpa_draw.argtypes = [u64, u32, u64, u32]
    L.tl_fpa_draw.restype = u64
    L.tl_fpa_switch_prob.argtypes = [f32]
    L.tl_fpa_switch_prob.restype = C.c_double
    L.tl_fpa_global_swaps.argtypes = [C.c_double, u32]
    L.tl_fpa_global_swaps.restype = u32
    L.tl_fpa_local_swaps.argtypes = [C.c_double, u32]
    L.tl_fpa_local_swaps.restype = u32
    L.tl_fpa_partners.argtypes = [u64, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.tl_flower_pollination_plan.argtypes = [u32, u32, u32, i32, i32, u64, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_fpa_selftest_pollinate.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, vp]
    L.tl_gravitational_search_max_n.argtypes = [vp]
    L.tl_gravitational_search_max_n.restype = u32
    L.tl_gravitational_search.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlGsaOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_gravitational_search_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlGsaOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32), vp, u32,
                                                vp, u32]
    L.tl_gravitational_search_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlGsaOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_gsa_draw.argtypes = [u64, u32, u64, u32]
    L.tl_gsa_draw.restype = u64
    L.tl_gsa_g.argtypes = [u32, u32]
    L.tl_gsa_g.restype = C.c_double
    L.tl_gsa_pull_swaps.argtypes = [C.c_double, C.c_double, C.c_double]
    L.tl_gsa_pull_swaps.restype = u32
    L.tl_gsa_masses.argtypes = [vp, u32, vp, vp]
    L.tl_gravitational_search_plan.argtypes = [u32, u32, u32, i32, i32, u64, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    L.tl_gsa_selftest_pull.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    f64p = C.POINTER(C.c_double)
    L.tl_kohonen_som_max_n.argtypes = [vp, u32, u32]
    L.tl_kohonen_som_max_n.restype = u32
    L.tl_kohonen_som.argtypes = [vp, vp, u32, vp, C.POINTER(TlSomOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_kohonen_som_trace.argtypes = [vp, vp, u32, vp, C.POINTER(TlSomOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, vp, vp, vp, vp, u32,
                                       C.POINTER(u32)]
    L.tl_kohonen_som_population.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(TlSomOpts), u64, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_som_draw.argtypes = [u64, u32, u32, u32]
    L.tl_som_draw.restype = u32
    L.tl_som_schedule.argtypes = [u32, u32, u32, C.c_double, C.c_double, f64p, f64p, f64p, C.POINTER(u32)]
    L.tl_som_h.argtypes = [C.c_double, C.c_double, f64p]
    L.tl_som_ring_init.argtypes = [vp, u32, u32, vp, vp]
    L.tl_kohonen_som_plan.argtypes = [u32, u32, u32, u32, i32, i32, u64, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32), C.POINTER(u32)]
    L.tl_som_selftest_bmu.argtypes = [vp, vp, u32, vp, u32, i32, u32, vp, vp, vp]
    L.tl_hill_climb_lds_max_n.argtypes = [vp]
    L.tl_hill_climb_lds_max_n.restype = u32
    L.tl_hill_climb.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlHillOpts), u64, vp, f32p, C.POINTER(TlStats)]
    L.tl_hill_climb_trace.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlHillOpts), u64, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_hill_climb_trace_chain.argtypes = [vp, vp, u32, vp, vp, C.POINTER(TlHillOpts), u64, u32, vp, f32p, C.POINTER(TlStats), vp, u32, C.POINTER(u32)]
    L.tl_hill_climb_population.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(TlHillOpts), u64, vp, vp, vp, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_hill_draw.argtypes = [u64, u32, u64, u32]
    L.tl_hill_draw.restype = u64
    L.tl_hill_climb_plan.argtypes = [u32, u32, i32, i32, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    fo = C.POINTER(TlFourierOpts)
    L.tl_fourier_curve.argtypes = [vp, vp, u32, vp, fo, vp, f32p, vp, C.POINTER(TlStats)]
    L.tl_fourier_curve_batch.argtypes = [vp, vp, u32, vp, fo, u32, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(TlStats), vp, u32, vp]
    L.tl_fourier_curve_work_bytes.argtypes = [u32, fo, u32, u32]
    L.tl_fourier_curve_work_bytes.restype = u64
    L.tl_fourier_curve_plan.argtypes = [u32, fo, u32, i32, C.POINTER(i32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.tl_fourier_basis.argtypes = [u32, vp]
    L.tl_fourier_init.argtypes = [vp, u32, u32, vp]
    L.tl_fourier_nearest.argtypes = [vp, u32, vp, u32, vp]
    L.tl_fourier_selftest_search.argtypes = [vp, vp, u32, vp, u32, i32, vp]
    bo, bs = C.POINTER(TlBnbOpts), C.POINTER(TlBnbStats)
    L.tl_branch_and_bound.argtypes = [vp, vp, vp, u32, vp, bo, vp, f32p, C.POINTER(u32), C.POINTER(u32), bs]
    L.tl_branch_and_bound_host.argtypes = [vp, vp, u32, vp, bo, vp, f32p, C.POINTER(u32), C.POINTER(u32), bs]
    L.tl_branch_and_bound_plan.argtypes = [u32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(u32), C.POINTER(u32)]
    oo, orr = C.POINTER(TlOneTreeOpts), C.POINTER(TlOneTreeResult)
    L.tl_one_tree_bound.argtypes = [vp, vp, vp, u32, oo, orr, vp, vp, vp, vp, u32, C.POINTER(TlStats)]
    L.tl_one_tree_bound_batch.argtypes = [vp, vp, vp, u32, oo, u32, orr, vp, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(TlStats)]
    L.tl_one_tree_bound_host.argtypes = [vp, vp, u32, oo, orr, vp, vp, vp, vp, u32]
    L.tl_one_tree_bound_plan.argtypes = [u32, i32, C.POINTER(i32), C.POINTER(u32)]
    L.tl_one_tree_bound_max_n.argtypes = [i32]
    L.tl_one_tree_bound_max_n.restype = u32
    L.tl_one_tree_bound_work_bytes.argtypes = [u32, u32, u32]
    L.tl_one_tree_bound_work_bytes.restype = u64
    L.tl_alpha_candidates.argtypes = [vp, vp, vp, u32, vp, u32, u32, u32, vp, vp, vp, vp, C.POINTER(TlStats)]
    L.tl_alpha_candidates_host.argtypes = [vp, vp, u32, vp, u32, u32, vp, vp, vp, vp]
    L.tl_alpha_candidates_plan.argtypes = [u32, u32, i32, C.POINTER(i32), C.POINTER(u32)]
    L.tl_alpha_candidates_max_n.argtypes = [i32]
    L.tl_alpha_candidates_max_n.restype = u32
    L.tl_lk_candidates.argtypes = [vp, vp, u32, u32]
    _lib = L
    return L
