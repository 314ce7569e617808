//! teeline-gpu — safe Rust binding of `libteeline_gpu.so` (C ABI declared in `include/teeline_gpu.h`, ABI version 5).
//!
//! The library is the MI355X (gfx950) engine that replaces the bodies of
//!   `two_opt::solve`        (src/tsp/two_opt.rs:7-67)
//!   `three_opt::solve`      (src/tsp/three_opt.rs:16-51)
//!   `lin_kernighan::solve`  (src/tsp/lin_kernighan.rs:35-100)
//!   `or_opt::solve`, `nearest_neighbor::solve`, `greedy_edge::solve`, `savings::solve`, `christofides::solve`, `bellman_karp::solve`, `DistanceMatrix::build`
//! of the `teeline` crate.  This crate knows nothing about `teeline`'s types (no dependency cycle): tours are
//! POSITIONS (indices into the city array), coordinates are `[x0, y0, x1, y1, ...]`, the optional matrix is the
//! reference's packed strict lower triangle (`DistanceMatrix::distances()`, distance_matrix.rs:171-173).
//! `src/tsp/gpu.rs` (added to the `teeline` crate by integration/patches/0001-gpu-feature.patch) maps
//! `TspProblem` / `Solution` onto these calls with the reference's exact `solve` signatures.
//!
//! Threading: a `tl_ctx` is single-threaded; `with_context` keeps one per thread, which is what the reference's callers
//! need (teeline-api runs solvers on `spawn_blocking` threads, tsp_service.rs:295,328).
//! There is no CPU fallback: without a gfx950 device every call returns `Err(Error { code: NoDevice, .. })`.

use std::cell::RefCell;
use std::ffi::{c_char, c_int, c_void, CStr};
use std::fmt;
use std::ptr;

pub const TL_ABI_VERSION: c_int = 5;

#[repr(C)]
pub struct TlCtx {
    _private: [u8; 0],
}

/// `tl_stats` (include/teeline_gpu.h)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct Stats {
    pub sweeps: u64,
    pub candidates: u64,
    pub moves: u64,
    pub reversed: u64,
    pub kernel_ms: f64,
    pub total_ms: f64,
}

/// `tl_lk_opts` = LKOptions (src/tsp/mod.rs:1249-1267)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct LkOpts {
    pub epochs: u32,
    pub platoo_epochs: u32,
    pub n_nearest: u32,
    pub max_depth: u32,
}

/// `tl_pso_opts`: what particle_swarm reads of HeuristicOptions (src/tsp/mod.rs:596-611); P = max(n_nearest, 30)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PsoOpts {
    pub epochs: u32,
    pub n_nearest: u32,
}

/// `tl_cs_opts`: what cuckoo_search reads of CSOptions (src/tsp/mod.rs:913-925); N = max(n_nearest, 25)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct CsOpts {
    pub epochs: u32,
    pub n_nearest: u32,
    pub mutation_probability: f32,
}

/// `tl_fpa_opts`: what flower_pollination reads of FPAOptions (src/tsp/mod.rs:998-1010); N = max(n_nearest, 25)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct FpaOpts {
    pub epochs: u32,
    pub n_nearest: u32,
    pub mutation_probability: f32,
}

/// `tl_som_opts`: SOMOptions (src/tsp/mod.rs:1465-1499), the form of the ring (0: the plan decides, 1: LDS, 2: workspace) and the
/// workspace one launch sequence plans with (0: the default).  The result depends on neither of the last two.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SomOpts {
    pub epochs: u32,
    pub neuron_multiplier: u32,
    pub learning_rate: f64,
    pub radius_fraction: f64,
    pub form: u32,
    pub reserved: u32,
    pub work_bytes: u64,
}

/// `tl_fourier_opts`: FourierOptions (src/tsp/mod.rs:1341-1384) and the launch parameters (0: the plan's), on none of which the
/// result depends: the chunk of cities whose gradient terms are formed at once, the steps of one launch, the lanes of a workgroup.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct FourierOpts {
    pub k_max: u32,
    pub m: u32,
    pub epochs: u32,
    pub chunk: u32,
    pub lambda: f64,
    pub lambda_decay: f64,
    pub lr: f64,
    pub span_steps: u32,
    pub threads: u32,
}

/// `tl_one_tree_opts`: one job of the Held-Karp lower bound.  `upper` is the length of any tour and has no default.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct OneTreeOpts {
    pub root: u32,
    pub iterations: u32,
    pub patience: u32,
    /// 0: the plan's; never in the result
    pub iters_per_launch: u32,
    pub lambda0: f64,
    pub upper: f64,
    pub reserved: u64,
}

impl OneTreeOpts {
    /// The defaults (root 0, 1 000 iterations, lambda0 2, patience 10) for this upper bound.
    pub fn with_upper(upper: f64) -> Self {
        OneTreeOpts { root: 0, iterations: 1000, patience: 10, iters_per_launch: 0, lambda0: 2.0, upper, reserved: 0 }
    }
}

/// `tl_one_tree_result`: stop is 1 tour, 2 lambda, 3 upper, 4 iterations (0: n <= 2).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct OneTreeResult {
    pub bound: f64,
    pub lambda: f64,
    pub best_iter: u32,
    pub iterations_run: u32,
    pub stop: u32,
    pub is_tour: u32,
    pub root_nb: [u32; 2],
    pub tour_nb: [u32; 2],
}

/// One job's outcome of `one_tree_bound_batch`: the figures, the best penalties and, where the 1-tree was a tour, that tour.
#[derive(Clone, Debug)]
pub struct OneTreeBound {
    pub result: OneTreeResult,
    pub pi: Vec<f64>,
    pub tour: Option<Vec<u32>>,
}

impl OneTreeBound {
    /// How far above the optimum a tour of this cost can be at most, in percent.
    pub fn gap_pct(&self, cost: f64) -> f64 {
        100.0 * (cost - self.result.bound) / self.result.bound
    }
}

impl Default for FourierOpts {
    fn default() -> Self {
        FourierOpts { k_max: 4, m: 200, epochs: 400, chunk: 0, lambda: 0.05, lambda_decay: 0.5, lr: 0.05, span_steps: 0, threads: 0 }
    }
}

/// `tl_hill_opts`: HeuristicOptions' epochs and platoo_epochs (src/tsp/mod.rs:598-608) and the window (0: the plan's, 1: the chain
/// epoch after epoch).  The result does not depend on the window.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct HillOpts {
    pub epochs: u32,
    pub platoo_epochs: u32,
    pub window: u32,
    pub reserved: u32,
}

impl Default for HillOpts {
    fn default() -> Self {
        HillOpts { epochs: 10_000, platoo_epochs: 500, window: 0, reserved: 0 }
    }
}

/// `tl_gsa_opts`: what gravitational_search reads of HeuristicOptions (src/tsp/mod.rs:596-611); N = max(n_nearest, 25)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GsaOpts {
    pub epochs: u32,
    pub n_nearest: u32,
    /// epochs of one launch at most; 0: the default.  The result does not depend on it.
    pub span_epochs: u32,
}

/// `tl_lk_progress_fn` (include/teeline_gpu.h): called by `tl_lk_live` on the calling thread while the search runs.
pub type LkProgressFn = unsafe extern "C" fn(user: *mut c_void, best_pos: *const u32, n: u32, best_dist: f32);

pub const MODE_REF_ORDER: c_int = 0;
pub const MODE_BEST_SWEEP: c_int = 1;
pub const DM_PACKED_LOWER: c_int = 0;
pub const DIST_EUC2D: c_int = 0;
pub const DIST_GEO: c_int = 1;

unsafe extern "C" {
    fn tl_abi_version() -> c_int;
    fn tl_create(device: c_int, flags: u32, out: *mut *mut TlCtx) -> c_int;
    fn tl_destroy(ctx: *mut TlCtx);
    fn tl_last_error(ctx: *const TlCtx) -> *const c_char;
    fn tl_dm_build(ctx: *mut TlCtx, xy: *const f32, n: u32, dist: c_int, layout: c_int, out_host: *mut f32, kernel_ms: *mut f64) -> c_int;
    fn tl_dm_is_euc2d(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, is_euc2d: *mut c_int) -> c_int;
    fn tl_tour_length(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, perm: *const u32, out_cost: *mut f32) -> c_int;
    fn tl_two_opt(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, mode: c_int,
                  out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> c_int;
    fn tl_two_opt_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, out_pos: *mut u32,
                        out_cost: *mut f32, stats: *mut Stats, move_log: *mut u32, log_cap: u32, log_len: *mut u32) -> c_int;
    fn tl_three_opt_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, out_pos: *mut u32,
                          out_cost: *mut f32, stats: *mut Stats, move_log: *mut u32, log_cap: u32, log_len: *mut u32) -> c_int;
    fn tl_or_opt_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, out_pos: *mut u32,
                       out_cost: *mut f32, stats: *mut Stats, move_log: *mut u32, log_cap: u32, log_len: *mut u32) -> c_int;
    fn tl_lk_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const LkOpts, seed: u64,
                   out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, snap_pos: *mut u32, snap_dist: *mut f32, snap_cap: u32,
                   snap_len: *mut u32) -> c_int;
    fn tl_lk_live(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const LkOpts, seed: u64,
                  out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, progress: LkProgressFn, user: *mut c_void) -> c_int;
    fn tl_three_opt(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32,
                    out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> c_int;
    fn tl_or_opt(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32,
                 out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> c_int;
    fn tl_or_opt_lds_max_n(ctx: *const TlCtx) -> u32;
    fn tl_or_opt_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, count: u32,
                            out_pos: *mut u32, out_costs: *mut f32, out_moves: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_two_opt_best_lds_max_n(ctx: *const TlCtx) -> u32;
    fn tl_two_opt_best_plan(n: u32, count: u32, cus: c_int, lds_bytes: c_int, force_scan: c_int, form: *mut c_int, threads: *mut c_int) -> c_int;
    fn tl_two_opt_best_force_scan(ctx: *mut TlCtx, on: c_int) -> c_int;
    fn tl_two_opt_best_population(ctx: *mut TlCtx, xy: *const f32, n: u32, init_pos: *const u32, count: u32, out_pos: *mut u32,
                                  out_costs: *mut f32, out_moves: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_three_opt_pop_max_n(ctx: *const TlCtx) -> u32;
    fn tl_three_opt_population_plan(n: u32, count: u32, cus: c_int, lds_bytes: c_int, work_bytes: u64, flags: u32, form: *mut c_int,
                                    threads: *mut c_int, batch: *mut u32) -> c_int;
    fn tl_three_opt_population_work_limit(ctx: *mut TlCtx, bytes: u64) -> c_int;
    fn tl_three_opt_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, count: u32,
                               out_pos: *mut u32, out_costs: *mut f32, out_moves: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_lk(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const LkOpts, seed: u64,
             out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> c_int;
    fn tl_lk_run_seed(seed: u64, run: u32) -> u64;
    fn tl_lk_population_max_n(ctx: *const TlCtx, opts: *const LkOpts) -> u32;
    fn tl_lk_population_plan(n: u32, opts: *const LkOpts, count: u32, cus: c_int, lds_bytes: c_int, force_form: c_int, form: *mut c_int,
                             threads: *mut c_int, per_cu: *mut u32) -> c_int;
    fn tl_lk_population_setting(ctx: *mut TlCtx, force_form: c_int, slice_scans: u32) -> c_int;
    fn tl_lk_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32, first_run: u32,
                        count: u32, opts: *const LkOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32, out_counters: *mut u64,
                        best_index: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_sim_anneal_lds_max_n(ctx: *const TlCtx) -> u32;
    fn tl_sim_anneal(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const SaOpts, seed: u64,
                     out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> c_int;
    fn tl_sim_anneal_trace_chain(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const SaOpts, seed: u64,
                                 chain: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, move_log: *mut u32, log_cap: u32,
                                 log_len: *mut u32) -> c_int;
    fn tl_sim_anneal_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                first_chain: u32, count: u32, opts: *const SaOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_sa_draw(seed: u64, chain: u32, epoch: u32, slot: u32) -> u64;
    fn tl_sa_schedule_epochs(opts: *const SaOpts, epochs: *mut u64) -> c_int;
    fn tl_tabu_search_lds_max_n(ctx: *const TlCtx) -> u32;
    fn tl_tabu_search(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, epochs: u32, seed: u64,
                      out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> c_int;
    fn tl_tabu_search_trace_chain(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, epochs: u32, seed: u64,
                                  chain: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, move_log: *mut u32, log_cap: u32,
                                  log_len: *mut u32) -> c_int;
    fn tl_tabu_search_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                 first_chain: u32, count: u32, epochs: u32, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                 out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_tabu_draw(seed: u64, chain: u32, n: u32, epoch: u32, attempt: u32, slot: u32) -> u64;
    fn tl_genetic_algorithm_max_n(ctx: *const TlCtx) -> u32;
    fn tl_genetic_algorithm(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, epochs: u32, mutation_probability: f32,
                            n_elite: u32, seed: u64, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_genetic_algorithm_trace_run(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, epochs: u32,
                                      mutation_probability: f32, n_elite: u32, seed: u64, run: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats,
                                      log: *mut u32, log_cap: u32, log_len: *mut u32, route_log: *mut u32, route_cap: u32) -> i32;
    fn tl_genetic_algorithm_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, first_run: u32, count: u32,
                                       epochs: u32, mutation_probability: f32, n_elite: u32, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                       best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_ga_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64;
    fn tl_ant_colony_max_n(ctx: *const TlCtx) -> u32;
    fn tl_ant_colony(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, epochs: u32, alpha: f32, beta: f32,
                     evaporation_rate: f32, num_ants: u32, seed: u64, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_ant_colony_trace_run(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, epochs: u32, alpha: f32, beta: f32,
                               evaporation_rate: f32, num_ants: u32, seed: u64, run: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats,
                               log: *mut u32, log_cap: u32, log_len: *mut u32, route_log: *mut u32, route_cap: u32, route_len: *mut u32) -> i32;
    fn tl_ant_colony_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32, first_run: u32,
                                count: u32, epochs: u32, alpha: f32, beta: f32, evaporation_rate: f32, num_ants: u32, seed: u64, out_pos: *mut u32,
                                out_costs: *mut f32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_aco_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64;
    fn tl_aco_pow(x: f32, a: f32) -> f32;
    fn tl_particle_swarm_max_n(ctx: *const TlCtx) -> u32;
    fn tl_particle_swarm(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const PsoOpts, seed: u64,
                         out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_particle_swarm_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const PsoOpts, seed: u64,
                               run: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, log: *mut u32, log_cap: u32, log_len: *mut u32,
                               route_log: *mut u32, route_cap: u32, epoch_log: *mut u32, epoch_cap: u32) -> i32;
    fn tl_particle_swarm_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                    first_run: u32, count: u32, opts: *const PsoOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                    out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_pso_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64;
    fn tl_pso_weight(epoch: u32, epochs: u32) -> f64;
    fn tl_pso_keep(x: f64) -> u32;
    fn tl_cuckoo_search_max_n(ctx: *const TlCtx) -> u32;
    fn tl_cuckoo_search(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const CsOpts, seed: u64,
                        out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_cuckoo_search_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const CsOpts, seed: u64,
                              run: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, log: *mut u32, log_cap: u32, log_len: *mut u32,
                              route_log: *mut u32, route_cap: u32, epoch_log: *mut u32, epoch_cap: u32) -> i32;
    fn tl_cuckoo_search_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                   first_run: u32, count: u32, opts: *const CsOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                   out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_cs_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64;
    fn tl_levy_from_words(words: *const u64, resamples: *mut u32) -> f64;
    fn tl_cs_flight_length(levy: f64, n: u32) -> u32;
    fn tl_cs_pa(mutation_probability: f32) -> f64;
    fn tl_flower_pollination_max_n(ctx: *const TlCtx) -> u32;
    fn tl_flower_pollination(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const FpaOpts, seed: u64,
                             out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_flower_pollination_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const FpaOpts, seed: u64,
                                   run: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, log: *mut u32, log_cap: u32, log_len: *mut u32,
                                   route_log: *mut u32, route_cap: u32, epoch_log: *mut u32, epoch_cap: u32) -> i32;
    fn tl_flower_pollination_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                        first_run: u32, count: u32, opts: *const FpaOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                        out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_fpa_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64;
    fn tl_fpa_switch_prob(mutation_probability: f32) -> f64;
    fn tl_fpa_global_swaps(levy: f64, len: u32) -> u32;
    fn tl_fpa_local_swaps(epsilon: f64, len: u32) -> u32;
    fn tl_fpa_partners(seed: u64, run: u32, epoch: u32, i: u32, flowers: u32, j: *mut u32, k: *mut u32) -> i32;
    fn tl_gravitational_search_max_n(ctx: *const TlCtx) -> u32;
    fn tl_gravitational_search(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const GsaOpts, seed: u64,
                               out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_gravitational_search_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const GsaOpts, seed: u64,
                                     run: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, log: *mut u32, log_cap: u32, log_len: *mut u32,
                                     route_log: *mut u32, route_cap: u32, epoch_log: *mut u32, epoch_cap: u32) -> i32;
    fn tl_gravitational_search_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                          first_run: u32, count: u32, opts: *const GsaOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                          out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_gsa_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64;
    fn tl_gsa_g(epoch: u32, epochs: u32) -> f64;
    fn tl_gsa_pull_swaps(r: f64, g: f64, mass: f64) -> u32;
    fn tl_gsa_masses(costs: *const f32, agents: u32, out_masses: *mut f64, out_rank: *mut u32) -> i32;
    fn tl_kohonen_som_max_n(ctx: *const TlCtx, neuron_multiplier: u32, form: u32) -> u32;
    fn tl_kohonen_som(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, opts: *const SomOpts, seed: u64, out_pos: *mut u32, out_cost: *mut f32,
                      stats: *mut Stats) -> i32;
    fn tl_kohonen_som_trace(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, opts: *const SomOpts, seed: u64, run: u32, out_pos: *mut u32,
                            out_cost: *mut f32, stats: *mut Stats, log: *mut u32, log_cap: u32, out_ring: *mut f64, cp_epochs: *mut u32, cp_tours: *mut u32,
                            cp_cost_bits: *mut u32, cp_cap: u32, cp_len: *mut u32) -> i32;
    fn tl_kohonen_som_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, first_run: u32, count: u32, opts: *const SomOpts, seed: u64,
                                 out_pos: *mut u32, out_costs: *mut f32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_som_draw(seed: u64, run: u32, epoch: u32, n: u32) -> u32;
    fn tl_som_schedule(epoch: u32, epochs: u32, neurons: u32, learning_rate: f64, radius_fraction: f64, eta: *mut f64, sigma: *mut f64, two_sigma_sq: *mut f64,
                       radius: *mut u32) -> i32;
    fn tl_som_h(d: f64, two_sigma_sq: f64, h: *mut f64) -> i32;
    fn tl_som_ring_init(xy: *const f32, n: u32, neuron_multiplier: u32, out_ring: *mut f64, out_cities: *mut f64) -> i32;
    fn tl_hill_climb_lds_max_n(ctx: *const TlCtx) -> u32;
    fn tl_hill_climb(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const HillOpts, seed: u64,
                     out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats) -> i32;
    fn tl_hill_climb_trace_chain(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, opts: *const HillOpts, seed: u64,
                                 chain: u32, out_pos: *mut u32, out_cost: *mut f32, stats: *mut Stats, log: *mut u32, log_cap: u32,
                                 log_len: *mut u32) -> i32;
    fn tl_hill_climb_population(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, init_pos: *const u32, init_count: u32,
                                first_chain: u32, count: u32, opts: *const HillOpts, seed: u64, out_pos: *mut u32, out_costs: *mut f32,
                                out_moves: *mut u32, best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_hill_draw(seed: u64, chain: u32, event: u64, slot: u32) -> u64;
    fn tl_fourier_curve_batch(ctx: *mut TlCtx, xy: *const f32, n: u32, dm_packed: *const f32, opts: *const FourierOpts, jobs: u32, out_pos: *mut u32,
                              out_costs: *mut f32, out_coeffs: *mut f64, coeff_stride: u32, best_index: *mut u32, stats: *mut Stats, log: *mut u32,
                              log_cap: u32, stage_coeffs: *mut f64) -> i32;
    fn tl_fourier_curve_work_bytes(n: u32, opts: *const FourierOpts, jobs: u32, log_cap: u32) -> u64;
    fn tl_one_tree_bound_batch(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, opts: *const OneTreeOpts, jobs: u32,
                               results: *mut OneTreeResult, out_pi: *mut f64, out_parent: *mut u32, out_tour: *mut u32, log: *mut f64, log_cap: u32,
                               best_index: *mut u32, stats: *mut Stats) -> i32;
    fn tl_one_tree_bound_host(xy: *const f32, dm_packed: *const f32, n: u32, opts: *const OneTreeOpts, result: *mut OneTreeResult, out_pi: *mut f64,
                              out_parent: *mut u32, out_tour: *mut u32, log: *mut f64, log_cap: u32) -> i32;
    fn tl_one_tree_bound_plan(n: u32, lds_bytes: c_int, threads: *mut c_int, iters_per_launch: *mut u32) -> i32;
    fn tl_one_tree_bound_max_n(lds_bytes: c_int) -> u32;
    fn tl_one_tree_bound_work_bytes(n: u32, jobs: u32, log_cap: u32) -> u64;
    fn tl_alpha_candidates(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, pi: *const f64, root: u32, k: u32, threads: u32,
                           out_cand: *mut u32, out_alpha: *mut f64, out_parent: *mut u32, out_root_nb: *mut u32, stats: *mut Stats) -> i32;
    fn tl_alpha_candidates_host(xy: *const f32, dm_packed: *const f32, n: u32, pi: *const f64, root: u32, k: u32, out_cand: *mut u32,
                                out_alpha: *mut f64, out_parent: *mut u32, out_root_nb: *mut u32) -> i32;
    fn tl_alpha_candidates_plan(n: u32, k: u32, lds_bytes: c_int, threads: *mut c_int, lds_used: *mut u32) -> i32;
    fn tl_alpha_candidates_max_n(lds_bytes: c_int) -> u32;
    fn tl_lk_candidates(ctx: *mut TlCtx, cand: *const u32, n: u32, k: u32) -> i32;
    fn tl_nearest_neighbor(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, n_nearest: u32,
                           out_pos: *mut u32, out_cost: *mut f32) -> c_int;
    fn tl_greedy_edge(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, out_pos: *mut u32, out_cost: *mut f32,
                      stats: *mut Stats) -> c_int;
    fn tl_christofides(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, out_pos: *mut u32, out_cost: *mut f32,
                       stats: *mut Stats) -> c_int;
    fn tl_bellman_karp(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, out_pos: *mut u32, out_cost: *mut f32,
                       out_optimal: *mut f32, out_is_tour: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_savings_hub(xy: *const f32, n: u32, out_hub: *mut u32) -> c_int;
    fn tl_savings(ctx: *mut TlCtx, xy: *const f32, dm_packed: *const f32, n: u32, hub: u32, out_pos: *mut u32, out_cost: *mut f32,
                  out_hub: *mut u32, stats: *mut Stats) -> c_int;
    fn tl_two_opt_multistart_devices(ctxs: *const *mut TlCtx, n_ctxs: c_int, xy: *const f32, n: u32, seed: u64, first: u32, count: u32,
                                     mode: c_int, out_best_pos: *mut u32, out_best_cost: *mut f32, out_best_restart: *mut u32,
                                     out_costs: *mut f32, stats: *mut Stats) -> c_int;
}

/// `tl_sa_opts` (SAOptions, mod.rs:689-706)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SaOpts {
    pub epochs: u32,
    pub cooling_rate: f32,
    pub min_temperature: f32,
    pub max_temperature: f32,
}

impl Default for SaOpts {
    fn default() -> Self {
        SaOpts { epochs: 10_000, cooling_rate: 1e-4, min_temperature: 1e-3, max_temperature: 1000.0 }
    }
}

/// u(seed, chain, epoch, slot) of the library's seeded stream (host only).
pub fn sa_draw(seed: u64, chain: u32, epoch: u32, slot: u32) -> u64 {
    // SAFETY: a pure function of its arguments.
    unsafe { tl_sa_draw(seed, chain, epoch, slot) }
}

/// u(seed, chain, epoch (n + 1) + attempt, slot): the draw of candidate `attempt` of a tabu-search epoch on n cities (host only).
pub fn tabu_draw(seed: u64, chain: u32, n: u32, epoch: u32, attempt: u32, slot: u32) -> u64 {
    // SAFETY: a pure function of its arguments.
    unsafe { tl_tabu_draw(seed, chain, n, epoch, attempt, slot) }
}

/// u(seed, chain, event, slot): a draw of the hill climb's stream (host only): the pair of epoch e on event e, slots 0 .. 21; the restart
/// after epoch e on the events 2^58 + e n + j, slot 26.
pub fn hill_draw(seed: u64, chain: u32, event: u64, slot: u32) -> u64 {
    // SAFETY: a pure function of its arguments.
    unsafe { tl_hill_draw(seed, chain, event, slot) }
}

/// u(seed, run, event, slot): a draw of the genetic algorithm's stream (host only; the events are laid out in include/teeline_gpu.h).
pub fn ga_draw(seed: u64, run: u32, event: u64, slot: u32) -> u64 {
    // SAFETY: a pure function of its arguments.
    unsafe { tl_ga_draw(seed, run, event, slot) }
}

/// The epochs `while epoch < epochs || temperature > min_temperature` runs (138 149 with the defaults); None beyond 2^32 - 1.
pub fn sa_schedule_epochs(opts: SaOpts) -> Option<u64> {
    let mut e = 0u64;
    // SAFETY: both pointers are to live locals.
    if unsafe { tl_sa_schedule_epochs(&opts, &mut e) } == 0 { Some(e) } else { None }
}

/// `tl_status` (include/teeline_gpu.h)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Code {
    BadArg,
    /// Input on which the reference solver itself panics (e.g. `two_opt::solve` with fewer than 3 cities underflows
    /// `n_indices - 2`, two_opt.rs:17,29); the shim turns this into `panic!`.
    RefPanics,
    NoDevice,
    Hip,
    NoMem,
    Unsupported,
    NoConverge,
    /// Another thread is inside a call with the same context (`with_context` keeps one per thread, so this crate never sees it).
    Busy,
    Other(i32),
}

impl Code {
    fn from_raw(rc: c_int) -> Code {
        match rc {
            -1 => Code::BadArg,
            -2 => Code::RefPanics,
            -3 => Code::NoDevice,
            -4 => Code::Hip,
            -5 => Code::NoMem,
            -6 => Code::Unsupported,
            -7 => Code::NoConverge,
            -8 => Code::Busy,
            x => Code::Other(x),
        }
    }
}

#[derive(Clone, Debug)]
pub struct Error {
    pub code: Code,
    pub message: String,
}

impl fmt::Display for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "libteeline_gpu {:?}: {}", self.code, self.message)
    }
}

impl std::error::Error for Error {}

/// Result of a solver call: the tour as positions, its cost as `DistanceMatrix::tour_length_by_pos` sums it
/// (distance_matrix.rs:235-245, bit for bit), and the counters.
#[derive(Clone, Debug)]
pub struct Tour {
    pub pos: Vec<u32>,
    pub cost: f32,
    pub stats: Stats,
}

/// One `tl_ctx`: a HIP stream and a device workspace on one GPU.  `!Sync`, `!Send`: use it from the thread that made it.
pub struct Context {
    raw: *mut TlCtx,
}

fn opt_ptr<T>(s: Option<&[T]>) -> *const T {
    s.map_or(ptr::null(), |v| v.as_ptr())
}

impl Context {
    pub fn new(device: i32, flags: u32) -> Result<Context, Error> {
        // SAFETY: plain C calls; `raw` is written by tl_create on success only.
        unsafe {
            if tl_abi_version() != TL_ABI_VERSION {
                return Err(Error { code: Code::Other(0), message: format!("libteeline_gpu ABI {} != {}", tl_abi_version(), TL_ABI_VERSION) });
            }
            let mut raw: *mut TlCtx = ptr::null_mut();
            let rc = tl_create(device, flags, &mut raw);
            if rc != 0 {
                let msg = CStr::from_ptr(tl_last_error(ptr::null())).to_string_lossy().into_owned();
                return Err(Error { code: Code::from_raw(rc), message: msg });
            }
            Ok(Context { raw })
        }
    }

    fn check(&self, rc: c_int) -> Result<(), Error> {
        if rc == 0 {
            return Ok(());
        }
        if rc == -8 {
            // TL_ERR_BUSY: the context's error string belongs to the thread that is inside the library; it is not read
            return Err(Error { code: Code::Busy, message: "the context is in use by another thread".to_string() });
        }
        // SAFETY: tl_last_error returns a NUL-terminated string owned by the context.
        let msg = unsafe { CStr::from_ptr(tl_last_error(self.raw)).to_string_lossy().into_owned() };
        Err(Error { code: Code::from_raw(rc), message: msg })
    }

    fn n_of(xy: &[f32]) -> u32 {
        assert!(xy.len() % 2 == 0, "xy holds (x, y) pairs");
        u32::try_from(xy.len() / 2).expect("more than u32::MAX cities")
    }

    fn check_inputs(n: u32, dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>) {
        let n = n as usize;
        if let Some(d) = dm_packed {
            assert_eq!(d.len(), n * n.saturating_sub(1) / 2, "dm_packed length != n(n-1)/2");
        }
        if let Some(p) = init_pos {
            assert_eq!(p.len(), n, "init tour length != number of cities");
        }
    }

    /// `DistanceMatrix::build` (distance_matrix.rs:122-153): packed strict lower triangle, EUC_2D or GEO.
    pub fn dm_build(&self, xy: &[f32], geo: bool) -> Result<Vec<f32>, Error> {
        let n = Self::n_of(xy);
        let mut out = vec![0f32; (n as usize) * (n as usize).saturating_sub(1) / 2];
        // SAFETY: out has n(n-1)/2 elements, xy has 2n.
        let rc = unsafe { tl_dm_build(self.raw, xy.as_ptr(), n, if geo { DIST_GEO } else { DIST_EUC2D }, DM_PACKED_LOWER, out.as_mut_ptr(), ptr::null_mut()) };
        self.check(rc).map(|_| out)
    }

    /// Does `dm_packed` hold exactly the EUC_2D distances of `xy`?  (`DistanceMatrix` keeps no distance type,
    /// distance_matrix.rs:86-93.)  If so the coordinate kernels give the same tours without the matrix.
    pub fn dm_is_euc2d(&self, xy: &[f32], dm_packed: &[f32]) -> Result<bool, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, Some(dm_packed), None);
        let mut flag: c_int = 0;
        // SAFETY: lengths checked above.
        let rc = unsafe { tl_dm_is_euc2d(self.raw, xy.as_ptr(), dm_packed.as_ptr(), n, &mut flag) };
        self.check(rc).map(|_| flag != 0)
    }

    /// `DistanceMatrix::tour_length_by_pos` (distance_matrix.rs:235-245).
    pub fn tour_length(&self, xy: &[f32], dm_packed: Option<&[f32]>, perm: &[u32]) -> Result<f32, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, Some(perm));
        let mut cost = 0f32;
        // SAFETY: lengths checked above.
        let rc = unsafe { tl_tour_length(self.raw, if dm_packed.is_some() { ptr::null() } else { xy.as_ptr() }, opt_ptr(dm_packed), n, perm.as_ptr(), &mut cost) };
        self.check(rc).map(|_| cost)
    }

    /// `two_opt::solve` (two_opt.rs:7-67).  `mode` = MODE_REF_ORDER reproduces the reference's tours.
    pub fn two_opt(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, mode: c_int) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: every buffer has the length the C ABI documents (n, 2n, n(n-1)/2), checked above.
        let rc = unsafe { tl_two_opt(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), mode, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// `two_opt::solve` together with the moves it applied, `(i, j)` in the reference's order (`swap_2opt(path, i+1, j)`,
    /// two_opt.rs:50): what `gpu::two_opt::solve` replays the reference's per-move progress messages from.  Coordinates
    /// (`dm_packed` None; `Err(Unsupported)` beyond the LDS-resident descent) or the matrix form.
    /// The list holds `Some((i, j))` per move and `None` where a new sweep begins (`TL_TRACE_SWEEP`).
    pub fn two_opt_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>) -> Result<(Tour, Vec<Option<(u32, u32)>>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut cap = (16 * n).max(64);
        loop {
            let mut log = vec![0u32; cap as usize];
            let mut len = 0u32;
            // SAFETY: every buffer has the length the C ABI documents (n, 2n, n(n-1)/2, log_cap), checked above.
            let rc = unsafe {
                tl_two_opt_trace(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats,
                                 log.as_mut_ptr(), cap, &mut len)
            };
            self.check(rc)?;
            if len <= cap {
                log.truncate(len as usize);
                return Ok((t, log.into_iter().map(|w| if w == 0xFFFF_FFFF { None } else { Some((w >> 16, w & 0xFFFF)) }).collect()));
            }
            cap = len; // the descent is deterministic: once more with room for every move
        }
    }

    /// `three_opt::solve` together with the moves it applied, `(i, j, k, case)` in order (three_opt.rs:36-45): what
    /// `gpu::three_opt::solve` replays the reference's per-move `PathUpdate`s from.
    pub fn three_opt_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>) -> Result<(Tour, Vec<[u32; 4]>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut cap = (4 * n).max(64);
        loop {
            let mut log = vec![0u32; 4 * cap as usize];
            let mut len = 0u32;
            // SAFETY: as in two_opt_trace; the log holds 4 words per move.
            let rc = unsafe {
                tl_three_opt_trace(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats,
                                   log.as_mut_ptr(), cap, &mut len)
            };
            self.check(rc)?;
            if len <= cap {
                return Ok((t, log.chunks_exact(4).take(len as usize).map(|m| [m[0], m[1], m[2], m[3]]).collect()));
            }
            cap = len;
        }
    }

    /// `or_opt::solve` together with the moves it applied, `(i, j, seg_len, reversed)` in order (or_opt.rs:45-51): what
    /// `gpu::or_opt::solve` replays the reference's per-move `PathUpdate`s from.
    pub fn or_opt_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>) -> Result<(Tour, Vec<[u32; 4]>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut cap = (4 * n).max(64);
        loop {
            let mut log = vec![0u32; 4 * cap as usize];
            let mut len = 0u32;
            // SAFETY: as in two_opt_trace; the log holds 4 words per move.
            let rc = unsafe {
                tl_or_opt_trace(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats,
                                log.as_mut_ptr(), cap, &mut len)
            };
            self.check(rc)?;
            if len <= cap {
                return Ok((t, log.chunks_exact(4).take(len as usize).map(|m| [m[0], m[1], m[2], m[3]]).collect()));
            }
            cap = len;
        }
    }

    /// `lin_kernighan::solve` together with every best tour it settles on and its `best_dist`, in order (lin_kernighan.rs:71,90):
    /// what `gpu::lin_kernighan::solve` sends as `PathUpdate`s.
    pub fn lin_kernighan_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: LkOpts, seed: u64)
                               -> Result<(Tour, Vec<(Vec<u32>, f32)>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut cap = (opts.epochs + 1).min(64).max(1);
        loop {
            let mut snaps = vec![0u32; cap as usize * n as usize];
            let mut dists = vec![0f32; cap as usize];
            let mut len = 0u32;
            // SAFETY: as in two_opt_trace; snap_pos holds snap_cap x n positions, snap_dist snap_cap values.
            let rc = unsafe {
                tl_lk_trace(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats,
                            snaps.as_mut_ptr(), dists.as_mut_ptr(), cap, &mut len)
            };
            self.check(rc)?;
            if len <= cap {
                let list = snaps.chunks_exact(n as usize).take(len as usize).zip(dists).map(|(p, d)| (p.to_vec(), d)).collect();
                return Ok((t, list));
            }
            cap = len; // deterministic for a seed: once more with room for every snapshot
        }
    }

    /// `lin_kernighan::solve` with `on_best(best_tour positions, best_dist)` called WHILE the search runs, once per best tour the ILS
    /// settles on, in order (lin_kernighan.rs:71,90) — `tl_lk_live`; what `gpu::lin_kernighan::solve` forwards to its channel.
    pub fn lin_kernighan_live<F: FnMut(&[u32], f32)>(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: LkOpts, seed: u64,
                                                     mut on_best: F) -> Result<Tour, Error> {
        unsafe extern "C" fn trampoline<F: FnMut(&[u32], f32)>(user: *mut c_void, best_pos: *const u32, n: u32, best_dist: f32) {
            // SAFETY: `user` is the `&mut F` handed to tl_lk_live below, alive for the whole call; best_pos holds n positions for the
            // duration of this callback.  A panic must not unwind into C: it aborts the process, like the reference's panics do not.
            let f = unsafe { &mut *(user as *mut F) };
            let tour = unsafe { std::slice::from_raw_parts(best_pos, n as usize) };
            if std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| f(tour, best_dist))).is_err() {
                std::process::abort();
            }
        }
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt; the callback and its state outlive the call.
        let rc = unsafe {
            tl_lk_live(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats,
                       trampoline::<F>, &mut on_best as *mut F as *mut c_void)
        };
        self.check(rc).map(|_| t)
    }

    /// `three_opt::solve` (three_opt.rs:16-51).
    pub fn three_opt(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_three_opt(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// `simulated_annealing::solve` (simulated_annealing.rs:10-83), chain 0 of `seed`.  The chain is the reference's; its random draws
    /// and the evaluation of exp are the library's own specification (include/teeline_gpu.h).  (Written against the header; not
    /// compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn sim_anneal(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: SaOpts, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt; opts is a plain struct that lives across the call.
        let rc = unsafe { tl_sim_anneal(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// Chain `chain` of `seed` with its accepted epochs `[epoch, from, to, cost bits]`, from which the reference's PathUpdate
    /// messages are replayed.
    pub fn sim_anneal_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: SaOpts, seed: u64, chain: u32)
                            -> Result<(Tour, Vec<[u32; 4]>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut cap: u32 = 1 << 14;
        loop {
            let mut log = vec![[0u32; 4]; cap as usize];
            let mut len: u32 = 0;
            // SAFETY: as in two_opt; log holds cap entries of 4 words.
            let rc = unsafe {
                tl_sim_anneal_trace_chain(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, chain, t.pos.as_mut_ptr(), &mut t.cost,
                                          &mut t.stats, log.as_mut_ptr() as *mut u32, cap, &mut len)
            };
            self.check(rc)?;
            if len <= cap {
                log.truncate(len as usize);
                return Ok((t, log));
            }
            cap = len;
        }
    }

    /// Chains `first_chain .. first_chain + count` of `seed` at once, every chain from `init_pos` (or city order); the tours and the
    /// index of the best one (lowest cost, then lowest chain).
    pub fn sim_anneal_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, first_chain: u32, count: u32, opts: SaOpts,
                                 seed: u64) -> Result<(Vec<Tour>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut pos = vec![0u32; n as usize * count as usize];
        let mut costs = vec![0f32; count as usize];
        let mut moves = vec![0u32; count as usize];
        let (mut best, mut st) = (0u32, Stats::default());
        // SAFETY: as in two_opt; the output arrays hold count x n, count and count entries.
        let rc = unsafe {
            tl_sim_anneal_population(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), if init_pos.is_some() { 1 } else { 0 }, first_chain,
                                     count, &opts, seed, pos.as_mut_ptr(), costs.as_mut_ptr(), moves.as_mut_ptr(), &mut best, &mut st)
        };
        self.check(rc)?;
        let tours = (0..count as usize)
            .map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: Stats { moves: moves[k] as u64, ..st } })
            .collect();
        Ok((tours, best))
    }

    /// Largest n of `sim_anneal` (the chain lives in one CU's LDS, 12 bytes per city).
    pub fn sim_anneal_lds_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_sim_anneal_lds_max_n(self.raw) }
    }

    /// `tabu_search::solve` (tabu_search.rs:9-110), chain 0 of `seed`: `epochs + 1` epochs, the best route seen.  The chain is the
    /// reference's; its random draws are the library's own specification (include/teeline_gpu.h).  (Written against the header; not
    /// compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn tabu_search(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_tabu_search(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), epochs, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// Chain `chain` of `seed` with every epoch `[taken attempt, from, to, cost bits]`, from which the reference's PathUpdate messages
    /// (one per new best) are replayed.
    pub fn tabu_search_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, seed: u64, chain: u32)
                             -> Result<(Tour, Vec<[u32; 4]>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let cap: u32 = epochs.saturating_add(1);
        let mut log = vec![[0u32; 4]; cap as usize];
        let mut len: u32 = 0;
        // SAFETY: as in two_opt; log holds cap entries of 4 words.
        let rc = unsafe {
            tl_tabu_search_trace_chain(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), epochs, seed, chain, t.pos.as_mut_ptr(), &mut t.cost,
                                       &mut t.stats, log.as_mut_ptr() as *mut u32, cap, &mut len)
        };
        self.check(rc)?;
        log.truncate(len.min(cap) as usize);
        Ok((t, log))
    }

    /// Chains `first_chain .. first_chain + count` of `seed` at once, every chain from `init_pos` (or city order); the best routes and
    /// the index of the best one (lowest cost, then lowest chain).
    pub fn tabu_search_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, first_chain: u32, count: u32, epochs: u32,
                                  seed: u64) -> Result<(Vec<Tour>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut pos = vec![0u32; n as usize * count as usize];
        let mut costs = vec![0f32; count as usize];
        let mut moves = vec![0u32; count as usize];
        let (mut best, mut st) = (0u32, Stats::default());
        // SAFETY: as in two_opt; the output arrays hold count x n, count and count entries.
        let rc = unsafe {
            tl_tabu_search_population(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), if init_pos.is_some() { 1 } else { 0 }, first_chain,
                                      count, epochs, seed, pos.as_mut_ptr(), costs.as_mut_ptr(), moves.as_mut_ptr(), &mut best, &mut st)
        };
        self.check(rc)?;
        let tours = (0..count as usize)
            .map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: Stats { moves: moves[k] as u64, ..st } })
            .collect();
        Ok((tours, best))
    }

    /// Largest n of `tabu_search` (the current tour lives in one CU's LDS, 12 bytes per city; the list's entries are 16 bits wide).
    pub fn tabu_search_lds_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_tabu_search_lds_max_n(self.raw) }
    }

    /// `genetic_algorithm::solve` (genetic_algorithm.rs:16-336), run 0 of `seed`.  The algorithm is the reference's; its random draws are
    /// the library's own specification (include/teeline_gpu.h).  (Written against the header; not compiled here: no Rust toolchain on
    /// the build machine, see scripts/check_rust.sh.)
    pub fn genetic_algorithm(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, mutation_probability: f32, n_elite: u32,
                             seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe {
            tl_genetic_algorithm(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), epochs, mutation_probability, n_elite, seed, t.pos.as_mut_ptr(),
                                 &mut t.cost, &mut t.stats)
        };
        self.check(rc).map(|_| t)
    }

    /// `ant_colony::solve` (ant_colony.rs:97-252), run 0 of `seed`.  The algorithm is the reference's; its random draws and its power
    /// function are the library's own specification (include/teeline_gpu.h).  (Written against the header; not compiled here: no Rust
    /// toolchain on the build machine, see scripts/check_rust.sh.)
    #[allow(clippy::too_many_arguments)]
    pub fn ant_colony(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, alpha: f32, beta: f32, evaporation_rate: f32,
                      num_ants: u32, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe {
            tl_ant_colony(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), epochs, alpha, beta, evaporation_rate, num_ants, seed,
                          t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats)
        };
        self.check(rc).map(|_| t)
    }

    /// `particle_swarm::solve` (particle_swarm.rs:22-129), run 0 of `seed`, max(n_nearest, 30) particles.  The algorithm is the reference's;
    /// its random draws and its rounding are the library's own specification (include/teeline_gpu.h).  (Written against the header; not
    /// compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn particle_swarm(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, n_nearest: u32, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let opts = PsoOpts { epochs, n_nearest };
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: the slices hold n cities / n positions (check_inputs); the outputs are sized for n.
        let rc = unsafe {
            tl_particle_swarm(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats)
        };
        self.check(rc).map(|_| t)
    }

    /// `cuckoo_search::solve` (cuckoo_search.rs:26-136), run 0 of `seed`, max(n_nearest, 25) nests.  The algorithm is the reference's; its
    /// random draws and its Levy step are the library's own specification (include/teeline_gpu.h).  (Written against the header; not
    /// compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn cuckoo_search(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, n_nearest: u32, mutation_probability: f32,
                         seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let opts = CsOpts { epochs, n_nearest, mutation_probability };
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: the slices hold n cities / n positions (check_inputs); the outputs are sized for n.
        let rc = unsafe {
            tl_cuckoo_search(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats)
        };
        self.check(rc).map(|_| t)
    }

    /// `flower_pollination::solve` (flower_pollination.rs:53-151), run 0 of `seed`, max(n_nearest, 25) flowers.  The algorithm is the
    /// reference's; its random draws are the library's own specification (include/teeline_gpu.h).  (Written against the header; not
    /// compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn flower_pollination(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, n_nearest: u32,
                              mutation_probability: f32, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let opts = FpaOpts { epochs, n_nearest, mutation_probability };
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: the slices hold n cities / n positions (check_inputs); the outputs are sized for n.
        let rc = unsafe {
            tl_flower_pollination(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats)
        };
        self.check(rc).map(|_| t)
    }

    /// `gravitational_search::solve` (gravitational_search.rs:23-145), run 0 of `seed`, max(n_nearest, 25) agents.  The algorithm is
    /// the reference's; its random draws, the order among equal masses and its exp are the library's own specification
    /// (include/teeline_gpu.h).  (Written against the header; not compiled here: no Rust toolchain on the build machine, see
    /// scripts/check_rust.sh.)
    pub fn gravitational_search(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, n_nearest: u32, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let opts = GsaOpts { epochs, n_nearest, span_epochs: 0 };
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: the slices hold n cities / n positions (check_inputs); the outputs are sized for n.
        let rc = unsafe {
            tl_gravitational_search(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats)
        };
        self.check(rc).map(|_| t)
    }

    /// `som::solve` (som.rs:12-186), run 0 of `seed`.  The algorithm is the reference's; the city drawn in an epoch, exp (with a cut
    /// at -8 before it) and the start ring's cos and sin are the library's own specification (include/teeline_gpu.h).  The map trains
    /// on the coordinates; `dm_packed` only prices the tour.  (Written against the header; not compiled here: no Rust toolchain on
    /// the build machine, see scripts/check_rust.sh.)
    pub fn kohonen_som(&self, xy: &[f32], dm_packed: Option<&[f32]>, epochs: u32, learning_rate: f64, radius_fraction: f64, neuron_multiplier: u32, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let opts = SomOpts { epochs, neuron_multiplier, learning_rate, radius_fraction, form: 0, reserved: 0, work_bytes: 0 };
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: the slices hold n cities (check_inputs); the outputs are sized for n.
        let rc = unsafe { tl_kohonen_som(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// Largest n of `kohonen_som` for a multiplier and a form (0 or 2: the cap of 65 536 neurons; 1: the ring in LDS).
    pub fn kohonen_som_max_n(&self, neuron_multiplier: u32, form: u32) -> u32 {
        // SAFETY: a live context.
        unsafe { tl_kohonen_som_max_n(self.raw, neuron_multiplier, form) }
    }

    /// `stochastic_hill::solve` (stochastic_hill.rs:7-97), chain 0 of `seed`: `epochs + 1` epochs, the best route.  The chain is the
    /// reference's (a candidate must beat the best cost; a plateau shuffles the current tour only); its random draws are the library's
    /// own specification (include/teeline_gpu.h).  `init_pos` None: city order.  (Written against the header; not compiled here: no
    /// Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn hill_climb(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: &HillOpts, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_hill_climb(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// Chain `chain` of `seed` with its events in order: an acceptance `[epoch, from, to, cost bits]`, a restart `[epoch, 0xFFFFFFFF, 0, 0]`,
    /// from which the reference's PathUpdate messages are replayed (the shuffles through `hill_draw`).
    pub fn hill_climb_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: &HillOpts, seed: u64, chain: u32)
                            -> Result<(Tour, Vec<[u32; 4]>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let cap: u32 = opts.epochs.saturating_add(1);  // at most one event an epoch
        let mut log = vec![[0u32; 4]; cap as usize];
        let mut len: u32 = 0;
        // SAFETY: as in two_opt; log holds cap entries of 4 words.
        let rc = unsafe {
            tl_hill_climb_trace_chain(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), opts, seed, chain, t.pos.as_mut_ptr(), &mut t.cost,
                                      &mut t.stats, log.as_mut_ptr() as *mut u32, cap, &mut len)
        };
        self.check(rc)?;
        log.truncate(len.min(cap) as usize);
        Ok((t, log))
    }

    /// Chains `first_chain .. first_chain + count` of `seed` at once, every chain from `init_pos` (or city order); the best routes and
    /// the index of the best one (lowest cost, then lowest chain).
    pub fn hill_climb_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, first_chain: u32, count: u32, opts: &HillOpts,
                                 seed: u64) -> Result<(Vec<Tour>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut pos = vec![0u32; n as usize * count as usize];
        let mut costs = vec![0f32; count as usize];
        let mut moves = vec![0u32; count as usize];
        let (mut best, mut st) = (0u32, Stats::default());
        // SAFETY: as in two_opt; the output arrays hold count x n, count and count entries.
        let rc = unsafe {
            tl_hill_climb_population(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), if init_pos.is_some() { 1 } else { 0 }, first_chain,
                                     count, opts, seed, pos.as_mut_ptr(), costs.as_mut_ptr(), moves.as_mut_ptr(), &mut best, &mut st)
        };
        self.check(rc)?;
        let tours = (0..count as usize)
            .map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: Stats { moves: moves[k] as u64, ..st } })
            .collect();
        Ok((tours, best))
    }

    /// `fourier::solve` (fourier.rs:10-312) for every option set of `jobs` at once, one workgroup each: the tours and the index of
    /// the best one (lowest cost, then lowest index).  The solver draws nothing, so there is no seed; job j equals the call with
    /// `jobs[j]` alone bit for bit.  The basis table, sqrt for hypot, the lowest index among samples at one f32 distance, (2 pi k)^2
    /// as t t and lambda as the running product are the library's own specification (include/teeline_gpu.h).  The curve descends on
    /// the coordinates; `dm_packed` only prices the tour.  (Written against the header; not compiled here: no Rust toolchain on the
    /// build machine, see scripts/check_rust.sh.)
    pub fn fourier_curve_batch(&self, xy: &[f32], dm_packed: Option<&[f32]>, jobs: &[FourierOpts]) -> Result<(Vec<Tour>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let count = jobs.len();
        let mut pos = vec![0u32; (n as usize).max(1) * count];
        let mut costs = vec![0f32; count];
        let (mut best, mut st) = (0u32, Stats::default());
        // SAFETY: the slices hold n cities (check_inputs); the outputs hold count x n and count entries; the optional outputs are null.
        let rc = unsafe {
            tl_fourier_curve_batch(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), jobs.as_ptr(), count as u32, pos.as_mut_ptr(), costs.as_mut_ptr(),
                                   ptr::null_mut(), 0, &mut best, &mut st, ptr::null_mut(), 0, ptr::null_mut())
        };
        self.check(rc)?;
        let tours = (0..count).map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: st }).collect();
        Ok((tours, best))
    }

    /// One job of `fourier_curve_batch`.
    pub fn fourier_curve(&self, xy: &[f32], dm_packed: Option<&[f32]>, opts: &FourierOpts) -> Result<Tour, Error> {
        self.fourier_curve_batch(xy, dm_packed, std::slice::from_ref(opts)).map(|(mut t, _)| t.remove(0))
    }

    /// The device workspace a `fourier_curve_batch` of these jobs takes (0 where it would be refused, or n < 2).
    pub fn fourier_curve_work_bytes(n: u32, jobs: &[FourierOpts]) -> u64 {
        // SAFETY: a host-only query over the slice.
        unsafe { tl_fourier_curve_work_bytes(n, jobs.as_ptr(), jobs.len() as u32, 0) }
    }

    /// The Held-Karp lower bound (not a solver and not the reference's) for every option set of `jobs` at once, one
    /// workgroup each: every job's outcome and the index of the first job with the largest bound.  The bound holds for every tour
    /// under the same f32 distances; job j equals the call with `jobs[j]` alone bit for bit.  (Written against the header; not
    /// compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn one_tree_bound_batch(&self, xy: &[f32], dm_packed: Option<&[f32]>, jobs: &[OneTreeOpts]) -> Result<(Vec<OneTreeBound>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let (count, m) = (jobs.len(), (n as usize).max(1));
        let mut res = vec![OneTreeResult::default(); count];
        let mut pi = vec![0f64; m * count];
        let mut tour = vec![0u32; m * count];
        let (mut best, mut st) = (0u32, Stats::default());
        // SAFETY: the slices hold n cities (check_inputs); the outputs hold count records and count x n entries; parents and log are null.
        let rc = unsafe {
            tl_one_tree_bound_batch(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, jobs.as_ptr(), count as u32, res.as_mut_ptr(), pi.as_mut_ptr(),
                                    ptr::null_mut(), tour.as_mut_ptr(), ptr::null_mut(), 0, &mut best, &mut st)
        };
        self.check(rc)?;
        let out = (0..count)
            .map(|k| OneTreeBound {
                result: res[k],
                pi: pi[k * n as usize..(k + 1) * n as usize].to_vec(),
                tour: if res[k].is_tour != 0 { Some(tour[k * n as usize..(k + 1) * n as usize].to_vec()) } else { None },
            })
            .collect();
        Ok((out, best))
    }

    /// One job of `one_tree_bound_batch`.
    pub fn one_tree_bound(&self, xy: &[f32], dm_packed: Option<&[f32]>, opts: &OneTreeOpts) -> Result<OneTreeBound, Error> {
        self.one_tree_bound_batch(xy, dm_packed, std::slice::from_ref(opts)).map(|(mut b, _)| b.remove(0))
    }

    /// The sequential restatement on the CPU (no context, no device), the same contract: the library's return code on refusal.
    pub fn one_tree_bound_host(xy: &[f32], dm_packed: Option<&[f32]>, opts: &OneTreeOpts) -> Result<OneTreeBound, i32> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let mut res = OneTreeResult::default();
        let mut pi = vec![0f64; (n as usize).max(1)];
        let mut tour = vec![0u32; (n as usize).max(1)];
        // SAFETY: the slices hold n cities; the outputs hold one record and n entries; parents and log are null.
        let rc = unsafe {
            tl_one_tree_bound_host(xy.as_ptr(), opt_ptr(dm_packed), n, opts, &mut res, pi.as_mut_ptr(), ptr::null_mut(), tour.as_mut_ptr(), ptr::null_mut(), 0)
        };
        if rc != 0 {
            return Err(rc);
        }
        pi.truncate(n as usize);
        tour.truncate(n as usize);
        Ok(OneTreeBound { result: res, pi, tour: if res.is_tour != 0 { Some(tour) } else { None } })
    }

    /// Alpha-nearness candidate lists (this project's own specification) under the penalties `pi` (None: zero),
    /// usually a `OneTreeBound`'s: n rows of min(k, n - 1) POSITIONS in (alpha, w, position) order, and their alphas.  (Written
    /// against the header; not compiled here: no Rust toolchain on the build machine, see scripts/check_rust.sh.)
    pub fn alpha_candidates(&self, xy: &[f32], dm_packed: Option<&[f32]>, pi: Option<&[f64]>, root: u32, k: u32) -> Result<(Vec<u32>, Vec<f64>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        assert!(pi.map_or(true, |p| p.len() == n as usize), "alpha_candidates: pi must hold n penalties");
        let kk = (k.min(n.saturating_sub(1)).min(64)) as usize;
        let mut rows = vec![0u32; (n as usize * kk).max(1)];
        let mut alpha = vec![0f64; (n as usize * kk).max(1)];
        let mut st = Stats::default();
        // SAFETY: the slices hold n cities and n penalties; the outputs hold n x min(k, n - 1) entries; the tree's outputs are null.
        let rc = unsafe {
            tl_alpha_candidates(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, pi.map_or(ptr::null(), |p| p.as_ptr()), root, k, 0, rows.as_mut_ptr(),
                                alpha.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), &mut st)
        };
        self.check(rc)?;
        rows.truncate(n as usize * kk);
        alpha.truncate(n as usize * kk);
        Ok((rows, alpha))
    }

    /// The sequential restatement on the CPU (no context, no device), the same contract: the library's return code on refusal.
    pub fn alpha_candidates_host(xy: &[f32], dm_packed: Option<&[f32]>, pi: Option<&[f64]>, root: u32, k: u32) -> Result<(Vec<u32>, Vec<f64>), i32> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        assert!(pi.map_or(true, |p| p.len() == n as usize), "alpha_candidates_host: pi must hold n penalties");
        let kk = (k.min(n.saturating_sub(1)).min(64)) as usize;
        let mut rows = vec![0u32; (n as usize * kk).max(1)];
        let mut alpha = vec![0f64; (n as usize * kk).max(1)];
        // SAFETY: as alpha_candidates.
        let rc = unsafe {
            tl_alpha_candidates_host(xy.as_ptr(), opt_ptr(dm_packed), n, pi.map_or(ptr::null(), |p| p.as_ptr()), root, k, rows.as_mut_ptr(), alpha.as_mut_ptr(),
                                     ptr::null_mut(), ptr::null_mut())
        };
        if rc != 0 {
            return Err(rc);
        }
        rows.truncate(n as usize * kk);
        alpha.truncate(n as usize * kk);
        Ok((rows, alpha))
    }

    /// The largest n of `alpha_candidates` on `lds_bytes` of LDS.
    pub fn alpha_candidates_max_n(lds_bytes: i32) -> u32 {
        // SAFETY: a host-only query.
        unsafe { tl_alpha_candidates_max_n(lds_bytes) }
    }

    /// (threads of a source city's workgroup, LDS bytes of its row) for n cities and lists of width k; None where the pair is refused.
    pub fn alpha_candidates_plan(n: u32, k: u32, lds_bytes: i32) -> Option<(i32, u32)> {
        let (mut t, mut used) = (0 as c_int, 0u32);
        // SAFETY: a host-only query with two live outputs.
        let rc = unsafe { tl_alpha_candidates_plan(n, k, lds_bytes, &mut t, &mut used) };
        if rc == 0 { Some((t, used)) } else { None }
    }

    /// tl_lk_candidates: every later Lin-Kernighan call of this context searches `rows` (n x k POSITIONS, e.g. `alpha_candidates`')
    /// instead of the kd-tree's lists; None clears them.  Alpha chooses the set, distance orders it: the library puts every row into
    /// ascending Euclidean distance, stably, before a search reads it.
    pub fn lk_candidates(&self, rows: Option<(&[u32], u32, u32)>) -> Result<(), Error> {
        let rc = match rows {
            None => unsafe { tl_lk_candidates(self.raw, ptr::null(), 0, 0) }, // SAFETY: NULL clears
            Some((r, n, k)) => {
                assert!(r.len() == n as usize * k as usize, "lk_candidates: rows must hold n x k positions");
                // SAFETY: the slice holds n x k entries; the library copies them.
                unsafe { tl_lk_candidates(self.raw, r.as_ptr(), n, k) }
            }
        };
        self.check(rc)
    }

    /// The largest n whose state fits `lds_bytes` of LDS, and (threads, iterations of a launch) for n, None where n is refused.
    pub fn one_tree_bound_max_n(lds_bytes: i32) -> u32 {
        // SAFETY: a host-only query.
        unsafe { tl_one_tree_bound_max_n(lds_bytes) }
    }
    pub fn one_tree_bound_plan(n: u32, lds_bytes: i32) -> Option<(i32, u32)> {
        let (mut t, mut span) = (0 as c_int, 0u32);
        // SAFETY: a host-only query with two live outputs.
        let rc = unsafe { tl_one_tree_bound_plan(n, lds_bytes, &mut t, &mut span) };
        if rc == 0 { Some((t, span)) } else { None }
    }
    /// The device workspace a batch of `jobs` jobs takes (0 for n <= 2).
    pub fn one_tree_bound_work_bytes(n: u32, jobs: u32) -> u64 {
        // SAFETY: a host-only query.
        unsafe { tl_one_tree_bound_work_bytes(n, jobs, 0) }
    }

    /// Largest n of `hill_climb` (the current tour lives in one CU's LDS, 12 bytes per city).
    pub fn hill_climb_lds_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_hill_climb_lds_max_n(self.raw) }
    }

    /// Largest n of `gravitational_search` (a workgroup keeps 8 n bytes in LDS).
    pub fn gravitational_search_max_n(&self) -> u32 {
        // SAFETY: a live context.
        unsafe { tl_gravitational_search_max_n(self.raw) }
    }

    /// Largest n of `flower_pollination` (a workgroup keeps 10 n bytes in LDS).
    pub fn flower_pollination_max_n(&self) -> u32 {
        // SAFETY: a live context.
        unsafe { tl_flower_pollination_max_n(self.raw) }
    }

    /// Largest n of `cuckoo_search` (a workgroup keeps 10 n bytes in LDS).
    pub fn cuckoo_search_max_n(&self) -> u32 {
        // SAFETY: a live context.
        unsafe { tl_cuckoo_search_max_n(self.raw) }
    }

    /// Largest n of `particle_swarm` (a workgroup keeps 14 n + 4 v_max bytes in LDS).
    pub fn particle_swarm_max_n(&self) -> u32 {
        // SAFETY: a live context.
        unsafe { tl_particle_swarm_max_n(self.raw) }
    }

    /// Largest n of `ant_colony` (a construct workgroup keeps 12 bytes per city in LDS beside its tiles).
    pub fn ant_colony_max_n(&self) -> u32 {
        // SAFETY: a live context.
        unsafe { tl_ant_colony_max_n(self.raw) }
    }

    /// Run `run` of `seed` with every generation `[best index, fitness bits, cost bits, population length]` and its best route, from which
    /// the reference's PathUpdate messages (one per generation, then one more) are replayed.
    pub fn genetic_algorithm_trace(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, epochs: u32, mutation_probability: f32,
                                   n_elite: u32, seed: u64, run: u32) -> Result<(Tour, Vec<[u32; 4]>, Vec<u32>), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut log = vec![[0u32; 4]; epochs.max(1) as usize];
        let mut routes = vec![0u32; epochs.max(1) as usize * n as usize];
        let mut len: u32 = 0;
        // SAFETY: as in two_opt; log holds `epochs` entries of 4 words, routes `epochs` x n.
        let rc = unsafe {
            tl_genetic_algorithm_trace_run(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), epochs, mutation_probability, n_elite, seed, run,
                                           t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats, log.as_mut_ptr() as *mut u32, epochs, &mut len, routes.as_mut_ptr(),
                                           epochs)
        };
        self.check(rc)?;
        log.truncate(len.min(epochs) as usize);
        routes.truncate(len.min(epochs) as usize * n as usize);
        Ok((t, log, routes))
    }

    /// Runs `first_run .. first_run + count` of `seed` at once, every run with `init_pos` as its initial tour (or none); the best routes
    /// and the index of the best one (lowest cost, then lowest run).
    pub fn genetic_algorithm_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, first_run: u32, count: u32, epochs: u32,
                                        mutation_probability: f32, n_elite: u32, seed: u64) -> Result<(Vec<Tour>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut pos = vec![0u32; n as usize * count as usize];
        let mut costs = vec![0f32; count as usize];
        let (mut best, mut st) = (0u32, Stats::default());
        // SAFETY: as in two_opt; the output arrays hold count x n and count entries.
        let rc = unsafe {
            tl_genetic_algorithm_population(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), first_run, count, epochs, mutation_probability,
                                            n_elite, seed, pos.as_mut_ptr(), costs.as_mut_ptr(), &mut best, &mut st)
        };
        self.check(rc)?;
        let tours = (0..count as usize).map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: st }).collect();
        Ok((tours, best))
    }

    /// Largest n of `genetic_algorithm` (a breeding workgroup keeps 14 bytes per city in LDS).
    pub fn genetic_algorithm_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_genetic_algorithm_max_n(self.raw) }
    }

    /// `or_opt::solve` (or_opt.rs:18-74).
    pub fn or_opt(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_or_opt(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// Largest n of the LDS-resident coordinate form of `or_opt_population` (the matrix form takes twice that).
    pub fn or_opt_lds_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_or_opt_lds_max_n(self.raw) }
    }

    /// Or-opt over a population: `init_pos` holds `count` tours of n positions back to back, each refined by its own
    /// `or_opt::solve` descent, all concurrently (`tl_or_opt_population`).  Tour k of the result is what `or_opt` returns for
    /// it alone; its `stats` are the call's (sums over the population) with `moves` replaced by that tour's own.
    pub fn or_opt_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: &[u32]) -> Result<Vec<Tour>, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        if n == 0 {
            return Ok(Vec::new());
        }
        assert!(init_pos.len() % n as usize == 0, "init_pos holds whole tours of n positions");
        let count = init_pos.len() / n as usize;
        let mut pos = vec![0u32; init_pos.len()];
        let mut costs = vec![0f32; count];
        let mut moves = vec![0u32; count];
        let mut stats = Stats::default();
        // SAFETY: as in two_opt; every output buffer holds count (x n) entries.
        let rc = unsafe {
            tl_or_opt_population(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), init_pos.as_ptr(), count as u32, pos.as_mut_ptr(),
                                 costs.as_mut_ptr(), moves.as_mut_ptr(), &mut stats)
        };
        self.check(rc)?;
        Ok((0..count)
            .map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: Stats { moves: moves[k] as u64, ..stats } })
            .collect())
    }

    /// Largest n whose best-sweep descent fits one CU's LDS (`tl_two_opt_best_lds_max_n`): beyond it a batch runs descent after descent.
    pub fn two_opt_best_lds_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_two_opt_best_lds_max_n(self.raw) }
    }

    /// Best-sweep batches of this context loop over `two_opt`'s chip-wide descent at every n (`tl_two_opt_best_force_scan`): the
    /// cross-check of the two forms.
    pub fn two_opt_best_force_scan(&self, on: bool) -> Result<(), Error> {
        // SAFETY: a setting of a live context.
        self.check(unsafe { tl_two_opt_best_force_scan(self.raw, on as c_int) })
    }

    /// Best-sweep 2-opt over a population (coordinates only): `init_pos` holds `count` tours of n positions back to back, each refined
    /// by its own `TL_MODE_BEST_SWEEP` descent, all concurrently (`tl_two_opt_best_population`).  Tour k of the result is what `two_opt`
    /// in that mode returns for it alone; its `stats` are the call's (sums over the population) with `moves` replaced by that tour's own.
    pub fn two_opt_best_population(&self, xy: &[f32], init_pos: &[u32]) -> Result<Vec<Tour>, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, None, None);
        if n == 0 {
            return Ok(Vec::new());
        }
        assert!(init_pos.len() % n as usize == 0, "init_pos holds whole tours of n positions");
        let count = init_pos.len() / n as usize;
        let mut pos = vec![0u32; init_pos.len()];
        let mut costs = vec![0f32; count];
        let mut moves = vec![0u32; count];
        let mut stats = Stats::default();
        // SAFETY: as in two_opt; every output buffer holds count (x n) entries.
        let rc = unsafe {
            tl_two_opt_best_population(self.raw, xy.as_ptr(), n, init_pos.as_ptr(), count as u32, pos.as_mut_ptr(), costs.as_mut_ptr(),
                                       moves.as_mut_ptr(), &mut stats)
        };
        self.check(rc)?;
        Ok((0..count)
            .map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: Stats { moves: moves[k] as u64, ..stats } })
            .collect())
    }

    /// The seed of run `run` of a Lin-Kernighan population seeded `seed` (`tl_lk_run_seed`): run 0 the seed itself, run r >= 1 output
    /// 2^63 + r of the seed's splitmix64 stream.
    pub fn lk_run_seed(seed: u64, run: u32) -> u64 {
        // SAFETY: a pure function of its arguments.
        unsafe { tl_lk_run_seed(seed, run) }
    }

    /// Largest n whose seeded LK runs take one workgroup each with these options (`tl_lk_population_max_n`).
    pub fn lk_population_max_n(&self, opts: LkOpts) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_lk_population_max_n(self.raw, &opts) }
    }

    /// Which form this context's later `lin_kernighan_population` calls take (-1: the plan's choice, 0: the loop over `tl_lk`, 1: one
    /// workgroup per run wherever it fits) and the scans a run advances per launch of form 1 (0: the default): the cross-check knob.
    pub fn lk_population_setting(&self, force_form: i32, slice_scans: u32) -> Result<(), Error> {
        // SAFETY: a setting of a live context.
        self.check(unsafe { tl_lk_population_setting(self.raw, force_form as c_int, slice_scans) })
    }

    /// Seeded runs `first_run .. first_run + count` of `lin_kernighan` at once (`tl_lk_population`): run r is the search of seed
    /// `lk_run_seed(seed, r)`.  `init_pos`: None (the NN seed), one tour of n positions for all runs, or `count` of them back to back.
    /// One `Tour` per run, its `stats` the call's with the run's own sweeps / candidates / moves / reversed; and the index of the
    /// cheapest (equal costs: the lowest run).
    pub fn lin_kernighan_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, first_run: u32, count: u32,
                                    opts: LkOpts, seed: u64) -> Result<(Vec<Tour>, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        if n == 0 || count == 0 {
            return Ok((Vec::new(), 0));
        }
        let init_count = init_pos.map_or(0, |p| {
            assert!(p.len() % n as usize == 0, "init_pos holds whole tours of n positions");
            (p.len() / n as usize) as u32
        });
        let mut pos = vec![0u32; count as usize * n as usize];
        let mut costs = vec![0f32; count as usize];
        let mut counters = vec![0u64; count as usize * 4];
        let mut best = 0u32;
        let mut stats = Stats::default();
        // SAFETY: as in lin_kernighan; every output buffer holds count (x n, x 4) entries.
        let rc = unsafe {
            tl_lk_population(self.raw, xy.as_ptr(), n, dm_packed.map_or(std::ptr::null(), |d| d.as_ptr()),
                             init_pos.map_or(std::ptr::null(), |p| p.as_ptr()), init_count, first_run, count, &opts, seed, pos.as_mut_ptr(),
                             costs.as_mut_ptr(), counters.as_mut_ptr(), &mut best, &mut stats)
        };
        self.check(rc)?;
        let tours = (0..count as usize)
            .map(|k| Tour {
                pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(),
                cost: costs[k],
                stats: Stats { sweeps: counters[4 * k], candidates: counters[4 * k + 1], moves: counters[4 * k + 2], reversed: counters[4 * k + 3], ..stats },
            })
            .collect();
        Ok((tours, best))
    }

    /// Largest n of the per-workgroup form of `three_opt_population` (either input form).
    pub fn three_opt_pop_max_n(&self) -> u32 {
        // SAFETY: a plain query of a live context.
        unsafe { tl_three_opt_pop_max_n(self.raw) }
    }

    /// Cap on the workspace of `three_opt_population`'s per-tour matrices (0: the default, 8 GiB).
    pub fn three_opt_population_work_limit(&self, bytes: u64) -> Result<(), Error> {
        // SAFETY: a plain setter of a live context.
        let rc = unsafe { tl_three_opt_population_work_limit(self.raw, bytes) };
        self.check(rc)
    }

    /// 3-opt over a population: `init_pos` holds `count` tours of n positions back to back, each refined by its own
    /// `three_opt::solve` descent (`tl_three_opt_population`).  Tour k of the result is what `three_opt` returns for it alone;
    /// its `stats` are the call's (sums over the population) with `moves` replaced by that tour's own.
    pub fn three_opt_population(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: &[u32]) -> Result<Vec<Tour>, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        if n == 0 {
            return Ok(Vec::new());
        }
        assert!(init_pos.len() % n as usize == 0, "init_pos holds whole tours of n positions");
        let count = init_pos.len() / n as usize;
        let mut pos = vec![0u32; init_pos.len()];
        let mut costs = vec![0f32; count];
        let mut moves = vec![0u32; count];
        let mut stats = Stats::default();
        // SAFETY: as in two_opt; every output buffer holds count (x n) entries.
        let rc = unsafe {
            tl_three_opt_population(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), init_pos.as_ptr(), count as u32, pos.as_mut_ptr(),
                                    costs.as_mut_ptr(), moves.as_mut_ptr(), &mut stats)
        };
        self.check(rc)?;
        Ok((0..count)
            .map(|k| Tour { pos: pos[k * n as usize..(k + 1) * n as usize].to_vec(), cost: costs[k], stats: Stats { moves: moves[k] as u64, ..stats } })
            .collect())
    }

    /// `lin_kernighan::solve` (lin_kernighan.rs:35-100).  The search is Euclidean over `xy` (the reference rebuilds its own
    /// matrix, :41); `dm_packed` (problem.distances of a GEO / EXPLICIT problem) feeds the NN seed (:47-55) and the total (:99).
    /// `seed` drives the double-bridge kicks (the reference draws them from an unseeded thread RNG, :73).
    pub fn lin_kernighan(&self, xy: &[f32], dm_packed: Option<&[f32]>, init_pos: Option<&[u32]>, opts: LkOpts, seed: u64) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, init_pos);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt; opts is a plain #[repr(C)] value.
        let rc = unsafe { tl_lk(self.raw, xy.as_ptr(), n, opt_ptr(dm_packed), opt_ptr(init_pos), &opts, seed, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// `nearest_neighbor::solve` (nearest_neighbor.rs:8-76).
    pub fn nearest_neighbor(&self, xy: &[f32], dm_packed: Option<&[f32]>, n_nearest: u32) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_nearest_neighbor(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, n_nearest, t.pos.as_mut_ptr(), &mut t.cost) };
        self.check(rc).map(|_| t)
    }

    /// `greedy_edge::solve` (greedy_edge.rs:21-65): every edge in ascending length order (ties: (i, j) ascending), n <= 65 535.
    pub fn greedy_edge(&self, xy: &[f32], dm_packed: Option<&[f32]>) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_greedy_edge(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// `christofides::solve` (christofides.rs:12-68): Prim's tree from position 0 (first minimum in position order), a greedy
    /// matching of its odd vertices (equal lengths in (i, j) order, a NaN length after +inf), Euler circuit and shortcut; n < 4 is
    /// the identity, n <= 65 535.  A tree that cannot span (a position every distance to which is NaN or >= f32::MAX) is
    /// `Error` with `TL_ERR_UNSUPPORTED`.
    pub fn christofides(&self, xy: &[f32], dm_packed: Option<&[f32]>) -> Result<Tour, Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        // SAFETY: as in two_opt.
        let rc = unsafe { tl_christofides(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, t.pos.as_mut_ptr(), &mut t.cost, &mut t.stats) };
        self.check(rc).map(|_| t)
    }

    /// `bellman_karp::solve` (bellman_karp.rs:24-87), the exact solver, n <= `BHK_MAX_N`: returns the route as the reference's
    /// tolerance walk leaves it, the DP's optimum and whether the route is a permutation — it need not be (`Tour::cost` is
    /// tour_length of the route as given either way).  A context created with `FLAG_BHK_EXACT_WALK` reads the route back by exact
    /// equality instead: always a tour while a finite one exists.
    pub fn bellman_karp(&self, xy: &[f32], dm_packed: Option<&[f32]>) -> Result<(Tour, f32, bool), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let (mut optimal, mut is_tour) = (0.0f32, 0u32);
        // SAFETY: as in two_opt; out_optimal and out_is_tour point at live values.
        let rc = unsafe {
            tl_bellman_karp(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, t.pos.as_mut_ptr(), &mut t.cost, &mut optimal, &mut is_tour,
                            &mut t.stats)
        };
        self.check(rc).map(|_| (t, optimal, is_tour != 0))
    }

    /// `savings::solve` (savings.rs:34-82): every edge in descending order of its saving against the hub (ties: (i, j) ascending;
    /// a NaN saving ranks below every number), n <= 65 535.  `hub`: a position, or `None` for the one nearest the centroid of `xy`
    /// (`savings_hub`).  Returns the tour and the hub used.
    pub fn savings(&self, xy: &[f32], dm_packed: Option<&[f32]>, hub: Option<u32>) -> Result<(Tour, u32), Error> {
        let n = Self::n_of(xy);
        Self::check_inputs(n, dm_packed, None);
        let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
        let mut used = 0u32;
        // SAFETY: as in two_opt; out_hub points at a live u32.
        let rc = unsafe {
            tl_savings(self.raw, xy.as_ptr(), opt_ptr(dm_packed), n, hub.unwrap_or(SAVINGS_HUB_AUTO), t.pos.as_mut_ptr(), &mut t.cost,
                       &mut used, &mut t.stats)
        };
        self.check(rc).map(|_| (t, used))
    }
}

/// `TL_SAVINGS_HUB_AUTO` (include/teeline_gpu.h)
pub const SAVINGS_HUB_AUTO: u32 = 0xFFFF_FFFF;
/// `tl_create` flag: `bellman_karp` reads its route back by exact f32 equality instead of the reference's tolerance walk.
pub const FLAG_BHK_EXACT_WALK: u32 = 1 << 25;
/// `tl_create` flag: `or_opt_population` runs its tours one after the other through `or_opt`'s chip-wide descent at every n.
pub const FLAG_OR_OPT_FORCE_SCAN: u32 = 1 << 26;
/// The rule `three_opt_population` follows (`tl_three_opt_population_plan`; pure, no device): `(form, threads, batch)` for `count`
/// tours of n cities on a device of `cus` CUs with `lds_bytes` of LDS and `work_bytes` of workspace; `None` for a device that is none.
pub fn three_opt_population_plan(n: u32, count: u32, cus: i32, lds_bytes: i32, work_bytes: u64, flags: u32) -> Option<(i32, i32, u32)> {
    let (mut form, mut threads, mut batch) = (0 as c_int, 0 as c_int, 0u32);
    // SAFETY: the three outputs are live locals.
    let rc = unsafe { tl_three_opt_population_plan(n, count, cus, lds_bytes, work_bytes, flags, &mut form, &mut threads, &mut batch) };
    if rc == 0 { Some((form, threads, batch)) } else { None }
}

/// The rule the best-sweep batch entries follow (`tl_two_opt_best_plan`; pure, no device): `(form, threads)` — form 0: one workgroup
/// of `threads` per descent, form 1: the loop over the chip-wide descent; `None` for a device that is none.
pub fn two_opt_best_plan(n: u32, count: u32, cus: i32, lds_bytes: i32, force_scan: bool) -> Option<(i32, i32)> {
    let (mut form, mut threads) = (0 as c_int, 0 as c_int);
    // SAFETY: the two outputs are live locals.
    let rc = unsafe { tl_two_opt_best_plan(n, count, cus, lds_bytes, force_scan as c_int, &mut form, &mut threads) };
    if rc == 0 { Some((form, threads)) } else { None }
}

/// `tl_create` flag: `three_opt_population` runs its tours one after the other through `three_opt`'s chip-wide descent.
pub const FLAG_3OPT_POP_FORCE_SCAN: u32 = 1 << 27;
/// `tl_create` flag: `three_opt_population` runs one workgroup per tour wherever a tour fits.
pub const FLAG_3OPT_POP_FORCE_WG: u32 = 1 << 28;
/// Largest n `bellman_karp` takes (a table of 2^(n-1) rows of 128 bytes).
pub const BHK_MAX_N: u32 = 26;

/// `hub_position` (savings.rs:94-117): the position nearest the centroid of `xy` (x0, y0, x1, y1, ...), in f32 throughout.  Host
/// code: needs no context and no GPU.
pub fn savings_hub(xy: &[f32]) -> u32 {
    let mut hub = 0u32;
    // SAFETY: xy holds 2 * n floats; out_hub points at a live u32.  The call cannot fail on non-null arguments.
    let _ = unsafe { tl_savings_hub(xy.as_ptr(), (xy.len() / 2) as u32, &mut hub) };
    hub
}

impl Drop for Context {
    fn drop(&mut self) {
        // SAFETY: raw came from tl_create and is destroyed once.
        unsafe { tl_destroy(self.raw) }
    }
}

/// Multi-start 2-opt over several GPUs of one node from one process (north-star config 4): restarts
/// `[first, first + count)` from seeded Fisher-Yates permutations, dealt in contiguous blocks over `ctxs` (one context
/// per device).  Returns the best tour, its restart id and every restart's cost.
pub fn two_opt_multistart(ctxs: &[Context], xy: &[f32], seed: u64, first: u32, count: u32) -> Result<(Tour, u32, Vec<f32>), Error> {
    assert!(!ctxs.is_empty());
    let n = Context::n_of(xy);
    let raws: Vec<*mut TlCtx> = ctxs.iter().map(|c| c.raw).collect();
    let mut t = Tour { pos: vec![0u32; n as usize], cost: 0.0, stats: Stats::default() };
    let mut best = 0u32;
    let mut costs = vec![0f32; count as usize];
    // SAFETY: buffers sized as the C ABI documents; the contexts outlive the call.
    let rc = unsafe {
        tl_two_opt_multistart_devices(raws.as_ptr(), raws.len() as c_int, xy.as_ptr(), n, seed, first, count, MODE_REF_ORDER,
                                      t.pos.as_mut_ptr(), &mut t.cost, &mut best, costs.as_mut_ptr(), &mut t.stats)
    };
    ctxs[0].check(rc).map(|_| (t, best, costs))
}

thread_local! {
    static CTX: RefCell<Option<Context>> = const { RefCell::new(None) };
}

/// Runs `f` with this thread's context (device `TEELINE_GPU_DEVICE`, default 0), creating it on first use.
pub fn with_context<R>(f: impl FnOnce(&Context) -> Result<R, Error>) -> Result<R, Error> {
    CTX.with(|cell| {
        let mut slot = cell.borrow_mut();
        if slot.is_none() {
            let dev = std::env::var("TEELINE_GPU_DEVICE").ok().and_then(|v| v.parse().ok()).unwrap_or(0);
            *slot = Some(Context::new(dev, 0)?);
        }
        f(slot.as_ref().expect("context was just created"))
    })
}

#[allow(dead_code)]
fn _assert_layout() {
    // the C structs are 48 and 16 bytes (include/teeline_gpu.h)
    const _: () = assert!(std::mem::size_of::<Stats>() == 48 && std::mem::size_of::<LkOpts>() == 16);
}
