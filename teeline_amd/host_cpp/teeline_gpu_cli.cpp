// teeline-gpu — CLI façade over the GPU path, mirroring teeline-cli (teeline-cli/src/main.rs) for the solvers this build
// accelerates: same sub-commands, same flags, byte-identical stdout.
//
//   teeline-gpu bound -i FILE [--upper U | --tour FILE] [--root R] [--iterations T] [--lambda L,L,..] [--patience P,P,..]
//               [--output-format text|json]: the Held-Karp lower bound, the lists a grid of jobs; prints the best
//               bound, its job, the upper bound used and the gap in percent, `proved=1` where the 1-tree is a tour
//   teeline-gpu candidates --alpha -k K -i FILE [--ascent-iterations I] [--root R]: the alpha-nearness lists, a line per city
//   solve lk / pipeline with an lk step --candidates alpha[:K] [--ascent-iterations I]: the ascent as `bound` runs it, the lists under its best
//   penalties (I = 0: zero penalties), and every lk step searches them (tl_lk_candidates); --stats names the lists' kind and width
//   solve / pipeline --lower-bound: the bound with the solved tour as upper; `bound` and `gap_pct` on stderr (text) or in the JSON object
//   teeline-gpu solve <solver|preset> [-i FILE] [--no-seed] [--output-format text|json] [--optimal-tour FILE]
//                                     [--distance-type euc_2d|geo] [--epochs E] [--platoo_epochs P] [--n_nearest K] [--max-depth D]
//   teeline-gpu pipeline --steps=nn,2opt,... [-i FILE] [same options]
//   teeline-gpu solvers [--short]
//     solver  : nn, gec, sav, chr, bhk, 2opt, 3opt, or_opt, lk, shuffle (and their long names), simulated_annealing (long name only: `sa` stays refused, mod.rs:559-590); presets (main.rs:354-369):
//               fast = nn,2opt; classic = nn,2opt,simulated_annealing; thorough = nn,3opt,simulated_annealing
//     annealing: --cooling-rate C --min-temperature LO --max-temperature HI (SAOptions, mod.rs:689-706; --epochs is the shared one),
//               --chains K (own flag: K chains of the seed at once, the best kept); `solve simulated_annealing` alone is pipeline(shuffle, simulated_annealing) (mod.rs:144-157)
//     tabu     : tabu_search (long name only: `tabu` stays refused) runs --epochs + 1 epochs of seeded draws (--seed); --tabu-chains K (own flag:
//               K chains of the seed at once, the best kept); `solve tabu_search` alone is pipeline(nn, tabu_search) (mod.rs:129-139)
//     genetic  : genetic_algorithm (long name only: `ga` stays refused) breeds --epochs generations of seeded draws (--seed) with
//               --mutation-probability P and --n-elite N (GAOptions, mod.rs:815-846); --ga-runs K (own flag: K runs of the seed at once,
//               the best kept); `solve genetic_algorithm` alone is pipeline(shuffle, genetic_algorithm) (mod.rs:144-157, 2152)
//     colony   : ant_colony (long name only: `aco` stays refused) runs --epochs epochs (default 150) of seeded draws (--seed) with --alpha A
//               --beta B --evaporation-rate R --num-ants N (AcoOptions, mod.rs:1082-1153); --runs K (K colonies of the seed at once, the
//               best kept); `solve ant_colony` alone is pipeline(shuffle, ant_colony) (mod.rs:2158)
//     swarm    : particle_swarm (long name only: `pso` stays refused) runs --epochs epochs (default 10000) of seeded draws (--seed) with
//               max(--n-nearest, 30) particles; --runs K (K swarms of the seed at once, the best kept); `solve particle_swarm` alone is
//               pipeline(shuffle, particle_swarm) (mod.rs:144-157)
//     cuckoos  : cuckoo_search (long name only: `cs` stays refused) runs --epochs epochs (default 10000) of seeded draws (--seed) with
//               max(--n-nearest, 25) nests and --mutation-probability P (CSOptions, mod.rs:913-925: pa = clamp(P, 0.01, 0.99)); --runs K
//               (K runs of the seed at once, the best kept); `solve cuckoo_search` alone is pipeline(shuffle, cuckoo_search) (mod.rs:2154)
//     flowers  : flower_pollination (long name only: `fpa` stays refused) runs --epochs epochs (default 10000) of seeded draws (--seed) with
//               max(--n-nearest, 25) flowers and --mutation-probability P (FPAOptions, mod.rs:998-1010: switch_prob = 0.8 where P < 0.01,
//               else P); --runs K (K runs of the seed at once, the best kept); `solve flower_pollination` alone is
//               pipeline(shuffle, flower_pollination) (mod.rs:2155)
//     gravity  : gravitational_search (long name only: `gsa` stays refused) runs --epochs epochs (default 10000) of seeded draws (--seed)
//               with max(--n-nearest, 25) agents; --runs K (K runs of the seed at once, the best kept); `solve gravitational_search`
//               alone is pipeline(shuffle, gravitational_search) (mod.rs:2157)
//     kohonen  : kohonen_som (long name only: `som` and `kohonen` stay refused) trains --epochs epochs (default 100000) of seeded draws
//               (--seed) with --learning_rate (0.8), --radius_fraction (0.1) and --neuron_multiplier (8): SOMOptions, mod.rs:1465-1499;
//               --runs K (K runs of the seed at once, the best kept); `solve kohonen_som` runs alone: the map is constructive and
//               ignores a start tour (it is in neither of mod.rs:129-157's lists)
//     hill    : hill_climb (the reference's `stochastic_hill` stays refused, `hill` unknown) runs --epochs + 1 epochs (default 10000)
//               of seeded draws (--seed) with --platoo_epochs (500): HeuristicOptions; --runs K (K chains of the seed at once, the best
//               kept); `solve hill_climb` alone is pipeline(shuffle, hill_climb) (mod.rs:141-157)
//     fourier : fourier_curve (the reference's `fourier` stays refused) descends a closed Fourier curve: --k-max (4), --m (200), --lambda
//               (0.05), --lambda-decay (0.5), --lr (0.05), --epochs (400): FourierOptions, mod.rs:1341-1384; --lambda and --lr take
//               comma lists whose product runs as one batch, the best kept; no seed (the solver draws nothing); `solve fourier_curve`
//               runs alone and ignores a start tour
//     exact   : branch_and_bound (the reference's `branch_bound` stays refused) is the depth-first branch and bound to 64 cities,
//               exact unless --n-nearest is given explicitly (a departure: the reference's default of 3 makes its default run a
//               heuristic); --max-nodes N and --time-limit-ms T are budgets, and a search they end says `proved=0` on stderr;
//               `solve branch_and_bound` alone is pipeline(nn, branch_and_bound) (mod.rs:127-135)
//     solve   : 2opt / 3opt / or_opt / lk auto-expand to pipeline(nn, solver) unless --no-seed (main.rs:387-397, mod.rs:129-139);
//               gec (greedy_edge), sav (savings) and chr (christofides) are constructions and run alone; so does bhk (bellman_karp),
//               the exact solver (n <= 26, mod.rs:2137) — as a later pipeline stage it ignores its seed
//     stdout  : print_solution "{:.5} {0|1}\n<id id ... >\n" (main.rs:645-652) or the JSON object of main.rs:700-712;
//               with --optimal-tour the comparison goes to stderr in text mode and into the JSON object in JSON mode
//   own flags (no counterpart in the reference): --seed S (LK kicks and the shuffle stage; the reference draws both from an
//   unseeded thread RNG), --best-sweep (TL_MODE_BEST_SWEEP), --device N, --stats,
//   `solve lk --runs K [--seed S]` with K >= 2 (and `pipeline --steps ...,lk --runs K`): K seeded runs of the last lk stage at once
//   (tl_lk_population: run r is the search of seed tl_lk_run_seed(S, r), all from the stage's warm start), the best printed; --stats then
//   also reports best_run, --output-format json gains "best_run" and "runs"; without --runs, or with K = 1, the output is what it was,
//   `solve 2opt --runs K [--seed S] [--best-sweep]` with K >= 2: K seeded restarts at once (tl_two_opt_multistart), the best printed,
//   --stats then also reports best_restart; without --runs, or with K = 1, the output is what it was,
//   --exact-walk (TL_FLAG_BHK_EXACT_WALK: bhk reads its route back by exact equality instead of the reference's tolerance walk, whose
//   result is now and then no tour — the stage then fails with "invalid tour", as in the reference),
//   --timing (one JSON line on stderr: milliseconds of main() by phase — read input, create context, every stage's wall and kernel
//   time, output — what bench.py's drop_in_end_to_end reads), --repeat K (run the stage list K times in this process, the last
//   run is printed: with --timing the first run is the cold one — code-object load, workspace allocation — the others steady),
//   --full-exit (leave through exit() with every static destructor — the HIP runtime's teardown, tens of milliseconds — instead of
//   flushing and _exit(); the default leaves quickly: the process holds nothing but GPU memory, which the driver reclaims)
#include "teeline_gpu.hpp"

#include <chrono>
#include <cstring>
#include <iostream>
#include <unistd.h>

using namespace teeline;
using namespace teeline::tsp;

namespace {

struct Args {
    std::string cmd, solver, file, steps, optimal_tour, distance_type, output_format = "text";
    bool no_seed = false, best = false, exact_walk = false, stats = false, short_list = false, progress_digest = false, timing = false, full_exit = false;
    int device = 0, repeat = 1;
    uint32_t runs = 1;  // --runs as given: `solve 2opt` reads it here
    pipeline::StageOptions opt;
    std::vector<double> fourier_lambdas, fourier_lrs;  // --lambda / --lr comma lists: their product is a fourier_curve batch
    // `bound` (the Held-Karp lower bound) and --lower-bound on solve / pipeline
    bool lower_bound = false;
    double upper = 0.0;                  // --upper U; 0: from --tour FILE, else from nn -> 2opt
    std::string tour_file;
    one_tree_bound::BoundOptions bound_opt;
    std::vector<double> bound_patiences;  // --patience P,P,..: with --lambda L,L,.. a grid of jobs, lambda the outer index
    // alpha-nearness candidate lists: `solve lk --candidates alpha[:K]` / pipelines with an lk step, and `candidates --alpha -k K`
    bool cand_alpha = false;
    uint32_t cand_k = 5;
    size_t ascent_iterations = 1000;     // --ascent-iterations I; 0: zero penalties, no ascent
};

[[noreturn]] void usage_exit(const char *why)
{
    if (why) std::fprintf(stderr, "error: %s\n", why);
    std::fprintf(stderr,
                 "usage: teeline-gpu solve <nn|gec|sav|chr|bhk|2opt|3opt|or_opt|lk|simulated_annealing|tabu_search|genetic_algorithm|ant_colony|particle_swarm|cuckoo_search|flower_pollination|gravitational_search|kohonen_som|hill_climb|fourier_curve|branch_and_bound|shuffle|fast|classic|thorough> [-i FILE] [--no-seed] [--output-format text|json]\n"
                 "                         [--optimal-tour FILE] [--distance-type euc_2d|geo] [--epochs E] [--platoo_epochs P]\n"
                 "                         [--n_nearest K] [--max-depth D] [--seed S] [--best-sweep] [--device N] [--stats]\n"
                 "                         [--progress-digest] [--exact-walk]\n"
                 "                         [--cooling-rate C] [--min-temperature LO] [--max-temperature HI] [--chains K] [--tabu-chains K]\n"
                 "                         [--mutation-probability P] [--n-elite N] [--ga-runs K]\n"
                 "                         [--alpha A] [--beta B] [--evaporation-rate R] [--num-ants N] [--runs K]\n"
                 "                         (solve 2opt --runs K: K seeded restarts of --seed at once, the best printed)\n"
                 "                         (solve lk --runs K: K seeded runs of --seed at once from the same start, the best printed)\n"
                 "                         [--max-nodes N] [--time-limit-ms T]\n"
                 "       teeline-gpu pipeline --steps=nn,2opt,... | --steps=greedy_edge,2opt,... | --steps=savings,2opt,... | --steps=christofides,lk,... [-i FILE] [options as above]\n"
                 "       teeline-gpu bound -i FILE [--upper U | --tour FILE] [--root R] [--iterations T] [--lambda L,L,...] [--patience P,P,...] [--output-format text|json]\n"
                 "       teeline-gpu candidates --alpha -k K -i FILE [--ascent-iterations I] [--root R]   (a line per city: its id, then its K candidates' ids)\n"
                 "       solve lk and pipelines with an lk step take --candidates alpha[:K] [--ascent-iterations I]: the ascent as `bound` runs it (upper from nn,2opt;\n"
                 "       I = 0: zero penalties), alpha-nearness lists of width K (5) under its best penalties, and every lk step searches them (--stats: lists=alpha:K)\n"
                 "       solve and pipeline also take --lower-bound: the Held-Karp bound with the solved tour as upper, `bound` and `gap_pct` on stderr or in the JSON object\n"
                 "       teeline-gpu solvers [--short]\n");
    std::exit(2);  // clap's usage-error exit code
}

size_t parse_usize(const std::string &flag, const std::string &v)
{
    char *end = nullptr;
    const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
    if (v.empty() || !end || *end != '\0' || v[0] == '-') {
        std::fprintf(stderr, "error: %s must be a positive integer\n", flag.c_str());
        std::exit(1);
    }
    return (size_t)x;
}

void exit_if_invalid(const std::string &why)  // an options struct's validate(): the message, or empty
{
    if (why.empty()) return;
    std::fprintf(stderr, "error: %s\n", why.c_str());
    std::exit(1);
}

Args parse(int argc, char **argv)
{
    Args a;
    if (argc < 2) usage_exit(nullptr);
    a.cmd = argv[1];
    // LKOptions::from_cli: heuristic = HeuristicOptions::from_cli, i.e. the CLI defaults 10000 / 500 / 3, not
    // LKOptions::default() (mod.rs:1321-1325)
    a.opt.lk.heuristic = a.opt.heuristic;
    int i = 2;
    if (a.cmd == "solve") {
        if (argc < 3 || argv[2][0] == '-') usage_exit("solve: SOLVER_NAME is required");
        a.solver = argv[2];
        i = 3;
    } else if (a.cmd != "pipeline" && a.cmd != "solvers" && a.cmd != "bound" && a.cmd != "candidates") {
        usage_exit("unknown sub-command");
    }
    for (; i < argc; ++i) {
        std::string s = argv[i], inline_val;
        bool has_inline = false;
        const size_t eq = s.find('=');
        if (s.rfind("--", 0) == 0 && eq != std::string::npos) {
            inline_val = s.substr(eq + 1);
            s = s.substr(0, eq);
            has_inline = true;
        }
        auto val = [&]() -> std::string {
            if (has_inline) return inline_val;
            if (i + 1 >= argc) usage_exit((s + ": a value is required").c_str());
            return argv[++i];
        };
        if (s == "-i" || s == "--input") a.file = val();
        else if (s == "--no-seed") a.no_seed = true;
        else if (s == "--steps") a.steps = val();
        else if (s == "--output-format") a.output_format = val();
        else if (s == "--optimal-tour") a.optimal_tour = val();
        else if (s == "--distance-type") a.distance_type = val();
        else if (s == "--epochs") a.opt.heuristic.epochs = a.opt.lk.heuristic.epochs = a.opt.sa.heuristic.epochs = a.opt.ga.heuristic.epochs = a.opt.aco.heuristic.epochs = a.opt.som.epochs = a.opt.fourier.epochs = parse_usize(s, val());
        else if (s == "--cooling-rate" || s == "--cooling_rate") a.opt.sa.cooling_rate = std::stof(val());
        else if (s == "--min-temperature" || s == "--min_temperature") a.opt.sa.min_temperature = std::stof(val());
        else if (s == "--max-temperature" || s == "--max_temperature") a.opt.sa.max_temperature = std::stof(val());
        else if (s == "--tabu-chains" || s == "--tabu_chains") a.opt.tabu_chains = (uint32_t)std::max<size_t>(1, parse_usize(s, val()));
        else if (s == "--mutation-probability" || s == "--mutation_probability") a.opt.ga.mutation_probability = a.opt.cs_mutation_probability = a.opt.fpa_mutation_probability = std::stof(val());
        else if (s == "--n-elite" || s == "--n_elite") a.opt.ga.n_elite = parse_usize(s, val());
        else if (s == "--ga-runs" || s == "--ga_runs") a.opt.ga_runs = (uint32_t)std::max<size_t>(1, parse_usize(s, val()));
        else if (s == "--alpha" && a.cmd != "candidates") a.opt.aco.alpha = std::stof(val());
        else if (s == "--beta") a.opt.aco.beta = std::stof(val());
        else if (s == "--evaporation-rate" || s == "--evaporation_rate") a.opt.aco.evaporation_rate = std::stof(val());
        else if (s == "--num-ants" || s == "--num_ants") a.opt.aco.num_ants = parse_usize(s, val());
        else if (s == "--runs") a.runs = a.opt.aco_runs = a.opt.pso_runs = a.opt.cs_runs = a.opt.fpa_runs = a.opt.gsa_runs = a.opt.som_runs = a.opt.hill_chains = (uint32_t)std::max<size_t>(1, parse_usize(s, val()));
        else if (s == "--chains") a.opt.sa_chains = (uint32_t)std::max<size_t>(1, parse_usize(s, val()));
        else if (s == "--platoo_epochs" || s == "--platoo-epochs") a.opt.heuristic.platoo_epochs = a.opt.lk.heuristic.platoo_epochs = parse_usize(s, val());
        else if (s == "--n_nearest" || s == "--n-nearest") a.opt.heuristic.n_nearest = a.opt.lk.heuristic.n_nearest = a.opt.bnb.n_nearest = parse_usize(s, val());  // (branch_and_bound: only an explicit K restricts it)
        else if (s == "--max-nodes" || s == "--max_nodes") a.opt.bnb.max_nodes = parse_usize(s, val());
        else if (s == "--time-limit-ms" || s == "--time_limit_ms") a.opt.bnb.time_limit_ms = (uint32_t)std::min<size_t>(parse_usize(s, val()), 0xFFFFFFFFu);
        else if (s == "--max-depth") a.opt.lk.max_depth = parse_usize(s, val());
        else if (s == "-v" || s == "--verbose") a.opt.heuristic.verbose = true;
        else if (s == "--seed") a.opt.seed = std::stoull(val());
        else if (s == "--best-sweep") a.best = true;
        else if (s == "--exact-walk") a.exact_walk = true;
        else if (s == "--device") a.device = std::stoi(val());
        else if (s == "--stats") a.stats = true;
        else if (s == "--short") a.short_list = true;
        else if (s == "--learning_rate" || s == "--learning-rate") a.opt.som.learning_rate = std::stod(val());
        else if (s == "--radius_fraction" || s == "--radius-fraction") a.opt.som.radius_fraction = std::stod(val());
        else if (s == "--neuron_multiplier" || s == "--neuron-multiplier") a.opt.som.neuron_multiplier = parse_usize(s, val());
        else if (s == "--k-max" || s == "--k_max") a.opt.fourier.k_max = parse_usize(s, val());
        else if (s == "--m") a.opt.fourier.m = parse_usize(s, val());
        else if (s == "--lambda-decay" || s == "--lambda_decay") a.opt.fourier.lambda_decay = std::stod(val());
        else if (s == "--lambda" || s == "--lr") {
            std::vector<double> &list = s == "--lambda" ? a.fourier_lambdas : a.fourier_lrs;
            const std::string v = val();
            list.clear();
            for (size_t at = 0; at <= v.size();) {
                const size_t comma = std::min(v.find(',', at), v.size());
                list.push_back(std::stod(v.substr(at, comma - at)));
                at = comma + 1;
            }
        }
        else if (s == "--lower-bound" || s == "--lower_bound") a.lower_bound = true;
        else if (s == "--upper") a.upper = std::stod(val());
        else if (s == "--tour") a.tour_file = val();
        else if (s == "--root") a.bound_opt.root = parse_usize(s, val());
        else if (s == "--iterations") a.bound_opt.iterations = parse_usize(s, val());
        else if (s == "--patience") {
            const std::string v = val();
            a.bound_patiences.clear();
            for (size_t at = 0; at <= v.size();) {
                const size_t comma = std::min(v.find(',', at), v.size());
                a.bound_patiences.push_back((double)parse_usize(s, v.substr(at, comma - at)));
                at = comma + 1;
            }
        }
        else if (s == "--candidates") {  // alpha[:K]
            const std::string v = val();
            const size_t colon = v.find(':');
            if (v.substr(0, colon) != "alpha") usage_exit("--candidates: alpha[:K]");
            a.cand_alpha = true;
            if (colon != std::string::npos) a.cand_k = (uint32_t)std::min<size_t>(parse_usize(s, v.substr(colon + 1)), 0xFFFFFFFFu);
        }
        else if (s == "--alpha" && a.cmd == "candidates") a.cand_alpha = true;
        else if (s == "-k" && a.cmd == "candidates") a.cand_k = (uint32_t)std::min<size_t>(parse_usize(s, val()), 0xFFFFFFFFu);
        else if (s == "--ascent-iterations" || s == "--ascent_iterations") a.ascent_iterations = parse_usize(s, val());
        else if (s == "--progress-digest") a.progress_digest = true;
        else if (s == "--timing") a.timing = true;
        else if (s == "--full-exit") a.full_exit = true;
        else if (s == "--repeat") a.repeat = std::max(1, std::stoi(val()));
        else usage_exit(("unexpected argument " + s).c_str());
    }
    if (a.output_format != "text" && a.output_format != "json") usage_exit("--output-format: text or json");
    if (!a.fourier_lambdas.empty()) a.opt.fourier.lambda = a.fourier_lambdas[0];
    if (!a.fourier_lrs.empty()) a.opt.fourier.lr = a.fourier_lrs[0];
    if (a.cand_alpha && a.cand_k == 0) usage_exit("the candidate lists' K must be >= 1");
    if (a.cmd == "candidates") {
        if (!a.cand_alpha) usage_exit("candidates: --alpha is required (the kd-tree's lists have no command of their own)");
        if (a.file.empty()) usage_exit("candidates: -i FILE is required");
        return a;
    }
    if (a.cmd == "bound") {
        if (a.file.empty()) usage_exit("bound: -i FILE is required");
        if (a.upper != 0.0 && !a.tour_file.empty()) usage_exit("bound: --upper or --tour, not both");
        return a;  // (--lambda is lambda0's list here, not the Fourier curve's)
    }
    if (a.fourier_lambdas.size() > 1 || a.fourier_lrs.size() > 1) {  // the grid, lambda the outer index: one job each, the best kept
        const std::vector<double> las = a.fourier_lambdas.empty() ? std::vector<double>{a.opt.fourier.lambda} : a.fourier_lambdas;
        const std::vector<double> lrs = a.fourier_lrs.empty() ? std::vector<double>{a.opt.fourier.lr} : a.fourier_lrs;
        for (double la : las)
            for (double lr : lrs) {
                fourier_curve::FourierOptions o = a.opt.fourier;
                o.lambda = la;
                o.lr = lr;
                a.opt.fourier_jobs.push_back(o);
            }
    }
    if (a.opt.heuristic.n_nearest == 0) {  // HeuristicOptions::validate (mod.rs:677-682), through solve_with_context
        std::fprintf(stderr, "error: n_nearest must be >= 1\n");
        std::exit(1);
    }
    if (a.opt.lk.max_depth == 0) {
        std::fprintf(stderr, "error: max_depth must be >= 1\n");
        std::exit(1);
    }
    exit_if_invalid(a.opt.sa.validate());   // SAOptions::from_cli validates (mod.rs:708-742)
    exit_if_invalid(a.opt.ga.validate());   // GAOptions::validate (mod.rs:833-846)
    exit_if_invalid(a.opt.aco.validate());  // AcoOptions::validate (mod.rs:1115-1153)
    a.opt.two_opt_mode = a.best ? TL_MODE_BEST_SWEEP : TL_MODE_REF_ORDER;
    return a;
}

std::vector<Solvers> parse_steps(const std::string &csv)
{
    std::vector<Solvers> v;
    std::stringstream ss(csv);
    for (std::string tok; std::getline(ss, tok, ',');) {
        Solvers s;
        std::string why;
        if (!solver_from_str(tok, s, why)) {
            std::fprintf(stderr, "error: %s: `%s`\n", why.c_str(), tok.c_str());
            std::exit(1);
        }
        v.push_back(s);
    }
    return v;
}

// milliseconds between the start of this process (field 22 of /proc/self/stat, clock ticks since boot) and now: what the dynamic
// loader and the static initialisers of libamdhip64 / libteeline_gpu took before main() (10 ms resolution); -1 if unreadable
double ms_since_process_start()
{
    std::ifstream st("/proc/self/stat");
    std::string line;
    if (!st || !std::getline(st, line)) return -1.0;
    const size_t rp = line.rfind(')');
    if (rp == std::string::npos) return -1.0;
    std::istringstream rest(line.substr(rp + 2));
    std::string tok;
    for (int f = 3; f <= 22 && (rest >> tok); ++f)
        if (f == 22) {
            const double start_s = std::strtod(tok.c_str(), nullptr) / (double)sysconf(_SC_CLK_TCK);
            std::ifstream up("/proc/uptime");
            double now_s = 0.0;
            if (!(up >> now_s)) return -1.0;
            return (now_s - start_s) * 1e3;
        }
    return -1.0;
}

bool g_full_exit = false;

int run(int argc, char **argv);

}  // namespace

int main(int argc, char **argv)
{
    const int rc = run(argc, argv);
    std::fflush(stdout);
    std::fflush(stderr);
    if (!g_full_exit) _exit(rc);  // skip the HIP runtime's static teardown (measured: tests/probes/create_cost_probe.cpp)
    return rc;
}

namespace {
int run(int argc, char **argv)
{
    using clk = std::chrono::steady_clock;
    const double ms_before_main = ms_since_process_start();
    const auto t_main = clk::now();
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    try {
        Args a = parse(argc, argv);
        g_full_exit = a.full_exit;
        if (a.cmd == "solvers") {  // `teeline solvers [--short]`, restricted to what this build runs
            static const char *rows[][3] = {{"nearest_neighbor", "nn", "heuristic"}, {"two_opt", "2opt", "heuristic"}, {"three_opt", "3opt", "heuristic"},
                                            {"or_opt", "or-opt", "heuristic"}, {"lin_kernighan", "lk", "heuristic"}, {"random_shuffle", "shuffle", "heuristic"}};
            if (!a.short_list) std::printf("%-22s %-8s TYPE\n", "NAME", "ALIAS");
            for (auto &r : rows) {
                if (a.short_list) std::printf("%s\n", r[1]);
                else std::printf("%-22s %-8s %s\n", r[0], r[1], r[2]);
            }
            return 0;
        }
        std::vector<Solvers> stages;
        const bool json_mode = a.cmd == "solve" && a.output_format == "json";  // `pipeline` always prints text (main.rs:425,430)
        if (a.cmd == "bound" || a.cmd == "candidates") {
            stages = {Solvers::NearestNeighbor, Solvers::TwoOpt};  // where neither --upper nor --tour gives the upper bound
        } else if (a.cmd == "solve") {
            std::string name = a.solver;
            for (auto &ch : name) ch = (char)std::tolower((unsigned char)ch);
            if (name == "fast") stages = {Solvers::NearestNeighbor, Solvers::TwoOpt};  // resolve_preset (main.rs:354-369)
            else if (name == "classic") stages = {Solvers::NearestNeighbor, Solvers::TwoOpt, Solvers::SimulatedAnnealing};
            else if (name == "thorough") stages = {Solvers::NearestNeighbor, Solvers::ThreeOpt, Solvers::SimulatedAnnealing};
            else {
                Solvers s;
                std::string why;
                if (!solver_from_str(name, s, why)) {
                    std::fprintf(stderr, "error: %s: `%s`\n", why.c_str(), a.solver.c_str());
                    return why == "unknown solver" ? 2 : 1;
                }
                // auto_expand_with_nn (mod.rs:129-139): deterministic local searches are seeded with a nearest-neighbour stage
                const bool expand = s == Solvers::TwoOpt || s == Solvers::ThreeOpt || s == Solvers::LinKernighan || s == Solvers::OrOpt || s == Solvers::TabuSearch || s == Solvers::BranchAndBound;
                if (s == Solvers::TwoOpt && a.runs >= 2) {  // seeded restarts: no warm start to build
                    a.opt.two_opt_runs = a.runs;
                    stages = {s};
                } else if (!a.no_seed && expand) stages = {Solvers::NearestNeighbor, s};
                else if (!a.no_seed && (s == Solvers::SimulatedAnnealing || s == Solvers::GeneticAlgorithm || s == Solvers::AntColony || s == Solvers::ParticleSwarm || s == Solvers::CuckooSearch || s == Solvers::FlowerPollination || s == Solvers::GravitationalSearch || s == Solvers::HillClimb)) stages = {Solvers::RandomShuffle, s};  // mod.rs:144-157
                else stages = {s};
            }
        } else {
            if (a.steps.empty()) {
                std::fprintf(stderr, "error: pipeline: provide --steps (TOML --config files are not read by this façade)\n");
                return 1;
            }
            stages = parse_steps(a.steps);
        }
        if (a.cmd != "bound" && a.cmd != "candidates" && a.runs >= 2 && !stages.empty() && stages.back() == Solvers::LinKernighan) a.opt.lk_runs = a.runs;  // seeded runs of the last lk stage
        for (const auto &w : pipeline::stage_warnings(stages)) std::fprintf(stderr, "warning: %s\n", w.c_str());

        tsplib::TspLibData data;
        if (a.file.empty()) {
            try {
                data = tsplib::read_from_string(std::string(std::istreambuf_iterator<char>(std::cin), {}));
            } catch (const std::exception &e) {
                std::fprintf(stderr, "Failed to read TSPLIB file from STDIN: \"%s\"\n", e.what());
                return 1;
            }
        } else {
            if (!std::ifstream(a.file)) {
                std::fprintf(stderr, "File doesnt exists: \"%s\"\n", a.file.c_str());  // main.rs:715-718
                return 1;
            }
            try {
                data = tsplib::read_from_file(a.file);
            } catch (const std::exception &e) {
                std::fprintf(stderr, "Error in TSPLIB file: \"%s\"\n", e.what());
                return 1;
            }
        }
        if (!a.distance_type.empty()) {  // --distance-type (main.rs:461-471): euc_2d | geo
            std::string d = a.distance_type;
            for (auto &ch : d) ch = (char)std::tolower((unsigned char)ch);
            if (d == "euc_2d" || d == "euc2d") data.distance_type = DistanceType::Euc2D;
            else if (d == "geo") data.distance_type = DistanceType::Geo;
            else {
                std::fprintf(stderr, "error: --distance-type: unknown distance type `%s`\n", a.distance_type.c_str());
                return 1;
            }
        }
        const double ms_read = ms_since(t_main);
        const auto t_ctx = clk::now();
        Context ctx(a.device, a.exact_walk ? TL_FLAG_BHK_EXACT_WALK : TL_FLAG_NONE);
        const double ms_create = ms_since(t_ctx);
        const auto t_prob = clk::now();
        TspProblem problem = data.problem(ctx);
        const double ms_problem = ms_since(t_prob);
        bool have_opt = false;
        opt_tour::OptTour ot;
        if (!a.optimal_tour.empty()) {
            try {
                ot = opt_tour::read_from_file(a.optimal_tour);
                have_opt = true;
            } catch (const std::exception &e) {
                std::fprintf(stderr, "--optimal-tour: %s\n", e.what());  // main.rs:486-493: reported, then ignored
            }
        }
        // --progress-digest (a test hook, not in teeline-cli): every stage gets a progress callback, as teeline-qt's sender would be,
        // and the message stream — which this mirror replays from the *_trace entries — is summarised on stderr: counts per kind and
        // an FNV-1a digest over (kind, ids as u64, f32 bits) per message (Done: the kind only), comparable across the mirrors
        struct Digest {
            uint64_t h = 1469598103934665603ull, n[4] = {0, 0, 0, 0};
            void byte(uint8_t b) { h = (h ^ b) * 1099511628211ull; }
            void word(uint64_t v, int bytes) { for (int k = 0; k < bytes; ++k) byte((uint8_t)(v >> (8 * k))); }
        } dg;
        ProgressFn on_progress = [&dg](ProgressKind kind, const std::vector<size_t> &ids, float v) {
            const int k = kind == ProgressKind::PathUpdate ? 0 : kind == ProgressKind::CityChange ? 1 : kind == ProgressKind::EpochUpdate ? 3 : 2;
            dg.n[k] += 1;
            dg.byte((uint8_t)k);
            if (k == 2) return;
            dg.word(ids.size(), 4);
            for (size_t id : ids) dg.word(id, 8);
            uint32_t bits;
            std::memcpy(&bits, &v, 4);
            dg.word(k == 0 ? bits : 0u, 4);
        };
        if (a.cmd == "bound") {
            double upper = a.upper;
            std::string upper_from = "--upper";
            if (!a.tour_file.empty()) {  // the tour's length by tl_tour_length, as --optimal-tour prices one
                cli::OptimalComparison cmp;
                if (!cli::compute_optimal_comparison(ctx, 0.0f, problem, opt_tour::read_from_file(a.tour_file), cmp) || !(cmp.optimal_cost > 0.0f)) {
                    std::fprintf(stderr, "error: bound: --tour: no tour of this instance in `%s`\n", a.tour_file.c_str());
                    return 1;
                }
                upper = (double)cmp.optimal_cost;
                upper_from = "--tour";
            } else if (upper == 0.0) {
                upper = (double)pipeline::run_pipeline_stages(ctx, problem, stages, a.opt).back().solution.total;
                upper_from = "nn,2opt";
            }
            const std::vector<double> las = a.fourier_lambdas.empty() ? std::vector<double>{a.bound_opt.lambda0} : a.fourier_lambdas;
            const std::vector<double> pats = a.bound_patiences.empty() ? std::vector<double>{(double)a.bound_opt.patience} : a.bound_patiences;
            std::vector<one_tree_bound::BoundOptions> jobs;
            for (double la : las)
                for (double pa : pats) {
                    one_tree_bound::BoundOptions o = a.bound_opt;
                    o.lambda0 = la;
                    o.patience = (size_t)pa;
                    jobs.push_back(o);
                }
            const one_tree_bound::Bound b = one_tree_bound::bound_batch(ctx, problem, upper, jobs);
            const one_tree_bound::BoundOptions &bo = jobs[b.job];
            if (a.output_format == "json")
                std::printf("{\"bound\":%s,\"gap_pct\":%s,\"iterations_run\":%u,\"job\":%u,\"jobs\":%zu,\"lambda\":%s,\"patience\":%zu,\"proved\":%s,\"upper\":%s,\"upper_from\":\"%s\"}\n",
                            cli::json_f64(b.bound).c_str(), cli::json_f64(b.gap_pct(upper)).c_str(), b.result.iterations_run, b.job, jobs.size(),
                            cli::json_f64(bo.lambda0).c_str(), bo.patience, b.is_tour ? "true" : "false", cli::json_f64(upper).c_str(), upper_from.c_str());
            else
                std::printf("bound=%.17g job=%u of %zu (lambda=%g patience=%zu) upper=%.17g (%s) gap_pct=%.4f%s\n", b.bound, b.job, jobs.size(), bo.lambda0, bo.patience,
                            upper, upper_from.c_str(), b.gap_pct(upper), b.is_tour ? " proved=1" : "");
            return 0;
        }
        // alpha-nearness lists: the ascent as `bound` runs it (upper from nn,2opt), its best penalties, the lists under them
        auto alpha_lists = [&]() {
            std::vector<double> pi;
            if (a.ascent_iterations > 0) {
                const double upper = (double)pipeline::run_pipeline_stages(ctx, problem, {Solvers::NearestNeighbor, Solvers::TwoOpt}, a.opt).back().solution.total;
                one_tree_bound::BoundOptions bo = a.bound_opt;
                bo.iterations = a.ascent_iterations;
                pi = one_tree_bound::bound(ctx, problem, upper, bo).pi;
            }
            return alpha_candidates::candidates(ctx, problem, a.cand_k, pi, (uint32_t)std::min<size_t>(a.bound_opt.root, 0xFFFFFFFFu));
        };
        if (a.cmd == "candidates") {
            const alpha_candidates::Lists L = alpha_lists();
            for (uint32_t i = 0; i < L.n; ++i) {
                std::printf("%zu:", problem.cities[i].id);
                for (uint32_t q = 0; q < L.k; ++q) std::printf(" %zu", problem.cities[L.rows[(size_t)i * L.k + q]].id);
                std::printf("\n");
            }
            return 0;
        }
        const bool has_lk = std::find(stages.begin(), stages.end(), Solvers::LinKernighan) != stages.end();
        uint32_t lists_k = 0;  // != 0: every lk step searches alpha lists of this width
        if (a.cand_alpha && !has_lk) std::fprintf(stderr, "warning: --candidates: no lk step searches them\n");
        if (a.cand_alpha && has_lk) {
            const alpha_candidates::Lists L = alpha_lists();
            if (L.k >= 1u) {
                alpha_candidates::set_lk_lists(ctx, L);
                lists_k = L.k;
            }
        }
        if (a.progress_digest) a.opt.progress = &on_progress;
        std::string runs_json;
        std::vector<pipeline::StageOutcome> outcomes;
        for (int rep = 0; rep < a.repeat; ++rep) {
            const auto t_run = clk::now();
            outcomes = pipeline::run_pipeline_stages(ctx, problem, stages, a.opt);
            char buf[160];
            std::snprintf(buf, sizeof(buf), "%s{\"wall_ms\": %.4f, \"stages\": [", rep ? ", " : "", ms_since(t_run));
            runs_json += buf;
            for (size_t k = 0; k < outcomes.size(); ++k) {
                std::snprintf(buf, sizeof(buf), "%s{\"solver\": \"%s\", \"wall_ms\": %.4f, \"kernel_ms\": %.4f}", k ? ", " : "", solver_name(outcomes[k].solver),
                              outcomes[k].duration_us * 1e-3, outcomes[k].solution.stats.kernel_ms);
                runs_json += buf;
            }
            runs_json += "]}";
        }
        if (lists_k) alpha_candidates::clear_lk_lists(ctx);
        const auto t_out = clk::now();
        if (a.progress_digest) {
            std::fprintf(stderr, "progress: path_updates=%llu city_changes=%llu done=%llu digest=%016llx", (unsigned long long)dg.n[0],
                         (unsigned long long)dg.n[1], (unsigned long long)dg.n[2], (unsigned long long)dg.h);
            if (dg.n[3]) std::fprintf(stderr, " epoch_updates=%llu", (unsigned long long)dg.n[3]);  // (ant_colony, particle_swarm, cuckoo_search, flower_pollination and gravitational_search stages only)
            std::fprintf(stderr, "\n");
        }
        const Solution &tour = outcomes.back().solution;
        if (!json_mode) std::fputs(cli::format_solution(tour, false).c_str(), stdout);
        cli::OptimalComparison cmp;
        const bool have_cmp = have_opt && cli::compute_optimal_comparison(ctx, tour.total, problem, ot, cmp);
        one_tree_bound::Bound lb;
        if (a.lower_bound) lb = one_tree_bound::bound(ctx, problem, (double)tour.total);  // the solved tour is the upper bound
        if (json_mode) std::fputs(cli::format_solution_json(tour, false, have_cmp ? &cmp : nullptr, a.lower_bound ? &lb : nullptr, outcomes.back().best_run, a.opt.lk_runs).c_str(), stdout);
        else if (have_cmp) std::fputs(cli::format_optimal_comparison(tour.total, cmp).c_str(), stderr);
        if (a.lower_bound && !json_mode) std::fputs(cli::format_lower_bound(tour.total, lb).c_str(), stderr);
        if (a.timing) {
            std::fflush(stdout);
            std::fprintf(stderr, "{\"timing_ms\": {\"before_main\": %.1f, \"read_input\": %.4f, \"tl_create\": %.4f, \"problem\": %.4f, \"runs\": [%s], \"output\": %.4f, \"main_total\": %.4f}, \"n\": %zu}\n",
                         ms_before_main, ms_read, ms_create, ms_problem, runs_json.c_str(), ms_since(t_out), ms_since(t_main), problem.cities.size());
        }
        if (a.stats)
            for (const auto &o : outcomes) {
                std::fprintf(stderr, "stage %s: cost=%.5f sweeps=%llu candidates=%llu moves=%llu kernel_ms=%.3f wall_ms=%llu", solver_name(o.solver),
                             o.solution.total, (unsigned long long)o.solution.stats.sweeps, (unsigned long long)o.solution.stats.candidates,
                             (unsigned long long)o.solution.stats.moves, o.solution.stats.kernel_ms, (unsigned long long)o.duration_ms);
                if (o.best_restart >= 0) std::fprintf(stderr, " best_restart=%lld", (long long)o.best_restart);
                if (o.best_run >= 0) std::fprintf(stderr, " best_run=%lld", (long long)o.best_run);
                if (o.solver == Solvers::LinKernighan) {  // the lists the step searched: their kind and width
                    const size_t n1 = problem.cities.empty() ? 0 : problem.cities.size() - 1;
                    if (lists_k) std::fprintf(stderr, " lists=alpha:%u", lists_k);
                    else std::fprintf(stderr, " lists=kdtree:%zu", std::min(a.opt.lk.heuristic.n_nearest, n1));
                }
                std::fprintf(stderr, "\n");
            }
        return 0;
    } catch (const ReferencePanic &e) {
        std::fprintf(stderr, "thread 'main' panicked: %s\n", e.what());
        return 101;  // Rust's panic exit code
    } catch (const std::exception &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
}
}  // namespace
