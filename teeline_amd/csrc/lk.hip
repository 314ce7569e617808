// lk.hip — Lin–Kernighan (reference: src/tsp/lin_kernighan.rs).  (Candidate lists: kdtree.hip; NN seed and brute-force lists:
// nn_knn.hip.)
//
// Compiled twice: as it stands (namespace tl, chains of up to TL_LK_MAX_DEPTH = 6 exchanges held in registers — LKOptions::default()
// is 5, the CLI's --max-depth default too) and through lk_deep.hip with TL_LK_MAX_DEPTH 16 in namespace tl_lk_deep for
// max_depth 7..16 (the reference's max_depth is an unbounded usize, mod.rs:1252; recursion lin_kernighan.rs:265-340).
//
// ONE translation unit in parts, a form of the solver each (lk_chain, chain_valid and lk_file_move are not force-inlined: parts
// compiled on their own would each carry a copy and decide its inlining for themselves).  Which form runs is lk_run's decision
// (tl_api_lk.hip):
//   lk_chain.h          what the forms share: constants, slot layouts, the two views, find_lk_chain, the arc model, index helpers.
//   lk_ils.h            k_lk_ils + k_lk_ils_commit, the LDS-resident ILS with speculative epochs: n <= 700, or TL_FLAG_LK_ILS_LDS.
//   lk_scan.h           the chip-wide form, a round = scan + step: every larger n.  k_lk_scan_sub<true, true> + k_lk_control<true>
//                       unless a flag asks for another scan (TL_FLAG_LK_CLASSIC_VIEW, and the tuning build's TL_FLAG_LK_NO_SPLIT,
//                       _SPLIT2, _SEPARATE_PICK, _SEPARATE_STEP); k_lk_control<false> + k_lk_rebuild below n = 1 500.
//   lk_scan_persist.h   k_lk_scan_persist: tuning build, TL_FLAG_LK_SCAN_PERSIST.  lk_scan.h includes it where the kernel stood.
//   lk_one_workgroup.h  k_lk_solve, a cross-check: TL_FLAG_LK_ONE_WORKGROUP; its LDS variant in the tuning build (TL_FLAG_LK_SMALL).
// The order of the includes is part of the build: kernel templates are emitted in the order in which the launch functions name
// them, plain kernels in the order of their definitions, and the code follows that order (behind another one k_lk_scan<false>
// schedules 18 instructions differently, and k_lk_scan_sub's call of lk_file_move spans another distance: scripts/isa_diff.py).
#include "tl_kernels.h"
#include <type_traits>

#pragma clang fp contract(off)

#ifndef TL_LK_MAX_DEPTH
#define TL_LK_MAX_DEPTH 6
#endif
#ifndef TL_LK_NS
#define TL_LK_NS tl
#endif

namespace TL_LK_NS {
using namespace tl;  // (a no-op for the default namespace)

#include "lk_chain.h"
#include "lk_ils.h"
#include "lk_scan.h"
#include "lk_one_workgroup.h"

}  // namespace TL_LK_NS
