// algames_base.hip -- kernels of the base configurations (ALG_CFGS_BASE of algames_kernels.hpp; the BASELINE shapes C1..C5 run
// these) and of their twins that read the scenario numbers from the game's block (ALG_CFGS_BASE_SCEN, Cfg::SCEN: a handle in
// ALG_SCEN_KERNELS_BASE mode runs these while any base kind is per game).  One translation unit per entry: the build compiles this file
// once per index and ext value with -DALG_BASE_SEL=<0..8> -DALG_BASE_EXT=<0 | 2> (__graft_entry__.HIP_UNITS), so the instantiations build
// in parallel and a change of one kernel shape rebuilds in seconds.  Launched from algames_hip.hip, which declares them `extern template`.
// (ALG_DEFINE_KERNELS_VIO: the entry's kernels and its solve with violation profiles, k_newton_solve_vio)
#include "algames_kernels.hpp"

#ifndef ALG_BASE_SEL
#error "compile with -DALG_BASE_SEL=<index into ALG_CFGS_BASE> [-DALG_BASE_EXT=<its ext column: 0 or 2>]"
#endif
#ifndef ALG_BASE_EXT
#define ALG_BASE_EXT 0          // (a command line that names the entry only builds the entry of ALG_CFGS_BASE, as it always did)
#endif
#if ALG_BASE_EXT != 0 && ALG_BASE_EXT != 2
#error "ALG_BASE_EXT is the ext column of ALG_CFGS_BASE (0) or of ALG_CFGS_BASE_SCEN (2)"
#endif
#if ALG_BASE_SEL == 0
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 2, ALG_BASE_EXT)
#elif ALG_BASE_SEL == 1
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 2, ALG_BASE_EXT)
#elif ALG_BASE_SEL == 2
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, ALG_BASE_EXT)
ALG_INSTANTIATE_HO_PARK(template, ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, ALG_BASE_EXT, 4)          // (budgeted solve of the straggler hand-off, ALG_CFGS_HANDOFF_E)
#elif ALG_BASE_SEL == 3
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 2, ALG_BASE_EXT)
#elif ALG_BASE_SEL == 4
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 3, ALG_BASE_EXT)
#elif ALG_BASE_SEL == 5
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_UNICYCLE, 1, 2, ALG_BASE_EXT)
#elif ALG_BASE_SEL == 6
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_UNICYCLE, 2, 2, ALG_BASE_EXT)
#elif ALG_BASE_SEL == 7
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_UNICYCLE, 3, 2, ALG_BASE_EXT)
ALG_INSTANTIATE_HO_PARK(template, ALG_MODEL_UNICYCLE, 3, 2, ALG_BASE_EXT, 4)
#elif ALG_BASE_SEL == 8
ALG_DEFINE_KERNELS_VIO(ALG_MODEL_UNICYCLE, 4, 2, ALG_BASE_EXT)
ALG_INSTANTIATE_HO_PARK(template, ALG_MODEL_UNICYCLE, 4, 2, ALG_BASE_EXT, 4)
#else
#error "ALG_BASE_SEL out of range (ALG_CFGS_BASE has nine entries)"
#endif
