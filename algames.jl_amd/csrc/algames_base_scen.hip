// algames_base_scen.hip -- the base configurations with the scenario numbers read from the game's block (ALG_CFGS_BASE_SCEN of
// algames_kernels.hpp, Cfg::SCEN: a handle in ALG_SCEN_KERNELS_BASE mode runs these while any base kind is per game).  One translation
// unit per entry, like algames_base.hip: compiled once per index with -DALG_BASE_SEL=<0..8> (__graft_entry__.HIP_UNITS).
// Launched from algames_hip.hip, which declares them `extern template`.
#include "algames_kernels.hpp"

#ifndef ALG_BASE_SEL
#error "compile with -DALG_BASE_SEL=<index into ALG_CFGS_BASE_SCEN>"
#endif
#if ALG_BASE_SEL == 0
ALG_DEFINE_KERNELS(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 2, 2)
#elif ALG_BASE_SEL == 1
ALG_DEFINE_KERNELS(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 2, 2)
#elif ALG_BASE_SEL == 2
ALG_DEFINE_KERNELS(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, 2)
ALG_INSTANTIATE_HO_PARK(template, ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, 2, 4)          // (budgeted solve of the straggler hand-off, ALG_CFGS_HANDOFF_SCEN)
#elif ALG_BASE_SEL == 3
ALG_DEFINE_KERNELS(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 2, 2)
#elif ALG_BASE_SEL == 4
ALG_DEFINE_KERNELS(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 3, 2)
#elif ALG_BASE_SEL == 5
ALG_DEFINE_KERNELS(ALG_MODEL_UNICYCLE, 1, 2, 2)
#elif ALG_BASE_SEL == 6
ALG_DEFINE_KERNELS(ALG_MODEL_UNICYCLE, 2, 2, 2)
#elif ALG_BASE_SEL == 7
ALG_DEFINE_KERNELS(ALG_MODEL_UNICYCLE, 3, 2, 2)
ALG_INSTANTIATE_HO_PARK(template, ALG_MODEL_UNICYCLE, 3, 2, 2, 4)
#elif ALG_BASE_SEL == 8
ALG_DEFINE_KERNELS(ALG_MODEL_UNICYCLE, 4, 2, 2)
ALG_INSTANTIATE_HO_PARK(template, ALG_MODEL_UNICYCLE, 4, 2, 2, 4)
#else
#error "ALG_BASE_SEL out of range (ALG_CFGS_BASE_SCEN has nine entries)"
#endif
