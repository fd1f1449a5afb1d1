// Explicit instantiations of the team kernels (several wavefronts per game; ALG_CFGS_MW_E of algames_kernels.hpp): their own
// translation unit so that they compile in parallel with the others.  Compiled once per ext value with -DALG_MW_EXT=<0 | 2>
// (__graft_entry__.HIP_UNITS): ALG_CFGS_MW, and ALG_CFGS_MW_SCEN, the twins that read the game's scenario block.
#include "algames_kernels.hpp"

#ifndef ALG_MW_EXT
#define ALG_MW_EXT 0            // (a command line without it builds ALG_CFGS_MW, as it always did)
#endif
#if ALG_MW_EXT != 0 && ALG_MW_EXT != 2
#error "ALG_MW_EXT is the ext column of ALG_CFGS_MW (0) or of ALG_CFGS_MW_SCEN (2)"
#endif
ALG_CFGS_MW_E(ALG_DEFINE_MW_VIO, ALG_MW_EXT)          // (the team kernels and their solves with violation profiles, k_newton_solve_vio)
// ... and the kernels that resume the games a budgeted one-wavefront solve parked (straggler hand-off, alg_set_handoff)
ALG_CFGS_HANDOFF_E(ALG_DEFINE_HO_RESUME, ALG_MW_EXT)
