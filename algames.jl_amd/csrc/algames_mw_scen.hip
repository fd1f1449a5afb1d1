// Explicit instantiations of the team kernels that read the game's scenario block (ALG_CFGS_MW_SCEN of algames_kernels.hpp) and of the
// kernels that resume the games a budgeted one-wavefront solve of that kind parked (ALG_CFGS_HANDOFF_SCEN): the twins of algames_mw.hip.
#include "algames_kernels.hpp"
ALG_CFGS_MW_SCEN(ALG_DEFINE_MW)
ALG_CFGS_HANDOFF_SCEN(ALG_DEFINE_HO_RESUME)
