// algames_plant.hip -- the step-wise plant knot of the receding-horizon loop (k_mpc_plant_advance of algames_kernels.hpp; alg_mpc_plant_advance):
// one small kernel per one-wavefront configuration of the library, around the device function the fused loops (k_mpc_loop_sched) run per knot.
// A translation unit of its own, so that the units holding the solver kernels compile from the source they always had.
#include "algames_kernels.hpp"

ALG_CFGS_BASE(ALG_DEFINE_PLANT)
ALG_CFGS_BASE_SCEN(ALG_DEFINE_PLANT)
ALG_CFGS_EXT(ALG_DEFINE_PLANT)
ALG_CFGS_DENSE(ALG_DEFINE_PLANT)
ALG_CFGS_DI1(ALG_DEFINE_PLANT)
