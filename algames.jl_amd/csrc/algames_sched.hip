// algames_sched.hip -- the receding-horizon loops that apply a schedule (k_mpc_loop_sched of algames_kernels.hpp; alg_mpc_set_schedule):
// one sibling per k_mpc_loop instantiation of the library.  Translation units of their own, so that the units holding k_mpc_loop and
// k_newton_solve compile from the source they always had.  The build compiles this file once per group with -DALG_SCHED_SEL=<0..20> and
// the flags of the group's unscheduled unit (__graft_entry__.HIP_UNITS).  Launched from algames_hip.hip, which declares them `extern template`.
#include "algames_kernels.hpp"

#ifndef ALG_SCHED_SEL
#error "compile with -DALG_SCHED_SEL=<group>"
#endif
#define ALG_SCHED_BASE_E(E)                                                                     \
    ALG_DEFINE_SCHED(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 2, E) ALG_DEFINE_SCHED(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 2, E)  \
    ALG_DEFINE_SCHED(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, E) ALG_DEFINE_SCHED(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 2, E)  \
    ALG_DEFINE_SCHED(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 3, E)
#define ALG_SCHED_BASE_UNI_E(E)                                                                 \
    ALG_DEFINE_SCHED(ALG_MODEL_UNICYCLE, 1, 2, E) ALG_DEFINE_SCHED(ALG_MODEL_UNICYCLE, 2, 2, E) \
    ALG_DEFINE_SCHED(ALG_MODEL_UNICYCLE, 3, 2, E) ALG_DEFINE_SCHED(ALG_MODEL_UNICYCLE, 4, 2, E)
#if ALG_SCHED_SEL == 0                  // ALG_CFGS_BASE, DoubleIntegrator
ALG_SCHED_BASE_E(0)
#elif ALG_SCHED_SEL == 1                // ALG_CFGS_BASE, Unicycle
ALG_SCHED_BASE_UNI_E(0)
#elif ALG_SCHED_SEL == 2                // ALG_CFGS_BASE_SCEN
ALG_SCHED_BASE_E(2)
#elif ALG_SCHED_SEL == 3
ALG_SCHED_BASE_UNI_E(2)
#elif ALG_SCHED_SEL == 4
ALG_CFGS_EXT_DI(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 5
ALG_CFGS_EXT_UNI(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 6
ALG_CFGS_EXT_BIC(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 7
ALG_CFGS_EXT_DI3(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 8
ALG_CFGS_MW(ALG_DEFINE_SCHED_MW)
#elif ALG_SCHED_SEL == 9
ALG_CFGS_MW_SCEN(ALG_DEFINE_SCHED_MW)
#elif ALG_SCHED_SEL == 10
ALG_CFGS_QUAD(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 11
ALG_CFGS_QUAD_EXT(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 12
ALG_CFGS_DI3D(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 13
ALG_CFGS_MW_DENSE(ALG_DEFINE_SCHED_MW)
#elif ALG_SCHED_SEL == 14
ALG_CFGS_P5(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 15
ALG_CFGS_P6(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 16
ALG_CFGS_DI1(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 17
ALG_CFGS_P7(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 18
ALG_CFGS_P8(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 19
ALG_CFGS_P9(ALG_DEFINE_SCHED)
#elif ALG_SCHED_SEL == 20
ALG_CFGS_P10(ALG_DEFINE_SCHED)
#else
#error "ALG_SCHED_SEL out of range (21 groups)"
#endif
