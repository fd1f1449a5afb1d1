// algames_kkt.hip -- the KKT solves with many right-hand sides (k_kkt_solve of algames_kernels.hpp; alg_kkt_solve): one kernel per
// configuration that has a k_direction.  Translation units of their own, so that the units holding the existing kernels compile from the
// source they always had.  The build compiles this file once per group with -DALG_KKT_SEL=<0..17> and the flags of the unit that holds the
// group's k_direction (__graft_entry__.HIP_UNITS).  Launched from algames_hip.hip, which declares them `extern template`.
#include "algames_kernels.hpp"

#ifndef ALG_KKT_SEL
#error "compile with -DALG_KKT_SEL=<group>"
#endif
#define ALG_KKT_BASE_DI_E(E)                                                                    \
    ALG_DEFINE_KKT(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 2, E) ALG_DEFINE_KKT(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 2, E)  \
    ALG_DEFINE_KKT(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, E) ALG_DEFINE_KKT(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 2, E)  \
    ALG_DEFINE_KKT(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 3, E)
#define ALG_KKT_BASE_UNI_E(E)                                                                   \
    ALG_DEFINE_KKT(ALG_MODEL_UNICYCLE, 1, 2, E) ALG_DEFINE_KKT(ALG_MODEL_UNICYCLE, 2, 2, E)     \
    ALG_DEFINE_KKT(ALG_MODEL_UNICYCLE, 3, 2, E) ALG_DEFINE_KKT(ALG_MODEL_UNICYCLE, 4, 2, E)
#if ALG_KKT_SEL == 0                    // ALG_CFGS_BASE, DoubleIntegrator
ALG_KKT_BASE_DI_E(0)
#elif ALG_KKT_SEL == 1                  // ALG_CFGS_BASE, Unicycle
ALG_KKT_BASE_UNI_E(0)
#elif ALG_KKT_SEL == 2                  // ALG_CFGS_BASE_SCEN
ALG_KKT_BASE_DI_E(2)
#elif ALG_KKT_SEL == 3
ALG_KKT_BASE_UNI_E(2)
#elif ALG_KKT_SEL == 4
ALG_CFGS_EXT_DI(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 5
ALG_CFGS_EXT_UNI(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 6
ALG_CFGS_EXT_BIC(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 7
ALG_CFGS_EXT_DI3(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 8
ALG_CFGS_QUAD(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 9
ALG_CFGS_QUAD_EXT(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 10
ALG_CFGS_DI3D(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 11
ALG_CFGS_P5(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 12
ALG_CFGS_P6(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 13
ALG_CFGS_DI1(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 14
ALG_CFGS_P7(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 15
ALG_CFGS_P8(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 16
ALG_CFGS_P9(ALG_DEFINE_KKT)
#elif ALG_KKT_SEL == 17
ALG_CFGS_P10(ALG_DEFINE_KKT)
#else
#error "ALG_KKT_SEL out of range (18 groups)"
#endif
