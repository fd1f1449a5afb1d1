// algames_unit.hip -- one list of configurations applied to one instantiation macro (both of algames_kernels.hpp): the source of every
// translation unit that holds the kernels, the scheduled loops, the KKT solves or the plant knots of one family.  The build names the two,
// e.g. -DALG_UNIT_CFGS=ALG_CFGS_P7 -DALG_UNIT_KERNELS=ALG_DEFINE_KKT, and picks the unit's flags by the family (the table of families in
// __graft_entry__.py).  Translation units of their own, so that they build in parallel and a unit that holds older kernels compiles from the
// source it always had.  Launched from algames_hip.hip, which declares every instantiation `extern template`.
#include "algames_kernels.hpp"

#if !defined(ALG_UNIT_CFGS) || !defined(ALG_UNIT_KERNELS)
#error "compile with -DALG_UNIT_CFGS=<an ALG_CFGS_* list> -DALG_UNIT_KERNELS=<an ALG_DEFINE_* macro>"
#endif
ALG_UNIT_CFGS(ALG_UNIT_KERNELS)
