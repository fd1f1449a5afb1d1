/*
 * algames_hip.h -- C ABI of the MI355X-native batched ALGAMES Newton / augmented-Lagrangian
 * hot path (libalgames_hip.so).
 *
 * The reference (RoboticExplorationLab/Algames.jl v0.1.6) has no FFI: its boundary is the
 * Julia API itself.  Every entry point below names the reference function (file:line under
 * /root/reference) that it replaces for a *batch* of B independent games that share
 * (model, p, N, dt, options, constraint structure) and differ in data (x0, targets,
 * multipliers, iterate).  A Julia host binds these with `ccall`.
 *
 * Conventions
 *   - all floating point data is IEEE fp64, all buffers are caller-owned host memory unless a
 *     function says "device"; the library owns device memory and its HIP stream.
 *   - batched buffers are game-major and contiguous: buf[g*len + e].
 *   - return value: 0 = ALG_OK, <0 = error, message in alg_last_error() (thread local).
 *     Numerical failure of individual games is reported per game (alg_game_stats.status),
 *     never as a call error.
 *   - a handle is not thread-safe; distinct handles are independent.
 *
 * Layouts (src/core/newton_core.jl:40-89)
 *   traj  (len n+S):  [ x_1 (n) | for k=1..N-1: x_{k+1} (n), u_{1,k} (mi) .. u_{p,k} (mi),
 *                                               lambda_{1,k} (n) .. lambda_{p,k} (n) ]
 *          i.e. x_1 followed by the reference's "horizontal" order = order of `Δtraj`
 *          (src/struct/primal_dual_traj.jl:46-107).  u_{i,k} holds joint-control entries
 *          pu[i] = {i + (j-1)p} in increasing order.
 *   res   (len S):    reference "vertical" order: for i=1..p, for k=1..N-1:
 *          [opt_i,x_{k+1} (n) | opt_i,u_{i,k} (mi)], then for k=1..N-1: dyn_k (n).
 *   jac   (S x S, column-major): rows vertical order, columns horizontal order.
 *   con duals / penalties / values (len alg_con_len()):
 *          [ collision avoidance: for pair q=(i,j) in the order of
 *            add_collision_avoidance! (constraints_methods.jl:21-33: for i, for j != i),
 *            for knot k=2..N: 1 row ]  then
 *          [ control bound: for knot k=1..N-1: rows (u-u_max)(m) then (u_min-u)(m) ].
 *          Rows of infinite bounds are kept (the reference drops them,
 *          control_bound_constraint.jl:35-38); they are never active and report value -inf.
 *          Extended constraints append, in this order and only when added:
 *          [ state bound: for player i, knot k=2..N: rows (x-x_max)(n) then (x_min-x)(n) ]
 *          [ wall: for player i, knot k=2..N: one row per wall ] [ circle: for player i, knot k=2..N: one row per circle ]
 *          [ 3-D wall: for player i, knot k=2..N: one row per Wall3D ] [ cylinder: for player i, knot k=2..N: one row per cylinder ]
 *          (spherical collision avoidance uses the collision-avoidance rows)
 *          alg_get_con_len() returns the current length.
 */
#ifndef ALGAMES_HIP_H
#define ALGAMES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALG_OK 0
#define ALG_ERR_ARG (-1)        /* bad argument / unsupported configuration            */
#define ALG_ERR_DEVICE (-2)     /* HIP runtime error                                   */
#define ALG_ERR_STATE (-3)      /* call sequence error (e.g. data not set)             */

/* src/dynamics/double_integrator.jl:13-31, src/dynamics/unicycle.jl:14-32 */
#define ALG_MODEL_DOUBLE_INTEGRATOR 0
#define ALG_MODEL_UNICYCLE 1
#define ALG_MODEL_BICYCLE 2             /* src/dynamics/bicycle.jl:2-41 (lf = lr = 0.05 unless alg_set_bicycle) */
#define ALG_MODEL_QUADROTOR 3           /* src/dynamics/quadrotor.jl:3-206: n = 12 p, m = 4 p; per player [x(3) | MRP attitude (3) | v(3) | omega(3)],
                                           rotor commands w1..w4; mass 0.5 (alg_set_quadrotor), J = diag(0.0023, 0.0023, 0.004), g = (0, 0, -9.81),
                                           motor_dist 0.175, kf 1.245, km 1.0 (the constructor's values) */
#define ALG_MAX_WALLS 8
#define ALG_MAX_CIRCLES 8

/* which trajectory buffer of the problem (problem.jl:27-29) */
#define ALG_TRAJ_PD 0      /* prob.pdtraj        */
#define ALG_TRAJ_TRIAL 1   /* prob.pdtraj_trial  */
#define ALG_TRAJ_DELTA 2   /* prob.Δpdtraj (x_1 slot is zero) */

/* per-game status */
#define ALG_STATUS_OK 0
#define ALG_STATUS_SINGULAR 1   /* zero / non-finite pivot in the Newton solve (reference: SingularException) */
#define ALG_STATUS_NAN 2        /* non-finite residual */
#define ALG_STATUS_PARKED 3     /* transient: the game used up the hand-off budget of the first launch and waits for the second (alg_set_handoff);
                                   never visible after alg_newton_solve / alg_synchronize */

typedef struct alg_handle alg_handle;

/* ProblemSize + model + dt (src/struct/problem_size.jl:18-35, problem.jl:35-53) */
typedef struct alg_desc {
    int32_t model;   /* ALG_MODEL_*                                           */
    int32_t p;       /* number of players                                     */
    int32_t d;       /* integrator dimension (DoubleIntegrator; unicycle: 2)  */
    int32_t N;       /* knot points                                           */
    double  dt;      /* step                                                  */
    int32_t batch;   /* number of games B owned by this handle                */
    int32_t device;  /* HIP device ordinal (ignored by the CPU oracle)        */
} alg_desc;

/* POD mirror of the `Options` fields read on the hot path (src/struct/options.jl:5-116). */
typedef struct alg_options {
    double  amplitude_init;  /* 1e-8  */
    int32_t shift;           /* 2^10  */
    int32_t regularize;      /* true  */
    double  reg_0;           /* 1e-3  */
    double  alpha_decrease;  /* 0.5   */
    double  beta;            /* 0.01  */
    int32_t ls_iter;         /* 25    */
    int32_t dual_reset;      /* true  */
    double  delta_min;       /* 1e-9  */
    double  rho_0;           /* 1.0   */
    double  rho_increase;    /* 10.0  */
    double  rho_max;         /* 1e7   */
    double  lambda_max;      /* 1e7   */
    double  alpha_dual;      /* 1.0   */
    double  alphax_dual[10]; /* ones  */
    double  eps_dyn, eps_sta, eps_con, eps_opt; /* 1e-3 */
    int32_t outer_iter;      /* 7     */
    int32_t inner_iter;      /* 20    */
    int64_t seed;            /* 100   */
} alg_options;

/* One `Statistics` record (src/struct/statistics.jl:5-15,44-57): what record! pushes. */
typedef struct alg_record {
    int32_t outer;     /* stats.outer_iter[end]        */
    int32_t ls_j;      /* line-search count j of the step taken after this record (0 if none) */
    double  alpha;     /* step taken after this record (0 if none)                            */
    double  res;       /* ||res||_1 / S                */
    double  delta;     /* Δ_traj passed to record!     */
    double  dyn_vio, con_vio, sta_vio, opt_vio; /* the four .max scalars */
    double  t_elap;    /* stats.t_elap[end] (statistics.jl:8,34): seconds the previous inner_iteration of this solve took
                          (@elapsed at solver_methods.jl:40-42; 0 for the first record), measured on the device with the
                          100 MHz real-time counter from the first to the last instruction of the game's iteration */
} alg_record;

/* Result of newton_solve! for one game (src/problem/solver_methods.jl:5-65). */
typedef struct alg_game_stats {
    int32_t status;        /* ALG_STATUS_*                                              */
    int32_t outer_iters;   /* `out`                                                     */
    int32_t newton_iters;  /* inner iterations that performed a linear solve            */
    int32_t records;       /* stats.iter                                                */
    int32_t converged;     /* exit test solver_methods.jl:49-53 met (not the k==outer_iter arm) */
    int32_t ls_failures;   /* failed line searches                                      */
    int32_t refinements;   /* correction solves of the Newton direction's iterative refinement (alg_set_refinement; 0 for the CPU oracle, whose pivoted LU needs none) */
    int32_t reserved;      /* 0.  (Team kernels: counts line-search steps whose norm from the group pass differed from the ordinary pass's -- a self-check that must stay 0, tests/test_gpu_line_search_batch.py) */
    alg_record last;       /* final record! (solver_methods.jl:63)                      */
} alg_game_stats;

/* Result of one inner_iteration (src/problem/solver_methods.jl:67-103). */
typedef struct alg_step_info {
    int32_t status;
    int32_t control_flow;  /* 0 = :continue, 1 = :break                                 */
    int32_t ls_j;          /* j returned by line_search (0 if the step was skipped)     */
    int32_t ls_failed;     /* j == ls_iter                                              */
    double  alpha;
    double  delta;         /* Δ_step                                                    */
    alg_record rec;        /* the record! made at the top of the iteration              */
} alg_step_info;

const char* alg_last_error(void);
void alg_default_options(alg_options* o);                 /* Options() defaults, options.jl:5-116 */

/* sizes derived from a descriptor (problem_size.jl:18-35) */
int alg_dims(const alg_desc* d, int32_t* n, int32_t* m, int32_t* mi, int32_t* S,
             int32_t* traj_len, int32_t* con_len);

/* GameProblem(N, dt, x0, model, opts, game_obj, game_con)  (problem.jl:35-53) */
int  alg_create(const alg_desc* d, alg_handle** out);
void alg_destroy(alg_handle* h);
int  alg_set_options(alg_handle* h, const alg_options* o);   /* also set_constraint_params!, game_constraints.jl:33-53 */
int  alg_get_options(alg_handle* h, alg_options* o);
/* Kernel shape of the fused solver entry points (alg_newton_solve*, alg_mpc_solve): wavefronts that work on one game.
 * 1 = one game per wavefront (large batches: every SIMD holds several games); 2 / 4 = a team of wavefronts per game (small
 * batches that would leave most of the 1024 SIMDs empty: the streaming phases of the solver are spread over the team, the
 * serial Newton-direction sweeps stay on one wavefront); 0 (default) = automatic: a team kernel when one is compiled for the
 * configuration and batch x width <= 2048 wavefronts.  Results agree with the one-wavefront kernel to rounding (the norms are
 * summed in a different order).  alg_get_waves_per_game returns the width the next solve will use. */
int  alg_set_waves_per_game(alg_handle* h, int32_t waves);
int  alg_get_waves_per_game(alg_handle* h, int32_t* waves);
/* Line search (solver_methods.jl:105-125) of the team kernels and the one-wavefront unicycle kernels: once the first step size has been
 * rejected the following ones are evaluated four at a time by a norm-only pass (bit-identical norms, the same step is accepted).
 * on = 0 selects the one-by-one search in the same binary (default 1).  Nothing else changes at the boundary. */
int  alg_set_line_search_groups(alg_handle* h, int32_t on);
int  alg_get_line_search_groups(alg_handle* h, int32_t* on);
/* Straggler hand-off for heterogeneous batches (no reference counterpart: the reference solves one game at a time).  A launch lasts as
 * long as its slowest game.  With iters = K > 0 the one-wavefront solver kernel behind alg_newton_solve* gives every game a budget of
 * K inner iterations BEGUN (solver_methods.jl:38: each makes a record!, whether or not it reaches the linear solve -- a game that converges
 * in 11 Newton iterations over 4 outer iterations begins 15); a game that needs more parks -- its whole state lives in its arena chunk -- and a second launch on the same
 * stream finishes the parked games with the team kernel (four wavefronts per game), which continues the same outer / inner loops.
 * Results per game: the iterations before the hand-off are the one-wavefront kernel's, the ones after it the team kernel's (the two
 * agree to rounding: the norms are summed in a different order, see alg_set_waves_per_game).  0 (default) = off.  Only configurations
 * with a team kernel accept K > 0 (3-player DoubleIntegrator d = 2, 3- / 4-player Unicycle, base constraint set -- with per-game scenario
 * data only in ALG_SCEN_KERNELS_BASE mode, alg_set_scenario_kernels; ALG_ERR_ARG
 * otherwise); the setting is ignored while the handle runs a team kernel itself and by alg_mpc_solve.  alg_get_handoff also returns
 * the number of games the most recent solve handed over (parked_last may be NULL). */
int  alg_set_handoff(alg_handle* h, int32_t iters);
int  alg_get_handoff(alg_handle* h, int32_t* iters, int32_t* parked_last);
/* Iterative refinement of the Newton direction (replaces the backward stability of `lu(core.jac) \\ core.res`, solver_methods.jl:87).
 * The structured elimination behind alg_newton_direction / alg_newton_step / alg_newton_solve* is a block LU without pivoting across
 * blocks; the forward and costate sweeps satisfy the dynamics and opt-x rows of J d = -res by construction, so all of the elimination's
 * error surfaces in the opt-u rows, which are evaluated after every solve (the gate).  While their row-wise backward error
 * max_c |rho_c| / (|J_c| |d| + |res_c|) exceeds `tol`, the direction is corrected by one more elimination on the residual (at most
 * `max_steps` correction solves per direction).  `tol` is the tolerance for games whose largest constraint penalty (ALConVal mu) has
 * reached `mu_tight`; below that it is relaxed in proportion mu_tight / mu_max, at most 256 x (a forward-error target needs a backward
 * error of target / cond(J), and cond(J) grows with the penalties).  The dense-direction configurations (Quadrotor, n > 16) use
 * tol / 128 without relaxation.  Within 2^10 of the tolerance a correction that does not at least halve max |rho| ends the refinement.
 * Defaults: max_steps = 2 (dense-direction configurations: 8), tol = 2^-34, mu_tight = 1.6e5;
 * max_steps = 0 switches gate and refinement off (the round-3 arithmetic).  alg_game_stats.refinements counts the correction
 * solves of a newton_solve!.  A correction solve uses the trial trajectory (ALG_TRAJ_TRIAL) as its output buffer: after
 * alg_newton_direction that buffer holds the last correction (x_1 restored), until the next line search rewrites it -- as in
 * the reference, pdtraj_trial is only meaningful between a line search and the update that follows it. */
int  alg_set_refinement(alg_handle* h, int32_t max_steps, double tol, double mu_tight);
int  alg_get_refinement(alg_handle* h, int32_t* max_steps, double* tol, double* mu_tight);
/* Inspection: the gate statistics of the most recent Newton direction of every game, before any correction; out is B x 3:
 * [ max |rho| over the opt-u rows, row-wise backward error max |rho_c| / (|J_c| |d| + |ru_c|), largest row scale ].
 * Not refreshed while the gate is off (max_steps = 0); zeros for the CPU oracle. */
int  alg_get_direction_gate(alg_handle* h, double* out);
/* Launch on a caller-provided hipStream_t (e.g. torch's current stream); NULL = library stream. */
int  alg_set_stream(alg_handle* h, void* hip_stream);

/* x0: B x n */
int alg_set_x0(alg_handle* h, const double* x0);
/* GameObjective(Q,R,xf,uf,N,model) (objective.jl:12-35): diagonals on the player's own indices.
 * Qdiag, xf: [B x] p x ni ; Rdiag, uf: [B x] p x mi.  per_game=0: one set shared by all games. */
int alg_set_lqr(alg_handle* h, const double* Qdiag, const double* Rdiag, const double* xf,
                const double* uf, int32_t per_game);
/* add_collision_cost!(game_obj, radius, mu) (objective.jl:84-100); NULL,NULL removes it. */
int alg_add_collision_cost(alg_handle* h, const double* radius /*p*/, const double* mu /*p*/);
/* add_collision_avoidance!(game_con, radius::Vector) (constraints_methods.jl:21-33) */
int alg_add_collision_avoidance(alg_handle* h, const double* radius /*p*/);
/* add_collision_avoidance!(game_con, i, j, radius) (constraints_methods.jl:5-19) and
 * add_spherical_collision_avoidance!(game_con, i, j, radius) (:45-64): ONE CollisionConstraint of player i against player j
 * (0-based) with its own radius -- asymmetric radii or a subset of the ordered pairs.  The multiplier / value rows keep the
 * all-pairs layout [pair q = i (p-1) + (j < i ? j : j-1)][knot]; a pair that was never added is inert (c = 0, zero Jacobian,
 * multiplier stays 0).  The first pair call on a handle starts from "no pair"; the vector forms (alg_add_collision_avoidance,
 * alg_add_spherical_collision_avoidance) set every ordered pair to r_i + r_j.  One constraint per ordered pair. */
int alg_add_collision_avoidance_pair(alg_handle* h, int32_t i, int32_t j, double radius);
int alg_add_spherical_collision_avoidance_pair(alg_handle* h, int32_t i, int32_t j, double radius);
/* add_control_bound!(game_con, u_max, u_min) (constraints_methods.jl:104-115); +-inf allowed */
int alg_add_control_bound(alg_handle* h, const double* u_max /*m*/, const double* u_min /*m*/);

/* Every adder of the extended set below (state bounds, walls, circles, and the 3-D set incl. spherical collision avoidance)
 * re-creates the handle's multiplier storage: all lambda = 0, all mu = the current opts.rho_0 -- like freshly built ALConVals
 * (it matters only when the first solve runs with dual_reset = false). */
/* BicycleGame(p; lf, lr) parameters (bicycle.jl:15); only for ALG_MODEL_BICYCLE */
int alg_set_bicycle(alg_handle* h, double lf, double lr);
/* QuadrotorGame(; p, mass) (quadrotor.jl:20-46): the constructor's one parameter (default 0.5 kg; inertia, gravity, motor_dist, kf, km are
 * fixed there); only for ALG_MODEL_QUADROTOR */
int alg_set_quadrotor(alg_handle* h, double mass);
/* add_state_bound!(game_con, i, x_max, x_min) (constraints_methods.jl:86-98; state_bound_constraint.jl): bounds on the joint
 * state (n each, +-inf allowed) attached to player `player` (0-based), knots 2..N */
int alg_add_state_bound(alg_handle* h, int32_t player, const double* x_max /*n*/, const double* x_min /*n*/);
/* add_wall_constraint!(game_con, walls) (constraints_methods.jl:152-195; wall_constraint.jl:30-96): every player, knots 2..N;
 * wall w: segment (x1,y1)-(x2,y2), normal (xv,yv) pointing into the forbidden half space */
int alg_add_wall_constraint(alg_handle* h, int32_t n_wall, const double* x1, const double* y1, const double* x2,
                            const double* y2, const double* xv, const double* yv);
/* add_circle_constraint!(game_con, xc, yc, radius) (constraints_methods.jl:120-148; TrajOpt CircleConstraint): every player */
int alg_add_circle_constraint(alg_handle* h, int32_t n_circle, const double* xc, const double* yc, const double* radius);
/* Per-player variants: add_wall_constraint!(game_con, i, walls) (constraints_methods.jl:161-187) and
 * add_circle_constraint!(game_con, i, xc, yc, radius) (:121-139).  The walls / circles join the handle's table (at most
 * ALG_MAX_WALLS / ALG_MAX_CIRCLES distinct entries; an entry that is already there is shared) and constrain player `player`
 * (0-based) only.  The constraint rows keep the layout [player][knot][table entry]: the rows of entries that do not constrain
 * a player exist but are inert (value 0, multiplier 0).  The all-player calls above replace the table. */
int alg_add_wall_constraint_player(alg_handle* h, int32_t player, int32_t n_wall, const double* x1, const double* y1,
                                   const double* x2, const double* y2, const double* xv, const double* yv);
int alg_add_circle_constraint_player(alg_handle* h, int32_t player, int32_t n_circle, const double* xc, const double* yc,
                                     const double* radius);
/* ---- 3-D half of the constraint set.  The reference addresses pz[i][1:3] (constraints_methods.jl:52-53,231-236,275): the
 * first three state entries of player i, which are its x, y, z positions for DoubleIntegratorGame(d = 3) -- the only model
 * these three calls accept (ALG_ERR_ARG otherwise). */
/* add_spherical_collision_avoidance!(game_con, radius) (constraints_methods.jl:45-81): as alg_add_collision_avoidance with the
 * 3-D distance; replaces a previously added planar collision avoidance (they share the constraint rows) */
int alg_add_spherical_collision_avoidance(alg_handle* h, const double* radius /*p*/);
/* add_wall_constraint!(game_con, walls::Vector{Wall3D}) (constraints_methods.jl:201-242; wall_constraint.jl:127-236): every
 * player, knots 2..N; wall w = parallelogram corner points p1, p2, p3 and normal v into the forbidden half space (n_wall x 3 each) */
int alg_add_wall3d_constraint(alg_handle* h, int32_t n_wall, const double* p1, const double* p2, const double* p3, const double* v);
/* add_wall_constraint!(game_con, walls::Vector{CylinderWall}) (constraints_methods.jl:249-284; cylinder_constraint.jl:35-127):
 * axis-aligned cylinders, origin p (n_cyl x 3), axis 0/1/2 = :x/:y/:z, length l, radius r; every player, knots 2..N */
int alg_add_cylinder_constraint(alg_handle* h, int32_t n_cyl, const double* p, const int32_t* axis, const double* l, const double* r);
/* add_wall_constraint!(game_con, i, walls::Vector{Wall3D}) (constraints_methods.jl:208-247) and
 * add_wall_constraint!(game_con, i, walls::Vector{CylinderWall}) (:256-299): the constraint joins state_conlist[i] of ONE player
 * (0-based here).  Same mechanism as the planar *_player adders: the entries join the handle's table of distinct 3-D walls /
 * cylinders (at most ALG_MAX_WALLS / ALG_MAX_CIRCLES; an identical entry is shared, row w of the ABI's block is table entry w for
 * every player) and a per-player mask says whom an entry constrains; a row whose bit is clear is inert (value 0, zero Jacobian,
 * multiplier untouched).  Can be called repeatedly; after an all-player set the masks become explicit first. */
int alg_add_wall3d_constraint_player(alg_handle* h, int32_t player, int32_t n_wall, const double* p1, const double* p2, const double* p3, const double* v);
int alg_add_cylinder_constraint_player(alg_handle* h, int32_t player, int32_t n_cyl, const double* p, const int32_t* axis, const double* l, const double* r);
/* current length of the constraint dual / penalty / value vectors of one game */
int alg_get_con_len(alg_handle* h, int32_t* con_len);

/* ---- per-game scenario data: the constraint and collision-cost NUMBERS may differ between the games of one handle.
 * What stays handle-wide is the structure the adders above set: which kinds exist, how many walls / circles / 3-D walls /
 * cylinders and pairs there are, the per-player masks, the cylinder axes and the +-inf pattern of the bounds (it decides the
 * rows that count).  data is B x len, game-major; len = alg_scenario_data_len(kind).
 *   - ALG_ERR_STATE if the kind was not added; ALG_ERR_ARG (nothing changes) if for any game: a value is non-finite where the
 *     handle's is finite, the +-inf pattern of a bound differs from the handle's, u_max < u_min or x_max < x_min, or a radius
 *     is <= 0 on a pair that exists, a circle or a cylinder.
 *   - per-game data runs on the EXT kernel instantiations unless alg_set_scenario_kernels (below) says otherwise.  The first call on a handle that is not EXT yet switches it, which
 *     re-creates the multipliers like every extended adder (lambda = 0, mu = rho_0); a configuration without an EXT
 *     instantiation (DoubleIntegrator d = 1) gets ALG_ERR_ARG.  Later calls only upload values and leave lambda and mu alone
 *     (an MPC caller may move obstacles between solves and keep the warm start).
 *   - any later adder (alg_add_*) drops ALL per-game data of the handle: the games share the handle's values again.
 *   - every entry point honours it: solves, the EXT team kernels (dense-direction configurations), the step-wise calls, IBR and
 *     alg_mpc_solve.  The tile-path team kernels exist for the base instantiations only, so a tile-path handle with per-game
 *     data runs the one-wavefront EXT kernels (e.g. the three-player double integrator at 64 MPC seeds) -- in the default mode;
 *     ALG_SCEN_KERNELS_BASE keeps teams and hand-off. */
#define ALG_SCEN_COLLISION_RADIUS 0  /* p*p: [i*p+j] = radius of ordered pair (i,j); diagonal and pairs never added are ignored */
#define ALG_SCEN_COLLISION_COST   1  /* 2p: radius (p) | mu (p)                                                            */
#define ALG_SCEN_CONTROL_BOUND    2  /* 2m: u_max (m) | u_min (m)                                                          */
#define ALG_SCEN_STATE_BOUND      3  /* 2pn: x_max (p x n) | x_min (p x n), the extc order                                 */
#define ALG_SCEN_WALL             4  /* 6 per table entry: x1 y1 x2 y2 xv yv                                               */
#define ALG_SCEN_CIRCLE           5  /* 3 per table entry: xc yc r                                                         */
#define ALG_SCEN_WALL3D           6  /* 12 per table entry: p1 p2 p3 v                                                     */
#define ALG_SCEN_CYLINDER         7  /* 5 per table entry: p (3) l r   (the axis stays handle-wide)                        */
int alg_scenario_data_len(alg_handle* h, int32_t kind, int32_t* len);     /* doubles per game; 0 if the kind was not added */
int alg_set_scenario_data(alg_handle* h, int32_t kind, const double* data /* B x len, or NULL = back to the shared values */);
int alg_get_scenario_data(alg_handle* h, int32_t kind, double* data /* B x len; the shared values repeated if not per game */);
/* Which kernels per-game data of the BASE kinds (0 .. 2: pair radii, collision cost, control bounds) runs on.
 *   ALG_SCEN_KERNELS_EXT (default): as described above -- the first alg_set_scenario_data call switches the handle to the EXT
 *     instantiations and re-creates lambda and mu.
 *   ALG_SCEN_KERNELS_BASE: a handle that carries only the base constraint set stays on the base kernels.  alg_set_scenario_data of
 *     kinds 0 .. 2 validates and uploads as above and touches nothing else: lambda, mu and alg_get_con_len stay as they are, on the
 *     first call as on later ones.  While any kind is per game the handle runs the twins of its base kernels that read the five
 *     numbers from the game's block (same constraint set, fused trial pass, LDS layout and register budget per lane), so the
 *     tile-path team kernels (automatic at B x W <= 2048, alg_set_waves_per_game), the straggler hand-off (a budget set before or
 *     after the data stays in force, alg_get_handoff reports the parked games), the step-wise calls, IBR and alg_mpc_solve all
 *     honour the per-game numbers.  With equal numbers in every block the results are bit-identical to the base kernels'.  Once the
 *     last kind went back to shared (data = NULL), or an adder dropped the per-game data, the handle runs the base kernels again.
 *     An adder of the extended set switches to EXT exactly as in the default mode (per-game data dropped, multipliers re-created).
 * The setting can change only while the handle carries no per-game data (ALG_ERR_STATE otherwise; nothing changes).
 * ALG_SCEN_KERNELS_BASE on a configuration without such kernels (DoubleIntegrator d = 1, the dense-direction configurations: p >= 5,
 * d = 3 with p != 2, Quadrotor) gets ALG_ERR_ARG and the handle keeps the default; a handle that already is EXT (bicycle, extended
 * constraints) accepts the call and ignores the setting.  in_use (may be NULL): the kernels the next launch takes -- 0 base,
 * 1 EXT, 2 base kernels reading per-game blocks. */
#define ALG_SCEN_KERNELS_EXT  0
#define ALG_SCEN_KERNELS_BASE 1
int alg_set_scenario_kernels(alg_handle* h, int32_t which);
int alg_get_scenario_kernels(alg_handle* h, int32_t* which, int32_t* in_use);

/* set_traj!/get_traj! (primal_dual_traj.jl:46-107) over the batch: B x traj_len.
 * (ALG_TRAJ_TRIAL after a solve: x_1 = x0; the rest is the library's scratch -- the line search accepts a trial by exchanging buffer
 * offsets, a solve that ends on the exchanged side copies pdtraj home: the trial buffer then holds pdtraj as in the reference, otherwise the iterate before it) */
int alg_set_traj(alg_handle* h, int32_t which, const double* z);
int alg_get_traj(alg_handle* h, int32_t which, double* z);
/* ALConVal lambda / mu (Altro 0.3.0): B x con_len each; NULL pointers are skipped */
int alg_set_con_duals(alg_handle* h, const double* lambda, const double* mu);
int alg_get_con_duals(alg_handle* h, double* lambda, double* mu);

/* init_traj! + rollout!(RK3) (solver_methods.jl:12-18, primal_dual_traj.jl:29-44).
 * f_init = rand is replaced by a counter-based generator (SplitMix64 keyed by seed, global game id
 * game_id0+g, element counter) because Julia's MersenneTwister stream cannot be reproduced
 * (SURVEY.md section 7 "hard parts").  use_shift!=0 applies the `shift` warm start to the stored pdtraj.
 * Any other `opts.f_init` (options.jl:11: zeros, randn, a closure) is a host-side matter: the caller makes the
 * guess (Julia shim: the reference's own init_traj!; Python: host.init_traj_host), stores it with alg_set_traj and
 * solves with init = 0 -- the states are rolled out either way (solver_methods.jl:17). */
int alg_init_traj(alg_handle* h, int64_t game_id0, int32_t use_shift);
/* rollout!(RK3, model, pdtraj.pr) only (keeps controls/duals as set by alg_set_traj). */
int alg_rollout(alg_handle* h, int32_t which);

/* residual! + regularize_residual! (global_quantities.jl:9-86).  `which` selects the iterate;
 * the proximal term is taken w.r.t. pdtraj with reg = reg_x = reg_u (0 disables).
 * res (B x S, vertical order) and res_norm (B, ||res||_1/S) may each be NULL. */
int alg_residual(alg_handle* h, int32_t which, double reg, double* res, double* res_norm);
/* residual_jacobian! + regularize_residual_jacobian! (global_quantities.jl:109-193) at pdtraj:
 * jac is B x S x S dense column-major (parity / inspection entry point; the solver itself never
 * materialises it). */
int alg_residual_jacobian(alg_handle* h, double reg, double* jac);
/* The same for games first_game .. first_game + n_games - 1 only: jac is n_games x S x S.  The active-set inspection
 * (active_set_methods.jl:127-170 works on ONE problem) uses this so that looking at one game of a large batch does not
 * materialise B dense Jacobians. */
int alg_residual_jacobian_games(alg_handle* h, double reg, int32_t first_game, int32_t n_games, double* jac);
/* Frees the device scratch the inspection entry points (dense Jacobians, MPC state logs) grow on demand.  The solver never
 * uses that buffer; the next inspection call allocates it again. */
int alg_release_scratch(alg_handle* h);
/* Per-knot violation profiles at pdtraj: the .vio vectors the reference's violation objects carry next to .max
 * (violations.jl:5-26 dynamics, :41-67 control, :86-114 state, :140-168 optimality).  dyn, con: B x (N-1) (steps 1..N-1);
 * sta, opt: B x N (knots 1..N; sta[0] is 0: no state constraint acts on x_1).  Any pointer may be NULL.  Evaluated on the device
 * from the residual and the constraint values at the current pdtraj (one assemble pass + one reduction kernel). */
int alg_get_violation_profile(alg_handle* h, double* dyn, double* con, double* sta, double* opt);
/* What the plan costs each player: the values of the GameObjective whose gradients the solver assembles -- LQRCost (objective.jl:12-35)
 * and CollisionCost, TrajectoryOptimization.stage_cost(::CollisionCost, x) (objective.jl:122-131).  The objective itself: constraints,
 * multipliers and penalties do not enter.  Player i of one game:
 *   J_i = sum_{k=1..N} w_k l_i(x_k, u_k),  w_k = dt for k < N, w_N = 1 (the weights of the cost gradients), l_i in three components:
 *     state      1/2 sum_a Q_i[a] (x[pz_i[a]] - xf_i[a])^2 over the player's own ni state entries (alg_set_lqr layout); every knot, x_1 included
 *     control    1/2 sum_a R_i[a] (u[pu_i[a]] - uf_i[a])^2; 0 at k = N
 *     collision  sum_{j != i} 1/2 mu_i max(0, r_i - |px_i - px_j|)^2 with the two position entries and the (mu_i, r_i) the collision-cost
 *                gradient uses -- the handle's values or the game's scenario block, in both alg_set_scenario_kernels modes; the planar
 *                distance for every model; 0 without alg_add_collision_cost
 * which: ALG_TRAJ_PD or ALG_TRAJ_TRIAL.  total: B x p x 3 [state, control, collision]; stage: B x N x p x 3, knot-major within a game, the
 * summands w_k l_i (they add up to total to rounding); either may be NULL, not both.
 * One launch, one wavefront per game whatever kernels the handle solves with; a game's numbers do not depend on the batch size or on its
 * place in the batch, bit for bit.  Non-finite input gives non-finite output for that game only; no status is set.
 * ALG_ERR_ARG, with nothing changed, for a null handle, another `which` or two null outputs; ALG_ERR_STATE if alg_set_lqr was not called.
 * The call changes nothing on the handle: trajectories, multipliers, statistics, history, profiles, step records and the direction-gate
 * figures stay as they are.  Uses the inspection scratch (alg_release_scratch). */
int alg_get_cost(alg_handle* h, int32_t which /* ALG_TRAJ_PD | ALG_TRAJ_TRIAL */, double* total /* B x p x 3, or NULL */, double* stage /* B x N x p x 3, or NULL */);
/* The constraint values of the plan, read-only: evaluate!(game_con, traj) (constraints_methods.jl:329-379) at ALG_TRAJ_PD or ALG_TRAJ_TRIAL,
 * without the dual and penalty update alg_dual_penalty_update performs with it.  vals: B x alg_get_con_len, the constraint layout at the top
 * of this file, row semantics of alg_dual_penalty_update's vals: c <= 0 is feasible, a row of an infinite bound reports -inf, an inert row
 * (a pair never added, a table entry whose player bit is clear) 0.
 * THE KNOT LAYOUT.  Every block of the constraint vector is per step, so con_len = (N - 1) * K1 with K1 = alg_con_knot_len the rows of
 * one step; step k pairs the control u_k with the state x_{k+1} it reaches.  One step's rows, in the ABI's order within each block:
 *   [ collision pair q = 0 .. p(p-1)-1 | u - u_max (m) | u_min - u (m) | per player i: state bound (x - x_max)(n), (x_min - x)(n)
 *     | per player i: walls | per player i: circles | per player i: 3-D walls | per player i: cylinders ]
 * with the blocks alg_get_con_len counts: the two base blocks always (a base block that was not added reports 0), the others once added.
 * The kinds of rows, in layout order: */
#define ALG_CON_COLLISION 0
#define ALG_CON_CONTROL   1
#define ALG_CON_STATE     2
#define ALG_CON_WALL      3
#define ALG_CON_CIRCLE    4
#define ALG_CON_WALL3D    5
#define ALG_CON_CYLINDER  6
#define ALG_CON_KINDS     7
/* The numbers are the handle's or the game's scenario block, in both alg_set_scenario_kernels modes.  One launch, one wavefront per game
 * whatever kernels the handle solves with; a game's rows do not depend on the batch size or on its place in the batch, bit for bit.
 * Non-finite input gives non-finite rows for that game only; no status is set.
 * ALG_ERR_ARG, with nothing changed, for a null handle, a null vals or another `which`; ALG_ERR_STATE if alg_set_x0 was not called.
 * The call changes nothing on the handle: trajectories, multipliers, penalties, the stored constraint values, statistics, history, profiles,
 * step records and the direction-gate figures stay as they are.  Uses the inspection scratch (alg_release_scratch). */
int alg_get_con_values(alg_handle* h, int32_t which /* ALG_TRAJ_PD | ALG_TRAJ_TRIAL */, double* vals /* B x con_len */);
int alg_con_knot_len(alg_handle* h, int32_t* len /* K1 = con_len / (N - 1) */);
/* Δtraj = -lu(jac) \ res ; set_traj!(Δpdtraj, Δtraj) (solver_methods.jl:87-88).  delta: B x S or NULL. */
int alg_newton_direction(alg_handle* h, double reg, double* delta, int32_t* status /*B or NULL*/);
/* KKT solves with many right-hand sides at the current iterate: J X = R with J the (regularised) residual Jacobian of
 * alg_residual_jacobian(reg) at pdtraj, solved on the device by the structured elimination of alg_newton_direction, refinement
 * gate included (alg_set_refinement); one launch, one assemble pass per game, one elimination per column.
 *   kind = ALG_KKT_RHS_USER: rhs holds n_games x nrhs columns of S doubles in the VERTICAL order of alg_residual; nrhs >= 1.
 *                            rhs = -res gives the Newton direction.
 *   kind = ALG_KKT_RHS_X0:   R = -d res / d x_1 (x_1 = the initial state x0), n columns: X = d z* / d x0, the sensitivity of the root
 *                            of res(z; x0) = 0 to the initial state.
 *   kind = ALG_KKT_RHS_XF:   R = -d res / d x_f, p ni columns in the xf order of alg_set_lqr: X = d z* / d x_f.
 *   For X0 / XF rhs must be NULL and nrhs the full count or 0 ("all").
 * The derivatives hold the multipliers and penalties (and the active sets behind them) fixed.  J is the reference's Jacobian
 * (global_quantities.jl:109-193), which drops the second-order terms of the dynamics: the sensitivities are exact for the
 * DoubleIntegrator (linear dynamics) and Gauss-Newton sensitivities for the other models.  reg != 0 solves the regularised system.
 * out: n_games x nrhs x S, every column in the HORIZONTAL order of alg_newton_direction's delta.  status: n_games entries or NULL, per
 * game the first status other than ALG_STATUS_OK among its columns.
 * ALG_ERR_ARG, with nothing changed, for an unknown kind, a bad count, a null or non-finite rhs (USER), a non-null rhs (X0 / XF), a
 * null out, or a game range outside the batch.
 * What the call leaves behind: pdtraj, x0, multipliers, penalties, statistics (`refinements` included) and the history are untouched;
 * ALG_TRAJ_DELTA of every game in the range holds its last column; ALG_TRAJ_TRIAL is scratch (x_1 restored); the
 * step records and the direction-gate figures (alg_get_direction_gate) are rewritten -- every solver entry point reassembles the records
 * before it reads them.  Uses the inspection scratch (alg_release_scratch). */
#define ALG_KKT_RHS_USER 0
#define ALG_KKT_RHS_X0   1
#define ALG_KKT_RHS_XF   2
int alg_kkt_solve(alg_handle* h, double reg, int32_t kind, int32_t nrhs, const double* rhs /* n_games x nrhs x S, vertical order; NULL unless USER */,
                  int32_t first_game, int32_t n_games, double* out /* n_games x nrhs x S, horizontal order */, int32_t* status /* n_games or NULL */);
/* Equilibrium sensitivities to objective and constraint parameters: X = -J^-1 d res / d theta at pdtraj, with J, reg, the refinement gate and
 * the per-game status rule of alg_kkt_solve, and the right-hand sides R = -d res / d theta built on the device: evaluated at pdtraj with the
 * game's multipliers and penalties (and the active sets behind them) held, from the numbers the game was assembled with -- per-game LQR data
 * (alg_set_lqr(per_game = 1)), the game's scenario block in both alg_set_scenario_kernels modes, else the handle's values.
 *   theta = one of the parameter vectors below, `len` = alg_param_len entries in the order of the setter named there.
 *   dirs == NULL (ndir must be 0): the len unit columns, ncol = len.
 *   dirs != NULL (ndir >= 1):      column c of game g is the directional derivative X v for v = dirs[g][c] (len finite doubles): one
 *                                  elimination per direction whatever len is; ncol = ndir.
 *   Only the rows of steps first_step .. first_step + n_steps - 1 (0-based, n_steps = 0 with first_step = 0: all N - 1) are stored and copied
 *   back: a step's block is b = n + m + n p doubles of the horizontal order (x_{k+1}, u_{.,k}, lambda_{.,k}), out is n_games x ncol x (n_steps b).
 *   The device scratch and the download are sized by the slice.
 * Columns of a parameter that does not enter the residual are exactly zero with status OK: a diagonal entry of the pair table, a pair that
 * was never added, a bound that is +-inf, a row outside its active set (a = (c >= 0) | (lambda > 0) is 0).  The collision cost enters through
 * the pairs with r_i - |d| > 0 only.
 * ALG_ERR_ARG, with nothing changed, for a null handle, an unknown param, ndir and dirs that disagree, non-finite dirs, a game range or step
 * range outside the problem, or a null out; ALG_ERR_STATE, with nothing changed, if the parameter's ingredient is not on the handle (no
 * alg_set_lqr for XF / Q / R / UF; no collision cost, collision avoidance or control bound for the last three).
 * What the call leaves behind is what alg_kkt_solve leaves behind: pdtraj, x0, multipliers, penalties, statistics, history and profiles are
 * untouched; ALG_TRAJ_DELTA holds the last column (all steps of it); ALG_TRAJ_TRIAL is scratch (x_1 restored).  Uses the inspection scratch. */
#define ALG_PARAM_X0               0   /* n            : x_1                                            */
#define ALG_PARAM_XF               1   /* p*ni         : xf order of alg_set_lqr                        */
#define ALG_PARAM_Q                2   /* p*ni         : Qdiag order of alg_set_lqr                     */
#define ALG_PARAM_R                3   /* p*mi         : Rdiag order                                    */
#define ALG_PARAM_UF               4   /* p*mi         : uf order                                       */
#define ALG_PARAM_COLLISION_COST   5   /* 2p           : radius (p) | mu (p), ALG_SCEN_COLLISION_COST   */
#define ALG_PARAM_COLLISION_RADIUS 6   /* p*p          : ordered pairs, ALG_SCEN_COLLISION_RADIUS       */
#define ALG_PARAM_CONTROL_BOUND    7   /* 2m           : u_max (m) | u_min (m), ALG_SCEN_CONTROL_BOUND  */
int alg_param_len(alg_handle* h, int32_t param, int32_t* len);
int alg_kkt_sensitivity(alg_handle* h, double reg, int32_t param,
                        int32_t ndir, const double* dirs /* n_games x ndir x len, or NULL */,
                        int32_t first_game, int32_t n_games,
                        int32_t first_step, int32_t n_steps /* 0 = all N-1 */,
                        double* out /* n_games x ncol x (n_steps*b) */, int32_t* status /* n_games or NULL */);
/* The normal equations of fitting parameters to an observed trajectory, reduced on the device: per game, with X_c = d z* / d theta of entry
 * col_index[c] of parameter col_param[c] -- exactly the unit column alg_kkt_sensitivity returns for it (same J, reg, refinement gate and
 * status rule; multipliers, penalties and active sets held) -- and r_e = z_e - target_e over the S entries of pdtraj behind x_1,
 *   loss = 1/2 sum_e w_e r_e^2,   g_c = sum_e w_e X_ec r_e,   H_cd = sum_e w_e X_ec X_ed       (gradient and Gauss-Newton matrix of loss).
 * Columns may mix parameter kinds in any order; the outputs follow the caller's order.  H comes back with both triangles, the lower a copy of
 * the upper: symmetric bit for bit.  Every entry is one sum over e = 0, 1, ... in a fixed order inside one wavefront: results are
 * bit-reproducible and do not depend on the game's place in the batch or in the range.  No column leaves the device: the download is H, g,
 * loss and status.  status: per game the first status other than ALG_STATUS_OK among its columns, kinds in the order they first appear; a
 * game whose status is not OK gets whatever the arithmetic gives in H, g and loss.
 * ALG_ERR_ARG, with nothing changed, for a null handle, ncol < 1 or > ALG_NORMAL_MAX_COLS, an unknown kind, an index outside
 * 0 .. alg_param_len(param) - 1, a (param, index) pair named twice, a null col_param, col_index, target, weight, H, g or loss, a non-finite
 * target, a weight that is non-finite or negative, or a game range outside the batch; ALG_ERR_STATE, with nothing changed, where
 * alg_kkt_sensitivity returns it (the ingredient of one of the kinds is not on the handle); the counts, pointers, ranges and columns are
 * checked first, then the handle's ingredients, and only then are target and weight read.
 * What the call leaves behind is what alg_kkt_sensitivity leaves behind: pdtraj, x0, multipliers, penalties, statistics, history and profiles
 * are untouched; ALG_TRAJ_DELTA holds the last column solved; ALG_TRAJ_TRIAL is scratch (x_1 restored).  Uses the inspection scratch:
 * n_games x ncol x S doubles of columns, per kind n_games x (its columns) x alg_param_len doubles of unit directions, and target, weight
 * and the results -- cut the game range to bound it. */
#define ALG_NORMAL_MAX_COLS 63
int alg_kkt_normal_equations(alg_handle* h, double reg,
                             int32_t ncol, const int32_t* col_param /* ncol x ALG_PARAM_* */, const int32_t* col_index /* ncol: 0 .. alg_param_len(param) - 1 */,
                             const double* target /* n_games x S, horizontal order (the order of alg_kkt_solve's out) */,
                             const double* weight /* S, or n_games x S when per_game_weight */, int32_t per_game_weight,
                             int32_t first_game, int32_t n_games,
                             double* H /* n_games x ncol x ncol */, double* g /* n_games x ncol */, double* loss /* n_games */,
                             int32_t* status /* n_games or NULL */);
/* line_search (solver_methods.jl:105-125) on the stored Δpdtraj. */
int alg_line_search(alg_handle* h, double reg, const double* res_norm /*B*/, double* alpha /*B*/,
                    int32_t* j /*B*/);
/* update_traj!(target, source, alpha, Δpdtraj) (primal_dual_traj.jl:109-128); alpha: B */
int alg_update_traj(alg_handle* h, int32_t target, int32_t source, const double* alpha);
/* record!'s scalars at pdtraj (statistics.jl:44-57, violations.jl) */
int alg_record_stats(alg_handle* h, alg_record* rec /*B*/);
/* reset!(game_con) (constraints_methods.jl:295-327) */
int alg_reset_con(alg_handle* h);
/* evaluate!(game_con, pdtraj.pr); dual_update!(game_con); penalty_update!(game_con)
 * (solver_methods.jl:57-61, constraints_methods.jl:329-379,421-440).  vals: B x con_len or NULL. */
int alg_dual_penalty_update(alg_handle* h, double* vals);

/* inner_iteration(prob, LS_count, t_elap, Δ, k, l) (solver_methods.jl:67-103) for every game;
 * reg is set to reg_0*l^4 as in solver_methods.jl:39.  delta_in (B or NULL = zeros) is the caller's Δ, which record! stores
 * in the Statistics record made at the top of the iteration (solver_methods.jl:75). */
int alg_newton_step(alg_handle* h, int32_t k_outer, int32_t l_inner, const double* delta_in /*B or NULL*/,
                    alg_step_info* info /*B*/);
/* newton_solve!(prob) (solver_methods.jl:5-65) for every game.  init!=0: run alg_init_traj first
 * (game ids game_id0+g); init==0: keep the stored controls/duals as the initial guess, still
 * rolling out the states (solver_methods.jl:17).  stats: B or NULL. */
int alg_newton_solve(alg_handle* h, int32_t init, int64_t game_id0, alg_game_stats* stats);
/* Same, asynchronous on the handle's stream: no host synchronisation, results stay on the device
 * until alg_get_stats().  Used by the benchmark so that HIP events bracket only device work. */
int alg_newton_solve_async(alg_handle* h, int32_t init, int64_t game_id0);
int alg_get_stats(alg_handle* h, alg_game_stats* stats /*B*/);
/* Statistics history of one game (statistics.jl:5-15): up to max_records; returns count in *n_out.
 * The history buffer is sized from the options (alg_set_options: outer_iter * inner_iter + 1 records per newton_solve!, never
 * fewer than ALG_HIST_MAX; the IBR entry points size it for ibr_iter * p solves) so that every record! of a solve is kept.
 * Only a request beyond 1 GiB of history for the whole batch is capped: alg_game_stats.records then exceeds *n_out (records
 * past the capacity are dropped, .last is always the final record) -- callers must treat n_out < records as truncation. */
#define ALG_HIST_MAX 192
int alg_get_history(alg_handle* h, int32_t game, int32_t max_records, alg_record* out, int32_t* n_out);
/* Per-record violation profiles: the .vio vectors the reference's record! pushes next to every .max (statistics.jl:44-57,
 * violations.jl:5-26, 41-67, 86-114, 140-168).  With max_records > 0 alg_newton_solve / alg_newton_solve_async also store, for every
 * record they push, the four vectors of alg_get_violation_profile at the iterate of that record: (N-1) + (N-1) + N + N doubles in that
 * call's layout (dyn, con: steps 1..N-1; sta, opt: knots 1..N, sta[0] = 0).  The buffer is an allocation of its own, B x max_records x
 * (4 N - 2) doubles; alg_record and the history buffer do not change.  Record r of a game goes to slot r while r < max_records; later
 * records are dropped, exactly as the history drops records past its capacity.  0 (default) = off: the buffer is freed and the solve runs
 * the kernels it always ran (with profiles on it runs their siblings, which add one phase behind every record!; results are bit-identical).
 * alg_set_history_profiles returns ALG_ERR_ARG, with a message and nothing changed, for a negative count, for a buffer beyond 1 GiB for
 * the batch, for a configuration without a sibling kernel (seven to ten players), and while a hand-off budget is set; alg_set_handoff(h,
 * K > 0) is refused in turn while profiles are on.
 * alg_get_history_vio: the profiles of one game.  dyn, con: n x (N-1); sta, opt: n x N, row-major, row r = record r of alg_get_history;
 * any pointer may be NULL; *n_out = n = min(records, capacity, max_records).  The profiles belong to the most recent alg_newton_solve /
 * alg_newton_solve_async: these two write them, every other entry point that pushes records (alg_newton_step, alg_record_stats,
 * alg_ibr_solve_player, alg_ibr_newton_solve, alg_mpc_solve, alg_mpc_solve_log) invalidates them -- *n_out = 0 until the next solve --
 * and alg_kkt_solve leaves them alone, as it leaves the history alone.  With profiles off: ALG_OK and *n_out = 0. */
int alg_set_history_profiles(alg_handle* h, int32_t max_records);
int alg_get_history_profiles(alg_handle* h, int32_t* max_records);
int alg_get_history_vio(alg_handle* h, int32_t game, int32_t max_records, double* dyn, double* con, double* sta, double* opt, int32_t* n_out);
int alg_synchronize(alg_handle* h);
/* Diagnostic (tests): every device allocation is followed by a 4 KiB guard zone and the per-game segments of the arenas are
 * padded to 128-byte lines; returns the number of guard zones / paddings a kernel has written to (0 = clean, <0 = error). */
int alg_debug_check_guards(alg_handle* h);

/* Iterated best response.
 * alg_ibr_solve_player: ibr_newton_solve!(prob, i) (solver_methods.jl:171-228) for every game, on the stored trajectory:
 *   player `player` (0-based) best-responds -- only x, u_player, lambda_player move (masks of newton_core.jl:205-294),
 *   residual norm over the player's rows + dynamics rows, player-specific violations (statistics.jl:59-73).
 *   Statistics accumulate (the reference does not reset them between players).
 * alg_ibr_newton_solve: ibr_newton_solve!(prob; ibr_opts) (solver_methods.jl:133-169): reset!(stats), init_traj! + rollout!,
 *   then up to ibr_iter sweeps over `ordering` (p 0-based player ids), leaving when no player changed
 *   (delta_min > maximum(stats.Δ_traj), literally as in the reference). init has the meaning of alg_newton_solve. */
int alg_ibr_solve_player(alg_handle* h, int32_t player, alg_game_stats* stats /*B or NULL*/);
int alg_ibr_newton_solve(alg_handle* h, int32_t init, int64_t game_id0, int32_t ibr_iter, const int32_t* ordering,
                         double delta_min, alg_game_stats* stats /*B or NULL*/);

/* Receding-horizon (MPC) support for BASELINE config 5.  The reference has no MPC loop, only the warm-start hooks
 * `opts.shift` (init_traj!, primal_dual_traj.jl:29-44) and `opts.dual_reset` (solver_methods.jl:25); the loop is
 * builder-defined: after a solve, x0 <- RK2(x_1, u_1) (the discretisation of
 * local_quantities.jl:13), then the next newton_solve! runs with shift = 1 and dual_reset = false.
 * alg_mpc_advance performs the x0 update for every game (asynchronously on the handle's stream) and adds the
 * finished solve's newton_iters / converged flag to per-game running totals. */
int alg_mpc_advance(alg_handle* h);
int alg_mpc_totals(alg_handle* h, int64_t* newton_iters /*B or NULL*/, int64_t* converged /*B or NULL*/, int32_t reset);
/* The whole loop in one launch: `steps` x (newton_solve! with init = 1 and game ids game_id0 + t*1000003 + g, then the
 * advance above); step 0 uses the handle's shift / dual_reset, later steps shift = 1 and dual_reset = false.  Every game
 * runs its own loop (one wavefront per game): games do not wait for each other between MPC steps.  Totals accumulate as
 * with alg_mpc_advance.  states: NULL (asynchronous launch) or host array (steps+1) x B x n receiving x0 before the loop
 * and after every step (synchronous). */
int alg_mpc_solve(alg_handle* h, int32_t steps, int64_t game_id0, double* states);
/* Schedules: values per game AND per MPC step of the numbers that may differ per game, applied inside alg_mpc_solve's single launch --
 * a goal that moves, an obstacle that follows a predicted path -- with the result the step-wise calls give (alg_set_scenario_data /
 * alg_set_lqr with the step's row, alg_newton_solve_async, alg_mpc_advance, once per step).
 *   kind: an ALG_SCEN_* value (len = alg_scenario_data_len(kind)), ALG_SCHED_LQR_TARGET (len = p*ni + p*mi: xf (p x ni) | uf (p x mi)) or
 *         ALG_SCHED_DISTURBANCE (below).
 *   data: rows x B x len, step-major; NULL drops the kind's schedule.
 *   - in step t (0-based within the call) of alg_mpc_solve game g solves with row min(t, rows - 1) of every scheduled kind: the last row is
 *     held.  The values hold for the whole horizon of that solve (the numbers are constant over a solve, as everywhere).
 *   - after the call the handle's per-game values of a scheduled kind are the row the last step used, on the device and in what
 *     alg_get_scenario_data returns.
 *   - only alg_mpc_solve reads schedules; every other entry point ignores them.
 *   - setting the schedule of a scenario kind makes the kind per game exactly as alg_set_scenario_data(kind, row 0) does (kernel switch and
 *     re-created multipliers in the default ALG_SCEN_KERNELS_EXT mode on the first per-game call, ALG_ERR_STATE if the kind was not added).
 *     ALG_SCHED_LQR_TARGET needs per-game LQR data (alg_set_lqr with per_game = 1; ALG_ERR_STATE otherwise); Qd and Rd stay as set.
 *   - every row is checked by the rules of alg_set_scenario_data (targets: finite); rows < 1 with data is refused.  On any failure the
 *     call returns ALG_ERR_ARG and nothing changes.
 *   - any adder (alg_add_*) drops ALL schedules, alg_set_scenario_data(kind, ...) drops the schedule of that kind, alg_set_lqr the
 *     target schedule.
 *   - in ALG_SCEN_KERNELS_BASE mode the block-reading twins of the base kernels read the game's block through the constant address space,
 *     which must not change during a kernel: a schedule of a base kind (0 .. 2) on such a handle gets ALG_ERR_ARG -- use the default
 *     mode.  ALG_SCHED_LQR_TARGET works in both modes.
 * alg_mpc_get_schedule: *rows = the rows of the kind's schedule, 0 = none. */
#define ALG_SCHED_LQR_TARGET 100
int alg_mpc_set_schedule(alg_handle* h, int32_t kind, int32_t rows, const double* data /* rows x B x len, step-major; NULL = drop */);
int alg_mpc_get_schedule(alg_handle* h, int32_t kind, int32_t* rows /* 0 = none */);
/* The plant disturbance, one more schedule kind of alg_mpc_set_schedule / alg_mpc_get_schedule with len = n: in step t, after the advance,
 * game g's state becomes x0 + w[min(t, rows - 1)][g] (one double addition per entry; the last row is held), written to x0 and to x_1 of
 * pdtraj and trial -- the three places alg_set_x0 writes -- and states[t+1] is the disturbed state.  Step-wise: alg_newton_solve_async,
 * alg_mpc_advance, read x_1, alg_set_x0(x_1 + w_t).
 *   - every entry must be finite; rows < 1 with data is refused; on a failure the call returns ALG_ERR_ARG and nothing changes.
 *   - it needs no per-game data of any other kind and works in both scenario-kernel modes (alg_set_scenario_kernels).
 *   - any adder (alg_add_*) drops it with all other schedules; alg_set_x0, alg_set_lqr and alg_set_scenario_data keep it.
 *   - only alg_mpc_solve / alg_mpc_solve_log read it. */
#define ALG_SCHED_DISTURBANCE 101
/* alg_mpc_solve with the closed-loop log: the same loop, arguments, errors and totals; alg_mpc_solve(h, s, id, st) is
 * alg_mpc_solve_log(h, s, id, st, NULL, NULL).
 *   controls[t][g]: the joint control the advance of step t applies -- u_1 of step t's solution, the m doubles that follow x_2 in the
 *                   alg_get_traj layout of pdtraj (player-major).
 *   stats[t][g]:    what alg_get_stats would return after step t's solve (last.t_elap as measured).
 * The call is synchronous if any of the three output pointers is non-NULL, asynchronous otherwise. */
int alg_mpc_solve_log(alg_handle* h, int32_t steps, int64_t game_id0,
                      double* states          /* (steps+1) x B x n, or NULL */,
                      double* controls        /* steps x B x m, or NULL     */,
                      alg_game_stats* stats   /* steps x B, or NULL         */);
/* The PLANT of the fused loop: the planner runs slower than the plant, and the plant is integrated finer than the planner's
 * discretisation (the reference's Options carry both knobs, mpc_horizon and upsampling, options.jl:97-102).  Three fields per handle:
 *   hold (r >= 1), substeps (s >= 1), integrator (ALG_PLANT_RK2 = 0, ALG_PLANT_RK4 = 1).  The default {1, 1, ALG_PLANT_RK2} is the loop above.
 * MPC step t is solve t, unchanged: game ids game_id0 + t*1000003 + g, schedule rows min(t, rows - 1) of every scenario and target kind
 * (constant over the solve), stats[t].  The solve is followed by r PLANT KNOTS j = 0 ... r - 1, numbered q = t*r + j:
 *   1. control:     u = u_{1+j} of solve t's pdtraj, held constant over the knot: in the alg_get_traj layout the m doubles at offset
 *                   n + j*b + n, b = n + m + n*p (player-major, as stored; the models' joint control vector is component-major).
 *   2. plant step:  x <- Phi(x, u): s sub-steps of length h = dt / (double)s (one double division).  ALG_PLANT_RK2: each sub-step is the
 *                   model's own discrete step, the expression alg_mpc_advance evaluates, called with h (s = 1: that expression with dt, bit
 *                   for bit).  ALG_PLANT_RK4: the classical four-stage method on the model's continuous dynamics, per player; the handle's
 *                   bicycle lengths and quadrotor mass apply.
 *   3. disturbance: if the handle carries one, x <- x + w[min(q, rows - 1)][g], one double addition per entry on the stored value.
 *   4. log:         controls[q][g] = u, states[q + 1][g] = x.
 * After the last knot x is the game's x0 in the three places alg_set_x0 writes; solve t + 1 runs with shift = r and dual_reset = false.
 * The totals gain the solve's newton_iters and converged once per solve.  Output sizes of alg_mpc_solve / alg_mpc_solve_log under a plant:
 * states (steps*r + 1) x B x n, controls steps*r x B x m, stats steps x B.
 * alg_mpc_set_plant: 1 <= hold <= N - 1, 1 <= substeps <= 256, integrator 0 or 1, reserved == 0; otherwise ALG_ERR_ARG and nothing changes.
 *   p = NULL restores the default.  The setting is independent of constraints and LQR data: adders, alg_set_options, alg_set_x0, alg_set_lqr,
 *   alg_set_scenario_data and schedules keep it.
 * alg_mpc_plant_advance(h, j): the step-wise form of one plant knot (asynchronous): step 2 for every game from the handle's current x0 and
 *   u_{1+j} of pdtraj, written to x0 and to x_1 of pdtraj and trial; the totals gain the solve only for j == 0; j outside 0 ... N - 2 is
 *   ALG_ERR_ARG.  With the default plant and j = 0 it is alg_mpc_advance, bit for bit.  The step-wise definition of the loop, per solve:
 *   the schedule rows; shift = r and dual_reset = 0 from solve 1 on; alg_newton_solve_async; alg_get_stats and the controls from
 *   alg_get_traj; for j < r: alg_mpc_plant_advance(j), read x0, alg_set_x0(x0 + w_q) if disturbed. */
#define ALG_PLANT_RK2 0
#define ALG_PLANT_RK4 1
typedef struct alg_mpc_plant { int32_t hold, substeps, integrator, reserved; } alg_mpc_plant;
int alg_mpc_set_plant(alg_handle* h, const alg_mpc_plant* p /* NULL = default */);
int alg_mpc_get_plant(alg_handle* h, alg_mpc_plant* p);
int alg_mpc_plant_advance(alg_handle* h, int32_t knot);
/* The closed-loop COST LOG of the fused loop: what the run cost each player, evaluated on the device.  States and controls alone do not
 * determine it: the running cost of a knot depends on the schedule row its solve used and on per-game numbers that live on the device.
 * With the log on (default off) alg_mpc_solve / alg_mpc_solve_log keep the state and control logs on the device whether or not the caller asks
 * for them (the loop kernels with per-step phases, as for any log) and queue one more kernel behind the loop, on the same stream: a call with
 * three NULL output pointers stays asynchronous.  Plant knot q = t*hold + j of solve t, player i:
 *   stage[q][g][i] = dt * l_i(states[q][g], controls[q][g]), the three components of alg_get_cost's l_i (LQRCost objective.jl:12-35,
 *   CollisionCost objective.jl:122-131): states[q] is the state at the beginning of the knot (the disturbance of the knot before included),
 *   controls[q] the control held, read through pu_i of the stored player-major order.  xf, uf: row min(t, rows - 1) of the
 *   ALG_SCHED_LQR_TARGET schedule if one is set, else the handle's; mu, r: row min(t, rows - 1) of an ALG_SCEN_COLLISION_COST schedule if one
 *   is set, else the game's block or the handle's values; Q and R as set.  No terminal term: states[knots] is not costed.
 *   total[g][i] = sum_q stage[q][g][i], per component.
 * States, controls, statistics, totals and everything the loop leaves on the handle are bit-identical with the log on and off.
 * The log lives in a buffer of the handle's own, (knots + 1) x B x p x 3 doubles, grown on demand and freed when the log is switched off; a
 * run whose log would exceed 1 GiB is refused with ALG_ERR_ARG before anything is launched.
 * alg_mpc_get_cost waits for the stream.  *knots_out = the plant knots of the most recent alg_mpc_solve / alg_mpc_solve_log; stage receives
 * the first min(max_knots, *knots_out) of them (knots x B x p x 3), total B x p x 3; either may be NULL.  The log belongs to that loop and
 * to the data it ran with: any adder (alg_add_*), alg_set_lqr, alg_set_scenario_data and alg_mpc_set_schedule invalidate it -- *knots_out = 0
 * and nothing is written -- until the next loop.  With the log off: ALG_OK and *knots_out = 0.  IBR and the step-wise MPC calls have no log. */
int alg_mpc_set_cost_log(alg_handle* h, int32_t on);
int alg_mpc_get_cost_log(alg_handle* h, int32_t* on);
int alg_mpc_get_cost(alg_handle* h, int32_t max_knots, double* stage /* knots x B x p x 3, or NULL */, double* total /* B x p x 3, or NULL */, int32_t* knots_out);
/* The closed-loop CONSTRAINT LOG of the fused loop: did the run stay feasible?  As with the cost log, states and controls alone do not
 * determine it: the constraint numbers of a knot are those of the schedule row its solve used, or of per-game blocks that live on the
 * device, and after the loop only the last row is left in the blocks.  With the log on (default off) alg_mpc_solve / alg_mpc_solve_log
 * behave as with the cost log: the state and control logs stay on the device whether or not the caller asks for them, one more kernel is
 * queued behind the loop (behind the cost kernel if both logs are on) on the same stream, and a call with three NULL output pointers stays
 * asynchronous.  Plant knot q = t*hold + j of solve t, in the knot layout of alg_get_con_values (K1 = alg_con_knot_len rows):
 *   the control-bound rows are evaluated on controls[q], the control applied over the knot; every other row on states[q + 1], the state the
 *   knot reaches, disturbance included -- the (u_k, x_{k+1}) pairing of a step of the constraint layout.  Every number comes from row
 *   min(t, rows - 1) of the kind's schedule (ALG_SCEN_COLLISION_RADIUS, _CONTROL_BOUND, _STATE_BOUND, _WALL, _CIRCLE, _WALL3D, _CYLINDER) if
 *   one is set, else from the game's block or the handle's values: the planner's own view in solve t, the convention of the cost log.
 *   Masks, pair sets, cylinder axes and the +-inf pattern are the handle's.
 * alg_mpc_get_con waits for the stream.  *knots_out = the plant knots of the most recent loop;
 *   vals   the first min(max_knots, *knots_out) knots, knots x B x K1;
 *   worst  B x ALG_CON_KINDS: the maximum of the kind's rows over ALL knots of the run; -inf for a kind that was not added, NaN if any of
 *          the kind's rows is NaN;
 *   first  B x ALG_CON_KINDS: the smallest q at which a row of the kind satisfies !(c <= 0) (a NaN counts), -1 if there is none;
 * any of the three may be NULL; worst and first cover the whole run whatever max_knots is.
 * States, controls, statistics, totals and everything the loop leaves on the handle are bit-identical with the log on and off; cost log and
 * constraint log may be on together.  The log lives in a buffer of the handle's own (knots x B x K1 doubles plus the summary), grown on
 * demand and freed when the log is switched off; a run whose log would exceed 1 GiB is refused with ALG_ERR_ARG before anything is launched.
 * The log belongs to the most recent loop and to the data it ran with: what invalidates the cost log invalidates it (any adder, alg_set_lqr,
 * alg_set_scenario_data, alg_mpc_set_schedule) -- *knots_out = 0 and nothing is written -- until the next loop.  With the log off: ALG_OK
 * and *knots_out = 0.  IBR and the step-wise MPC calls have no log. */
int alg_mpc_set_con_log(alg_handle* h, int32_t on);
int alg_mpc_get_con_log(alg_handle* h, int32_t* on);
int alg_mpc_get_con(alg_handle* h, int32_t max_knots, double* vals /* knots x B x K1, or NULL */, double* worst /* B x 7, or NULL */,
                    int32_t* first /* B x 7, or NULL */, int32_t* knots_out);

#ifdef __cplusplus
}
#endif
#endif /* ALGAMES_HIP_H */
