// algames_kernels.hpp -- the __global__ entry points (one workgroup = one wavefront = one game) and the list of compiled
// (model, p, d, ext) instantiations, as lists ALG_CFGS_*(X).  Every list is explicitly instantiated in translation units of its own, so
// that they build in parallel: algames_unit.hip applies one instantiation macro to one list, both named by the build (the table of
// families in __graft_entry__.py); algames_base.hip holds one base configuration per unit, algames_mw.hip the teams and their hand-off.
// ext = 2 (Cfg::SCEN without Cfg::EXT): the base kernels with the scenario numbers read from the game's block.
#pragma once
#include "algames_device.hpp"

using namespace alg;

// ------------------------------------------------------------------------------------------------
// Kernels
// ------------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(C::NT, C::WPE) k_newton_solve(Params pr_arg, int init, uint64_t game_id0) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    newton_solve<C>(pr, G, L, init, game_id0 + (uint64_t)g);
}

// The fused solve that also stores the four .vio vectors of every record (alg_set_history_profiles; vio_profile_phase, algames_solver.hpp;
// DESIGN.md 3.6).  A sibling of k_newton_solve, not one more argument or a runtime branch of it: k_newton_solve's source, and with it the
// binary of every solve without profiles, stays what it was.  `vio`: B x vio_max x (4 N - 2) doubles, per record [dyn (N-1) | con (N-1) |
// sta (N) | opt (N)]; the phase reads the two arguments from the kernel-argument segment (NewtonVioArgs), the by-value copies are unused.
// Seven to ten players have none: one game per CU, the longest compiles of the library (alg_set_history_profiles refuses them).
// The siblings are a kernel family of their own, in a namespace of their own (history_vio::k_newton_solve_vio<C>): the k_newton_solve* /
// k_mpc_loop* families are pinned kernel for kernel against the build before the KKT solves (tests/test_kkt_solve_build.py), these are
// listed by tests/test_history_vio_abi.py.
template <class C> inline constexpr bool vio_sibling_v = C::P <= 6;
namespace history_vio {
template <class C>
__global__ void __launch_bounds__(C::NT, C::WPE) k_newton_solve_vio(Params pr_arg, int init, uint64_t game_id0, double* vio_arg, int vio_max_arg) {
    static_assert(vio_sibling_v<C>, "no profile sibling for seven to ten players");
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    newton_solve<C, 0, false, true>(pr, G, L, init, game_id0 + (uint64_t)g);
}
} // namespace history_vio

// Straggler hand-off (alg_set_handoff; newton_solve<C, HO>, algames_solver.hpp): the budgeted one-wavefront solve, whose games park after
// `budget` inner iterations, and the team kernel that resumes the parked games (block b takes the b-th entry of the handle's queue; the
// launch covers the whole batch, blocks past the queue's count leave at once).
template <class C>
__global__ void __launch_bounds__(C::NT, C::WPE) k_newton_solve_ho(Params pr_arg, int init, uint64_t game_id0, int budget) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    newton_solve<C, 1>(pr, G, L, init, game_id0 + (uint64_t)g, -1, -1, budget);
}
template <class C>
__global__ void __launch_bounds__(C::NT, C::WPE) k_newton_resume(Params pr_arg) {        // (C = Cfg<..., NW, 0>: no line-search staging in LDS)
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int* q = as_global(pr.ho_queue);
    if ((int)blockIdx.x >= __builtin_amdgcn_readfirstlane(q[0])) return;
    const int g = __builtin_amdgcn_readfirstlane(q[1 + blockIdx.x]);
    Game G = game_view(pr, g);
    newton_solve<C, 2>(pr, G, L, 0, 0);
}

template <class C>
// (no occupancy bound: the host-driven stepping entry point is not throughput code, and inner_iteration's live ranges at the four-waves-per-SIMD
// budget are sized for the fused kernel, where the surrounding loops are in the same function)
__global__ void __launch_bounds__(WAVE) k_newton_step(Params pr_arg, int k, int l, const double* delta_in, alg_step_info* out) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    int ls = 0; double dl = delta_in ? delta_in[g] : 0.0;          // the caller's Δ goes into record! (solver_methods.jl:75)
    inner_iteration<C>(pr, G, L, ls, dl, k, l, out + g, nullptr);
    settle_traj<C>(pr, G);
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_residual(Params pr_arg, int which, double reg, double* rn_out) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    ResOut ro;
    // the proximal term is taken w.r.t. pdtraj (regularize_residual!, global_quantities.jl:67-86)
    assemble_pass<C, 2>(pr, G, L.a, which, reg != 0.0 ? 0 : -1, reg, 0.0, ro);
    __syncthreads();
    if (rn_out && threadIdx.x == 0) rn_out[g] = ro.l1 / (double)pr.S;
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_jacobian(Params pr_arg, double reg, double* J, int g0) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x + g0;        // games g0 .. g0 + gridDim.x - 1; J holds gridDim.x blocks
    Game G = game_view(pr, g);
    ResOut ro;
    assemble_pass<C, 1>(pr, G, L.a, 0, -1, 0.0, reg, ro);
    __syncthreads();
    jacobian_dense<C>(pr, G, reg, J + (size_t)blockIdx.x * pr.S * pr.S);
}

template <class C>
__global__ void __launch_bounds__(WAVE, C::WPE) k_direction(Params pr_arg, double reg, int* status) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    ResOut ro;
    assemble_pass<C, 1>(pr, G, L.a, 0, -1, 0.0, reg, ro);
    __syncthreads();
    const int st = refined_direction<C, false, false>(pr, G, L, reg, -1, nullptr);
    if (status && threadIdx.x == 0) status[g] = st;
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_line_search(Params pr_arg, double reg, const double* rn, double* alpha, int* j) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    double a; int jj;
    line_search<C>(pr, G, L, reg, rn[g], -1.0, &a, &jj);
    if (threadIdx.x == 0) { alpha[g] = a; j[g] = jj; }
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_update(Params pr_arg, int tgt, int src, const double* alpha) {
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    update_traj<C>(pr, G, tgt, src, alpha[g]);
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_record(Params pr_arg, alg_record* out) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    make_record<C>(pr, G, L, 0.0, 0, 0.0, out + g);
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_dual_update(Params pr_arg) {
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    dual_penalty_update<C>(pr, G);
}

template <class C>
__global__ void __launch_bounds__(WAVE) k_init(Params pr_arg, uint64_t game_id0, int use_shift, int do_init, int which) {
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    if (do_init) {
        init_traj<C>(pr, G, G.z(0), game_id0 + (uint64_t)g, use_shift != 0);
        if (threadIdx.x < C::n) G.z(1)[threadIdx.x] = G.x0(pr)[threadIdx.x];
        __syncthreads();
        rollout<C>(pr, G.z(0));
    } else {
        rollout<C>(pr, G.z(which));
    }
}

// mode 0: ibr_newton_solve!(prob, player) on the stored trajectory ; mode 1: ibr_newton_solve!(prob; ibr_opts)
template <class C>
__global__ void __launch_bounds__(WAVE, (C::WPE < 2 ? C::WPE : 2)) k_ibr(Params pr_arg, int mode, int player, int init, uint64_t game_id0,
                                                      int ibr_iter, IbrOrder order, double delta_min) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    ibr_newton_solve<C>(pr, G, L, mode == 0, player, init, game_id0 + (uint64_t)g, ibr_iter, order, delta_min);
}

// builder-defined MPC advance: x0 <- RK2(x_1, u_1) per game (lanes < P own a player), totals += solve
template <class C>
__device__ __forceinline__ void mpc_advance(CPR pr, const Game& G) {
    const int lane = phase_lane();
    if constexpr (C::QUAD) {
        if (lane < C::P) {
            double xi[12], ui[4], xo[12];
#pragma unroll
            for (int j = 0; j < 12; j++) xi[j] = G.z(0)[lane + j * C::P];
#pragma unroll
            for (int j = 0; j < 4; j++) ui[j] = G.z(0)[C::n + hu<C>(0, lane) + j];
            quad_rk2(xi, ui, pr.qmass, pr.dt, xo);
#pragma unroll
            for (int j = 0; j < 12; j++) { const int a = lane + j * C::P; G.x0w(pr)[a] = xo[j]; G.z(0)[a] = xo[j]; G.z(1)[a] = xo[j]; }
        }
    } else if (lane < C::P) {
        double x[C::n], u[C::m], xo[C::ni];
        for (int j = 0; j < C::ni; j++) x[lane + j * C::P] = G.z(0)[lane + j * C::P];
        for (int j = 0; j < C::mi; j++) u[lane + j * C::P] = G.z(0)[C::n + hu<C>(0, lane) + j];
        model_rk2<C>(pr, lane, x, u, pr.dt, xo);
        for (int j = 0; j < C::ni; j++) {
            const int a = lane + j * C::P;
            G.x0w(pr)[a] = xo[j]; G.z(0)[a] = xo[j]; G.z(1)[a] = xo[j];
        }
    }
    if (lane == 0) { G.mpc(pr)[0] += G.st(pr)->newton_iters; G.mpc(pr)[1] += G.st(pr)->converged; }
}
template <class C>
__global__ void __launch_bounds__(WAVE) k_mpc_advance(Params pr_arg) {
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    mpc_advance<C>(pr, G);
}

// The whole receding-horizon loop of one game in one wave (BASELINE config 5): `steps` x (newton_solve! from the shifted
// warm start, advance x0 by one RK2 step).  Games never wait for each other between MPC steps, so a game that needs many
// Newton iterations at one step only delays itself.  Step 0 uses the handle's shift / dual_reset, later steps shift = 1
// and dual_reset = false (the reference's warm-start hooks, options.jl / primal_dual_traj.jl:29-44).
// Register budget of the 256-VGPR class for every configuration: the loop carries more live state (step counter, state log,
// totals) than a single solve; at 128 VGPRs the DoubleIntegrator instantiations spilled SGPRs so heavily that the 2-player
// one faulted on a null base pointer (tests/test_gpu_parity_ext.py::test_no_kernel_writes_outside_its_buffers runs this
// kernel for every instantiation).
// (the loop's own arguments are re-read from the kernel-argument segment where they are used, like `Params`: as by-value arguments they
// were live -- in SGPRs, i.e. spilled -- across every phase of every solve)
// The loop kernels of the teams of four (BASELINE C5 runs k_mpc_loop<Cfg<UNICYCLE, 3, 2, 0, 4>>) also run the solve's set-up on laundered views
// (newton_solve<C, 0, LOOP = true>): 20 -> 13 SGPR spills in that kernel.  Only there: the solver-level functions are left to the inliner, and a loop
// kernel that instantiates another newton_solve than the configuration's solve kernel changes the inliner's decisions for BOTH kernels of the
// configuration -- with the switch on everywhere the C3 solve kernel (team of two) went from 8 to 10 spills (round 6, measured per combination).
#ifndef ALG_LOOP_LAUNDER
#define ALG_LOOP_LAUNDER 1
#endif
template <class C> inline constexpr bool mpc_loop_launder_v = ALG_LOOP_LAUNDER != 0 && C::NW == 4;
struct MpcLoopArgs { Params pr; int steps; uint64_t game_id0; double* states; };
// (the 4-player bicycle with the extended constraint set -- 8 controls x 17 right-hand sides in registers -- sits at the 256-register
// ceiling with the loop's own state on top: it takes the one-wavefront-per-SIMD budget, where the allocator parks the overflow in the
// accumulation registers instead of scratch; the loop runs small batches, never two wavefronts per SIMD)
template <class C> inline constexpr int mpc_loop_wpe = (C::WPE < 2 || (C::MODEL == ALG_MODEL_BICYCLE && C::P == 4)) ? 1 : 2;
template <class C>
__global__ void __launch_bounds__(C::NT, mpc_loop_wpe<C>) k_mpc_loop(Params pr_arg, int steps_arg, uint64_t game_id0_arg, double* states_arg) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
#if defined(__HIP_DEVICE_COMPILE__)
    const ALG_AS4 MpcLoopArgs& ka = *(const ALG_AS4 MpcLoopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const MpcLoopArgs& ka = *(const MpcLoopArgs*)nullptr;      // host pass: never executed
#endif
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    // (the loop's arguments are read through a laundered copy of the segment pointer wherever they are used -- `kq()` -- so that no load is shared
    // between the prologue, the loop test and the loop body: a shared load is a value live, i.e. spilled, across every phase of every solve)
    auto kq = [&]() -> const ALG_AS4 MpcLoopArgs& { return *(const ALG_AS4 MpcLoopArgs*)uniform_u64((unsigned long long)&ka); };
    {
        double* const st0 = kq().states; const int l0 = phase_lane();
        if (st0 && l0 < C::n) { const Game H = G.fresh(); CPR pr0 = phase_params(pr); st0[(size_t)phase_int(g) * C::n + l0] = H.x0(pr0)[l0]; }
    }
    if (kq().steps < 1) return;
    for (int t = 0; ; t++) {
        // (everything the step needs besides `t` is re-derived from opaque roots inside the loop -- the game's index, the lane's predicates, the
        // arguments: as invariants of this loop they were live, i.e. spilled, across every phase of every solve)
        const int gq = phase_int(g);
        newton_solve<C, 0, mpc_loop_launder_v<C>>(pr, G, L, 1, kq().game_id0 + (uint64_t)t * 1000003ull + (uint64_t)gq, t == 0 ? -1 : 1, t == 0 ? -1 : 0);
        __syncthreads();
        mpc_advance<C>(phase_params(pr), G.fresh());
        __syncthreads();
        double* const states = kq().states;
        const int ln = phase_lane();
        if (states && ln < C::n) { CPR prs = phase_params(pr); states[((size_t)(t + 1) * prs.B + phase_int(g)) * C::n + ln] = G.fresh().z(0)[ln]; }
        __syncthreads();
        if (t + 1 >= kq().steps) break;
    }
}

// The receding-horizon loop with a SCHEDULE (alg_mpc_set_schedule): per game and per MPC step values of the numbers that may differ per
// game -- the kinds of the scenario block and the LQR targets xf / uf.  A sibling of k_mpc_loop, not one more argument of it: k_mpc_loop's
// source, and with it the binary of every unscheduled loop, stays what it was; the siblings live in translation units of
// their own (ALG_DEFINE_SCHED*) and are launched only while the handle carries a schedule, a disturbance or a plant (alg_mpc_set_plant), or the
// call asks for a log (alg_mpc_solve_log): the sibling is the loop with per-step phases.
// The schedule sits in device memory in compact form, rows x B x len doubles per kind, with a table of len block offsets per kind (the host's
// scen_map; ALG_SCHED_TO_LQR marks an offset into the game's LQR block, a negative entry is skipped like alg_set_scenario_data skips it).
// Before every solve the game's wavefronts copy row min(t, rows - 1) of every kind into the game's own blocks with ordinary vector stores.
// The solver reads those blocks with vector loads (as_global), through the CU's vector L1 the stores went through, behind a workgroup
// barrier.  The ALG_AS4 readers of the block (Cfg::SCEN without Cfg::EXT: constant address space, memory the compiler takes as unchanged
// during a kernel) must not meet a scheduled scenario kind: the host refuses that (alg_mpc_set_schedule).
constexpr int ALG_SCHED_MAX_KINDS = 9;                 // the eight ALG_SCEN_* kinds + ALG_SCHED_LQR_TARGET
constexpr int ALG_SCHED_TO_LQR = 1 << 30;
struct MpcSchedKind { const double* data; const int* map; int rows, len; };
struct MpcSched { int nk, pad_; MpcSchedKind k[ALG_SCHED_MAX_KINDS]; };
// The per-step phases besides the schedule (alg_mpc_solve_log, ALG_SCHED_DISTURBANCE): the LOG of step t -- the control the advance
// applies (u_1 of pdtraj, the m doubles behind x_2) and the game's alg_game_stats as the solve left them -- and the plant DISTURBANCE
// w[min(t, rows - 1)][g], added to the advanced state.  A null pointer skips its part.  Descriptors of their own in the kernel-argument segment.
struct MpcLoopLog { double* controls; alg_game_stats* stats; const double* dist; int dist_rows, pad_; };
template <class C>
__device__ __forceinline__ void mpc_apply_schedule(CPR pr, const ALG_AS4 MpcSched& sd, const int g, const int t) {
    const int tid = phase_lane(), nk = sd.nk;
    double* const scen = as_global(const_cast<double*>(pr.scen)) + (size_t)g * pr.scen_stride;
    double* const lqr = as_global(const_cast<double*>(pr.lqr)) + (size_t)g * pr.lqr_stride;
    for (int k = 0; k < nk; k++) {
        const int len = sd.k[k].len, rows = sd.k[k].rows, row = t < rows ? t : rows - 1;      // the last row is held
        const double* const src = as_global(sd.k[k].data) + ((size_t)row * pr.B + g) * len;
        const int* const map = as_global(sd.k[k].map);
        for (int e = tid; e < len; e += C::NT) {
            const int o = map[e];
            if (o < 0) continue;
            if (o & ALG_SCHED_TO_LQR) lqr[o & ~ALG_SCHED_TO_LQR] = src[e];
            else scen[o] = src[e];
        }
    }
}
// the log phase: after the solve of step t, before the advance (which shifts nothing but x0 / x_1, yet the totals belong to the same step)
template <class C>
__device__ __forceinline__ void mpc_log_step(CPR pr, const Game& G, const ALG_AS4 MpcLoopLog& lg, const int g, const int t) {
    const int tid = phase_lane();
    const size_t at = (size_t)t * pr.B + g;
    double* const uc = lg.controls;
    if (uc && tid < C::m) as_global(uc)[at * C::m + tid] = G.z(0)[2 * C::n + tid];
    alg_game_stats* const so = lg.stats;
    constexpr int W = (int)(sizeof(alg_game_stats) / 8);
    static_assert(sizeof(alg_game_stats) % 8 == 0, "alg_game_stats is copied in 8-byte words");
    if (so && tid < W) reinterpret_cast<unsigned long long*>(as_global(so) + at)[tid] = reinterpret_cast<const unsigned long long*>(G.st(pr))[tid];
}
// the disturbance phase: after the advance, x0 <- x0 + w_t with one double addition per entry on the STORED x0 (the sum the host forms in the
// step-wise definition: alg_set_x0(x_1 + w_t)), written to the three places alg_set_x0 writes.  Not part of mpc_advance, nor of its RK2
// expression: the unscheduled kernels share that function, and a sum folded into it would round differently.
template <class C>
__device__ __forceinline__ void mpc_disturb(CPR pr, const Game& G, const ALG_AS4 MpcLoopLog& lg, const int g, const int t) {
    const double* const w = lg.dist;
    if (!w) return;
    const int tid = phase_lane(), rows = lg.dist_rows, row = t < rows ? t : rows - 1;      // the last row is held
    if (tid < C::n) {
        const double v = G.x0w(pr)[tid] + as_global(w)[((size_t)row * pr.B + g) * C::n + tid];
        G.x0w(pr)[tid] = v; G.z(0)[tid] = v; G.z(1)[tid] = v;
    }
}
// The PLANT (alg_mpc_set_plant): every solve is followed by `hold` plant knots j = 0 ... hold - 1; knot j holds u_{1+j} of the
// solve's pdtraj and integrates the state over dt in `substeps` sub-steps of h = dt / substeps, with the model's own RK2 step (the expression
// mpc_advance evaluates, called with h) or the classical RK4 on the model's continuous dynamics.  {1, 1, RK2} is the loop without a plant.
struct MpcPlant { int hold, substeps, integrator, pad_; };
struct MpcLoopSchedArgs { Params pr; int steps; uint64_t game_id0; double* states; MpcSched sd; MpcLoopLog lg; MpcPlant pl; };
__host__ __device__ inline bool mpc_plant_is_default(int hold, int substeps, int integrator) { return hold == 1 && substeps == 1 && integrator == ALG_PLANT_RK2; }
// the model's own discrete step (model_rk2, quad_rk2) on the player's own entries: the same expressions, entry for entry
template <class C>
__device__ __forceinline__ void plant_rk2(CPR pr, const double (&xi)[C::ni], const double (&ui)[C::mi], const double dt, double (&xn)[C::ni]) {
    if constexpr (C::QUAD) {
        quad_rk2(xi, ui, pr.qmass, dt, xn);
    } else if constexpr (C::MODEL == ALG_MODEL_DOUBLE_INTEGRATOR) {
#pragma unroll
        for (int j = 0; j < C::D; j++) {
            const double vm = xi[C::D + j] + (ui[j] * dt) * 0.5;
            xn[j] = xi[j] + vm * dt;
            xn[C::D + j] = xi[C::D + j] + ui[j] * dt;
        }
    } else if constexpr (C::MODEL == ALG_MODEL_BICYCLE) {
        const double v = xi[2], psi = xi[3], a = ui[0];
        const BikeGeom g = bike_geom(ui[1], pr.lf, pr.lr);
        const double vm = v + (a * dt) * 0.5, psm = psi + (v * g.sg * dt) * 0.5;
        double s, c; sincos(g.beta + psm, &s, &c);
        xn[0] = xi[0] + (vm * c) * dt;
        xn[1] = xi[1] + (vm * s) * dt;
        xn[2] = v + a * dt;
        xn[3] = psi + (vm * g.sg) * dt;
    } else {
        const double th = xi[2], v = xi[3], om = ui[0], a = ui[1];
        const double thm = th + (om * dt) * 0.5, vm = v + (a * dt) * 0.5;
        double s, c;
        sincos(thm, &s, &c);
        xn[0] = xi[0] + (c * vm) * dt;
        xn[1] = xi[1] + (s * vm) * dt;
        xn[2] = th + om * dt;
        xn[3] = v + a * dt;
    }
}
// classical RK4: the stage vector, the running sum and the stage state are register arrays with compile-time indices
template <class C>
__device__ __forceinline__ void plant_rk4(CPR pr, const double (&xi)[C::ni], const double (&ui)[C::mi], const double h, double (&xn)[C::ni]) {
    double k[C::ni], acc[C::ni], t[C::ni];
    model_f<C>(pr, xi, ui, k);
#pragma unroll
    for (int j = 0; j < C::ni; j++) { acc[j] = k[j]; t[j] = xi[j] + (h * 0.5) * k[j]; }
    model_f<C>(pr, t, ui, k);
#pragma unroll
    for (int j = 0; j < C::ni; j++) { acc[j] = acc[j] + 2.0 * k[j]; t[j] = xi[j] + (h * 0.5) * k[j]; }
    model_f<C>(pr, t, ui, k);
#pragma unroll
    for (int j = 0; j < C::ni; j++) { acc[j] = acc[j] + 2.0 * k[j]; t[j] = xi[j] + h * k[j]; }
    model_f<C>(pr, t, ui, k);
#pragma unroll
    for (int j = 0; j < C::ni; j++) xn[j] = xi[j] + (h / 6.0) * (acc[j] + k[j]);
}
// One plant knot of one game: x0 <- Phi(x0, u_{1+knot} of pdtraj), written to the three places alg_set_x0 writes; lanes < P own a player, as
// in mpc_advance.  The totals gain the solve once per solve (knot 0).  `uc` (or null) receives the control held, in the stored order.
// Serves the fused loop (k_mpc_loop_sched) and alg_mpc_plant_advance (k_mpc_plant_advance): fused equals step-wise bit for bit.
template <class C>
__device__ __forceinline__ void mpc_plant_knot(CPR pr, const Game& G, const int knot, const int substeps, const int integrator, double* const uc) {
    const int lane = phase_lane();
    const double* const u = G.z(0) + C::n + knot * C::b + C::n;
    if (uc && lane < C::m) uc[lane] = u[lane];
    if (lane < C::P) {
        double xi[C::ni], ui[C::mi], xo[C::ni];
#pragma unroll
        for (int j = 0; j < C::ni; j++) xi[j] = G.x0(pr)[lane + j * C::P];
#pragma unroll
        for (int j = 0; j < C::mi; j++) ui[j] = u[lane * C::mi + j];
        const double h = pr.dt / (double)substeps;
        for (int s = 0; s < substeps; s++) {
            // (an opaque copy of h per sub-step: products of h and the held control are loop invariants, and hoisted out of the loop they sit in
            // another block than the additions they feed -- no longer one fused multiply-add as in mpc_advance, i.e. other bits)
            const double hs = phase_f64(h);
            if (integrator == ALG_PLANT_RK4) plant_rk4<C>(pr, xi, ui, hs, xo);
            else plant_rk2<C>(pr, xi, ui, hs, xo);
#pragma unroll
            for (int j = 0; j < C::ni; j++) xi[j] = xo[j];
        }
#pragma unroll
        for (int j = 0; j < C::ni; j++) { const int a = lane + j * C::P; G.x0w(pr)[a] = xi[j]; G.z(0)[a] = xi[j]; G.z(1)[a] = xi[j]; }
    }
    if (lane == 0 && knot == 0) { G.mpc(pr)[0] += G.st(pr)->newton_iters; G.mpc(pr)[1] += G.st(pr)->converged; }
}
// alg_mpc_plant_advance: the step-wise form of one plant knot (one wavefront per game, like every step-wise entry point)
template <class C>
__global__ void __launch_bounds__(WAVE) k_mpc_plant_advance(Params pr_arg, int knot, MpcPlant pl) {
    CPR pr = kernel_params();
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    mpc_plant_knot<C>(pr, G, knot, pl.substeps, pl.integrator, nullptr);
}
// the second phase of a knot in the fused loop: the disturbance row of knot q (one addition on the STORED value, like mpc_disturb) and the
// state log states[q + 1]
template <class C>
__device__ __forceinline__ void mpc_plant_store(CPR pr, const Game& G, const ALG_AS4 MpcLoopLog& lg, double* const states, const int g, const int q) {
    const int tid = phase_lane();
    if (tid >= C::n) return;
    double v = G.x0w(pr)[tid];
    const double* const w = lg.dist;
    if (w) {
        const int rows = lg.dist_rows, row = q < rows ? q : rows - 1;      // the last row is held
        v = v + as_global(w)[((size_t)row * pr.B + g) * C::n + tid];
        G.x0w(pr)[tid] = v; G.z(0)[tid] = v; G.z(1)[tid] = v;
    }
    if (states) as_global(states)[((size_t)(q + 1) * pr.B + g) * C::n + tid] = v;
}
// the statistics of solve t (the part of mpc_log_step that is per solve under a plant too)
__device__ __forceinline__ void mpc_log_stats(CPR pr, const Game& G, const ALG_AS4 MpcLoopLog& lg, const int g, const int t) {
    alg_game_stats* const so = lg.stats;
    constexpr int W = (int)(sizeof(alg_game_stats) / 8);
    const int tid = phase_lane();
    if (so && tid < W) reinterpret_cast<unsigned long long*>(as_global(so) + ((size_t)t * pr.B + g))[tid] = reinterpret_cast<const unsigned long long*>(G.st(pr))[tid];
}
template <class C>
__global__ void __launch_bounds__(C::NT, mpc_loop_wpe<C>) k_mpc_loop_sched(Params pr_arg, int steps_arg, uint64_t game_id0_arg, double* states_arg, MpcSched sd_arg,
                                                                            MpcLoopLog lg_arg, MpcPlant pl_arg) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
#if defined(__HIP_DEVICE_COMPILE__)
    const ALG_AS4 MpcLoopSchedArgs& ka = *(const ALG_AS4 MpcLoopSchedArgs*)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const MpcLoopSchedArgs& ka = *(const MpcLoopSchedArgs*)nullptr;      // host pass: never executed
#endif
    const int g = blockIdx.x;
    Game G = game_view(pr, g);
    auto kq = [&]() -> const ALG_AS4 MpcLoopSchedArgs& { return *(const ALG_AS4 MpcLoopSchedArgs*)uniform_u64((unsigned long long)&ka); };
    {
        double* const st0 = kq().states; const int l0 = phase_lane();
        if (st0 && l0 < C::n) { const Game H = G.fresh(); CPR pr0 = phase_params(pr); st0[(size_t)phase_int(g) * C::n + l0] = H.x0(pr0)[l0]; }
    }
    if (kq().steps < 1) return;
    for (int t = 0; ; t++) {
        // the schedule phase: between the advance of step t - 1 and the solve of step t (and before step 0), bracketed by barriers, everything
        // of it re-derived from the opaque roots -- nothing of it lives across the solve
        __syncthreads();
        mpc_apply_schedule<C>(phase_params(pr), kq().sd, phase_int(g), t);
        __syncthreads();
        const int gq = phase_int(g);
        // (the warm start of solve t >= 1 is shifted by the knots the plant held: 1 without a plant)
        newton_solve<C, 0, mpc_loop_launder_v<C>>(pr, G, L, 1, kq().game_id0 + (uint64_t)t * 1000003ull + (uint64_t)gq, t == 0 ? -1 : kq().pl.hold, t == 0 ? -1 : 0);
        __syncthreads();
        if (mpc_plant_is_default(kq().pl.hold, kq().pl.substeps, kq().pl.integrator)) {
            // the log phase, the advance, the disturbance phase: each behind a barrier, each from the opaque roots like the schedule phase
            mpc_log_step<C>(phase_params(pr), G.fresh(), kq().lg, phase_int(g), t);
            __syncthreads();
            mpc_advance<C>(phase_params(pr), G.fresh());
            __syncthreads();
            mpc_disturb<C>(phase_params(pr), G.fresh(), kq().lg, phase_int(g), t);
            __syncthreads();
            double* const states = kq().states;
            const int ln = phase_lane();
            if (states && ln < C::n) { CPR prs = phase_params(pr); states[((size_t)(t + 1) * prs.B + phase_int(g)) * C::n + ln] = G.fresh().z(0)[ln]; }
            __syncthreads();
        } else {
            // the plant phase: the statistics of the solve, then `hold` knots of two phases each -- [control log | plant step] and
            // [disturbance | state log] -- each behind a barrier and from the opaque roots; only t and the knot counter live across them
            mpc_log_stats(phase_params(pr), G.fresh(), kq().lg, phase_int(g), t);
            for (int j = 0; j < kq().pl.hold; j++) {
                __syncthreads();
                {
                    CPR prk = phase_params(pr);
                    double* const uc = kq().lg.controls;
                    const size_t q = (size_t)t * kq().pl.hold + j;
                    mpc_plant_knot<C>(prk, G.fresh(), j, kq().pl.substeps, kq().pl.integrator, uc ? as_global(uc) + (q * prk.B + phase_int(g)) * C::m : nullptr);
                }
                __syncthreads();
                mpc_plant_store<C>(phase_params(pr), G.fresh(), kq().lg, kq().states, phase_int(g), t * kq().pl.hold + j);
            }
            __syncthreads();
        }
        if (t + 1 >= kq().steps) break;
    }
}

// Players' costs of a plan and of a closed-loop run (k_player_cost, k_closed_loop_cost)
#include "algames_cost.hpp"
// Constraint values of a plan and of a closed-loop run, row by row (k_con_values, k_closed_loop_con)
#include "algames_con.hpp"
// The KKT column kernel: solves with many right-hand sides and parameter sensitivities (k_kkt_sens)
#include "algames_sens.hpp"

// ------------------------------------------------------------------------------------------------
// Instantiation lists: X(model, p, d, ext)
// ------------------------------------------------------------------------------------------------
// The nine base configurations, by their ext column E: 0 = the scenario numbers are kernel constants, 2 = they are read from the game's
// block (Cfg::SCEN without Cfg::EXT; alg_set_scenario_kernels).  The kernels of entry k live in a unit of their own (algames_base.hip), the
// scheduled loops and the KKT solves in one unit per half.
#define ALG_CFGS_BASE_DI_E(X, E)                            \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 2, E)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 2, E)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, E)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 2, E)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 3, E)
#define ALG_CFGS_BASE_UNI_E(X, E)                           \
    X(ALG_MODEL_UNICYCLE, 1, 2, E)                           \
    X(ALG_MODEL_UNICYCLE, 2, 2, E)                           \
    X(ALG_MODEL_UNICYCLE, 3, 2, E)                           \
    X(ALG_MODEL_UNICYCLE, 4, 2, E)
#define ALG_CFGS_BASE_DI(X) ALG_CFGS_BASE_DI_E(X, 0)
#define ALG_CFGS_BASE_UNI(X) ALG_CFGS_BASE_UNI_E(X, 0)
#define ALG_CFGS_BASE_SCEN_DI(X) ALG_CFGS_BASE_DI_E(X, 2)
#define ALG_CFGS_BASE_SCEN_UNI(X) ALG_CFGS_BASE_UNI_E(X, 2)
#define ALG_CFGS_BASE(X) ALG_CFGS_BASE_DI(X) ALG_CFGS_BASE_UNI(X)
#define ALG_CFGS_BASE_SCEN(X) ALG_CFGS_BASE_SCEN_DI(X) ALG_CFGS_BASE_SCEN_UNI(X)
#define ALG_CFGS_EXT_DI(X)                                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 2, 1)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 2, 1)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, 1)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 2, 1)
#define ALG_CFGS_EXT_UNI(X)                                 \
    X(ALG_MODEL_UNICYCLE, 1, 2, 1)                           \
    X(ALG_MODEL_UNICYCLE, 2, 2, 1)                           \
    X(ALG_MODEL_UNICYCLE, 3, 2, 1)                           \
    X(ALG_MODEL_UNICYCLE, 4, 2, 1)
#define ALG_CFGS_EXT_BIC(X)                                 \
    X(ALG_MODEL_BICYCLE, 1, 2, 1)                            \
    X(ALG_MODEL_BICYCLE, 2, 2, 1)                            \
    X(ALG_MODEL_BICYCLE, 3, 2, 1)                            \
    X(ALG_MODEL_BICYCLE, 4, 2, 1)
#define ALG_CFGS_EXT_DI3(X)                                 \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 3, 1)
// QuadrotorGame (quadrotor.jl:22: p <= 4), dense Newton direction
#define ALG_CFGS_QUAD(X)                                    \
    X(ALG_MODEL_QUADROTOR, 1, 3, 0)                          \
    X(ALG_MODEL_QUADROTOR, 2, 3, 0)                          \
    X(ALG_MODEL_QUADROTOR, 3, 3, 0)                          \
    X(ALG_MODEL_QUADROTOR, 4, 3, 0)
#define ALG_CFGS_QUAD_EXT(X)                                \
    X(ALG_MODEL_QUADROTOR, 1, 3, 1)                          \
    X(ALG_MODEL_QUADROTOR, 2, 3, 1)                          \
    X(ALG_MODEL_QUADROTOR, 3, 3, 1)                          \
    X(ALG_MODEL_QUADROTOR, 4, 3, 1)
// DoubleIntegrator in three dimensions with p = 1, 3, 4 (n = 6, 18, 24: dense Newton direction)
#define ALG_CFGS_DI3D(X)                                    \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 3, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 3, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 3, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 3, 1)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 3, 1)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 3, 1)
// DoubleIntegratorGame(p, d = 1) (double_integrator.jl:13-25 takes any d; round 6): n = 2 p, m = p.  px[i] = (i, i + p) is (position, velocity) of
// player i here -- the reference's index sets do not depend on d -- and the collision terms act on that pair as they do in the reference.
// p = 2, 4 take the tile path, p = 1, 3 (n = 2, 6) the dense direction; base constraint set
#define ALG_CFGS_DI1(X)                                     \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 1, 1, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 2, 1, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 1, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 1, 0)
// Five and six players (n = 20 / 24: dense Newton direction).  The reference itself caps p at 10 (options.jl:68)
#define ALG_CFGS_P5(X)                                      \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 5, 2, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 5, 2, 1)                  \
    X(ALG_MODEL_UNICYCLE, 5, 2, 0)                           \
    X(ALG_MODEL_UNICYCLE, 5, 2, 1)                           \
    X(ALG_MODEL_BICYCLE, 5, 2, 1)
#define ALG_CFGS_P6(X)                                      \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 6, 2, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 6, 2, 1)                  \
    X(ALG_MODEL_UNICYCLE, 6, 2, 0)                           \
    X(ALG_MODEL_UNICYCLE, 6, 2, 1)                           \
    X(ALG_MODEL_BICYCLE, 6, 2, 1)
#define ALG_CFGS_P56(X) ALG_CFGS_P5(X) ALG_CFGS_P6(X)
// Seven to nine players (round 6; n = 28 ... 36, m = 14 ... 18: the dense direction with the value matrices of all players LDS-resident --
// 65 / 93 / 128 KB of the CU's 160, one game per CU).  Ten players (the reference's cap, options.jl:68):
// 131 KB of value matrices, the step's workspace in the TIGHT layout of DirLds<C, true> -- 161 KB.
#define ALG_CFGS_PN(X, N)                                   \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, N, 2, 0)                  \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, N, 2, 1)                  \
    X(ALG_MODEL_UNICYCLE, N, 2, 0)                           \
    X(ALG_MODEL_UNICYCLE, N, 2, 1)                           \
    X(ALG_MODEL_BICYCLE, N, 2, 1)
#define ALG_CFGS_P7(X) ALG_CFGS_PN(X, 7)
#define ALG_CFGS_P8(X) ALG_CFGS_PN(X, 8)
#define ALG_CFGS_P9(X) ALG_CFGS_PN(X, 9)
#define ALG_CFGS_P10(X) ALG_CFGS_PN(X, 10)
#define ALG_CFGS_P789(X) ALG_CFGS_P7(X) ALG_CFGS_P8(X) ALG_CFGS_P9(X) ALG_CFGS_P10(X)
#define ALG_CFGS_DENSE(X) ALG_CFGS_QUAD(X) ALG_CFGS_QUAD_EXT(X) ALG_CFGS_DI3D(X) ALG_CFGS_P56(X) ALG_CFGS_P789(X)
#define ALG_CFGS_EXT(X) ALG_CFGS_EXT_DI(X) ALG_CFGS_EXT_UNI(X) ALG_CFGS_EXT_BIC(X) ALG_CFGS_EXT_DI3(X)
// every one-wavefront configuration of the library, in the order the host's declarations and dispatch_cfg walk them (algames_hip.hip)
#define ALG_CFGS_ONE(X) ALG_CFGS_BASE(X) ALG_CFGS_BASE_SCEN(X) ALG_CFGS_EXT(X) ALG_CFGS_DENSE(X) ALG_CFGS_DI1(X)

// every kernel of one instantiation; PREFIX is `template` (definition) or `extern template` (declaration)
#define ALG_INSTANTIATE_KERNELS(PREFIX, M, P, D, E)                                                                        \
    PREFIX __global__ void k_newton_solve<Cfg<M, P, D, E>>(Params, int, uint64_t);                                \
    PREFIX __global__ void k_newton_step<Cfg<M, P, D, E>>(Params, int, int, const double*, alg_step_info*);                      \
    PREFIX __global__ void k_residual<Cfg<M, P, D, E>>(Params, int, double, double*);                    \
    PREFIX __global__ void k_jacobian<Cfg<M, P, D, E>>(Params, double, double*, int);                             \
    PREFIX __global__ void k_direction<Cfg<M, P, D, E>>(Params, double, int*);                                    \
    PREFIX __global__ void k_line_search<Cfg<M, P, D, E>>(Params, double, const double*, double*, int*);          \
    PREFIX __global__ void k_update<Cfg<M, P, D, E>>(Params, int, int, const double*);                            \
    PREFIX __global__ void k_record<Cfg<M, P, D, E>>(Params, alg_record*);                                        \
    PREFIX __global__ void k_dual_update<Cfg<M, P, D, E>>(Params);                                                \
    PREFIX __global__ void k_init<Cfg<M, P, D, E>>(Params, uint64_t, int, int, int);                              \
    PREFIX __global__ void k_ibr<Cfg<M, P, D, E>>(Params, int, int, int, uint64_t, int, IbrOrder, double);        \
    PREFIX __global__ void k_mpc_advance<Cfg<M, P, D, E>>(Params);                                                \
    PREFIX __global__ void k_mpc_loop<Cfg<M, P, D, E>>(Params, int, uint64_t, double*);
// Team kernels (Cfg::NW wavefronts per game, small batches): X(model, p, d, ext, nw).  Only the fused solver and the fused
// receding-horizon loop exist in this shape; the step-wise entry points always use one wavefront per game.
#define ALG_CFGS_MW_E(X, E)                                 \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, E, 4)               \
    X(ALG_MODEL_UNICYCLE, 3, 2, E, 4)                        \
    X(ALG_MODEL_UNICYCLE, 4, 2, E, 2)                        \
    X(ALG_MODEL_UNICYCLE, 4, 2, E, 4)
#define ALG_CFGS_MW(X) ALG_CFGS_MW_E(X, 0)
// ... and their twins that read the game's scenario block
#define ALG_CFGS_MW_SCEN(X) ALG_CFGS_MW_E(X, 2)
// Team kernels of the dense-direction configurations: where the LDS footprint leaves room for few
// workgroups per CU at any batch size the automatic choice is the team of four regardless of the batch (team_width, algames_hip.hip)
#define ALG_CFGS_MW_DENSE(X)                                \
    X(ALG_MODEL_QUADROTOR, 2, 3, 0, 4)                       \
    X(ALG_MODEL_QUADROTOR, 3, 3, 0, 4)                       \
    X(ALG_MODEL_QUADROTOR, 4, 3, 0, 4)                       \
    X(ALG_MODEL_QUADROTOR, 2, 3, 1, 4)                       \
    X(ALG_MODEL_QUADROTOR, 3, 3, 1, 4)                       \
    X(ALG_MODEL_QUADROTOR, 4, 3, 1, 4)                       \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 3, 0, 4)               \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 3, 0, 4)               \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 3, 1, 4)               \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 4, 3, 1, 4)
#define ALG_INSTANTIATE_MW(PREFIX, M, P, D, E, W)                                                                         \
    PREFIX __global__ void k_newton_solve<Cfg<M, P, D, E, W>>(Params, int, uint64_t);                                     \
    PREFIX __global__ void k_mpc_loop<Cfg<M, P, D, E, W>>(Params, int, uint64_t, double*);
// Hand-off pairs: X(model, p, d, ext, w) = the budgeted one-wavefront kernel of (model, p, d, ext) parks, the team kernel of width w resumes
// (base configurations that have a team kernel in ALG_CFGS_MW)
#define ALG_CFGS_HANDOFF_E(X, E)                            \
    X(ALG_MODEL_DOUBLE_INTEGRATOR, 3, 2, E, 4)               \
    X(ALG_MODEL_UNICYCLE, 3, 2, E, 4)                        \
    X(ALG_MODEL_UNICYCLE, 4, 2, E, 4)
#define ALG_CFGS_HANDOFF(X) ALG_CFGS_HANDOFF_E(X, 0)
#define ALG_CFGS_HANDOFF_SCEN(X) ALG_CFGS_HANDOFF_E(X, 2)
#define ALG_INSTANTIATE_HO_PARK(PREFIX, M, P, D, E, W) PREFIX __global__ void k_newton_solve_ho<Cfg<M, P, D, E>>(Params, int, uint64_t, int);
#define ALG_INSTANTIATE_HO_RESUME(PREFIX, M, P, D, E, W) PREFIX __global__ void k_newton_resume<Cfg<M, P, D, E, W, 0>>(Params);
#define ALG_DEFINE_HO_RESUME(M, P, D, E, W) ALG_INSTANTIATE_HO_RESUME(template, M, P, D, E, W)
#define ALG_DECLARE_HO(M, P, D, E, W) ALG_INSTANTIATE_HO_PARK(extern template, M, P, D, E, W) ALG_INSTANTIATE_HO_RESUME(extern template, M, P, D, E, W)
#define ALG_DEFINE_MW(M, P, D, E, W) ALG_INSTANTIATE_MW(template, M, P, D, E, W)
#define ALG_DECLARE_MW(M, P, D, E, W) ALG_INSTANTIATE_MW(extern template, M, P, D, E, W)
#define ALG_DEFINE_KERNELS(M, P, D, E) ALG_INSTANTIATE_KERNELS(template, M, P, D, E)
#define ALG_DECLARE_KERNELS(M, P, D, E) ALG_INSTANTIATE_KERNELS(extern template, M, P, D, E)
// The solves with violation profiles (k_newton_solve_vio): one per solve kernel of the lists above except seven to ten players, in the unit of
// the solve kernel itself (ALG_DEFINE_KERNELS_VIO / ALG_DEFINE_MW_VIO = the family's kernels plus the sibling; the build's table of families
// names them for every family that has the sibling).  ALG_VIO_ONE: the one-wavefront configurations that have one, for the host's declarations.
#define ALG_INSTANTIATE_VIO(PREFIX, M, P, D, E) PREFIX __global__ void history_vio::k_newton_solve_vio<Cfg<M, P, D, E>>(Params, int, uint64_t, double*, int);
#define ALG_INSTANTIATE_VIO_MW(PREFIX, M, P, D, E, W) PREFIX __global__ void history_vio::k_newton_solve_vio<Cfg<M, P, D, E, W>>(Params, int, uint64_t, double*, int);
#define ALG_DEFINE_KERNELS_VIO(M, P, D, E) ALG_DEFINE_KERNELS(M, P, D, E) ALG_INSTANTIATE_VIO(template, M, P, D, E)
#define ALG_DEFINE_MW_VIO(M, P, D, E, W) ALG_DEFINE_MW(M, P, D, E, W) ALG_INSTANTIATE_VIO_MW(template, M, P, D, E, W)
#define ALG_DECLARE_VIO(M, P, D, E) ALG_INSTANTIATE_VIO(extern template, M, P, D, E)
#define ALG_DECLARE_VIO_MW(M, P, D, E, W) ALG_INSTANTIATE_VIO_MW(extern template, M, P, D, E, W)
#define ALG_VIO_ONE(X) ALG_CFGS_BASE(X) ALG_CFGS_BASE_SCEN(X) ALG_CFGS_EXT(X) ALG_CFGS_QUAD(X) ALG_CFGS_QUAD_EXT(X) ALG_CFGS_DI3D(X) ALG_CFGS_P56(X) ALG_CFGS_DI1(X)
// The scheduled receding-horizon loops (k_mpc_loop_sched): one per loop kernel of the lists above, in units of their own
#define ALG_INSTANTIATE_SCHED(PREFIX, M, P, D, E) PREFIX __global__ void k_mpc_loop_sched<Cfg<M, P, D, E>>(Params, int, uint64_t, double*, MpcSched, MpcLoopLog, MpcPlant);
#define ALG_INSTANTIATE_SCHED_MW(PREFIX, M, P, D, E, W) PREFIX __global__ void k_mpc_loop_sched<Cfg<M, P, D, E, W>>(Params, int, uint64_t, double*, MpcSched, MpcLoopLog, MpcPlant);
#define ALG_DEFINE_SCHED(M, P, D, E) ALG_INSTANTIATE_SCHED(template, M, P, D, E)
#define ALG_DECLARE_SCHED(M, P, D, E) ALG_INSTANTIATE_SCHED(extern template, M, P, D, E)
#define ALG_DEFINE_SCHED_MW(M, P, D, E, W) ALG_INSTANTIATE_SCHED_MW(template, M, P, D, E, W)
// The step-wise plant knot (k_mpc_plant_advance): one per one-wavefront configuration (ALG_CFGS_ONE), in a unit of their own -- with the two
// cost kernels of algames_cost.hpp (k_player_cost, k_closed_loop_cost) and the two constraint kernels of algames_con.hpp (k_con_values,
// k_closed_loop_con): one wavefront per game for every handle, like the plant knot
#define ALG_INSTANTIATE_PLANT(PREFIX, M, P, D, E)                                                                          \
    PREFIX __global__ void k_mpc_plant_advance<Cfg<M, P, D, E>>(Params, int, MpcPlant);                                    \
    PREFIX __global__ void k_player_cost<Cfg<M, P, D, E>>(Params, int, double*, double*);                                  \
    PREFIX __global__ void k_closed_loop_cost<Cfg<M, P, D, E>>(Params, CostLoopArgs);                                      \
    PREFIX __global__ void k_con_values<Cfg<M, P, D, E>>(Params, int, double*);                                            \
    PREFIX __global__ void k_closed_loop_con<Cfg<M, P, D, E>>(Params, ConLoopArgs);
#define ALG_DEFINE_PLANT(M, P, D, E) ALG_INSTANTIATE_PLANT(template, M, P, D, E)
#define ALG_DECLARE_PLANT(M, P, D, E) ALG_INSTANTIATE_PLANT(extern template, M, P, D, E)
#define ALG_DECLARE_SCHED_MW(M, P, D, E, W) ALG_INSTANTIATE_SCHED_MW(extern template, M, P, D, E, W)
// The KKT column kernel (k_kkt_sens): one per configuration that has a k_direction, in units of their own
#define ALG_INSTANTIATE_KKT(PREFIX, M, P, D, E)                                                                            \
    PREFIX __global__ void k_kkt_sens<Cfg<M, P, D, E>>(Params, double, int, int, int, const double*, int, int, int, double*, int*);
#define ALG_DEFINE_KKT(M, P, D, E) ALG_INSTANTIATE_KKT(template, M, P, D, E)
#define ALG_DECLARE_KKT(M, P, D, E) ALG_INSTANTIATE_KKT(extern template, M, P, D, E)
