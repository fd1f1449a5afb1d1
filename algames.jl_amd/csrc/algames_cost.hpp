// algames_cost.hpp -- what a plan, or a closed-loop run, costs each player (alg_get_cost, alg_mpc_get_cost).
// The objective itself, not the augmented Lagrangian: constraints, multipliers and penalties do not enter.
//   J_i = sum_k w_k l_i(x_k, u_k),  w_k = dt (k < N), w_N = 1: the weights of the cost gradients (phase_a_pos_item, objective.jl:12-35)
//   l_i = [ state:     1/2 sum_a Q_i[a] (x[pz_i[a]] - xf_i[a])^2                                       (LQRCost, objective.jl:12-35)
//         | control:   1/2 sum_a R_i[a] (u[pu_i[a]] - uf_i[a])^2, 0 at the terminal knot
//         | collision: sum_{j != i} 1/2 mu_i max(0, r_i - |px_i - px_j|)^2, planar for every model ]   (CollisionCost, objective.jl:122-131)
// One wavefront per game, items (knot, player).  The lanes that carry items are the largest multiple of P in the wavefront (63 of 64 for three
// players), so a lane keeps its player over all of its trips: lane l owns player l % P and the knots l / P, l / P + L / P, ...  The P lanes of
// a knot read its [x | u] once between them -- entry a P + i of x and the mi doubles of u_i go to lane i: n + m contiguous doubles per knot, the
// multipliers behind them are never touched -- and take the other players' two position entries from the lines those loads brought in.
// The totals: every lane adds its items in trip order, the per-lane sums meet in a 3 x 64 LDS buffer, and lane (i, c) adds the sums of the lanes
// of player i in lane order.  The order of every sum is a function of the item index alone: a game's result does not depend on the batch.
// Non-finite input stays in its game and shows in its output (the positive part is taken with a comparison, which keeps a NaN).
#pragma once
#include "algames_device.hpp"

namespace alg {

template <class C> inline constexpr int cost_lanes_v = (WAVE / C::P) * C::P;

// player i's rows of the LQR numbers: Q, xf (ni each), R, uf (mi each).  Read where they are used -- the same few lines for every item of a
// lane, so they come from the vector L1 -- and not kept in registers over the trips: the quadrotor's 32 doubles would not fit the budget.
struct CostLqr { const double* Q; const double* xf; const double* R; const double* uf; };
// l_i(x, u) of one item, unweighted: o = [state, control, collision].  xs: the knot's joint state (n doubles); us: its joint control in the
// stored player-major order (m doubles), or null at the terminal knot; colcost: the handle carries a collision cost (mu, rad: player i's numbers)
template <class C>
__device__ __forceinline__ void player_stage_cost(const double* __restrict__ xs, const double* __restrict__ us, const CostLqr& q, const int i,
                                                  const bool colcost, const double mu, const double rad, double (&o)[3]) {
    constexpr int P = C::P, UN = C::ni <= 6 ? C::ni : 4;       // (the quadrotor's twelve entries, unrolled at once, spilled: 36 loads in flight)
    double s = 0.0, c = 0.0, cl = 0.0;
#pragma unroll UN
    for (int a = 0; a < C::ni; a++) { const double e = xs[a * P + i] - q.xf[a]; s += q.Q[a] * (e * e); }
    if (us) {
#pragma unroll
        for (int a = 0; a < C::mi; a++) { const double e = us[i * C::mi + a] - q.uf[a]; c += q.R[a] * (e * e); }
    }
    if (P > 1 && colcost) {
        const double x0 = xs[i], x1 = xs[P + i];
#pragma unroll
        for (int jj = 0; jj < P - 1; jj++) {
            const int j = jj < i ? jj : jj + 1;
            const double gap = rad - sqrt(pair_dist2(x0 - xs[j], x1 - xs[P + j]));
            const double pen = gap < 0.0 ? 0.0 : gap;                    // max(0, gap) that keeps a NaN
            cl += (0.5 * mu) * (pen * pen);
        }
    }
    o[0] = 0.5 * s; o[1] = 0.5 * c; o[2] = cl;
}

// the per-lane sums of a game -> total[(i, c)], lanes of player i in lane order
template <class C>
__device__ __forceinline__ void cost_reduce(double* __restrict__ red, const double (&acc)[3], const int lane, double* __restrict__ total) {
    constexpr int P = C::P, L = cost_lanes_v<C>;
#pragma unroll
    for (int c = 0; c < 3; c++) red[lane * 3 + c] = acc[c];
    __syncthreads();
    if (total && lane < 3 * P) {
        const int i = lane / 3, c = lane % 3;
        double s = 0.0;
        for (int l = i; l < L; l += P) s += red[l * 3 + c];
        total[lane] = s;
    }
}

} // namespace alg

// The plan in ALG_TRAJ_PD or ALG_TRAJ_TRIAL.  total: B x p x 3 or null; stage: B x N x p x 3 (w_k applied) or null.
template <class C>
__global__ void __launch_bounds__(alg::WAVE, 4) k_player_cost(alg::Params pr_arg, int which, double* total, double* stage) {
    using namespace alg;
    __shared__ double red[WAVE * 3];
    CPR pr = kernel_params();
    constexpr int P = C::P, L = cost_lanes_v<C>, KPT = L / P;              // KPT knots per trip
    const int g = blockIdx.x, lane = game_tid(), N = pr.N, i = lane % P;
    Game G = game_view(pr, g);
    double acc[3] = {0.0, 0.0, 0.0};
    if (lane < L) {
        const double* __restrict__ z = G.z(which);
        const bool colcost = pr.has_colcost != 0;
        const double mu = colcost ? scen_player<C, P>(pr, G, pr.cc_mu, SC_CCM, i, [](int q) { return q; }) : 0.0;
        const double rad = colcost ? scen_player<C, P>(pr, G, pr.cc_radius, SC_CCR, i, [](int q) { return q; }) : 0.0;
        const CostLqr q{G.Qd(pr) + i * C::ni, G.xf(pr) + i * C::ni, G.Rd(pr) + i * C::mi, G.uf(pr) + i * C::mi};
        double* const so = stage ? as_global(stage) + (size_t)g * N * (P * 3) : nullptr;
        for (int k = lane / P; k < N; k += KPT) {
            const bool last = k == N - 1;
            const double* xs = zstate<C>(z, k);
            double l[3];
            player_stage_cost<C>(xs, last ? nullptr : z + C::n + hu<C>(k, 0), q, i, colcost, mu, rad, l);
            const double w = last ? 1.0 : pr.dt;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double v = w * l[c];
                acc[c] += v;
                if (so) so[(k * P + i) * 3 + c] = v;
            }
        }
    }
    cost_reduce<C>(red, acc, lane, total ? as_global(total) + (size_t)g * (P * 3) : nullptr);
}

// The log of a fused receding-horizon loop (mpc_solve_impl's states and controls, device-resident): items (plant knot q, player), running
// cost dt l_i(states[q], controls[q]) with the targets / collision-cost numbers of the schedule row solve t = q / hold used (the last row is
// held), else the game's.  stage: knots x B x p x 3; total: B x p x 3.  No terminal term: states[knots] is not costed.
struct CostLoopArgs {
    const double* states;       // (knots + 1) x B x n
    const double* controls;     // knots x B x m, stored player-major order
    const double* tgt;          // ALG_SCHED_LQR_TARGET rows: rows x B x (p ni + p mi), or null
    const double* cc;           // ALG_SCEN_COLLISION_COST rows: rows x B x 2 p [radius | mu], or null
    double* stage;
    double* total;
    int knots, hold, tgt_rows, cc_rows;
};
template <class C>
__global__ void __launch_bounds__(alg::WAVE, 4) k_closed_loop_cost(alg::Params pr_arg, CostLoopArgs a) {
    using namespace alg;
    __shared__ double red[WAVE * 3];
    CPR pr = kernel_params();
    constexpr int P = C::P, L = cost_lanes_v<C>, KPT = L / P;
    const int g = blockIdx.x, lane = game_tid(), B = pr.B, i = lane % P;
    Game G = game_view(pr, g);
    double acc[3] = {0.0, 0.0, 0.0};
    if (lane < L) {
        const bool colcost = pr.has_colcost != 0;
        double mu = 0.0, rad = 0.0;
        if (colcost && !a.cc) {
            mu = scen_player<C, P>(pr, G, pr.cc_mu, SC_CCM, i, [](int q) { return q; });
            rad = scen_player<C, P>(pr, G, pr.cc_radius, SC_CCR, i, [](int q) { return q; });
        }
        CostLqr q{G.Qd(pr) + i * C::ni, G.xf(pr) + i * C::ni, G.Rd(pr) + i * C::mi, G.uf(pr) + i * C::mi};
        const double dt = pr.dt;
        for (int kq = lane / P; kq < a.knots; kq += KPT) {
            const int t = kq / a.hold;
            if (a.tgt) {
                const int row = t < a.tgt_rows ? t : a.tgt_rows - 1;
                const double* r = as_global(a.tgt) + ((size_t)row * B + g) * (P * (C::ni + C::mi));
                q.xf = r + i * C::ni; q.uf = r + P * C::ni + i * C::mi;
            }
            if (colcost && a.cc) {
                const int row = t < a.cc_rows ? t : a.cc_rows - 1;
                const double* r = as_global(a.cc) + ((size_t)row * B + g) * (2 * P);
                rad = r[i]; mu = r[P + i];
            }
            const size_t at = (size_t)kq * B + g;
            double l[3];
            player_stage_cost<C>(as_global(a.states) + at * C::n, as_global(a.controls) + at * C::m, q, i, colcost, mu, rad, l);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double v = dt * l[c];
                acc[c] += v;
                as_global(a.stage)[(at * P + i) * 3 + c] = v;
            }
        }
    }
    cost_reduce<C>(red, acc, lane, as_global(a.total) + (size_t)g * (P * 3));
}
