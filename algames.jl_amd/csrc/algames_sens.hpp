// algames_sens.hpp -- the KKT column kernel: J X = R for many right-hand sides, answered on the device.
// k_kkt_sens<C> is the one kernel behind alg_kkt_solve, alg_kkt_sensitivity and, through per-kind launches, alg_kkt_normal_equations: one
// assemble pass at pdtraj, then per column a loader, the structured elimination of refined_direction and a store.
//   the loader writes the column's right-hand side into the three right-hand-side blocks of the step records (Rec::RX / RU / RD) of all
//   N - 1 steps -- the blocks the refinement's correction solves already rewrite (dir_urow_residual<..., WRITE>).  The sweeps solve
//   J d = -record, so a column of J X = R is stored negated and a column of X = -J^-1 (d res / d theta) v as sum_c v_c d res / d theta_c.
//   the store copies the blocks of the requested steps only: out holds n_steps * b doubles per column (all N - 1 steps: the S doubles behind
//   the x_1 slot of the delta buffer, horizontal order).
// The right-hand-side kinds (the param argument):
//   SENS_RHS_USER  the caller's column of S doubles, in the vertical order of alg_residual (alg_kkt_solve's ALG_KKT_RHS_USER): J X = R.  A
//                  plain sign flip per entry: with R = -res the records hold what k_direction's hold, bit for bit.
//   ALG_PARAM_*    d res / d theta built here, evaluated at pdtraj with the game's multipliers and penalties and the numbers the game was
//                  assembled with (per-game LQR data, the game's scenario block or the handle's values, through ALG_SCEN_AT).  A unit column
//                  is v = e_c, formed without a direction in memory.  ALG_KKT_RHS_X0 / XF of alg_kkt_solve are the unit columns of
//                  ALG_PARAM_X0 / XF.
// The terms, row by row of the oracle's residual (w_k = dt, 1 on the terminal step -- the stage / terminal weight jacobian_dense hands to
// qhat_entry; joint state index s = a P + j is entry a of player j):
//   X0   rd of step 0:            A_0[:, c]  (A_entry on the coefficient block of record 0)
//   XF   rx_i[a P + i]:           -w_k Q_i[a]  (the xf order of alg_set_lqr)
//   Q    rx_i[a P + i]:           w_k (x - xf_i[a])
//   R    ru[c]:                   dt (u - uf)                  UF  ru[c]: -dt R
//   COLLISION_COST  rx_i at the positions of i and j, pairs with r_i - |d| > 0 only, g_a = mu_i (r_i (eps + d_a) / (eps_n + |d|) - d_a):
//                   d g_a / d r_i = mu_i (eps + d_a) / (eps_n + |d|),  d g_a / d mu_i = g_a / mu_i;  -w_k at i, +w_k at j
//   COLLISION_RADIUS  rx_i at the positions of i and j: (-/+ 2 d_a) a mu 2 R_ij with a = (c >= 0) | (lambda > 0); three position entries where
//                   the spherical form was added
//   CONTROL_BOUND   ru[c]: -a mu of the row, per half; a row of an infinite bound has no term
// Flat loops over the entries of a block, one entry per lane and trip, vector stores only; every column rewrites all three blocks because a
// correction pass of the refinement zeroes rx / rd and overwrites ru.  No LDS beyond k_direction's.
#pragma once
#include "algames_device.hpp"

constexpr int SENS_RHS_USER = -1;           // internal: not an ALG_PARAM_* of the C ABI (alg_kkt_sensitivity and alg_param_len refuse it)

template <class C>
__device__ void sens_load_rhs(CPR pr0, const Game& G0, const int param, const int col, const double* const dir) {
    CPR pr = phase_params(pr0);
    const Game G = G0.fresh();
    constexpr int n = C::n, m = C::m, P = C::P, ni = C::ni, mi = C::mi;
    using R = Rec<C>;
    const int N = phase_int(pr.N), tid = phase_lane();
    const double dt = phase_f64(pr.dt);
    double* __restrict__ recs = G.rec(pr);
    const double* __restrict__ z = G.z(0);
    const double* __restrict__ dv = as_global(dir);
    auto v = [&](int c) -> double { return dir ? gld(dv, c) : (c == col ? 1.0 : 0.0); };
    // rx: rows opt_i,x_{k+1}, entry q = i n + s of the step
    for (int e = tid; e < (N - 1) * P * n; e += C::NT) {
        const int k = e / (P * n), q = e % (P * n), i = q / n, s = q % n, a = s / P, j = s % P;
        const double w = (k + 1 < N - 1) ? dt : 1.0;
        const double* __restrict__ x = z + n + hx<C>(k);
        if (param == SENS_RHS_USER) { gst(recs, k * R::LEN + R::RX + q, -gld(dv, vx<C>(N, i, k) + s)); continue; }
        double r = 0.0;
        if (param == ALG_PARAM_XF) {
            if (j == i) r = -(w * gld(G.Qd(pr), i * ni + a)) * v(i * ni + a);
        } else if (param == ALG_PARAM_Q) {
            if (j == i) r = (w * (gld(x, s) - gld(G.xf(pr), i * ni + a))) * v(i * ni + a);
        } else if (param == ALG_PARAM_COLLISION_COST) {
            if (P > 1 && a < 2) {
                const double rad = ALG_SCEN_AT(C, pr, G, cc_radius, SC_CCR, i), mu = ALG_SCEN_AT(C, pr, G, cc_mu, SC_CCM, i);
                const double vr = v(i), vm = v(P + i);
                const double xi0 = gld(x, i), xi1 = gld(x, P + i);
                for (int j2 = 0; j2 < P; j2++) {
                    if (j2 == i || (j != i && j2 != j)) continue;
                    const double dl0 = xi0 - gld(x, j2), dl1 = xi1 - gld(x, P + j2), nrm = sqrt(pair_dist2(dl0, dl1));
                    if (fmax(0.0, rad - nrm) > 0.0) {
                        const double eps = 1e-10, eps_norm = eps * sqrt((double)n);
                        const double dla = a == 0 ? dl0 : dl1, f = (eps + dla) / (eps_norm + nrm);
                        const double dg = vr * (mu * f) + vm * (rad * f - dla);
                        r += j == i ? -(w * dg) : w * dg;
                    }
                }
            }
        } else if (param == ALG_PARAM_COLLISION_RADIUS) {
            const int dim = (C::PD == 3 && pr.ca_dim == 3) ? 3 : 2;
            if (P > 1 && a < dim) {
                const double xi0 = gld(x, i), xi1 = gld(x, P + i), xi2 = dim == 3 ? gld(x, 2 * P + i) : 0.0;
                const unsigned mask = pr.ca_mask[i];
                for (int j2 = 0; j2 < P; j2++) {
                    if (j2 == i || (j != i && j2 != j)) continue;
                    const double dl0 = xi0 - gld(x, j2), dl1 = xi1 - gld(x, P + j2), dl2 = dim == 3 ? xi2 - gld(x, 2 * P + j2) : 0.0;
                    const double on = (double)((mask >> j2) & 1u);
                    const double Rr = ALG_SCEN_AT(C, pr, G, ca_pair_r, SC_CAR, i * MAXP + j2);
                    const double c = ca_value(on, Rr, __builtin_fma(dl2, dl2, pair_dist2(dl0, dl1)));
                    const int ci = con_col<C>(N, pairq<C>(i, j2), k + 1);
                    const double am = on * al_active_mu(c, gld(G.lam(pr), ci), gld(G.mu(pr), ci));
                    const double dla = a == 0 ? dl0 : (a == 1 ? dl1 : dl2);
                    const double t = v(i * P + j2) * ((2.0 * dla) * (am * (2.0 * Rr)));
                    r += j == i ? -t : t;
                }
            }
        }
        gst(recs, k * R::LEN + R::RX + q, r + 0.0);                 // (+ 0.0: a zero entry is +0 whatever the sign of its factors)
    }
    // ru: rows opt_i,u_{i,k}, joint control index c = jc P + i
    for (int e = tid; e < (N - 1) * m; e += C::NT) {
        const int k = e / m, c = e % m, i = c % P, jc = c / P, pi = i * mi + jc;
        if (param == SENS_RHS_USER) { gst(recs, k * R::LEN + R::RU + c, -gld(dv, vu<C>(N, i, k) + jc)); continue; }
        double r = 0.0;
        if (param == ALG_PARAM_R || param == ALG_PARAM_UF || param == ALG_PARAM_CONTROL_BOUND) {
            const double u = gld(z, n + hu<C>(k, i) + jc);
            if (param == ALG_PARAM_R) r = (dt * (u - gld(G.uf(pr), pi))) * v(pi);
            else if (param == ALG_PARAM_UF) r = -(dt * gld(G.Rd(pr), pi)) * v(pi);
            else {
                for (int half = 0; half < 2; half++) {
                    const int ci = con_ctl<C>(pr, k, half * m + c);
                    const double cv = half == 0 ? u - ALG_SCEN_AT(C, pr, G, umax, SC_UMAX, c) : ALG_SCEN_AT(C, pr, G, umin, SC_UMIN, c) - u;
                    if (isfinite(cv)) r -= al_active_mu(cv, gld(G.lam(pr), ci), gld(G.mu(pr), ci)) * v(half * m + c);
                }
            }
        }
        gst(recs, k * R::LEN + R::RU + c, r + 0.0);
    }
    // rd: the dynamics rows; x_1 enters step 0 alone
    for (int e = tid; e < (N - 1) * n; e += C::NT) {
        const int k = e / n, row = e % n;
        if (param == SENS_RHS_USER) { gst(recs, k * R::LEN + R::RD + row, -gld(dv, vd<C>(N, k) + row)); continue; }
        double r = 0.0;
        if (param == ALG_PARAM_X0 && k == 0) {
            if (!dir) r = A_entry<C>(recs + R::COEF, dt, row, col);
            else for (int c = 0; c < n; c++) r += A_entry<C>(recs + R::COEF, dt, row, c) * gld(dv, c);
        }
        gst(recs, k * R::LEN + R::RD + row, r + 0.0);
    }
}
// the column's solution, steps step0 .. step0 + nstep - 1 only: nstep blocks of b doubles of the delta buffer, horizontal order
template <class C>
__device__ void sens_store_column(CPR pr0, const Game& G0, double* const dst, const int step0, const int nstep) {
    const Game G = G0.fresh();
    const int cnt = phase_int(nstep) * C::b, tid = phase_lane();
    const double* __restrict__ dz = G.z(2) + C::n + phase_int(step0) * C::b;
    double* __restrict__ o = as_global(dst);
    for (int e = tid; e < cnt; e += C::NT) gst(o, e, gld(dz, e));
}
// One wavefront per game, games g0 .. g0 + gridDim.x - 1.  dirs: gridDim.x x ncol x len, or null: ncol = len unit columns (SENS_RHS_USER: the columns themselves, len = S).  out: gridDim.x x
// ncol x (nstep b); status: the first non-OK status of the game's columns.  Arguments are re-read from the kernel-argument segment where
// they are used, like k_mpc_loop's; only the column counter and the status live across the columns.
struct SensArgs { Params pr; double reg; int param, ncol, len; const double* dirs; int g0, step0, nstep; double* out; int* status; };
template <class C>
__global__ void __launch_bounds__(WAVE, C::WPE) k_kkt_sens(Params pr_arg, double reg_arg, int param_arg, int ncol_arg, int len_arg, const double* dirs_arg, int g0_arg,
                                                           int step0_arg, int nstep_arg, double* out_arg, int* status_arg) {
    __shared__ Lds<C> L;
    CPR pr = kernel_params();
#if defined(__HIP_DEVICE_COMPILE__)
    const ALG_AS4 SensArgs& ka = *(const ALG_AS4 SensArgs*)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const SensArgs& ka = *(const SensArgs*)nullptr;      // host pass: never executed
#endif
    auto kq = [&]() -> const ALG_AS4 SensArgs& { return *(const ALG_AS4 SensArgs*)uniform_u64((unsigned long long)&ka); };
    const int gl = blockIdx.x;
    Game G = game_view(pr, gl + kq().g0);
    ResOut ro;
    assemble_pass<C, 1>(pr, G, L.a, 0, -1, 0.0, kq().reg, ro);
    __syncthreads();
    int worst = ALG_STATUS_OK;
    for (int r = 0; r < kq().ncol; r++) {
        const size_t at = (size_t)phase_int(gl) * kq().ncol + r;
        const double* const src = kq().dirs;
        sens_load_rhs<C>(pr, G, kq().param, r, src ? src + at * (size_t)kq().len : nullptr);
        game_sync();
        const int st = refined_direction<C, false, false>(pr, G, L, kq().reg, -1, nullptr);
        if (worst == ALG_STATUS_OK) worst = st;
        game_sync();
        sens_store_column<C>(pr, G, kq().out + at * ((size_t)kq().nstep * C::b), kq().step0, kq().nstep);
        game_sync();
    }
    int* const so = kq().status;
    if (so && phase_lane() == 0) as_global(so)[phase_int(gl)] = worst;
}
