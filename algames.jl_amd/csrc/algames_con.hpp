// algames_con.hpp -- the constraint values of a plan, or of a closed-loop run, row by row (alg_get_con_values, alg_mpc_get_con).
// evaluate!(game_con, traj) (constraints_methods.jl:329-379) without the dual and penalty update that alg_dual_penalty_update performs with it:
// c <= 0 is feasible, a row of an infinite bound reports -inf, an inert row (a pair never added, a table entry whose player bit is clear) 0.
// Every block of the ABI's constraint vector is per step, so con_len = (N - 1) K1 with the K1 rows of one step in the ABI's block order:
//   [ pair q = 0 .. p(p-1)-1 | u - u_max (m) | u_min - u (m) | per player: (x - x_max)(n), (x_min - x)(n) | per player: walls | per player: circles
//     | per player: 3-D walls | per player: cylinders ]                                                      (the blocks alg_get_con_len counts)
// A step pairs (u_k, x_{k+1}): the control-bound rows read the control of the step, every other row the state the step reaches.
// One wavefront per game, items (knot, row) flattened: item e = knot K1 + row goes to lane e % 64 of trip e / 64.  A lane loads the one to
// six entries of the knot's [x | u] its row needs; the lanes of a trip that share a knot ask for the same lines together, so a knot's lines
// come in once per trip and not once per row.  In the closed-loop log (knots x B x K1) the items of a trip that share a knot are stored side
// by side; in a plan they go to their places in the ABI's layout.  The rows are evaluated by the device functions of the assemble passes
// (pair_dist2, ca_value, wall_val, circ_val, wall3_val, cyl_val, the ext_* accessors, ALG_SCEN_AT); dual_penalty_update's own expressions.
// No LDS.  Lane and trip of an item depend on the item alone, and the summary of a run (worst, first) is a maximum and a minimum: a game's
// output does not depend on the batch, bit for bit.  Non-finite input stays in its game (the maximum is taken with comparisons that keep a NaN).
#pragma once
#include "algames_device.hpp"

namespace alg {

__device__ __forceinline__ double con_max_nan(double a, double b) { return (a != a || a > b) ? a : b; }    // a NaN on either side stays
__device__ __forceinline__ int wave_min_i32(int v) {
    { const auto a = __builtin_amdgcn_permlane32_swap(v, v, false, false); v = min(a[0], a[1]); }
    { const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false); v = min(a[0], a[1]); }
    v = min(v, dpp_i32<0x128>(v)); v = min(v, dpp_i32<0x124>(v)); v = min(v, dpp_i32<0x122>(v)); v = min(v, dpp_i32<0x121>(v));
    return v;
}

// Row r of step k (0-based: control u_k, state x_{k+1}).  x: the n doubles of the state, u: the m doubles of the control in the stored
// player-major order.  sched(kind, len): the schedule row of an ALG_CON_* kind this knot's solve used (len doubles per game, the caller's order
// of alg_mpc_set_schedule), or null: the game's block / the handle's values.  kind: the row's ALG_CON_* kind, -1 for a row of a base block
// that was not added (it reports 0 and counts for no kind); abi: the row's place in the ABI's constraint layout.
template <class C, class S>
__device__ __forceinline__ double con_row(CPR pr, const Game& G, S&& sched, const double* __restrict__ x, const double* __restrict__ u,
                                          int r, const int k, int& kind, int& abi) {
    constexpr int n = C::n, m = C::m, P = C::P, NP = C::NPAIR;
    const int K = pr.N - 1;
    if constexpr (P > 1) {
        if (r < NP) {
            const int i = r / (P - 1), jj = r % (P - 1), j = jj < i ? jj : jj + 1;
            abi = r * K + k; kind = pr.has_colavoid ? ALG_CON_COLLISION : -1;
            if (!pr.has_colavoid) return 0.0;
            const double on = (double)((pr.ca_mask[i] >> j) & 1u);
            double R = ALG_SCEN_AT(C, pr, G, ca_pair_r, SC_CAR, i * MAXP + j);
            if (const double* row = sched(ALG_CON_COLLISION, P * P); row && on != 0.0) R = row[i * P + j];     // (entries of pairs never added are ignored, as the loop ignores them)
            double s2 = pair_dist2(x[i] - x[j], x[P + i] - x[P + j]);
            if constexpr (C::PD == 3) { const double d2 = pr.ca_dim == 3 ? x[2 * P + i] - x[2 * P + j] : 0.0; s2 = __builtin_fma(d2, d2, s2); }
            return ca_value(on, R, s2);
        }
    }
    r -= NP;
    if (r < 2 * m) {
        const int c = r < m ? r : r - m;
        abi = pr.col_len + k * 2 * m + r; kind = pr.has_ctl ? ALG_CON_CONTROL : -1;
        if (!pr.has_ctl) return 0.0;
        const double uv = u[uoff<C>(c)];
        const double* row = sched(ALG_CON_CONTROL, 2 * m);
        if (r < m) return uv - (row ? row[c] : ALG_SCEN_AT(C, pr, G, umax, SC_UMAX, c));
        return (row ? row[m + c] : ALG_SCEN_AT(C, pr, G, umin, SC_UMIN, c)) - uv;
    }
    if constexpr (C::EXT) {
        r -= 2 * m;
        const double* ec = scen_ext(pr, G);
        const int nsb = pr.has_sb ? 2 * n : 0;
        if (r < P * nsb) {
            const int i = r / (2 * n), row = r - i * 2 * n;
            abi = ext_sb_row(pr, i, k, row); kind = ALG_CON_STATE;
            const double* sr = sched(ALG_CON_STATE, 2 * P * n);
            if (row < n) return x[row] - (sr ? sr : ext_sbmax(pr, ec))[i * n + row];
            return (sr ? sr + P * n : ext_sbmin(pr, ec))[i * n + row - n] - x[row - n];
        }
        r -= P * nsb;
        if (r < P * pr.nwall) {
            const int i = r / pr.nwall, w = r - i * pr.nwall;
            abi = ext_wall_row(pr, i, k, w); kind = ALG_CON_WALL;
            const double on = (double)((pr.wall_mask[i] >> w) & 1u);
            double gx, gy;
            if (const double* row = sched(ALG_CON_WALL, 6 * pr.nwall)) {          // the caller's entry (x1 y1 x2 y2 xv yv) as a table of one wall
                double W1[5 * ALG_MAX_WALLS + 1];
#pragma unroll
                for (int f = 0; f < 6; f++) W1[f * ALG_MAX_WALLS] = row[6 * w + f];
                return on * wall_val(W1, 0, x[i], x[P + i], &gx, &gy);
            }
            return on * wall_val(ext_walls(pr, ec), w, x[i], x[P + i], &gx, &gy);
        }
        r -= P * pr.nwall;
        if (r < P * pr.ncirc) {
            const int i = r / pr.ncirc, c = r - i * pr.ncirc;
            abi = ext_circ_row(pr, i, k, c); kind = ALG_CON_CIRCLE;
            const double on = (double)((pr.circ_mask[i] >> c) & 1u);
            double gx, gy;
            if (const double* row = sched(ALG_CON_CIRCLE, 3 * pr.ncirc)) {        // (xc yc r) as a table of one circle
                double C1[2 * ALG_MAX_CIRCLES + 1];
#pragma unroll
                for (int f = 0; f < 3; f++) C1[f * ALG_MAX_CIRCLES] = row[3 * c + f];
                return on * circ_val(C1, 0, x[i], x[P + i], &gx, &gy);
            }
            return on * circ_val(ext_circs(pr, ec), c, x[i], x[P + i], &gx, &gy);
        }
        if constexpr (C::PD == 3) {
            r -= P * pr.ncirc;
            if (r < P * pr.nwall3) {
                const int i = r / pr.nwall3, q = r - i * pr.nwall3;
                abi = ext_wall3_row(pr, i, k, q); kind = ALG_CON_WALL3D;
                const double pos[3] = {x[i], x[P + i], x[2 * P + i]}; double g3[3];
                const double* row = sched(ALG_CON_WALL3D, 12 * pr.nwall3);          // the table's own order: p1 p2 p3 v
                return (double)((pr.wall3_mask[i] >> q) & 1u) * wall3_val(row ? row : ext_walls3(pr, ec), q, pos, g3);
            }
            r -= P * pr.nwall3;
            if (r < P * pr.ncyl) {
                const int i = r / pr.ncyl, q = r - i * pr.ncyl;
                abi = ext_cyl_row(pr, i, k, q); kind = ALG_CON_CYLINDER;
                const double pos[3] = {x[i], x[P + i], x[2 * P + i]}; double g3[3];
                const double on = (double)((pr.cyl_mask[i] >> q) & 1u);
                const double* Y = ext_cyls(pr, ec);
                if (const double* row = sched(ALG_CON_CYLINDER, 5 * pr.ncyl)) {    // (p l r) of the caller with the handle's axis
                    const double Y1[6] = {row[5 * q], row[5 * q + 1], row[5 * q + 2], Y[6 * q + 3], row[5 * q + 3], row[5 * q + 4]};
                    return on * cyl_val(Y1, 0, pos, g3);
                }
                return on * cyl_val(Y, q, pos, g3);
            }
        }
    }
    abi = -1; kind = -1;        // not reached: r < K1
    return 0.0;
}

} // namespace alg

// The plan in ALG_TRAJ_PD or ALG_TRAJ_TRIAL.  vals: B x con_len, the ABI's constraint layout.
template <class C>
__global__ void __launch_bounds__(alg::WAVE, 4) k_con_values(alg::Params pr_arg, int which, double* vals) {
    using namespace alg;
    CPR pr = kernel_params();
    const int g = blockIdx.x, lane = game_tid(), K = pr.N - 1, K1 = pr.con_len / K, items = K * K1;
    Game G = game_view(pr, g);
    const double* __restrict__ z = which == ALG_TRAJ_PD ? G.z(0) : G.z(1);      // (G.zo[which] would park the view in LDS: a dynamic index into it)
    double* const out = as_global(vals) + (size_t)g * pr.con_len;
    for (int e = lane; e < items; e += WAVE) {
        const int k = e / K1, r = e - k * K1;
        const double* xu = z + C::n + hx<C>(k);                    // [x_{k+1} | u_k | ...] of step k
        int kind, abi;
        const double c = con_row<C>(pr, G, [](int, int) -> const double* { return nullptr; }, xu, xu + C::n, r, k, kind, abi);
        if (abi >= 0) out[abi] = c;
    }
}

// The log of a fused receding-horizon loop (mpc_solve_impl's states and controls, device-resident): items (plant knot q, row), the control
// rows on controls[q], every other row on states[q + 1], with the numbers of the schedule row solve t = q / hold used (the last row is held),
// else the game's.  vals: knots x B x K1; worst: B x 7 (maximum of the kind's rows over the run, -inf for a kind that was not added, NaN if
// a row is NaN); first: B x 7 (the first knot with a row that is not <= 0, -1 if none).
struct ConLoopArgs {
    const double* states;       // (knots + 1) x B x n
    const double* controls;     // knots x B x m, stored player-major order
    const double* sched[ALG_CON_KINDS];   // per ALG_CON_* kind: the rows of its schedule (rows x B x len, the caller's order), or null
    int rows[ALG_CON_KINDS];
    double* vals;
    double* worst;
    int* first;
    int knots, hold;
};
// The argument struct behind Params in the kernel-argument segment, read in place like Params itself (kernel_params)
__device__ __forceinline__ const ALG_AS4 ConLoopArgs& con_loop_args() {
    constexpr unsigned long AT = (sizeof(alg::Params) + alignof(ConLoopArgs) - 1) / alignof(ConLoopArgs) * alignof(ConLoopArgs);
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const ALG_AS4 ConLoopArgs*)((const ALG_AS4 char*)__builtin_amdgcn_kernarg_segment_ptr() + AT);
#else
    return *(const ALG_AS4 ConLoopArgs*)(unsigned long)(64 + AT);      // host pass: never executed
#endif
}
template <class C>
__global__ void __launch_bounds__(alg::WAVE, 4) k_closed_loop_con(alg::Params pr_arg, ConLoopArgs a_arg) {
    using namespace alg;
    CPR pr0 = kernel_params();
    const ALG_AS4 ConLoopArgs& a0 = con_loop_args();
    const int g = blockIdx.x, lane = game_tid(), B = pr0.B, K1 = pr0.con_len / (pr0.N - 1), knots = a0.knots, items = knots * K1;   // (below 2^27: the 1 GiB cap)
    constexpr int NONE = 0x7fffffff;
    double w[ALG_CON_KINDS]; int f[ALG_CON_KINDS];
#pragma unroll
    for (int c = 0; c < ALG_CON_KINDS; c++) { w[c] = -__builtin_inf(); f[c] = NONE; }
    for (int e = lane; e < items; e += WAVE) {
        // opaque copies per trip (phase_params): the block counts, masks, table pointers and schedule pointers of every kind are read where a row
        // uses them, by scalar loads, instead of being hoisted in front of the loop and kept -- or spilled -- in SGPRs across it
        CPR pr = phase_params(pr0);
        const ALG_AS4 ConLoopArgs& a = *(const ALG_AS4 ConLoopArgs*)uniform_u64((unsigned long long)&a0);
        const Game G = game_view(pr, g);
        const int q = e / K1, r = e - q * K1, t = q / a.hold;
        const size_t at = (size_t)q * B + g;
        auto sched = [&](int kind, int len) -> const double* {
            if (!a.sched[kind]) return nullptr;
            const int row = t < a.rows[kind] ? t : a.rows[kind] - 1;
            return as_global(a.sched[kind]) + ((size_t)row * B + g) * len;
        };
        int kind, abi;
        const double c = con_row<C>(pr, G, sched, as_global(a.states) + (at + B) * C::n, as_global(a.controls) + at * C::m, r, 0, kind, abi);
        as_global(a.vals)[at * K1 + r] = c;
#pragma unroll
        for (int s = 0; s < ALG_CON_KINDS; s++)
            if (kind == s) { w[s] = con_max_nan(w[s], c); if (!(c <= 0.0)) f[s] = min(f[s], q); }
    }
    double wo = 0.0; int fo = 0;
#pragma unroll
    for (int s = 0; s < ALG_CON_KINDS; s++) {
        const double ws = wave_butterfly(w[s], [](double x, double y) { return con_max_nan(x, y); }) + 0.0;     // (+ 0.0: a maximum of -0 and +0 reads +0 whatever the order)
        const int fs = wave_min_i32(f[s]);
        if (lane == s) { wo = ws; fo = fs == NONE ? -1 : fs; }
    }
    if (lane < ALG_CON_KINDS) { as_global(a0.worst)[g * ALG_CON_KINDS + lane] = wo; as_global(a0.first)[g * ALG_CON_KINDS + lane] = fo; }
}
