// algames_normal.hpp -- the normal equations of a parameter fit (alg_kkt_normal_equations).
// k_sens_gram reduces the unit columns X_1 .. X_q that k_kkt_sens left in the inspection scratch, and the residual r = z - target of the game's
// pdtraj, to one weighted Gram matrix per game: with Y = [X_1 .. X_q | r] (S rows, q + 1 <= 64 columns) and W = diag(w),
//   G = Y' W Y,   H = G[:q, :q],   g = G[:q, q],   loss = G[q, q] / 2.
// Not a template over Cfg: only the problem sizes enter.  One workgroup of GRAM_WAVES wavefronts per game.  G is cut into 16 x 16 tiles; the
// pairs (I <= J) of the upper triangle, at most ten, are dealt to the wavefronts round robin, and a wavefront walks the rows of one pair at a
// time, eight rows e0 .. e0 + 7 per step with two v_mfma_f64_16x16x4_f64:
//   lane l loads rows e, e + 1 with e = e0 + 2 (l >> 4) of its column in one 16-byte load; the first MFMA takes the even rows, the second the odd
//   A operand of lane l: A[l & 15][k = l >> 4] = w_e y_e of column 16 I + (l & 15);   B[l >> 4][l & 15] = y_e of column 16 J + (l & 15)
//   (a diagonal pair uses the one loaded value for both);   C/D: col = lane & 15, row = (lane >> 4) + 4 reg.
// Every entry of G is therefore one chain over the rows in an order that depends on S alone, inside one wavefront: no cross-wave reduction, no
// atomic, no LDS, and the result of a game depends on nothing but the game.  Rows past S and columns past q + 1 are zero operands (the load
// address is clamped, the value selected): no lane leaves an MFMA and nothing is read past a column.  A column starts at a multiple of S
// doubles, so for odd S the 16-byte loads are 8-byte aligned only (global memory takes them).  Two rows per lane against one, C2 with 24
// columns on an MI355X: 0.69 ms against 1.15 ms (profiles/normal_speed.txt) -- a 128-byte line of a column serves two loads instead of four.
// Of a diagonal tile only the entries c <= d are stored (the two triangles of such a tile differ in which factor carried w_e); every entry goes
// to (c, d) and (d, c), so H is symmetric bit for bit.  Vector stores only.
#pragma once
#include "algames_device.hpp"

constexpr int GRAM_WAVES = 4;
constexpr int GRAM_STEPS = 4;      // steps of eight rows whose loads are issued before their MFMAs run
typedef double double2u_t __attribute__((ext_vector_type(2), aligned(8)));

// One tile pair's chain over the rows.  The value of the lane's column at row e is p[e] - (res ? tg[e] : 0) where ok, else 0 (x - 0 is x: a
// scratch column passes unchanged, and r is one subtraction).  The lane's rows e, e + 1 come from one load at min(e, S - 2) (S >= 2: S is a
// multiple of b = n + m + n p); a pair that starts on the last row sits in the second half of the clamped load, and a row past S is zero.
// The trip count is S rounded up to a multiple of 8 GRAM_STEPS rows: the steps past the end multiply zeros.  Every lane loads tg[e] and w_e
// (four addresses per wavefront and step, one cache line) and selects, so the loop has no branch.
template <bool DIAG>
__device__ __forceinline__ double4_t gram_chain(const double* __restrict__ pa, const bool ra, const bool oa, const double* __restrict__ pb, const bool rb, const bool ob,
                                                const double* __restrict__ tg, const double* __restrict__ wt, const int S, const int lk) {
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int e0 = 0; e0 < S; e0 += 8 * GRAM_STEPS) {
        double a[2 * GRAM_STEPS], b[2 * GRAM_STEPS];
#pragma unroll
        for (int u = 0; u < GRAM_STEPS; u++) {
            const int e = e0 + 8 * u + 2 * lk, eb = e < S - 2 ? e : S - 2;
            const bool sh = e == S - 1, in0 = e < S, in1 = e + 1 < S;
            const double2u_t t2 = *(const double2u_t*)(tg + eb), w2 = *(const double2u_t*)(wt + eb), x2 = *(const double2u_t*)(pa + eb);
            const double t0 = sh ? t2.y : t2.x, w0 = sh ? w2.y : w2.x, x0 = sh ? x2.y : x2.x;
            const double y0 = (oa && in0) ? x0 - (ra ? t0 : 0.0) : 0.0, y1 = (oa && in1) ? x2.y - (ra ? t2.y : 0.0) : 0.0;
            a[2 * u] = w0 * y0; a[2 * u + 1] = w2.y * y1;
            if (DIAG) { b[2 * u] = y0; b[2 * u + 1] = y1; }
            else {
                const double2u_t z2 = *(const double2u_t*)(pb + eb);
                const double z0 = sh ? z2.y : z2.x;
                b[2 * u] = (ob && in0) ? z0 - (rb ? t0 : 0.0) : 0.0; b[2 * u + 1] = (ob && in1) ? z2.y - (rb ? t2.y : 0.0) : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 2 * GRAM_STEPS; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    return acc;
}

// table: per column c < q two 64-bit integers, the offset of game g0's column in `cols` and its stride from game to game (doubles): the
// columns of a parameter kind lie in the segment of that kind's k_kkt_sens launch.  target: gridDim.x x S; weight: S, or gridDim.x x S if
// per_game_w.  gstatus: ngroup x gridDim.x, the status words of the launches in launch order; status: the first that is not OK.
__global__ void __launch_bounds__(GRAM_WAVES * WAVE) k_sens_gram(Params pr_arg, const long long* table, const double* cols, const double* target, const double* weight,
                                                                 int per_game_w, int q, int g0, int ngroup, const int* gstatus, double* Hout, double* gout, double* loss,
                                                                 int* status) {
    CPR pr = kernel_params();
    const int gl = blockIdx.x, lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = pr.S, T = (q + 16) >> 4;                                   // tiles of the q + 1 columns
    const Game G = game_view(pr, g0 + gl);
    const double* __restrict__ z = G.z(0) + pr.n;                            // the S entries of pdtraj behind x_1
    const double* __restrict__ tg = as_global(target) + (size_t)gl * S;
    const double* __restrict__ wt = as_global(weight) + (per_game_w ? (size_t)gl * S : (size_t)0);
    const long long* __restrict__ tab = as_global(table);
    const double* __restrict__ cb = as_global(cols);
    const int li = lane & 15, lk = lane >> 4;
    // column c: a column of the scratch, the residual column q (pdtraj minus target), or a zero column (any readable address)
    auto column = [&](int c, const double* __restrict__& p, bool& res, bool& ok) {
        ok = c <= q; res = c == q;
        const int cc = c < q ? c : 0;
        const double* __restrict__ ps = cb + tab[2 * cc] + (long long)gl * tab[2 * cc + 1];
        p = c < q ? ps : z;
    };
    int pair = 0;
    for (int I = 0; I < T; I++) {
        for (int J = I; J < T; J++, pair++) {
            if (pair % GRAM_WAVES != wave) continue;                         // wave-uniform
            const double* __restrict__ pa; const double* __restrict__ pb; bool ra, rb, oa, ob;
            column(16 * I + li, pa, ra, oa);
            column(16 * J + li, pb, rb, ob);
            const double4_t acc = I == J ? gram_chain<true>(pa, ra, oa, pb, rb, ob, tg, wt, S, lk) : gram_chain<false>(pa, ra, oa, pb, rb, ob, tg, wt, S, lk);
            const int d = 16 * J + li;
            for (int r = 0; r < 4; r++) {
                const int c = 16 * I + lk + 4 * r;
                const double v = acc[r];
                if (c <= d && d <= q) {
                    if (d < q) {
                        double* __restrict__ Hg = as_global(Hout) + (size_t)gl * q * q;
                        gst(Hg, c * q + d, v); gst(Hg, d * q + c, v);
                    } else if (c < q) as_global(gout)[(size_t)gl * q + c] = v;
                    else as_global(loss)[gl] = 0.5 * v;
                }
            }
        }
    }
    if (threadIdx.x == 0 && status) {
        int worst = ALG_STATUS_OK;
        for (int k = 0; k < ngroup; k++) {
            const int s = as_global(gstatus)[(size_t)k * gridDim.x + gl];
            if (worst == ALG_STATUS_OK) worst = s;
        }
        as_global(status)[gl] = worst;
    }
}
