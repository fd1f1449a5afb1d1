"""Shared helpers of the KKT-solve / sensitivity tests (tests/test_kkt_sensitivity_family.py on the CPU, tests/test_gpu_kkt_solve.py on the GPU):
the problems, the reference right-hand sides and the reference solve.  No test lives here.

The reference is always the ORACLE's Jacobian (orc_residual_jacobian) with numpy's LAPACK solve, never the HIP Jacobian:

    X_ref = np.linalg.solve(J, R)                                    J X = R, what alg_kkt_solve(ALG_KKT_RHS_USER) answers
    R_x0  = -[A_0 in the dyn_1 rows, 0 elsewhere]                    A_0 from OracleBatch.kat_dynamics at (x_1, u_1): X = d z* / d x0
    R_xf  = -(res(x_f + e) - res(x_f - e)) / 2                       oracle residual differences (res is affine in x_f: exact to rounding)

An oracle "twin" is a list of (OracleBatch, game index), one entry per game of the device batch: the games of one oracle batch, or -- for
per-game scenario data, which the oracle does not have -- one OracleBatch(B = 1) per game."""
import numpy as np

DI, UNI, BIC, QUAD = 0, 1, 2, 3
DT = 0.1
# ---- the shapes: one per kernel kind (name, model, p, d, how the handle reaches its kernels) -----------------------------------------------------------
# "base": base kernels; "wall": the family's far-away wall / the extended set of test_gpu_parity_ext (EXT kernels); "bic": EXT by its model;
# "twin": ALG_SCEN_KERNELS_BASE with per-game pair radii (the E = 2 twins); "dense": the dense-direction kinds
SHAPES = {
    "di3": (DI, 3, 2, "base"), "uni4": (UNI, 4, 2, "base"), "di2_d1": (DI, 2, 1, "base"),
    "di3_ext": (DI, 3, 2, "wall"), "bic2": (BIC, 2, 2, "bic"), "di3_twin": (DI, 3, 2, "twin"),
    "di5": (DI, 5, 2, "dense"), "di3_d3": (DI, 3, 3, "dense"), "quad2": (QUAD, 2, 2, "dense"),
}
REGS = (0.0, 1e-3)
NCOL = 5                                           # random USER columns per game


def FT(model, p, d=2):
    """steps per chunk of the fused trial pass (test_gpu_horizon_shapes.FT)"""
    import test_gpu_horizon_shapes as HS
    return HS.FT(model, p, d)


def horizons(name):
    """N in {2, 3, 5, 7, 9}: N = 2 puts step 0 on the terminal step, 5 / 7 / 9 sit on both sides of the sweep rings of 4, 6 and 8; tile shapes
    also N - 1 = FT + 1; dense kinds stop at N = 7."""
    model, p, d, how = SHAPES[name]
    if how == "dense":
        return [2, 3, 5, 7]
    return [2, 3, 5, 7, 9, FT(model, p, d) + 2]


class OracleAsProduct:
    """stands in for the `alg` argument of the _pair helpers of the parity tests: their "HIP" half becomes a second oracle batch, so that the
    very same random problem can be built without a GPU"""

    def __init__(self, orc):
        import algames_jl_amd
        self._lib, self.Batch = orc.lib(), algames_jl_amd.Batch

    def hip_lib(self):
        return self._lib


def twin_of(o):
    return [(o, g) for g in range(o.B)]


def pair_problem(alg, orc, name, N, B=4):
    """(device batch, oracle twin) of shape `name` on the random full-magnitude data of the parity tests' _pair (every constraint row with a
    multiplier and a penalty of O(1)); seed N as in test_newton_direction_over_horizons.  alg = OracleAsProduct(orc) builds it on the CPU."""
    model, p, d, how = SHAPES[name]
    if model == QUAD:
        import test_gpu_parity_quad as PQ
        g, o = PQ._pair(alg, orc, p, N, B=B, seed=N)
        return g, twin_of(o)
    if how in ("wall", "bic"):
        import test_gpu_parity_ext as PE
        g, o = PE._pair(alg, orc, model, p, N, B=B, seed=N)
        return g, twin_of(o)
    from test_gpu_parity import _pair
    g, o = _pair(alg, orc, model, p, d, N, B=B, seed=N)
    if how != "twin":
        return g, twin_of(o)
    # per-game pair radii on the base kernels' block-reading twins: game k's radii on its own OracleBatch(B = 1) with game k's data
    rad = 0.3 + 0.1 * np.arange(p) + 0.05 * np.random.default_rng(1000 + N).random((B, p))
    if hasattr(g, "set_scenario_kernels") and g.lib.prefix == "alg_":
        g.set_scenario_kernels(1)
        g.set_scenario_data(0, np.stack([(r[:, None] + r[None, :]).reshape(-1) * (1 - np.eye(p).reshape(-1)) for r in rad]))
        assert g.get_scenario_kernels() == (1, 2)
    z, (lam, mu) = o.get_traj(), o.get_con_duals()
    rng = np.random.default_rng(N)                   # _pair's own draws, in its order
    ni = o.n // p
    Q, R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, o.mi))
    xf, uf = rng.random((B, p, ni)), rng.random((B, p, o.mi)) - 0.5
    x0 = rng.random((B, o.n))
    assert np.array_equal(x0, z[:, :o.n])
    tw = []
    for k in range(B):
        q = orc.OracleBatch(model, p, N, DT, 1, d=d)
        q.set_x0(x0[k:k + 1]); q.set_lqr(Q[k:k + 1], R[k:k + 1], xf[k:k + 1], uf[k:k + 1])
        q.add_collision_cost(np.full(p, 3.0), 1.0 + np.arange(p))
        q.add_collision_avoidance(rad[k])
        umax = np.full(q.m, 0.6); umin = np.full(q.m, -0.4); umax[0] = np.inf
        q.add_control_bound(umax, umin)
        q.set_traj(z[k:k + 1]); q.set_con_duals(lam[k:k + 1], mu[k:k + 1])
        tw.append((q, 0))
    return g, tw


def recording(b):
    """b.set_lqr keeps its arguments in b._lqr (the family builds its targets inside)"""
    orig = b.set_lqr

    def set_lqr(Q, R, xf, uf):
        b._lqr = tuple(np.array(v, dtype=np.float64) for v in (Q, R, xf, uf))
        return orig(Q, R, xf, uf)
    b.set_lqr = set_lqr
    return b


def family_problem(make, name, N, B=4):
    """the short-horizon family of test_gpu_horizon_shapes (players crossing a circle: collision cost, collision avoidance, control bounds) on
    make(model, p, N, dt, B, d) -> batch, with its LQR data recorded; "wall" / "twin" shapes as there (far-away wall; equal blocks uploaded in
    ALG_SCEN_KERNELS_BASE mode)."""
    import test_gpu_horizon_shapes as HS
    model, p, d, how = SHAPES[name]
    b = HS.family(lambda *a: recording(make(*a)), model, p, d, N, B=B, wall=(how == "wall"), **HS.TUNED.get((model, p, d), {}))
    if how == "twin" and b.lib.prefix == "alg_":
        b.set_scenario_kernels(1)
        for k in (0, 1, 2):
            b.set_scenario_data(k, b.get_scenario_data(k))
        assert b.get_scenario_kernels() == (1, 2)
    return b


# ---- index maps (newton_core.jl:40-89), 0-based ------------------------------------------------------------------------------------------------------------
def vx(b, i, k):
    return i * (b.N - 1) * (b.n + b.mi) + k * (b.n + b.mi)


def vu(b, i, k):
    return vx(b, i, k) + b.n


def vd(b, k):
    return b.p * (b.N - 1) * (b.n + b.mi) + k * b.n


def hx(b, k):
    return k * b.b


def hu(b, k, i=0):
    return k * b.b + b.n + i * b.mi


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------
def jacobians(tw, reg):
    """the oracle's J per game, (B, S, S) [row vertical, column horizontal]"""
    return np.stack([o.residual_jacobian(reg, games=(g, 1))[0] for o, g in tw])


def residuals(tw, reg=0.0):
    return np.stack([o.residual(0, reg)[0][g] for o, g in tw])


def solve_ref(J, R):
    """X (B, S, q) with J X = R, LAPACK (partial pivoting) per game"""
    return np.stack([np.linalg.solve(J[g], R[g]) for g in range(len(J))])


def refine_ld(J, R, X, steps=3):
    """the same solution refined with residuals in long double (fixed-precision iterative refinement towards the exact solution of the
    double-precision data): what solve_ref is measured against"""
    out = []
    for g in range(len(J)):
        Rl, Xl = R[g].astype(np.longdouble), X[g].astype(np.longdouble)
        rows, cols = np.nonzero(J[g])                # (J is block-banded: the long-double product runs over its non-zeros only)
        Jnz = J[g][rows, cols].astype(np.longdouble)[:, None]
        for _ in range(steps):
            r = Rl.copy()
            np.subtract.at(r, rows, Jnz * Xl[cols])
            Xl = Xl + np.linalg.solve(J[g], r.astype(np.float64)).astype(np.longdouble)
        out.append(Xl)
    return np.stack(out)


def col_err(X, Xr):
    """worst |X - Xr| / max |Xr| over the columns of (B, S, q) arrays"""
    Xr = np.asarray(Xr)
    den = np.abs(Xr).max(axis=1, keepdims=True)
    return float((np.abs(np.asarray(X, dtype=Xr.dtype) - Xr) / np.where(den > 0, den, 1)).max())


def user_columns(B, S, seed, ncol=NCOL):
    return np.random.default_rng([seed, 77]).uniform(-1.0, 1.0, (B, S, ncol))


def rhs_x0(tw):
    """R = -d res / d x_1 per game, (B, S, n): -A_0 in the dyn_1 rows (A_0 = d x_2 / d x_1 of the discrete dynamics at (x_1, u_1), the one
    block J has no column for), zero elsewhere"""
    out = []
    for o, g in tw:
        z = o.get_traj()[g]
        x1, us = z[:o.n], z[2 * o.n:2 * o.n + o.m]
        uj = np.empty(o.m)                           # joint control index c = j p + i <- stored (player by player) i mi + j
        for i in range(o.p):
            for j in range(o.mi):
                uj[j * o.p + i] = us[i * o.mi + j]
        A0 = o.kat_dynamics(x1, uj)[3][:, :o.n]
        R = np.zeros((o.S, o.n))
        R[vd(o, 0):vd(o, 0) + o.n] = -A0
        out.append(R)
    return np.stack(out)


def rhs_xf(tw, lqr):
    """R = -d res / d x_f per game, (B, S, p ni), columns in the xf order of set_lqr: central differences of the oracle's residual with step 1
    (res is affine in x_f).  lqr = [(Q, R, xf, uf) of twin entry k, shaped for that entry's batch]; the batches get their data back."""
    out, done = [None] * len(tw), {}
    for k, ((o, g), (Q, Rr, xf, uf)) in enumerate(zip(tw, lqr)):
        if id(o) not in done:                        # one pass per oracle batch serves all of its games
            ni = o.n // o.p
            R = np.zeros((o.B, o.S, o.p * ni))
            for i in range(o.p):
                for a in range(ni):
                    rr = []
                    for s in (1.0, -1.0):
                        x = np.array(xf); x[..., i, a] += s
                        o.set_lqr(Q, Rr, x, uf)
                        rr.append(o.residual(0, 0.0)[0])
                    R[:, :, i * ni + a] = -(rr[0] - rr[1]) / 2
            o.set_lqr(Q, Rr, xf, uf)
            done[id(o)] = R
        out[k] = done[id(o)][g]
    return np.stack(out)


def rhs_xf_analytic(b, Q):
    """the same right-hand side written down: +w_k Q_i[a] in row opt_i,x_{k+1}[a p + i] of every step (w_k = dt, 1 on the terminal step); Q (B, p, ni)"""
    ni = b.n // b.p
    R = np.zeros((len(Q), b.S, b.p * ni))
    for k in range(b.N - 1):
        w = b.dt if k + 1 < b.N - 1 else 1.0
        for i in range(b.p):
            for a in range(ni):
                R[:, vx(b, i, k) + a * b.p + i, i * ni + a] = w * Q[:, i, a]
    return R


def copy_iterate(src, tw):
    """the oracle twin linearises where the device batch does: its trajectory, multipliers and penalties are the device batch's"""
    z, (lam, mu) = src.get_traj(), src.get_con_duals()
    for k, (o, g) in enumerate(tw):
        if o.B == 1:
            o.set_traj(z[k:k + 1]); o.set_con_duals(lam[k:k + 1], mu[k:k + 1])
    if tw and tw[0][0].B > 1:
        tw[0][0].set_traj(z); tw[0][0].set_con_duals(lam, mu)
