"""Shared helpers of the extended-constraint horizon tests (tests/test_ext_horizon_family.py on the CPU, tests/test_gpu_ext_horizons.py on the
GPU): the constrained problem family, its cached reference solves, the configurations and the layout of the constraint rows.  No test lives here.

`ext_family` is the short-horizon family of tests/test_gpu_horizon_shapes.py (players on a circle of radius 0.4 +- 0.05 crossing to radius 0.6 on
the far side: collision cost, collision avoidance, control bounds) without its inert wall and with extended constraints that are ACTIVE from the
shortest horizons on.  With dt = 0.1 a player moves a few hundredths per step, so the obstacles sit where the players start:

  circle     (0, 0, r = 0.38): every player crosses the middle, and the players that start at a radius below 0.38 start inside it;
  walls      x <= 0.39 for |y| < 0.3 (player 0 starts at x = 0.33 ... 0.45; the players from the far side end there) and y >= -0.25 for
             -0.9 < x < -0.3 (in front of player 0's target);
  state      player 0: |velocity| <= 0.15 (double integrator: reached at the third knot under the control bound 0.8),
  bound      speed >= 0.45 (unicycle / bicycle: they start at 0.5 and brake for a target at rest);
  d = 3      spherical instead of planar collision avoidance, a ceiling panel (Wall3D) at z = 0.05 between the start heights +- 0.1, and a
             cylinder of radius 0.15 around the x axis, which player 0 starts next to or inside.
  quadrotor  the same obstacles around two quadrotors that start at rest on the circle at heights +- 0.1 with the hover thrust as control target
             (HS.family has no quadrotor branch); the state bound holds player 0's velocities to +- 0.15.

tests/test_ext_horizon_family.py holds, on the CPU, that every kind of row reaches a multiplier above 1e-2 at short and at long horizons and that
the family is not amplifying (oracle against the long-double arbiter)."""
import numpy as np

import test_gpu_horizon_shapes as HS

DI, UNI, BIC, QUAD = HS.DI, HS.UNI, HS.BIC, HS.QUAD
KEY = "ext"                                        # cache key of the family in HS.reference / HS.mpc_reference

CIRCLE_R = {DI: 0.355, UNI: 0.22, BIC: 0.22, QUAD: 0.355}
WALLS = ([0.42, -0.9, 0.1], [-0.3, -0.25, -0.10], [0.42, -0.3, 0.5], [0.3, -0.25, -0.10], [1.0, 0.0, 0.0], [0.0, -1.0, -1.0])       # x1, y1, x2, y2, xv, yv of the three walls
V_MAX, SPEED_MIN = 0.15, 0.45
CEILING = ([[-1.0, -1.0, 0.08]], [[1.0, -1.0, 0.08]], [[1.0, 1.0, 0.08]], [[0.0, 0.0, 1.0]])
CYLINDER = ([[-1.0, -0.1, 0.0]], [0], [2.0], [0.07])
HOVER = 0.5 * 9.81 / 4 / 1.245                      # m g / (4 kf), scenarios.quadrotor_crossing
# What the CPU preconditions made of the starting point: seeds of configurations whose seed-0 games miss one of them -- the lone double integrator
# has no active extended row at N = 2, the quadrotors none on the ceiling panel at N = 7, and the five-step loops of the three-player double
# integrator (N = 5) and of the bicycles (N = 3) take different numbers of iterations in double and in long double.
EXT_TUNED = {(DI, 1, 2): dict(seed=2), (DI, 3, 2): dict(seed=2), (BIC, 2, 2): dict(seed=4), (QUAD, 2, 3): dict(seed=2)}
# The random step-wise data is _pair(seed = N) but for the one (configuration, N) whose seed-N batch has a kind of extended row with one sign
# only (a single player, a single knot: eight circle rows in the batch, all of them below zero).
PAIR_SEED = {((DI, 1, 3), 2): 102}


def _quad_base(make, p, N, B, seed):
    """two (p) quadrotors at rest on the family's circle, heights +- 0.1, flying to the far side: Q of scenarios.quadrotor_crossing times ten,
    R = 0.1 around the hover thrust, rotor commands in [0, 3]"""
    rng = np.random.default_rng([seed, QUAD, p, 3, N])
    b = make(QUAD, p, N, HS.DT, B, 3)
    ang = 2 * np.pi * np.arange(p) / p + rng.uniform(-0.3, 0.3, (B, p))
    rad = 0.4 + rng.uniform(-0.05, 0.05, (B, p))
    hz = rng.uniform(-0.1, 0.1, (B, 2, p))
    x0 = np.zeros((B, b.n)); xf = np.zeros((B, p, 12))
    x0[:, 0:p], x0[:, p:2 * p], x0[:, 2 * p:3 * p] = rad * np.cos(ang), rad * np.sin(ang), hz[:, 0]
    xf[:, :, 0], xf[:, :, 1], xf[:, :, 2] = 0.6 * np.cos(ang + np.pi + 0.4), 0.6 * np.sin(ang + np.pi + 0.4), hz[:, 1]
    Q = np.concatenate([np.full(3, 10.0), np.full(3, 5.0), np.full(3, 2.0), np.full(3, 2.0)])
    b.set_x0(x0)
    b.set_lqr(np.broadcast_to(Q, (B, p, 12)).copy(), np.full((B, p, 4), 0.1), xf, np.full((B, p, 4), HOVER))
    b.set_options(**HS.OPTS)
    b.add_collision_cost(np.full(p, 1.0), np.full(p, 2.0))
    b.add_spherical_collision_avoidance(np.full(p, 0.13))
    b.add_control_bound(np.full(b.m, 3.0), np.zeros(b.m))
    return b


def ext_family(make, model, p, d, N, B=4, seed=0, turn=0.5):
    """HS.family(make, model, p, d, N) without the inert wall, plus the active extended constraints of the module text."""
    d3 = d == 3 or model == QUAD
    b = _quad_base(make, p, N, B, seed) if model == QUAD else HS.family(make, model, p, d, N, B=B, seed=seed, turn=turn, spherical=d3)
    xmax, xmin = np.full(b.n, np.inf), np.full(b.n, -np.inf)
    if model == DI:
        vel = [a * p for a in range(d, 2 * d)]                             # player 0's velocities: state index a p + i
        xmax[vel], xmin[vel] = V_MAX, -V_MAX
    elif model == QUAD:
        vel = [a * p for a in range(6, 9)]
        xmax[vel], xmin[vel] = V_MAX, -V_MAX
    else:
        xmin[3 * p] = SPEED_MIN
    b.add_state_bound(0, xmax, xmin)
    b.add_wall_constraint(*WALLS)
    b.add_circle_constraint([0.0], [0.0], [CIRCLE_R[model]])
    if d3:
        b.add_wall3d_constraint(*CEILING)
        b.add_cylinder_constraint(*CYLINDER)
    return b


def build(make, model, p, d, N):
    return ext_family(make, model, p, d, N, **EXT_TUNED.get((model, p, d), {}))


def hip_ext_family(alg, model, p, d, N):
    return build(lambda *a: alg.Batch(alg.hip_lib(), *a[:5], d=a[5]), model, p, d, N)


def reference(orc, cfg, N, kind=""):
    """the oracle's (kind "") or the long-double arbiter's ("x") solve of ext_family(*cfg, N), cached as HS.reference caches the base family's"""
    return HS.reference(orc, *cfg, N, kind=kind, build=build, key=KEY)


def mpc_reference(orc, cfg, N, kind=""):
    return HS.mpc_reference(orc, cfg, N, kind=kind, build=build, key=KEY)


# ---- the layout of the constraint rows -------------------------------------------------------------------------------------------------------------
KINDS_2D, KINDS_3D = ("sb", "wall", "circ"), ("sb", "wall", "circ", "wall3", "cyl")


def ext_rows(b, nwall, ncirc, nwall3=0, ncyl=0, sb=True):
    """kind -> (first row, shape (p, K, entries)) of the extended rows of a batch: they close the constraint vector as
    [state bounds (p, K, 2 n)] [walls (p, K, nwall)] [circles (p, K, ncirc)] [Wall3D (p, K, nwall3)] [cylinders (p, K, ncyl)]
    (algames_solver.hpp, dual_penalty_update), behind the collision-avoidance and control-bound rows."""
    K, out, end = b.N - 1, {}, b.con_len
    for kind, cnt in (("cyl", ncyl), ("wall3", nwall3), ("circ", ncirc), ("wall", nwall), ("sb", 2 * b.n if sb else 0)):
        if cnt:
            end -= b.p * K * cnt
            out[kind] = (end, (b.p, K, cnt))
    assert end >= 0
    return out


def family_rows(b, cfg):
    """ext_rows of ext_family(*cfg, N): three walls, one circle; d = 3 / quadrotor: one Wall3D panel, one cylinder"""
    return ext_rows(b, 3, 1, *((1, 1) if cfg[2] == 3 else ()))


def kind_of(v, rows):
    """the rows of each kind out of a (B, con_len) array: kind -> (B, p, K, entries)"""
    return {k: v[:, e0:e0 + int(np.prod(sh))].reshape((len(v),) + sh) for k, (e0, sh) in rows.items()}


def ext_start(rows):
    return min(e0 for e0, _ in rows.values())


# ---- the configurations ------------------------------------------------------------------------------------------------------------------------------
DI2_D3 = (DI, 2, 3)
TILE_EXT = [(m, p, 2) for m in (DI, UNI, BIC) for p in (1, 2, 3, 4)] + [DI2_D3]                    # the 13 tile EXT instantiations
DENSE_EXT = [(DI, 5, 2), (UNI, 6, 2), (BIC, 5, 2), (DI, 1, 3), (DI, 3, 3), (QUAD, 2, 3)]          # dense E = 1 kinds: N = 2 ... 7
DENSE_EXT_P10 = [(DI, 10, 2), (BIC, 10, 2)]                                                         # N = 2, 3, 4
MASK_HORIZONS = (2, 3, 5, 7, 9)
SOLVE_CHUNK = [(DI, 3, 2), (UNI, 3, 2), (UNI, 4, 2), (BIC, 2, 2)]                                  # whole solves at HS.horizons(cfg)
SOLVE_SHORT = [(DI, 1, 2), (DI, 4, 2), (UNI, 1, 2), (BIC, 4, 2), DI2_D3]                           # whole solves at N = 2 ... 18
TEAM_DENSE = [(QUAD, 2, 3), (DI, 3, 3)]                                                             # dense EXT teams of four, N = 2 ... 7
MPC_EXT = [(DI, 3, 2), (UNI, 3, 2), (BIC, 2, 2)]


def step_horizons(cfg):
    return range(2, 19) if cfg in TILE_EXT else (range(2, 8) if cfg in DENSE_EXT else (2, 3, 4))


def solve_horizons(cfg):
    return HS.horizons(*cfg) if cfg in SOLVE_CHUNK else (list(range(2, 8)) if cfg in TEAM_DENSE else list(range(2, 19)))


def solve_problems():
    """every (configuration, horizons) of ext_family that the GPU tests solve"""
    return [(cfg, solve_horizons(cfg)) for cfg in SOLVE_CHUNK + SOLVE_SHORT + TEAM_DENSE]


def name(cfg):
    return HS._name(cfg)


def pair(alg, orc, cfg, N, B=4, seed=None):
    """(product batch, oracle batch, rows) on the random full-magnitude data of the parity tests' _pair, all ingredients on, seed N: every extended
    row with a multiplier of O(1) (three in ten: 0) and a penalty in [1, 3]"""
    model, p, d = cfg
    seed = PAIR_SEED.get((cfg, N), N) if seed is None else seed
    if d == 3:
        if cfg == DI2_D3:
            import test_gpu_parity_3d as P3
            g, o = P3._pair(alg, orc, N, B=B, seed=seed)
        else:
            import test_gpu_parity_dense as PD
            g, o = PD._pair(alg, orc, model, p, N, B=B, seed=seed)
        return g, o, ext_rows(o, 2, 2, 2, 3)
    import test_gpu_parity_ext as PE
    g, o = PE._pair(alg, orc, model, p, N, B=B, seed=seed)
    return g, o, ext_rows(o, 2, 3)


# ---- masks and pair subsets --------------------------------------------------------------------------------------------------------------------------
MASK_PROBLEMS = [("walls_circles", (UNI, 3, 2)), ("walls_circles", (BIC, 2, 2)), ("walls_circles", (DI, 4, 2)), ("wall3d_cylinders", DI2_D3),
                 ("pairs", (DI, 3, 2))]
PAIRS = ((0, 1, 0.9), (2, 0, 0.35))


def _inert(b, rows, on):
    """(con_len,) bool: the rows of the entries that do not constrain their player; on: kind -> {player: entries that do}"""
    out = np.zeros(b.con_len, bool)
    for kind, per_player in on.items():
        e0, (p, K, cnt) = rows[kind]
        m = np.ones((p, K, cnt), bool)
        for i, entries in per_player.items():
            m[i, :, list(entries)] = False
        out[e0:e0 + m.size] = m.reshape(-1)
    return out


def mask_pair(alg, orc, which, cfg, N, B=4):
    """(product batch, oracle batch, inert rows (con_len,) bool) of the problems whose constraint entries hold for some players only:
    the per-player wall / circle problem of test_gpu_parity_ext, the per-player Wall3D / cylinder problem of test_gpu_parity_3d, and the
    extended set behind two ordered collision-avoidance pairs of unequal radii."""
    model, p, d = cfg
    if which == "walls_circles":
        import test_gpu_parity_ext as PE
        g, o = PE._per_player_pair(alg, orc, model, p, N, B=B)
        rows = ext_rows(o, 3, 2 if p > 2 else 1, sb=False)
        circ = {p - 1: {0}}
        if p > 2:
            circ[1] = {0, 1}
        return g, o, _inert(o, rows, {"wall": {0: {0, 1}, p - 1: {1, 2}}, "circ": circ})
    if which == "wall3d_cylinders":
        import test_gpu_parity_3d as P3
        g, o = P3._per_player_pair(alg, orc, model, p, N, B=B)
        rows = ext_rows(o, 0, 0, 2, 3, sb=False)
        return g, o, _inert(o, rows, {"wall3": {0: {0, 1}, p - 1: {1}}, "cyl": {p - 1: {0, 1}, 0: {1, 2}}})
    import test_gpu_parity_ext as PE
    g, o = PE._pair(alg, orc, model, p, N, B=B, seed=N, ingredients=("cost", "ctl", "sb", "wall", "circ"))
    z = o.get_traj()
    for b in (g, o):
        for i, j, r in PAIRS:
            b.add_collision_avoidance_pair(i, j, r)
    assert g.con_len == o.con_len
    rng = np.random.default_rng([N, 11])
    lam, mu = rng.random((B, o.con_len)), 1.0 + 2.0 * rng.random((B, o.con_len))
    lam[rng.random((B, o.con_len)) < 0.3] = 0.0
    for b in (g, o):
        b.set_traj(z); b.set_con_duals(lam, mu)
    K, inert = N - 1, np.zeros(o.con_len, bool)
    for i in range(p):
        for j in range(p):
            if i != j and (i, j) not in {(a, c) for a, c, _ in PAIRS}:
                q = i * (p - 1) + (j if j < i else j - 1)
                inert[q * K:(q + 1) * K] = True
    return g, o, inert
