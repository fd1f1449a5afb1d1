"""Shared helpers of the failure-exit tests (tests/test_failure_family.py on the CPU, tests/test_gpu_failure_exits.py on the GPU): batches in
which SOME games end with status SINGULAR or NAN, built through make(model, p, N, dt, B, d) so that the same code gives a Batch, an OracleBatch
and the long-double arbiter (kind "x"); the comparison functions of the GPU tests, which import without a GPU.  No test lives here.

A failure has to be structurally exact -- a pivot that is a zero in any arithmetic and any elimination order, an entry that is a NaN -- or double
and long double, oracle and device part on it.  Every game of a batch has a ROLE:

entry batch (`entry`, newton_solve(init=False), regularize = 0, reg_0 = 0, no dual reset, 3 outer x 5 inner iterations): the random
full-magnitude data of test_gpu_parity._pair (Q, R, xf, uf, x0, trajectory, multipliers, penalties; collision cost, collision avoidance,
control bounds +0.6 / -0.4, optionally the far-away wall that switches the handle to the EXT kernels), seed N, and
  H  healthy: that data unchanged;
  S  singular: Q = R = 0, the players' first coordinates 10 apart (no pair term of the cost or of the avoidance is active), the controls
     inside their bounds, every constraint multiplier 0, the dynamics multipliers random (the residual is not zero): the control block of the
     KKT matrix is an exact zero;
  N  poisoned: one control slot of the trajectory is NaN (player 0's first control at the middle step).
  A lone player has no pair term and would converge in one Newton iteration: its control targets lie 3 lower, below the lower bound.
  After set_traj the builder rolls the states out (rollout(0)), as newton_solve does itself: the step-wise entry points then see the same
  structure (without it the S game keeps random states with active pair terms and is singular only to rounding).

late batch (`late`, newton_solve(init=True), alpha_dual = lambda_max = inf, 4 outer x 8 inner iterations): control bounds +0.6 / -0.4 and a
collision avoidance between players 10 apart (never active).  The first dual update gives lambda = inf to every control-bound row with a
value above zero and 0 to every row below, so
  L  late-failing: uf = 10 on every control -- the bounds are violated after the first outer iteration, the first record of the second one
     finds a non-finite residual entry: NAN after several records, inside outer iteration 2;
  H  healthy: x0 = xf (at rest) and uf = 0 (quadrotors: the hover thrust, under an upper bound of 1.5) -- converges in the first outer
     iteration with every bound value near -0.4 / -0.6.

loop batch (`loop`): the short-horizon family of test_gpu_horizon_shapes with a NaN in x0[1] of game 2 (mpc_solve draws new controls, so S and
N do not survive it): NAN at the first record of every step.

`control=True` builds the same batch with every failing game's data replaced by H data: games are independent blocks, a healthy game must
leave identical bits in both."""
import numpy as np

import test_gpu_horizon_shapes as HS

DI, UNI, BIC, QUAD = HS.DI, HS.UNI, HS.BIC, HS.QUAD
OK, SINGULAR, NAN = 0, 1, 2
GID0 = HS.GID0
ENTRY_OPTS = dict(regularize=0, reg_0=0.0, dual_reset=0, outer_iter=3, inner_iter=5)
LATE_OPTS = dict(alpha_dual=np.inf, lambda_max=np.inf, outer_iter=4, inner_iter=8)
ENTRY_LAYOUTS = ("HSNH", "SHHN", "SNNS")           # a failing game between healthy ones; first and last game fail; no healthy game
LATE_LAYOUTS = ("HLLH", "LHHL")
STATUS_OF = {"H": OK, "S": SINGULAR, "N": NAN, "L": NAN}
DIRECTION_STATUS_OF = {"H": OK, "S": SINGULAR, "N": SINGULAR}   # alg_newton_direction has no residual test: a non-finite pivot is SINGULAR
COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures")
U_MAX, U_MIN = 0.6, -0.4
FAR = 10.0
HOVER = 0.5 * 9.81 / 4 / 1.245                      # m g / (4 kf), scenarios.quadrotor_crossing
QUAD_U_MAX = 1.5                                    # upper control bound of the quadrotors in the late batch (the hover thrust, 0.98, lies above 0.6)
LOOP_STEPS, LOOP_GAME = 3, 2
# What the CPU preconditions (tests/test_failure_family.py) made of the seed N: the (configuration, N) whose seed-N batch has a healthy game with
# fewer than three Newton iterations, a healthy game that diverges (the quadrotors from random attitudes, without regularisation), or a
# history that differs between double and long double.
ENTRY_SEED = {((DI, 1, 2), 2): 1402, ((DI, 1, 2), 3): 203, ((UNI, 1, 2), 2): 1402, ((DI, 2, 3), 3): 103, ((DI, 2, 1), 3): 203, ((QUAD, 2, 2), 7): 22007}


def dims(cfg):
    """(model, p, d) as the constructor takes them: the quadrotor lives in three dimensions whatever the configuration lists say"""
    model, p, d = cfg
    return model, p, (3 if model == QUAD else d)


def statuses(roles, of=STATUS_OF):
    return [of[r] for r in roles]


def failing(roles):
    return np.array([r != "H" for r in roles])


def _control_slots(b):
    """(N - 1, m) trajectory indices of the controls, joint order, through split_traj of an index array"""
    return b.split_traj(np.arange(b.traj_len, dtype=np.float64)[None])[1][0].astype(np.int64)


def nan_slot(b):
    """the control slot the N role poisons: the first control of the middle step (player 0's: with two players or more the states it reaches
    enter the pair terms, so the KKT matrix is non-finite too, not only the residual)"""
    return int(_control_slots(b)[(b.N - 1) // 2, 0])


def _entry_arrays(b, cfg, N, roles, wall, seed=None):
    """the data of the entry batch for a batch b that already carries its constraints: dict(Q, R, xf, uf, x0, z, lam, mu)"""
    model, p, _ = dims(cfg)
    B = b.B
    rng = np.random.default_rng(ENTRY_SEED.get((tuple(cfg), N), N) if seed is None else seed)
    ni, shift = b.n // p, (0.3 if model == QUAD else 0.0)       # (quadrotor: negative rotor commands as in test_gpu_parity_quad._pair)
    Q, R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, b.mi))
    xf, uf = rng.random((B, p, ni)), rng.random((B, p, b.mi)) - 0.5
    if p == 1:
        uf -= 3.0                                   # (a lone player has no pair term: its targets lie below the lower bound, the bound rows make the iterations)
    x0 = rng.random((B, b.n)) - shift
    z = rng.random((B, b.traj_len)) - shift
    base = b.con_len - (b.p * (b.N - 1) if wall else 0)         # (the wall's rows close the constraint vector: the rows in front of them keep their data)
    lam, mu = rng.random((B, base)), 1.0 + 2.0 * rng.random((B, base))
    lam[rng.random((B, base)) < 0.3] = 0.0
    if wall:
        lam = np.concatenate([lam, rng.random((B, b.con_len - base))], axis=1)
        mu = np.concatenate([mu, 1.0 + 2.0 * rng.random((B, b.con_len - base))], axis=1)
    ctl = _control_slots(b).reshape(-1)
    for game, role in enumerate(roles):
        if role == "S":
            Q[game], R[game], lam[game] = 0.0, 0.0, 0.0
            x0[game, 0:p] = FAR * np.arange(p)
            z[game, ctl] = 0.5 * (z[game, ctl] + shift) - 0.2      # in [-0.2, 0.3): inside (-0.4, 0.6)
        elif role == "N":
            z[game, nan_slot(b)] = np.nan
    z[:, :b.n] = x0
    return dict(Q=Q, R=R, xf=xf, uf=uf, x0=x0, z=z, lam=lam, mu=mu)


def _set_entry_arrays(b, a):
    b.set_x0(a["x0"]); b.set_lqr(a["Q"], a["R"], a["xf"], a["uf"])
    b.set_traj(a["z"]); b.set_con_duals(a["lam"], a["mu"])
    b.rollout(0)


def entry(make, cfg, N, roles, wall=False, control=False, B=4, seed=None):
    """The entry batch of the module text; roles: one of H, S, N per game."""
    model, p, d = dims(cfg)
    assert len(roles) == B and set(roles) <= set("HSN")
    if control:
        roles = "H" * B
    b = make(model, p, N, HS.DT, B, d)
    if model == BIC:
        b.set_bicycle(0.07, 0.04)
    if p > 1:
        b.add_collision_cost(np.full(p, 3.0), 1.0 + np.arange(p))
        b.add_collision_avoidance(0.3 + 0.1 * np.arange(p))
    umax = np.full(b.m, U_MAX); umax[0] = np.inf
    b.add_control_bound(umax, np.full(b.m, U_MIN))
    if wall:
        before = b.con_len
        b.add_wall_constraint([5.0], [5.0], [6.0], [5.0], [0.0], [1.0])
        assert b.con_len - before == b.p * (b.N - 1)
    b.set_options(**ENTRY_OPTS)
    _set_entry_arrays(b, _entry_arrays(b, cfg, N, roles, wall, seed))
    return b


def repair_entry(b, cfg, N, wall=False):
    """overwrites the data of an entry batch with the control batch's (every game H) through set_lqr, set_x0, set_traj and set_con_duals"""
    _set_entry_arrays(b, _entry_arrays(b, cfg, N, "H" * b.B, wall))


def late(make, cfg, N, roles, wall=False, control=False, B=4, seed=None):
    """The late batch of the module text; roles: H or L per game."""
    model, p, d = dims(cfg)
    assert len(roles) == B and set(roles) <= set("HL")
    if control:
        roles = "H" * B
    b = make(model, p, N, HS.DT, B, d)
    rng = np.random.default_rng([N if seed is None else seed, 5])
    ni = b.n // p
    Q, R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, b.mi))
    xf = np.zeros((B, p, ni)); uf = np.zeros((B, p, b.mi))
    npos = 1 if (model == DI and d == 1) else (3 if d == 3 else 2)
    xf[:, :, :npos] = rng.random((B, p, npos))
    xf[:, :, 0] += FAR * np.arange(p)
    if model in (UNI, BIC):
        xf[:, :, 3 if model == BIC else 2] = rng.random((B, p))                         # heading (bicycle: x, y, v, psi); speed 0: at rest
    if model == QUAD:
        uf[:] = HOVER
    x0 = xf.transpose(0, 2, 1).reshape(B, b.n).copy()                                   # state index a p + i
    for game, role in enumerate(roles):
        if role == "L":
            uf[game] = 10.0
            x0[game] += 0.1 * rng.random(b.n)
    if model == BIC:
        b.set_bicycle(0.07, 0.04)
    b.set_x0(x0); b.set_lqr(Q, R, xf, uf)
    b.set_options(**LATE_OPTS)
    if p > 1:
        b.add_collision_avoidance(0.3 + 0.1 * np.arange(p))
    b.add_control_bound(np.full(b.m, QUAD_U_MAX if model == QUAD else U_MAX), np.full(b.m, U_MIN))
    if wall:
        b.add_wall_constraint([5.0], [5.0], [6.0], [5.0], [0.0], [1.0])
    return b


def ctl_rows(b):
    """slice of the control-bound rows in the constraint vector: they follow the collision rows (algames_solver.hpp, dual_penalty_update)"""
    off = b.p * (b.p - 1) * (b.N - 1)
    return slice(off, off + 2 * b.m * (b.N - 1))


def loop(make, cfg, N, control=False, B=4):
    """The loop batch: HS.family with game LOOP_GAME's x0[1] = nan."""
    b = HS.family(make, *cfg, N, B=B, **HS.TUNED.get(tuple(cfg), {}))
    if not control:
        x0 = b.get_x0()
        x0[LOOP_GAME, 1] = np.nan
        b.set_x0(x0)
    return b


def oracle_make(orc, kind=""):
    return lambda *a: orc.OracleBatch(*a[:5], d=a[5], kind=kind)


def hip_make(alg):
    return lambda *a: alg.Batch(alg.hip_lib(), *a[:5], d=a[5])


# ---- the comparison functions of the GPU tests (tests/test_failure_family.py runs them with the oracle's library in the device's place) -------------
TOL_Z, TOL_STAT, TOL_LAM, TOL_REC, TOL_X = 1e-8, 1e-9, 1e-6, 1e-9, 1e-13      # test_gpu_parity's docstring; record fields; rolled-out states
VIO = ("res", "dyn_vio", "con_vio", "sta_vio", "opt_vio")
WORST = {}                                                                      # family -> worst healthy-game |hip - oracle| (printed by each test)


def note(family, err):
    WORST[family] = max(WORST.get(family, 0.0), float(err))


def game_bits(b, game):
    """HS._bits of one game: its trajectory, multipliers, penalties, statistics (but the wall time) and history"""
    bits = HS._bits(b)
    nh = len(b.get_history(0).dtype.names) - 1
    head = len(bits) - nh * b.B
    return [a[game] for a in bits[:head]] + bits[head + nh * game:head + nh * (game + 1)]


def assert_isolated(g, c, roles, what):
    """b. every healthy game of g has the bits of the same game of the control batch c"""
    for game in np.nonzero(~failing(roles))[0]:
        for i, (x, y) in enumerate(zip(game_bits(g, game), game_bits(c, game))):
            assert np.shape(x) == np.shape(y) and np.array_equal(x, y, equal_nan=True), (what, "isolation", int(game), i)


def assert_discrete_parity(g, o, what, games=None):
    """a. statistics counters and outer / ls_j of every history record, every game"""
    sg, so = g.get_stats(), o.get_stats()
    games = range(o.B) if games is None else games
    for f in COUNTS:
        assert np.array_equal(sg[f][list(games)], so[f][list(games)]), (what, f, sg[f], so[f])
    for game in games:
        hg, ho = g.get_history(game), o.get_history(game)
        assert len(hg) == len(ho) == so["records"][game], (what, int(game), len(hg), len(ho))
        for f in ("outer", "ls_j"):
            assert np.array_equal(hg[f], ho[f]), (what, int(game), f, hg[f], ho[f])


def assert_healthy_parity(g, o, roles, what, family):
    """c. healthy games against the oracle: trajectory 1e-8 absolute, final statistics 1e-9, mu bit-equal and lambda 1e-6 relative on converged games"""
    sg, so = g.get_stats(), o.get_stats()
    zg, zo = g.get_traj(0), o.get_traj(0)
    (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
    for game in np.nonzero(~failing(roles))[0]:
        err = np.abs(zg[game] - zo[game]).max()
        print(what, "game", int(game), "|hip - orc| %.2e" % err)
        note(family, err)
        assert err <= TOL_Z, (what, int(game), err)
        for f in VIO:
            a, b = sg["last"][f][game], so["last"][f][game]
            assert np.isclose(a, b, rtol=TOL_STAT, atol=TOL_STAT), (what, int(game), f, a, b)
        if so["converged"][game] == 1:
            assert np.array_equal(mg[game], mo[game]), (what, int(game), "mu")
            fin = np.isfinite(lo[game])
            assert np.array_equal(np.isfinite(lg[game]), fin), (what, int(game), "lambda")
            dl = np.abs(lg[game][fin] - lo[game][fin]).max(initial=0.0)
            assert dl <= TOL_LAM * max(1.0, np.abs(lo[game][fin]).max(initial=0.0)), (what, int(game), "lambda", dl)


def assert_failing_parity(g, o, roles, what):
    """d. failing games against the oracle.  Every record: the fields that are finite in the oracle to 1e-9 relative; the residual norm of the
    failing record (the one before the solve's closing record) non-finite on both sides for N and L games; the violation maxima of a record
    with a non-finite residual norm are printed only (maxima over entries some of which are NaN: the device's fmax reductions drop NaNs,
    the oracle's comparisons keep whichever side the order of the entries favours).  The iterate: a game that failed before its
    first Newton iteration (S, N) still holds its input -- controls and dynamics multipliers equal, NaNs in the same slots, the rolled-out
    states with the same NaN mask and within 1e-13; an L game has iterated: its iterate agrees like a healthy game's (1e-8) with the same
    NaN mask, its mu is bit-equal, its lambda infinite in the same rows and within 1e-6 relative elsewhere."""
    so = o.get_stats()
    zg, zo = g.get_traj(0), o.get_traj(0)
    Xg, Ug, Lg = g.split_traj(zg); Xo, Uo, Lo = o.split_traj(zo)
    (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
    for game in np.nonzero(failing(roles))[0]:
        role = roles[game]
        hg, ho = g.get_history(game), o.get_history(game)
        assert len(hg) == len(ho) >= 2, (what, int(game))
        sane = np.isfinite(ho["res"])                  # records of a finite iterate; the violation maxima of the others are printed only
        assert np.array_equal(np.isfinite(hg["res"]), sane), (what, role, int(game), "res", hg["res"], ho["res"])
        for f in VIO + ("alpha", "delta"):
            if f in VIO[1:]:
                ok = sane & np.isfinite(ho[f])
                if not sane.all():
                    print(what, role, "game", int(game), f, "of the non-finite records: hip", hg[f][~sane], "orc", ho[f][~sane])
            else:
                ok = np.isfinite(ho[f])
            assert np.isfinite(hg[f][ok]).all() and np.allclose(hg[f][ok], ho[f][ok], rtol=TOL_REC, atol=1e-14), (what, role, int(game), f, hg[f], ho[f])
        if role in "NL":
            assert not np.isfinite(hg["res"][-2]) and not np.isfinite(ho["res"][-2]), (what, role, int(game), hg["res"], ho["res"])
        assert np.array_equal(np.isnan(zg[game]), np.isnan(zo[game])), (what, role, int(game), "NaN mask")
        if so["newton_iters"][game] == 0:
            assert np.array_equal(Ug[game], Uo[game], equal_nan=True) and np.array_equal(Lg[game], Lo[game], equal_nan=True), (what, role, int(game), "u, lambda")
            fin = np.isfinite(Xo[game])
            assert np.abs(Xg[game][fin] - Xo[game][fin]).max(initial=0.0) <= TOL_X * max(1.0, np.abs(Xo[game][fin]).max(initial=0.0)), (what, role, int(game), "x")
            assert np.array_equal(lg[game], lo[game]) and np.array_equal(mg[game], mo[game]), (what, role, int(game), "constraint multipliers")
        else:
            fin = np.isfinite(zo[game])
            err = np.abs(zg[game][fin] - zo[game][fin]).max(initial=0.0)
            assert err <= TOL_Z, (what, role, int(game), err)
            assert np.array_equal(mg[game], mo[game]), (what, role, int(game), "mu")
            assert np.array_equal(np.isinf(lg[game]), np.isinf(lo[game])) and np.array_equal(np.isnan(lg[game]), np.isnan(lo[game])), (what, role, int(game), "infinite lambda")
            fin = np.isfinite(lo[game])
            dl = np.abs(lg[game][fin] - lo[game][fin]).max(initial=0.0)
            assert dl <= TOL_LAM * max(1.0, np.abs(lo[game][fin]).max(initial=0.0)), (what, role, int(game), "lambda", dl)
            if role == "L":
                assert np.isinf(lo[game][ctl_rows(o)]).any(), (what, int(game), "no infinite multiplier")


def solve(b, init):
    return b.newton_solve(init=init, game_id0=GID0)


def compare_solve(g, c, o, roles, what, family):
    """a - e of the module text of tests/test_gpu_failure_exits.py on three solved batches: device, control batch on the device, oracle"""
    assert g.get_stats()["status"].tolist() == statuses(roles) == o.get_stats()["status"].tolist(), (what, g.get_stats()["status"], o.get_stats()["status"])
    assert_discrete_parity(g, o, what)
    assert_isolated(g, c, roles, what)
    assert_healthy_parity(g, o, roles, what, family)
    assert_failing_parity(g, o, roles, what)
    HS._guards_ok(g)


def run_case(make, orc, builder, cfg, N, roles, what, family, wall=False, prepare=None):
    """Builds the three batches of one case, solves them and compares; prepare(batch) configures the device batches (waves per game,
    scenario kernels, hand-off budget ...).  Returns (device batch, control batch, oracle batch)."""
    init = builder is late
    g, c = builder(make, cfg, N, roles, wall=wall), builder(make, cfg, N, roles, wall=wall, control=True)
    o = builder(oracle_make(orc), cfg, N, roles, wall=wall)
    for b in (g, c):
        if prepare:
            prepare(b)
        solve(b, init)
    solve(o, init)
    compare_solve(g, c, o, roles, what, family)
    return g, c, o


def tile_horizons(cfg):
    return (2, 3, 7, HS.FT(*cfg) + 2)


DENSE_HORIZONS = (2, 3, 7)


def horizons(cfg):
    """the horizons of a configuration in every family: N in {2, 3, 7} on the dense shapes, {2, 3, 7, FT + 2} on the tile shapes"""
    return DENSE_HORIZONS if tuple(cfg) in HS.DENSE_CONFIGS else tile_horizons(cfg)


# ---- the bodies of the GPU tests: `alg` is the product, or test_gpu_fuzz._OracleAsHip on a machine without a GPU ------------------------------------
def solve_family(alg, orc, cfg, horizons, family, prepare=None, wall=False, entry_layouts=ENTRY_LAYOUTS, late_layouts=LATE_LAYOUTS, after=None):
    """entry batch with every layout and late batch with every layout at every horizon: a - e; after(g, c, o, roles, kind) adds a family's own checks"""
    make = hip_make(alg)
    for N in horizons:
        for builder, layouts, kind in ((entry, entry_layouts, "entry"), (late, late_layouts, "late")):
            for roles in layouts:
                what = (family, HS._name(cfg), N, kind, roles)
                g, c, o = run_case(make, orc, builder, cfg, N, roles, what, (family,) + tuple(cfg), wall=wall, prepare=prepare)
                if after:
                    after(g, c, o, roles, kind)
    print(family, HS._name(cfg), "worst healthy-game |hip - orc| %.2e" % WORST.get((family,) + tuple(cfg), 0.0))


def stepwise_family(alg, orc, cfg, N, roles="HSNH"):
    """alg_newton_direction, alg_kkt_solve (the oracle, which stands in for the device on the CPU, has none) and alg_newton_step on the entry
    batch"""
    import kkt_reference as K
    make, what = hip_make(alg), ("step-wise", HS._name(cfg), N)
    g, c, o = entry(make, cfg, N, roles), entry(make, cfg, N, roles, control=True), entry(oracle_make(orc), cfg, N, roles)
    ok = ~failing(roles)
    before = HS._bits(g)
    dg, sg = g.newton_direction(0.0); dc, sc = c.newton_direction(0.0); do, so = o.newton_direction(0.0)
    assert sg.tolist() == so.tolist() == statuses(roles, DIRECTION_STATUS_OF), (what, sg, so)
    assert np.all(sc == 0), (what, sc)
    assert np.all(np.isfinite(dg[ok])), what
    err = (np.abs(dg[ok] - do[ok]) / np.abs(do[ok]).max(axis=1, keepdims=True)).max()
    print(what, "direction, healthy games: worst relative difference %.2e" % err)
    assert err <= 1e-9, (what, err)
    assert np.array_equal(dg[ok], dc[ok]), (what, "direction: isolation")
    if g.lib.prefix != "orc_":
        T = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1)))
        R = K.user_columns(g.B, g.S, N)
        X, st = g.kkt_solve(T(R), reg=0.0); Xc, stc = c.kkt_solve(T(R), reg=0.0)
        assert st.tolist() == statuses(roles, DIRECTION_STATUS_OF) and np.all(stc == 0), (what, "kkt_solve", st, stc)
        assert np.all(np.isfinite(X[ok])), (what, "kkt_solve: status OK with a non-finite column")
        J = np.stack([o.residual_jacobian(0.0, games=(int(game), 1))[0] for game in np.nonzero(ok)[0]])
        Xr = K.solve_ref(J, R[ok])
        fwd = K.col_err(T(X[ok]), Xr)
        lin = np.abs(np.einsum("brc,bcq->brq", J, T(X[ok])) - R[ok]).max() / max(1.0, np.abs(R[ok]).max())
        print(what, "kkt_solve, healthy games: forward %.2e backward %.2e" % (fwd, lin))
        assert fwd <= 1e-9 and lin <= 1e-8, (what, fwd, lin)                     # TOL_X, TOL_LIN of test_gpu_kkt_solve
        assert np.array_equal(X[ok], Xc[ok]), (what, "kkt_solve: isolation")
        f = np.nonzero(~ok)[0]
        if len(f) == 2 and f[1] == f[0] + 1:
            _, st2 = g.kkt_solve(T(R[f]), reg=0.0, games=(int(f[0]), 2))
            assert st2.tolist() == [SINGULAR, SINGULAR], (what, "games", st2)
        _, stx = g.kkt_solve(kind="x0", reg=0.0)
        assert stx.tolist() == st.tolist(), (what, "x0", stx)
    for i, (x, y) in enumerate(zip(before, HS._bits(g))):
        assert np.array_equal(x, y, equal_nan=True), (what, "an inspection entry point changed the handle", i)
    z0 = g.get_traj(0)
    ig, ic, io = g.newton_step(1, 1), c.newton_step(1, 1), o.newton_step(1, 1)
    assert ig["status"].tolist() == io["status"].tolist() == statuses(roles), (what, ig["status"], io["status"])
    for f in ("control_flow", "ls_j", "ls_failed"):
        assert np.array_equal(ig[f], io[f]), (what, f, ig[f], io[f])
        assert np.array_equal(ig[f][ok], ic[f][ok]), (what, f, "isolation")
    assert np.array_equal(ig["alpha"], io["alpha"]), (what, ig["alpha"], io["alpha"])
    zg, zc, zo = g.get_traj(0), c.get_traj(0), o.get_traj(0)
    assert np.array_equal(zg[ok], zc[ok]), (what, "newton_step: isolation")
    err = np.abs(zg[ok] - zo[ok]).max() / max(1.0, np.abs(zo[ok]).max())
    note(("step-wise",) + tuple(cfg), err)
    assert err <= 1e-9, (what, err)                                                     # test_inner_iteration_parity
    assert np.array_equal(zg[~ok], z0[~ok], equal_nan=True), (what, "a failed step moved the iterate")
    HS._guards_ok(g)


def ibr_family(alg, orc, cfg, N, roles="HSNH"):
    """ibr_newton_solve(ibr_iter = 2, init = False) and ibr_solve_player(0) on the entry batch: statuses, discrete parity, isolation"""
    make = hip_make(alg)
    for which in ("ibr_newton_solve", "ibr_solve_player"):
        what = (which, HS._name(cfg), N)
        g, c, o = entry(make, cfg, N, roles), entry(make, cfg, N, roles, control=True), entry(oracle_make(orc), cfg, N, roles)
        for b in (g, c, o):
            _ = b.ibr_newton_solve(ibr_iter=2, init=False, game_id0=GID0) if which == "ibr_newton_solve" else b.ibr_solve_player(0)
        assert g.get_stats()["status"].tolist() == statuses(roles) == o.get_stats()["status"].tolist(), (what, g.get_stats()["status"], o.get_stats()["status"])
        assert_discrete_parity(g, o, what)
        assert_isolated(g, c, roles, what)
        ok = ~failing(roles)
        err = np.abs(g.get_traj(0)[ok] - o.get_traj(0)[ok]).max() / max(1.0, np.abs(o.get_traj(0)[ok]).max())
        print(what, "healthy games |hip - orc| / max(1, max |z|) %.2e" % err)
        note(("ibr",) + tuple(cfg), err)
        assert err <= TOL_Z, (what, err)
        HS._guards_ok(g)


def afterwards_family(alg, cfg, N, prepare=None, roles="HSNH", late_roles="HLLH"):
    """A failing solve, then the failing games' data overwritten with H data, then a second solve: the bits of a fresh handle that only ever
    saw the repaired data, and the hand-off count of that handle.  And after the late batch: alpha_dual / lambda_max back at their defaults, a
    solve with init = True."""
    make, what = hip_make(alg), ("afterwards", HS._name(cfg), N)
    g, fresh = entry(make, cfg, N, roles), entry(make, cfg, N, roles, control=True)
    for b in (g, fresh):
        if prepare:
            prepare(b)
    st = solve(g, False)
    assert st["status"].tolist() == statuses(roles), (what, st["status"])
    repair_entry(g, cfg, N)
    s1 = solve(g, False)
    solve(fresh, False)
    assert np.all(s1["status"] == 0) and s1["newton_iters"].min() >= 3, (what, s1["status"], s1["newton_iters"])
    HS._same_bits(g, fresh, what)
    assert g.get_handoff() == fresh.get_handoff(), (what, g.get_handoff(), fresh.get_handoff())
    HS._guards_ok(g)
    g, fresh = late(make, cfg, N, late_roles), late(make, cfg, N, late_roles)
    d = g.lib.default_opts()
    for b in (g, fresh):
        if prepare:
            prepare(b)
    st = solve(g, True)
    assert st["status"].tolist() == statuses(late_roles), (what, "late", st["status"])
    for b in (g, fresh):
        b.set_options(alpha_dual=d.alpha_dual, lambda_max=d.lambda_max)
    s1 = solve(g, True)
    solve(fresh, True)
    assert np.all(s1["status"] == 0) and np.isfinite(g.get_traj(0)).all() and np.isfinite(g.get_con_duals()[0]).all(), (what, "late", s1["status"])
    HS._same_bits(g, fresh, what + ("late",))
    assert g.get_handoff() == fresh.get_handoff(), (what, "late", g.get_handoff(), fresh.get_handoff())
    HS._guards_ok(g)


# ---- what the GPU tests run ---------------------------------------------------------------------------------------------------------------------------
STEP_CONFIGS = [HS.DI3, HS.UNI4, (DI, 2, 1), (DI, 5, 2), (DI, 3, 3), (QUAD, 2, 2), (BIC, 2, 2)]     # one per detection site of the direction code
IBR_CONFIGS = [HS.DI3, HS.UNI3, (DI, 5, 2)]
LOOP_HORIZONS = (3, 6)
# the handle afterwards: (configuration, how the handle is set up -- waves per game, 0 = what the library picks, and the hand-off budget)
AFTERWARDS = [(HS.DI3, 1, 0), (HS.UNI4, 2, 0), ((DI, 5, 2), 0, 0), (HS.DI3, 1, 3)]
DENSE_EXT_TEAMS = [(DI, 3, 3), (QUAD, 2, 2)]        # with the far-away wall: the dense EXT team kernels (test_gpu_ext_horizons: TEAM_DENSE)


def solve_problems():
    """every (configuration, far-away wall, horizons) the solve families of tests/test_gpu_failure_exits.py use"""
    out = [(cfg, False, tile_horizons(cfg)) for cfg in HS.BASE_CONFIGS] + [(cfg, wall, tile_horizons(cfg)) for cfg, wall in HS.EXT_CONFIGS]
    return out + [(cfg, False, DENSE_HORIZONS) for cfg in HS.DENSE_CONFIGS] + [(cfg, True, DENSE_HORIZONS) for cfg in DENSE_EXT_TEAMS]
