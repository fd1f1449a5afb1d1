"""Per-game scenario data (alg_set_scenario_data): the games of one handle differ in obstacles, bounds and radii.

The oracle has no per-game entry, so game g of a device batch is compared against its own OracleBatch(B = 1), built with that
game's adders, its x0 and LQR block and newton_solve(init=True, game_id0=7+g) -- the device batch solves with game_id0 = 7 and
keys its generator by game_id0 + g, so the initial guesses match."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DI, UNI, BIC, QUAD = 0, 1, 2, 3
K_RAD, K_COST, K_CTL, K_SB, K_WALL, K_CIRC, K_W3, K_CYL = range(8)
GID0 = 7


# ---- ingredients: (kind, values of game g -> packed row, adder of game g's values on a batch) ---------------------------------------
def _avoid(p, rng, B, spherical=False):
    r = 0.08 + 0.06 * rng.random((B, p))
    pack = lambda v: (v[:, None] + v[None, :]).reshape(-1) * (1 - np.eye(p).reshape(-1))
    add = lambda b, v: b.add_spherical_collision_avoidance(v) if spherical else b.add_collision_avoidance(v)
    return K_RAD, r, pack, add


def _cost(p, rng, B):
    v = np.concatenate([0.2 + 0.3 * rng.random((B, p)), 1.0 + 2.0 * rng.random((B, p))], axis=1)
    return K_COST, v, lambda v: v, lambda b, v: b.add_collision_cost(v[:p], v[p:])


def _ctl(m, rng, B):
    umax = 0.4 + 0.4 * rng.random((B, m)); umin = -0.3 - 0.4 * rng.random((B, m))
    umax[:, 0] = np.inf                                   # the same +-inf pattern in every game
    v = np.concatenate([umax, umin], axis=1)
    return K_CTL, v, lambda v: v, lambda b, v: b.add_control_bound(v[:m], v[m:])


def _sb(p, n, players, rng, B):
    mx = np.full((B, p, n), np.inf); mn = np.full((B, p, n), -np.inf)
    fin = rng.random((p, n)) < 0.6
    for i in players:
        mx[:, i] = np.where(fin[i], 0.4 + 0.5 * rng.random((B, n)), np.inf)
        mn[:, i] = np.where(fin[i], -0.1 + 0.2 * rng.random((B, n)), -np.inf)
    v = np.concatenate([mx.reshape(B, -1), mn.reshape(B, -1)], axis=1)

    def add(b, v):
        x, y = v[:p * n].reshape(p, n), v[p * n:].reshape(p, n)
        for i in players:
            b.add_state_bound(i, x[i], y[i])
    return K_SB, v, lambda v: v, add


def _walls(rng, B, nw=2):
    w = np.array([[0.0, 0.5, 1.0, 0.5, 0.0, 1.0], [0.2, 1.0, 0.9, 0.1, 0.6, 0.8]])[:nw]
    v = (w[None] + 0.05 * (rng.random((B, nw, 6)) - 0.5)).reshape(B, -1)
    return K_WALL, v, lambda v: v, lambda b, v: b.add_wall_constraint(*v.reshape(nw, 6).T)


def _player_circles(rng, B, sets):
    """sets: [(player, number of circles)] -- distinct entries, so the table is the concatenation in call order"""
    tot = sum(c for _, c in sets)
    base = np.stack([rng.random(tot), rng.random(tot), 0.15 + 0.1 * rng.random(tot)], axis=1)
    v = (base[None] + np.concatenate([0.05 * (rng.random((B, tot, 2)) - 0.5), 0.03 * rng.random((B, tot, 1))], axis=2)).reshape(B, -1)

    def add(b, v):
        t = v.reshape(tot, 3); at = 0
        for i, c in sets:
            b.add_circle_constraint_player(i, *t[at:at + c].T); at += c
    return K_CIRC, v, lambda v: v, add


def _wall3d(rng, B):
    w = np.array([0.0, 0.0, 0.5, 1.0, 0.0, 0.5, 0.0, 1.0, 0.5, 0.0, 0.0, 1.0])
    v = w[None] + 0.05 * (rng.random((B, 12)) - 0.5) * np.repeat([1, 1, 1, 0], 3)[None]
    return K_W3, v, lambda v: v, lambda b, v: b.add_wall3d_constraint(v[0:3], v[3:6], v[6:9], v[9:12])


def _cyl(rng, B):
    v = np.concatenate([0.5 + 0.1 * (rng.random((B, 3)) - 0.5), 0.8 + 0.2 * rng.random((B, 1)), 0.1 + 0.1 * rng.random((B, 1))], axis=1)
    return K_CYL, v, lambda v: v, lambda b, v: b.add_cylinder_constraint(v[None, 0:3], [2], [v[3]], [v[4]])


FAMILIES = {   # name: (model, p, d, N, ingredient builder(rng, B, n, m))
    "di3_cost_avoid_ctl": (DI, 3, 2, 10, lambda r, B, n, m, p: [_cost(p, r, B), _avoid(p, r, B), _ctl(m, r, B)]),
    "uni4_walls_player_circles": (UNI, 4, 2, 8, lambda r, B, n, m, p: [_walls(r, B), _player_circles(r, B, [(0, 1), (2, 2)])]),
    "bic2_state_bound": (BIC, 2, 2, 10, lambda r, B, n, m, p: [_sb(p, n, (0, 1), r, B), _ctl(m, r, B)]),
    "di3d_sphere_wall3d_cyl": (DI, 2, 3, 8, lambda r, B, n, m, p: [_avoid(p, r, B, spherical=True), _wall3d(r, B), _cyl(r, B)]),
    "quad2_cost_ctl": (QUAD, 2, 3, 6, lambda r, B, n, m, p: [_cost(p, r, B), _ctl(m, r, B)]),
    "di5_ext": (DI, 5, 2, 5, lambda r, B, n, m, p: [_cost(p, r, B), _avoid(p, r, B), _ctl(m, r, B), _walls(r, B, 1)]),
}


class Case:
    def __init__(self, alg, name, B=8, seed=0, per_game=True):
        model, p, d, N, build = FAMILIES[name]
        self.model, self.p, self.d, self.N, self.dt, self.B = model, p, d, N, 0.1, B
        self.g = alg.Batch(alg.hip_lib(), model, p, N, self.dt, B, d=d)
        g = self.g
        rng = np.random.default_rng(seed)
        ni = g.n // p
        self.Q, self.R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, g.mi))
        self.xf, self.uf = rng.random((B, p, ni)), 0.2 * (rng.random((B, p, g.mi)) - 0.5)
        self.x0 = self._x0(rng, g.n)
        self.ingr = build(rng, B, g.n, g.m, p)
        self.per_game = per_game
        self.setup(self.g, None)
        if per_game:
            for kind, v, pack, _ in self.ingr:
                g.set_scenario_data(kind, np.stack([pack(v[k]) for k in range(B)]))

    def _x0(self, rng, n):
        x0 = 0.1 * rng.random((self.B, n))
        p = self.p
        x0[:, 0:p] += np.linspace(0.0, 0.8, p)[None]                 # players apart in x
        x0[:, p:2 * p] += np.linspace(0.8, 0.0, p)[None]
        return x0

    def setup(self, b, game):
        """adders of game `game` (None: game 0's values on the whole batch) + x0 / LQR"""
        sl = slice(None) if game is None else slice(game, game + 1)
        b.set_x0(self.x0[sl]); b.set_lqr(self.Q[sl], self.R[sl], self.xf[sl], self.uf[sl])
        for kind, v, pack, add in self.ingr:
            add(b, v[0 if game is None else game])

    def oracle(self, orc, game, kind=""):
        o = orc.OracleBatch(self.model, self.p, self.N, self.dt, 1, d=self.d, kind=kind)
        self.setup(o, game)
        return o


def _arbiter_solve(c, orc, game):
    x = c.oracle(orc, game, kind="x")
    return x, x.newton_solve(init=True, game_id0=GID0 + game)


def _same_solve(g, o, game, st_g, st_o, arbiter=None):
    """the suite's rule (tests/test_gpu_fuzz.py::_compare_solve) for game `game` of g against the one-game oracle o: discrete history
    identical; trajectory within 1e-8 of the largest entry and last-record statistics within rtol 1e-6 (atol 1e-9) -- or, where the problem
    amplifies rounding beyond that, the HIP path no further from the long-double arbiter (arbiter() builds and solves it) than four times
    the oracle's distance"""
    for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
        assert st_g[f][game] == st_o[f][0], (f, game, st_g[f][game], st_o[f][0])
    hg, ho = g.get_history(game), o.get_history(0)
    assert len(hg) == len(ho)
    for f in ("outer", "ls_j"):
        assert np.array_equal(hg[f], ho[f]), (f, game)
    zg, zo = g.get_traj()[game], o.get_traj()[0]
    scale = max(1.0, np.abs(zo).max())
    x = None
    if np.abs(zg - zo).max() > 1e-8 * scale:
        assert arbiter is not None, (game, np.abs(zg - zo).max())
        x, sx = arbiter()
        zx = x.get_traj()[0]
        assert np.abs(zg - zx).max() <= 4.0 * np.abs(zo - zx).max() + 1e-8 * scale, (game, "trajectory")
    for f in ("res", "dyn_vio", "con_vio", "sta_vio", "opt_vio"):
        a, b = st_g["last"][f][game], st_o["last"][f][0]
        if np.isclose(a, b, rtol=1e-6, atol=1e-9):
            continue
        assert arbiter is not None, (f, game, a, b)
        if x is None:
            x, sx = arbiter()
        c = sx["last"][f][0]
        assert abs(a - c) <= 4.0 * abs(b - c) + 1e-6 * abs(c) + 1e-9, (f, game, a, b, c)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_solve_parity_per_game(alg, orc, name):
    c = Case(alg, name)
    st = c.g.newton_solve(init=True, game_id0=GID0)
    for game in range(c.B):
        o = c.oracle(orc, game)
        so = o.newton_solve(init=True, game_id0=GID0 + game)
        _same_solve(c.g, o, game, st, so, arbiter=lambda: _arbiter_solve(c, orc, game))


@pytest.mark.parametrize("name", ["di3_cost_avoid_ctl", "uni4_walls_player_circles", "bic2_state_bound", "di3d_sphere_wall3d_cyl"])
def test_step_wise_entry_points_per_game(alg, orc, name):
    c = Case(alg, name, B=4, seed=3)
    g = c.g
    rng = np.random.default_rng(11)
    z = rng.random((c.B, g.traj_len)); z[:, :g.n] = c.x0
    lam, mu = rng.random((c.B, g.con_len)), 1.0 + rng.random((c.B, g.con_len))
    g.set_traj(z); g.set_con_duals(lam, mu)
    os_ = []
    for game in range(c.B):
        o = c.oracle(orc, game)
        assert o.con_len == g.con_len
        o.set_traj(z[game:game + 1]); o.set_con_duals(lam[game:game + 1], mu[game:game + 1])
        os_.append(o)
    rg, ng = g.residual(0, 1e-3)
    Jg = g.residual_jacobian(1e-3)
    vg = g.violation_profile()
    for game, o in enumerate(os_):
        ro, no = o.residual(0, 1e-3)
        assert np.abs(rg[game] - ro[0]).max() <= 1e-12 * (1 + np.abs(ro).max())
        Jo = o.residual_jacobian(1e-3)
        assert np.abs(Jg[game] - Jo[0]).max() <= 1e-12 * np.abs(Jo).max()
        vo = o.violation_profile()
        for f in ("dyn", "con", "sta", "opt"):
            assert np.allclose(vg[f][game], vo[f][0], rtol=1e-12, atol=1e-14), f
    vals_g = g.dual_penalty_update()
    for game, o in enumerate(os_):
        vals_o = o.dual_penalty_update()
        fin = np.isfinite(vals_o[0])
        assert np.array_equal(np.isfinite(vals_g[game]), fin)
        assert np.allclose(vals_g[game][fin], vals_o[0][fin], rtol=1e-12, atol=1e-14)
        (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
        assert np.allclose(lg[game], lo[0], rtol=1e-12, atol=1e-14) and np.array_equal(mg[game], mo[0])
    ig = g.newton_step(1, 1)
    for game, o in enumerate(os_):
        io = o.newton_step(1, 1)
        for f in ("status", "control_flow", "ls_j", "ls_failed"):
            assert ig[f][game] == io[f][0], f
        assert np.allclose(ig["rec"]["res"][game], io["rec"]["res"][0], rtol=1e-9)
        assert np.abs(g.get_traj()[game] - o.get_traj()[0]).max() <= 1e-8 * max(1.0, np.abs(o.get_traj()).max())


def test_ibr_per_game(alg, orc):
    c = Case(alg, "di3_cost_avoid_ctl", B=4, seed=4)
    st = c.g.ibr_newton_solve(ibr_iter=3, init=True, game_id0=GID0)
    for game in range(c.B):
        o = c.oracle(orc, game)
        so = o.ibr_newton_solve(ibr_iter=3, init=True, game_id0=GID0 + game)
        for f in ("status", "converged"):
            assert st[f][game] == so[f][0], f
        assert np.abs(c.g.get_traj()[game] - o.get_traj()[0]).max() <= 1e-8 * max(1.0, np.abs(o.get_traj()).max())


def test_mpc_per_game(alg, orc):
    c = Case(alg, "di3_cost_avoid_ctl", B=8, seed=5)
    sg = c.g.mpc_solve(10, game_id0=GID0, record_states=True)
    for game in range(c.B):
        o = c.oracle(orc, game)
        so = o.mpc_solve(10, game_id0=GID0 + game, record_states=True)
        assert np.abs(sg[:, game] - so[:, 0]).max() <= 1e-8 * max(1.0, np.abs(so).max())      # states (steps + 1, B, n)


def _all_outputs(b):
    st = b.get_stats()
    (lam, mu) = b.get_con_duals()
    return [b.get_traj(), lam, mu] + [st[f] for f in ("status", "outer_iters", "newton_iters", "records", "converged")] + \
           [st["last"][f] for f in ("res", "dyn_vio", "con_vio", "sta_vio", "opt_vio")]


@pytest.mark.parametrize("name", ["di3_cost_avoid_ctl", "uni4_walls_player_circles", "bic2_state_bound"])
def test_permuting_the_games_permutes_every_output(alg, name):
    c = Case(alg, name, B=8, seed=6)
    perm = np.random.default_rng(1).permutation(c.B)
    c2 = Case(alg, name, B=8, seed=6, per_game=False)
    c2.x0, c2.Q, c2.R, c2.xf, c2.uf = c.x0[perm], c.Q[perm], c.R[perm], c.xf[perm], c.uf[perm]
    c2.g.set_x0(c2.x0); c2.g.set_lqr(c2.Q, c2.R, c2.xf, c2.uf)
    for kind, v, pack, _ in c.ingr:
        c2.g.set_scenario_data(kind, np.stack([pack(v[k]) for k in perm]))
    # the generator is keyed by game: the permuted batch starts from the permuted initial guesses
    c.g.init_traj(game_id0=GID0)
    c2.g.set_traj(c.g.get_traj()[perm])
    c.g.newton_solve(init=False); c2.g.newton_solve(init=False)
    for a, b in zip(_all_outputs(c.g), _all_outputs(c2.g)):
        assert np.array_equal(a[perm], b)


def test_identity_per_game_equal_to_shared_is_bit_identical(alg):
    a = Case(alg, "di3_cost_avoid_ctl", B=8, seed=7, per_game=False)
    b = Case(alg, "di3_cost_avoid_ctl", B=8, seed=7, per_game=False)
    # handle a: EXT with shared values (a wall pushes it to the EXT instantiation); handle b: the same + per-game copies of them
    for c in (a, b):
        c.g.add_wall_constraint([5.0], [5.0], [6.0], [5.0], [0.0], [1.0])       # far away: inert, but EXT
    for kind, v, pack, _ in b.ingr:
        b.g.set_scenario_data(kind, np.tile(pack(v[0]), (b.B, 1)))
    a.g.newton_solve(init=True, game_id0=GID0); b.g.newton_solve(init=True, game_id0=GID0)
    for x, y in zip(_all_outputs(a.g), _all_outputs(b.g)):
        assert np.array_equal(x, y)
    for game in range(a.B):
        ha, hb = a.g.get_history(game), b.g.get_history(game)
        for f in ha.dtype.names:
            if f != "t_elap":                                      # (wall time of the iteration)
                assert np.array_equal(ha[f], hb[f]), f


def test_warm_start_keeps_the_duals(alg, orc):
    c = Case(alg, "di3_cost_avoid_ctl", B=4, seed=8)
    g = c.g
    g.newton_solve(init=True, game_id0=GID0)
    lam0, mu0 = g.get_con_duals()
    kind, v, pack, add = c.ingr[1]                               # collision avoidance: move the radii
    v2 = v * 1.1
    g.set_scenario_data(kind, np.stack([pack(x) for x in v2]))
    lam1, mu1 = g.get_con_duals()
    assert np.array_equal(lam0, lam1) and np.array_equal(mu0, mu1)
    z = g.get_traj()
    g.set_options(dual_reset=0)
    st = g.newton_solve(init=False, game_id0=GID0)
    c.ingr[1] = (kind, v2, pack, add)
    for game in range(c.B):
        o = c.oracle(orc, game)
        o.set_options(dual_reset=0)
        o.set_traj(z[game:game + 1]); o.set_con_duals(lam0[game:game + 1], mu0[game:game + 1])
        so = o.newton_solve(init=False, game_id0=GID0 + game)
        _same_solve(g, o, game, st, so)


def test_errors(alg):
    c = Case(alg, "di3_cost_avoid_ctl", B=2, seed=9)
    g = c.g
    E = alg.AlgamesError
    u = g.get_scenario_data(K_CTL)
    bad = u.copy(); bad[1, 0] = 1.0                               # u_max[0] is +inf on the handle
    with pytest.raises(E, match="code -1"):
        g.set_scenario_data(K_CTL, bad)
    bad = u.copy(); bad[0, 1], bad[0, g.m + 1] = -1.0, 1.0        # u_max < u_min
    with pytest.raises(E, match="code -1"):
        g.set_scenario_data(K_CTL, bad)
    r = g.get_scenario_data(K_RAD)
    bad = r.copy(); bad[1, 1] = 0.0                               # pair (0, 1) exists
    with pytest.raises(E, match="code -1"):
        g.set_scenario_data(K_RAD, bad)
    ok = r.copy(); ok[:, 0] = -5.0                                # the diagonal is ignored
    g.set_scenario_data(K_RAD, ok)
    assert np.array_equal(g.get_scenario_data(K_RAD)[:, 0], r[:, 0])
    assert g.scenario_data_len(K_SB) == 0
    with pytest.raises(E, match="code -3"):
        g.set_scenario_data(K_SB, np.zeros((2, 0)))
    with pytest.raises(ValueError):
        g.set_scenario_data(K_CTL, np.zeros((3, 2 * g.m)))
    # an adder drops the per-game data
    g.set_scenario_data(K_CTL, np.stack([u[0], u[0] * 0.5]))
    assert not np.array_equal(g.get_scenario_data(K_CTL)[1], u[0])
    g.add_control_bound(u[0][:g.m], u[0][g.m:])
    assert np.array_equal(g.get_scenario_data(K_CTL), np.tile(u[0], (2, 1)))
    # no EXT instantiation: DoubleIntegrator d = 1
    h = alg.Batch(alg.hip_lib(), DI, 2, 6, 0.1, 2, d=1)
    h.add_collision_cost(np.ones(2), np.ones(2))
    with pytest.raises(E, match="EXT kernel"):
        h.set_scenario_data(K_COST, np.ones((2, 4)))


def test_shards_of_one_game_and_of_equal_games_take_the_whole_batchs_path(alg):
    """a shard of one game, or of games whose numbers are equal, runs the EXT kernels like the whole batch: same bits"""
    from algames_jl_amd import scenarios, sharding
    B = 4
    model, N, dt, x0, obj, con, opts = scenarios.c2_double_integrator(np.arange(B), N=12)
    cons = []
    for k in range(B):
        gc = alg.GameConstraintValues(alg.ProblemSize(N, model))
        alg.add_collision_avoidance(gc, 0.12 if k < 2 else 0.1 + 0.01 * k)       # games 0 and 1 equal
        cons.append(gc)
    whole = alg.GameProblem(N, dt, x0, model, opts, obj, cons)
    for devices in ([0, 0], [0, 0, 0, 0]):
        sh = sharding.ShardedGameProblem(N, dt, x0, model, opts, obj, cons, devices=devices)
        alg.newton_solve(whole)
        sharding.newton_solve_sharded(sh)
        assert np.array_equal(whole.batch.get_traj(), sh.get_traj()), devices


def test_active_set_analysis_uses_each_games_own_radii(alg):
    """active_set on a problem built from one GameConstraintValues per game: game 1's active set, residual and null space are those
    of game 1's radii (pair radius 2 in game 0: every pair active; 2e-3 in game 1: none), equal to a one-game problem of game 1"""
    A = alg.active_set
    N, p = 10, 3
    model = alg.UnicycleGame(p=p)
    rng = np.random.default_rng(21)
    Q = [rng.random(4) for _ in range(p)]; R = [rng.random(2) for _ in range(p)]
    obj = alg.GameObjective(Q, R, [(i + 1) * np.ones(4) for i in range(p)], [2.0 * (i + 1) * np.ones(2) for i in range(p)], N, model)

    def con(radius):
        gc = alg.GameConstraintValues(alg.ProblemSize(N, model))
        alg.add_collision_avoidance(gc, radius)
        return gc
    x0 = rng.random((2, model.n))
    opts = alg.Options(inner_print=False, outer_print=False)
    prob = alg.GameProblem(N, 0.1, x0, model, opts, obj, [con(1.0), con(1e-3)])
    one = alg.GameProblem(N, 0.1, x0[1:], model, opts, obj, [con(1e-3)], game_id0=1)
    prob.batch.init_traj(0); one.batch.init_traj(1)               # the generator is keyed by game_id0 + g: the same guess
    assert np.array_equal(prob.batch.get_traj()[1], one.batch.get_traj()[0])
    cores = []
    for pr, game in ((prob, 1), (one, 0), (prob, 0)):
        core = A.ActiveSetCore(pr.probsize)
        A.update_nullspace(core, pr, game=game, constraint_rows=True)
        A.residual(core, pr, game=game)
        cores.append(core)
    c1, ref, c0 = cores
    S = prob.probsize.S
    assert c1.vmask == ref.vmask and c1.hmask == ref.hmask
    assert c1.vmask == list(range(1, S + 1))                       # game 1: no pair active
    assert len(c0.vmask) > S                                        # game 0: pairs active
    assert np.abs(c1.jac - ref.jac).max() <= 1e-12 * np.abs(ref.jac).max()
    assert np.abs(c1.res - ref.res).max() <= 1e-12 * max(1.0, np.abs(ref.res).max())
    assert c1.null.mat.shape == ref.null.mat.shape


def test_errors_of_the_extended_kinds(alg):
    """non-finite values where the handle's are finite, x_max < x_min, circle / cylinder radii <= 0: ALG_ERR_ARG, nothing changes"""
    E = alg.AlgamesError
    g = alg.Batch(alg.hip_lib(), DI, 2, 6, 0.1, 2, d=3)
    g.add_collision_cost(np.full(2, 0.3), np.full(2, 2.0))
    xmax = np.full(g.n, np.inf); xmin = np.full(g.n, -np.inf); xmax[:3], xmin[:3] = 1.0, -1.0
    g.add_state_bound(0, xmax, xmin)
    g.add_circle_constraint([0.5], [0.5], [0.2])
    g.add_cylinder_constraint([[0.5, 0.5, 0.0]], [2], [1.0], [0.1])
    before = {k: g.get_scenario_data(k) for k in (K_COST, K_SB, K_CIRC, K_CYL)}

    def refused(kind, game, entry, value, what):
        bad = before[kind].copy(); bad[game, entry] = value
        with pytest.raises(E, match="code -1") as e:
            g.set_scenario_data(kind, bad)
        assert what in str(e.value), str(e.value)
        assert np.array_equal(g.get_scenario_data(kind), before[kind])
    refused(K_COST, 1, 0, np.nan, "non-finite")                    # collision-cost radius of player 0
    refused(K_COST, 0, 3, np.inf, "non-finite")                    # mu of player 1
    refused(K_CIRC, 1, 0, np.inf, "non-finite")                    # xc
    refused(K_CIRC, 1, 2, 0.0, "radius must be positive")
    refused(K_CYL, 0, 4, -0.1, "radius must be positive")
    refused(K_SB, 1, 0, -2.0, "Upper bounds")                      # x_max[0] of player 0 below x_min[0] = -1
    refused(K_SB, 1, g.n + 5, 0.0, "+-inf pattern")                 # an infinite bound made finite
    ok = before[K_SB].copy(); ok[1, 0] = 0.5                       # and a valid change goes through
    g.set_scenario_data(K_SB, ok)
    assert np.array_equal(g.get_scenario_data(K_SB), ok)


@pytest.mark.timeout(900)
def test_c2_shape_at_4096_games_with_per_game_radii_and_bounds(alg, orc):
    from algames_jl_amd import scenarios
    B = 4096
    model, N, dt, x0, obj, con, opts = scenarios.c2_double_integrator(np.arange(B))
    rng = np.random.default_rng(12)
    r = 0.1 + 0.05 * rng.random((B, 3))                          # pair radii r_i + r_j in [0.2, 0.3]
    umax = 1.0 + rng.random((B, 6)); umin = -1.0 - rng.random((B, 6))
    g = alg.Batch(alg.hip_lib(), 0, 3, N, dt, B)
    g.set_options(**opts.to_abi())
    Q, R = np.broadcast_to(obj.Qdiag, (B,) + obj.Qdiag.shape).copy(), np.broadcast_to(obj.Rdiag, (B,) + obj.Rdiag.shape).copy()
    xf, uf = np.broadcast_to(obj.xf, (B,) + obj.xf.shape).copy(), np.broadcast_to(obj.uf, (B,) + obj.uf.shape).copy()
    g.set_x0(x0); g.set_lqr(Q, R, xf, uf)
    g.add_collision_cost(obj.collision_radius, obj.collision_μ)
    g.add_collision_avoidance(r[0]); g.add_control_bound(umax[0], umin[0])
    g.set_scenario_data(K_RAD, ((r[:, :, None] + r[:, None, :]) * (1 - np.eye(3))).reshape(B, 9))
    g.set_scenario_data(K_CTL, np.concatenate([umax, umin], axis=1))
    st = g.newton_solve(init=True, game_id0=GID0)
    for game in np.random.default_rng(13).choice(B, 64, replace=False):
        o = orc.OracleBatch(0, 3, N, dt, 1)
        o.set_options(**opts.to_abi())
        o.set_x0(x0[game:game + 1]); o.set_lqr(Q[game:game + 1], R[game:game + 1], xf[game:game + 1], uf[game:game + 1])
        o.add_collision_cost(obj.collision_radius, obj.collision_μ)
        o.add_collision_avoidance(r[game]); o.add_control_bound(umax[game], umin[game])
        so = o.newton_solve(init=True, game_id0=GID0 + int(game))
        _same_solve(g, o, int(game), st, so)
    assert g.lib.debug_check_guards(g.h) == 0


def test_sharded_problem_with_a_list_of_game_cons(alg):
    from algames_jl_amd import scenarios, sharding
    B = 16
    model, N, dt, x0, obj, con, opts = scenarios.c2_double_integrator(np.arange(B), N=12)
    rng = np.random.default_rng(14)
    cons = []
    for k in range(B):
        gc = alg.GameConstraintValues(alg.ProblemSize(N, model))
        alg.add_collision_avoidance(gc, 0.1 + 0.05 * rng.random(3))
        alg.add_control_bound(gc, 1.0 + rng.random(6), -1.0 - rng.random(6))
        cons.append(gc)
    whole = alg.GameProblem(N, dt, x0, model, opts, obj, cons)
    sh = sharding.ShardedGameProblem(N, dt, x0, model, opts, obj, cons, devices=[0, 0])
    alg.newton_solve(whole)
    sharding.newton_solve_sharded(sh)
    assert np.array_equal(whole.batch.get_traj(), sh.get_traj())
    a, b = whole.batch.get_stats(), sh.get_stats()
    for f in ("status", "newton_iters", "converged"):
        assert np.array_equal(a[f], b[f])
