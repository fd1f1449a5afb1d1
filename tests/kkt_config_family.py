"""Every configuration of the KKT column kernel k_kkt_sens<C> (alg_kkt_solve, alg_kkt_sensitivity, alg_kkt_normal_equations), and the problems
its tests run on (tests/test_kkt_config_family.py on the CPU, tests/test_gpu_kkt_configs.py on the GPU).  No test lives here.

CONFIGS is the list ALG_CFGS_ONE expands to in csrc/algames_kernels.hpp, written out: (model, p, d, E) with E = 0 the base constraint set,
E = 1 the extended set (EXT kernels), E = 2 the base kernels reading per-game blocks.  How a handle reaches each one (`how`):

    E = 0   test_gpu_parity._pair with the base ingredients (collision cost, collision avoidance, control bounds); the quadrotor through
            test_gpu_parity_quad._pair
    E = 1   d = 2: test_gpu_parity_ext._pair (the bicycle by its model, the others by state bounds, walls and circles);
            d = 3: test_gpu_parity_dense._pair with all its ingredients (spherical avoidance, 3-D walls, cylinders), two double integrators
            in three dimensions included
    E = 2   the base problem with alg_set_scenario_kernels(BASE) and per-game control bounds (and per-game pair radii where p > 1); the
            oracle twin is then one OracleBatch(B = 1) per game

Horizons: N = 2 puts step 0 on the terminal step, N = 3 is the first with a stage step, N = 5 passes the sweep ring of 4; the index maps
under test (the loader's e -> (k, q, i, s, a, j), con_col / con_ctl / pairq, A_entry, the store's slices of b) depend on the horizon through
first / stage / terminal steps only, and the longer rings and chunk edges of refined_direction are test_gpu_horizon_shapes'.  B = 3 games,
so that the game offsets are in play.

The reference's own figures on these problems (test_kkt_config_family, printed per configuration), worst over all 79 configurations,
N in HORIZONS, reg in {0, 1e-3}:
    numpy solve against its long-double-refined solution, USER columns                        3.3e-12 (bound 1e-11)
    |J X_ref - R| / max(1, |R|_inf), USER and Q / collision_radius / control_bound columns    5.4e-11 (bound 1e-10)
both on ten unicycles, base set, N = 5; every configuration below seven players, and every per-game and pair-table problem, stays under 7e-13 / 5e-12.  The host-written right-hand
sides against central differences of the oracle's residual: 5.9e-10 max |R| at worst on the collision cost's radii, 5.2e-11 on the pair
radii (bound 1e-8), 1.6e-13 on the entries the residual is affine in (bound 1e-12), with no activity flip in any problem.

Also here: the per-game problems (every base kind differs between the games, EXT and BASE kernels) and the partial pair tables
(test_gpu_parity.PAIR_CASES) of the GPU tests, with their oracle twins."""
import numpy as np

import kkt_reference as K
import param_reference as PR

DI, UNI, BIC, QUAD = K.DI, K.UNI, K.BIC, K.QUAD
HORIZONS = (2, 3, 5)
B = 3
K_RAD, K_COST, K_CTL = 0, 1, 2                     # ALG_SCEN_* kinds of the base constraint set

_BASE = [(DI, 1, 2), (DI, 2, 2), (DI, 3, 2), (DI, 4, 2), (DI, 2, 3), (UNI, 1, 2), (UNI, 2, 2), (UNI, 3, 2), (UNI, 4, 2)]
CONFIGS = (
    [c + (0,) for c in _BASE]                                                                   # ALG_CFGS_BASE
    + [c + (2,) for c in _BASE]                                                                 # ALG_CFGS_BASE_SCEN
    + [(m, p, 2, 1) for m in (DI, UNI, BIC) for p in (1, 2, 3, 4)] + [(DI, 2, 3, 1)]            # ALG_CFGS_EXT
    + [(QUAD, p, 3, e) for e in (0, 1) for p in (1, 2, 3, 4)]                                   # ALG_CFGS_QUAD, ALG_CFGS_QUAD_EXT
    + [(DI, p, 3, e) for e in (0, 1) for p in (1, 3, 4)]                                        # ALG_CFGS_DI3D
    + [c for p in range(5, 11) for c in ((DI, p, 2, 0), (DI, p, 2, 1), (UNI, p, 2, 0), (UNI, p, 2, 1), (BIC, p, 2, 1))]   # ALG_CFGS_P5 ... P10
    + [(DI, p, 1, 0) for p in (1, 2, 3, 4)]                                                     # ALG_CFGS_DI1
)
assert len(CONFIGS) == len(set(CONFIGS)) == 79
_MODEL = {DI: "di", UNI: "uni", BIC: "bic", QUAD: "quad"}


def cfg_id(cfg):
    return "%s%d_d%d_e%d" % (_MODEL[cfg[0]], cfg[1], cfg[2], cfg[3])


IDS = [cfg_id(c) for c in CONFIGS]


def how(cfg):
    model, p, d, E = cfg
    if E == 2:
        return "twin"
    if E == 0:
        return "quad" if model == QUAD else "base"
    return "ext" if d == 2 else "dense_ext"


def cfg_class(cfg):
    """the classes the worst figures are quoted by"""
    model, p, d, E = cfg
    if d == 1:
        return "d1"
    if E == 2:
        return "twin"
    if model == QUAD:
        return "quad"
    if p >= 5:
        return "p5-6" if p <= 6 else "p7-10"
    if d == 3 and p != 2:
        return "di d3 dense"
    return ("base", "ext")[E]


def is_device(g):
    return g.lib.prefix == "alg_"


def _twin_bounds(rng, Bn, m):
    umax, umin = 0.6 + 0.1 * rng.random((Bn, m)), -0.4 - 0.1 * rng.random((Bn, m))
    umax[:, 0] = np.inf
    return umax, umin


def pair_problem(alg, orc, cfg, N, B=B):
    """(device batch, oracle twin) of configuration cfg on the random full-magnitude data of the parity tests' _pair (every constraint row
    with a multiplier and a penalty of O(1), 30 % of the multipliers zero), seed N, with the numbers recorded (param_reference.recorded).
    alg = kkt_reference.OracleAsProduct(orc) builds the same problem on the CPU."""
    model, p, d, E = cfg
    kind = how(cfg)
    with PR.recorded():
        if kind == "quad":
            import test_gpu_parity_quad as PQ
            g, o = PQ._pair(alg, orc, p, N, B=B, seed=N)
        elif kind == "ext":
            import test_gpu_parity_ext as PE
            g, o = PE._pair(alg, orc, model, p, N, B=B, seed=N)
        elif kind == "dense_ext":
            import test_gpu_parity_dense as PD
            g, o = PD._pair(alg, orc, model, p, N, B, seed=N, ingredients=PD.ALL)
        else:
            from test_gpu_parity import _pair
            g, o = _pair(alg, orc, model, p, d, N, B=B, seed=N)
        if kind != "twin":
            return g, K.twin_of(o)
        # per-game control bounds, and pair radii where there are pairs, on the block-reading twins: game k's numbers on its own OracleBatch
        rs = np.random.default_rng(1000 + N)
        rad = 0.3 + 0.1 * np.arange(p) - 0.1 * rs.random((B, p))        # (below _pair's radii: rows with c < 0 stay)
        umax, umin = _twin_bounds(rs, B, o.m)
        if is_device(g):
            g.set_scenario_kernels(1)
            g.set_scenario_data(K_CTL, np.concatenate([umax, umin], axis=1))
            if p > 1:
                g.set_scenario_data(K_RAD, np.stack([(r[:, None] + r[None, :]).reshape(-1) * (1 - np.eye(p).reshape(-1)) for r in rad]))
        z, (lam, mu) = o.get_traj(), o.get_con_duals()
        rng = np.random.default_rng(N)                   # _pair's own draws, in its order
        ni = o.n // p
        Q, R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, o.mi))
        xf, uf = rng.random((B, p, ni)), rng.random((B, p, o.mi)) - 0.5
        x0 = rng.random((B, o.n))
        assert np.array_equal(x0, z[:, :o.n])
        tw = []
        for k in range(B):
            q = orc.OracleBatch(model, p, N, K.DT, 1, d=d)
            q.set_x0(x0[k:k + 1]); q.set_lqr(Q[k:k + 1], R[k:k + 1], xf[k:k + 1], uf[k:k + 1])
            if p > 1:
                q.add_collision_cost(np.full(p, 3.0), 1.0 + np.arange(p))
                q.add_collision_avoidance(rad[k])
            q.add_control_bound(umax[k], umin[k])
            q.set_traj(z[k:k + 1]); q.set_con_duals(lam[k:k + 1], mu[k:k + 1])
            tw.append((q, 0))
        return g, tw


def per_game_kernels(case, mode):
    """(setting, in use) of alg_get_scenario_kernels on a per-game problem: EXT (0, 1); BASE (1, 2), but (1, 1) with the spherical form"""
    return (0, 1) if mode == "ext" else (1, 1) if case[3] else (1, 2)


def runs_its_kernel(g, cfg):
    """the device handle is the configuration it is named after: model, players, dimension and the kernels the next launch takes"""
    return (g.desc.model, g.p, g.d, g.get_scenario_kernels()[1]) == tuple(cfg)


# ---- per-game numbers of every base kind, EXT and BASE kernels ------------------------------------------------------------------------------------------
# (model, p, d, spherical avoidance, modes); the quadrotor carries collision cost and control bounds only
# (the spherical form is an extended ingredient: asked for the base kernels, its handle stays on the EXT kernels -- the planar form of the
# same configuration is what reaches the block-reading twin of two double integrators in three dimensions)
PER_GAME = [(DI, 3, 2, False, ("ext", "base")), (UNI, 4, 2, False, ("ext", "base")), (DI, 2, 3, True, ("ext", "base")),
            (DI, 5, 2, False, ("ext",)), (QUAD, 2, 3, False, ("ext",)), (DI, 2, 3, False, ("base",))]
# one dimension has neither EXT kernels nor block-reading twins (ALG_CFGS_DI1 is E = 0 only): the library refuses per-game data in both modes
PER_GAME_REFUSED = (DI, 2, 1, False)
PER_GAME_CASES = [(c[:4], mode) for c in PER_GAME for mode in c[4]]
per_game_id = lambda c: "%s%d_d%d%s" % (_MODEL[c[0]], c[1], c[2], "_sph" if c[3] else "")
PER_GAME_IDS = ["%s-%s" % (per_game_id(c), mode) for c, mode in PER_GAME_CASES]
PER_GAME_HORIZONS = (3, 5)
PER_GAME_B = 4
# (case, N) -> seed where seed 0 leaves a collision-cost pair within the difference step of r_i - |d| = 0 (four unicycles, N = 5: one flip).
# A condition on the data, asserted by test_kkt_config_family (flips == 0 on the oracle alone), not a tolerance.
PER_GAME_SEED = {((UNI, 4, 2, False), 5): 1}


class PerGame:
    """The data of one per-game problem: B games that differ in their collision cost (r_i, mu_i), pair radii and control bounds -- the ranges of
    test_gpu_scenario_data._cost / _avoid / _ctl, one infinite bound -- in x0 and in the LQR blocks; a random iterate and multipliers with about
    30 % zeros, so that rows are inactive."""

    def __init__(self, orc, case, N, B=PER_GAME_B, seed=None):
        self.case, self.N, self.B = case, N, B
        model, p, d, sph = case
        seed = PER_GAME_SEED.get((case, N), 0) if seed is None else seed
        o = orc.OracleBatch(model, p, N, K.DT, 1, d=d)
        n, m, mi, ni = o.n, o.m, o.mi, o.n // p
        self.p, self.m = p, m
        rng = np.random.default_rng([seed, N, model, p, d])
        self.Q, self.R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, mi))
        self.xf, self.uf = rng.random((B, p, ni)), 0.2 * (rng.random((B, p, mi)) - 0.5)
        shift = 0.3 if model == QUAD else 0.0                            # (negative rotor commands: test_gpu_parity_quad)
        self.x0 = rng.random((B, n)) - shift
        self.cost = np.concatenate([0.2 + 0.3 * rng.random((B, p)), 1.0 + 2.0 * rng.random((B, p))], axis=1)
        self.rad = None if model == QUAD else 0.08 + 0.06 * rng.random((B, p))
        umax, umin = 0.4 + 0.4 * rng.random((B, m)), -0.3 - 0.4 * rng.random((B, m))
        umax[:, 0] = np.inf
        self.ctl = np.concatenate([umax, umin], axis=1)
        self.rng = rng
        self.z = None

    def iterate(self, b):
        """the random iterate and multipliers, drawn once the constraint layout is known (the same for every batch of the problem)"""
        if self.z is None:
            rng = self.rng
            z = rng.random((self.B, b.traj_len)) - (0.3 if self.case[0] == QUAD else 0.0)
            z[:, :b.n] = self.x0
            # the players close to each other at every step (the first two state blocks, where collision cost and planar avoidance read
            # their positions): distances of 0 ... 0.64, 0.23 on average, against cost radii of 0.2 ... 0.5 and pair radii of 0.16 ... 0.28,
            # so that every game has pairs inside the collision cost and avoidance rows with c >= 0 and with c < 0
            for k in range(self.N - 1):
                at = b.n + K.hx(b, k)
                z[:, at:at + 2 * self.p] = 0.3 + 0.45 * rng.random((self.B, 2 * self.p))
            lam, mu = rng.random((self.B, b.con_len)), 1.0 + 2.0 * rng.random((self.B, b.con_len))
            lam[rng.random((self.B, b.con_len)) < 0.3] = 0.0
            # A control bound enters its right-hand side through the row's activity alone.  So that every game's columns depend on ITS
            # bounds, game k >= 1 holds, at step 0, control 1 between its own upper bound and game 0's and its last control between the two
            # lower bounds, both rows with lambda = 0: active under one game's bound, inactive under the other's.
            p, m = self.p, self.m
            for k in range(1, self.B):
                for half, c in ((0, 1), (1, m - 1)):
                    i, j = c % p, c // p
                    z[k, b.n + K.hu(b, 0, i) + j] = 0.5 * (self.ctl[0, half * m + c] + self.ctl[k, half * m + c])
                    lam[k, p * (p - 1) * (self.N - 1) + half * m + c] = 0.0
            self.z, self.lam, self.mu = z, lam, mu
        assert (b.traj_len, b.con_len) == (self.z.shape[1], self.lam.shape[1])
        return self.z, self.lam, self.mu

    def _adders(self, b, k):
        p, m = self.p, self.m
        b.add_collision_cost(self.cost[k, :p], self.cost[k, p:])
        if self.rad is not None:
            (b.add_spherical_collision_avoidance if self.case[3] else b.add_collision_avoidance)(self.rad[k])
        b.add_control_bound(self.ctl[k, :m], self.ctl[k, m:])

    def device(self, alg, mode, perm=None):
        """the device batch: game 0's numbers through the adders, then every kind per game; mode "ext": set_scenario_data switches the handle
        to the EXT kernels (the default), "base": alg_set_scenario_kernels(BASE) first, None: game 0's numbers for every game.  perm: the
        games in that order."""
        model, p, d, sph = self.case
        perm = np.arange(self.B) if perm is None else np.asarray(perm)
        g = alg.Batch(alg.hip_lib(), model, p, self.N, K.DT, self.B, d=d)
        g.set_x0(self.x0[perm]); g.set_lqr(self.Q[perm], self.R[perm], self.xf[perm], self.uf[perm])
        self._adders(g, 0)
        if mode is not None:
            self.upload(g, mode, perm)
        z, lam, mu = self.iterate(g)
        g.set_traj(z[perm]); g.set_con_duals(lam[perm], mu[perm])
        return g

    def upload(self, g, mode, perm=None):
        """every kind per game (mode as in `device`); yields nothing, raises what the library refuses"""
        p = self.p
        perm = np.arange(self.B) if perm is None else np.asarray(perm)
        if mode == "base":
            g.set_scenario_kernels("base")
        pack = lambda r: (r[:, None] + r[None, :]).reshape(-1) * (1 - np.eye(p).reshape(-1))
        g.set_scenario_data(K_COST, self.cost[perm])
        if self.rad is not None:
            g.set_scenario_data(K_RAD, np.stack([pack(r) for r in self.rad[perm]]))
        g.set_scenario_data(K_CTL, self.ctl[perm])

    def twin(self, orc):
        """one OracleBatch(B = 1) per game, with that game's numbers recorded"""
        model, p, d, sph = self.case
        tw = []
        with PR.recorded():
            for k in range(self.B):
                o = orc.OracleBatch(model, p, self.N, K.DT, 1, d=d)
                o.set_x0(self.x0[k:k + 1]); o.set_lqr(self.Q[k:k + 1], self.R[k:k + 1], self.xf[k:k + 1], self.uf[k:k + 1])
                self._adders(o, k)
                z, lam, mu = self.iterate(o)
                o.set_traj(z[k:k + 1]); o.set_con_duals(lam[k:k + 1], mu[k:k + 1])
                tw.append((o, 0))
        return tw


PER_GAME_KINDS = ("collision_cost", "collision_radius", "control_bound")


def with_numbers_of(o, other, param):
    """a context in which batch o reports batch `other`'s recorded numbers of `param`: what a loader that read another game's block builds"""
    import contextlib
    key = {"collision_cost": "add_collision_cost", "collision_radius": "add_collision_avoidance", "control_bound": "add_control_bound"}[param]

    @contextlib.contextmanager
    def ctx():
        own = o._num
        o._num = dict(own, **{key: other._num[key]})
        try:
            yield
        finally:
            o._num = own
    return ctx()


# ---- partial, asymmetric pair tables ------------------------------------------------------------------------------------------------------------------------------
def pair_table_problem(alg, orc, case, N=5, B=4, stale=False):
    """(device batch, oracle twin, pairs) of a handle of test_gpu_parity.PAIR_CASES at horizon N: collision cost and control bounds of _pair
    (seed 3), collision avoidance on the listed ordered pairs only, each with its own radius, and that test's multipliers (seed 11) -- non-zero
    on the rows of the never-added pairs too.
    stale: the device handle carried the all-pairs form before (added, then taken off with a null radius): the same problem, but the handle's
    table still holds a radius where no pair exists -- on a fresh handle those entries are 0 and a loader that forgot the pair mask would
    write the same zeros."""
    from test_gpu_parity import _pair
    model, p, d, _, pairs, sph = case
    with PR.recorded():
        g, o = _pair(alg, orc, model, p, d, N, B=B, seed=3, ingredients=("cost", "ctl"))
        z = g.get_traj()
        if stale and is_device(g):
            (g.add_spherical_collision_avoidance if sph else g.add_collision_avoidance)(0.5 + 0.1 * np.arange(p))
            g.lib.check((g.lib.add_spherical_collision_avoidance if sph else g.lib.add_collision_avoidance)(g.h, None))
        for b in (g, o):
            for (i, j, r) in pairs:
                b.add_collision_avoidance_pair(i, j, r, spherical=sph)
    rng = np.random.default_rng(11)
    lam, mu = rng.random((B, g.con_len)), 1.0 + 2.0 * rng.random((B, g.con_len))
    lam[rng.random((B, g.con_len)) < 0.3] = 0.0
    assert g.con_len == o.con_len
    for b in (g, o):
        b.set_traj(z); b.set_con_duals(lam, mu)
    return g, K.twin_of(o), pairs
