"""Every configuration of the four log kernels -- k_player_cost<C>, k_con_values<C> (a stored plan: alg_get_cost, alg_get_con_values) and
k_closed_loop_cost<C>, k_closed_loop_con<C> (the log of the fused receding-horizon loop: alg_mpc_get_cost, alg_mpc_get_con) -- and the plans and
closed-loop runs their tests use (tests/test_log_config_family.py on the CPU, tests/test_gpu_log_configs.py on the GPU).  No test lives here.

The configurations, and how a handle reaches each one, are kkt_config_family's (CONFIGS: the 79 entries of ALG_CFGS_ONE; pair_problem: the
all-player adders of the parity tests' _pair helpers, numbers recorded by param_reference.recorded).  The references are cost_reference and
con_reference; the structure tables con_reference needs are read back from a device handle (con_reference.tables_from_batch) and, for the
CPU, rebuilt here from the recorded adder arguments (tables_recorded) -- the GPU test holds the two against each other.

The cost kernels deal items (knot, player) to L(p) = KPT(p) p lanes, KPT(p) = 64 // p knots per trip.

Plans.  Horizons N in {2, 3, KPT, KPT + 1, 2 KPT + 1}: the trip edges of the cost kernels and a third trip of one knot (p = 10: 2, 3, 6, 7, 13;
p = 1: 2, 3, 64, 65, 129).  A plan is a trajectory set through set_traj, no solve.  It is drawn as con_reference._draw_case draws z
(0.8 normal, x0 = 0.5 normal in front) and redrawn with the next sub-seed, at most 50 times, until con_reference.preconditions holds (margin
>= 1e-6, every kind the handle carries with rows of both signs); decided in numpy before a device sees it.  The LQR numbers of a plan handle
are the recorded ones with zero entries of Q and R (uf != 0 already), as test_gpu_cost._numbers has them.  Should alg_create refuse a long
horizon of a dense kind, plan_handle walks down to the largest accepted horizon that still gives a second trip (N >= KPT + 1).

Closed-loop runs.  One per configuration: B = 3 games, N = 4, outer_iter = 1, inner_iter = 2 (the logs are evaluated on whatever the loop
returns; the quadrotor takes inner_iter = 6, see options_of), Plant(2, 2, "rk4") at even positions of CONFIGS and the default plant at odd ones, the smallest number of steps with
steps hold >= 2 KPT + 1 knots, a four-row disturbance of +-0.01, a two-row lqr_target schedule at even positions.

What the library admits decides the rest.  A schedule of a scenario kind makes the kind per game exactly as alg_set_scenario_data does: on a
handle of the base set (E = 0) that switches the handle to its EXT instantiation, in ALG_SCEN_KERNELS_BASE mode (E = 2) a base kind cannot be
scheduled at all, and one dimension has neither.  A run that is to launch the kernels of ITS configuration can therefore carry
    E = 0   no scenario schedule and no per-game block: the collision cost comes from the handle's shared values (source 2);
    E = 2   per-game control bounds and pair radii in the blocks (kkt_config_family.pair_problem), the collision cost from a per-game block
            (source 1) or the shared values (2);
    E = 1   a two-row control_bound schedule and a two-row schedule of one more kind (circle on the planar sets, cylinder on the 3-D sets);
            the collision cost from a two-row schedule (0), a per-game block (1) or the shared values (2).
Within what its E admits the members of a class take the sources in turn (SOURCE); one player has no pairs and no collision cost.
The module-level assertion holds that every cfg_class meets every source the library admits for one of its members, and both plants."""
import contextlib
import types

import numpy as np

import algames_jl_amd as A
import con_reference as KR
import cost_reference as CR
import kkt_config_family as F
import kkt_reference as K
import param_reference as PR

DI, UNI, BIC, QUAD = K.DI, K.UNI, K.BIC, K.QUAD
CONFIGS, IDS, how, cfg_class, pair_problem = F.CONFIGS, F.IDS, F.how, F.cfg_class, F.pair_problem
B, N_LOOP, DT, GID0 = 3, 4, K.DT, 11
WAVE = 64
SRC_SCHEDULE, SRC_BLOCK, SRC_SHARED = 0, 1, 2
ADMITTED = {0: (SRC_SHARED,), 2: (SRC_BLOCK, SRC_SHARED), 1: (SRC_SCHEDULE, SRC_BLOCK, SRC_SHARED)}
# (configuration) -> sub-seed of its closed-loop data where sub-seed 0 misses a precondition of tests/test_log_config_family.py
LOOP_SEED = {(BIC, 4, 2, 1): 1, (DI, 9, 2, 1): 3, (QUAD, 3, 3, 1): 2}
# (configuration, N) -> first sub-seed of its plan draw (the redraw loop starts there)
PLAN_SEED = {((DI, 2, 3, 1), 2): 100}


def KPT(p):
    return WAVE // p


def L(p):
    return KPT(p) * p


def plan_horizons(cfg):
    k = KPT(cfg[1])
    return sorted({2, 3, k, k + 1, 2 * k + 1} - {0, 1})


def model_of(cfg):
    model, p, d, _ = cfg
    return {DI: lambda: A.DoubleIntegratorGame(p=p, d=d), UNI: lambda: A.UnicycleGame(p=p), BIC: lambda: A.BicycleGame(p=p),
            QUAD: lambda: A.QuadrotorGame(p=p)}[model]()


def plant_of(i):
    """(hold, substeps, integrator) of the configuration at position i, None for the default plant"""
    return (2, 2, "rk4") if i % 2 == 0 else None


def _sources():
    """Within what its E admits, the members of a cfg_class take the sources in turn, in the order of CONFIGS: a class with two EXT
    members that have pairs (the 3-D double integrators) gets the schedule and the block from them and the shared values from its base
    members.  One player has no pairs and no collision cost: None."""
    turn, out = {}, {}
    for cfg in CONFIGS:
        if cfg[1] == 1:
            out[cfg] = None
            continue
        adm, key = ADMITTED[cfg[3]], (cfg_class(cfg), cfg[3])
        out[cfg] = adm[turn.get(key, 0) % len(adm)]
        turn[key] = turn.get(key, 0) + 1
    return out


SOURCE = _sources()
for _cls in sorted({cfg_class(c) for c in CONFIGS}):
    _mem = [(i, c) for i, c in enumerate(CONFIGS) if cfg_class(c) == _cls]
    _admitted = {s for _, c in _mem if c[1] > 1 for s in ADMITTED[c[3]]}
    assert {SOURCE[c] for _, c in _mem} - {None} == _admitted, (_cls, "collision-cost sources")
    assert {plant_of(i) is None for i, _ in _mem} == {True, False}, (_cls, "plants")


def options_of(cfg):
    """outer_iter = 1, inner_iter = 2; six Newton iterations for the quadrotor.  Its players fall (the control bounds of the parity problems
    do not carry their weight), which the logs do not mind, but after two iterations the plans leave the body rates undamped and single runs
    reach the finite escape time of the rate dynamics within the 65 to 129 knots: not finite, so not comparable (with four iterations one of the eight still does).  With six the solves have
    converged -- eight give the same runs to three digits -- and every quadrotor run is finite (asserted on the oracle by tests/test_log_config_family.py, on the device by the GPU test)."""
    return dict(outer_iter=1, inner_iter=6 if cfg[0] == QUAD else 2)


def steps_of(cfg, hold):
    return -(-(2 * KPT(cfg[1]) + 1) // hold)


# ---- the structure tables, from the recorded adder arguments -------------------------------------------------------------------------------------
_TABLE_ADDERS = ("add_state_bound", "add_wall_constraint", "add_circle_constraint", "add_wall3d_constraint", "add_cylinder_constraint")


@contextlib.contextmanager
def recorded_tables():
    """while active, every Batch keeps the arguments of its extended all-player adders in self._tab (state bounds: per player)"""
    orig = {k: getattr(A.Batch, k) for k in _TABLE_ADDERS}

    def wrap(k):
        def f(self, *a):
            tab = self.__dict__.setdefault("_tab", {})
            if k == "add_state_bound":
                tab.setdefault(k, {})[int(a[0])] = (np.array(a[1], dtype=np.float64), np.array(a[2], dtype=np.float64))
            else:
                tab[k] = tuple(np.array(v, dtype=np.float64) for v in a)
            return orig[k](self, *a)
        return f
    for k in _TABLE_ADDERS:
        setattr(A.Batch, k, wrap(k))
    try:
        yield
    finally:
        for k in _TABLE_ADDERS:
            setattr(A.Batch, k, orig[k])


def problem(alg, orc, cfg, N, B=B):
    """kkt_config_family.pair_problem with the extended adders' arguments recorded as well"""
    with recorded_tables():
        return pair_problem(alg, orc, cfg, N, B=B)


def tables_recorded(tw):
    """con_reference's tables (the dict of tables_from_batch) of an oracle twin, from the recorded numbers: every pair, every table entry for
    every player, state bounds of the players that got one (the others: infinite)"""
    o = tw[0][0]
    p, n = o.p, o.n
    per = [PR.numbers(q, gi) for q, gi in tw]
    nums = {}
    if "pair" in per[0]:
        nums[KR.S_CAR] = np.stack([x["pair"].reshape(-1) for x in per])
    if "umax" in per[0]:
        nums[KR.S_CTL] = np.stack([np.concatenate([x["umax"], x["umin"]]) for x in per])
    t = getattr(o, "_tab", {})
    tile = lambda a: np.tile(np.asarray(a, dtype=np.float64).reshape(1, -1), (len(tw), 1))
    axes = None
    if "add_state_bound" in t:
        sb = np.stack([np.full((p, n), np.inf), np.full((p, n), -np.inf)])
        for i, (xmax, xmin) in t["add_state_bound"].items():
            sb[0, i], sb[1, i] = xmax, xmin
        nums[KR.S_SB] = tile(sb)
    if "add_wall_constraint" in t:
        nums[KR.S_WALL] = tile(np.stack(t["add_wall_constraint"], axis=1))
    if "add_circle_constraint" in t:
        nums[KR.S_CIRC] = tile(np.stack(t["add_circle_constraint"], axis=1))
    if "add_wall3d_constraint" in t:
        nums[KR.S_WALL3] = tile(np.stack([a.reshape(-1, 3) for a in t["add_wall3d_constraint"]], axis=1))
    if "add_cylinder_constraint" in t:
        pp, ax, ln, r = t["add_cylinder_constraint"]
        nums[KR.S_CYL] = tile(np.concatenate([pp.reshape(-1, 3), ln.reshape(-1, 1), r.reshape(-1, 1)], axis=1))
        axes = ax.astype(int)
    masks = {k: np.ones((p, nums[k].shape[1] // w), dtype=bool) for k, w in ((KR.S_WALL, 6), (KR.S_CIRC, 3), (KR.S_WALL3, 12), (KR.S_CYL, 5)) if k in nums}
    return dict(nums=nums, pairs=~np.eye(p, dtype=bool), spherical=getattr(o, "_dims", 2) == 3, masks=masks, axes=axes)


def tables_device(g, tw):
    """tables_from_batch of the device handle, held against the recorded tables: the same kinds, the same numbers (the diagonal of the pair
    table carries no pair), the state bounds of a subset of players and the cylinders' axes included"""
    rec = tables_recorded(tw)
    tab = KR.tables_from_batch(g, spherical=rec["spherical"], axes=rec["axes"])
    assert sorted(tab["nums"]) == sorted(rec["nums"]), (sorted(tab["nums"]), sorted(rec["nums"]))
    off = ~np.eye(g.p, dtype=bool).reshape(-1)
    for k, a in rec["nums"].items():
        d = tab["nums"][k]
        assert d.shape == a.shape, (k, d.shape, a.shape)
        sel = off if k == KR.S_CAR else slice(None)
        assert np.array_equal(d[:, sel], a[:, sel]), ("the handle's numbers of kind %d are not the recorded ones" % k)
    return tab


def lqr_numbers(tw):
    """Q, xf (B, p, ni), R, uf (B, p, mi) of the twin's games"""
    per = [PR.numbers(q, gi) for q, gi in tw]
    return tuple(np.stack([x[k] for x in per]) for k in ("Q", "R", "xf", "uf"))


def cost_numbers(tw):
    """(rad, mu) (B, p) of the recorded collision cost, (None, None) without one"""
    per = [PR.numbers(q, gi) for q, gi in tw]
    if "cc_r" not in per[0]:
        return None, None
    return np.stack([x["cc_r"] for x in per]), np.stack([x["cc_mu"] for x in per])


# ---- plans --------------------------------------------------------------------------------------------------------------------------------------
def plan_lqr(tw):
    """the recorded LQR numbers with zero entries of Q and R (test_gpu_cost._numbers); uf != 0 as recorded"""
    Q, R, xf, uf = (a.copy() for a in lqr_numbers(tw))
    p, ni = Q.shape[1], Q.shape[2]
    Q[:, 0, 1] = 0.0; R[:, 0, 0] = 0.0; Q[:, p - 1, ni - 1] = 0.0
    assert np.all(uf != 0.0)
    return Q, R, xf, uf


def draw_plan(cfg, N, tab, stub, sub=0):
    """(z (B, traj_len), attempts) of the plan of (cfg, N); sub > 0: a further trajectory of the same handle (the trial buffer)"""
    n, m, p = stub.n, stub.m, stub.p
    first = PLAN_SEED.get((cfg, N), 0)
    for attempt in range(first, first + 50):
        rng = np.random.default_rng([4000 + sub, CONFIGS.index(cfg), N, attempt])
        z = 0.8 * rng.normal(size=(stub.B, n + (N - 1) * (n + m + p * n)))
        z[:, :n] = 0.5 * rng.normal(size=(stub.B, n))
        try:
            KR.preconditions(*KR.plan(stub, tab, tab["nums"], z, N))
            return z, attempt - first + 1
        except AssertionError:
            continue
    raise AssertionError("no plan of %s at N = %d meets con_reference.preconditions in 50 draws" % (F.cfg_id(cfg), N))


def stub_of(b, games=B):
    return types.SimpleNamespace(B=games, p=b.p, n=b.n, m=b.m, mi=b.mi)


def plan_handle(alg, orc, cfg, N):
    """(handle, twin, N in force): walks down from N while alg_create refuses the horizon, never below a second trip"""
    floor = min(N, KPT(cfg[1]) + 1)
    while True:
        try:
            g, tw = problem(alg, orc, cfg, N)
            return g, tw, N
        except A.AlgamesError:
            if N <= floor:
                raise
            N -= 1


# ---- closed-loop runs -----------------------------------------------------------------------------------------------------------------------------
class Run:
    """The data of the closed-loop run of one configuration: everything but the handle.  `tab` are the handle's structure tables (recorded
    or read back) and `tw` its oracle twin; the schedules and blocks are drawn from them."""

    def __init__(self, cfg, tw, tab, plant="position", source="position", target="position", steps=None):
        i = CONFIGS.index(cfg)
        model, p, d, E = cfg
        o = tw[0][0]
        self.cfg, self.i, self.p, self.n, self.m, self.ni, self.mi = cfg, i, p, o.n, o.m, o.n // p, o.mi
        self.plant = plant_of(i) if plant == "position" else plant
        self.hold = 1 if self.plant is None else self.plant[0]
        self.steps = steps_of(cfg, self.hold) if steps is None else steps
        self.knots = self.steps * self.hold
        self.source = SOURCE[cfg] if source == "position" else source
        rng = np.random.default_rng([7000 + LOOP_SEED.get(cfg, 0), i])
        self.Q, self.R, self.xf, self.uf = lqr_numbers(tw)
        self.rad, self.mu = cost_numbers(tw)
        self.W = 0.01 * (2.0 * rng.random((4, B, o.n)) - 1.0)
        self.tgt = None
        if (i % 2 == 0) if target == "position" else target:
            self.tgt = np.stack([np.concatenate([(self.xf + 0.2 * t * (rng.random(self.xf.shape) - 0.5)).reshape(B, -1),
                                                 (self.uf * (1.0 + 0.3 * t)).reshape(B, -1)], axis=1) for t in range(2)])
        # collision cost: radii on both sides of the players' distances (x0 in the unit box), another radius and mu per game and row
        self.cc_rows = self.cc_block = None
        one = lambda t: np.concatenate([0.3 + 0.6 * rng.random((B, p)), (1.0 + np.arange(p)) * (1.0 + 0.5 * t + 0.3 * rng.random((B, p)))], axis=1)
        if self.source == SRC_SCHEDULE:
            self.cc_rows = np.stack([one(0), one(1)])
        elif self.source == SRC_BLOCK:
            self.cc_block = one(0)
        # constraint schedules, on the EXT sets only (the docstring of this file)
        self.sched = {}
        if E == 1:
            ctl = tab["nums"][KR.S_CTL]
            grow = lambda t: 1.0 + 0.2 * t + 0.05 * np.arange(B)[:, None]
            self.sched[KR.S_CTL] = np.stack([np.where(np.isfinite(ctl), ctl * grow(t), ctl) for t in range(2)])
            if KR.S_CYL in tab["nums"]:
                cyl = tab["nums"][KR.S_CYL].reshape(B, -1, 5)
                step = np.array([0.03, -0.02, 0.02, 0.05, 0.04]) * (1.0 + 0.2 * rng.random((B, cyl.shape[1], 1)))
                self.sched[KR.S_CYL] = np.stack([(cyl + t * step).reshape(B, -1) for t in range(2)])
            elif KR.S_CIRC in tab["nums"]:
                circ = tab["nums"][KR.S_CIRC].reshape(B, -1, 3)
                step = np.array([0.02, -0.03, 0.05]) * (1.0 + 0.2 * rng.random((B, circ.shape[1], 1)))
                self.sched[KR.S_CIRC] = np.stack([(circ + t * step).reshape(B, -1) for t in range(2)])

    # -- the device ------------------------------------------------------------------------------------------------------------------------------
    def configure(self, g, alg, cost_log=True, con_log=True, games=slice(None)):
        """options, plant, schedules, blocks and logs on a device handle of the configuration (games: the games of the run the handle carries)"""
        g.set_options(**options_of(self.cfg))
        if self.plant is not None:
            g.mpc_set_plant(alg.Plant(*self.plant))
        g.mpc_set_schedule("disturbance", self.W[:, games])
        if self.tgt is not None:
            g.mpc_set_schedule("lqr_target", self.tgt[:, games])
        if self.cc_rows is not None:
            g.mpc_set_schedule("collision_cost", self.cc_rows[:, games])
        if self.cc_block is not None:
            g.set_scenario_data("collision_cost", self.cc_block[games])
        for k, a in self.sched.items():
            g.mpc_set_schedule(int(k), a[:, games])
        g.mpc_set_cost_log(cost_log); g.mpc_set_con_log(con_log)

    # -- the references ----------------------------------------------------------------------------------------------------------------------------
    def cost_rows_in_force(self):
        """(knots, B, 2 p) [radius | mu] of every knot, None without a collision cost"""
        if self.rad is None:
            return None
        if self.cc_rows is not None:
            return np.stack([self.cc_rows[min(q // self.hold, 1)] for q in range(self.knots)])
        row = self.cc_block if self.cc_block is not None else np.concatenate([self.rad, self.mu], axis=1)
        return np.tile(row[None], (self.knots, 1, 1))

    def cost_reference(self, states, controls):
        """(stage, total, tol_stage, tol_total): cost_reference.closed_loop_cost with the rows, the block or the shared values according to the
        source, and the tolerance of test_gpu_cost._check_loop -- cost_reference.bound with dt mu r^2 (p - 1) of the row in force"""
        p = self.p
        rad, mu = self.rad, self.mu
        if self.cc_block is not None:
            rad, mu = self.cc_block[:, :p], self.cc_block[:, p:]
        ref_s, ref_t = CR.closed_loop_cost(model_of(self.cfg), DT, self.hold, states, controls, self.Q, self.R, self.xf, self.uf, rad, mu,
                                           target_rows=self.tgt, cost_rows=self.cc_rows)
        rows = self.cost_rows_in_force()
        if rows is None:
            return ref_s, ref_t, CR.bound(ref_s), CR.bound(ref_t)
        sc = DT * rows[..., p:] * rows[..., :p] ** 2 * (p - 1)                       # (knots, B, p)
        return ref_s, ref_t, CR.bound(ref_s, sc), CR.bound(ref_t, sc.sum(axis=0))

    def con_reference(self, b, tab, states, controls):
        """vals, scale, margin (knots, B, K1), kinds (K1,)"""
        return KR.closed_loop(b, tab, tab["nums"], states, controls, self.hold, self.sched or None)

    # -- the same loop on the oracle ---------------------------------------------------------------------------------------------------------------
    def oracle_loop(self, orc, alg):
        """states (knots + 1, B, n), controls (knots, B, m): step-wise solves on the oracle joined by the numpy plant, the schedules applied
        row by row (host.mpc_rollout's step-wise form).  The oracle's constraint numbers are shared by a batch, so game k runs on a handle
        of its own that carries game k's rows."""
        states, controls = np.zeros((self.knots + 1, B, self.n)), np.zeros((self.knots, B, self.m))
        for k in range(B):
            _, tw = problem(alg, orc, self.cfg, N_LOOP)
            o, gi = tw[k]
            s, c = self._oracle_game(o, gi, k)
            states[:, k], controls[:, k] = s, c
        return states, controls

    def _oracle_game(self, o, gi, k):
        model, p, d, E = self.cfg
        n, m, hold = self.n, self.m, self.hold
        o.set_options(**options_of(self.cfg))
        x = o.get_traj()[:, :n].copy()
        states, controls = [x[gi].copy()], []
        lqr = [a if o.B > 1 else a[k:k + 1] for a in (self.Q, self.R, self.xf, self.uf)]
        if self.cc_block is not None:
            o.add_collision_cost(self.cc_block[k, :p], self.cc_block[k, p:])
        for t in range(self.steps):
            if t == 1:
                o.set_options(shift=hold, dual_reset=0)
            r = min(t, 1)
            if t <= 1:                                   # two rows everywhere: the second is held
                if self.tgt is not None:
                    row = self.tgt[r] if o.B > 1 else self.tgt[r, k:k + 1]
                    w = p * self.ni
                    o.set_lqr(lqr[0], lqr[1], row[:, :w].reshape(-1, p, self.ni), row[:, w:].reshape(-1, p, self.mi))
                if self.cc_rows is not None:
                    o.add_collision_cost(self.cc_rows[r, k, :p], self.cc_rows[r, k, p:])
                if self.sched:
                    lam, mu = o.get_con_duals()
                    o.add_control_bound(self.sched[KR.S_CTL][r, k, :m], self.sched[KR.S_CTL][r, k, m:])
                    if KR.S_CIRC in self.sched:
                        c3 = self.sched[KR.S_CIRC][r, k].reshape(-1, 3)
                        o.add_circle_constraint(c3[:, 0], c3[:, 1], c3[:, 2])
                    if KR.S_CYL in self.sched:
                        c5 = self.sched[KR.S_CYL][r, k].reshape(-1, 5)
                        o.add_cylinder_constraint(c5[:, :3], o._tab["add_cylinder_constraint"][1].astype(np.int32), c5[:, 3], c5[:, 4])
                    o.set_con_duals(lam, mu)             # (the oracle's table adders re-create the multipliers; a schedule row does not)
            o.newton_solve_async(init=True, game_id0=GID0 + t * 1000003 + (k - gi))
            zt = o.get_traj()
            for j in range(hold):
                q = t * hold + j
                u = zt[:, 2 * n + j * o.b:2 * n + j * o.b + m]
                controls.append(u[gi].copy())
                x = plant(o, self.cfg, x, u, self.plant)
                x[gi] += self.W[min(q, 3), k]
                states.append(x[gi].copy())
            o.set_x0(np.ascontiguousarray(x))
        return np.stack(states), np.stack(controls)


def plant(o, cfg, x, u_pm, pl):
    """one plant knot of every game of the oracle handle o: test_mpc_plant_family.plant_step for the models it states, the same
    integrators on the oracle's continuous dynamics (kat_dynamics) for the bicycle and the quadrotor"""
    from test_mpc_plant_family import component_major, plant_step
    model, p, d, _ = cfg
    hold, sub, integ = (1, 1, "rk2") if pl is None else pl
    if model in (DI, UNI):
        return plant_step(model, p, d, x, u_pm, DT, sub, integ)
    u = component_major(np.asarray(u_pm, dtype=np.float64), p, o.mi)
    out = np.array(x, dtype=np.float64)
    h = DT / float(sub)
    for g in range(out.shape[0]):
        f = lambda y: o.kat_dynamics(y, u[g])[0]
        y = out[g]
        for _ in range(sub):
            if integ == "rk2":
                y = y + h * f(y + (0.5 * h) * f(y))
            else:
                k1 = f(y); k2 = f(y + (0.5 * h) * k1); k3 = f(y + (0.5 * h) * k2); k4 = f(y + h * k3)
                y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out[g] = y
    return out
