"""Schedules of the fused receding-horizon loop (alg_mpc_set_schedule): per game and per MPC step values of the numbers that may differ
per game, applied inside alg_mpc_solve's single launch.

  1. fused == step-wise on the device (the step-wise loop applies the step's rows through set_scenario_data / set_lqr: the definition);
  2. the schedule bites, and a schedule whose rows all equal the handle's values reproduces the unscheduled loop bit for bit;
  3. lock-step against the oracle: the oracle has no per-game entry, so game g at step t is compared with its own one-game oracle batch
     built with row t's values, which receives x0, the warm start, lambda and mu from the device before the solve;
  4. the error paths."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

DI, UNI, BIC, QUAD = 0, 1, 2, 3
K_RAD, K_COST, K_CTL, K_SB, K_WALL, K_CIRC, K_W3, K_CYL = range(8)
TARGET = "lqr_target"
GID0 = 7


# ---- 1. fused == step-wise ---------------------------------------------------------------------------------------------------------------
def _final_state(prob):
    b = prob.batch
    lam, mu = b.get_con_duals()
    return b.get_traj(), lam, mu


def _fused_vs_stepwise(alg, ids, steps, rows, waves, share, tol, **kw):
    pf, S = alg.scenarios.c5_scheduled(ids, rows, **kw)
    ps, _ = alg.scenarios.c5_scheduled(ids, rows, **kw)
    for p_ in (pf, ps):
        p_.batch.set_waves_per_game(waves)
    assert pf.batch.get_waves_per_game() == ps.batch.get_waves_per_game()
    it_f, cv_f, st_f = alg.mpc_solve(pf, steps, record_states=True, schedule=S, fused=True)
    it_s, cv_s, st_s = alg.mpc_solve(ps, steps, record_states=True, schedule=S, fused=False)
    same = it_f == it_s
    diff = np.abs(st_f - st_s)[:, same].max()
    print("scheduled fused loop vs step-wise (%d wavefronts per game): seeds with the same iteration total %.4f, max state diff on those %.3e"
          % (pf.batch.get_waves_per_game(), same.mean(), diff))
    assert same.mean() >= share, (np.nonzero(~same)[0], it_f[~same], it_s[~same])
    assert diff < tol, diff
    assert np.array_equal(cv_f[same], cv_s[same])
    assert np.abs(st_f[-1] - st_f[0]).max() > 0.3               # the vehicles really travel
    return pf, ps, S, same


def test_fused_scheduled_loop_equals_the_step_wise_loop_one_wavefront(alg):
    """64 seeds of the scheduled C5 set, one wavefront per game, a moving circle and moving goals, rows < steps (the last row is held).
    The project's rule for fused against step-wise (tests/test_gpu_full_batch.py): >= 98 % of the seeds with equal iteration totals, on
    those the states below 1e-9 and the converged counts equal."""
    steps, rows = 16, 12
    pf, ps, S, same = _fused_vs_stepwise(alg, np.arange(128, 192), steps, rows, 1, 0.98, 1e-9)
    bf, bs = pf.batch, ps.batch
    # the state after the call: the handle's values are the row the last step used -- what the step-wise calls left
    last = S["circle"][rows - 1]
    assert np.array_equal(bf.get_scenario_data("circle"), last) and np.array_equal(bs.get_scenario_data("circle"), last)
    assert bf.mpc_get_schedule("circle") == 0 and bf.mpc_get_schedule(TARGET) == 0      # host.mpc_solve drops what it uploaded
    assert bf.lib.debug_check_guards(bf.h) == 0
    # ... on the device too, scenario blocks and LQR targets: a plain solve after either loop is the same solve
    for b in (bf, bs):
        b.set_options(shift=1, dual_reset=0)
    bit = same & np.all(bf.get_traj() == bs.get_traj(), axis=1)
    sf, ss = bf.newton_solve(init=True, game_id0=99), bs.newton_solve(init=True, game_id0=99)
    eq = same & (sf["newton_iters"] == ss["newton_iters"])
    print("plain solve after the loops: loop states bit-identical for %d seeds, same iteration count for %d, max diff %.3e"
          % (bit.sum(), eq.sum(), np.abs(bf.get_traj() - bs.get_traj())[eq].max()))
    assert eq.sum() >= 0.98 * same.sum()
    assert np.array_equal(bf.get_traj()[bit], bs.get_traj()[bit])
    assert np.abs(bf.get_traj() - bs.get_traj())[eq].max() < 1e-8
    # the LQR targets themselves: the residual at a common point (same trajectory, same multipliers) is the same only with the same xf / uf
    rng = np.random.default_rng(0)
    z, lam, mu = rng.random((bf.B, bf.traj_len)), rng.random((bf.B, bf.con_len)), 1.0 + rng.random((bf.B, bf.con_len))
    p0, _ = alg.scenarios.c5_scheduled(np.arange(128, 192), rows)                        # the targets of row 0, the circle of the last row
    p0.batch.set_scenario_data("circle", last)
    for b in (bf, bs, p0.batch):
        b.set_traj(z); b.set_con_duals(lam, mu)
    rf, rs, r0 = bf.residual()[0], bs.residual()[0], p0.batch.residual()[0]
    assert np.array_equal(rf, rs)
    assert np.abs(r0 - rf).max() > 1e-3


def test_fused_scheduled_loop_equals_the_step_wise_loop_team_of_four(alg):
    """The automatic shape at 64 seeds -- a team of four wavefronts per game, which the tile-path configurations have on the base kernels:
    the set without the circle, moving goals -- against the team's own step-wise run, with the bounds of
    tests/test_gpu_full_batch.py::test_team_kernel_receding_horizon_loop."""
    pf, ps, S, same = _fused_vs_stepwise(alg, np.arange(300, 364), 12, 8, 0, 0.8, 1e-6, circle=False)
    assert pf.batch.get_waves_per_game() == 4
    assert pf.batch.lib.debug_check_guards(pf.batch.h) == 0


# ---- 2. the schedule bites ----------------------------------------------------------------------------------------------------------------
def test_the_schedule_bites_and_a_constant_schedule_changes_nothing(alg):
    """Same seeds, 16 steps, 12 rows: against the loop in the frozen world of row 0 the scheduled loop ends elsewhere.  By the last row the
    goals have moved 0.044 and the circle 0.22 ... 0.33, and the vehicles track the goals with Q = I.  The oracle alone, run step-wise
    on seeds 128 ... 143 with the moving goals only, ends 0.021 ... 1.02 away from its frozen-world run (largest state entry per game,
    median 0.43: where the closed loop meets its hard solves the two runs part for good).  Solver noise between two runs of one loop is
    below 1e-9 (the fused-against-step-wise bound), so: more than 1e-3 in every game -- a million times the noise, a twentieth of the
    smallest figure of the oracle -- and a median above 0.02.  A schedule whose rows all equal the handle's values is the unscheduled
    loop, bit for bit."""
    ids, steps, rows = np.arange(128, 192), 16, 12
    pm, S = alg.scenarios.c5_scheduled(ids, rows)
    frozen = {k: np.repeat(v[:1], rows, axis=0) for k, v in S.items()}
    pu, _ = alg.scenarios.c5_scheduled(ids, rows)
    pu.batch.set_scenario_data("circle", S["circle"][0])           # every game its own circle, nothing scheduled
    pc, _ = alg.scenarios.c5_scheduled(ids, rows)
    for p_ in (pm, pu, pc):
        p_.batch.set_waves_per_game(1)
    it_m, cv_m, st_m = alg.mpc_solve(pm, steps, record_states=True, schedule=S)
    it_u, cv_u, st_u = alg.mpc_solve(pu, steps, record_states=True)
    it_c, cv_c, st_c = alg.mpc_solve(pc, steps, record_states=True, schedule=frozen)
    assert np.array_equal(st_c, st_u) and np.array_equal(it_c, it_u) and np.array_equal(cv_c, cv_u)
    for a, b in zip(_final_state(pc), _final_state(pu)):
        assert np.array_equal(a, b)
    moved = np.abs(st_m[-1] - st_u[-1]).max(axis=1)
    print("scheduled vs frozen world, final states: min over games %.3e, max %.3e" % (moved.min(), moved.max()))
    assert moved.min() > 1e-3 and np.median(moved) > 0.02, moved
    # strongly differing rows: nothing of row t survives into the solve of step t + 1 (alternating far-apart circles and targets)
    alt = {k: v.copy() for k, v in S.items()}
    alt["circle"][1::2, :, :2] += 0.4
    alt[TARGET][1::2, :, :] += 0.5
    pa, _ = alg.scenarios.c5_scheduled(ids[:16], rows); pb, _ = alg.scenarios.c5_scheduled(ids[:16], rows)
    alt = {k: np.ascontiguousarray(v[:, :16]) for k, v in alt.items()}
    for p_ in (pa, pb):
        p_.batch.set_waves_per_game(1)
    it_a, cv_a, st_a = alg.mpc_solve(pa, 8, record_states=True, schedule=alt, fused=True)
    it_b, cv_b, st_b = alg.mpc_solve(pb, 8, record_states=True, schedule=alt, fused=False)
    same = it_a == it_b
    print("alternating rows, fused vs step-wise: same totals %.3f, max state diff %.3e" % (same.mean(), np.abs(st_a - st_b)[:, same].max()))
    assert same.mean() >= 0.8 and np.abs(st_a - st_b)[:, same].max() < 1e-9


# ---- 3. lock-step against the oracle ------------------------------------------------------------------------------------------------------
def _pairs(p):
    return lambda v: (v[:, None] + v[None, :]).reshape(-1) * (1 - np.eye(p).reshape(-1))


class Family:
    """One configuration with its ingredients (kind, base values (B, .), values of game -> ABI row, adder, per-step change) and the kinds
    that are scheduled.  Row t of a kind = base + t * step (the +-inf pattern of bounds is kept: inf + finite = inf)."""

    GAP = {K_CIRC: (0.02, 0.02), K_CYL: (0.06, 0.02)}          # clearance between the way and the obstacle: from, width

    # seeds fixed after a run of every family with the oracle alone on the CPU: every solve of the 6 steps converges in at most 10 Newton
    # iterations without a failed line search (an obstacle that becomes active costs the augmented-Lagrangian loop 11 ... 50 iterations, so
    # the scheduled obstacles of these families pass close by; the scheduled collision costs and targets are what shapes the solutions here,
    # the active moving circle is the matter of the tests against the step-wise loop above)
    SEEDS = {"di3d_cylinder_target": 2}

    def __init__(self, name, B=8, steps=6, rows=4, seed=None):
        seed = self.SEEDS.get(name, 0) if seed is None else seed
        self.name, self.B, self.steps, self.rows, self.dt, self.mode = name, B, steps, rows, 0.1, "ext"
        rng = np.random.default_rng(seed)
        r = rng.random
        if name == "uni3_circle_target":               # tile path, EXT: unicycles, one circle for every player
            self.model, self.p, self.d, self.N = UNI, 3, 2, 8
            circ = np.concatenate([0.45 + 0.1 * r((B, 2)), 0.12 + 0.03 * r((B, 1))], axis=1)
            cost = np.concatenate([0.2 + 0.2 * r((B, 3)), 1.0 + r((B, 3))], axis=1)
            self.ingr = [(K_COST, cost, lambda v: v, lambda b, v: b.add_collision_cost(v[:3], v[3:]), 0.05 * cost),
                         (K_RAD, 0.04 + 0.02 * r((B, 3)), _pairs(3), lambda b, v: b.add_collision_avoidance(v), None),
                         (K_CIRC, circ, lambda v: v, lambda b, v: b.add_circle_constraint(v[0:1], v[1:2], v[2:3]),
                          np.concatenate([0.01 * (r((B, 2)) - 0.5), np.zeros((B, 1))], axis=1))]
        elif name == "di3d_cylinder_target":           # the 3-D set
            self.model, self.p, self.d, self.N = DI, 2, 3, 8
            cyl = np.concatenate([0.5 + 0.1 * (r((B, 2)) - 0.5), 0.01 * r((B, 1)), 0.8 + 0.2 * r((B, 1)), 0.1 + 0.05 * r((B, 1))], axis=1)     # p (3) l r, axis z
            cost = np.concatenate([0.2 + 0.2 * r((B, 2)), 1.0 + r((B, 2))], axis=1)
            self.ingr = [(K_COST, cost, lambda v: v, lambda b, v: b.add_collision_cost(v[:2], v[2:]), 0.05 * cost),
                         (K_RAD, 0.05 + 0.03 * r((B, 2)), _pairs(2), lambda b, v: b.add_spherical_collision_avoidance(v), None),
                         (K_CYL, cyl, lambda v: v, lambda b, v: b.add_cylinder_constraint(v[None, 0:3], [2], [v[3]], [v[4]]),
                          np.concatenate([0.01 * (r((B, 2)) - 0.5), np.zeros((B, 3))], axis=1))]
        elif name == "di5_cost_target":                # dense direction (n = 20), EXT
            self.model, self.p, self.d, self.N = DI, 5, 2, 6
            cost = np.concatenate([0.2 + 0.2 * r((B, 5)), 1.0 + r((B, 5))], axis=1)
            self.ingr = [(K_COST, cost, lambda v: v, lambda b, v: b.add_collision_cost(v[:5], v[5:]), 0.05 * cost),
                         (K_RAD, 0.04 + 0.02 * r((B, 5)), _pairs(5), lambda b, v: b.add_collision_avoidance(v), None)]
        elif name in ("di3_base_target", "di3_base_mode_target"):     # base kernels (the team of four at this batch size); BASE mode: the block-reading twins
            self.model, self.p, self.d, self.N = DI, 3, 2, 10
            self.mode = "base" if name == "di3_base_mode_target" else "ext"
            one = lambda v: np.tile(v[:1], (B, 1))     # the games share the scenario numbers: nothing but the targets differs
            umax, umin = 0.6 + 0.4 * r((B, 6)), -0.5 - 0.4 * r((B, 6))
            ctl = np.concatenate([umax, umin], axis=1)
            self.ingr = [(K_COST, one(np.concatenate([0.2 + 0.3 * r((B, 3)), 1.0 + 2.0 * r((B, 3))], axis=1)), lambda v: v, lambda b, v: b.add_collision_cost(v[:3], v[3:]), None),
                         (K_RAD, one(0.06 + 0.04 * r((B, 3))), _pairs(3), lambda b, v: b.add_collision_avoidance(v), None),
                         (K_CTL, ctl if self.mode == "base" else one(ctl), lambda v: v, lambda b, v: b.add_control_bound(v[:6], v[6:]), None)]
        else:
            raise ValueError(name)
        p = self.p
        self.ni, self.mi = {DI: (2 * self.d, self.d), UNI: (4, 2), QUAD: (12, 4)}[self.model]
        n = p * self.ni
        self.Q, self.R = 1 + r((B, p, self.ni)), 0.5 + r((B, p, self.mi))
        self.xf, self.uf = r((B, p, self.ni)), 0.2 * (r((B, p, self.mi)) - 0.5)
        self.dxf = 0.04 * (r((B, p, self.ni)) - 0.5)
        x0 = 0.1 * r((B, n))
        x0[:, 0:p] += np.linspace(0.0, 0.8, p)[None]; x0[:, p:2 * p] += np.linspace(0.8, 0.0, p)[None]
        if self.model == UNI:
            # an easy start for the nonlinear model: every vehicle already drives towards its target, which lies a little beside the end of
            # the straight line it would follow with zero controls over the horizon
            th, v = 2 * np.pi * r((B, p)), 0.3 + 0.1 * r((B, p))
            x0[:, 2 * p:3 * p], x0[:, 3 * p:4 * p] = th, v
            T = self.dt * (self.N - 1)
            self.xf[:, :, 0] = x0[:, 0:p] + T * v * np.cos(th) + 0.04 * (r((B, p)) - 0.5)
            self.xf[:, :, 1] = x0[:, p:2 * p] + T * v * np.sin(th) + 0.04 * (r((B, p)) - 0.5)
            self.xf[:, :, 2], self.xf[:, :, 3] = th, v
            self.uf[:] = 0.0
            self.dxf[:, :, 2:] = 0.0
        self.x0 = x0
        # the scheduled obstacle sits beside the middle of player 0's way to its target: active in part of the games
        mid = 0.5 * (np.stack([x0[:, 0], x0[:, p]], axis=1) + self.xf[:, 0, :2])
        for i, (kind, v, pack, add, step) in enumerate(self.ingr):
            if kind in (K_CIRC, K_CYL):
                way = self.xf[:, 0, :2] - np.stack([x0[:, 0], x0[:, p]], axis=1)
                nrm = np.stack([-way[:, 1], way[:, 0]], axis=1) / np.linalg.norm(way, axis=1, keepdims=True)
                v[:, :2] = mid + nrm * (v[:, -1:] + self.GAP[kind][0] + self.GAP[kind][1] * r((B, 1)))

    # values of step t (row min(t, rows - 1))
    def values(self, i, t):
        kind, v, pack, add, step = self.ingr[i]
        return v if step is None else v + min(t, self.rows - 1) * step

    def target(self, t):
        return self.xf + min(t, self.rows - 1) * self.dxf

    def schedule(self):
        S = {}
        for i, (kind, v, pack, add, step) in enumerate(self.ingr):
            if step is not None:
                S[kind] = np.stack([np.stack([pack(x) for x in self.values(i, t)]) for t in range(self.rows)])
        S[TARGET] = np.stack([np.concatenate([self.target(t).reshape(self.B, -1), self.uf.reshape(self.B, -1)], axis=1) for t in range(self.rows)])
        return S

    def setup(self, b, game, t):
        """x0, LQR and adders with the values of step t: of game `game`, or (None) game 0's on the whole batch"""
        sl = slice(None) if game is None else slice(game, game + 1)
        b.set_x0(self.x0[sl]); b.set_lqr(self.Q[sl], self.R[sl], self.target(t)[sl], self.uf[sl])
        for i, (kind, v, pack, add, step) in enumerate(self.ingr):
            add(b, self.values(i, t)[0 if game is None else game])

    def device(self, alg):
        g = alg.Batch(alg.hip_lib(), self.model, self.p, self.N, self.dt, self.B, d=self.d)
        if self.mode == "base":
            g.set_scenario_kernels("base")
        self.setup(g, None, 0)
        if self.mode == "base":                        # per-game control bounds keep the handle on the block-reading twins
            g.set_scenario_data(K_CTL, np.stack([self.ingr[2][2](x) for x in self.ingr[2][1]]))
        else:
            for i, (kind, v, pack, add, step) in enumerate(self.ingr):
                if step is None and not np.array_equal(v, np.tile(v[:1], (self.B, 1))):       # what differs per game but is not scheduled
                    g.set_scenario_data(kind, np.stack([pack(x) for x in v]))
        for kind, a in self.schedule().items():
            g.mpc_set_schedule(kind, a)
        return g

    def oracle(self, orc, game, t):
        o = orc.OracleBatch(self.model, self.p, self.N, self.dt, 1, d=self.d)
        self.setup(o, game, t)
        return o


FAMILIES = ["uni3_circle_target", "di3d_cylinder_target", "di5_cost_target", "di3_base_target", "di3_base_mode_target"]


def lockstep(fam, orc, run_to):
    """run_to(t) -> (traj, lam, mu, stats) of every game after t steps of the loop under test.  Step t of game g: the one-game oracle batch
    with row t's values takes that state, runs the one newton_solve! + advance, and must meet run_to(t + 1).  Returns the worst distances."""
    worst, iters = 0.0, []
    state = run_to(0)
    for t in range(fam.steps):
        z, lam, mu, _ = state
        state = run_to(t + 1)
        zn, _, _, st = state
        for game in range(fam.B):
            o = fam.oracle(orc, game, t)
            assert o.con_len == lam.shape[1]
            if t > 0:
                o.set_options(shift=1, dual_reset=0)
            o.set_x0(z[game:game + 1, :o.n].copy()); o.set_traj(z[game:game + 1]); o.set_con_duals(lam[game:game + 1], mu[game:game + 1])
            so = o.newton_solve(init=True, game_id0=GID0 + t * 1000003 + game)
            # the inputs are chosen so that the strict bound applies to every solve: nothing is left out
            assert so["converged"][0] == 1 and so["newton_iters"][0] <= 10 and so["ls_failures"][0] == 0 and so["status"][0] == 0, (fam.name, t, game, so)
            iters.append(int(so["newton_iters"][0]))
            if st is not None:
                for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
                    assert st[f][game] == so[f][0], (fam.name, f, t, game, st[f][game], so[f][0])
            o.mpc_advance()
            zo = o.get_traj()[0]
            err = np.abs(zn[game] - zo).max()
            worst = max(worst, err)
            assert err <= 1e-8 * max(1.0, np.abs(zo).max()), (fam.name, t, game, err)
    return worst, iters


@pytest.mark.parametrize("name", FAMILIES)
def test_scheduled_loop_lock_step_against_the_oracle(alg, orc, name):
    """8 games x 6 steps per family, 4 rows (held from step 3 on).  The state before step t is what the fused loop of t steps leaves (a
    fresh handle per length: the loop is deterministic), so every compared solve ran inside a multi-step launch.  Bounds of
    tests/test_gpu_scenario_data.py: identical counts, trajectory within 1e-8."""
    fam = Family(name)
    kept = {}

    def run_to(t):
        g = fam.device(alg)
        kept[t] = g
        st = None
        if t > 0:
            g.mpc_solve(t, game_id0=GID0)
            st = g.get_stats()
            assert g.lib.debug_check_guards(g.h) == 0
        lam, mu = g.get_con_duals()
        return g.get_traj(), lam, mu, st
    worst, iters = lockstep(fam, orc, run_to)
    print("%s: %d solves, Newton iterations %d ... %d, worst |z - z_oracle| %.3e" % (name, len(iters), min(iters), max(iters), worst))
    g = kept[fam.steps]
    in_use = 0 if name == "di3_base_target" else {"ext": 1, "base": 2}[fam.mode]     # base kernels / EXT kernels / block-reading twins
    assert g.get_scenario_kernels()[1] == in_use
    if name.startswith("di3_base"):
        assert g.get_waves_per_game() == 4              # the team kernels carry the phase too
    for kind, a in fam.schedule().items():
        if kind != TARGET:
            assert np.array_equal(g.get_scenario_data(kind), a[-1])
        assert g.mpc_get_schedule(kind) == fam.rows


# ---- 4. the error paths -------------------------------------------------------------------------------------------------------------------
def _handle(alg, B=4, mode="ext"):
    g = alg.Batch(alg.hip_lib(), DI, 3, 8, 0.1, B)
    if mode == "base":
        g.set_scenario_kernels("base")
    rng = np.random.default_rng(5)
    x0 = 0.1 * rng.random((B, g.n)); x0[:, 0:3] += np.linspace(0.0, 0.8, 3)[None]; x0[:, 3:6] += np.linspace(0.8, 0.0, 3)[None]
    g.set_x0(x0)
    g.add_collision_avoidance(np.full(3, 0.05))
    umax = np.full(6, 1.0); umax[0] = np.inf
    g.add_control_bound(umax, -np.ones(6))
    return g, x0, rng


def _lqr(g, rng, per_game=True):
    lead = (g.B,) if per_game else ()
    g.set_lqr(1 + rng.random(lead + (3, 4)), 0.5 + rng.random(lead + (3, 2)), rng.random(lead + (3, 4)), np.zeros(lead + (3, 2)))


def _solve(g, x0):
    g.set_x0(x0)
    g.newton_solve(init=True, game_id0=GID0)
    return g.get_traj()


def test_errors_leave_the_handle_as_it_was(alg):
    E = alg.AlgamesError
    g, x0, rng = _handle(alg)
    _lqr(g, rng, per_game=False)
    B, m = g.B, g.m
    before = _solve(g, x0)
    ctl = np.tile(g.get_scenario_data(K_CTL)[None], (5, 1, 1))
    # a target schedule before per-game LQR data
    with pytest.raises(E, match="code -3"):
        g.mpc_set_schedule(TARGET, np.zeros((2, B, 18)))
    # a wrong +-inf pattern in row 3 of 5
    bad = ctl.copy(); bad[3, 1, 0] = 1.0
    with pytest.raises(E, match="code -1") as e:
        g.mpc_set_schedule(K_CTL, bad)
    assert "row 3" in str(e.value) and "+-inf pattern" in str(e.value)
    # a radius <= 0
    rad = np.tile(g.get_scenario_data(K_RAD)[None], (3, 1, 1)); rad[2, 0, 1] = 0.0
    with pytest.raises(E, match="code -1"):
        g.mpc_set_schedule(K_RAD, rad)
    # a kind that was never added
    with pytest.raises(E, match="code -3"):
        g.mpc_set_schedule(K_CIRC, np.zeros((2, B, 0)))
    # rows < 1 with data, an unknown kind (straight at the C ABI)
    a = np.zeros((1, B, 2 * m))
    assert g.lib.mpc_set_schedule(g.h, K_CTL, 0, a.ctypes.data_as(alg._abi._D)) == alg._abi.ALG_ERR_ARG
    assert g.lib.mpc_set_schedule(g.h, 55, 1, a.ctypes.data_as(alg._abi._D)) == alg._abi.ALG_ERR_ARG
    with pytest.raises(ValueError):
        g.mpc_set_schedule(K_CTL, np.zeros((2, B + 1, 2 * m)))
    with pytest.raises(ValueError):
        g.mpc_set_schedule("no_such_kind", np.zeros((2, B, 3)))
    # nothing changed: still the base kernels, no schedule, the same solve
    assert g.get_scenario_kernels()[1] == 0
    assert all(g.mpc_get_schedule(k) == 0 for k in list(range(8)) + [TARGET])
    assert np.array_equal(_solve(g, x0), before)
    # non-finite targets
    _lqr(g, rng)
    before = _solve(g, x0)
    t = np.zeros((2, B, 18)); t[1, 2, 5] = np.nan
    with pytest.raises(E, match="code -1"):
        g.mpc_set_schedule(TARGET, t)
    assert g.mpc_get_schedule(TARGET) == 0 and np.array_equal(_solve(g, x0), before)


def test_a_base_kind_cannot_be_scheduled_in_base_mode(alg):
    g, x0, rng = _handle(alg, mode="base")
    _lqr(g, rng)
    before = _solve(g, x0)
    ctl = np.tile(g.get_scenario_data(K_CTL)[None], (2, 1, 1))
    with pytest.raises(alg.AlgamesError, match="code -1") as e:
        g.mpc_set_schedule(K_CTL, ctl)
    assert "default mode" in str(e.value)
    assert g.get_scenario_kernels() == (1, 0) and g.mpc_get_schedule(K_CTL) == 0
    assert np.array_equal(_solve(g, x0), before)
    g.mpc_set_schedule(TARGET, np.zeros((2, g.B, 18)))           # the targets work in both modes
    assert g.mpc_get_schedule(TARGET) == 2


def test_what_drops_a_schedule(alg):
    g, x0, rng = _handle(alg)
    _lqr(g, rng)
    ctl = np.tile(g.get_scenario_data(K_CTL)[None], (3, 1, 1)); ctl[1:, :, 1] = 0.7
    rad = np.tile(g.get_scenario_data(K_RAD)[None], (2, 1, 1))
    tgt = np.zeros((2, g.B, 18))

    def set_all():
        g.mpc_set_schedule(K_CTL, ctl); g.mpc_set_schedule(K_RAD, rad); g.mpc_set_schedule(TARGET, tgt)
        assert (g.mpc_get_schedule(K_CTL), g.mpc_get_schedule(K_RAD), g.mpc_get_schedule(TARGET)) == (3, 2, 2)
    set_all()
    assert g.get_scenario_kernels()[1] == 1                       # the kind became per game as set_scenario_data(row 0) makes it
    g.set_scenario_data(K_CTL, ctl[0])                            # ... drops that kind's schedule only
    assert (g.mpc_get_schedule(K_CTL), g.mpc_get_schedule(K_RAD), g.mpc_get_schedule(TARGET)) == (0, 2, 2)
    _lqr(g, rng)                                                  # alg_set_lqr: the target schedule
    assert (g.mpc_get_schedule(K_RAD), g.mpc_get_schedule(TARGET)) == (2, 0)
    set_all()
    g.mpc_set_schedule(K_RAD, None)                               # data = NULL
    assert (g.mpc_get_schedule(K_CTL), g.mpc_get_schedule(K_RAD), g.mpc_get_schedule(TARGET)) == (3, 0, 2)
    g.add_collision_avoidance(np.full(3, 0.06))                   # an adder: all of them, with the per-game data
    assert all(g.mpc_get_schedule(k) == 0 for k in (K_CTL, K_RAD, TARGET))
    # and the loop after the drop is the unscheduled loop of a handle that never had a schedule (same calls otherwise)
    h, _, _ = _handle(alg)
    h.set_scenario_data(K_CTL, ctl[0])
    h.add_collision_avoidance(np.full(3, 0.06))
    lq = np.random.default_rng(6)
    Q, R, xf, uf = 1 + lq.random((g.B, 3, 4)), 0.5 + lq.random((g.B, 3, 2)), lq.random((g.B, 3, 4)), np.zeros((g.B, 3, 2))
    for b in (g, h):
        b.set_x0(x0); b.set_lqr(Q, R, xf, uf)
    sg, sh = g.mpc_solve(4, game_id0=GID0, record_states=True), h.mpc_solve(4, game_id0=GID0, record_states=True)
    assert g.get_scenario_kernels()[1] == h.get_scenario_kernels()[1] == 1
    assert np.array_equal(sg, sh) and np.array_equal(g.get_traj(), h.get_traj())
    assert g.lib.debug_check_guards(g.h) == 0
