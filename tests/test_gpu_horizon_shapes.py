"""Every solver kernel shape over short and chunk-edge horizons.

The fused solver's loops are written around compile-time depths with a clamped or broken-off tail: the fused trial pass and the group line
search walk the horizon in chunks of FT steps (FT below), the forward and costate sweeps keep a prefetch ring of SWEEP_DEPTH = 6 (512-register
kernels) or 4 (256-register kernels: unicycle, bicycle, n >= 16, every team kernel) steps, the FWDW costate sweep one of 8, the streaming copies
move 8 / 4 / 2 elements per lane and trip, and the shift warm start ends x, u and lambda at three different steps.  A horizon N - 1 equal to such
a depth, one less or one more is where these loops can go wrong, so every shape is run at

    N = 2 ... 18                                      (depths 4, 6, 8 and FT = 8 with their neighbours, twice over)
    N - 1 in {FT - 1, FT, FT + 1, 2 FT, 2 FT + 1}     (the shape's own FT: adds N = 27, 28 for FT = 13 and N = 30, 31, 32 for FT = 15)

on a problem family that is not trivial at short horizons (`family`): the players cross a small circle with collision cost, collision
avoidance and control bounds all in play, so that from N = 3 on every horizon has games with several outer iterations and multipliers
>= 0.07, backtracking and failed line searches appear from N ~ 5, and the longer horizons contain non-converging 7-outer solves with the
penalties at their ceiling.  tests/test_horizon_family.py holds these preconditions on the CPU (oracle against the long-double arbiter).

The oracle's and the arbiter's solves are cached per (model, p, d, N, wall) and shared by the shapes that solve the same problem."""
import numpy as np
import pytest

import test_gpu_fuzz as FZ
from test_gpu_parity import _pair

pytestmark = pytest.mark.gpu

DI, UNI, BIC, QUAD = 0, 1, 2, 3
GID0 = 7                                           # the game id test_gpu_fuzz._compare_solve solves with
ALG_STATUS_PARKED = 3
EXT, BASE = 0, 1                                   # ALG_SCEN_KERNELS_*
K_RAD, K_COST, K_CTL = 0, 1, 2                     # ALG_SCEN_COLLISION_RADIUS / _COLLISION_COST / _CONTROL_BOUND
OPTS = dict(outer_iter=7, inner_iter=20, reg_0=1e-5, beta=0.2)
DT = 0.1


def FT(model, p, d=2):
    """Steps per chunk of the fused trial pass, keyed as AsmLds<C>::FT (algames_device.hpp:955; FT_DI3 / FT_UNI3 / FT_UNI4 at :39-41)."""
    if model == DI and p == 3 and d == 2:
        return 13
    if model == UNI and p == 3:
        return 15
    if model == UNI and p == 4:
        return 13
    return 8


def horizons(model, p, d=2):
    ft = FT(model, p, d)
    edge = {ft + k + 1 for k in (-1, 0, 1)} | {2 * ft + 1, 2 * ft + 2}
    if ft == 15:
        edge.add(30)                               # the workload horizon of the 3-player unicycle: the last step of its second chunk
    return sorted(set(range(2, 19)) | edge)


def family(make, model, p, d, N, B=4, seed=0, turn=0.5, wall=False, spherical=False):
    """The short-horizon family on the Batch / OracleBatch API: make(model, p, N, dt, B, d) -> batch.  Players start on a circle of radius
    0.4 +- 0.05 at angles 2 pi i / p +- 0.3 and go to the point at radius 0.6 on the far side, rotated by 0.4 rad (d = 3: heights
    +- 0.1 on top; d = 1: the x coordinates of these points for two players, who meet head-on and stop against each other; more players on a
    line that do the same diverge in the oracle itself -- |oracle - arbiter| up to 1e4 -- so they keep their order, 0.5 apart, and go to targets
    0.15 apart, closer than the pair radius 0.26); unicycles and bicycles head for the target +- `turn` rad at speed 0.5.  Q = 10, R = 0.1,
    uf = 0, collision cost of radius 1.0 and mu 2.0, collision avoidance 0.13 per player, control bounds +- 0.8.  wall: one far-away wall
    (never active) that switches the handle to the extended-constraint kernels.  spherical (d = 3): the collision avoidance measures the
    distance in x, y, z (add_spherical_collision_avoidance) instead of x, y."""
    rng = np.random.default_rng([seed, model, p, d, N])
    b = make(model, p, N, DT, B, d)
    ni, mi = b.n // p, b.mi
    ang = 2 * np.pi * np.arange(p) / p + rng.uniform(-0.3, 0.3, (B, p))
    rad = 0.4 + rng.uniform(-0.05, 0.05, (B, p))
    tx, ty = 0.6 * np.cos(ang + np.pi + 0.4), 0.6 * np.sin(ang + np.pi + 0.4)
    x0 = np.zeros((B, b.n)); xf = np.zeros((B, p, ni))
    x0[:, 0:p] = rad * np.cos(ang); xf[:, :, 0] = tx
    hz = rng.uniform(-0.1, 0.1, (B, 2, p))
    turn = rng.uniform(-turn, turn, (B, p))
    if model == DI:
        if d == 1 and p > 2:                       # on a line nobody can pass: the order is kept, the targets lie closer than the pair radius 0.26
            mid = np.arange(p) - 0.5 * (p - 1)
            x0[:, 0:p] = 0.5 * mid + (rad - 0.4); xf[:, :, 0] = 0.15 * mid + 0.3 + 0.1 * np.sin(ang)
        if d >= 2:
            x0[:, p:2 * p] = rad * np.sin(ang); xf[:, :, 1] = ty
        if d == 3:
            x0[:, 2 * p:3 * p] = hz[:, 0]; xf[:, :, 2] = hz[:, 1]
    else:                                          # unicycle / bicycle: x, y, heading, speed
        x0[:, p:2 * p] = rad * np.sin(ang); xf[:, :, 1] = ty
        head = np.arctan2(ty - x0[:, p:2 * p], tx - x0[:, 0:p])
        x0[:, 2 * p:3 * p] = head + turn; xf[:, :, 2] = head
        x0[:, 3 * p:4 * p] = 0.5
    if model == BIC:
        b.set_bicycle(0.07, 0.04)
    b.set_x0(x0)
    b.set_lqr(np.full((B, p, ni), 10.0), np.full((B, p, mi), 0.1), xf, np.zeros((B, p, mi)))
    b.set_options(**OPTS)
    if p > 1:
        b.add_collision_cost(np.full(p, 1.0), np.full(p, 2.0))
        (b.add_spherical_collision_avoidance if spherical else b.add_collision_avoidance)(np.full(p, 0.13))
    b.add_control_bound(np.full(b.m, 0.8), np.full(b.m, -0.8))
    if wall:
        b.add_wall_constraint([5.0], [5.0], [6.0], [5.0], [0.0], [1.0])
    return b


class Solved:
    """A reference batch of the family, solved at most once: newton_solve returns the statistics of that one solve, everything else is the
    batch's own (its buffers hold the solve's results and nobody writes them)."""

    def __init__(self, batch):
        self._b, self._st = batch, None

    def newton_solve(self, init=True, game_id0=GID0):
        assert init and game_id0 == GID0
        if self._st is None:
            self._st = self._b.newton_solve(init=True, game_id0=GID0)
        return self._st.copy()

    def __getattr__(self, k):
        if k.startswith(("set_", "add_", "init_", "update_", "mpc_", "reset_", "rollout", "newton_", "ibr_", "dual_")):
            raise AttributeError("a cached reference solve is read-only: " + k)
        return getattr(self._b, k)


# What the CPU preconditions (tests/test_horizon_family.py) made of the starting point: the seed of three configurations whose seed-0 games
# never fail a line search at any horizon, and a single unicycle (control bounds only) that starts up to 2.5 rad off its course.
TUNED = {(DI, 4, 2): dict(seed=1), (DI, 2, 3): dict(seed=2), (UNI, 1, 2): dict(turn=2.5)}
_REF = {}


def _oracle_family(orc, cfg, N, wall, kind, build):
    """family(*cfg, N) -- or another family, build(make, model, p, d, N) -- on the oracle (kind "") or the long-double arbiter ("x")"""
    make = lambda *a: orc.OracleBatch(*a[:5], d=a[5], kind=kind)
    return build(make, *cfg, N) if build else family(make, *cfg, N, wall=wall, **TUNED.get(tuple(cfg), {}))


def reference(orc, model, p, d, N, wall=False, kind="", build=None, key=None):
    """The oracle (kind "") or the long-double arbiter ("x") of family(model, p, d, N), B = 4, seed 0: built once per session, solved on first use.
    build / key: another problem family, build(make, model, p, d, N) -> batch, cached under its own key."""
    assert (build is None) == (key is None)
    k = (key, model, p, d, N, wall, kind)
    if k not in _REF:
        _REF[k] = Solved(_oracle_family(orc, (model, p, d), N, wall, kind, build))
    return _REF[k]


def hip_family(alg, model, p, d, N, **kw):
    return family(lambda *a: alg.Batch(alg.hip_lib(), *a[:5], d=a[5]), model, p, d, N, **{**TUNED.get((model, p, d), {}), **kw})


# ---- the configurations -------------------------------------------------------------------------------------------------------------------------
DI3, UNI3, UNI4 = (DI, 3, 2), (UNI, 3, 2), (UNI, 4, 2)
BASE_CONFIGS = [(DI, 1, 2), (DI, 2, 2), DI3, (DI, 4, 2), (UNI, 1, 2), (UNI, 2, 2), UNI3, UNI4, (DI, 2, 3), (DI, 2, 1), (DI, 4, 1)]
DENSE_CONFIGS = [(DI, 5, 2), (UNI, 5, 2), (DI, 3, 3), (QUAD, 2, 2)]            # (b): one of each dense kind, N = 2 ... 10
TEAM_CONFIGS = [(DI3, 4), (UNI3, 4), (UNI4, 2), (UNI4, 4)]
EXT_CONFIGS = [(DI3, True), (UNI3, True), (UNI4, True), ((BIC, 2, 2), False)]    # (configuration, far-away wall)
TWIN_CONFIGS = [(DI3, 1), (UNI3, 1), (UNI4, 1)] + TEAM_CONFIGS
HANDOFF_CONFIGS = [DI3, UNI3, UNI4]
MPC_CONFIGS = [(DI3, 1), (DI3, 0), (UNI3, 1), (UNI3, 0), (UNI4, 1), (UNI4, 0)]  # waves per game: 1, or 0 = the team the library picks for four games
MPC_HORIZONS, MPC_STEPS = (2, 3, 4, 5, 6, 9), 5
SHIFT_CONFIGS = [DI3, UNI4, (DI, 5, 2)]
WORST = {}                                                                     # shape -> worst |hip - oracle| over its horizons (printed by each test)


def handoff_horizons(cfg):
    ft = FT(*cfg)
    return [2, 3, 5, 7, ft, ft + 2]


def family_problems():
    """Every (configuration, wall, horizons) of the family the GPU tests below solve: what tests/test_horizon_family.py holds the preconditions for."""
    return [(cfg, False, horizons(*cfg)) for cfg in BASE_CONFIGS] + [(cfg, wall, horizons(*cfg)) for cfg, wall in EXT_CONFIGS]


def _name(v):
    if isinstance(v, tuple) and len(v) == 3 and not isinstance(v[0], tuple):
        return "%s%d%s" % (("di", "uni", "bic", "quad")[v[0]], v[1], "" if v[2] == 2 else "_d%d" % v[2])
    return None


def _note(shape, err):
    WORST[shape] = max(WORST.get(shape, 0.0), float(err))


def _compare(g, orc, cfg, N, wall=False, tag=(), build=None, key=None):
    """g.newton_solve against the cached oracle of the same problem: test_gpu_fuzz._compare_solve with the arbiter (discrete history
    identical, 1e-8, else the arbiter rule; no game left out), then mu bit-equal and lambda <= 1e-6 relative on the games the oracle
    converged (test_gpu_parity._assert_solve_parity).  Returns the worst |hip - oracle| over the games of status OK.  build / key: the
    problem family g was built from, where it is not `family` (see reference)."""
    o, x = reference(orc, *cfg, N, wall=wall, build=build, key=key), reference(orc, *cfg, N, wall=wall, kind="x", build=build, key=key)
    FZ._compare_solve(g, o, (cfg[0], cfg[1], N, DT) + tuple(tag), x=x)
    so = o.newton_solve()
    conv = so["converged"] == 1
    (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
    assert lg.shape == lo.shape
    if conv.any():
        assert np.array_equal(mg[conv], mo[conv]), (cfg, N, tag)
        assert np.abs(lg[conv] - lo[conv]).max() <= 1e-6 * max(1.0, np.abs(lo[conv]).max()), (cfg, N, tag, np.abs(lg[conv] - lo[conv]).max())
    ok = so["status"] == 0
    return np.abs(g.get_traj(0) - o.get_traj(0))[ok].max(initial=0.0)


def _guards_ok(g):
    assert g.lib.debug_check_guards(g.h) == 0


def _bits(b):
    """everything a solve leaves behind, for bit-wise comparison: trajectory, multipliers, penalties, statistics (but the wall time), history of every game"""
    st = b.get_stats()
    lam, mu = b.get_con_duals()
    out = [b.get_traj(), lam, mu] + [st[f] for f in st.dtype.names if f != "last"] + [st["last"][f] for f in st["last"].dtype.names if f != "t_elap"]
    for game in range(b.B):
        h = b.get_history(game)
        out += [h[f] for f in h.dtype.names if f != "t_elap"]
    return out


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(_bits(a), _bits(b))):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, i)


# ---- a. one wavefront per game --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", BASE_CONFIGS, ids=_name)
def test_one_wavefront_solve_over_horizons(alg, orc, cfg):
    """Whole solves of the one-wavefront base kernels (fused trial pass, group line search, both sweeps, settle copies, dual and penalty update)
    at every horizon of the rule above."""
    for N in horizons(*cfg):
        g = hip_family(alg, *cfg, N)
        g.set_waves_per_game(1)
        assert g.get_waves_per_game() == 1 and g.get_scenario_kernels() == (EXT, 0)
        _note(("w1",) + cfg, _compare(g, orc, cfg, N))
        _guards_ok(g)
    print("one wavefront", cfg, "worst |hip - orc| %.2e" % WORST[("w1",) + cfg])


# ---- b. the Newton direction, step-wise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", BASE_CONFIGS + DENSE_CONFIGS, ids=_name)
def test_newton_direction_over_horizons(alg, orc, cfg):
    """alg_newton_direction on random full-magnitude data (test_gpu_parity._pair: every constraint row with a multiplier and a penalty of
    O(1)) -- the ring tails of the sweeps with numbers that are not those of a nearly converged iterate.  Bounds of
    test_newton_direction_parity: 1e-9 relative to the oracle, J d = -res to 1e-8."""
    import test_gpu_parity_quad as PQ
    model, p, d = cfg
    worst = 0.0
    for N in range(2, 19 if cfg in BASE_CONFIGS else 11):
        g, o = PQ._pair(alg, orc, p, N, B=4, seed=N) if model == QUAD else _pair(alg, orc, model, p, d, N, B=4, seed=N)
        for reg in (1e-3, 1e-7 * 2 ** 4):
            dg, sg = g.newton_direction(reg); do, so = o.newton_direction(reg)
            assert np.all(sg == 0) and np.all(so == 0), (cfg, N)
            err = (np.abs(dg - do) / np.abs(do).max(axis=1, keepdims=True)).max()
            worst = max(worst, err)
            assert err < 1e-9, (cfg, N, reg, err)
            J = o.residual_jacobian(reg); res = o.residual()[0]
            lin = np.einsum("brc,bc->br", J, dg) + res
            assert np.abs(lin).max() <= 1e-8 * max(1.0, np.abs(res).max()), (cfg, N, reg, np.abs(lin).max())
            zd = g.get_traj(2)
            assert np.all(zd[:, :g.n] == 0) and np.array_equal(zd[:, g.n:], dg), (cfg, N)
        _guards_ok(g)
    print("direction", cfg, "worst relative difference %.2e" % worst)


# ---- c. teams ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,nw", TEAM_CONFIGS, ids=lambda v: _name(v) or "w%d" % v)
def test_team_solve_over_horizons(alg, orc, cfg, nw):
    """The team kernels (their sweeps run on wavefront 0 behind dir_sync with a ring of four and have no step-wise entry point): against the
    oracle as in (a), against the one-wavefront solve of the same handle with the bounds of test_team_kernels_against_the_oracle, nothing left
    in alg_game_stats.reserved, and the same bits from a second solve."""
    for N in horizons(*cfg):
        g = hip_family(alg, *cfg, N)
        g.set_waves_per_game(nw)
        assert g.get_waves_per_game() == nw
        _note(("team", nw) + cfg, _compare(g, orc, cfg, N, tag=("w%d" % nw,)))
        assert np.all(g.get_stats()["reserved"] == 0), (cfg, nw, N)
        first = _bits(g)
        z_team = first[0]
        g.newton_solve(init=True, game_id0=GID0)
        for i, (x, y) in enumerate(zip(first, _bits(g))):
            assert np.array_equal(x, y, equal_nan=True), (cfg, nw, N, "second solve", i)
        g.set_waves_per_game(1)
        s1 = g.newton_solve(init=True, game_id0=GID0)
        so = reference(orc, *cfg, N).newton_solve()
        for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
            assert np.array_equal(s1[f], so[f]), (cfg, nw, N, f, s1[f], so[f])
        assert np.abs(g.get_traj() - z_team).max() <= 1e-8, (cfg, nw, N, np.abs(g.get_traj() - z_team).max(axis=1))
        _guards_ok(g)
    print("team of", nw, cfg, "worst |hip - orc| %.2e" % WORST[("team", nw) + cfg])


# ---- d. extended-constraint instantiations, and the base kernels' block-reading twins -------------------------------------------------------------------
@pytest.mark.parametrize("cfg,wall", EXT_CONFIGS, ids=lambda v: _name(v) or ("wall" if v else "plain"))
def test_ext_solve_over_horizons(alg, orc, cfg, wall):
    """The EXT instantiations of the same loops: the tile-path shapes switched by one wall at (5, 5) - (6, 5) that no player comes near, and
    the two-player bicycle (EXT by its model)."""
    for N in horizons(*cfg):
        g = hip_family(alg, *cfg, N, wall=wall)
        assert g.get_scenario_kernels()[1] == 1
        _note(("ext",) + cfg, _compare(g, orc, cfg, N, wall=wall, tag=("ext",)))
        _guards_ok(g)
    print("EXT", cfg, "worst |hip - orc| %.2e" % WORST[("ext",) + cfg])


@pytest.mark.parametrize("cfg,nw", TWIN_CONFIGS, ids=lambda v: _name(v) or "w%d" % v)
def test_block_reading_twins_give_the_base_kernels_bits(alg, cfg, nw):
    """alg_set_scenario_kernels(BASE) with every game's block a copy of the shared values: trajectory, lambda, mu, statistics and histories
    bit-equal to the base kernel's at every horizon, on one wavefront and on a team."""
    for N in horizons(*cfg):
        a, b = hip_family(alg, *cfg, N), hip_family(alg, *cfg, N)
        b.set_scenario_kernels(BASE)
        kinds = [k for k in (K_RAD, K_COST, K_CTL) if b.scenario_data_len(k)]
        assert kinds == [K_RAD, K_COST, K_CTL]
        for k in kinds:
            b.set_scenario_data(k, b.get_scenario_data(k))
        assert a.get_scenario_kernels() == (EXT, 0) and b.get_scenario_kernels() == (BASE, 2)
        for h in (a, b):
            h.set_waves_per_game(nw)
            assert h.get_waves_per_game() == nw
            h.newton_solve(init=True, game_id0=GID0)
        _same_bits(a, b, (cfg, nw, N))
        _guards_ok(b)


# ---- e. hand-off ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [1, 3])
@pytest.mark.parametrize("cfg", HANDOFF_CONFIGS, ids=_name)
def test_handoff_over_horizons(alg, orc, cfg, budget):
    """Park on the one-wavefront kernel after `budget` inner iterations, resume on the team kernel: no PARKED status left, exactly the games
    whose plain solve made more than budget + 1 records reported as parked, the others bit-equal to the plain solve, the parked ones on the
    oracle's discrete path with z <= 1e-8 on the converged games and mu bit-equal."""
    n_parked = n_early = 0
    for N in handoff_horizons(cfg):
        plain, ho = hip_family(alg, *cfg, N), hip_family(alg, *cfg, N)
        for h in (plain, ho):
            h.set_waves_per_game(1)
        ho.set_handoff(budget)
        s0, s1 = plain.newton_solve(init=True, game_id0=GID0), ho.newton_solve(init=True, game_id0=GID0)
        k, parked = ho.get_handoff()
        over = (s0["records"] - 1) > budget
        assert k == budget and parked == int(over.sum()), (cfg, N, parked, s0["records"])
        assert not (s1["status"] == ALG_STATUS_PARKED).any(), (cfg, N, s1["status"])
        early = ~over
        z0, z1 = plain.get_traj(), ho.get_traj()
        (l0, m0), (l1, m1) = plain.get_con_duals(), ho.get_con_duals()
        for x, y in ((z0, z1), (l0, l1), (m0, m1)):
            assert np.array_equal(x[early].view(np.uint64), y[early].view(np.uint64)), (cfg, N, "a game that never parked")
        for f in ("newton_iters", "outer_iters", "converged", "status", "records", "ls_failures"):
            assert np.array_equal(s0[f][early], s1[f][early]), (cfg, N, f)
        o = reference(orc, *cfg, N)
        so, zo, mo = o.newton_solve(), o.get_traj(0), o.get_con_duals()[1]
        for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
            assert np.array_equal(s1[f][over], so[f][over]), (cfg, N, f, s1[f], so[f])
        conv = over & (so["converged"] == 1)
        if conv.any():
            err = np.abs(z1[conv] - zo[conv]).max()
            _note(("handoff", budget) + cfg, err)
            assert err <= 1e-8, (cfg, N, err)
            assert np.array_equal(m1[conv], mo[conv]), (cfg, N)
        n_parked += int(over.sum()); n_early += int(early.sum())
        _guards_ok(ho)
    assert n_parked > 0, (n_parked, n_early)                               # (with these budgets every unicycle game parks: the bits of the never-parked games are the double integrator's to hold)
    print("hand-off", cfg, "budget", budget, "parked", n_parked, "never parked", n_early, "worst |hip - orc| on parked, converged games %.2e" % WORST.get(("handoff", budget) + cfg, 0.0))


# ---- f. the fused receding-horizon loop -----------------------------------------------------------------------------------------------------------------
_MPC_REF = {}


def mpc_loop(b, steps=MPC_STEPS, fused=True):
    """(Newton iterations, converged solves, states (steps + 1, B, n)) of the receding-horizon loop of a fresh family batch: the one launch of
    alg_mpc_solve, or the step-wise launches it is held to (host.mpc_solve: shift 1 and no dual reset from the second step on)."""
    b.mpc_totals(reset=True)
    if fused:
        states = b.mpc_solve(steps, GID0, record_states=True)
    else:
        states = [b.get_x0()]
        for t in range(steps):
            if t == 1:
                b.set_options(shift=1, dual_reset=0)
            b.newton_solve_async(init=True, game_id0=GID0 + t * 1000003)
            b.mpc_advance()
            states.append(b.get_x0())
        states = np.stack(states)
    it, cv = b.mpc_totals()
    return it, cv, states


def mpc_reference(orc, cfg, N, kind="", build=None, key=None):
    assert (build is None) == (key is None)
    k = (key, cfg, N, kind)
    if k not in _MPC_REF:
        _MPC_REF[k] = mpc_loop(_oracle_family(orc, cfg, N, False, kind, build))
    return _MPC_REF[k]


@pytest.mark.parametrize("cfg,nw", MPC_CONFIGS, ids=lambda v: _name(v) or ("w1" if v else "team"))
def test_fused_mpc_loop_over_horizons(alg, orc, cfg, nw):
    """Five steps of the fused loop at N = 2 ... 6 and 9 (shifted warm starts with s = 1 at horizons of one to eight steps): against the
    step-wise launches -- totals equal, states <= 1e-9, on one wavefront bit-equal -- and against the oracle's loop -- totals equal, states <=
    1e-7 (test_mpc_receding_horizon_parity)."""
    for N in MPC_HORIZONS:
        f, s = hip_family(alg, *cfg, N), hip_family(alg, *cfg, N)
        for h in (f, s):
            h.set_waves_per_game(nw)
        assert f.get_waves_per_game() == s.get_waves_per_game() and (f.get_waves_per_game() == 1) == (nw == 1)
        it_f, cv_f, st_f = mpc_loop(f)
        it_s, cv_s, st_s = mpc_loop(s, fused=False)
        assert np.array_equal(it_f, it_s) and np.array_equal(cv_f, cv_s), (cfg, nw, N, it_f, it_s, cv_f, cv_s)
        assert np.abs(st_f - st_s).max() <= 1e-9, (cfg, nw, N, np.abs(st_f - st_s).max())
        if nw == 1:
            assert np.array_equal(st_f, st_s), (cfg, N, np.abs(st_f - st_s).max())
        it_o, cv_o, st_o = mpc_reference(orc, cfg, N)
        assert np.array_equal(it_f, it_o) and np.array_equal(cv_f, cv_o), (cfg, nw, N, it_f, it_o, cv_f, cv_o)
        err = np.abs(st_f - st_o).max()
        _note(("mpc", nw) + cfg, err)
        assert st_f.shape == st_o.shape == (MPC_STEPS + 1, f.B, f.n) and err <= 1e-7, (cfg, nw, N, err)
        _guards_ok(f)
    print("fused loop", cfg, "waves", f.get_waves_per_game(), "worst |hip - orc| over the states %.2e" % WORST[("mpc", nw) + cfg])


# ---- g. the shift warm start ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", SHIFT_CONFIGS, ids=_name)
def test_init_traj_shift_at_the_ends_of_the_horizon(alg, orc, cfg):
    """alg_init_traj(use_shift) with s = 0, 1, N - 2, N - 1, N, N + 1 and 1024 at N = 2, 3 and 6 (x, u and lambda end at three different
    steps, primal_dual_traj.jl:29-44): U and lambda bit-equal to the oracle, X <= 1e-13 (test_init_traj_and_rollout_parity), and what was
    shifted in is what was stored s steps later."""
    for N in (2, 3, 6):
        for s in sorted({v for v in (0, 1, N - 2, N - 1, N, N + 1, 1024) if v >= 0}):
            g, o = _pair(alg, orc, *cfg, N, B=4, seed=11)
            z = np.random.default_rng(100 * N + s).random((g.B, g.traj_len)) + 0.25
            for b in (g, o):
                b.set_options(shift=s)
                b.set_traj(z, 0)
                b.init_traj(game_id0=1000, use_shift=True)
            _, U0, L0 = g.split_traj(z)
            Xg, Ug, Lg = g.split_traj(g.get_traj(0)); Xo, Uo, Lo = o.split_traj(o.get_traj(0))
            assert np.array_equal(Ug, Uo) and np.array_equal(Lg, Lo), (cfg, N, s)
            assert np.abs(Xg - Xo).max() <= 1e-13, (cfg, N, s, np.abs(Xg - Xo).max())
            for k in range(N - 1):
                if k + s < N - 1:                                      # both shifted in (the last control and the last costate exist: k + s <= N - 2)
                    assert np.array_equal(Ug[:, k], U0[:, k + s]) and np.array_equal(Lg[:, :, k], L0[:, :, k + s]), (cfg, N, s, k)
                else:                                                  # drawn: amplitude_init 1e-8 x U(0, 1)
                    assert np.all((Ug[:, k] > 0) & (Ug[:, k] < 1e-8)) and np.all((Lg[:, :, k] > 0) & (Lg[:, :, k] < 1e-8)), (cfg, N, s, k)
            _guards_ok(g)


# ---- h. the caller's stream -------------------------------------------------------------------------------------------------------------------------
_STREAM_CHILD = """
import sys
import torch
torch.cuda.set_device(0)                       # torch's HIP runtime first, as in bench.py
import numpy as np
import algames_jl_amd as alg
import test_gpu_horizon_shapes as HS
cfg, N = HS.UNI3, 10
a, b = HS.hip_family(alg, *cfg, N), HS.hip_family(alg, *cfg, N)
a.newton_solve(init=True, game_id0=HS.GID0)
stream = torch.cuda.Stream()
assert stream.cuda_stream != 0
b.set_stream(stream.cuda_stream)
b.newton_solve(init=True, game_id0=HS.GID0)
HS._same_bits(a, b, "caller's stream")
b.set_stream(0)
st = b.newton_solve(init=True, game_id0=HS.GID0)
HS._same_bits(a, b, "back on the library's stream")
assert st["newton_iters"].min() > 0 and st["outer_iters"].max() >= 2
stream.synchronize()
print("STREAM_OK")
"""


def test_solve_on_the_callers_stream():
    """alg_set_stream: the same problem on the library's stream and on a torch.cuda.Stream() gives the same bits; 0 hands the handle its own
    stream back and it still solves.  In a child process of its own: torch brings its own HIP runtime, which finds no device once the
    library's has initialised the GPU in the same process -- a caller that shares a stream with torch starts torch first, as bench.py does."""
    import os, subprocess, sys
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "oracle"), tests] + [q for q in [os.environ.get("PYTHONPATH")] if q]))
    r = subprocess.run([sys.executable, "-c", _STREAM_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "STREAM_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
