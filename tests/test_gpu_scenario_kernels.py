"""Per-game scenario data on the base kernels (alg_set_scenario_kernels, ALG_SCEN_KERNELS_BASE): a handle that carries only the base
constraint set (pair radii, collision cost, control bounds) keeps its base kernels -- fused trial pass, team kernels, straggler hand-off,
MPC loop -- when the numbers differ per game, and its multipliers on the first upload.

The oracle has no per-game entry: as in tests/test_gpu_scenario_data.py, game g of a device batch is compared with its own
OracleBatch(B = 1) built from game g's adders and solved with game_id0 + g.  That file's Case, _same_solve and _arbiter_solve are used
here; where one of its test bodies asks exactly what is asked of the base kernels, the body itself runs with Case replaced by the
BASE-mode case below (_in_base_mode)."""
import numpy as np
import pytest

import test_gpu_scenario_data as SD
from test_gpu_scenario_data import DI, UNI, K_RAD, K_COST, K_CTL, GID0, _avoid, _cost, _ctl, _same_solve, _arbiter_solve, _all_outputs

pytestmark = pytest.mark.gpu

EXT, BASE = 0, 1                                  # ALG_SCEN_KERNELS_*
ALG_STATUS_PARKED = 3
_ALL3 = lambda r, B, n, m, p: [_cost(p, r, B), _avoid(p, r, B), _ctl(m, r, B)]
# name: (model, p, d, N, ingredients).  N - 1 = 9 / 11 / 7 steps: the fused pass ends on a short chunk (AsmLds::FT: 8 steps per chunk, 13 for the
# 3-player double integrator and the 4-player unicycle, 15 for the 3-player unicycle)
FAMILIES = {
    "di2": (DI, 2, 2, 12, _ALL3), "di3": (DI, 3, 2, 10, _ALL3), "di4": (DI, 4, 2, 12, _ALL3), "di2_d3": (DI, 2, 3, 10, _ALL3),
    "uni2": (UNI, 2, 2, 12, _ALL3), "uni3": (UNI, 3, 2, 10, _ALL3), "uni4": (UNI, 4, 2, 8, _ALL3),
    "di3_cost_avoid_ctl": SD.FAMILIES["di3_cost_avoid_ctl"],
    "di3_avoid": (DI, 3, 2, 10, lambda r, B, n, m, p: [_avoid(p, r, B)]),
    "uni3_avoid_ctl": (UNI, 3, 2, 10, lambda r, B, n, m, p: [_avoid(p, r, B), _ctl(m, r, B)]),
}


class BaseCase(SD.Case):
    """SD.Case over FAMILIES above, its handle in `mode` (BASE unless said otherwise) before any per-game data is uploaded"""
    made = None                      # a list only while _in_base_mode runs a body (the cases that body built); otherwise nothing is kept alive

    def __init__(self, alg, name, B=8, seed=0, per_game=True, mode=BASE):
        saved = SD.FAMILIES
        SD.FAMILIES = FAMILIES
        try:
            super().__init__(alg, name, B=B, seed=seed, per_game=False)
        finally:
            SD.FAMILIES = saved
        self.g.set_scenario_kernels(mode)
        self.per_game = per_game
        if per_game:
            self.upload()
        if BaseCase.made is not None:
            BaseCase.made.append(self)

    def upload(self):
        for kind, v, pack, _ in self.ingr:
            self.g.set_scenario_data(kind, np.stack([pack(v[k]) for k in range(self.B)]))


def _in_base_mode(body, *args):
    """run a test body of tests/test_gpu_scenario_data.py with its Case built in BASE mode; every handle it made must have run the base kernels'
    block-reading twins"""
    assert SD.Case is not BaseCase and BaseCase.made is None          # not nested; the other file's names are as that file defines them
    saved, made = SD.Case, []
    SD.Case, BaseCase.made = BaseCase, made
    try:
        body(*args)
    finally:
        SD.Case, BaseCase.made = saved, None
    assert made
    for c in made:
        assert c.g.get_scenario_kernels() == (BASE, 2)


# ---- 1. path taken -----------------------------------------------------------------------------------------------------------------------
def test_base_mode_keeps_kernels_layout_and_multipliers(alg):
    rng = np.random.default_rng(1)
    got = {}
    for mode in (BASE, EXT):
        c = BaseCase(alg, "di3_avoid", B=4, seed=1, per_game=False, mode=mode)
        g = c.g
        assert g.get_scenario_kernels() == (mode, 0)
        con_len = g.con_len
        lam, mu = rng.random((c.B, con_len)), 1.0 + rng.random((c.B, con_len))
        g.set_con_duals(lam, mu)
        c.upload()                                                         # per-game radii
        lam1, mu1 = g.get_con_duals()
        got[mode] = (g.get_scenario_kernels(), g.con_len == con_len, np.array_equal(lam1, lam) and np.array_equal(mu1, mu))
        if mode == EXT:                                                    # what the option changes: the default re-creates lambda and mu
            assert np.all(lam1 == 0.0) and np.all(mu1 == 1.0)               # lambda = 0, mu = rho_0 (Options() default)
            continue
        g.set_scenario_data(K_RAD, None)                                   # the last kind back to shared: the base kernels again
        assert g.get_scenario_kernels() == (BASE, 0)
        c.upload()
        assert g.get_scenario_kernels() == (BASE, 2)
        g.add_wall_constraint([5.0], [5.0], [6.0], [5.0], [0.0], [1.0])    # an extended adder switches to EXT as ever
        assert g.get_scenario_kernels() == (BASE, 1)
        assert g.con_len > con_len
        assert np.array_equal(g.get_scenario_data(K_RAD), np.tile(g.get_scenario_data(K_RAD)[0], (c.B, 1)))       # per-game data dropped
    assert got[BASE] == ((BASE, 2), True, True)
    assert got[EXT] == ((EXT, 1), True, False)


# ---- 2. the same bits as the base kernel when the numbers are equal ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,waves", [("C2", 1), ("C5", 1), ("C3", 1), ("C5", 4)])
def test_equal_blocks_give_the_base_kernels_bits(alg, cfg, waves):
    """handle a: base kernels, shared values; handle b: BASE mode, every game's block a copy of those values (C2 shape N = 40, the 3- and the
    4-player unicycle on one wavefront, and the 3-player unicycle on a team of four; 64 games)"""
    a = alg.scenarios.make_problem(cfg, np.arange(64)); b = alg.scenarios.make_problem(cfg, np.arange(64))
    b.batch.set_scenario_kernels(BASE)
    kinds = [k for k in (K_RAD, K_COST, K_CTL) if b.batch.scenario_data_len(k)]
    assert K_RAD in kinds
    for k in kinds:
        b.batch.set_scenario_data(k, b.batch.get_scenario_data(k))
    assert a.batch.get_scenario_kernels() == (EXT, 0) and b.batch.get_scenario_kernels() == (BASE, 2)
    for pr in (a, b):
        pr.batch.set_waves_per_game(waves)
        assert pr.batch.get_waves_per_game() == waves
        alg.newton_solve(pr)
    for x, y in zip(_all_outputs(a.batch), _all_outputs(b.batch)):
        assert np.array_equal(x, y)
    sa, sb = a.batch.get_stats(), b.batch.get_stats()
    for f in sa.dtype.names:
        if f != "last":
            assert np.array_equal(sa[f], sb[f]), f
    for f in sa["last"].dtype.names:
        if f != "t_elap":
            assert np.array_equal(sa["last"][f], sb["last"][f]), f
    for game in range(64):
        ha, hb = a.batch.get_history(game), b.batch.get_history(game)
        for f in ha.dtype.names:
            if f != "t_elap":                                              # (wall time of the iteration)
                assert np.array_equal(ha[f], hb[f]), (f, game)


# ---- 3. parity per game ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["di2", "di3", "di4", "di2_d3", "uni2", "uni3", "uni4"])
def test_solve_parity_per_game(alg, orc, name):
    c = BaseCase(alg, name)
    assert c.g.get_scenario_kernels() == (BASE, 2)
    st = c.g.newton_solve(init=True, game_id0=GID0)
    for game in range(c.B):
        o = c.oracle(orc, game)
        so = o.newton_solve(init=True, game_id0=GID0 + game)
        _same_solve(c.g, o, game, st, so, arbiter=lambda: _arbiter_solve(c, orc, game))


@pytest.mark.parametrize("name", ["di2", "di3", "di4", "di2_d3", "uni2", "uni3", "uni4"])
def test_step_wise_entry_points_per_game(alg, orc, name):
    _in_base_mode(SD.test_step_wise_entry_points_per_game, alg, orc, name)


def test_ibr_per_game(alg, orc):
    _in_base_mode(SD.test_ibr_per_game, alg, orc)


def test_mpc_per_game(alg, orc):
    _in_base_mode(SD.test_mpc_per_game, alg, orc)


def test_warm_start_keeps_the_duals(alg, orc):
    _in_base_mode(SD.test_warm_start_keeps_the_duals, alg, orc)


# ---- 4. teams ----------------------------------------------------------------------------------------------------------------------------------
def test_small_batch_with_per_game_radii_runs_the_team_kernel(alg, orc):
    c = BaseCase(alg, "uni3_avoid_ctl", B=64, seed=15)
    assert c.g.get_scenario_kernels() == (BASE, 2)
    assert c.g.get_waves_per_game() == 4
    d = BaseCase(alg, "uni3_avoid_ctl", B=64, seed=15, mode=EXT)          # the gap this closes: the same data in default mode
    assert d.g.get_scenario_kernels() == (EXT, 1) and d.g.get_waves_per_game() == 1
    sg = c.g.mpc_solve(10, game_id0=GID0, record_states=True)
    for game in range(c.B):
        o = c.oracle(orc, game)
        so = o.mpc_solve(10, game_id0=GID0 + game, record_states=True)
        assert np.abs(sg[:, game] - so[:, 0]).max() <= 1e-8 * max(1.0, np.abs(so).max()), game


# ---- 5. hand-off -------------------------------------------------------------------------------------------------------------------------------
def _handoff_inputs(alg, B=512):
    from algames_jl_amd import scenarios
    model, N, dt, x0, obj, con, opts = scenarios.c2_double_integrator(np.arange(B))       # N = 40
    rng = np.random.default_rng(5)                                                        # draws in this order
    x0[:, :6] += rng.uniform(-0.3, 0.3, (B, 6))
    r = 0.2 + 0.1 * rng.random((B, 3))                                                    # pair radii 0.4 .. 0.6
    umax = 8.0 + rng.random((B, 6)); umin = -8.0 - rng.random((B, 6))
    cons = []
    for g in range(B):
        gc = alg.GameConstraintValues(alg.ProblemSize(N, model))
        alg.add_collision_avoidance(gc, r[g]); alg.add_control_bound(gc, umax[g], umin[g])
        cons.append(gc)
    return model, N, dt, x0, obj, cons, opts


def _handoff_solve(alg, prob, handoff=0):
    b = prob.batch
    b.set_waves_per_game(1)
    if handoff:
        b.set_handoff(handoff)
    alg.newton_solve(prob)
    return prob.stats.summary.copy(), b.get_traj().copy(), b.get_con_duals()


def test_handoff_with_per_game_radii_and_bounds(alg, orc):
    """512 games of the C2 shape, x0 +- 0.3, radii and control bounds drawn per game, budget K = 24.  Reference side, checked on the CPU: the
    one-game oracles make 14 ... 89 records (median 20), 508 of 512 converge, no status other than OK, 89 games (17.4 %) make more than 25
    records and park; oracle (double) and arbiter (long double) differ in (status, outer_iters, newton_iters, converged) in 0 of 512 games -- the
    reference uses none of the 10 % that may be left out below.  Measured on the MI355X: the plain solve makes 14 ... 89 records (median 20), 89
    games park; the plain solve takes the oracle's path on 89 of the 89 parked games, so none is left out; 85 of them converge, with
    |z - z_oracle| median 2.1e-13, max 5.6e-13."""
    B, K = 512, 24
    model, N, dt, x0, obj, cons, opts = _handoff_inputs(alg, B)
    mk = lambda **kw: alg.GameProblem(N, dt, x0, model, opts, obj, cons, **kw)
    plain = mk(scenario_kernels="base")
    assert plain.batch.get_scenario_kernels() == (BASE, 2)
    s0, z0, _ = _handoff_solve(alg, plain)
    dflt = mk()                                                              # default mode: the EXT kernels have no hand-off pair
    dflt.batch.set_waves_per_game(1)
    with pytest.raises(alg.AlgamesError, match="code -1"):
        dflt.batch.set_handoff(K)
    ho = mk(scenario_kernels="base")
    s1, z1, (lam1, mu1) = _handoff_solve(alg, ho, handoff=K)
    k, parked = ho.batch.get_handoff()
    assert k == K
    over = (s0["records"] - 1) > K
    print("records (plain): min %d median %d max %d; parked %d, expected %d" % (s0["records"].min(), np.median(s0["records"]), s0["records"].max(), parked, over.sum()))
    assert parked == int(over.sum()) > 0, (parked, int(over.sum()))
    assert not (s1["status"] == ALG_STATUS_PARKED).any()
    early = ~over
    assert early.sum() > 0
    assert np.array_equal(z0[early].view(np.uint64), z1[early].view(np.uint64))
    for f in ("newton_iters", "outer_iters", "converged", "status", "records", "ls_failures"):
        assert np.array_equal(s0[f][early], s1[f][early]), f
    # the parked games against their one-game oracles
    late = np.nonzero(over)[0]
    fields = ("status", "outer_iters", "newton_iters", "converged", "ls_failures")
    sc, zc, muc = {}, {}, {}
    for g in late:
        o = alg.GameProblem(N, dt, x0[g:g + 1], model, opts, obj, cons[g], backend=orc.lib(), game_id0=int(g))
        alg.newton_solve(o)
        sc[g], zc[g], muc[g] = o.stats.summary.copy(), o.batch.get_traj()[0].copy(), o.batch.get_con_duals()[1][0].copy()
    same_plain = np.array([all(s0[f][g] == sc[g][f][0] for f in ("newton_iters", "outer_iters", "converged", "status")) for g in late])
    print("parked games whose plain solve takes the oracle's path: %d of %d" % (same_plain.sum(), len(late)))
    assert same_plain.sum() >= 0.9 * len(late), (int(same_plain.sum()), len(late))
    ok = late[same_plain]
    for f in fields:
        bad = [int(g) for g in ok if s1[f][g] != sc[g][f][0]]
        assert not bad, (f, bad[:8])
    conv = [g for g in ok if sc[g]["converged"][0] == 1]
    assert conv
    err = np.array([np.abs(z1[g] - zc[g]).max() for g in conv])
    print("parked, converged: %d games, |z - z_oracle| median %.3e max %.3e" % (len(conv), np.median(err), err.max()))
    assert np.median(err) < 1e-9 and err.max() < 1e-6, (np.median(err), err.max())
    assert all(np.array_equal(mu1[g], muc[g]) for g in conv)                  # penalties: bit-equal (powers of rho_increase)


def test_a_budget_set_before_the_data_stays_in_force(alg):
    c = BaseCase(alg, "di3_cost_avoid_ctl", B=16, seed=16, per_game=False)
    c.g.set_waves_per_game(1); c.g.set_handoff(2)
    c.upload()
    assert c.g.get_scenario_kernels() == (BASE, 2)
    st = c.g.newton_solve(init=True, game_id0=GID0)
    k, parked = c.g.get_handoff()
    assert k == 2 and parked == int(((st["records"] - 1) > 2).sum()) > 0
    assert not (st["status"] == ALG_STATUS_PARKED).any()


# ---- 6. permutation and shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["di3_cost_avoid_ctl"])
def test_permuting_the_games_permutes_every_output(alg, name):
    _in_base_mode(SD.test_permuting_the_games_permutes_every_output, alg, name)


def test_sharded_problem_equals_the_whole_problem(alg):
    from algames_jl_amd import scenarios, sharding
    B = 16
    model, N, dt, x0, obj, con, opts = scenarios.c2_double_integrator(np.arange(B), N=12)
    rng = np.random.default_rng(14)
    cons = []
    for k in range(B):
        gc = alg.GameConstraintValues(alg.ProblemSize(N, model))
        alg.add_collision_avoidance(gc, 0.12 if k < 9 else 0.1 + 0.05 * rng.random(3))       # the first shard's games are all equal
        alg.add_control_bound(gc, 1.0 + rng.random(6), -1.0 - rng.random(6))
        cons.append(gc)
    whole = alg.GameProblem(N, dt, x0, model, opts, obj, cons, scenario_kernels="base")
    sh = sharding.ShardedGameProblem(N, dt, x0, model, opts, obj, cons, devices=[0, 0], scenario_kernels="base")
    assert whole.batch.get_scenario_kernels() == (BASE, 2)
    assert all(s.batch.get_scenario_kernels() == (BASE, 2) for s in sh.shards)
    alg.newton_solve(whole)
    sharding.newton_solve_sharded(sh)
    assert np.array_equal(whole.batch.get_traj(), sh.get_traj())
    a, b = whole.batch.get_stats(), sh.get_stats()
    for f in ("status", "newton_iters", "outer_iters", "records", "converged"):
        assert np.array_equal(a[f], b[f]), f


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors(alg):
    E = alg.AlgamesError
    c = BaseCase(alg, "di3_cost_avoid_ctl", B=2, seed=9)
    g = c.g
    before = [g.get_scenario_data(k) for k in (K_RAD, K_COST, K_CTL)]
    with pytest.raises(E, match="code -3") as e:                              # mode change while per-game data is loaded
        g.set_scenario_kernels(EXT)
    assert "alg_set_scenario_kernels" in str(e.value)
    assert g.get_scenario_kernels() == (BASE, 2)
    assert all(np.array_equal(x, g.get_scenario_data(k)) for x, k in zip(before, (K_RAD, K_COST, K_CTL)))
    with pytest.raises(E, match="code -1"):
        g.set_scenario_kernels(2)
    with pytest.raises(E, match="code -1"):
        g.set_scenario_kernels(-1)
    for k in (K_RAD, K_COST, K_CTL):
        g.set_scenario_data(k, None)
    g.set_scenario_kernels(EXT)                                               # no per-game data left: accepted
    assert g.get_scenario_kernels() == (EXT, 0)
    # configurations without such kernels: DoubleIntegrator d = 1, five players
    for kw in (dict(p=2, d=1), dict(p=5, d=2)):
        h = alg.Batch(alg.hip_lib(), DI, kw["p"], 6, 0.1, 2, d=kw["d"])
        with pytest.raises(E, match="code -1") as e:
            h.set_scenario_kernels(BASE)
        assert "alg_set_scenario_kernels" in str(e.value)
        assert h.get_scenario_kernels() == (EXT, 0)
    # a handle that already is EXT accepts the call and ignores the setting
    b = alg.Batch(alg.hip_lib(), 2, 2, 6, 0.1, 2)                             # bicycle
    b.set_scenario_kernels(BASE)
    assert b.get_scenario_kernels()[1] == 1
    with pytest.raises(ValueError):
        g.set_scenario_kernels("fused")


# ---- 8. full size ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_c2_shape_at_4096_games_with_per_game_radii_and_bounds(alg, orc):
    from algames_jl_amd import scenarios
    B = 4096
    model, N, dt, x0, obj, con, opts = scenarios.c2_double_integrator(np.arange(B))
    rng = np.random.default_rng(12)
    r = 0.1 + 0.05 * rng.random((B, 3))                          # pair radii r_i + r_j in [0.2, 0.3]
    umax = 1.0 + rng.random((B, 6)); umin = -1.0 - rng.random((B, 6))
    g = alg.Batch(alg.hip_lib(), 0, 3, N, dt, B)
    g.set_scenario_kernels(BASE)
    g.set_options(**opts.to_abi())
    Q, R = np.broadcast_to(obj.Qdiag, (B,) + obj.Qdiag.shape).copy(), np.broadcast_to(obj.Rdiag, (B,) + obj.Rdiag.shape).copy()
    xf, uf = np.broadcast_to(obj.xf, (B,) + obj.xf.shape).copy(), np.broadcast_to(obj.uf, (B,) + obj.uf.shape).copy()
    g.set_x0(x0); g.set_lqr(Q, R, xf, uf)
    g.add_collision_cost(obj.collision_radius, obj.collision_μ)
    g.add_collision_avoidance(r[0]); g.add_control_bound(umax[0], umin[0])
    g.set_scenario_data(K_RAD, ((r[:, :, None] + r[:, None, :]) * (1 - np.eye(3))).reshape(B, 9))
    g.set_scenario_data(K_CTL, np.concatenate([umax, umin], axis=1))
    assert g.get_scenario_kernels() == (BASE, 2) and g.get_waves_per_game() == 1
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
