"""The SINGULAR and NAN exits of every solver kernel shape.

Every other GPU test solves batches in which every game succeeds.  Here some games of a batch of four fail -- structurally: an exact zero
pivot (S), a NaN in the iterate (N), an infinite multiplier after the first dual update (L: NAN inside outer iteration 2, after several
records), a NaN in x0 (the receding-horizon loop) -- next to healthy games (H), on the problem families of tests/failure_family.py, whose
preconditions tests/test_failure_family.py holds on the CPU.  Every case also solves a CONTROL batch on the device, the same problem with the
failing games' data replaced by H data, and asserts (failure_family.compare_solve):

  a. discrete parity with the oracle: status, outer_iters, newton_iters, records, converged, ls_failures, outer / ls_j of every record;
  b. isolation: everything a healthy game leaves behind (HS._bits: trajectory, lambda, mu, statistics, history) is bit-equal to the control
     batch's -- games are independent blocks;
  c. healthy games against the oracle with the tolerances of test_gpu_parity: trajectory 1e-8, final statistics 1e-9, mu bit-equal and
     lambda 1e-6 relative on converged games;
  d. failing games against the oracle: record fields that are finite in the oracle to 1e-9 relative, a non-finite residual norm in the
     failing record of N / L games, the iterate of a game that failed before its first Newton iteration equal to the oracle's NaN for NaN
     (rolled-out states 1e-13), the iterate of an L game within 1e-8 with infinite lambda in the same rows;
  e. no write outside the buffers (debug_check_guards).

Horizons: N in {2, 3, 7, FT + 2} on the tile shapes (a single step, the first interior knot, a horizon inside the first chunk of the fused
pass, the first horizon that enters a second chunk), N in {2, 3, 7} on the dense shapes (failure_family.horizons); the fused loop, whose
failing game fails at its first record whatever the horizon, at N = 3 and 6.  Each family is a test function of its own."""
import numpy as np
import pytest

import failure_family as FF
import test_gpu_horizon_shapes as HS
from test_gpu_horizon_shapes import DI, DI3, UNI3, UNI4, _name, _guards_ok

pytestmark = pytest.mark.gpu

CAP = 64                                            # capacity of the profile buffer, records per game


def _waves(nw):
    def prepare(b):
        b.set_waves_per_game(nw)
        assert b.get_waves_per_game() == nw
    return prepare


# ---- 1. one wavefront per game ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", HS.BASE_CONFIGS, ids=_name)
def test_one_wavefront_failure_exits(alg, orc, cfg):
    def prepare(b):
        _waves(1)(b)
        assert b.get_scenario_kernels() == (HS.EXT, 0)
    FF.solve_family(alg, orc, cfg, FF.tile_horizons(cfg), "one wavefront", prepare)


# ---- 2. teams ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,nw", HS.TEAM_CONFIGS, ids=lambda v: _name(v) or "w%d" % v)
def test_team_failure_exits(alg, orc, cfg, nw):
    """The status reaches the wavefronts that do not run the sweeps through LDS: every wavefront leaves the loops the same way."""
    def after(g, c, o, roles, kind):
        assert np.all(g.get_stats()["reserved"] == 0), (cfg, nw, roles, kind)
    FF.solve_family(alg, orc, cfg, FF.tile_horizons(cfg), "team", _waves(nw), after=after)


# ---- 3. extended-constraint kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,wall", HS.EXT_CONFIGS, ids=lambda v: _name(v) or ("wall" if v else "plain"))
def test_ext_failure_exits(alg, orc, cfg, wall):
    def prepare(b):
        assert b.get_scenario_kernels()[1] == 1
    FF.solve_family(alg, orc, cfg, FF.tile_horizons(cfg), "EXT", prepare, wall=wall)


# ---- 4. dense configurations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", HS.DENSE_CONFIGS, ids=_name)
def test_dense_failure_exits(alg, orc, cfg):
    FF.solve_family(alg, orc, cfg, FF.DENSE_HORIZONS, "dense")


@pytest.mark.parametrize("cfg", FF.DENSE_EXT_TEAMS, ids=_name)
def test_dense_ext_team_failure_exits(alg, orc, cfg):
    """the dense-direction EXT team kernels (four wavefronts per game, test_gpu_ext_horizons.test_dense_ext_team_solve_over_horizons)"""
    def prepare(b):
        _waves(4)(b)
        assert b.get_scenario_kernels()[1] == 1

    def after(g, c, o, roles, kind):
        assert np.all(g.get_stats()["reserved"] == 0), (cfg, roles, kind)
    FF.solve_family(alg, orc, cfg, FF.DENSE_HORIZONS, "dense EXT team", prepare, wall=True, after=after)


# ---- 5. the block-reading twins of the base kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [DI3, UNI3], ids=_name)
def test_scenario_base_failure_exits(alg, orc, cfg):
    def prepare(b):                                 # (test_gpu_history_vio.test_base_scen_on_equals_off)
        b.set_scenario_kernels(HS.BASE)
        for k in (HS.K_RAD, HS.K_COST, HS.K_CTL):
            if b.scenario_data_len(k):
                b.set_scenario_data(k, b.get_scenario_data(k))
        assert b.get_scenario_kernels() == (HS.BASE, 2)
    FF.solve_family(alg, orc, cfg, FF.tile_horizons(cfg), "scenario base", prepare)


# ---- 6. hand-off ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", HS.HANDOFF_CONFIGS, ids=_name)
def test_handoff_failure_exits(alg, orc, cfg):
    """Late batch with a budget of 3: the L games park and fail inside the resume kernel.  Entry batch with a budget of 1: S / N fail in the
    first launch and must not be queued.  The control batch runs with the same budget."""
    for builder, layouts, budget, kind in ((FF.late, FF.LATE_LAYOUTS, 3, "late"), (FF.entry, FF.ENTRY_LAYOUTS, 1, "entry")):
        def prepare(b):
            _waves(1)(b)
            b.set_handoff(budget)
        for N in FF.tile_horizons(cfg):
            for roles in layouts:
                what = ("hand-off", _name(cfg), N, kind, roles)
                g, c, o = FF.run_case(FF.hip_make(alg), orc, builder, cfg, N, roles, what, ("hand-off",) + cfg, prepare=prepare)
                sg, so = g.get_stats(), o.get_stats()
                assert not (sg["status"] == HS.ALG_STATUS_PARKED).any(), (what, sg["status"])
                over = (so["records"] - 1) > budget
                assert g.get_handoff() == (budget, int(over.sum())), (what, g.get_handoff(), so["records"])
                if kind == "late":
                    assert over[FF.failing(roles)].all(), (what, so["records"])      # the L games fail inside k_newton_resume
                else:
                    assert not over[FF.failing(roles)].any(), (what, so["records"])
    print("hand-off", cfg, "worst healthy-game |hip - orc| %.2e" % FF.WORST.get(("hand-off",) + cfg, 0.0))


# ---- 7. per-record violation profiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,nw", [(DI3, 1), (UNI4, 2), ((DI, 5, 2), 0)], ids=lambda v: _name(v) or "w%d" % v)
def test_profiles_with_failing_games(alg, orc, cfg, nw):
    """set_history_profiles(CAP): the solve with profiles is the solve without them, bit for bit, with failing games in the batch; a failing
    game has a profile row per record; the healthy games' rows are the control batch's."""
    make = FF.hip_make(alg)
    for builder, roles, init in ((FF.entry, "HSNH", False), (FF.late, "HLLH", True)):
        for N in FF.horizons(cfg):
            what = ("profiles", _name(cfg), N, roles)
            on, off, c = builder(make, cfg, N, roles), builder(make, cfg, N, roles), builder(make, cfg, N, roles, control=True)
            for b in (on, off, c):
                if nw:
                    _waves(nw)(b)
            on.set_history_profiles(CAP); c.set_history_profiles(CAP)
            for b in (on, off, c):
                FF.solve(b, init)
            assert on.get_stats()["status"].tolist() == FF.statuses(roles), (what, on.get_stats()["status"])
            HS._same_bits(on, off, what)
            st = on.get_stats()
            for game in range(on.B):
                v = on.get_history_vio(game)
                assert all(len(a) == st["records"][game] for a in v.values()), (what, game, st["records"][game], {k: len(a) for k, a in v.items()})
                if roles[game] == "H":
                    vc = c.get_history_vio(game)
                    for k in v:
                        assert np.array_equal(v[k], vc[k], equal_nan=True), (what, game, k)
            _guards_ok(on)


# ---- 8. the step-wise entry points: one configuration per detection site ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", FF.STEP_CONFIGS, ids=_name)
def test_stepwise_status(alg, orc, cfg):
    """alg_newton_direction(0.0): [0, 1, 1, 0]; alg_kkt_solve at reg = 0: the same, for a range of games and for the x0 columns too, nothing
    of the handle changed; alg_newton_step(1, 1): [0, 1, 2, 0].  Healthy games as in test_gpu_parity / test_gpu_kkt_solve and bit-equal to the
    control batch's."""
    for N in FF.horizons(cfg):
        FF.stepwise_family(alg, orc, cfg, N)
    print("step-wise", cfg, "worst healthy-game |hip - orc| %.2e" % FF.WORST.get(("step-wise",) + cfg, 0.0))


# ---- 9. iterated best response ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", FF.IBR_CONFIGS, ids=_name)
def test_ibr_failure_exits(alg, orc, cfg):
    for N in FF.horizons(cfg):
        FF.ibr_family(alg, orc, cfg, N)
    print("IBR", cfg, "worst healthy-game |hip - orc| / max(1, max |z|) %.2e" % FF.WORST.get(("ibr",) + cfg, 0.0))


# ---- 10. the fused receding-horizon loop ------------------------------------------------------------------------------------------------------------
def _stepwise_log(b, steps):
    """the definition of mpc_solve_log without schedules (test_gpu_mpc_log.stepwise)"""
    b.mpc_totals(reset=True)
    states, controls, stats = [b.get_x0()], [], []
    for t in range(steps):
        if t == 1:
            b.set_options(shift=1, dual_reset=0)
        b.newton_solve_async(init=True, game_id0=HS.GID0 + t * 1000003)
        stats.append(b.get_stats())
        controls.append(b.get_traj()[:, 2 * b.n:2 * b.n + b.m].copy())
        b.mpc_advance()
        states.append(b.get_x0())
    return np.stack(states), np.stack(controls), np.stack(stats)


@pytest.mark.parametrize("cfg,nw", HS.MPC_CONFIGS, ids=lambda v: _name(v) or ("w1" if v else "team"))
def test_fused_mpc_loop_with_a_failing_game(alg, orc, cfg, nw):
    """Three steps at N = 3 and 6, game 2 with x0[1] = nan: mpc_solve fused == step-wise as test_fused_mpc_loop_over_horizons holds it
    (totals equal, states 1e-9, on one wavefront bit-equal; NaN for NaN), mpc_solve_log fused == step-wise bit for bit
    (test_gpu_mpc_log); the healthy games bit-equal to the control batch's; the failing game NAN at every step without an iteration; totals
    and discrete per-step statistics equal to the oracle's loop."""
    import test_gpu_mpc_log as ML
    make, K, bad = FF.hip_make(alg), FF.LOOP_STEPS, FF.LOOP_GAME
    ok = np.arange(4) != bad
    for N in (3, 6):
        what = ("loop", _name(cfg), nw, N)
        f, s, c, fl, sl, cl = [FF.loop(make, cfg, N, control=ctl) for ctl in (False, False, True, False, False, True)]
        for b in (f, s, c, fl, sl, cl):
            b.set_waves_per_game(nw)
        it_f, cv_f, st_f = HS.mpc_loop(f, steps=K)
        it_s, cv_s, st_s = HS.mpc_loop(s, steps=K, fused=False)
        it_c, cv_c, st_c = HS.mpc_loop(c, steps=K)
        assert np.array_equal(it_f, it_s) and np.array_equal(cv_f, cv_s), (what, it_f, it_s, cv_f, cv_s)
        assert np.array_equal(np.isnan(st_f), np.isnan(st_s)), what
        assert np.nanmax(np.abs(st_f - st_s)) <= 1e-9, (what, np.nanmax(np.abs(st_f - st_s)))
        if f.get_waves_per_game() == 1:
            assert np.array_equal(st_f, st_s, equal_nan=True), what
        assert np.isfinite(st_f[:, ok]).all() and np.array_equal(st_f[:, ok], st_c[:, ok]), (what, "states: isolation")
        assert np.array_equal(it_f[ok], it_c[ok]) and np.array_equal(cv_f[ok], cv_c[ok]), (what, "totals: isolation")
        assert it_f[bad] == 0 and cv_f[bad] == 0, (what, it_f, cv_f)
        # the logged loop
        fl.mpc_totals(reset=True); cl.mpc_totals(reset=True)
        xs_f, us_f, gs_f = fl.mpc_solve_log(K, HS.GID0)
        xs_c, us_c, gs_c = cl.mpc_solve_log(K, HS.GID0)
        xs_s, us_s, gs_s = _stepwise_log(sl, K)
        assert np.array_equal(xs_f, xs_s, equal_nan=True) and np.array_equal(us_f, us_s, equal_nan=True), what
        ML.assert_stats_equal(gs_f, gs_s, what)
        assert np.array_equal(xs_f, st_f, equal_nan=True), (what, "mpc_solve_log against mpc_solve")
        assert np.array_equal(xs_f[:, ok], xs_c[:, ok]) and np.array_equal(us_f[:, ok], us_c[:, ok]), (what, "log: isolation")
        for fld in ML.COUNTS:
            assert np.array_equal(gs_f[fld][:, ok], gs_c[fld][:, ok]), (what, fld, "isolation")
        for fld in ML.LAST:
            assert np.array_equal(gs_f["last"][fld][:, ok], gs_c["last"][fld][:, ok]), (what, "last." + fld, "isolation")
        assert np.all(gs_f["status"][:, bad] == FF.NAN) and np.all(gs_f["newton_iters"][:, bad] == 0) and np.all(gs_f["converged"][:, bad] == 0), (what, gs_f["status"])
        assert np.all(gs_f["status"][:, ok] == 0), (what, gs_f["status"])
        itl, cvl = fl.mpc_totals()
        assert np.array_equal(itl, it_f) and np.array_equal(cvl, cv_f) and cvl[bad] == 0 and itl[bad] == 0, (what, itl, cvl)
        # the oracle's loop, step by step
        o = FF.loop(FF.oracle_make(orc), cfg, N)
        xs_o, us_o, gs_o = _stepwise_log(o, K)
        it_o, cv_o = o.mpc_totals()
        assert np.array_equal(it_f, it_o) and np.array_equal(cv_f, cv_o), (what, it_f, it_o, cv_f, cv_o)
        for fld in FF.COUNTS:
            assert np.array_equal(gs_f[fld], gs_o[fld]), (what, fld, gs_f[fld], gs_o[fld])
        assert np.array_equal(gs_f["last"]["outer"], gs_o["last"]["outer"]), what
        err = np.abs(xs_f[:, ok] - xs_o[:, ok]).max()
        FF.note(("loop", nw) + cfg, err)
        assert err <= 1e-7, (what, err)                                                   # test_mpc_receding_horizon_parity
        assert np.array_equal(np.isnan(xs_f), np.isnan(xs_o)), (what, "NaN mask of the states")
        _guards_ok(f); _guards_ok(fl)
    print("fused loop", cfg, "waves", f.get_waves_per_game(), "worst healthy-game |hip - orc| over the states %.2e" % FF.WORST[("loop", nw) + cfg])


def test_fused_mpc_loop_with_a_failing_game_a_schedule_and_a_plant(alg):
    """The team of the 3-player unicycle under a plant (hold = 2, substeps = 2, RK4) and a schedule of control bounds, game 2 with x0[1] = nan: fused == step-wise bit for bit (test_gpu_mpc_plant), the healthy games bit-equal to the control
    batch's, the failing game NAN at every step."""
    import test_gpu_mpc_log as ML
    import test_gpu_mpc_plant as PL
    cfg, N, K, bad = UNI3, 6, FF.LOOP_STEPS, FF.LOOP_GAME
    ok = np.arange(4) != bad
    plant = alg.Plant(2, 2, "rk4")
    f, s, c = [FF.loop(FF.hip_make(alg), cfg, N, control=ctl) for ctl in (False, False, True)]
    for b in (f, s, c):
        b.set_waves_per_game(0)
        assert b.get_waves_per_game() > 1
    cur = f.get_scenario_data(HS.K_CTL)
    sched = {HS.K_CTL: np.stack([cur, 0.9 * cur])}
    QR = (np.full((4, 3, 4), 10.0), np.full((4, 3, 2), 0.1))
    rf, rc = PL.fused(f, K, sched, None, plant), PL.fused(c, K, sched, None, plant)
    rs = PL.stepwise(s, K, sched, None, QR, plant)
    PL.assert_same_loop(rf, rs, ML.final(f), ML.final(s), "loop with a failing game")
    (xs, us, gs), (xc, uc, gc) = rf, rc
    assert xs.shape == (2 * K + 1, 4, f.n) and us.shape == (2 * K, 4, f.m) and gs.shape == (K, 4)
    assert np.isfinite(xs[:, ok]).all() and np.array_equal(xs[:, ok], xc[:, ok]) and np.array_equal(us[:, ok], uc[:, ok]), "isolation"
    for fld in ML.COUNTS:
        assert np.array_equal(gs[fld][:, ok], gc[fld][:, ok]), (fld, "isolation")
    for fld in ML.LAST:
        assert np.array_equal(gs["last"][fld][:, ok], gc["last"][fld][:, ok]), ("last." + fld, "isolation")
    assert np.all(gs["status"][:, bad] == FF.NAN) and np.all(gs["newton_iters"][:, bad] == 0) and np.all(gs["status"][:, ok] == 0), gs["status"]
    assert gs["newton_iters"][:, ok].min() >= 1
    it, cv = f.mpc_totals()
    assert it[bad] == 0 and cv[bad] == 0, (it, cv)
    _guards_ok(f)


# ---- 11. the handle afterwards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,nw,budget", FF.AFTERWARDS, ids=lambda v: _name(v) or str(v))
def test_the_handle_after_a_failing_solve(alg, cfg, nw, budget):
    """Control slots, cache flags, the hand-off queue and the trial buffer a failed or parked game leaves behind must not reach the next solve."""
    def prepare(b):
        if nw:
            _waves(nw)(b)
        if budget:
            b.set_handoff(budget)
    for N in FF.horizons(cfg):
        FF.afterwards_family(alg, cfg, N, prepare)
