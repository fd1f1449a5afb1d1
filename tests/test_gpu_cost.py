"""Players' costs on the device (alg_get_cost; the cost log of the fused loop, alg_mpc_set_cost_log / alg_mpc_get_cost) against the numpy
statement of the definition, tests/cost_reference.py (pinned on the oracle's cost gradients by tests/test_cost_reference.py).

Tolerance, per component: 1e-12 (ref + w mu_i r_i^2 x number of pair terms), the second term on the collision component only
(cost_reference.bound).  Derived, not measured: all summands are non-negative, a total takes fewer than 5 000 rounding operations at these
shapes (5 000 x 2^-53 = 5.6e-13), and the cancellation in r - |.| is absolute in r.

  1. plans (no solve: a random trajectory, multipliers included, goes in through set_traj): the shapes where the item mapping can go wrong --
     lanes that carry items are the largest multiple of p in the wavefront, so N p straddles 63 / 64 / 60 --, every model, one and ten
     players, no collision cost;
  2. data and ordering: uf != 0 and zero entries of Q / R (all cases), per-game LQR and per-game collision cost in both scenario-kernel modes,
     the trial buffer, stage against total, a handle that solves with teams of four;
  3. independence of the batch, bit for bit, and a NaN that stays in its game;
  4. nothing on the handle moves;
  5. the closed loop: plant, disturbance, target schedule and collision-cost schedule of two rows (the last is held) -- the log against the
     reference on the returned states and controls, mpc_rollout fused against step-wise, log on against log off bit for bit, the asynchronous
     form, invalidation, truncation; once more on a unicycle with the default plant."""
import ctypes

import numpy as np
import pytest

import cost_reference as CR

pytestmark = pytest.mark.gpu

DI, UNI, BIC, QUAD = 0, 1, 2, 3
DT = 0.1
COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures", "refinements", "reserved")
LAST = ("outer", "ls_j", "alpha", "res", "delta", "dyn_vio", "con_vio", "sta_vio", "opt_vio")        # every field but t_elap


def _model(alg, model, p, d):
    return {DI: lambda: alg.DoubleIntegratorGame(p=p, d=d), UNI: lambda: alg.UnicycleGame(p=p), BIC: lambda: alg.BicycleGame(p=p),
            QUAD: lambda: alg.QuadrotorGame(p=p)}[model]()


def _numbers(rng, B, p, ni, mi, per_game):
    """Q, R with zero entries, xf, uf != 0, radii that leave some pairs of _traj active and some not, mu"""
    lead = (B,) if per_game else ()
    Q, R = 0.5 + rng.random(lead + (p, ni)), 0.1 + rng.random(lead + (p, mi))
    Q[..., 0, 1] = 0.0; R[..., 0, 0] = 0.0; Q[..., p - 1, ni - 1] = 0.0
    xf, uf = rng.normal(size=lead + (p, ni)), 0.5 * rng.normal(size=lead + (p, mi))
    rad, mu = 0.4 + 0.8 * rng.random(lead + (p,)), 1.0 + 9.0 * rng.random(lead + (p,))
    return Q, R, xf, uf, rad, mu


def _traj(rng, b):
    """random states (positions within a box of 1.5: distances on both sides of the radii), controls and multipliers"""
    X = rng.normal(size=(b.B, b.N, b.n)); X[:, :, :2 * b.p] = 1.5 * rng.random((b.B, b.N, 2 * b.p))
    U = rng.normal(size=(b.B, b.N - 1, b.m)); L = rng.normal(size=(b.B, b.p, b.N - 1, b.n))
    return X, U, b.join_traj(X, U, L)


def _setup(alg, model, p, d, N, B=2, seed=0, colcost=True, per_game=False, scen=None, waves=None):
    b = alg.Batch(alg.hip_lib(), model, p, N, DT, B, d=d)
    rng = np.random.default_rng([seed, model, p, d, N])
    Q, R, xf, uf, rad, mu = _numbers(rng, B, p, b.ni, b.mi, per_game)
    if scen == "base":
        b.set_scenario_kernels("base")
    b.set_x0(np.zeros((B, b.n)))
    b.set_lqr(Q, R, xf, uf)
    if colcost:
        b.add_collision_cost(rad[0] if per_game else rad, mu[0] if per_game else mu)
        if per_game:
            b.set_scenario_data("collision_cost", np.concatenate([rad, mu], axis=1))
    if waves is not None:
        b.set_waves_per_game(waves)
    X, U, z = _traj(rng, b)
    b.set_traj(z)
    return b, _model(alg, model, p, d), (Q, R, xf, uf) + ((rad, mu) if colcost else (None, None)), X, U, z


def _pairs_scale(b, rad, mu):
    return None if rad is None else np.broadcast_to(mu * rad ** 2 * (b.p - 1), (b.B, b.p))


def _check_plan(b, mdl, nums, X, U, total, stage, what):
    ref_t, ref_s = CR.batch_plan_cost(mdl, DT, X, U, *nums)
    sc = _pairs_scale(b, nums[4], nums[5])
    w = np.full(b.N, DT); w[-1] = 1.0
    tol_t = CR.bound(ref_t, None if sc is None else w.sum() * sc)
    tol_s = CR.bound(ref_s, None if sc is None else w[None, :, None] * sc[:, None, :])
    et, es = np.abs(total - ref_t), np.abs(stage - ref_s)
    print(what, "worst total error / tolerance %.3g, stage %.3g" % ((et / np.maximum(tol_t, 1e-300)).max(), (es / np.maximum(tol_s, 1e-300)).max()))
    assert np.all(et <= tol_t), (what, et.max())
    assert np.all(es <= tol_s), (what, es.max())
    # stage sums to total; the terminal knot carries no control term
    assert np.all(np.abs(stage.sum(axis=1) - total) <= tol_t), what
    assert np.all(stage[:, -1, :, 1] == 0.0), what
    assert b.lib.debug_check_guards(b.h) == 0
    return ref_t, ref_s


SHAPES = [(DI, 3, 2, 2), (DI, 3, 2, 3), (DI, 3, 2, 21), (DI, 3, 2, 22), (DI, 3, 2, 23), (DI, 2, 2, 32), (DI, 2, 2, 33), (DI, 2, 1, 4), (DI, 2, 3, 4),
          (UNI, 4, 2, 17), (BIC, 2, 2, 4), (QUAD, 2, 3, 3), (DI, 10, 2, 7)]


@pytest.mark.parametrize("model,p,d,N", SHAPES)
def test_plan_costs_over_the_shapes(alg, model, p, d, N):
    b, mdl, nums, X, U, _ = _setup(alg, model, p, d, N)
    total, stage = b.get_cost(stage=True)
    ref_t, _ = _check_plan(b, mdl, nums, X, U, total, stage, (model, p, d, N))
    assert all(ref_t[..., c].max() > 0.0 for c in range(3))                     # every component is exercised
    # either output alone gives the same bits
    assert np.array_equal(b.get_cost(), total)
    only = np.empty_like(stage)
    b.lib.check(b.lib.get_cost(b.h, 0, None, only.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    assert np.array_equal(only, stage)


def test_one_player_has_no_pairs_and_no_collision_cost_gives_zero(alg):
    b, mdl, nums, X, U, _ = _setup(alg, DI, 1, 2, 5)
    total, stage = b.get_cost(stage=True)
    _check_plan(b, mdl, nums[:4] + (None, None), X, U, total, stage, "one player")
    assert np.all(total[..., 2] == 0.0) and np.all(stage[..., 2] == 0.0)
    b, mdl, nums, X, U, _ = _setup(alg, UNI, 3, 2, 6, colcost=False)
    total, stage = b.get_cost(stage=True)
    _check_plan(b, mdl, nums, X, U, total, stage, "no collision cost")
    assert np.all(total[..., 2] == 0.0) and np.all(stage[..., 2] == 0.0)


@pytest.mark.parametrize("scen", ["ext", "base"])
def test_per_game_lqr_and_per_game_collision_cost(alg, scen):
    b, mdl, nums, X, U, _ = _setup(alg, DI, 3, 2, 9, B=3, per_game=True, scen=scen)
    assert b.get_scenario_kernels()[1] == (1 if scen == "ext" else 2)
    total, stage = b.get_cost(stage=True)
    ref_t, _ = _check_plan(b, mdl, nums, X, U, total, stage, "per game, " + scen)
    assert not np.allclose(ref_t[0], ref_t[1])


def test_the_trial_buffer(alg):
    b, mdl, nums, X, U, z = _setup(alg, UNI, 3, 2, 7)
    X2, U2, z2 = _traj(np.random.default_rng(77), b)
    b.set_traj(z2, which=alg.ALG_TRAJ_TRIAL)
    t1, s1 = b.get_cost(alg.ALG_TRAJ_TRIAL, stage=True)
    _check_plan(b, mdl, nums, X2, U2, t1, s1, "trial")
    t0, s0 = b.get_cost(alg.ALG_TRAJ_PD, stage=True)
    _check_plan(b, mdl, nums, X, U, t0, s0, "pd")
    assert not np.allclose(t0, t1)


def test_a_handle_that_solves_with_teams_of_four(alg):
    b, mdl, nums, X, U, _ = _setup(alg, DI, 3, 2, 12, waves=4)
    assert b.get_waves_per_game() == 4
    total, stage = b.get_cost(stage=True)
    _check_plan(b, mdl, nums, X, U, total, stage, "teams of four")


def test_argument_errors_leave_the_outputs_alone(alg):
    b, *_ = _setup(alg, DI, 2, 2, 4)
    out = np.full((b.B, b.p, 3), 7.0)
    D = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert b.lib.get_cost(b.h, 2, D, None) == alg.ALG_ERR_ARG and b"which" in b.lib.last_error()
    assert b.lib.get_cost(b.h, -1, D, None) == alg.ALG_ERR_ARG
    assert b.lib.get_cost(b.h, 0, None, None) == alg.ALG_ERR_ARG and b"null" in b.lib.last_error()
    assert np.all(out == 7.0)
    fresh = alg.Batch(alg.hip_lib(), DI, 2, 4, DT, 2)
    assert fresh.lib.get_cost(fresh.h, 0, D, None) == alg.ALG_ERR_STATE and np.all(out == 7.0)


def test_a_games_costs_do_not_depend_on_the_batch(alg):
    b3, mdl, nums, X, U, z = _setup(alg, DI, 3, 2, 23, B=3, per_game=True, seed=4)
    t3, s3 = b3.get_cost(stage=True)
    _check_plan(b3, mdl, nums, X, U, t3, s3, "B = 3")
    # game 2 alone
    b1 = alg.Batch(alg.hip_lib(), DI, 3, 23, DT, 1)
    Q, R, xf, uf, rad, mu = nums
    b1.set_x0(np.zeros((1, b1.n))); b1.set_lqr(Q[2:], R[2:], xf[2:], uf[2:])
    b1.add_collision_cost(rad[2], mu[2])
    b1.set_traj(z[2:].copy())
    t1, s1 = b1.get_cost(stage=True)
    assert np.array_equal(t1[0], t3[2]) and np.array_equal(s1[0], s3[2])
    # a NaN in game 1's plan (x of knot 3, player 0's first position) stays there
    zn = z.copy(); zn[1, b3.n + 1 * b3.b + 0] = np.nan
    b3.set_traj(zn)
    tn, sn = b3.get_cost(stage=True)
    for g in (0, 2):
        assert np.array_equal(tn[g], t3[g]) and np.array_equal(sn[g], s3[g])
    assert np.isnan(tn[1, 0, 0]) and np.all(np.isnan(tn[1, :, 2]))          # player 0's state term, every player's pairs with player 0
    assert np.all(np.isfinite(tn[1, 1:, :2])) and np.all(np.isnan(sn[1, 2, :, 2])) and np.all(np.isfinite(sn[1, :2]))
    assert b3.lib.debug_check_guards(b3.h) == 0 and b1.lib.debug_check_guards(b1.h) == 0


def _snapshot(b):
    lam, mu = b.get_con_duals()
    return dict(z0=b.get_traj(0), z1=b.get_traj(1), z2=b.get_traj(2), lam=lam, mu=mu, stats=b.get_stats(), gate=b.get_direction_gate(),
                hist=[b.get_history(g) for g in range(b.B)], x0=b.get_x0())


def test_nothing_else_on_the_handle_moves(alg):
    prob = alg.scenarios.make_problem("C2", np.arange(3), N=10)
    alg.newton_solve(prob)
    b = prob.batch
    before = _snapshot(b)
    assert all(len(h) > 1 for h in before["hist"])
    total, stage = alg.player_costs(prob, stage=True)
    trial = alg.player_costs(prob, which="trial")
    assert total.shape == (3, 3, 3) and stage.shape == (3, 10, 3, 3) and trial.shape == (3, 3, 3) and np.all(np.isfinite(total))
    after = _snapshot(b)
    for k in before:
        if k == "hist":
            assert all(h0.tobytes() == h1.tobytes() for h0, h1 in zip(before[k], after[k]))
        else:
            assert before[k].tobytes() == after[k].tobytes(), k
    assert b.lib.debug_check_guards(b.h) == 0


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------
STEPS, GID0, LB, LN, LP = 3, 11, 3, 6, 3


def _loop_data(model):
    rng = np.random.default_rng([9, model])
    ni, mi, n = 4, 2, 4 * LP
    Q, R = 1.0 + rng.random((LB, LP, ni)), 0.1 + 0.2 * rng.random((LB, LP, mi))
    xf = np.zeros((LB, LP, ni)); xf[:, :, :2] = 0.6 * rng.random((LB, LP, 2)) + 0.2
    uf = 0.05 * rng.normal(size=(LB, LP, mi))
    rad, mu = np.array([0.5, 0.6, 0.7]), np.array([2.0, 3.0, 4.0])
    x0 = np.zeros((LB, n)); x0[:, :2 * LP] = 0.5 * rng.random((LB, 2 * LP))
    if model == UNI:
        x0[:, 3 * LP:] = 0.1
    tgt = np.stack([np.concatenate([(xf + 0.1 * t * (rng.random(xf.shape) - 0.5)).reshape(LB, -1), uf.reshape(LB, -1)], axis=1) for t in range(2)])
    cc = np.stack([np.concatenate([np.tile(rad, (LB, 1)) * (1.0 + 0.2 * t + 0.1 * rng.random((LB, LP))), np.tile(mu, (LB, 1)) * (1.0 + 0.5 * t)], axis=1) for t in range(2)])
    W = 0.01 * (2.0 * rng.random((4, LB, n)) - 1.0)
    return dict(Q=Q, R=R, xf=xf, uf=uf, rad=rad, mu=mu, x0=x0, tgt=tgt, cc=cc, W=W)


def _loop_problem(alg, model, D):
    mdl = alg.DoubleIntegratorGame(p=LP, d=2) if model == DI else alg.UnicycleGame(p=LP)
    obj = alg.GameObjective([np.diag(q) for q in D["Q"][0]], [np.diag(r) for r in D["R"][0]], list(D["xf"][0]), list(D["uf"][0]), LN, mdl)
    obj.Qdiag, obj.Rdiag, obj.xf, obj.uf = D["Q"], D["R"], D["xf"], D["uf"]
    alg.add_collision_cost(obj, D["rad"], D["mu"])
    con = alg.GameConstraintValues(alg.ProblemSize(LN, mdl))
    alg.add_control_bound(con, np.full(mdl.m, 5.0), np.full(mdl.m, -5.0))
    opts = alg.Options(); opts.outer_iter, opts.inner_iter = 3, 6
    return mdl, alg.GameProblem(LN, DT, D["x0"], mdl, opts, obj, con, game_id0=GID0)


def _loop_handle(alg, model, D, plant, log):
    mdl, prob = _loop_problem(alg, model, D)
    b = prob.batch
    prob._sync_options()
    b.mpc_set_schedule("lqr_target", D["tgt"]); b.mpc_set_schedule("collision_cost", D["cc"]); b.mpc_set_schedule("disturbance", D["W"])
    if plant is not None:
        b.mpc_set_plant(plant)
    b.mpc_set_cost_log(log)
    assert b.mpc_get_cost_log() == log
    return mdl, prob, b


def _check_loop(mdl, D, hold, states, controls, stage, total, what):
    ref_s, ref_t = CR.closed_loop_cost(mdl, DT, hold, states, controls, D["Q"], D["R"], D["xf"], D["uf"], np.tile(D["rad"], (LB, 1)), np.tile(D["mu"], (LB, 1)),
                                       target_rows=D["tgt"], cost_rows=D["cc"])
    knots = controls.shape[0]
    sc = np.stack([DT * (lambda r: r[:, LP:] * r[:, :LP] ** 2 * (LP - 1))(D["cc"][min(q // hold, 1)]) for q in range(knots)])      # (knots, B, p)
    tol_s, tol_t = CR.bound(ref_s, sc), CR.bound(ref_t, sc.sum(axis=0))
    es, et = np.abs(stage - ref_s), np.abs(total - ref_t)
    print(what, "worst stage error / tolerance %.3g, total %.3g" % ((es / np.maximum(tol_s, 1e-300)).max(), (et / np.maximum(tol_t, 1e-300)).max()))
    assert np.all(es <= tol_s), (what, es.max())
    assert np.all(et <= tol_t), (what, et.max())
    assert np.all(ref_t[..., :2] > 0.0) and ref_t[..., 2].max() > 0.0
    return tol_s, tol_t


def _same_stats(a, c):
    return all(np.array_equal(a[f], c[f]) for f in COUNTS) and all(np.array_equal(a["last"][f], c["last"][f]) for f in LAST)


@pytest.mark.parametrize("model,plant", [(DI, (2, 2, "rk4")), (UNI, None)])
def test_the_cost_log_of_the_fused_loop(alg, model, plant):
    D = _loop_data(model)
    pl = None if plant is None else alg.Plant(*plant)
    hold = 1 if plant is None else plant[0]
    knots = STEPS * hold
    mdl, prob, b = _loop_handle(alg, model, D, pl, True)
    assert b.mpc_get_cost() == (None, None)                               # no loop yet
    states, controls, stats = b.mpc_solve_log(STEPS, GID0)
    stage, total = b.mpc_get_cost()
    assert stage.shape == (knots, LB, LP, 3) and total.shape == (LB, LP, 3)
    _check_loop(mdl, D, hold, states, controls, stage, total, "log on, model %d" % model)
    # truncation: fewer knots than the run, the total stays the run's
    s2, t2 = b.mpc_get_cost(max_knots=2)
    assert s2.shape[0] == 2 and np.array_equal(s2, stage[:2]) and np.array_equal(t2, total)
    final_on = _snapshot(b)
    totals_on = b.mpc_totals()
    # invalidation by alg_set_lqr; the next loop writes a new log
    b.set_lqr(D["Q"], D["R"], D["xf"], D["uf"])
    assert b.mpc_get_cost() == (None, None)
    assert b.lib.debug_check_guards(b.h) == 0
    # log off: the same states, controls, statistics and everything the loop leaves on the handle, bit for bit
    _, _, bo = _loop_handle(alg, model, D, pl, False)
    so, co, sto = bo.mpc_solve_log(STEPS, GID0)
    assert np.array_equal(so, states) and np.array_equal(co, controls) and _same_stats(sto, stats)
    assert bo.mpc_get_cost() == (None, None)
    final_off = _snapshot(bo)
    for k in ("z0", "z1", "z2", "lam", "mu", "x0", "gate"):
        assert final_on[k].tobytes() == final_off[k].tobytes(), k
    assert _same_stats(final_on["stats"], final_off["stats"])
    assert all(np.array_equal(x, y) for x, y in zip(totals_on, bo.mpc_totals()))
    assert bo.lib.debug_check_guards(bo.h) == 0
    # the asynchronous form: no output pointer, the log alone
    _, _, ba = _loop_handle(alg, model, D, pl, True)
    ba.lib.check(ba.lib.mpc_solve_log(ba.h, STEPS, GID0, None, None, None))
    sa, ta = ba.mpc_get_cost()
    assert np.array_equal(sa, stage) and np.array_equal(ta, total)
    # switching the log off drops it
    ba.mpc_set_cost_log(False)
    assert ba.mpc_get_cost() == (None, None) and ba.mpc_get_cost_log() is False
    assert ba.lib.debug_check_guards(ba.h) == 0


@pytest.mark.parametrize("model,plant", [(DI, (2, 2, "rk4")), (UNI, None)])
def test_rollout_costs_fused_against_step_wise(alg, model, plant):
    D = _loop_data(model)
    pl = None if plant is None else alg.Plant(*plant)
    hold = 1 if plant is None else plant[0]
    sched = {"lqr_target": D["tgt"], "collision_cost": D["cc"]}
    mdl, pf = _loop_problem(alg, model, D)
    rf = alg.mpc_rollout(pf, steps=STEPS, schedule=sched, disturbance=D["W"], fused=True, plant=pl, costs=True)
    _, ps = _loop_problem(alg, model, D)
    rs = alg.mpc_rollout(ps, steps=STEPS, schedule=sched, disturbance=D["W"], fused=False, plant=pl, costs=True)
    assert rf.stage_cost.shape == rs.stage_cost.shape == (STEPS * hold, LB, LP, 3) and rf.cost.shape == rs.cost.shape == (LB, LP, 3)
    assert np.array_equal(rf.states, rs.states) and np.array_equal(rf.controls, rs.controls)
    tol_s, tol_t = _check_loop(mdl, D, hold, rf.states, rf.controls, rf.stage_cost, rf.cost, "rollout fused, model %d" % model)
    _check_loop(mdl, D, hold, rs.states, rs.controls, rs.stage_cost, rs.cost, "rollout step-wise, model %d" % model)
    assert np.all(np.abs(rf.stage_cost - rs.stage_cost) <= tol_s) and np.all(np.abs(rf.cost - rs.cost) <= tol_t)
    assert pf.batch.mpc_get_cost_log() is False                          # the call restores the handle's setting
    plain = alg.mpc_rollout(pf, steps=1)
    assert plain.stage_cost is None and plain.cost is None
    assert pf.batch.lib.debug_check_guards(pf.batch.h) == 0 and ps.batch.lib.debug_check_guards(ps.batch.h) == 0
