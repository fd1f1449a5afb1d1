"""Constraint values on the device (alg_get_con_values; the constraint log of the fused loop, alg_mpc_set_con_log / alg_mpc_get_con) against the
numpy statement of the definition, tests/con_reference.py (pinned on the oracle's evaluate! by tests/test_con_reference.py).

Tolerance: 64 * 2^-53 * s per row, s the row's scale (con_reference: fewer than about 25 roundings on partial sums bounded by s; the factor
covers contraction differences); inert rows and rows of infinite bounds exactly.  The data keeps every indicator argument 1e-6 from its
switch and gives every kind rows of both signs (asserted: con_reference.preconditions).

  1. plans (no solve: a random trajectory through set_traj) over the shapes of con_reference.CASES.  The kernels deal items (knot, row),
     item e = knot K1 + row, to lane e % 64 of trip e / 64: the trip edges are the multiples of 64 items.  Horizons: N = 2 (one step), N = 3,
     and those at which (N - 1) K1 lands on either side of an edge -- K1 = 18 (three players, base): 54 | 72; K1 = 4 (one player): 64 | 68;
     K1 = 6 (d = 1): 60 | 66; K1 = 20 (d = 3, spherical pairs, a 3-D wall, two cylinders): 60 | 80; K1 = 42 (bicycle): 42 | 84; the extended
     planar set (K1 = 108), four unicycles (156), two quadrotors (114) and ten players with a state bound (930) cross edges inside a knot.
     The trial buffer as well;
  2. data: per-game numbers of every kind (default mode), the base kinds in ALG_SCEN_KERNELS_BASE mode, masks and a pair subset (inert rows
     exactly 0), infinite bounds (exactly -inf), a handle that solves with teams of four;
  3. agreement with the mutating path, alg_dual_penalty_update's vals on the same iterate;
  4. a game alone against the same game as number 2 of 3, bit for bit; a NaN stays in its game; nothing on the handle moves;
  5. the closed loop: three MPC steps on ext_horizon_family.ext_family for each of its MPC_EXT shapes with a plant (hold 2, two RK4
     sub-steps), a disturbance and two-row schedules of the circle and of the control bound; the 3-player unicycle with the default plant;
     a base handle in ALG_SCEN_KERNELS_BASE mode with per-game pair radii; two-row schedules of every kind at once; mpc_rollout fused
     against step-wise."""
import ctypes

import numpy as np
import pytest

import con_reference as CR
import ext_horizon_family as EH

pytestmark = pytest.mark.gpu

DI, UNI, BIC, QUAD = 0, 1, 2, 3
ALG_ERR_ARG = -1
COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures", "refinements", "reserved")
LAST = ("outer", "ls_j", "alpha", "res", "delta", "dyn_vio", "con_vio", "sta_vio", "opt_vio")        # every field but t_elap
PLAN = [("di2_p3_base", 2), ("di2_p3_base", 3), ("di2_p3_base", 4), ("di2_p3_base", 5), ("di2_p3_ext", 2), ("di2_p3_ext", 3),
        ("di2_p1", 2), ("di2_p1", 3), ("di2_p1", 17), ("di2_p1", 18), ("di1_p2", 2), ("di1_p2", 11), ("di1_p2", 12),
        ("di3_p2", 2), ("di3_p2", 3), ("di3_p2", 4), ("di3_p2", 5), ("uni_p4", 2), ("uni_p4", 3), ("bic_p2", 2), ("bic_p2", 3),
        ("quad_p2", 2), ("quad_p2", 3), ("di2_p10_sb", 2), ("di2_p10_sb", 3)]
K1 = {"di2_p3_base": 18, "di2_p3_ext": 108, "di2_p1": 4, "di1_p2": 6, "di3_p2": 20, "uni_p4": 156, "bic_p2": 42, "quad_p2": 114, "di2_p10_sb": 930}


def _plan_check(prob, z, N, what, which=0):
    b = prob.batch
    tab = CR.tables(prob)
    ref, scale, margin, kinds = CR.plan(b, tab, tab["nums"], z, N)
    CR.preconditions(ref, scale, margin, kinds)
    got = b.get_con_values(which)
    assert got.shape == (b.B, b.con_len)
    worst = CR.check(got, ref, scale, what)
    print(f"{what}: worst error / tolerance {worst:.3g}")
    return got, ref, scale, kinds


@pytest.mark.parametrize("name,N", PLAN)
def test_plan_values_over_the_shapes(alg, name, N):
    prob, z = CR.make_case(name, N, 2, seed=N)
    b = prob.batch
    assert b.con_knot_len() == K1[name] and b.con_len == (N - 1) * K1[name]
    b.set_traj(z)
    _plan_check(prob, z, N, f"{name} N={N}")
    # the trial buffer: another trajectory, the plan's buffer untouched
    z1 = 0.9 * np.roll(z, 1, axis=0)
    b.set_traj(z1, which=alg.ALG_TRAJ_TRIAL)
    tab = CR.tables(prob)
    ref, scale, margin, _ = CR.plan(b, tab, tab["nums"], z1, N)
    assert margin.min() >= 1e-6
    CR.check(b.get_con_values(alg.ALG_TRAJ_TRIAL), ref, scale, f"{name} N={N} trial")
    assert np.array_equal(b.get_traj(), z)
    assert b.lib.debug_check_guards(b.h) == 0


@pytest.mark.parametrize("name,mode", [("di2_p3_ext", "ext"), ("di3_p2", "ext"), ("quad_p2", "ext"), ("di2_p3_base", "ext"), ("di2_p3_base", "base")])
def test_per_game_numbers_of_every_kind_in_both_modes(alg, name, mode):
    N = 4
    prob, z = CR.make_case(name, N, 3, seed=7, per_game=True, scenario_kernels=mode)
    b = prob.batch
    assert b.get_scenario_kernels()[1] == (2 if mode == "base" else 1)
    tab = CR.tables(prob)
    for k, a in tab["nums"].items():
        assert not np.array_equal(a[0], a[1]), k                       # the games' numbers differ
    b.set_traj(z)
    got, ref, scale, kinds = _plan_check(prob, z, N, f"{name} per game, {mode}")
    assert np.isneginf(ref).any() and np.array_equal(np.isneginf(got), np.isneginf(ref))
    if name in ("di2_p3_ext", "di3_p2"):
        assert (scale == 0).any() and np.all(got[scale == 0] == 0.0)   # masks and the pair subset: inert rows exactly 0


def test_a_handle_that_solves_with_teams_of_four(alg):
    prob, z = CR.make_case("di2_p3_base", 6, 2, seed=3)
    b = prob.batch
    b.set_waves_per_game(4)
    assert b.get_waves_per_game() == 4
    b.set_traj(z)
    _plan_check(prob, z, 6, "teams of four")


@pytest.mark.parametrize("name", ["di2_p3_base", "di2_p3_ext", "di3_p2", "bic_p2"])
def test_agreement_with_the_mutating_path(alg, name):
    N = 5
    prob, z = CR.make_case(name, N, 2, seed=9)
    b = prob.batch
    b.set_traj(z)
    got, ref, scale, _ = _plan_check(prob, z, N, name)
    lam0, mu0 = b.get_con_duals()
    again = b.get_con_values()
    lam1, mu1 = b.get_con_duals()
    assert np.array_equal(got, again) and np.array_equal(lam0, lam1) and np.array_equal(mu0, mu1)
    mut = b.dual_penalty_update()
    CR.check(got, mut, np.where(np.isfinite(ref), scale, 0.0), name + " against alg_dual_penalty_update")
    print(f"{name}: bit-equal to alg_dual_penalty_update's vals: {np.array_equal(got, mut)}")
    lam2, _ = b.get_con_duals()
    assert not np.array_equal(lam0, lam2)                               # that path does move the multipliers


def test_argument_errors_leave_the_outputs_alone(alg):
    prob, z = CR.make_case("di1_p2", 3, 2)
    b = prob.batch
    out = np.full((2, b.con_len), 7.0)
    D = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert b.lib.get_con_values(b.h, 2, D) == ALG_ERR_ARG and b.lib.get_con_values(b.h, -1, D) == ALG_ERR_ARG
    assert b.lib.get_con_values(b.h, 0, None) == ALG_ERR_ARG
    assert np.all(out == 7.0)
    fresh = alg.Batch(alg.hip_lib(), DI, 2, 3, 0.1, 2, d=1)
    assert fresh.lib.get_con_values(fresh.h, 0, D) == -3 and np.all(out == 7.0)          # ALG_ERR_STATE: no x0


def test_a_games_rows_do_not_depend_on_the_batch_and_a_nan_stays_in_its_game(alg):
    N = 5
    for name in ("di2_p3_ext", "di3_p2", "di2_p3_base"):
        prob3, z = CR.make_case(name, N, 3, seed=5, per_game=True)
        b3 = prob3.batch
        b3.set_traj(z)
        all3 = b3.get_con_values()
        prob1 = alg.GameProblem(N, 0.1, prob3.x0[1:2], prob3.model, alg.Options(), CR._objective(prob3.model, N), [prob3.game_cons[1]])
        prob1.batch.set_traj(z[1:2])
        alone = prob1.batch.get_con_values()
        assert alone.tobytes() == all3[1:2].tobytes(), name
        zn = z.copy()
        zn[1, prob3.batch.n:2 * prob3.batch.n] = np.nan                   # x_2 of game 1
        b3.set_traj(zn)
        bad = b3.get_con_values()
        assert np.isnan(bad[1]).any() and bad[0].tobytes() == all3[0].tobytes() and bad[2].tobytes() == all3[2].tobytes(), name
        assert b3.lib.debug_check_guards(b3.h) == 0


def _snapshot(b):
    lam, mu = b.get_con_duals()
    return dict(z0=b.get_traj(0), z1=b.get_traj(1), z2=b.get_traj(2), lam=lam, mu=mu, stats=b.get_stats(), gate=b.get_direction_gate(),
                hist=[b.get_history(g) for g in range(b.B)], x0=b.get_x0())


def test_nothing_on_the_handle_moves(alg):
    prob = alg.scenarios.make_problem("C2", np.arange(3), N=10)
    alg.newton_solve(prob)
    b = prob.batch
    before = _snapshot(b)
    assert all(len(h) > 1 for h in before["hist"])
    v, t = alg.constraint_values(prob), alg.constraint_values(prob, which="trial")
    assert v.shape == t.shape == (3, b.con_len) and not np.isnan(v).any()
    after = _snapshot(b)
    for k in before:
        if k == "hist":
            assert all(h0.tobytes() == h1.tobytes() for h0, h1 in zip(before[k], after[k]))
        else:
            assert before[k].tobytes() == after[k].tobytes(), k
    assert b.lib.debug_check_guards(b.h) == 0


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------
STEPS, GID0 = 3, 11


def _same_stats(a, c):
    return all(np.array_equal(a[f], c[f]) for f in COUNTS) and all(np.array_equal(a["last"][f], c["last"][f]) for f in LAST)


def _family_handle(alg, cfg, plant, con_log, cost_log=False):
    """ext_family with two-row schedules of its circle (the second row's circle is wider: the players start inside it) and of its control
    bound (wide: never reached), a disturbance, the plant"""
    N = 3 if cfg[0] == BIC else 5
    b = EH.hip_ext_family(alg, *cfg, N)
    rng = np.random.default_rng([21, cfg[0]])
    circ, ctl = b.get_scenario_data("circle"), b.get_scenario_data("control_bound")
    crow = np.stack([circ, circ + np.array([0.02, -0.03, 0.5]) * (1.0 + 0.1 * rng.random((b.B, 1)))])
    wide = np.where(np.isfinite(ctl), np.sign(ctl) * 50.0, ctl)
    urow = np.stack([wide, np.where(np.isfinite(wide), wide * 1.2, wide)])
    W = 0.01 * (2.0 * rng.random((4, b.B, b.n)) - 1.0)
    b.mpc_set_schedule("circle", crow); b.mpc_set_schedule("control_bound", urow); b.mpc_set_schedule("disturbance", W)
    if plant is not None:
        b.mpc_set_plant(plant)
    b.mpc_set_con_log(con_log); b.mpc_set_cost_log(cost_log)
    assert b.mpc_get_con_log() == con_log
    return b, {CR.S_CIRC: crow, CR.S_CTL: urow}


def _check_log(b, tab, sched, hold, states, controls, vals, worst, first, what):
    ref, scale, margin, kinds = CR.closed_loop(b, tab, tab["nums"], states, controls, hold, sched)
    assert margin.min() >= 1e-6
    ratio = CR.check(vals, ref, scale, what)
    print(f"{what}: worst error / tolerance {ratio:.3g}")
    w, f = CR.summary(vals, kinds)                                       # from the device's own values
    assert np.array_equal(worst, w, equal_nan=True) and np.array_equal(np.signbit(worst), np.signbit(w)), what
    assert np.array_equal(first, f), what
    added = sorted(set(kinds.tolist()) - {-1})
    assert np.all(np.isneginf(worst[:, [c for c in range(7) if c not in added]]))
    return kinds, added


@pytest.mark.parametrize("cfg,plant", [(c, (2, 2, "rk4")) for c in EH.MPC_EXT] + [((UNI, 3, 2), None)])
def test_the_constraint_log_of_the_fused_loop(alg, cfg, plant):
    pl = None if plant is None else alg.Plant(*plant)
    hold = 1 if plant is None else plant[0]
    knots = STEPS * hold
    b, sched = _family_handle(alg, cfg, pl, True)
    tab = CR.tables_from_batch(b)                                        # the handle's numbers before the loop leaves its last rows in the blocks
    assert b.mpc_get_con() == (None, None, None)                         # no loop yet
    states, controls, stats = b.mpc_solve_log(STEPS, GID0)
    vals, worst, first = b.mpc_get_con()
    K = b.con_knot_len()
    assert vals.shape == (knots, b.B, K) and worst.shape == (b.B, 7) and first.shape == (b.B, 7) and first.dtype == np.int32
    kinds, added = _check_log(b, tab, sched, hold, states, controls, vals, worst, first, f"log on, cfg {cfg}, plant {plant}")
    # the test cannot pass on an all-feasible run, nor on an all-violated one: the wider circle of row 1 holds every game's players from
    # the first knot of solve 1 at the latest, the wide control bounds are never reached
    assert np.all((first[:, 4] >= 0) & (first[:, 4] <= hold)) and np.all(worst[:, 4] > 0) and np.all(first[:, 1] == -1) and np.all(worst[:, 1] < 0)
    # truncation: fewer knots than the run, the summary stays the run's
    v2, w2, f2 = b.mpc_get_con(max_knots=2)
    assert v2.shape[0] == 2 and np.array_equal(v2, vals[:2]) and w2.tobytes() == worst.tobytes() and np.array_equal(f2, first)
    final_on, totals_on = _snapshot(b), b.mpc_totals()
    # log off: the same states, controls, statistics, totals and everything the loop leaves on the handle, bit for bit
    bo, _ = _family_handle(alg, cfg, pl, False)
    so, co, sto = bo.mpc_solve_log(STEPS, GID0)
    assert np.array_equal(so, states) and np.array_equal(co, controls) and _same_stats(sto, stats)
    assert bo.mpc_get_con() == (None, None, None)
    final_off = _snapshot(bo)
    for k in ("z0", "z1", "z2", "lam", "mu", "x0", "gate"):
        assert final_on[k].tobytes() == final_off[k].tobytes(), k
    assert _same_stats(final_on["stats"], final_off["stats"])
    assert all(np.array_equal(x, y) for x, y in zip(totals_on, bo.mpc_totals()))
    # cost log and constraint log together: each as it is alone
    bc, _ = _family_handle(alg, cfg, pl, False, cost_log=True)
    bc.mpc_solve_log(STEPS, GID0)
    stage, total = bc.mpc_get_cost()
    bb, _ = _family_handle(alg, cfg, pl, True, cost_log=True)
    sb, cb, _ = bb.mpc_solve_log(STEPS, GID0)
    vb, wb, fb = bb.mpc_get_con()
    stage_b, total_b = bb.mpc_get_cost()
    assert np.array_equal(sb, states) and np.array_equal(cb, controls)
    assert vb.tobytes() == vals.tobytes() and wb.tobytes() == worst.tobytes() and np.array_equal(fb, first)
    assert stage_b.tobytes() == stage.tobytes() and total_b.tobytes() == total.tobytes()
    # the asynchronous form: no output pointer, the log alone
    ba, _ = _family_handle(alg, cfg, pl, True)
    ba.lib.check(ba.lib.mpc_solve_log(ba.h, STEPS, GID0, None, None, None))
    va, wa, fa = ba.mpc_get_con()
    assert va.tobytes() == vals.tobytes() and wa.tobytes() == worst.tobytes() and np.array_equal(fa, first)
    # invalidation by each of the four calls; the next loop writes a new log
    ba.set_lqr(np.ones((ba.p, ba.ni)), np.ones((ba.p, ba.mi)), np.zeros((ba.p, ba.ni)), np.zeros((ba.p, ba.mi)))
    assert ba.mpc_get_con() == (None, None, None)
    ba.mpc_solve_log(STEPS, GID0)
    assert ba.mpc_get_con()[0].shape == vals.shape
    ba.set_scenario_data("circle", sched[CR.S_CIRC][0])
    assert ba.mpc_get_con() == (None, None, None)
    ba.mpc_solve_log(STEPS, GID0)
    assert ba.mpc_get_con()[0] is not None
    ba.mpc_set_schedule("circle", sched[CR.S_CIRC])
    assert ba.mpc_get_con() == (None, None, None)
    ba.mpc_solve_log(STEPS, GID0)
    assert ba.mpc_get_con()[0] is not None
    ba.add_control_bound(np.full(ba.m, 60.0), np.full(ba.m, -60.0))      # an adder (it drops the schedules as well)
    assert ba.mpc_get_con() == (None, None, None)
    # a run whose log would exceed 1 GiB is refused before anything is launched
    x0, tot = ba.get_x0(), ba.mpc_totals()
    too_many = (1 << 30) // (8 * ba.B * ba.con_knot_len() * hold) + 1
    assert ba.lib.mpc_solve_log(ba.h, too_many, GID0, None, None, None) == ALG_ERR_ARG and b"constraint log" in ba.lib.last_error()
    assert np.array_equal(ba.get_x0(), x0) and all(np.array_equal(x, y) for x, y in zip(tot, ba.mpc_totals()))
    assert ba.mpc_get_con() == (None, None, None)
    # switching the log off drops it
    b.mpc_set_con_log(False)
    assert b.mpc_get_con() == (None, None, None) and b.mpc_get_con_log() is False
    for h in (b, bo, bc, bb, ba):
        assert h.lib.debug_check_guards(h.h) == 0


@pytest.mark.parametrize("name", ["di2_p3_ext", "di3_p2"])
def test_two_row_schedules_of_every_kind_the_handle_carries(alg, name):
    """pair radii (a subset / spherical), control and state bounds, walls and circles with masks, a 3-D wall and cylinders: row 1 is another
    draw of the same structure, held over the last step -- the kernel reads every kind's row in the caller's order"""
    N, B = 4, 2
    prob, _ = CR.make_case(name, N, B, seed=4, per_game=True)
    other, _ = CR.make_case(name, N, B, seed=5, per_game=True)
    b, tab = prob.batch, CR.tables(prob)
    sched = {k: np.stack([a, CR.tables(other)["nums"][k]]) for k, a in tab["nums"].items()}
    assert all(not np.array_equal(a[0], a[1]) for a in sched.values())
    prob.opts.outer_iter, prob.opts.inner_iter = 2, 4
    prob._sync_options()
    for k, a in sched.items():
        b.mpc_set_schedule(k, a)
    b.mpc_set_con_log(True)
    states, controls, _ = b.mpc_solve_log(STEPS, GID0)
    vals, worst, first = b.mpc_get_con()
    assert np.isfinite(states).all() and vals.shape == (STEPS, B, b.con_knot_len())
    kinds, added = _check_log(b, tab, sched, 1, states, controls, vals, worst, first, f"every kind scheduled, {name}")
    assert added == ([0, 1, 2, 3, 4] if name == "di2_p3_ext" else [0, 1, 5, 6])
    # the rows of solve 1 and 2 are not those of row 0: the schedule was read
    ref0 = CR.closed_loop(b, tab, tab["nums"], states, controls, 1, None)[0]
    for c in added:
        with np.errstate(invalid="ignore"):                             # (-inf) - (-inf) of the infinite bounds' rows
            d = vals[1:, :, kinds == c] - ref0[1:, :, kinds == c]
        assert np.abs(d[np.isfinite(d)]).max() > 0.0, c
    assert b.lib.debug_check_guards(b.h) == 0


def test_a_base_handle_with_per_game_pair_radii_on_the_base_kernels(alg):
    prob, _ = CR.make_case("di2_p3_base", 5, 4, seed=2, per_game=True, scenario_kernels="base")
    b = prob.batch
    assert b.get_scenario_kernels()[1] == 2
    prob.opts.outer_iter, prob.opts.inner_iter = 3, 6
    prob._sync_options()
    b.mpc_set_con_log(True)
    tab = CR.tables(prob)
    states, controls, stats = b.mpc_solve_log(STEPS, GID0)
    vals, worst, first = b.mpc_get_con()
    assert vals.shape == (STEPS, 4, 18)
    _check_log(b, tab, None, 1, states, controls, vals, worst, first, "base kernels, per-game pair radii")
    assert b.get_scenario_kernels()[1] == 2 and b.lib.debug_check_guards(b.h) == 0


@pytest.mark.parametrize("plant", [(2, 2, "rk4"), None])
def test_rollout_constraints_fused_against_step_wise(alg, plant):
    pl = None if plant is None else alg.Plant(*plant)
    hold = 1 if plant is None else plant[0]
    B = 3
    pf, rng = CR.rollout_problem(None, B)
    rows = CR.circle_rows(rng, B)
    ctl = np.stack([np.concatenate([np.full((B, 6), 0.3), np.full((B, 6), -0.25)], axis=1) * s for s in (1.0, 0.5)])
    W = 0.01 * (2.0 * rng.random((4, B, 12)) - 1.0)
    sched = {"circle": rows, "control_bound": ctl}
    rf = alg.mpc_rollout(pf, steps=STEPS, schedule=sched, disturbance=W, fused=True, plant=pl, constraints=True, costs=True)
    ps, _ = CR.rollout_problem(None, B)
    rs = alg.mpc_rollout(ps, steps=STEPS, schedule=sched, disturbance=W, fused=False, plant=pl, constraints=True)
    assert rf.con.shape == rs.con.shape == (STEPS * hold, B, 24) and rf.stage_cost is not None and rs.stage_cost is None
    assert np.array_equal(rf.states, rs.states) and np.array_equal(rf.controls, rs.controls)
    tab = CR.tables(pf)
    ref, scale, margin, kinds = CR.closed_loop(pf.batch, tab, tab["nums"], rf.states, rf.controls, hold, {CR.S_CIRC: rows, CR.S_CTL: ctl})
    assert margin.min() >= 1e-6
    for ro, what in ((rf, "rollout fused"), (rs, "rollout step-wise")):
        print(what, "worst error / tolerance %.3g" % CR.check(ro.con, ref, scale, what))
        w, f = CR.summary(ro.con, kinds)
        assert np.array_equal(ro.con_worst, w) and np.array_equal(ro.con_first, f), what
    CR.check(rf.con, rs.con, scale, "fused against step-wise")
    assert np.array_equal(rf.con_first, rs.con_first)
    assert pf.batch.mpc_get_con_log() is False and pf.batch.mpc_get_cost_log() is False      # the call restores the handle's settings
    plain = alg.mpc_rollout(pf, steps=1)
    assert plain.con is None and plain.con_worst is None and plain.con_first is None
    assert pf.batch.lib.debug_check_guards(pf.batch.h) == 0 and ps.batch.lib.debug_check_guards(ps.batch.h) == 0
