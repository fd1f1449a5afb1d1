"""The four log kernels -- k_player_cost<C>, k_con_values<C> (plans) and k_closed_loop_cost<C>, k_closed_loop_con<C> (the log of the fused
receding-horizon loop) -- on every configuration of ALG_CFGS_ONE (tests/log_config_family.py: 79), against cost_reference and con_reference.
tests/test_log_config_family.py holds the preconditions on the CPU; the tolerances are the references' own (cost_reference.bound,
con_reference.check), none is introduced here.

  1. plans of every configuration at the horizons N in {2, 3, KPT, KPT + 1, 2 KPT + 1} (KPT = 64 // p: the trip edges of the cost kernels and a
     third trip of one knot), the trial buffer at N = KPT + 1;
  2. the closed-loop run of every configuration over at least 2 KPT + 1 knots: both logs against the references evaluated on the states and
     controls the loop returned, with the schedule rows, the per-game block or the shared values the configuration's source prescribes;
  3. a game alone against the same game as number 2 of 3, bit for bit, over several trips;
  4. the clamp of the schedule row over the trips; 5. an unscheduled loop after a scheduled one reads the rows that one left in the blocks;
  6. the handle's log buffers grow, are reused by shorter runs and are freed.
Every handle is checked to run the kernels of the configuration it is named after (kkt_config_family.runs_its_kernel) before and after."""
import copy

import numpy as np
import pytest

import con_reference as KR
import cost_reference as CR
import kkt_config_family as F
import log_config_family as LF

pytestmark = pytest.mark.gpu

DI, UNI, BIC, QUAD = LF.DI, LF.UNI, LF.BIC, LF.QUAD
WORST = {}                                          # (what, cfg_class) -> worst error / tolerance so far


def _note(what, cfg, ratio):
    key = (what, LF.cfg_class(cfg))
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print("%-22s %-12s %-12s error / tolerance %.3g (class so far %.3g)" % (what, F.cfg_id(cfg), key[1], ratio, WORST[key]))


def _ratio(got, ref, tol):
    return float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())


def _check_plan(g, cfg, mdl, lqr, rad, mu, tab, z, N, which):
    X, U, _ = g.split_traj(z)
    # costs
    total, stage = g.get_cost(which, stage=True)
    ref_t, ref_s = CR.batch_plan_cost(mdl, LF.DT, X, U, *lqr, rad, mu)
    sc = None if rad is None else mu * rad ** 2 * (g.p - 1)                                   # (B, p)
    w = np.full(N, LF.DT); w[-1] = 1.0
    tol_t = CR.bound(ref_t, None if sc is None else w.sum() * sc)
    tol_s = CR.bound(ref_s, None if sc is None else w[None, :, None] * sc[:, None, :])
    _note("plan cost total", cfg, _ratio(total, ref_t, tol_t)); _note("plan cost stage", cfg, _ratio(stage, ref_s, tol_s))
    assert np.all(np.abs(total - ref_t) <= tol_t), (cfg, N, which, "total")
    assert np.all(np.abs(stage - ref_s) <= tol_s), (cfg, N, which, "stage")
    assert np.all(np.abs(stage.sum(axis=1) - total) <= tol_t), (cfg, N, which, "stage does not sum to total")
    assert np.all(stage[:, -1, :, 1] == 0.0), (cfg, N, which, "the terminal knot carries a control term")
    if rad is None:
        assert np.all(total[..., 2] == 0.0) and np.all(stage[..., 2] == 0.0)
    # constraint rows
    ref, scale, margin, kinds = KR.plan(g, tab, tab["nums"], z, N)
    KR.preconditions(ref, scale, margin, kinds)
    got = g.get_con_values(which)
    assert got.shape == (g.B, g.con_len)
    _note("plan constraint rows", cfg, KR.check(got, ref, scale, "%s N=%d buffer %d" % (F.cfg_id(cfg), N, which)))


@pytest.mark.parametrize("cfg", LF.CONFIGS, ids=LF.IDS)
def test_plan_costs_and_constraint_rows_on_every_configuration(alg, orc, cfg):
    mdl = LF.model_of(cfg)
    kpt = LF.KPT(cfg[1])
    for N0 in LF.plan_horizons(cfg):
        g, tw, N = LF.plan_handle(alg, orc, cfg, N0)
        assert N == N0 or N >= kpt + 1, (cfg, N0, N)
        if N != N0:
            print("%s: alg_create refused N = %d, N = %d in force" % (F.cfg_id(cfg), N0, N))
        assert F.runs_its_kernel(g, cfg), (cfg, g.get_scenario_kernels())
        tab = LF.tables_device(g, tw)
        lqr = LF.plan_lqr(tw)
        g.set_lqr(*lqr)
        rad, mu = LF.cost_numbers(tw)
        assert g.con_len == (N - 1) * g.con_knot_len()
        z, _ = LF.draw_plan(cfg, N, tab, LF.stub_of(g), 0)
        g.set_traj(z)
        if N0 == kpt + 1:                                # the trial buffer: a second trajectory, the plan's buffer untouched
            z1, _ = LF.draw_plan(cfg, N, tab, LF.stub_of(g), 1)
            g.set_traj(z1, which=alg.ALG_TRAJ_TRIAL)
            _check_plan(g, cfg, mdl, lqr, rad, mu, tab, z1, N, alg.ALG_TRAJ_TRIAL)
        _check_plan(g, cfg, mdl, lqr, rad, mu, tab, z, N, alg.ALG_TRAJ_PD)
        assert np.array_equal(g.get_traj(), z)
        assert F.runs_its_kernel(g, cfg) and g.lib.debug_check_guards(g.h) == 0
        g.close()


# ---- the closed loop --------------------------------------------------------------------------------------------------------------------------
def _check_cost_log(run, states, controls, stage, total, what):
    ref_s, ref_t, tol_s, tol_t = run.cost_reference(states, controls)
    assert stage.shape == ref_s.shape and total.shape == ref_t.shape
    _note(what + " cost stage", run.cfg, _ratio(stage, ref_s, tol_s)); _note(what + " cost total", run.cfg, _ratio(total, ref_t, tol_t))
    assert np.all(np.abs(stage - ref_s) <= tol_s), (what, run.cfg, "stage", np.abs(stage - ref_s).max())
    assert np.all(np.abs(total - ref_t) <= tol_t), (what, run.cfg, "total", np.abs(total - ref_t).max())
    return ref_s, ref_t, tol_s, tol_t


def _check_con_log(run, g, tab, states, controls, vals, worst, first, what):
    ref, scale, margin, kinds = run.con_reference(g, tab, states, controls)
    assert margin.min() >= 1e-6, "%s: an indicator argument lies %.2e from its switch on the device's own states" % (F.cfg_id(run.cfg), margin.min())
    assert vals.shape == ref.shape
    _note(what + " constraint rows", run.cfg, KR.check(vals, ref, scale, what + " " + F.cfg_id(run.cfg)))
    w, f = KR.summary(vals, kinds)                                       # from the device's own values
    assert np.array_equal(worst, w, equal_nan=True) and np.array_equal(np.signbit(worst), np.signbit(w)), (what, run.cfg)
    assert np.array_equal(first, f), (what, run.cfg)
    added = sorted(set(kinds.tolist()) - {-1})
    assert np.all(np.isneginf(worst[:, [c for c in range(7) if c not in added]]))


def _loop(alg, orc, run, cfg=None, cost_log=True, con_log=True, steps=None, x0=None, before=None):
    """a fresh handle of the run's configuration, configured, looped: (handle, twin, tables, states, controls)"""
    cfg = run.cfg if cfg is None else cfg
    g, tw = LF.problem(alg, orc, cfg, LF.N_LOOP)
    tab = LF.tables_device(g, tw)                     # the handle's numbers before the loop leaves its last rows in the blocks
    if before is not None:
        before(g)
    run.configure(g, alg, cost_log, con_log)
    if x0 is not None:
        g.set_x0(x0)
    states, controls, _ = g.mpc_solve_log(run.steps if steps is None else steps, LF.GID0)
    return g, tw, tab, states, controls


@pytest.mark.parametrize("cfg", LF.CONFIGS, ids=LF.IDS)
def test_closed_loop_logs_on_every_configuration(alg, orc, cfg):
    kpt = LF.KPT(cfg[1])
    g, tw = LF.problem(alg, orc, cfg, LF.N_LOOP)
    tab = LF.tables_device(g, tw)
    run = LF.Run(cfg, tw, tab)
    run.configure(g, alg)
    assert F.runs_its_kernel(g, cfg), (cfg, g.get_scenario_kernels())
    assert g.mpc_get_cost() == (None, None) and g.mpc_get_con() == (None, None, None)
    states, controls, stats = g.mpc_solve_log(run.steps, LF.GID0)
    assert F.runs_its_kernel(g, cfg), (cfg, g.get_scenario_kernels())
    knots = controls.shape[0]
    assert knots == run.knots >= 2 * kpt + 1                            # three trips of the cost kernel, the third of at least one knot
    assert np.isfinite(states).all() and np.isfinite(controls).all()
    stage, total = g.mpc_get_cost()
    vals, worst, first = g.mpc_get_con()
    assert stage.shape == (knots, LF.B, g.p, 3) and vals.shape == (knots, LF.B, g.con_knot_len())
    _check_con_log(run, g, tab, states, controls, vals, worst, first, "loop")
    ref_s, ref_t, _, _ = _check_cost_log(run, states, controls, stage, total, "loop")
    assert np.all(ref_t[..., :2] > 0.0) and (run.rad is None or ref_t[..., 2].max() > 0.0)
    if run.rad is None:
        assert np.all(stage[..., 2] == 0.0) and np.all(total[..., 2] == 0.0)
    # fewer knots than the run: the leading rows of the full read bit for bit, with the run's totals
    s2, t2 = g.mpc_get_cost(max_knots=kpt + 1)
    assert s2.shape[0] == kpt + 1 and s2.tobytes() == stage[:kpt + 1].tobytes() and t2.tobytes() == total.tobytes()
    v2, w2, f2 = g.mpc_get_con(max_knots=kpt + 1)
    assert v2.shape[0] == kpt + 1 and v2.tobytes() == vals[:kpt + 1].tobytes() and w2.tobytes() == worst.tobytes() and np.array_equal(f2, first)
    assert g.lib.debug_check_guards(g.h) == 0
    g.close()


@pytest.mark.parametrize("cfg", [(DI, 3, 2, 0), (QUAD, 2, 3, 1), (UNI, 10, 2, 0)], ids=F.cfg_id)
def test_a_game_alone_equals_the_game_in_the_batch_over_several_trips(alg, orc, cfg):
    """Game 2 of 3 against the same game alone.  Both handles solve with one wavefront per game, so that the loop itself gives the same
    states and controls (asserted first); the log kernels then have to give the same bits whatever the batch."""
    g3, tw = LF.problem(alg, orc, cfg, LF.N_LOOP)
    tab = LF.tables_device(g3, tw)
    run = LF.Run(cfg, tw, tab)
    x0, z3, (lam3, mu3) = g3.get_x0(), g3.get_traj(), g3.get_con_duals()
    g3.set_waves_per_game(1)
    run.configure(g3, alg)
    s3, c3, _ = g3.mpc_solve_log(run.steps, LF.GID0)
    assert c3.shape[0] >= 2 * LF.KPT(cfg[1]) + 1
    g1, _ = LF.problem(alg, orc, cfg, LF.N_LOOP, B=1)
    g1.set_waves_per_game(1)
    g1.set_x0(x0[2:3]); g1.set_lqr(*[a[2:3] for a in LF.lqr_numbers(tw)])
    for i, (xmax, xmin) in sorted(getattr(tw[0][0], "_tab", {}).get("add_state_bound", {}).items()):
        g1.add_state_bound(i, xmax, xmin)             # (the state bounds of the parity problems are drawn after the games' data: B = 1 drew others)
    g1.set_traj(z3[2:3]); g1.set_con_duals(lam3[2:3], mu3[2:3])        # (what the loop starts from, should any of it survive its first solve)
    run.configure(g1, alg, games=slice(2, 3))
    s1, c1, _ = g1.mpc_solve_log(run.steps, LF.GID0 + 2)
    assert F.runs_its_kernel(g3, cfg) and F.runs_its_kernel(g1, cfg)
    assert s1[:, 0].tobytes() == s3[:, 2].tobytes() and c1[:, 0].tobytes() == c3[:, 2].tobytes(), "the loops themselves differ"
    st3, t3 = g3.mpc_get_cost(); st1, t1 = g1.mpc_get_cost()
    assert st1[:, 0].tobytes() == st3[:, 2].tobytes() and t1[0].tobytes() == t3[2].tobytes()
    v3, w3, f3 = g3.mpc_get_con(); v1, w1, f1 = g1.mpc_get_con()
    assert v1[:, 0].tobytes() == v3[:, 2].tobytes() and w1[0].tobytes() == w3[2].tobytes() and np.array_equal(f1[0], f3[2])
    _check_cost_log(run, s3, c3, st3, t3, "batch of three")
    assert g3.lib.debug_check_guards(g3.h) == 0 and g1.lib.debug_check_guards(g1.h) == 0


def test_schedule_row_clamp_over_trips(alg, orc):
    cfg = (DI, 3, 2, 0)
    kpt = LF.KPT(3)
    g, tw = LF.problem(alg, orc, cfg, LF.N_LOOP)
    run = LF.Run(cfg, tw, LF.tables_device(g, tw), plant=(2, 2, "rk4"), target=True)
    assert run.hold == 2 and run.knots >= 2 * kpt + 1 and run.tgt.shape[0] == 2
    w = 3 * run.ni

    def looped(tgt, lqr_row=None):
        r = copy.copy(run)
        r.tgt = tgt
        before = None
        if lqr_row is not None:
            before = lambda h: h.set_lqr(run.Q, run.R, lqr_row[:, :w].reshape(LF.B, 3, run.ni), lqr_row[:, w:].reshape(LF.B, 3, run.mi))
        h, _, _, s, c = _loop(alg, orc, r, before=before)
        assert F.runs_its_kernel(h, cfg) and h.lib.debug_check_guards(h.h) == 0
        return (s, c) + h.mpc_get_cost()

    # a schedule of one row is that row set with set_lqr, no schedule
    one, plain = looped(run.tgt[1:]), looped(None, lqr_row=run.tgt[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, plain))
    # rows beyond the run are never read: steps + 2 rows against the same schedule cut to steps rows
    rng = np.random.default_rng(5)
    long = np.stack([run.tgt[0] + 0.05 * rng.normal(size=run.tgt[0].shape) for _ in range(run.steps + 2)])
    full, cut = looped(long), looped(long[:run.steps])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, cut))
    r = copy.copy(run); r.tgt = long
    _check_cost_log(r, full[0], full[1], full[2], full[3], "a row per step")
    # two rows over three trips: the second is held, and the third trip's stage rows are not what row 0 would give
    s, c, stage, total = looped(run.tgt)
    _, _, tol_s, _ = _check_cost_log(run, s, c, stage, total, "two rows, three trips")
    r0 = copy.copy(run); r0.tgt = run.tgt[:1]
    ref0 = r0.cost_reference(s, c)[0]
    assert stage.shape[0] > 2 * kpt and np.all(np.abs(stage[2 * kpt:, ..., 0] - ref0[2 * kpt:, ..., 0]) > 100.0 * tol_s[2 * kpt:, ..., 0])


@pytest.mark.parametrize("mode", ["ext", "base"])
def test_unscheduled_loop_after_a_scheduled_one_reads_what_it_left(alg, orc, mode):
    """ALG_SCEN_KERNELS_EXT: a base handle, which the schedule moves to its EXT instantiation.  ALG_SCEN_KERNELS_BASE: a base kind cannot be
    scheduled on a handle that stays on the base kernels (refused, asserted), so the mode is run where it is admitted -- on a handle of the
    extended set, where the setting is kept and has no effect."""
    cfg = (DI, 3, 2, 0) if mode == "ext" else (DI, 3, 2, 1)
    g, tw = LF.problem(alg, orc, cfg, LF.N_LOOP)
    tab = LF.tables_device(g, tw)
    run = LF.Run(cfg, tw, tab, source=LF.SRC_SCHEDULE)
    rows = np.concatenate([run.cc_rows, 1.3 * run.cc_rows[:1]])         # three rows; the first loop stops at the second
    assert rows.shape[0] == 3 and not np.array_equal(rows[1], rows[2])
    run.cc_rows = rows
    if mode == "base":
        refused, _ = LF.problem(alg, orc, (DI, 3, 2, 0), LF.N_LOOP)
        refused.set_scenario_kernels("base")
        with pytest.raises(alg.AlgamesError, match="cannot be scheduled in ALG_SCEN_KERNELS_BASE mode"):
            refused.mpc_set_schedule("collision_cost", rows)
        g.set_scenario_kernels("base")
    run.configure(g, alg, cost_log=False, con_log=False)
    assert g.get_scenario_kernels() == ((1 if mode == "base" else 0), 1)
    first_steps = 2
    g.mpc_solve_log(first_steps, LF.GID0)
    g.mpc_set_schedule("collision_cost", None)
    assert g.mpc_get_schedule("collision_cost") == 0
    g.mpc_set_cost_log(True); g.mpc_set_con_log(True)
    states, controls, _ = g.mpc_solve_log(run.steps, LF.GID0)
    stage, total = g.mpc_get_cost()
    left = copy.copy(run)
    left.cc_rows, left.cc_block = None, rows[min(first_steps - 1, rows.shape[0] - 1)]
    assert np.array_equal(g.get_scenario_data("collision_cost"), left.cc_block)
    _check_cost_log(left, states, controls, stage, total, "after a schedule, " + mode)
    # ... and neither of the other rows, nor the handle's shared values, would pass
    for other in (rows[0], rows[2], np.concatenate([run.rad, run.mu], axis=1)):
        o = copy.copy(left); o.cc_block = other
        ref_s, _, tol_s, _ = o.cost_reference(states, controls)
        assert not np.all(np.abs(stage - ref_s) <= tol_s)
    vals, worst, first = g.mpc_get_con()
    _check_con_log(left, g, tab, states, controls, vals, worst, first, "after a schedule, " + mode)
    assert g.lib.debug_check_guards(g.h) == 0


def test_log_buffers_grow_and_are_reused(alg, orc):
    cfg = (DI, 3, 2, 0)
    g, tw = LF.problem(alg, orc, cfg, LF.N_LOOP)
    run = LF.Run(cfg, tw, LF.tables_device(g, tw))
    run.configure(g, alg)
    assert run.knots >= 2 * LF.KPT(3) + 1

    def reads(h, s, c):
        return (s, c) + h.mpc_get_cost() + h.mpc_get_con()

    for steps in (2, run.steps, 2):                   # the buffers grow for the second run; the third reuses them, its total at another offset
        x0 = g.get_x0()
        s, c, _ = g.mpc_solve_log(steps, LF.GID0)
        mine = reads(g, s, c)
        assert mine[2].shape[0] == mine[4].shape[0] == steps * run.hold
        fresh, _, _, sf, cf = _loop(alg, orc, run, steps=steps, x0=x0)
        theirs = reads(fresh, sf, cf)
        for a, b, name in zip(mine, theirs, ("states", "controls", "stage", "total", "vals", "worst", "first")):
            assert a.tobytes() == b.tobytes(), (steps, name)
        if steps == run.steps:                        # ... and the long run is right, not only repeatable
            _check_cost_log(run, s, c, mine[2], mine[3], "grown buffers")
        assert g.lib.debug_check_guards(g.h) == 0 and fresh.lib.debug_check_guards(fresh.h) == 0
        fresh.close()
    # switching a log off frees it; switching it on again works
    g.mpc_set_cost_log(False); g.mpc_set_con_log(False)
    assert g.mpc_get_cost() == (None, None) and g.mpc_get_con() == (None, None, None)
    assert g.mpc_get_cost_log() is False and g.mpc_get_con_log() is False
    g.mpc_set_cost_log(True); g.mpc_set_con_log(True)
    assert g.mpc_get_cost() == (None, None) and g.mpc_get_con() == (None, None, None)       # no loop since
    s, c, _ = g.mpc_solve_log(3, LF.GID0)
    stage, total = g.mpc_get_cost()
    r = copy.copy(run); r.steps, r.knots = 3, 3 * run.hold
    _check_cost_log(r, s, c, stage, total, "after off and on")
    assert g.mpc_get_con()[0].shape[0] == 3 * run.hold and g.lib.debug_check_guards(g.h) == 0
