"""The plant of the fused receding-horizon loop (alg_mpc_set_plant, alg_mpc_plant_advance): the planner slower than the plant, the plant finer
than the planner's discretisation.

  1. the default plant set explicitly is today's loop bit for bit, and alg_mpc_plant_advance(0) is alg_mpc_advance;
  2. fused == step-wise, bit for bit, with schedule, disturbance and full log: the seven kernel shapes of tests/test_gpu_mpc_log.py under
     (hold, substeps, integrator) = (2, 1, rk2), (3, 4, rk4) and (N - 1, 2, rk4), and N = 3 with hold 1 and 2 (the step-wise loop is the
     definition: schedule rows, shift = hold and dual_reset = 0 from solve 1 on, newton_solve_async, get_stats and the controls of get_traj,
     per knot mpc_plant_advance(j), x0 read back, set_x0(x0 + w_q));
  3. lock-step against the oracle's own closed loop under the numpy plant (tests/test_mpc_plant_family.py holds the preconditions on the CPU);
  4. the log against the numpy plant, knot by knot;
  5. shards reproduce the whole batch;
  6. refused arguments leave the handle as it was; what keeps the plant;
  7. no kernel writes outside its buffers after a loop with hold = N - 1.

Shapes: those of tests/test_gpu_mpc_log.py (6 games, 4 for seven players, N = 8, a disturbance of 3 rows), 4 solves."""
import numpy as np
import pytest

import test_gpu_horizon_shapes as HS
import test_gpu_mpc_log as LG
import test_gpu_mpc_schedule as SCH
import test_mpc_disturbed_family as DF
import test_mpc_plant_family as PF

pytestmark = pytest.mark.gpu

STEPS, GID0 = 4, LG.GID0
COMBOS = [(2, 1, "rk2"), (3, 4, "rk4"), (LG.N - 1, 2, "rk4")]
DIST = LG.DIST


def _plant(alg, combo):
    return alg.Plant(*combo)


def stepwise(b, steps, sched, W, QR, plant, gid0=GID0):
    """The definition, on the Batch API"""
    n, m, r = b.n, b.m, plant.hold
    b.mpc_set_plant(plant)
    b.mpc_totals(reset=True)
    states, controls, stats = [b.get_x0()], [], []
    for t in range(steps):
        if t == 1:
            b.set_options(shift=r, dual_reset=0)
        for kind, a in sched.items():
            row = min(t, a.shape[0] - 1)
            if t > 0 and row == min(t - 1, a.shape[0] - 1):
                continue
            if kind == LG.TARGET:
                w = b.p * b.ni
                b.set_lqr(QR[0], QR[1], a[row][:, :w].reshape(b.B, b.p, b.ni), a[row][:, w:].reshape(b.B, b.p, b.mi))
            else:
                b.set_scenario_data(kind, a[row])
        b.newton_solve_async(init=True, game_id0=gid0 + t * 1000003)
        stats.append(b.get_stats())
        z = b.get_traj()
        for j in range(r):
            q = t * r + j
            controls.append(z[:, 2 * n + j * b.b:2 * n + j * b.b + m].copy())
            b.mpc_plant_advance(j)
            x = b.get_x0()
            if W is not None:
                x = x + W[min(q, W.shape[0] - 1)]
                b.set_x0(x)
            states.append(x)
    return np.stack(states), np.stack(controls), np.stack(stats)


def fused(b, steps, sched, W, plant, gid0=GID0):
    for kind, a in sched.items():
        b.mpc_set_schedule(kind, a)
    if W is not None:
        b.mpc_set_schedule(DIST, W)
    b.mpc_set_plant(plant)
    b.mpc_totals(reset=True)
    return b.mpc_solve_log(steps, gid0)


def assert_same_loop(rf, rs, ff, fs, what):
    (st_f, uc_f, gs_f), (st_s, uc_s, gs_s) = rf, rs
    assert st_f.shape == st_s.shape and uc_f.shape == uc_s.shape and gs_f.shape == gs_s.shape, what
    print("   %s: fused against step-wise: max |dx| %.3e, max |du| %.3e" % (what, np.abs(st_f - st_s).max(), np.abs(uc_f - uc_s).max()))
    assert np.array_equal(st_f, st_s, equal_nan=True), (what, np.abs(st_f - st_s).max())
    assert np.array_equal(uc_f, uc_s, equal_nan=True), (what, np.abs(uc_f - uc_s).max())
    LG.assert_stats_equal(gs_f, gs_s, what)
    for a, b_, part in zip(ff, fs, ("pdtraj", "lambda", "mu", "newton_iters total", "converged total")):
        assert np.array_equal(a, b_, equal_nan=True), (what, part)
    # the totals gain every solve once, whatever the plant holds
    assert np.array_equal(ff[3], gs_f["newton_iters"].sum(axis=0)) and np.array_equal(ff[4], gs_f["converged"].sum(axis=0)), what


# ---- 1. the default plant ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["di3_one_wavefront", "uni3_team_of_four", "quad2_team_of_four"])
def test_the_default_plant_set_explicitly_is_the_loop_without_a_plant(alg, name):
    plain, sched, W, QR = LG.build(alg, name)
    expl = LG.build(alg, name)[0]
    assert plain.mpc_get_plant() == alg.Plant()
    expl.mpc_set_plant(alg.Plant(1, 1, "rk2"))
    assert expl.mpc_get_plant() == alg.Plant()
    rp, re_ = LG.fused(plain, STEPS, sched, W), LG.fused(expl, STEPS, sched, W)
    assert rp[0].shape == (STEPS + 1, plain.B, plain.n) and rp[1].shape == (STEPS, plain.B, plain.m)
    assert_same_loop(re_, rp, LG.final(expl), LG.final(plain), name)
    # ... and the unscheduled, unlogged loop (k_mpc_loop itself) too
    plain2, expl2 = LG.build(alg, name)[0], LG.build(alg, name)[0]
    expl2.mpc_set_plant(alg.Plant())
    for b in (plain2, expl2):
        b.mpc_totals(reset=True)
    assert np.array_equal(plain2.mpc_solve(STEPS, GID0, record_states=True), expl2.mpc_solve(STEPS, GID0, record_states=True))
    for a, c in zip(LG.final(plain2), LG.final(expl2)):
        assert np.array_equal(a, c)


@pytest.mark.parametrize("name", ["di3_one_wavefront", "uni3_circle_ext", "di3_base_mode_twin", "bic2", "quad2_team_of_four", "di7_dense"] + list(LG.ADVANCE_SHAPES))
def test_plant_advance_of_the_default_plant_is_mpc_advance(alg, name):
    a, c = LG.build(alg, name)[0], LG.build(alg, name)[0]
    for b in (a, c):
        b.mpc_totals(reset=True)
        b.newton_solve_async(init=True, game_id0=GID0)
    a.mpc_advance()
    c.mpc_plant_advance(0)
    print("%s: mpc_plant_advance(0) against mpc_advance: max |dx0| %.3e" % (name, np.abs(a.get_x0() - c.get_x0()).max()))
    for u, v in zip(LG.final(a), LG.final(c)):
        assert np.array_equal(u, v, equal_nan=True), name
    assert np.array_equal(a.get_traj(1), c.get_traj(1), equal_nan=True)          # x_1 of trial too
    assert np.abs(a.get_x0() - LG.build(alg, name)[0].get_x0()).max() > 1e-4     # the state moved
    assert a.mpc_totals()[0].min() >= 1
    # knot 1 adds nothing to the totals and applies u_2
    it = c.mpc_totals()[0].copy()
    x, u2 = c.get_x0(), c.get_traj()[:, 2 * c.n + c.b:2 * c.n + c.b + c.m].copy()
    c.mpc_plant_advance(1)
    assert np.array_equal(c.mpc_totals()[0], it)
    if name.startswith("di3"):
        assert np.abs(c.get_x0() - PF.plant_step(0, 3, 2, x, u2, HS.DT)).max() <= 1e-13
    assert c.lib.debug_check_guards(c.h) == 0


# ---- 2. fused == step-wise, bit for bit ----------------------------------------------------------------------------------------------------------
_RUNS = {}


def runs(alg, name, combo):
    if (name, combo) not in _RUNS:
        plant = _plant(alg, combo)
        bf, sched, W, QR = LG.build(alg, name)
        bs = LG.build(alg, name)[0]
        rf = fused(bf, STEPS, sched, W, plant)
        guards = bf.lib.debug_check_guards(bf.h)
        rs = stepwise(bs, STEPS, sched, W, QR, plant)
        _RUNS[(name, combo)] = dict(bf=bf, bs=bs, fused=rf, step=rs, final_f=LG.final(bf), final_s=LG.final(bs), guards=guards, W=W)
    return _RUNS[(name, combo)]


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "%d-%d-%s" % c)
@pytest.mark.parametrize("name", list(LG.SHAPES))
def test_fused_loop_under_a_plant_equals_the_step_wise_definition_bit_for_bit(alg, name, combo):
    r = runs(alg, name, combo)
    model, p, d, nb, waves, extra = LG.SHAPES[name]
    bf, hold = r["bf"], combo[0]
    if waves:
        assert bf.get_waves_per_game() == waves
    assert bf.get_scenario_kernels()[1] == LG.KERNELS[name]
    st_f, uc_f, gs_f = r["fused"]
    assert st_f.shape == (STEPS * hold + 1, nb, bf.n) and uc_f.shape == (STEPS * hold, nb, bf.m) and gs_f.shape == (STEPS, nb)
    print("%s %s: %d wavefronts per game, Newton iterations per solve %d ... %d, converged %d of %d, |u| up to %.3f"
          % (name, combo, bf.get_waves_per_game(), gs_f["newton_iters"].min(), gs_f["newton_iters"].max(), gs_f["converged"].sum(), gs_f["converged"].size,
             np.abs(uc_f).max()))
    assert_same_loop(r["fused"], r["step"], r["final_f"], r["final_s"], "%s %s" % (name, combo))
    assert gs_f["newton_iters"].min() >= 1 and np.abs(uc_f).max() > 1e-3          # every solve iterates, the controls are not trivial
    assert np.all(np.isfinite(st_f)) and np.abs(st_f[-1] - st_f[0]).max() > 1e-3  # the plant moves the state
    assert bf.mpc_get_plant() == _plant(alg, combo)                               # the loop keeps the handle's plant
    assert r["guards"] == 0 and bf.lib.debug_check_guards(bf.h) == 0 and r["bs"].lib.debug_check_guards(r["bs"].h) == 0


@pytest.mark.parametrize("hold", [1, 2])
@pytest.mark.parametrize("cfg", [(0, 3, 2), (1, 3, 2)], ids=["di3", "uni3"])
def test_the_shortest_horizon(alg, cfg, hold):
    """N = 3: the warm start shifted by hold = 1 keeps one knot of the plan, by hold = 2 = N - 1 none; sub-steps and RK4 on top"""
    plant = alg.Plant(hold, 2, "rk4")
    bf, bs = (HS.hip_family(alg, *cfg, 3, B=6) for _ in range(2))
    for b in (bf, bs):
        b.set_waves_per_game(1)
    rng = np.random.default_rng([9, cfg[0], hold])
    W = 0.005 * (2.0 * rng.random((3, 6, bf.n)) - 1.0)
    rf = fused(bf, 5, {}, W, plant)
    rs = stepwise(bs, 5, {}, W, None, plant)
    assert rf[0].shape == (5 * hold + 1, 6, bf.n)
    assert_same_loop(rf, rs, LG.final(bf), LG.final(bs), "N = 3, %s, hold %d" % (cfg, hold))
    # alg_mpc_solve returns the same states
    bm = HS.hip_family(alg, *cfg, 3, B=6)
    bm.set_waves_per_game(1)
    bm.mpc_set_schedule(DIST, W); bm.mpc_set_plant(plant); bm.mpc_totals(reset=True)
    assert np.array_equal(bm.mpc_solve(5, GID0, record_states=True), rf[0])
    assert bf.lib.debug_check_guards(bf.h) == 0 and bm.lib.debug_check_guards(bm.h) == 0


# ---- 3. lock-step against the oracle ----------------------------------------------------------------------------------------------------------------
_FAM = {}


def family_run(alg, name, combo):
    if (name, combo) not in _FAM:
        fam = SCH.Family(name)
        g = fam.device(alg)
        g.mpc_set_schedule(DIST, DF.disturbance(fam))
        g.mpc_set_plant(_plant(alg, combo))
        out = g.mpc_solve_log(fam.steps, game_id0=SCH.GID0)
        _FAM[(name, combo)] = (fam, g, out, g.lib.debug_check_guards(g.h))
    return _FAM[(name, combo)]


@pytest.mark.parametrize("name, combo", PF.CASES, ids=PF.IDS)
def test_loop_under_a_plant_lock_step_against_the_oracle(alg, orc, name, combo):
    """The families and plants of tests/test_mpc_plant_family.py, 8 games x 6 solves in one launch against the oracle's closed loop under the
    numpy plant: counts identical, states and controls within 1e-8 relative to the largest entry, no game left out."""
    fam, g, (st, uc, gs), guards = family_run(alg, name, combo)
    assert guards == 0
    o = PF.plant_loop(fam, orc, combo)
    assert st.shape == o["states"].shape and uc.shape == o["controls"].shape and gs.shape == o["stats"].shape
    for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
        assert np.array_equal(gs[f], o["stats"][f]), (name, combo, f, gs[f], o["stats"][f])
    for what, a, b_ in (("states", st, o["states"]), ("controls", uc, o["controls"])):
        scale = max(1.0, np.abs(b_).max())
        err = np.abs(a - b_).max()
        print("%s %s: %d solves, Newton iterations %d ... %d, converged %d, worst |hip - oracle| %s %.3e (relative %.3e)"
              % (name, combo, gs.size, gs["newton_iters"].min(), gs["newton_iters"].max(), gs["converged"].sum(), what, err, err / scale))
        assert err <= 1e-8 * scale, (name, combo, what, err)


# ---- 4. the log against the numpy plant -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, combo", PF.CASES, ids=PF.IDS)
def test_the_log_is_the_numpy_plant_knot_by_knot(alg, name, combo):
    """states[q + 1] against the numpy plant from states[q] and controls[q], plus the disturbance row: 1e-13 max(1, |x|_inf) -- a cap from
    fewer than a hundred roundings per entry at substeps <= 4, not a measurement"""
    fam, g, (st, uc, gs), _ = family_run(alg, name, combo)
    hold, s, integ = combo
    W = DF.disturbance(fam)
    worst = 0.0
    for q in range(fam.steps * hold):
        nxt = PF.plant_step(fam.model, fam.p, fam.d, st[q], uc[q], fam.dt, s, integ) + W[min(q, DF.ROWS_W - 1)]
        worst = max(worst, (np.abs(st[q + 1] - nxt).max(axis=1) / np.maximum(1.0, np.abs(st[q + 1]).max(axis=1))).max())
    print("%s %s: numpy plant under the logged controls against the logged states: %.3e" % (name, combo, worst))
    assert worst <= 1e-13, worst


# ---- 5. shards ------------------------------------------------------------------------------------------------------------------------------------------
def test_shards_reproduce_the_whole_batch_under_a_plant(alg):
    ids, sigma, plant = np.arange(6), 0.004, alg.Plant(3, 4, "rk4")

    def run(sub, fused_=True):
        prob, W = alg.scenarios.c5_disturbed(sub, STEPS * plant.hold, sigma, N=LG.N)
        prob.opts.outer_iter, prob.opts.inner_iter, prob.opts.reg_0 = 7, 20, 1e-5
        prob.batch.set_waves_per_game(1)
        out = alg.mpc_rollout(prob, STEPS, disturbance=W, fused=fused_, plant=plant)
        assert prob.batch.mpc_get_schedule(DIST) == 0 and prob.batch.mpc_get_plant() == alg.Plant()      # dropped and restored
        return out
    whole = run(ids)
    assert whole.states.shape == (STEPS * 3 + 1, 6, 12) and whole.controls.shape == (STEPS * 3, 6, 6) and whole.stats.shape == (STEPS, 6)
    lo, hi = run(ids[:3]), run(ids[3:])
    for f in ("states", "controls"):
        assert np.array_equal(getattr(whole, f), np.concatenate([getattr(lo, f), getattr(hi, f)], axis=1)), f
    LG.assert_stats_equal(whole.stats, np.concatenate([lo.stats, hi.stats], axis=1), "shards")
    assert np.array_equal(whole.newton_iters, np.concatenate([lo.newton_iters, hi.newton_iters]))
    assert np.array_equal(whole.converged, np.concatenate([lo.converged, hi.converged]))
    # ... and host.mpc_rollout's own step-wise path is the same loop
    sw = run(ids, fused_=False)
    assert np.array_equal(whole.states, sw.states) and np.array_equal(whole.controls, sw.controls)
    LG.assert_stats_equal(whole.stats, sw.stats, "mpc_rollout step-wise")
    assert np.array_equal(whole.newton_iters, sw.newton_iters) and np.array_equal(whole.converged, sw.converged)
    assert np.abs(whole.states[-1] - whole.states[0]).max() > 0.1     # the vehicles travel


# ---- 6. errors; what keeps the plant ----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_handle_as_it_was_and_what_keeps_the_plant(alg):
    name, E, C = "di3_one_wavefront", alg._abi.ALG_ERR_ARG, alg._abi.C
    P = alg._abi.alg_mpc_plant
    g, sched, W, QR = LG.build(alg, name)
    good = alg.Plant(2, 3, "rk4")
    g.mpc_set_plant(good)
    for bad in (P(LG.N, 1, 0, 0), P(0, 1, 0, 0), P(-1, 1, 0, 0), P(1, 0, 0, 0), P(1, 257, 0, 0), P(1, 1, 2, 0), P(1, 1, -1, 0), P(1, 1, 0, 1)):
        assert g.lib.mpc_set_plant(g.h, C.byref(bad)) == E, (bad.hold, bad.substeps, bad.integrator, bad.reserved)
        assert g.lib.last_error().startswith(b"alg_mpc_set_plant")
        assert g.mpc_get_plant() == good
    for knot in (-1, LG.N - 1):
        assert g.lib.mpc_plant_advance(g.h, knot) == E
    assert g.lib.mpc_get_plant(g.h, None) == E
    # the bounds themselves are accepted
    g.mpc_set_plant(alg.Plant(LG.N - 1, 256, "rk2")); assert g.mpc_get_plant() == alg.Plant(LG.N - 1, 256, "rk2")
    g.mpc_set_plant(good)
    # an adder, alg_set_options, alg_set_x0, alg_set_lqr, alg_set_scenario_data and schedules keep it
    g.add_collision_avoidance(np.full(3, 0.06))
    g.set_options(shift=1)
    g.set_scenario_data(SCH.K_RAD, g.get_scenario_data(SCH.K_RAD))
    g.mpc_set_schedule(DIST, W); g.mpc_set_schedule(DIST, None)
    x0 = g.get_x0(); g.set_x0(x0)
    g.set_lqr(np.full((g.B, 3, 4), 10.0), np.full((g.B, 3, 2), 0.1), np.zeros((g.B, 3, 4)), np.zeros((g.B, 3, 2)))
    assert g.mpc_get_plant() == good
    # NULL restores the default, and the handle then runs the loop a fresh handle runs
    g2, ref = LG.build(alg, name)[0], LG.build(alg, name)[0]
    g2.mpc_set_plant(good); g2.mpc_set_plant(None)
    assert g2.mpc_get_plant() == alg.Plant()
    assert np.array_equal(g2.mpc_solve(3, GID0, record_states=True), ref.mpc_solve(3, GID0, record_states=True))
    assert g.lib.debug_check_guards(g.h) == 0 and g2.lib.debug_check_guards(g2.h) == 0


# ---- 7. guards ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LG.SHAPES))
def test_no_write_outside_the_buffers_after_a_loop_that_holds_the_whole_plan(alg, name):
    r = runs(alg, name, COMBOS[2])
    assert COMBOS[2][0] == LG.N - 1
    assert r["guards"] == 0
    assert r["bf"].lib.debug_check_guards(r["bf"].h) == 0 and r["bs"].lib.debug_check_guards(r["bs"].h) == 0
