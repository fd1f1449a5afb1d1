"""The closed-loop log and the plant disturbance of the fused receding-horizon loop (alg_mpc_solve_log, ALG_SCHED_DISTURBANCE).

  1. fused == step-wise, bit for bit, one case per kernel shape the phases can differ on (the step-wise loop is the definition: schedule rows,
     newton_solve_async, get_stats and u_1 of get_traj, mpc_advance, x_1 read back, set_x0(x_1 + w_t));
  2. a log alone, and an all-zero disturbance, change nothing of alg_mpc_solve's results;
  3. the logged control is the applied one: a numpy RK2 step of states[t] under controls[t] meets states[t+1] - w_t;
  4. the disturbance bites;
  5. lock-step against the oracle's own disturbed closed loop (tests/test_mpc_disturbed_family.py holds the preconditions on the CPU);
  6. shards reproduce the whole batch;
  7. the error paths leave the handle as it was; what drops the disturbance;
  8. no kernel writes outside its buffers.

Shapes: B = 6 games (4 for seven players), 5 steps, N = 8, the options of the horizon family, a disturbance of 3 rows (held from step 2 on)."""
import numpy as np
import pytest

import test_gpu_horizon_shapes as HS
import test_gpu_mpc_schedule as SCH
import test_mpc_disturbed_family as DF

pytestmark = pytest.mark.gpu

DI, UNI, BIC, QUAD = 0, 1, 2, 3
B, STEPS, N, ROWS, GID0 = 6, 5, 8, 3, 7
DIST, TARGET = "disturbance", "lqr_target"
COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures", "refinements", "reserved")
LAST = ("outer", "ls_j", "alpha", "res", "delta", "dyn_vio", "con_vio", "sta_vio", "opt_vio")        # every field but t_elap


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------------
def _quadrotors(make, nb):
    """two quadrotors (n = 24, m = 8) that change sides at height 0.5: the set of scenarios.quadrotor_crossing on the Batch API"""
    b = make(QUAD, 2, N, HS.DT, nb, 3)
    rng = np.random.default_rng(3)
    p, hover = 2, 0.5 * 9.81 / 4 / 1.245
    ang = 2 * np.pi * np.arange(p) / p + rng.uniform(-0.1, 0.1, (nb, p))
    x0 = np.zeros((nb, b.n)); xf = np.zeros((nb, p, 12))
    x0[:, 0:p], x0[:, p:2 * p], x0[:, 2 * p:3 * p] = 0.6 * np.cos(ang), 0.6 * np.sin(ang), 0.5 + rng.uniform(-0.05, 0.05, (nb, p))
    xf[:, :, 0], xf[:, :, 1], xf[:, :, 2] = 0.6 * np.cos(ang + np.pi + 0.3), 0.6 * np.sin(ang + np.pi + 0.3), 0.5
    Q = np.tile(np.concatenate([np.ones(3), 0.5 * np.ones(3), 0.2 * np.ones(3), 0.2 * np.ones(3)]), (nb, p, 1))
    b.set_x0(x0)
    b.set_lqr(Q, np.full((nb, p, 4), 0.1), xf, np.full((nb, p, 4), hover))
    b.set_options(**HS.OPTS)
    b.add_collision_avoidance(np.full(p, 0.1))
    b.add_control_bound(np.full(b.m, 3.0), np.zeros(b.m))
    return b, Q, np.full((nb, p, 4), 0.1), xf, np.full((nb, p, 4), hover)


# name -> (model, p, d, games, waves per game, extras)
SHAPES = {
    "di3_one_wavefront": (DI, 3, 2, B, 1, ()),
    "uni3_team_of_four": (UNI, 3, 2, B, 4, ("target",)),
    "uni3_circle_ext": (UNI, 3, 2, B, 0, ("circle",)),
    "di3_base_mode_twin": (DI, 3, 2, B, 0, ("base", "target")),
    "bic2": (BIC, 2, 2, B, 0, ()),
    "quad2_team_of_four": (QUAD, 2, 3, B, 4, ()),
    "di7_dense": (DI, 7, 2, 4, 0, ("target",)),
}
# the kernels every shape must run on (get_scenario_kernels()[1]): 0 base, 1 EXT (the circle; the bicycle, which is compiled as EXT only),
# 2 the block-reading twins of the base kernels
KERNELS = {"di3_one_wavefront": 0, "uni3_team_of_four": 0, "uni3_circle_ext": 1, "di3_base_mode_twin": 2, "bic2": 1, "quad2_team_of_four": 0, "di7_dense": 0}
# Shapes that build() knows and the tests parametrised over SHAPES do not run: two double integrators on a line (d = 1) and in space (d = 3), the
# trip counts of the RK2 step's loop over the dimensions that no shape above has (tests/test_gpu_mpc_plant.py, the default plant's advance)
ADVANCE_SHAPES = {"di2_line": (DI, 2, 1, B, 0, ()), "di2_space": (DI, 2, 3, B, 0, ())}


def build(alg, name):
    """(batch, schedule {kind: rows}, disturbance, LQR data for the step-wise target rows) of one shape; deterministic"""
    model, p, d, nb, waves, extra = SHAPES.get(name) or ADVANCE_SHAPES[name]

    lqr = {}

    def make(model_, p_, N_, dt_, B_, d_):
        b = alg.Batch(alg.hip_lib(), model_, p_, N_, dt_, B_, d=d_)
        if "base" in extra:
            b.set_scenario_kernels("base")
        set_lqr = b.set_lqr

        def keep_lqr(Q, R, xf, uf):                        # the family's targets, for the target schedule
            if not lqr:
                lqr.update(xf=np.array(xf, dtype=np.float64))
            set_lqr(Q, R, xf, uf)
        b.set_lqr = keep_lqr
        return b
    if model == QUAD:
        b, Q, R, xf, uf = _quadrotors(make, nb)
    else:
        b = HS.family(make, model, p, d, N, B=nb)
        ni, mi = b.n // p, b.mi
        Q, R, uf = np.full((nb, p, ni), 10.0), np.full((nb, p, mi), 0.1), np.zeros((nb, p, mi))
        xf = None
    rng = np.random.default_rng([5, model, p])
    if "circle" in extra:
        b.add_circle_constraint([0.05], [0.1], [0.08])
    if "base" in extra:                                   # per-game radii keep the handle on the block-reading twins
        b.set_scenario_data(SCH.K_RAD, np.stack([SCH._pairs(p)(0.13 + 0.01 * rng.random(p)) for _ in range(nb)]))
    b.set_waves_per_game(waves)
    sched = {}
    if "target" in extra:                                 # the targets drift, 4 rows
        ni, mi = b.n // p, b.mi
        xf = lqr["xf"]
        dxf = 0.02 * (rng.random((nb, p, ni)) - 0.5)
        if model != DI:
            dxf[:, :, 2:] = 0.0
        sched[TARGET] = np.stack([np.concatenate([(xf + t * dxf).reshape(nb, -1), uf.reshape(nb, -1)], axis=1) for t in range(4)])
    amp = np.full(b.n, 0.005); amp[:d * p] = 0.01
    W = amp * (2.0 * rng.random((ROWS, nb, b.n)) - 1.0)
    return b, sched, W, (Q, R)


def stepwise(b, steps, sched, W, QR):
    """The definition, on the Batch API"""
    n, m = b.n, b.m
    b.mpc_totals(reset=True)
    states, controls, stats = [b.get_x0()], [], []
    for t in range(steps):
        if t == 1:
            b.set_options(shift=1, dual_reset=0)
        for kind, a in sched.items():
            r = min(t, a.shape[0] - 1)
            if t > 0 and r == min(t - 1, a.shape[0] - 1):
                continue
            if kind == TARGET:
                w = b.p * b.ni
                b.set_lqr(QR[0], QR[1], a[r][:, :w].reshape(b.B, b.p, b.ni), a[r][:, w:].reshape(b.B, b.p, b.mi))
            else:
                b.set_scenario_data(kind, a[r])
        b.newton_solve_async(init=True, game_id0=GID0 + t * 1000003)
        stats.append(b.get_stats())
        controls.append(b.get_traj()[:, 2 * n:2 * n + m].copy())
        b.mpc_advance()
        x1 = b.get_x0()
        if W is not None:
            x1 = x1 + W[min(t, W.shape[0] - 1)]
            b.set_x0(x1)
        states.append(x1)
    return np.stack(states), np.stack(controls), np.stack(stats)


def fused(b, steps, sched, W):
    for kind, a in sched.items():
        b.mpc_set_schedule(kind, a)
    if W is not None:
        b.mpc_set_schedule(DIST, W)
    b.mpc_totals(reset=True)
    return b.mpc_solve_log(steps, GID0)


def final(b):
    lam, mu = b.get_con_duals()
    return (b.get_traj(), lam, mu) + b.mpc_totals()


_RUNS = {}


def runs(alg, name):
    """both loops of one shape, run once per session"""
    if name not in _RUNS:
        bf, sched, W, QR = build(alg, name)
        bs = build(alg, name)[0]
        assert bf.get_waves_per_game() == bs.get_waves_per_game() and bf.get_scenario_kernels() == bs.get_scenario_kernels()
        rf = fused(bf, STEPS, sched, W)
        guards = bf.lib.debug_check_guards(bf.h)
        rs = stepwise(bs, STEPS, sched, W, QR)
        _RUNS[name] = dict(bf=bf, bs=bs, fused=rf, step=rs, final_f=final(bf), final_s=final(bs), guards=guards, W=W, sched=sched)
    return _RUNS[name]


def assert_stats_equal(a, b, what):
    for f in COUNTS:
        assert np.array_equal(a[f], b[f]), (what, f, a[f], b[f])
    for f in LAST:
        assert np.array_equal(a["last"][f], b["last"][f], equal_nan=f not in ("outer", "ls_j")), (what, "last." + f, a["last"][f], b["last"][f])


# ---- 1. fused == step-wise, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_logged_disturbed_loop_equals_the_step_wise_loop_bit_for_bit(alg, name):
    r = runs(alg, name)
    model, p, d, nb, waves, extra = SHAPES[name]
    bf = r["bf"]
    if waves:
        assert bf.get_waves_per_game() == waves
    assert bf.get_scenario_kernels()[1] == KERNELS[name]
    (st_f, uc_f, gs_f), (st_s, uc_s, gs_s) = r["fused"], r["step"]
    assert st_f.shape == (STEPS + 1, nb, bf.n) and uc_f.shape == (STEPS, nb, bf.m) and gs_f.shape == (STEPS, nb)
    print("%s: %d wavefronts per game, Newton iterations per solve %d ... %d, converged %d of %d, |u| up to %.3f"
          % (name, bf.get_waves_per_game(), gs_f["newton_iters"].min(), gs_f["newton_iters"].max(), gs_f["converged"].sum(), gs_f["converged"].size,
             np.abs(uc_f).max()))
    print("   fused against step-wise: max |dx| %.3e, max |du| %.3e, games with equal iteration totals %d of %d"
          % (np.abs(st_f - st_s).max(), np.abs(uc_f - uc_s).max(), (r["final_f"][3] == r["final_s"][3]).sum(), nb))
    assert np.array_equal(st_f, st_s, equal_nan=True), np.abs(st_f - st_s).max()
    assert np.array_equal(uc_f, uc_s, equal_nan=True), np.abs(uc_f - uc_s).max()
    assert_stats_equal(gs_f, gs_s, name)
    for a, b_, what in zip(r["final_f"], r["final_s"], ("pdtraj", "lambda", "mu", "newton_iters total", "converged total")):
        assert np.array_equal(a, b_), (name, what)
    assert np.array_equal(r["final_f"][3], gs_f["newton_iters"].sum(axis=0)) and np.array_equal(r["final_f"][4], gs_f["converged"].sum(axis=0))
    assert gs_f["newton_iters"].min() >= 1 and np.abs(uc_f).max() > 1e-3          # every solve iterates, the controls are not trivial


# ---- 2. log-only changes nothing -------------------------------------------------------------------------------------------------------------------
def test_a_log_alone_and_a_zero_disturbance_change_nothing(alg):
    name = "di3_one_wavefront"
    plain, logged, zero = (build(alg, name)[0] for _ in range(3))
    for b in (plain, logged, zero):
        b.mpc_totals(reset=True)
    st_p = plain.mpc_solve(STEPS, GID0, record_states=True)
    st_l, uc_l, gs_l = logged.mpc_solve_log(STEPS, GID0)
    zero.mpc_set_schedule(DIST, np.zeros((2, zero.B, zero.n)))
    st_z, uc_z, gs_z = zero.mpc_solve_log(STEPS, GID0)
    for st, b in ((st_l, logged), (st_z, zero)):
        assert np.array_equal(st, st_p)
        for a, c in zip(final(b), final(plain)):
            assert np.array_equal(a, c)
    assert np.array_equal(uc_l, uc_z)
    assert_stats_equal(gs_l, gs_z, "zero disturbance")
    # the last row of the stats log is what alg_get_stats returns after the call, t_elap included
    for b, gs in ((logged, gs_l), (zero, gs_z)):
        assert gs[STEPS - 1].tobytes() == b.get_stats().tobytes()
    # parts of the log: each output alone gives the same numbers
    part = build(alg, name)[0]
    st_o, uc_o, gs_o = part.mpc_solve_log(STEPS, GID0, states=False, controls=True, stats=False)
    assert st_o is None and gs_o is None and np.array_equal(uc_o, uc_l)
    assert logged.lib.debug_check_guards(logged.h) == 0 and part.lib.debug_check_guards(part.h) == 0


# ---- 3. the logged control is the applied one ------------------------------------------------------------------------------------------------------
def test_the_logged_control_is_the_one_the_advance_applied(alg):
    """Double integrator, independent of the solver: x+ = [q + dt v + dt^2 / 2 u, v + dt u] is what every two-stage Runge-Kutta rule gives for
    this model with the control held, so states[t+1] - w_t must meet it to rounding: entries are O(1), a handful of operations each, so
    1e-13 (the numpy expression is not the device's fma sequence)."""
    r = runs(alg, "di3_one_wavefront")
    st, uc, _ = r["fused"]
    W, p, d, dt = r["W"], 3, 2, HS.DT
    worst = 0.0
    for t in range(STEPS):
        x, u = st[t], uc[t].reshape(-1, p, d)                        # u player-major; x entry = player + component * p
        q, v = x[:, :d * p].reshape(-1, d, p), x[:, d * p:].reshape(-1, d, p)
        a = u.transpose(0, 2, 1)
        nxt = np.concatenate([(q + dt * v + 0.5 * dt * dt * a).reshape(-1, d * p), (v + dt * a).reshape(-1, d * p)], axis=1)
        worst = max(worst, np.abs(st[t + 1] - W[min(t, ROWS - 1)] - nxt).max())
    print("numpy RK2 under the logged controls against the logged states: %.3e" % worst)
    assert worst <= 1e-13, worst


# ---- 4. the disturbance bites ----------------------------------------------------------------------------------------------------------------------
def test_the_disturbance_bites(alg):
    r = runs(alg, "di3_one_wavefront")
    quiet = build(alg, "di3_one_wavefront")[0]
    quiet.mpc_totals(reset=True)
    st_q = quiet.mpc_solve(STEPS, GID0, record_states=True)
    it_q = quiet.mpc_totals()[0]
    moved = np.abs(r["fused"][0] - st_q).max()
    print("disturbed against undisturbed states: %.3e; iteration totals %s against %s" % (moved, r["final_f"][3], it_q))
    assert moved >= 0.5 * 0.01, moved
    assert np.array_equal(r["fused"][0][0], st_q[0])                  # the same start
    assert np.any(r["final_f"][3] != it_q)


# ---- 5. lock-step against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCH.FAMILIES)
def test_logged_disturbed_loop_lock_step_against_the_oracle(alg, orc, name):
    """The five families and the disturbance of tests/test_mpc_disturbed_family.py, 8 games x 6 steps in one launch against the oracle's own
    closed loop: counts identical, states and controls within 1e-8 (relative to the largest entry), the last record's statistics within
    rtol 1e-6 / atol 1e-9 -- the rules of test_gpu_fuzz._compare_solve, the arbiter rule included (|hip - x| <= 4 |oracle - x| + tol), which
    the CPU preconditions say is not needed."""
    fam = SCH.Family(name)
    W = DF.disturbance(fam)
    g = fam.device(alg)
    g.mpc_set_schedule(DIST, W)
    st, uc, gs = g.mpc_solve_log(fam.steps, game_id0=SCH.GID0)
    assert g.lib.debug_check_guards(g.h) == 0
    o = DF.oracle_loop(fam, orc)
    for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
        assert np.array_equal(gs[f], o["stats"][f]), (name, f, gs[f], o["stats"][f])
    consulted, tol = False, 1e-8
    x = None
    worst = {}
    for what, a, b_ in (("states", st, o["states"]), ("controls", uc, o["controls"])):
        scale = max(1.0, np.abs(b_).max())
        err = np.abs(a - b_).max()
        worst[what] = err
        if err > tol * scale:
            consulted = True
            x = DF.oracle_loop(fam, orc, "x")
            eg, eo = np.abs(a - x[what]).max(), np.abs(b_ - x[what]).max()
            print("arbiter consulted:", name, what, "|hip-orc| %.2e |hip-x| %.2e |orc-x| %.2e" % (err, eg, eo))
            assert eg <= 4.0 * eo + tol * scale, (name, what, err, eg, eo)
    for f in ("res", "dyn_vio", "con_vio", "sta_vio", "opt_vio"):
        a, b_ = gs["last"][f], o["stats"]["last"][f]
        if not np.allclose(a, b_, rtol=1e-6, atol=1e-9):
            consulted = True
            x = DF.oracle_loop(fam, orc, "x") if x is None else x
            c = x["stats"]["last"][f]
            assert np.all(np.abs(a - c) <= 4.0 * np.abs(b_ - c) + 1e-6 * np.abs(c) + 1e-9), (name, f, a, b_, c)
    print("%s: %d solves, Newton iterations %d ... %d, worst |hip - oracle| states %.3e controls %.3e, arbiter consulted: %s"
          % (name, gs.size, gs["newton_iters"].min(), gs["newton_iters"].max(), worst["states"], worst["controls"], consulted))
    assert g.mpc_get_schedule(DIST) == DF.ROWS_W


# ---- 6. shards reproduce the whole batch -----------------------------------------------------------------------------------------------------------
def test_shards_reproduce_the_whole_batch(alg):
    ids, sigma = np.arange(6), 0.004

    def run(sub, fused_=True):
        prob, W = alg.scenarios.c5_disturbed(sub, STEPS, sigma, N=N)
        prob.opts.outer_iter, prob.opts.inner_iter, prob.opts.reg_0 = 7, 20, 1e-5
        prob.batch.set_waves_per_game(1)
        out = alg.mpc_rollout(prob, STEPS, disturbance=W[:ROWS], fused=fused_)
        assert prob.batch.mpc_get_schedule(DIST) == 0                 # mpc_rollout drops what it uploaded
        return out, prob, W
    whole, prob, W = run(ids)
    assert np.array_equal(W[:, 3:], alg.scenarios.c5_disturbed(ids[3:], STEPS, sigma, N=N)[1])
    lo, hi = run(ids[:3])[0], run(ids[3:])[0]
    for f in ("states", "controls"):
        assert np.array_equal(getattr(whole, f), np.concatenate([getattr(lo, f), getattr(hi, f)], axis=1)), f
    assert_stats_equal(whole.stats, np.concatenate([lo.stats, hi.stats], axis=1), "shards")
    assert np.array_equal(whole.newton_iters, np.concatenate([lo.newton_iters, hi.newton_iters]))
    assert np.array_equal(whole.converged, np.concatenate([lo.converged, hi.converged]))
    # ... and host.mpc_rollout's own step-wise path is the same loop
    sw = run(ids, fused_=False)[0]
    assert np.array_equal(whole.states, sw.states) and np.array_equal(whole.controls, sw.controls)
    assert_stats_equal(whole.stats, sw.stats, "mpc_rollout step-wise")
    assert np.array_equal(whole.newton_iters, sw.newton_iters) and np.array_equal(whole.converged, sw.converged)
    assert np.abs(whole.states[-1] - whole.states[0]).max() > 0.1     # the vehicles travel


# ---- 7. errors; what drops the disturbance ------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_as_it_was_and_what_drops_the_disturbance(alg):
    name, D, E = "di3_one_wavefront", alg._abi._D, alg._abi.ALG_ERR_ARG
    ref = build(alg, name)[0]
    before = ref.mpc_solve(3, GID0, record_states=True)
    g = build(alg, name)[0]
    w = np.full((2, g.B, g.n), 0.01)
    assert g.lib.mpc_set_schedule(g.h, 101, 0, w.ctypes.data_as(D)) == E                    # rows < 1 with data
    assert g.lib.mpc_set_schedule(g.h, 101, -2, w.ctypes.data_as(D)) == E
    bad = w.copy(); bad[1, 2, 3] = np.nan
    assert g.lib.mpc_set_schedule(g.h, 101, 2, bad.ctypes.data_as(D)) == E                  # a NaN entry, straight at the C ABI
    assert b"row 1" in g.lib.last_error() and b"finite" in g.lib.last_error()
    bad[1, 2, 3] = np.inf
    assert g.lib.mpc_set_schedule(g.h, 101, 2, bad.ctypes.data_as(D)) == E
    assert g.lib.mpc_set_schedule(g.h, 102, 2, w.ctypes.data_as(D)) == E                    # an unknown kind
    rows = alg._abi.C.c_int32(5)
    assert g.lib.mpc_get_schedule(g.h, 102, alg._abi.C.byref(rows)) == E
    with pytest.raises(ValueError, match="finite"):
        g.mpc_set_schedule(DIST, bad)
    with pytest.raises(ValueError, match="expected shape"):
        g.mpc_set_schedule(DIST, np.zeros((2, g.B, g.n + 1)))
    assert g.mpc_get_schedule(DIST) == 0
    assert np.array_equal(g.mpc_solve(3, GID0, record_states=True), before)                 # still the unscheduled loop, the earlier result
    for a, c in zip(final(g), final(ref)):
        assert np.array_equal(a, c)
    # a failed replacement keeps the disturbance that was set
    g.mpc_set_schedule(DIST, w)
    assert g.lib.mpc_set_schedule(g.h, 101, 2, bad.ctypes.data_as(D)) == E and g.mpc_get_schedule(DIST) == 2
    # alg_set_x0, alg_set_lqr and alg_set_scenario_data keep it, data = NULL and any adder drop it
    g.set_x0(np.zeros((g.B, g.n)))
    g.set_lqr(np.full((g.B, 3, 4), 10.0), np.full((g.B, 3, 2), 0.1), np.zeros((g.B, 3, 4)), np.zeros((g.B, 3, 2)))
    g.set_scenario_data(SCH.K_RAD, g.get_scenario_data(SCH.K_RAD))
    assert g.mpc_get_schedule(DIST) == 2
    g.mpc_set_schedule(DIST, None)
    assert g.mpc_get_schedule(DIST) == 0
    g.mpc_set_schedule(DIST, w); g.mpc_set_schedule(TARGET, np.zeros((2, g.B, 18)))
    g.add_collision_avoidance(np.full(3, 0.06))
    assert g.mpc_get_schedule(DIST) == 0 and g.mpc_get_schedule(TARGET) == 0
    assert g.lib.debug_check_guards(g.h) == 0


# ---- 8. guards ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_no_write_outside_the_buffers_after_a_logged_disturbed_loop(alg, name):
    r = runs(alg, name)
    assert r["guards"] == 0
    assert r["bf"].lib.debug_check_guards(r["bf"].h) == 0 and r["bs"].lib.debug_check_guards(r["bs"].h) == 0
