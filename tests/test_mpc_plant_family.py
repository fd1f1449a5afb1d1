"""The plant of the fused receding-horizon loop (alg_mpc_set_plant) on the CPU: the numpy plant, the preconditions of the lock-step test of
tests/test_gpu_mpc_plant.py, the host-side validation and the resources of the new kernels.  No GPU needed.

  * the numpy plant: midpoint RK2 and classical RK4 on x' = [v, u] (double integrator) and x' = [v cos th, v sin th, om, a] (unicycle, state
    [x | y | th | v], each block of length p), `substeps` sub-steps of h = dt / substeps; the player-major controls of the trajectory layout
    are permuted to the models' component-major order first.  Anchor: its RK2 step with one sub-step equals the oracle's mpc_advance to
    4 ulp of the largest state entry;
  * the five families of tests/test_gpu_mpc_schedule.py (8 games x 6 solves, their schedules kept) under the disturbance of
    tests/test_mpc_disturbed_family.py indexed by the plant knot q = t * hold + j, for three plants each: the closed loop of the oracle
    (double) and of the long-double arbiter -- OracleBatch solves with set_options(shift=hold, dual_reset=0) joined by the numpy plant -- take
    the same discrete path (counts, ls_j, alpha) in every game and solve, and their states and controls differ by no more than 2.5e-9
    relative: a quarter of the 1e-8 the HIP path is held to.  No game is left out.

The plants: (hold, substeps, integrator) = (2, 1, rk2), (3, 4, rk4) and (N - 1, 2, rk4).  di3d_cylinder_target takes (2, 2, rk2) in place of
the first: at (2, 1, rk2) oracle and arbiter part ways in one of its games (a line search that two arithmetics decide differently), which
would make the GPU test leave that game out; with two sub-steps the family takes one path in every game.

The loops are computed once per (family, plant, arithmetic) and shared with the GPU test."""
import importlib.util
import os

import numpy as np
import pytest

import test_gpu_mpc_schedule as SCH
import test_mpc_disturbed_family as DF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DI, UNI = 0, 1
COUNTS = DF.COUNTS
_LOOPS = {}


def combos(name):
    """the three plants of a family, as (hold, substeps, integrator)"""
    N = SCH.Family(name).N
    first = (2, 2, "rk2") if name == "di3d_cylinder_target" else (2, 1, "rk2")
    return [first, (3, 4, "rk4"), (N - 1, 2, "rk4")]


CASES = [(name, c) for name in SCH.FAMILIES for c in combos(name)]
IDS = ["%s-%d-%d-%s" % ((name,) + c) for name, c in CASES]


# ---- the numpy plant -------------------------------------------------------------------------------------------------------------------------
def component_major(u, p, mi):
    """(B, m) player-major (as stored in the trajectory) -> component-major (the models' joint control vector): entry i + j * p"""
    return u.reshape(-1, p, mi).transpose(0, 2, 1).reshape(-1, p * mi)


def f_cont(model, p, d, x, u):
    """continuous dynamics of the joint state (B, n) under the joint control (B, m), component-major"""
    if model == DI:
        return np.concatenate([x[:, d * p:], u], axis=1)
    if model == UNI:
        th, v = x[:, 2 * p:3 * p], x[:, 3 * p:4 * p]
        return np.concatenate([v * np.cos(th), v * np.sin(th), u[:, :p], u[:, p:]], axis=1)
    raise ValueError(model)


def plant_step(model, p, d, x, u_pm, dt, substeps=1, integrator="rk2"):
    """x (B, n), u_pm (B, m) player-major -> Phi(x, u): `substeps` sub-steps of h = dt / substeps, midpoint RK2 or classical RK4"""
    mi = d if model == DI else 2
    u = component_major(np.asarray(u_pm, dtype=np.float64), p, mi)
    x = np.array(x, dtype=np.float64)
    h = dt / float(substeps)
    f = lambda y: f_cont(model, p, d, y, u)
    for _ in range(substeps):
        if integrator == "rk2":
            x = x + h * f(x + (0.5 * h) * f(x))
        else:
            k1 = f(x); k2 = f(x + (0.5 * h) * k1); k3 = f(x + (0.5 * h) * k2); k4 = f(x + h * k3)
            x = x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


# ---- the closed loop of the oracle under a plant -----------------------------------------------------------------------------------------------
def plant_loop(fam, orc, combo, kind=""):
    """The disturbed, scheduled closed loop of every game of the family under the plant `combo` on the oracle (kind "") or the arbiter ("x"):
    the pattern of test_mpc_disturbed_family.oracle_loop with set_options(shift=hold, dual_reset=0) and the numpy plant between the solves.
    Returns dict(states (steps*hold+1, B, n), controls (steps*hold, B, m), stats (steps, B), ls_j / alpha [t][g])."""
    key = (fam.name, combo, kind)
    if key in _LOOPS:
        return _LOOPS[key]
    r, s, integ = combo
    W = DF.disturbance(fam)
    n, m = fam.p * fam.ni, fam.p * fam.mi
    b = n + m + n * fam.p
    out = dict(states=np.zeros((fam.steps * r + 1, fam.B, n)), controls=np.zeros((fam.steps * r, fam.B, m)), stats=[[None] * fam.B for _ in range(fam.steps)],
               ls_j=[[None] * fam.B for _ in range(fam.steps)], alpha=[[None] * fam.B for _ in range(fam.steps)])
    for game in range(fam.B):
        z = lam = mu = None
        out["states"][0, game] = fam.x0[game]
        for t in range(fam.steps):
            o = orc.OracleBatch(fam.model, fam.p, fam.N, fam.dt, 1, d=fam.d, kind=kind)
            fam.setup(o, game, t)
            if t > 0:
                o.set_options(shift=r, dual_reset=0)
                o.set_x0(out["states"][t * r, game][None].copy()); o.set_traj(z); o.set_con_duals(lam, mu)
            o.newton_solve_async(init=True, game_id0=SCH.GID0 + t * 1000003 + game)
            out["stats"][t][game] = o.get_stats()[0]
            h = o.get_history(0)
            out["ls_j"][t][game], out["alpha"][t][game] = h["ls_j"].copy(), h["alpha"].copy()
            zt = o.get_traj()
            x = out["states"][t * r, game][None].copy()
            for j in range(r):
                q = t * r + j
                u = zt[:, 2 * n + j * b:2 * n + j * b + m]
                out["controls"][q, game] = u[0]
                x = plant_step(fam.model, fam.p, fam.d, x, u, fam.dt, s, integ) + W[min(q, DF.ROWS_W - 1), game][None]
                out["states"][q + 1, game] = x[0]
            o.set_x0(np.ascontiguousarray(x))
            z = o.get_traj()
            lam, mu = o.get_con_duals()
    out["stats"] = np.array([[s_ for s_ in row] for row in out["stats"]], dtype=out["stats"][0][0].dtype)
    _LOOPS[key] = out
    return out


# ---- tests -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model, p, d, N", [(DI, 3, 2, 10), (DI, 2, 3, 8), (DI, 5, 2, 6), (UNI, 3, 2, 8)])
def test_the_numpy_rk2_step_is_the_oracles_mpc_advance(orc, model, p, d, N):
    """The anchor of the numpy plant: one RK2 sub-step of length dt under u_1 against the oracle's mpc_advance, 4 ulp of the largest state entry"""
    rng = np.random.default_rng([3, model, p, d])
    B, dt = 4, 0.1
    o = orc.OracleBatch(model, p, N, dt, B, d=d)
    n, m = o.n, o.m
    z = rng.standard_normal((B, o.traj_len))
    o.set_x0(np.ascontiguousarray(z[:, :n]))
    ni, mi = n // p, m // p
    o.set_lqr(np.ones((B, p, ni)), np.ones((B, p, mi)), np.zeros((B, p, ni)), np.zeros((B, p, mi)))
    o.set_traj(z)
    want = plant_step(model, p, d, z[:, :n], z[:, 2 * n:2 * n + m], dt)
    o.mpc_advance()
    got = o.get_traj()[:, :n]
    err, ulp = np.abs(got - want).max(), np.spacing(np.abs(z[:, :n]).max())
    print("numpy RK2 against the oracle's mpc_advance: %.2e (ulp of the largest entry %.2e)" % (err, ulp))
    assert err <= 4.0 * ulp, (err, ulp)
    # ... and the plant's parts are what they say: sub-steps and RK4 move the unicycle (nonlinear), and RK4 = RK2 on the double integrator
    fine = plant_step(model, p, d, z[:, :n], z[:, 2 * n:2 * n + m], dt, 4, "rk4")
    if model == DI:
        assert np.abs(fine - want).max() <= 64 * ulp
    else:
        assert 1e-7 < np.abs(fine - want).max() < 1e-2


@pytest.mark.parametrize("name, combo", CASES, ids=IDS)
def test_plant_family_loops_take_one_path_and_do_not_amplify(orc, name, combo):
    """Oracle against arbiter, every game and every solve, nothing left out"""
    fam = SCH.Family(name)
    r, s, integ = combo
    assert 1 <= r <= fam.N - 1 and DF.ROWS_W < fam.steps * r
    o, x = plant_loop(fam, orc, combo), plant_loop(fam, orc, combo, "x")
    for f in COUNTS:
        assert np.array_equal(o["stats"][f], x["stats"][f]), (name, combo, f, o["stats"][f], x["stats"][f])
    for t in range(fam.steps):
        for game in range(fam.B):
            assert np.array_equal(o["ls_j"][t][game], x["ls_j"][t][game]) and np.array_equal(o["alpha"][t][game], x["alpha"][t][game]), (name, combo, t, game)
    assert o["stats"]["newton_iters"].min() >= 1                        # every solve iterates
    es = np.abs(o["states"] - x["states"]).max(axis=(0, 2)) / np.maximum(1.0, np.abs(x["states"]).max(axis=(0, 2)))
    ec = np.abs(o["controls"] - x["controls"]).max(axis=(0, 2)) / np.maximum(1.0, np.abs(x["controls"]).max(axis=(0, 2)))
    print("%s %s: Newton iterations %d ... %d per solve, converged %d of %d, worst |orc - arbiter| states %.2e controls %.2e"
          % (name, combo, o["stats"]["newton_iters"].min(), o["stats"]["newton_iters"].max(), o["stats"]["converged"].sum(), o["stats"]["converged"].size,
             es.max(), ec.max()))
    assert es.shape == (fam.B,) and ec.shape == (fam.B,)                # no game is left out
    assert es.max() <= 2.5e-9, (name, combo, es)
    assert ec.max() <= 2.5e-9, (name, combo, ec)


def test_plant_defaults_and_host_side_validation(alg, orc):
    P = alg.Plant
    assert P() == P(1, 1, "rk2") and P().is_default and not P(2).is_default and not P(1, 1, "rk4").is_default
    assert P(1, 1, 1).integrator == "rk4" and P(1, 1, 0) == P()
    assert alg.host.Plant is P and alg.ALG_PLANT_RK2 == 0 and alg.ALG_PLANT_RK4 == 1
    for bad in (dict(hold=0), dict(hold=-1), dict(substeps=0), dict(substeps=257), dict(integrator="rk3"), dict(integrator=2), dict(hold=1.5), dict(substeps=True)):
        with pytest.raises(ValueError, match="Plant:"):
            P(**bad)
    assert P(substeps=256).substeps == 256
    # Plant.from_options: substeps = opts.upsampling, the rest default
    opts = alg.Options()
    assert P.from_options(opts) == P(1, opts.upsampling, "rk2") and opts.upsampling == 2
    opts.upsampling = 5
    assert P.from_options(opts) == P(1, 5, "rk2")
    # the Batch layer refuses what the horizon rules out before any library call (an oracle-backed batch needs no GPU; the oracle has no plant
    # entry points, so a call that got through would say so)
    b = orc.OracleBatch(0, 3, 6, 0.1, 2)
    with pytest.raises(ValueError, match=r"hold must be in 1 \.\.\. N - 1 = 5"):
        b.mpc_set_plant(P(hold=6))
    with pytest.raises(ValueError, match="expected a Plant"):
        b.mpc_set_plant((2, 1, "rk2"))
    for knot in (-1, 5):
        with pytest.raises(ValueError, match=r"knot must be in 0 \.\.\. N - 2 = 4"):
            b.mpc_plant_advance(knot)
    with pytest.raises(alg.AlgamesError, match="no orc_mpc_set_plant"):
        b.mpc_set_plant(P(hold=5))
    with pytest.raises(alg.AlgamesError, match="no orc_mpc_plant_advance"):
        b.mpc_plant_advance(4)
    assert b.mpc_get_plant() == P()                                     # a backend without the entry point runs the loop without a plant

    class Prob:                                       # the part of a GameProblem mpc_rollout / mpc_solve touch before they validate
        batch = b
        opts = alg.Options()
    for f in (alg.mpc_rollout, alg.mpc_solve):
        with pytest.raises(ValueError, match="expected a Plant"):
            f(Prob, 3, plant="rk4")
        with pytest.raises(ValueError, match="hold must be in"):
            f(Prob, 3, plant=P(hold=9))
    Prob.opts.mpc_horizon = 0                          # steps=None takes opts.mpc_horizon
    with pytest.raises(ValueError, match="steps must be >= 1, got 0"):
        alg.mpc_rollout(Prob)


def test_the_header_declares_and_the_library_exports_the_plant_entry_points(alg):
    import ctypes
    import re
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "algames_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+ALG_PLANT_RK2\s+0\b", txt) and re.search(r"#define\s+ALG_PLANT_RK4\s+1\b", txt)
    assert re.search(r"typedef\s+struct\s+alg_mpc_plant\s*\{\s*int32_t\s+hold\s*,\s*substeps\s*,\s*integrator\s*,\s*reserved\s*;\s*\}\s*alg_mpc_plant\s*;", txt)
    assert re.search(r"int\s+alg_mpc_set_plant\s*\(\s*alg_handle\s*\*\s*h\s*,\s*const\s+alg_mpc_plant\s*\*\s*p\s*\)", txt)
    assert re.search(r"int\s+alg_mpc_get_plant\s*\(\s*alg_handle\s*\*\s*h\s*,\s*alg_mpc_plant\s*\*\s*p\s*\)", txt)
    assert re.search(r"int\s+alg_mpc_plant_advance\s*\(\s*alg_handle\s*\*\s*h\s*,\s*int32_t\s+knot\s*\)", txt)
    assert ctypes.sizeof(alg._abi.alg_mpc_plant) == 16
    dll = ctypes.CDLL(alg.HIP_LIB_PATH)              # loads without a GPU; no compute call is made
    lib = alg.hip_lib()
    for name in ("mpc_set_plant", "mpc_get_plant", "mpc_plant_advance"):
        assert hasattr(dll, "alg_" + name) and name in alg._abi.SIGNATURES and name not in lib.absent
    # a null handle is refused before any device call
    assert dll.alg_mpc_set_plant(None, None) == alg._abi.ALG_ERR_ARG
    assert dll.alg_mpc_get_plant(None, None) == alg._abi.ALG_ERR_ARG
    assert dll.alg_mpc_plant_advance(None, 0) == alg._abi.ALG_ERR_ARG


def test_the_plant_kernels_stay_within_registers(alg):
    """k_mpc_plant_advance<C> for every one-wavefront configuration of the library (one per k_mpc_advance<C>): no scratch, no spill, no LDS --
    the RK4 stage vectors are register arrays -- and the loops with per-step phases, which carry the plant phase, keep the conditions of
    tests/test_mpc_schedule_build.py (repeated here for the four-quadrotor loops, whose plant phase holds the largest stage vectors)."""
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    spec = importlib.util.spec_from_file_location("_resources", os.path.join(ROOT, "algames.jl_amd", "_resources.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.kernel_resources(alg.HIP_LIB_PATH)
    adv = sorted(k for k in res if k.startswith("k_mpc_advance<"))
    plant = sorted(k for k in res if k.startswith("k_mpc_plant_advance<"))
    assert len(adv) >= 79 and [k.replace("k_mpc_plant_advance<", "k_mpc_advance<") for k in plant] == adv
    for k in plant:
        v = res[k]
        print("%-52s vgpr %3d sgpr %3d" % (k, v["vgpr"], v["sgpr"]))
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)
    for k in ("k_mpc_loop_sched<Cfg<3, 4, 3, 0, 1> >", "k_mpc_loop_sched<Cfg<3, 4, 3, 0, 4> >", "k_mpc_loop_sched<Cfg<3, 4, 3, 1, 4> >"):
        v, parent = res[k], res[k.replace("k_mpc_loop_sched<", "k_mpc_loop<")]
        assert v["vgpr_spill"] == 0 and (v["scratch"] == 0 or parent["scratch"] > 0) and v["lds"] == parent["lds"], (k, v, parent)
    plant_units = [u for u in ge.HIP_UNITS if u[1] == "algames_plant"]
    assert len(plant_units) == 1 and os.path.exists(os.path.join(ge.CSRC, plant_units[0][0]))
