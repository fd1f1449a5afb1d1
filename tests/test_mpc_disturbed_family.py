"""The disturbed scenario set and the preconditions of the lock-step test of tests/test_gpu_mpc_log.py, on the CPU.

  * scenarios.c5_disturbed is a pure function of the scenario ids: a shard of the ids gives the same rows;
  * the five families of tests/test_gpu_mpc_schedule.py (8 games x 6 steps, their schedules kept) under a disturbance uniform in +-0.01 on
    the position entries and +-0.005 on the others, 4 rows (held from step 3 on): the closed loop of the oracle (double) and of the
    long-double arbiter -- newton_solve, get_stats, get_traj, mpc_advance, set_x0(x_1 + w_t), per game -- take the same discrete path in every
    game and step, and their states and controls differ by no more than the 2.5e-9 (relative to the largest entry) that
    tests/test_horizon_family.py allows: a quarter of the 1e-8 the HIP path is held to.

The loops are computed once per (family, arithmetic) and shared with the GPU test."""
import numpy as np
import pytest

import test_gpu_mpc_schedule as SCH

COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures")
ROWS_W, SEED_W = 4, 11
_LOOPS = {}


def disturbance(fam):
    """(ROWS_W, B, n): uniform in +-0.01 on the positions (the first d p entries: entry = player + component * p), +-0.005 on the others"""
    n = fam.p * fam.ni
    amp = np.full(n, 0.005)
    amp[:fam.d * fam.p] = 0.01
    return amp * (2.0 * np.random.default_rng(SEED_W).random((ROWS_W, fam.B, n)) - 1.0)


def oracle_loop(fam, orc, kind=""):
    """The disturbed, scheduled closed loop of every game of the family on the oracle (kind "") or the arbiter ("x"): the oracle has no
    per-game entry, so game g at step t runs in a one-game batch built with row t's values that takes over state, warm start and
    multipliers of step t - 1.  Returns dict(states (steps+1, B, n), controls (steps, B, m), stats (steps, B), ls_j / alpha [t][g],
    traj (B, .), lam, mu)."""
    key = (fam.name, kind)
    if key in _LOOPS:
        return _LOOPS[key]
    W = disturbance(fam)
    n = fam.p * fam.ni
    m = fam.p * fam.mi
    out = dict(states=np.zeros((fam.steps + 1, fam.B, n)), controls=np.zeros((fam.steps, fam.B, m)), stats=[[None] * fam.B for _ in range(fam.steps)],
               ls_j=[[None] * fam.B for _ in range(fam.steps)], alpha=[[None] * fam.B for _ in range(fam.steps)], traj=[], lam=[], mu=[])
    for game in range(fam.B):
        z = lam = mu = None
        out["states"][0, game] = fam.x0[game]
        for t in range(fam.steps):
            o = orc.OracleBatch(fam.model, fam.p, fam.N, fam.dt, 1, d=fam.d, kind=kind)
            fam.setup(o, game, t)
            if t > 0:
                o.set_options(shift=1, dual_reset=0)
                o.set_x0(out["states"][t, game][None].copy()); o.set_traj(z); o.set_con_duals(lam, mu)
            o.newton_solve_async(init=True, game_id0=SCH.GID0 + t * 1000003 + game)
            out["stats"][t][game] = o.get_stats()[0]
            h = o.get_history(0)
            out["ls_j"][t][game], out["alpha"][t][game] = h["ls_j"].copy(), h["alpha"].copy()
            out["controls"][t, game] = o.get_traj()[0, 2 * n:2 * n + m]
            o.mpc_advance()
            x1 = o.get_traj()[:, :n] + W[min(t, ROWS_W - 1), game][None]
            o.set_x0(np.ascontiguousarray(x1))
            out["states"][t + 1, game] = x1[0]
            z = o.get_traj()
            lam, mu = o.get_con_duals()
        out["traj"].append(z[0]); out["lam"].append(lam[0]); out["mu"].append(mu[0])
    out["stats"] = np.array([[s for s in row] for row in out["stats"]], dtype=out["stats"][0][0].dtype)
    for f in ("traj", "lam", "mu"):
        out[f] = np.stack(out[f])
    _LOOPS[key] = out
    return out


def test_the_disturbed_set_is_a_pure_function_of_the_scenario_ids(alg, orc):
    ids, steps, sigma = np.arange(40, 48), 9, 0.004
    prob, W = alg.scenarios.c5_disturbed(ids, steps, sigma, backend=orc.lib())
    assert W.shape == (steps, 8, prob.probsize.n) and W.dtype == np.float64 and W.flags["C_CONTIGUOUS"]
    assert np.all(np.isfinite(W)) and np.abs(W).max() <= np.sqrt(3.0) * sigma and np.abs(W).max() > sigma
    assert abs(W.std() / sigma - 1.0) < 0.1 and abs(W.mean()) < 0.2 * sigma
    plain = alg.scenarios.make_problem("C5", ids, backend=orc.lib())
    assert np.array_equal(prob.x0, plain.x0)                            # the C5 set itself
    _, W2 = alg.scenarios.c5_disturbed(ids[3:6], steps, sigma, backend=orc.lib())
    assert np.array_equal(W2, W[:, 3:6])
    _, W3 = alg.scenarios.c5_disturbed(ids, 4, sigma, backend=orc.lib())   # ... and of the step: a shorter loop sees the same first rows
    assert np.array_equal(W3, W[:4])
    assert len(np.unique(W)) == W.size                                  # keyed by id, step and entry: no two draws coincide


@pytest.mark.parametrize("name", SCH.FAMILIES)
def test_disturbed_family_loops_take_one_path_and_do_not_amplify(orc, name):
    """Oracle against arbiter, every game and every step, nothing left out.  Measured (seed 11, amplitudes as stated): see DESIGN.md 3.3 and
    the figures this test prints; worst relative distance over the five families 2.1e-16 (states), 1.9e-15 (controls); 1 ... 41 Newton
    iterations per solve, all 240 solves converged."""
    fam = SCH.Family(name)
    assert ROWS_W < fam.steps                                           # the held row is exercised
    W = disturbance(fam)
    npos = fam.d * fam.p
    assert np.abs(W[..., :npos]).max() <= 0.01 and np.abs(W[..., npos:]).max() <= 0.005 and np.abs(W).max() > 0.009
    o, x = oracle_loop(fam, orc), oracle_loop(fam, orc, "x")
    for f in COUNTS:
        assert np.array_equal(o["stats"][f], x["stats"][f]), (name, f, o["stats"][f], x["stats"][f])
    for t in range(fam.steps):
        for game in range(fam.B):
            assert np.array_equal(o["ls_j"][t][game], x["ls_j"][t][game]) and np.array_equal(o["alpha"][t][game], x["alpha"][t][game]), (name, t, game)
    assert o["stats"]["newton_iters"].min() >= 1                        # every solve iterates
    es = np.abs(o["states"] - x["states"]).max(axis=(0, 2)) / np.maximum(1.0, np.abs(x["states"]).max(axis=(0, 2)))
    ec = np.abs(o["controls"] - x["controls"]).max(axis=(0, 2)) / np.maximum(1.0, np.abs(x["controls"]).max(axis=(0, 2)))
    print("%s: Newton iterations %d ... %d per solve, converged %d of %d, worst |orc - arbiter| states %.2e controls %.2e"
          % (name, o["stats"]["newton_iters"].min(), o["stats"]["newton_iters"].max(), o["stats"]["converged"].sum(), o["stats"]["converged"].size,
             es.max(), ec.max()))
    assert es.max() <= 2.5e-9, (name, es)
    assert ec.max() <= 2.5e-9, (name, ec)
