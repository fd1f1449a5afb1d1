"""The preconditions of tests/test_gpu_horizon_shapes.py, on the CPU: its short-horizon problem family, solved by the oracle (double) and by
the long-double arbiter for every (configuration, horizon) the GPU tests use, is neither trivial nor amplifying.

  * the discrete histories of oracle and arbiter are equal in every game;
  * |oracle - arbiter| <= 2.5e-9 (relative to the largest entry, as the parity rule measures) in every game: a quarter of the 1e-8 the HIP
    path is held to, so the reference alone leaves room;
  * from N = 3 on every horizon has a game with at least two outer iterations and a multiplier above 1e-2;
  * over a configuration's horizons together at least one accepted step backtracked (1 < ls_j < ls_iter) and at least one line search failed;
  * the five-step receding-horizon loops of the family agree between oracle and arbiter: totals equal, states <= 2.5e-8 (a quarter of the
    1e-7 of the loop's parity bound), so the step-to-step warm starts do not amplify.

A family that misses one of these is changed (test_gpu_horizon_shapes.family / TUNED), not the conditions."""
import numpy as np
import pytest

import test_gpu_horizon_shapes as HS

COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures")


@pytest.mark.parametrize("cfg,wall,Ns", HS.family_problems(), ids=lambda v: HS._name(v) or (("wall" if v else "plain") if isinstance(v, bool) else "N"))
def test_family_is_neither_trivial_nor_amplifying(orc, cfg, wall, Ns):
    backtracked = failed = False
    worst = 0.0
    for N in Ns:
        o, x = HS.reference(orc, *cfg, N, wall=wall), HS.reference(orc, *cfg, N, wall=wall, kind="x")
        so, sx = o.newton_solve(), x.newton_solve()
        ls_iter = o.opts.ls_iter
        for f in COUNTS:
            assert np.array_equal(so[f], sx[f]), (cfg, N, f, so[f], sx[f])
        zo, zx = o.get_traj(0), x.get_traj(0)
        for game in range(o.B):
            ho, hx = o.get_history(game), x.get_history(game)
            assert len(ho) == len(hx) == so["records"][game], (cfg, N, game)
            for f in ("outer", "ls_j", "alpha"):
                assert np.array_equal(ho[f], hx[f]), (cfg, N, game, f)
            err = np.abs(zo[game] - zx[game]).max() / max(1.0, np.abs(zx[game]).max())
            worst = max(worst, err)
            assert err <= 2.5e-9, (cfg, N, game, err)
            steps = ho["ls_j"][:-1]                                     # (the last record of a solve follows no line search)
            backtracked |= bool(np.any((steps > 1) & (steps < ls_iter)))
        failed |= bool(so["ls_failures"].sum() > 0)
        if N >= 3:
            lam = o.get_con_duals()[0]
            assert np.any((so["outer_iters"] >= 2) & (lam.max(axis=1) > 1e-2)), (cfg, N, so["outer_iters"], lam.max(axis=1))
    print(cfg, "wall" if wall else "", "worst |orc - arbiter| %.2e" % worst)
    assert backtracked and failed, (cfg, backtracked, failed)


@pytest.mark.parametrize("cfg", sorted({c for c, _ in HS.MPC_CONFIGS}), ids=HS._name)
def test_family_loops_do_not_amplify(orc, cfg):
    worst = 0.0
    for N in HS.MPC_HORIZONS:
        it_o, cv_o, st_o = HS.mpc_reference(orc, cfg, N)
        it_x, cv_x, st_x = HS.mpc_reference(orc, cfg, N, kind="x")
        assert np.array_equal(it_o, it_x) and np.array_equal(cv_o, cv_x), (cfg, N, it_o, it_x, cv_o, cv_x)
        assert it_o.min() >= HS.MPC_STEPS                                # every solve of every loop iterates
        worst = max(worst, np.abs(st_o - st_x).max())
        assert np.abs(st_o - st_x).max() <= 2.5e-8, (cfg, N, np.abs(st_o - st_x).max())
    print(cfg, "loops: worst |orc - arbiter| over the states %.2e" % worst)


def test_horizon_rule_follows_the_chunk_depths():
    """N = 2 ... 18 plus N - 1 in {FT - 1, FT, FT + 1, 2 FT, 2 FT + 1}: every ring depth (4, 6, 8) and every chunk length with both neighbours."""
    for cfg in HS.BASE_CONFIGS:
        Ns, ft = HS.horizons(*cfg), HS.FT(*cfg)
        for depth in (4, 6, 8, ft, 2 * ft):
            assert {depth, depth + 1, depth + 2} <= set(Ns) | ({2 * ft} if depth == 2 * ft else set()), (cfg, depth)
    assert [N for N in HS.horizons(*HS.DI3) if N > 18] == [27, 28] and [N for N in HS.horizons(*HS.UNI3) if N > 18] == [30, 31, 32]
    assert all(set(HS.handoff_horizons(c)) <= set(HS.horizons(*c)) for c in HS.HANDOFF_CONFIGS)
    assert set(HS.MPC_HORIZONS) <= set(range(2, 19))
