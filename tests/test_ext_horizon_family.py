"""The preconditions of tests/test_gpu_ext_horizons.py, on the CPU: its constrained problem family (tests/ext_horizon_family.py), solved by the
oracle (double) and by the long-double arbiter for every (configuration, horizon) the GPU tests use, has its extended rows ACTIVE at the short
and at the long horizons and is not amplifying; and the random step-wise data of the parity tests' _pair is well posed at every horizon.

  * the discrete histories of oracle and arbiter are equal in every game, no game ends with a status other than OK;
  * |oracle - arbiter| <= 2.5e-9 per game, relative to max(1, max |z|): a quarter of the 1e-8 the HIP path is held to (the margin of
    tests/test_horizon_family.py); five-step loops: totals equal, states <= 2.5e-8;
  * at every N >= 3 some game ends with an extended-row multiplier above 1e-2; at N = 2 some game has an extended row with a value > 0 at the
    solution or a multiplier > 0;
  * over a configuration's horizons each kind of extended row it carries (state bound, wall, circle; d = 3: Wall3D, cylinder) reaches a
    multiplier above 1e-2 at some N - 1 <= 5 and at some N - 1 >= 9 (a configuration whose horizons end below that: at its longest horizon);
  * over a configuration's horizons an accepted step backtracked, a line search failed, a game converged and a game did not.

A family that misses one of these is changed (ext_horizon_family: geometry, EXT_TUNED), not the conditions."""
import numpy as np
import pytest

import ext_horizon_family as EF
import test_gpu_horizon_shapes as HS
from kkt_reference import OracleAsProduct

COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures")


@pytest.mark.parametrize("cfg,Ns", EF.solve_problems(), ids=lambda v: EF.name(v) or "N")
def test_ext_family_is_active_and_not_amplifying(orc, cfg, Ns):
    backtracked = failed = False
    converged = set()
    worst = 0.0
    short, long_ = {}, {}
    for N in Ns:
        o, x = EF.reference(orc, cfg, N), EF.reference(orc, cfg, N, kind="x")
        so, sx = o.newton_solve(), x.newton_solve()
        ls_iter = o.opts.ls_iter
        for f in COUNTS:
            assert np.array_equal(so[f], sx[f]), (cfg, N, f, so[f], sx[f])
        assert np.all(so["status"] == 0), (cfg, N, so["status"])
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
        converged |= set(so["converged"].tolist())
        rows = EF.family_rows(o, cfg)
        lam = EF.kind_of(o.get_con_duals()[0], rows)
        top = {k: float(v.max()) for k, v in lam.items()}
        if N >= 3:
            assert max(top.values()) > 1e-2, (cfg, N, top)
        else:
            vals = EF.kind_of(o.kat_evaluate_con(), rows)
            assert any(np.any(v[np.isfinite(v)] > 0) for v in vals.values()) or max(top.values()) > 0, (cfg, N, top)
        for k, v in top.items():
            if N - 1 <= 5:
                short[k] = max(short.get(k, 0.0), v)
            if N - 1 >= min(9, max(Ns) - 1):
                long_[k] = max(long_.get(k, 0.0), v)
    print(cfg, "worst |orc - arbiter| %.2e" % worst, "multipliers, short horizons", short, "long horizons", long_)
    assert set(short) == set(long_) == set(EF.KINDS_3D if cfg[2] == 3 else EF.KINDS_2D)
    assert min(short.values()) > 1e-2 and min(long_.values()) > 1e-2, (cfg, short, long_)
    assert backtracked and failed and converged == {0, 1}, (cfg, backtracked, failed, converged)


@pytest.mark.parametrize("cfg", EF.MPC_EXT, ids=EF.name)
def test_ext_family_loops_do_not_amplify(orc, cfg):
    worst = 0.0
    for N in HS.MPC_HORIZONS:
        it_o, cv_o, st_o = EF.mpc_reference(orc, cfg, N)
        it_x, cv_x, st_x = EF.mpc_reference(orc, cfg, N, kind="x")
        assert np.array_equal(it_o, it_x) and np.array_equal(cv_o, cv_x), (cfg, N, it_o, it_x, cv_o, cv_x)
        assert it_o.min() >= HS.MPC_STEPS                                # every solve of every loop iterates
        worst = max(worst, np.abs(st_o - st_x).max())
        assert np.abs(st_o - st_x).max() <= 2.5e-8, (cfg, N, np.abs(st_o - st_x).max())
    print(cfg, "loops: worst |orc - arbiter| over the states %.2e" % worst)


@pytest.mark.parametrize("cfg", EF.TILE_EXT + EF.DENSE_EXT + EF.DENSE_EXT_P10, ids=EF.name)
def test_random_step_data_is_well_posed_at_every_horizon(orc, cfg):
    """The random full-magnitude data of the step-wise GPU tests (EF.pair, built here on two oracle batches): at every horizon the Newton
    direction exists and solves its linear system, J d + res <= 1e-10 max(1, |res|), some game violates a state constraint, and every kind of
    extended row has a row with a value above and a row with a value below zero somewhere in the batch."""
    worst = 0.0
    for N in EF.step_horizons(cfg):
        a, o, rows = EF.pair(OracleAsProduct(orc), orc, cfg, N)
        assert set(rows) == set(EF.KINDS_3D if cfg[2] == 3 else EF.KINDS_2D)
        for reg in (1e-3, 1e-7 * 2 ** 4):
            d, st = a.newton_direction(reg)
            assert np.all(st == 0), (cfg, N, reg, st)
            res = o.residual()[0]
            for game in range(o.B):
                J = o.residual_jacobian(reg, games=(game, 1))[0]
                lin = np.abs(J @ d[game] + res[game]).max() / max(1.0, np.abs(res[game]).max())
                worst = max(worst, lin)
                assert lin <= 1e-10, (cfg, N, reg, game, lin)
        assert np.any(o.record()["sta_vio"] > 0), (cfg, N)
        for k, v in EF.kind_of(o.kat_evaluate_con(), rows).items():
            v = v[np.isfinite(v)]
            assert np.any(v > 0) and np.any(v < 0), (cfg, N, k)
    print(cfg, "worst |J d + res| / max(1, |res|) %.2e" % worst)
