"""The preconditions of tests/test_gpu_failure_exits.py, on the CPU: the failure family (tests/failure_family.py) fails where it is meant to
fail, exactly -- the oracle (double) and the long-double arbiter agree on every discrete outcome of every game -- and the comparison functions
of the GPU tests pass with the oracle's library in the device's place.

For every (configuration, N, layout) the GPU tests use:
  1. oracle and arbiter agree on status, records, outer_iters, newton_iters, converged and ls_failures of every game;
  2. entry batch: S has status SINGULAR, N has status NAN, both make 2 records and no Newton iteration; H has status OK and at least three
     Newton iterations, and is not amplifying: |oracle - arbiter| <= 2.5e-9 relative to max(1, max |z|), a quarter of the 1e-8 the HIP path
     is held to (the margin of tests/test_horizon_family.py);
  3. entry batch: newton_direction(0.0) gives SINGULAR for S and N (it has no residual test), newton_step(1, 1) SINGULAR and NAN;
  4. late batch: L has status NAN, outer_iters == 2 and at least 4 records; H has status OK and converged == 1;
  5. late batch: at the dual update of outer iteration 1 (the oracle replayed with outer_iter = 1, then dual_penalty_update) no
     control-bound value lies in (-1e-5, 1e-5) -- 1000 x the 1e-8 the trajectories are held to, so the sign of a value, which decides between
     a multiplier of 0 and one of inf, cannot differ between device and oracle;
  6. the bodies of the GPU tests (failure_family.solve_family, stepwise_family, ibr_family, afterwards_family) pass on the oracle.
The loop batch: NAN at the first record of every step on oracle and arbiter, no iteration, nothing converged.

A family that misses one of these is changed (failure_family: the data, ENTRY_SEED), not the conditions."""
import numpy as np
import pytest

import failure_family as FF
import test_gpu_fuzz as FZ
import test_gpu_horizon_shapes as HS

PROBLEMS = FF.solve_problems()
IDS = ["%s%s" % (HS._name(cfg), "-wall" if wall else "") for cfg, wall, _ in PROBLEMS]


def _both(orc, builder, cfg, N, roles, wall, init):
    out = []
    for kind in ("", "x"):
        b = builder(FF.oracle_make(orc, kind), cfg, N, roles, wall=wall)
        out.append((b, FF.solve(b, init)))
    (o, so), (x, sx) = out
    for f in FF.COUNTS:
        assert np.array_equal(so[f], sx[f]), (cfg, N, roles, f, so[f], sx[f])
    for game in range(o.B):
        ho, hx = o.get_history(game), x.get_history(game)
        assert len(ho) == len(hx) == so["records"][game], (cfg, N, roles, game)
        for f in ("outer", "ls_j", "alpha"):
            assert np.array_equal(ho[f], hx[f]), (cfg, N, roles, game, f)
    return o, so, x


@pytest.mark.parametrize("cfg,wall,Ns", PROBLEMS, ids=IDS)
def test_entry_batch_fails_exactly(orc, cfg, wall, Ns):
    worst = 0.0
    for N in Ns:
        for roles in FF.ENTRY_LAYOUTS:
            o, so, x = _both(orc, FF.entry, cfg, N, roles, wall, False)
            fl = FF.failing(roles)
            assert so["status"].tolist() == FF.statuses(roles), (cfg, N, roles, so["status"])
            assert np.all(so["records"][fl] == 2) and np.all(so["newton_iters"][fl] == 0), (cfg, N, roles, so["records"], so["newton_iters"])
            assert np.all(so["newton_iters"][~fl] >= 3), (cfg, N, roles, so["newton_iters"])
            zo, zx = o.get_traj(0), x.get_traj(0)
            for game in np.nonzero(~fl)[0]:
                err = np.abs(zo[game] - zx[game]).max() / max(1.0, np.abs(zx[game]).max())
                worst = max(worst, err)
                assert err <= 2.5e-9, (cfg, N, roles, game, err)
            for kind in ("", "x"):
                b = FF.entry(FF.oracle_make(orc, kind), cfg, N, roles, wall=wall)
                _, sd = b.newton_direction(0.0)
                assert sd.tolist() == FF.statuses(roles, FF.DIRECTION_STATUS_OF), (cfg, N, roles, kind, sd)
                assert b.newton_step(1, 1)["status"].tolist() == FF.statuses(roles), (cfg, N, roles, kind)
    print(cfg, "entry batch: worst healthy-game |orc - arbiter| %.2e" % worst)


@pytest.mark.parametrize("cfg,wall,Ns", PROBLEMS, ids=IDS)
def test_late_batch_fails_in_the_second_outer_iteration(orc, cfg, wall, Ns):
    worst, margin = 0.0, np.inf
    for N in Ns:
        for roles in FF.LATE_LAYOUTS:
            o, so, x = _both(orc, FF.late, cfg, N, roles, wall, True)
            fl = FF.failing(roles)
            assert so["status"].tolist() == FF.statuses(roles), (cfg, N, roles, so["status"])
            assert np.all(so["outer_iters"][fl] == 2) and np.all(so["records"][fl] >= 4), (cfg, N, roles, so["outer_iters"], so["records"])
            assert np.all(so["converged"][~fl] == 1), (cfg, N, roles, so["converged"])
            zo, zx = o.get_traj(0), x.get_traj(0)
            for game in np.nonzero(~fl)[0]:
                err = np.abs(zo[game] - zx[game]).max() / max(1.0, np.abs(zx[game]).max())
                worst = max(worst, err)
                assert err <= 2.5e-9, (cfg, N, roles, game, err)
            b = FF.late(FF.oracle_make(orc), cfg, N, roles, wall=wall)
            b.set_options(outer_iter=1)
            FF.solve(b, True)
            v = b.dual_penalty_update()[:, FF.ctl_rows(b)]
            margin = min(margin, np.abs(v).min())
            assert np.abs(v).min() >= 1e-5, (cfg, N, roles, np.abs(v).min())
            assert np.array_equal((v > 0).any(axis=1), fl), (cfg, N, roles, "the games with a violated bound are the L games")
    print(cfg, "late batch: worst healthy-game |orc - arbiter| %.2e, smallest |control-bound value| at the first dual update %.2e" % (worst, margin))


@pytest.mark.parametrize("cfg", sorted({c for c, _ in HS.MPC_CONFIGS}), ids=HS._name)
def test_loop_batch_fails_at_the_first_record_of_every_step(orc, cfg):
    for N in FF.LOOP_HORIZONS:
        tot = []
        for kind in ("", "x"):
            b = FF.loop(FF.oracle_make(orc, kind), cfg, N)
            per_step = []
            b.mpc_totals(reset=True)
            for t in range(FF.LOOP_STEPS):
                if t == 1:
                    b.set_options(shift=1, dual_reset=0)
                st = b.newton_solve(init=True, game_id0=FF.GID0 + t * 1000003)
                b.mpc_advance()
                assert st["status"][FF.LOOP_GAME] == FF.NAN and st["records"][FF.LOOP_GAME] == 2 and st["newton_iters"][FF.LOOP_GAME] == 0, (cfg, N, kind, t, st)
                assert np.all(np.delete(st["status"], FF.LOOP_GAME) == 0), (cfg, N, kind, t, st["status"])
                per_step.append([st[f] for f in FF.COUNTS])
            tot.append((np.array(per_step),) + b.mpc_totals())
        for a, c in zip(*tot):
            assert np.array_equal(a, c), (cfg, N)
        assert tot[0][1][FF.LOOP_GAME] == 0 and tot[0][2][FF.LOOP_GAME] == 0


@pytest.mark.parametrize("cfg,wall,Ns", PROBLEMS, ids=IDS)
def test_the_solve_comparisons_pass_on_the_oracle(alg, orc, cfg, wall, Ns):
    FF.solve_family(FZ._OracleAsHip(alg, orc), orc, cfg, Ns, "oracle in the device's place", wall=wall)


def test_the_other_bodies_pass_on_the_oracle(alg, orc):
    a = FZ._OracleAsHip(alg, orc)
    for cfg in FF.STEP_CONFIGS:
        for N in FF.horizons(cfg):
            FF.stepwise_family(a, orc, cfg, N)
    for cfg in FF.IBR_CONFIGS:
        for N in FF.horizons(cfg):
            FF.ibr_family(a, orc, cfg, N)
    for cfg in sorted({c for c, _, _ in FF.AFTERWARDS}):
        for N in FF.horizons(cfg):
            FF.afterwards_family(a, cfg, N)
