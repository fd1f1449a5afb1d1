"""The extended constraint set over short and ring-edge horizons.

tests/test_gpu_horizon_shapes.py runs every solver kernel shape where its loops end, but reaches the EXT instantiations with extended rows that
are never active (one far-away wall, or the bicycle model alone): value < 0, multiplier 0, no Gauss-Newton term, and a state-bound term
R::RQ of the step records that is identically zero.  Here the same horizons are run with the extended rows ACTIVE:

  a. the step-wise entry points on random full-magnitude data (the parity tests' _pair, all ingredients on, seed N: every extended row with a
     multiplier of O(1) and a penalty in [1, 3]): the 13 tile EXT instantiations at N = 2 ... 18, the dense E = 1 kinds at N = 2 ... 7, ten
     players at N = 2, 3, 4;
  b. the per-player masks and a collision-avoidance pair subset at N = 2, 3, 5, 7, 9: inert rows report 0 and keep their multiplier;
  c. whole solves of the constrained family of tests/ext_horizon_family.py on one wavefront and on the dense EXT teams;
  d. the fused receding-horizon loop on EXT kernels.

N = 2 makes step 0 the terminal step and K = N - 1 = 1 in every row decode; N - 1 in {3, 4, 5} and {5, 6, 7} sit around the sweeps' prefetch
rings of four and six.  Bounds: those of tests/test_gpu_parity_ext.py / _3d.py / _dense.py and of tests/test_gpu_horizon_shapes.py, unchanged.
The preconditions (rows active at short and long horizons, oracle = arbiter, random data well posed) are held on the CPU by
tests/test_ext_horizon_family.py."""
import numpy as np
import pytest

import ext_horizon_family as EF
import test_gpu_fuzz as FZ  # noqa: F401  (HS._compare goes through it)
import test_gpu_horizon_shapes as HS

pytestmark = pytest.mark.gpu

B = 4
REC = ("res", "dyn_vio", "con_vio", "sta_vio", "opt_vio")
DUAL_OPTS = dict(rho_increase=7.0, rho_max=50.0, lambda_max=1.5, alpha_dual=0.7, alphax_dual=[0.5, 1.0, 1.5, 2.0] + [1.0] * 6)
REGS = (1e-3, 1e-7 * 2 ** 4)


def _residuals(g, o, what, worst):
    for which, reg in ((0, 0.0), (0, 1e-3)):
        rg, ng = g.residual(which, reg); ro, no = o.residual(which, reg)
        worst["residual"] = max(worst.get("residual", 0.0), np.abs(rg - ro).max() / (1 + np.abs(ro).max()))
        assert np.abs(rg - ro).max() <= 1e-12 * (1 + np.abs(ro).max()), (what, which, reg, np.abs(rg - ro).max())
        assert np.allclose(ng, no, rtol=1e-13, atol=0), (what, which, reg)
    zt = np.random.default_rng(9).random((g.B, g.traj_len)); zt[:, :g.n] = g.get_traj()[:, :g.n]
    g.set_traj(zt, 1); o.set_traj(zt, 1)
    rg, ng = g.residual(1, 0.37); ro, no = o.residual(1, 0.37)
    worst["residual"] = max(worst["residual"], np.abs(rg - ro).max() / (1 + np.abs(ro).max()))
    assert np.abs(rg - ro).max() <= 1e-12 * (1 + np.abs(ro).max()), (what, "trial", np.abs(rg - ro).max())
    assert np.allclose(ng, no, rtol=1e-13, atol=0), (what, "trial")


def _directions(g, o, what, worst):
    for reg in REGS:
        dg, sg = g.newton_direction(reg); do, so = o.newton_direction(reg)
        assert np.all(sg == 0) and np.all(so == 0), (what, reg, sg, so)
        err = (np.abs(dg - do) / np.abs(do).max(axis=1, keepdims=True)).max()
        worst["direction"] = max(worst.get("direction", 0.0), err)
        assert err < 1e-9, (what, reg, err)
        res = o.residual()[0]
        for game in range(o.B):
            J = o.residual_jacobian(reg, games=(game, 1))[0]
            lin = np.abs(J @ dg[game] + res[game]).max()
            assert lin <= 1e-8 * max(1.0, np.abs(res).max()), (what, reg, game, lin)
        zd = g.get_traj(2)
        assert np.all(zd[:, :g.n] == 0) and np.array_equal(zd[:, g.n:], dg), (what, reg)


def _dual_update(g, o, what, worst, inert=None):
    """dual_penalty_update with the options of test_dual_penalty_update_and_reset_parity, then reset_con; inert: rows that must report 0 and
    keep the multiplier they were given"""
    lam0 = o.get_con_duals()[0]
    for b in (g, o):
        b.set_options(**DUAL_OPTS)
    vg, vo = g.dual_penalty_update(), o.dual_penalty_update()
    fin = np.isfinite(vo)
    assert np.array_equal(np.isfinite(vg), fin), what
    (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
    worst["dual"] = max(worst.get("dual", 0.0), np.abs(vg[fin] - vo[fin]).max(), np.abs(lg - lo).max())
    assert np.abs(vg[fin] - vo[fin]).max() < 1e-14, (what, np.abs(vg[fin] - vo[fin]).max())
    assert np.abs(lg - lo).max() < 1e-14 and np.array_equal(mg, mo), (what, np.abs(lg - lo).max())
    if inert is not None:
        assert inert.any() and not inert.all()
        for v, l in ((vg, lg), (vo, lo)):
            assert np.all(v[:, inert] == 0.0) and np.array_equal(l[:, inert], lam0[:, inert]), what
    g.reset_con(); o.reset_con()
    (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
    assert np.array_equal(lg, lo) and np.array_equal(mg, mo) and np.all(lg == 0) and np.all(mg == 1.0), what


# ---- a. the step-wise entry points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", EF.TILE_EXT + EF.DENSE_EXT + EF.DENSE_EXT_P10, ids=EF.name)
def test_step_wise_entry_points_over_horizons(alg, orc, cfg):
    worst = {}
    for N in EF.step_horizons(cfg):
        what = (cfg, N)
        g, o, _ = EF.pair(alg, orc, cfg, N, B=B)
        assert g.get_scenario_kernels()[1] == 1
        _residuals(g, o, what, worst)
        a, b = g.record(), o.record()
        for f in REC:
            assert np.allclose(a[f], b[f], rtol=1e-12, atol=1e-15), (what, f, a[f], b[f])
        vg, vo = g.violation_profile(), o.violation_profile()
        for f in ("dyn", "con", "sta", "opt"):
            assert vg[f].shape == vo[f].shape
            worst["profile"] = max(worst.get("profile", 0.0), np.abs(vg[f] - vo[f]).max() / (1 + np.abs(vo[f]).max()))
            assert np.abs(vg[f] - vo[f]).max() <= 1e-9 * (1 + np.abs(vo[f]).max()), (what, f)
            assert np.array_equal(vg[f].max(axis=1), a[f + "_vio"]), (what, f)
        if N <= 10:
            g2, o2, _ = EF.pair(alg, orc, cfg, N, B=2)
            for reg in (0.0, 1e-3 * 3 ** 4):
                Jg, Jo = g2.residual_jacobian(reg), o2.residual_jacobian(reg)
                worst["jacobian"] = max(worst.get("jacobian", 0.0), np.abs(Jg - Jo).max() / np.abs(Jo).max())
                assert np.abs(Jg - Jo).max() <= 1e-12 * np.abs(Jo).max(), (what, reg)
        _directions(g, o, what, worst)
        _dual_update(g, o, what, worst)
        g, o, _ = EF.pair(alg, orc, cfg, N, B=B)
        for l in (1, 2):
            ig, io = g.newton_step(1, l), o.newton_step(1, l)
            for f in ("status", "control_flow", "ls_j", "ls_failed"):
                assert np.array_equal(ig[f], io[f]), (what, l, f, ig[f], io[f])
            assert np.array_equal(ig["alpha"], io["alpha"]), (what, l)
            for f in REC:
                assert np.allclose(ig["rec"][f], io["rec"][f], rtol=1e-9, atol=1e-14), (what, l, f)
            zg, zo = g.get_traj(0), o.get_traj(0)
            worst["step"] = max(worst.get("step", 0.0), np.abs(zg - zo).max() / max(1.0, np.abs(zo).max()))
            assert np.abs(zg - zo).max() <= 1e-9 * max(1.0, np.abs(zo).max()), (what, l)
        HS._guards_ok(g)
    print("step-wise", cfg, "worst differences", {k: "%.2e" % v for k, v in worst.items()})


# ---- b. masks and pair subsets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,cfg", EF.MASK_PROBLEMS, ids=lambda v: EF.name(v) or v)
def test_masks_and_pair_subsets_over_horizons(alg, orc, which, cfg):
    worst = {}
    for N in EF.MASK_HORIZONS:
        what = (which, cfg, N)
        g, o, inert = EF.mask_pair(alg, orc, which, cfg, N, B=B)
        assert g.get_scenario_kernels()[1] == 1
        _residuals(g, o, what, worst)
        _directions(g, o, what, worst)
        _dual_update(g, o, what, worst, inert=inert)
        HS._guards_ok(g)
    print(which, cfg, "worst differences", {k: "%.2e" % v for k, v in worst.items()})


# ---- c. whole solves with the extended rows active --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", EF.SOLVE_CHUNK + EF.SOLVE_SHORT, ids=EF.name)
def test_one_wavefront_ext_solve_over_horizons(alg, orc, cfg):
    """Whole solves of the one-wavefront EXT kernels on the constrained family: HS._compare (discrete history identical, 1e-8, else the arbiter
    rule; mu bit-equal and lambda <= 1e-6 relative on the games the oracle converged)."""
    for N in EF.solve_horizons(cfg):
        g = EF.hip_ext_family(alg, *cfg, N)
        g.set_waves_per_game(1)
        assert g.get_waves_per_game() == 1 and g.get_scenario_kernels()[1] == 1
        HS._note(("ext w1",) + cfg, HS._compare(g, orc, cfg, N, tag=("ext family",), build=EF.build, key=EF.KEY))
        HS._guards_ok(g)
    print("EXT family, one wavefront", cfg, "worst |hip - orc| %.2e" % HS.WORST[("ext w1",) + cfg])


@pytest.mark.parametrize("cfg", EF.TEAM_DENSE, ids=EF.name)
def test_dense_ext_team_solve_over_horizons(alg, orc, cfg):
    """The dense-direction EXT team kernels (four wavefronts per game) on the 3-D constrained family: against the oracle as above, nothing left
    in alg_game_stats.reserved, the same bits from a second solve, and the one-wavefront solve of the same handle with equal discrete counts
    and z <= 1e-8 from the team's (the bounds of test_team_solve_over_horizons)."""
    nw = 4
    for N in EF.solve_horizons(cfg):
        g = EF.hip_ext_family(alg, *cfg, N)
        g.set_waves_per_game(nw)
        assert g.get_waves_per_game() == nw and g.get_scenario_kernels()[1] == 1
        HS._note(("ext team",) + cfg, HS._compare(g, orc, cfg, N, tag=("ext family", "w%d" % nw), build=EF.build, key=EF.KEY))
        assert np.all(g.get_stats()["reserved"] == 0), (cfg, N)
        first = HS._bits(g)
        z_team = first[0]
        g.newton_solve(init=True, game_id0=HS.GID0)
        for i, (x, y) in enumerate(zip(first, HS._bits(g))):
            assert np.array_equal(x, y, equal_nan=True), (cfg, N, "second solve", i)
        g.set_waves_per_game(1)
        s1 = g.newton_solve(init=True, game_id0=HS.GID0)
        so = EF.reference(orc, cfg, N).newton_solve()
        for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
            assert np.array_equal(s1[f], so[f]), (cfg, N, f, s1[f], so[f])
        assert np.abs(g.get_traj() - z_team).max() <= 1e-8, (cfg, N, np.abs(g.get_traj() - z_team).max(axis=1))
        HS._guards_ok(g)
    print("EXT family, dense team of", nw, cfg, "worst |hip - orc| %.2e" % HS.WORST[("ext team",) + cfg])


# ---- d. the fused receding-horizon loop on EXT kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", EF.MPC_EXT, ids=EF.name)
def test_fused_ext_mpc_loop_over_horizons(alg, orc, cfg):
    """Five steps of the fused loop of the EXT kernels on the constrained family, one wavefront per game: against the step-wise launches --
    totals equal, states bit-equal -- and against the oracle's loop -- totals equal, states <= 1e-7."""
    for N in HS.MPC_HORIZONS:
        f, s = EF.hip_ext_family(alg, *cfg, N), EF.hip_ext_family(alg, *cfg, N)
        for h in (f, s):
            h.set_waves_per_game(1)
            assert h.get_waves_per_game() == 1 and h.get_scenario_kernels()[1] == 1
        it_f, cv_f, st_f = HS.mpc_loop(f)
        it_s, cv_s, st_s = HS.mpc_loop(s, fused=False)
        assert np.array_equal(it_f, it_s) and np.array_equal(cv_f, cv_s), (cfg, N, it_f, it_s, cv_f, cv_s)
        assert np.array_equal(st_f, st_s), (cfg, N, np.abs(st_f - st_s).max())
        it_o, cv_o, st_o = EF.mpc_reference(orc, cfg, N)
        assert np.array_equal(it_f, it_o) and np.array_equal(cv_f, cv_o), (cfg, N, it_f, it_o, cv_f, cv_o)
        err = np.abs(st_f - st_o).max()
        HS._note(("ext mpc",) + cfg, err)
        assert st_f.shape == st_o.shape == (HS.MPC_STEPS + 1, f.B, f.n) and err <= 1e-7, (cfg, N, err)
        HS._guards_ok(f)
    print("EXT family, fused loop", cfg, "worst |hip - orc| over the states %.2e" % HS.WORST[("ext mpc",) + cfg])
