"""Per-record violation profiles from the fused solve (alg_set_history_profiles): the four .vio vectors of every record of the history.

T1  against the oracle, record by record: the oracle replayed per game with its step-wise entry points (test_history_vio_abi.oracle_replay,
    held on the CPU against the oracle's own history), on the problems of test_gpu_parity.test_violation_profile_parity.
T2  profiles on == profiles off, bit for bit: everything a solve leaves behind, over the horizons of test_gpu_horizon_shapes.
T3  self-consistency on the same runs: per-knot maxima == the record's *_vio, sta[:, 0] == 0, the last row == alg_get_violation_profile, the
    re-pushed final record carries the previous record's rows.
T4  capacity, refusals, invalidation, the caller's stream."""
import numpy as np
import pytest

import test_gpu_horizon_shapes as HS
from test_gpu_horizon_shapes import DI, UNI, BIC, QUAD, DI3, UNI3, UNI4, GID0, hip_family, horizons, _bits, _same_bits, _guards_ok
from test_history_vio_abi import FIELDS, T1_B, T1_CASES, T1_GID0, oracle_replay, t1_problem

pytestmark = pytest.mark.gpu

CAP = 160                       # outer_iter x inner_iter + 1 = 141 records at most with the family's options
RTOL = 4 * 2.3e-16              # tests/test_gpu_boundary.py: fused maxima against the flat row loops


def _close(a, b):
    return np.isclose(a, b, rtol=RTOL, atol=1e-300)


# ---- T1 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,p,N,ext", T1_CASES)
def test_profiles_against_the_oracle_record_by_record(alg, orc, model, p, N, ext):
    g = t1_problem(lambda *a: alg.Batch(alg.hip_lib(), *a), model, p, N, ext)
    make_o = lambda: t1_problem(lambda *a: orc.OracleBatch(*a), model, p, N, ext)
    o = make_o()
    g.set_history_profiles(16)
    assert g.get_history_profiles() == 16
    sg, so = g.newton_solve(init=True, game_id0=T1_GID0), o.newton_solve(init=True, game_id0=T1_GID0)
    for f in ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures"):
        assert np.array_equal(sg[f], so[f]), (f, sg[f], so[f])
    worst = 0.0
    for game in range(T1_B):
        hg, ho = g.get_history(game), o.get_history(game)
        assert len(hg) == len(ho) >= 2
        for f in ("outer", "ls_j", "alpha"):
            assert np.array_equal(hg[f], ho[f]), (game, f, hg[f], ho[f])
        vg, vo = g.get_history_vio(game), oracle_replay(make_o, ho, game)
        for f in FIELDS:
            assert vg[f].shape == vo[f].shape == (len(ho), N - 1 if f in ("dyn", "con") else N), (game, f, vg[f].shape, vo[f].shape)
            for r in range(len(ho)):
                err, bound = np.abs(vg[f][r] - vo[f][r]).max(), 1e-9 * (1 + np.abs(vo[f][r]).max())
                worst = max(worst, err / bound)
                assert err <= bound, (game, f, r, err, bound)
    _guards_ok(g)
    print("T1", (model, p, N, ext), "worst error / bound %.2e" % worst)


# ---- T2 + T3 --------------------------------------------------------------------------------------------------------------------------------------------
def _consistency(g, what):
    """T3 on a handle that has just solved with profiles on (MODE-2 pass of alg_get_violation_profile last: it rewrites the step records)"""
    st = g.get_stats()
    n_re = 0
    for game in range(g.B):
        h, v = g.get_history(game), g.get_history_vio(game)
        n = min(len(h), g.get_history_profiles())
        for f in FIELDS:
            assert v[f].shape == (n, g.N - 1 if f in ("dyn", "con") else g.N), (what, game, f, v[f].shape, n)
            for r in range(n):
                if np.all(np.isfinite(v[f][r])) and np.isfinite(h[f + "_vio"][r]):
                    assert _close(v[f][r].max(), h[f + "_vio"][r]), (what, game, f, r, v[f][r].max(), h[f + "_vio"][r])
        assert np.all(v["sta"][:, 0] == 0.0), (what, game)
        if n == len(h) >= 2 and st["status"][game] == 0 and all(h[f + "_vio"][-1] == h[f + "_vio"][-2] for f in FIELDS):
            n_re += 1                                   # the final record is the re-push of the one before it
            for f in FIELDS:
                assert np.array_equal(v[f][-1], v[f][-2]), (what, game, f, "re-push")
    last = g.violation_profile()
    for game in range(g.B):
        h, v = g.get_history(game), g.get_history_vio(game)
        if len(v["dyn"]) == len(h) and st["status"][game] == 0:
            for f in FIELDS:
                ok = _close(v[f][-1], last[f][game])
                assert np.all(ok), (what, game, f, "last row against alg_get_violation_profile", v[f][-1][~ok], last[f][game][~ok])
    return n_re


def _on_off(alg, cfg, N, what, nw=None, prepare=None, **kw):
    off, on = hip_family(alg, *cfg, N, **kw), hip_family(alg, *cfg, N, **kw)
    for h in (off, on):
        if prepare:
            prepare(h)
        if nw is not None:
            h.set_waves_per_game(nw)
            assert h.get_waves_per_game() == nw
    on.set_history_profiles(CAP)
    assert off.get_history_profiles() == 0 and on.get_history_profiles() == CAP
    s0, s1 = off.newton_solve(init=True, game_id0=GID0), on.newton_solve(init=True, game_id0=GID0)
    assert s0["records"].max() <= CAP
    _same_bits(off, on, what)
    assert np.array_equal(off.get_traj(1), on.get_traj(1), equal_nan=True) and np.array_equal(off.get_traj(2), on.get_traj(2), equal_nan=True), what
    assert np.array_equal(off.get_direction_gate(), on.get_direction_gate(), equal_nan=True), what
    assert off.get_history_vio(0)["dyn"].shape == (0, N - 1)
    n_re = _consistency(on, what)
    assert np.array_equal(off.dual_penalty_update(), on.dual_penalty_update(), equal_nan=True), what      # constraint values, then lambda and mu once more
    for x, y in zip(off.get_con_duals(), on.get_con_duals()):
        assert np.array_equal(x, y, equal_nan=True), what
    _guards_ok(on); _guards_ok(off)
    return n_re


@pytest.mark.parametrize("cfg", [DI3, UNI3, UNI4, (DI, 2, 2), (DI, 2, 1)], ids=HS._name)
def test_one_wavefront_on_equals_off(alg, cfg):
    n_re = sum(_on_off(alg, cfg, N, ("w1", cfg, N), nw=1) for N in horizons(*cfg))
    assert n_re > 0                                     # the re-push path was met
    print("one wavefront", cfg, "games whose final record is a re-push:", n_re)


@pytest.mark.parametrize("cfg,nw", [(DI3, 4), (UNI4, 2)], ids=lambda v: HS._name(v) or "w%d" % v)
def test_team_on_equals_off(alg, cfg, nw):
    for N in horizons(*cfg):
        _on_off(alg, cfg, N, ("team", nw, cfg, N), nw=nw)


@pytest.mark.parametrize("cfg,wall", [(DI3, True), ((BIC, 2, 2), False)], ids=lambda v: HS._name(v) or ("wall" if v else "plain"))
def test_ext_on_equals_off(alg, cfg, wall):
    for N in horizons(*cfg):
        _on_off(alg, cfg, N, ("ext", cfg, N), nw=1, wall=wall)


@pytest.mark.parametrize("cfg", [(DI, 5, 2), (DI, 3, 3), (QUAD, 2, 2)], ids=HS._name)
def test_dense_on_equals_off(alg, cfg):
    for N in range(2, 11):
        _on_off(alg, cfg, N, ("dense", cfg, N))


def test_base_scen_on_equals_off(alg):
    def prepare(b):
        b.set_scenario_kernels(HS.BASE)
        for k in (HS.K_RAD, HS.K_COST, HS.K_CTL):
            b.set_scenario_data(k, b.get_scenario_data(k))
        assert b.get_scenario_kernels() == (HS.BASE, 2)
    for N in horizons(*DI3):
        _on_off(alg, DI3, N, ("scen", N), nw=1, prepare=prepare)


@pytest.mark.parametrize("N", [65, 66])
def test_knot_stride_past_one_wavefront(alg, N):
    g = hip_family(alg, *DI3, N)
    g.set_waves_per_game(1)
    g.set_history_profiles(CAP)
    g.newton_solve(init=True, game_id0=GID0)
    _consistency(g, ("stride", N))
    _guards_ok(g)


# ---- T4 -------------------------------------------------------------------------------------------------------------------------------------------------
def _refused(alg, g, fn):
    before = g.get_history_profiles(), g.get_handoff()[0]
    with pytest.raises(alg.AlgamesError, match=r"\(code -1\)"):
        fn()
    assert (g.get_history_profiles(), g.get_handoff()[0]) == before


def test_capacity_drops_the_records_past_it(alg):
    full, cap = hip_family(alg, *DI3, 9), hip_family(alg, *DI3, 9)
    full.set_history_profiles(CAP); cap.set_history_profiles(3)
    sf, sc = full.newton_solve(init=True, game_id0=GID0), cap.newton_solve(init=True, game_id0=GID0)
    assert sf["records"].min() > 3
    _same_bits(full, cap, "capacity 3")
    for game in range(full.B):
        vf, vc = full.get_history_vio(game), cap.get_history_vio(game)
        for f in FIELDS:
            assert len(vf[f]) == sf["records"][game] and len(vc[f]) == 3
            assert np.array_equal(vf[f][:3], vc[f]), (game, f)
        assert len(full.get_history_vio(game, max_records=2)["opt"]) == 2
    _guards_ok(cap); _guards_ok(full)


def test_refusals_leave_the_handle_as_it_was(alg):
    g = hip_family(alg, *DI3, 9)
    g.set_waves_per_game(1)
    _refused(alg, g, lambda: g.set_history_profiles(-1))
    _refused(alg, g, lambda: g.set_history_profiles(2 ** 24))                  # 4 games x 2^24 records x 34 doubles: 18 GB
    g.set_handoff(3)
    _refused(alg, g, lambda: g.set_history_profiles(8))                        # a hand-off budget is set
    g.set_handoff(0)
    g.set_history_profiles(8)
    _refused(alg, g, lambda: g.set_handoff(3))                                 # ... and the other way round
    _refused(alg, g, lambda: g.set_history_profiles(-1))
    _refused(alg, g, lambda: g.set_history_profiles(2 ** 24))
    assert g.get_history_profiles() == 8
    g.newton_solve(init=True, game_id0=GID0)
    assert len(g.get_history_vio(0)["dyn"]) == min(8, len(g.get_history(0)))
    seven = alg.Batch(alg.hip_lib(), DI, 7, 5, 0.1, 2)
    _refused(alg, seven, lambda: seven.set_history_profiles(4))
    assert seven.get_history_profiles() == 0
    seven.set_history_profiles(0)
    _guards_ok(g)


def test_other_entry_points_invalidate_and_zero_frees(alg):
    g, never = hip_family(alg, *DI3, 9), hip_family(alg, *DI3, 9)
    g.set_history_profiles(CAP)
    g.newton_solve(init=True, game_id0=GID0)
    n = len(g.get_history(1))
    assert len(g.get_history_vio(1)["sta"]) == n > 1
    g.kkt_solve(kind="x0", reg=1e-3)                                                  # leaves the history, and the profiles, alone
    assert len(g.get_history_vio(1)["sta"]) == n
    g.newton_step(1, 1)
    assert all(len(v) == 0 for v in g.get_history_vio(1).values())
    g.newton_solve(init=True, game_id0=GID0)
    assert len(g.get_history_vio(1)["sta"]) == n
    g.mpc_solve(2, GID0)
    assert all(len(v) == 0 for v in g.get_history_vio(1).values())
    g.set_history_profiles(0)                                                  # frees the buffer: the handle solves like one that never had it
    assert g.get_history_profiles() == 0
    g2 = hip_family(alg, *DI3, 9)
    g2.set_history_profiles(4); g2.set_history_profiles(0)
    for h in (g2, never):
        h.newton_solve(init=True, game_id0=GID0)
    _same_bits(g2, never, "enabled, then switched off")
    assert all(len(v) == 0 for v in g2.get_history_vio(0).values())
    _guards_ok(g); _guards_ok(g2)


_STREAM_CHILD = """
import torch
torch.cuda.set_device(0)                       # torch's HIP runtime first, as in bench.py
import numpy as np
import algames_jl_amd as alg
import test_gpu_horizon_shapes as HS
cfg, N = HS.UNI3, 10
a, b = HS.hip_family(alg, *cfg, N), HS.hip_family(alg, *cfg, N)
for h in (a, b):
    h.set_history_profiles(160)
a.newton_solve(init=True, game_id0=HS.GID0)
stream = torch.cuda.Stream()
assert stream.cuda_stream != 0
b.set_stream(stream.cuda_stream)
b.newton_solve_async(init=True, game_id0=HS.GID0)
b.synchronize()
HS._same_bits(a, b, "caller's stream")
for game in range(a.B):
    va, vb = a.get_history_vio(game), b.get_history_vio(game)
    assert len(va["dyn"]) == len(a.get_history(game)) > 1
    for f in va:
        assert va[f].shape == vb[f].shape and np.array_equal(va[f], vb[f]), (game, f)
stream.synchronize()
print("STREAM_VIO_OK")
"""


def test_async_solve_on_the_callers_stream_gives_the_same_rows():
    """in a child process of its own, like test_gpu_horizon_shapes.test_solve_on_the_callers_stream: torch's HIP runtime has to come first"""
    import os, subprocess, sys
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "oracle"), tests] + [q for q in [os.environ.get("PYTHONPATH")] if q]))
    r = subprocess.run([sys.executable, "-c", _STREAM_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "STREAM_VIO_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
