"""The preconditions of tests/test_gpu_log_configs.py as properties of the data, on the CPU and about the references alone (oracle + numpy),
for every configuration of the log kernels (tests/log_config_family.py: 79, none left out).  No GPU needed.

  * the table of lanes: KPT(p) = 64 // p knots per trip, L(p) = KPT p lanes carry items -- cost_lanes_v as written in csrc/algames_cost.hpp;
  * the plan draws of every configuration and horizon meet con_reference.preconditions (margin >= 1e-6, every kind the handle carries with
    rows of both signs) within 50 draws, the second trajectory of the trial buffer as well, and every cost component of the plan reference
    is exercised;
  * the closed-loop run of every configuration, taken on the oracle (step-wise solves joined by the numpy plant, the same schedules row by
    row): states and controls are finite; every indicator margin of con_reference.closed_loop is >= 1e-4, two decades above the 1e-6 the GPU
    test asserts on the device's own states, so that a device-against-oracle difference cannot move a row across a switch; the state and
    control components of the cost are > 0 for every game and player, the collision component for at least one game where the configuration
    carries a collision cost; row 0 and row 1 of every schedule differ.
A configuration that misses a precondition gets another sub-seed in log_config_family.LOOP_SEED / PLAN_SEED; the condition stays."""
import re
import os

import numpy as np
import pytest

import con_reference as KR
import cost_reference as CR
import kkt_reference as K
import log_config_family as LF
from test_kkt_sensitivity_family import _as_product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_list_and_the_table_of_lanes():
    assert len(LF.CONFIGS) == len(set(LF.CONFIGS)) == len(LF.IDS) == 79
    assert [LF.L(p) for p in range(1, 11)] == [64, 64, 63, 64, 60, 60, 63, 64, 63, 60]
    assert [LF.KPT(p) for p in range(1, 11)] == [64, 32, 21, 16, 12, 10, 9, 8, 7, 6]
    src = open(os.path.join(ROOT, "algames.jl_amd", "csrc", "algames_cost.hpp")).read()
    assert re.search(r"cost_lanes_v\s*=\s*\(WAVE\s*/\s*C::P\)\s*\*\s*C::P\s*;", src), "cost_lanes_v is no longer (WAVE / P) P"
    assert len(re.findall(r"KPT\s*=\s*L\s*/\s*P", src)) == 2                       # both cost kernels: knots per trip
    assert LF.plan_horizons((LF.DI, 10, 2, 0)) == [2, 3, 6, 7, 13] and LF.plan_horizons((LF.DI, 1, 2, 0)) == [2, 3, 64, 65, 129]
    assert LF.plan_horizons((LF.DI, 2, 2, 0)) == [2, 3, 32, 33, 65] and LF.plan_horizons((LF.UNI, 3, 2, 0)) == [2, 3, 21, 22, 43]


def test_sources_and_plants_over_the_classes():
    """what the module-level assertion of the helper holds, printed"""
    for cls in sorted({LF.cfg_class(c) for c in LF.CONFIGS}):
        mem = [(i, c) for i, c in enumerate(LF.CONFIGS) if LF.cfg_class(c) == cls]
        print("%-12s %2d configurations, sources %s, plants %s" % (cls, len(mem), sorted({LF.SOURCE[c] for _, c in mem} - {None}),
                                                                   sorted({str(LF.plant_of(i)) for i, _ in mem})))
    # an E = 1 member of every class that has one meets all three sources
    for cls in sorted({LF.cfg_class(c) for c in LF.CONFIGS if c[3] == 1 and c[1] > 1}):
        assert {LF.SOURCE[c] for c in LF.CONFIGS if LF.cfg_class(c) == cls} >= {0, 1, 2}, cls


@pytest.mark.parametrize("cfg", LF.CONFIGS, ids=LF.IDS)
def test_plan_draws_meet_the_preconditions(orc, alg, cfg):
    mdl = LF.model_of(cfg)
    worst = 0
    for N in LF.plan_horizons(cfg):
        _, tw = LF.problem(_as_product(orc), orc, cfg, N)
        assert len(tw) == LF.B
        o = tw[0][0]
        tab = LF.tables_recorded(tw)
        stub = LF.stub_of(o)
        for sub in ((0, 1) if N == LF.KPT(cfg[1]) + 1 else (0,)):
            z, attempts = LF.draw_plan(cfg, N, tab, stub, sub)
            worst = max(worst, attempts)
            vals, scale, margin, kinds = KR.plan(stub, tab, tab["nums"], z, N)
            KR.preconditions(vals, scale, margin, kinds)
            assert vals.shape[0] == LF.B and vals.shape[1] % (N - 1) == 0
        # the plan reference exercises every component the configuration has
        X, U, _ = _sizes(o, N).split_traj(z)
        rad, mu = LF.cost_numbers(tw)
        tot, _ = CR.batch_plan_cost(mdl, LF.DT, X, U, *LF.plan_lqr(tw), rad, mu)
        # (one player in one dimension has a single control entry, and plan_lqr zeroes its weight)
        live = [0] + ([] if (cfg[1], cfg[2]) == (1, 1) else [1]) + ([] if rad is None else [2])
        assert all(tot[..., c].max() > 0.0 for c in live), (cfg, N)
    print(LF.F.cfg_id(cfg), "horizons", LF.plan_horizons(cfg), "most draws for one plan:", worst)


def _sizes(o, N):
    """the part of a Batch split_traj needs, at the oracle handle's sizes"""
    import types
    import algames_jl_amd as A
    s = types.SimpleNamespace(n=o.n, m=o.m, p=o.p, N=N, mi=o.mi, b=o.b)
    s.split_traj = lambda z: A.Batch.split_traj(s, z)
    return s


@pytest.mark.parametrize("cfg", LF.CONFIGS, ids=LF.IDS)
def test_closed_loop_runs_on_the_oracle(orc, alg, cfg):
    i = LF.CONFIGS.index(cfg)
    _, tw = LF.problem(_as_product(orc), orc, cfg, LF.N_LOOP)
    tab = LF.tables_recorded(tw)
    run = LF.Run(cfg, tw, tab)
    assert run.knots >= 2 * LF.KPT(cfg[1]) + 1 and (run.steps - 1) * run.hold < 2 * LF.KPT(cfg[1]) + 1      # the smallest such count
    assert run.source == LF.SOURCE[cfg] and (run.source is None) == (cfg[1] == 1)
    assert (run.tgt is not None) == (i % 2 == 0) and (run.plant is not None) == (i % 2 == 0)
    assert (KR.S_CTL in run.sched) == (cfg[3] == 1) and (len(run.sched) == (2 if cfg[3] == 1 else 0))
    states, controls = run.oracle_loop(orc, _as_product(orc))
    assert states.shape == (run.knots + 1, LF.B, run.n) and controls.shape == (run.knots, LF.B, run.m)
    assert np.isfinite(states).all() and np.isfinite(controls).all()
    vals, scale, margin, kinds = run.con_reference(LF.stub_of(tw[0][0]), tab, states, controls)
    assert margin.min() >= 1e-4, "an indicator argument lies %.2e from its switch" % margin.min()
    ref_s, ref_t, tol_s, tol_t = run.cost_reference(states, controls)
    assert np.all(ref_t[..., :2] > 0.0), "a state or control component is zero"
    if run.rad is not None:
        assert ref_t[..., 2].max() > 0.0, "no game pays a collision cost"
    else:
        assert np.all(ref_t[..., 2] == 0.0)
    for name, rows in [("lqr_target", run.tgt), ("collision_cost", run.cc_rows), ("disturbance", run.W)] + sorted(run.sched.items()):
        if rows is not None:
            assert not np.array_equal(rows[0], rows[1]), name
    # the third trip of the cost kernel sees the second row of every schedule: a loop that read row 0 there would be told apart
    assert (2 * LF.KPT(cfg[1])) // run.hold >= 1
    print("%s: %d steps, hold %d, %d knots, source %s, margin %.2e, |x| <= %.2e, |u| <= %.2e, collision share %.2e"
          % (LF.F.cfg_id(cfg), run.steps, run.hold, run.knots, run.source, margin.min(), np.abs(states).max(), np.abs(controls).max(),
             ref_t[..., 2].sum() / ref_t.sum()))
