"""Per-game scenario data, host side (no GPU): structure extraction and rejection, the packed B x len arrays, the per-player table
mapping, shard slicing, the optional ABI entry points on a backend that lacks them, and the Julia shim's use of them."""
import os
import re

import numpy as np
import pytest

import algames_jl_amd as alg
from algames_jl_amd import host, sharding
from algames_jl_amd._abi import (ALG_SCEN_COLLISION_RADIUS, ALG_SCEN_COLLISION_COST, ALG_SCEN_CONTROL_BOUND, ALG_SCEN_STATE_BOUND,
                                 ALG_SCEN_WALL, ALG_SCEN_CIRCLE, ALG_SCEN_WALL3D, ALG_SCEN_CYLINDER, SIGNATURES, OPTIONAL, CLib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6


def _con(model, radius=0.1, umax=1.0, walls=None, circles=None):
    gc = host.GameConstraintValues(host.ProblemSize(N, model))
    host.add_collision_avoidance(gc, radius)
    u = np.full(model.m, umax); u[0] = np.inf
    host.add_control_bound(gc, u, -np.full(model.m, umax))
    if walls is not None:
        host.add_wall_constraint(gc, walls)
    if circles is not None:
        host.add_circle_constraint(gc, *circles)
    return gc


def test_structure_is_equal_for_different_numbers():
    m = host.UnicycleGame(p=3)
    a = _con(m, 0.1, 1.0, [host.Wall([0, 0], [1, 0], [0, 1])])
    b = _con(m, 0.2, 2.0, [host.Wall([0, 0.1], [1, 0.3], [0, 1])])
    assert host.scenario_structure(a) == host.scenario_structure(b)


@pytest.mark.parametrize("field,make", [
    ("collision avoidance (all pairs)", lambda m: host.GameConstraintValues(host.ProblemSize(N, m))),
    ("control bound +-inf pattern", lambda m: _con(m, umax=np.inf)),
    ("walls", lambda m: _con(m, walls=[host.Wall([0, 0], [1, 0], [0, 1])] * 2)),
    ("circles", lambda m: _con(m, circles=([0.5], [0.5], [0.1]))),
    ("state bound players", lambda m: (lambda gc: (host.add_state_bound(gc, 2, np.ones(m.n), -np.ones(m.n)), gc)[1])(_con(m))),
])
def test_differing_structure_is_rejected_naming_game_and_field(field, make):
    m = host.UnicycleGame(p=3)
    cons = [_con(m), _con(m, 0.3), make(m)]
    with pytest.raises(alg.AlgamesError) as e:
        host.scenario_data(cons)
    assert "game_con[2]" in str(e.value) and field in str(e.value)


def test_packed_arrays_of_a_small_example():
    m = host.DoubleIntegratorGame(p=2, d=2)                       # n = 8, m = 4
    cons = []
    for k in range(2):
        gc = host.GameConstraintValues(host.ProblemSize(N, m))
        host.add_collision_avoidance(gc, [0.1 + k, 0.2])
        host.add_control_bound(gc, np.array([np.inf, 1.0, 2.0, 3.0 + k]), np.array([-1.0, -2.0, -3.0, -4.0]))
        host.add_state_bound(gc, 2, np.full(8, 5.0 + k), -np.full(8, np.inf))
        host.add_circle_constraint(gc, [0.5], [0.25 * k], [0.125])
        cons.append(gc)
    obj = host.GameObjective([np.ones(4)] * 2, [np.ones(2)] * 2, [np.zeros(4)] * 2, [np.zeros(2)] * 2, N, m)
    host.add_collision_cost(obj, [1.0, 1.0], [2.0, 2.0])          # the same for both games: not uploaded
    d = host.scenario_data(cons, obj)
    assert sorted(d) == [ALG_SCEN_COLLISION_RADIUS, ALG_SCEN_CONTROL_BOUND, ALG_SCEN_STATE_BOUND, ALG_SCEN_CIRCLE]
    assert np.array_equal(d[ALG_SCEN_COLLISION_RADIUS], [[0, 0.1 + 0.2, 0.1 + 0.2, 0], [0, 1.1 + 0.2, 1.1 + 0.2, 0]])
    assert np.array_equal(d[ALG_SCEN_CONTROL_BOUND], [[np.inf, 1, 2, 3, -1, -2, -3, -4], [np.inf, 1, 2, 4, -1, -2, -3, -4]])
    sb = d[ALG_SCEN_STATE_BOUND].reshape(2, 2, 2, 8)             # game, max / min, player, n
    assert np.all(sb[:, 0, 0] == np.inf) and np.all(sb[:, 1] == -np.inf)
    assert np.all(sb[0, 0, 1] == 5.0) and np.all(sb[1, 0, 1] == 6.0)
    assert np.array_equal(d[ALG_SCEN_CIRCLE], [[0.5, 0.0, 0.125], [0.5, 0.25, 0.125]])
    # a per-game collision cost (B, p) is packed as radius | mu
    obj2 = host.GameObjective([np.ones(4)] * 2, [np.ones(2)] * 2, [np.zeros(4)] * 2, [np.zeros(2)] * 2, N, m)
    host.add_collision_cost(obj2, [[1.0, 1.5], [1.0, 2.5]], [[2.0, 2.0], [3.0, 2.0]])
    d2 = host.scenario_data(cons, obj2)
    assert np.array_equal(d2[ALG_SCEN_COLLISION_COST], [[1.0, 1.5, 2.0, 2.0], [1.0, 2.5, 3.0, 2.0]])
    # every game equal: nothing to upload
    assert host.scenario_data([cons[0], cons[0]], obj) == {}
    # ... unless every kind is asked for (GameProblem: a shard runs the whole batch's kernels whatever its games' numbers)
    d1 = host.scenario_data([cons[1]], obj, every_kind=True)
    assert sorted(d1) == [ALG_SCEN_COLLISION_RADIUS, ALG_SCEN_COLLISION_COST, ALG_SCEN_CONTROL_BOUND, ALG_SCEN_STATE_BOUND, ALG_SCEN_CIRCLE]
    assert np.array_equal(d1[ALG_SCEN_CIRCLE], [[0.5, 0.25, 0.125]])


def test_active_set_resolves_each_games_constraint_values():
    from algames_jl_amd import active_set

    class P:
        pass
    m = host.DoubleIntegratorGame(p=2, d=2)
    a, b = _con(m, 0.1), _con(m, 0.2)
    prob = P(); prob.game_con, prob.game_cons = a, [a, b]
    assert active_set.game_con_of(prob, 1) is b and active_set.game_con_of(prob, 0) is a
    assert active_set.collision_convals(active_set.game_con_of(prob, 1))[(1, 2)].radius == 0.2 + 0.2
    prob.game_cons = None
    assert active_set.game_con_of(prob, 1) is a


def _pw(x):
    return host.Wall([x, 0.0], [x + 1.0, 0.0], [0.0, 1.0])


def test_per_player_walls_map_onto_game_0s_table():
    m = host.UnicycleGame(p=3)

    def con(w1, w2, w3):
        gc = host.GameConstraintValues(host.ProblemSize(N, m))
        host.add_wall_constraint(gc, 1, [_pw(w1), _pw(w2)])
        host.add_wall_constraint(gc, 3, [_pw(w3)])
        return gc
    # game 0: player 3's wall is player 1's first one -> table [w(0), w(1)], entry 0 shared by players 1 and 3
    d = host.scenario_data([con(0.0, 1.0, 0.0), con(0.5, 1.5, 0.5)])
    assert np.array_equal(d[ALG_SCEN_WALL], [[0, 0, 1, 0, 0, 1, 1, 0, 2, 0, 0, 1], [0.5, 0, 1.5, 0, 0, 1, 1.5, 0, 2.5, 0, 0, 1]])
    # another game gives the shared entry different values for the two players: rejected
    with pytest.raises(alg.AlgamesError, match=r"game_con\[1\].*share entry 0"):
        host.scenario_data([con(0.0, 1.0, 0.0), con(0.5, 1.5, 0.7)])
    # game 0 distinct, game 1 equal: fine (game 1 just has two equal table entries)
    d = host.scenario_data([con(0.0, 1.0, 2.0), con(0.0, 1.0, 0.0)])
    assert d[ALG_SCEN_WALL].shape == (2, 18) and np.array_equal(d[ALG_SCEN_WALL][1, 12:], d[ALG_SCEN_WALL][1, :6])


def test_3d_tables_pack_without_the_cylinder_axis():
    m = host.DoubleIntegratorGame(p=2, d=3)
    cons = []
    for k in range(2):
        gc = host.GameConstraintValues(host.ProblemSize(N, m))
        host.add_wall_constraint(gc, [host.Wall3D([0, 0, k], [1, 0, 0], [0, 1, 0], [0, 0, 1])])
        host.add_wall_constraint(gc, [host.CylinderWall([0.5, 0.5, 0.0], "z", 1.0, 0.1 + k)])
        cons.append(gc)
    d = host.scenario_data(cons)
    assert np.array_equal(d[ALG_SCEN_WALL3D][1], [0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1])
    assert np.array_equal(d[ALG_SCEN_CYLINDER], [[0.5, 0.5, 0.0, 1.0, 0.1], [0.5, 0.5, 0.0, 1.0, 1.1]])
    gc = host.GameConstraintValues(host.ProblemSize(N, m))
    host.add_wall_constraint(gc, [host.Wall3D([0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1])])
    host.add_wall_constraint(gc, [host.CylinderWall([0.5, 0.5, 0.0], "x", 1.0, 0.1)])
    with pytest.raises(alg.AlgamesError, match="cylinders"):
        host.scenario_data([cons[0], gc])


def test_shard_slicing():
    m = host.DoubleIntegratorGame(p=2, d=2)
    cons = [_con(m, 0.1 + 0.01 * k) for k in range(5)]
    assert sharding._slice_con(cons, 2, 4) == cons[2:4]
    assert sharding._slice_con(cons[0], 2, 4) is cons[0]
    obj = host.GameObjective([np.ones(4)] * 2, [np.ones(2)] * 2, [np.zeros(4)] * 2, [np.zeros(2)] * 2, N, m)
    host.add_collision_cost(obj, np.arange(10.0).reshape(5, 2), np.ones((5, 2)))
    o = sharding._slice_obj(obj, 1, 3)
    assert np.array_equal(o.collision_radius, [[2, 3], [4, 5]]) and o.collision_μ.shape == (2, 2)
    assert obj.collision_radius.shape == (5, 2)


def test_scenario_entry_points_are_declared_and_optional():
    for name in ("scenario_data_len", "set_scenario_data", "get_scenario_data"):
        assert name in SIGNATURES and name in OPTIONAL
    hdr = open(os.path.join(ROOT, "include", "algames_hip.h")).read()
    for k, kind in enumerate(("COLLISION_RADIUS", "COLLISION_COST", "CONTROL_BOUND", "STATE_BOUND", "WALL", "CIRCLE", "WALL3D", "CYLINDER")):
        assert re.search(rf"#define ALG_SCEN_{kind}\s+{k}\b", hdr)


def test_the_oracle_loads_and_refuses_per_game_calls(orc):
    lib = orc.lib()
    assert isinstance(lib, CLib) and lib.missing == []
    assert set(lib.absent) == set(OPTIONAL)
    b = orc.OracleBatch(0, 2, N, 0.1, 2)
    b.add_collision_avoidance(0.1)
    with pytest.raises(alg.AlgamesError, match="orc_set_scenario_data"):
        lib.set_scenario_data(b.h, ALG_SCEN_COLLISION_RADIUS, None)
    with pytest.raises(alg.AlgamesError, match="not supported"):
        b.set_scenario_data(ALG_SCEN_COLLISION_RADIUS, np.zeros((2, 4)))
    with pytest.raises(alg.AlgamesError, match="orc_scenario_data_len"):
        b.scenario_data_len(ALG_SCEN_COLLISION_RADIUS)


def test_game_problem_rejects_a_list_of_the_wrong_length():
    m = host.DoubleIntegratorGame(p=2, d=2)
    obj = host.GameObjective([np.ones(4)] * 2, [np.ones(2)] * 2, [np.zeros(4)] * 2, [np.zeros(2)] * 2, N, m)
    x0 = np.zeros((3, m.n))
    with pytest.raises(ValueError, match="2 game_con for a batch of 3"):
        host.GameProblem(N, 0.1, x0, m, host.Options(), obj, [_con(m), _con(m)], backend=object())


def test_julia_shim_checks_structure_and_uploads_per_game_values():
    text = open(os.path.join(ROOT, "algames.jl_amd", "julia", "AlgamesHIP.jl")).read()
    setup = text[text.index("function setup!"):]
    setup = setup[:setup.index("\nend\n")]
    assert "scenario_structure(probs[g])" in setup and "upload_scenarios!(bp)" in setup
    assert re.search(r"ccall\(\(:alg_set_scenario_data, LIB\)", text)
    assert re.search(r"ccall\(\(:alg_scenario_data_len, LIB\)", text)
    up = text[text.index("function upload_scenarios!"):]
    assert "scenario_values(bp, pr, kind" in up[:up.index("\nend\n")]
