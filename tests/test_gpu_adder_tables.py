"""The state the constraint adders of the C ABI leave behind -- the four extended-constraint tables (walls, circles, 3-D walls, cylinders)
with their per-player masks, `con_len`, the messages of refused calls -- and the choice of compiled kernel instantiations behind
`alg_set_waves_per_game`, `alg_set_handoff` and the switch to the EXT kernels.  The parity tests reach all of this only through whole
solves; here every test is a handful of adder calls and at most one constraint evaluation (`dual_penalty_update`).

Expected tables restate the documented rules (include/algames_hip.h): a table holds the DISTINCT entries in the order they were first
added, `get_scenario_data` returns them entry by entry (a cylinder: p (3), l, r -- the axis stays handle-wide); constraint values come
from the CPU oracle given the same calls, with the tolerance tests/test_gpu_parity_ext.py uses for them (1e-14 absolute, values O(1))."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DI, UNI = 0, 1
B, N = 2, 4
MAX_ENTRIES = 8                  # ALG_MAX_WALLS = ALG_MAX_CIRCLES
ALG_ERR_ARG = -1
# kind -> (model, p, d, doubles per entry, fields of an entry that get_scenario_data returns)
KINDS = {"wall": (UNI, 3, 2, 6, range(6)), "circle": (UNI, 3, 2, 3, range(3)),
         "wall3d": (DI, 2, 3, 12, range(12)), "cylinder": (DI, 2, 3, 6, (0, 1, 2, 4, 5))}


def _batch(alg, kind):
    model, p, d = KINDS[kind][:3]
    return alg.Batch(alg.hip_lib(), model, p, N, 0.1, B, d=d)


def _entries(kind, count, seed=0):
    """`count` distinct entries of a kind, one per row (entry-major, as the tables keep the 3-D kinds)."""
    e = 0.1 + np.random.default_rng(seed).random((count, KINDS[kind][3]))       # radii (last field of circles and cylinders) positive
    if kind == "cylinder":
        e[:, 3] = np.arange(count) % 3                                            # axis
    return e


def _add(b, kind, rows, player=None):
    """The adder of `kind`: for every player (player None) or for one."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, KINDS[kind][3])
    if kind in ("wall", "circle"):
        args = [np.ascontiguousarray(c) for c in rows.T]
    elif kind == "wall3d":
        args = [np.ascontiguousarray(rows[:, 3 * k:3 * k + 3]) for k in range(4)]
    else:
        args = [np.ascontiguousarray(rows[:, :3]), rows[:, 3].astype(np.int32), np.ascontiguousarray(rows[:, 4]), np.ascontiguousarray(rows[:, 5])]
    name = {"wall": "add_wall_constraint", "circle": "add_circle_constraint", "wall3d": "add_wall3d_constraint", "cylinder": "add_cylinder_constraint"}[kind]
    if player is None:
        getattr(b, name)(*args)
    else:
        getattr(b, name + "_player")(player, *args)


def _model(kind, rows):
    """What get_scenario_data returns after `rows` were added in this order: the distinct entries, first occurrence first."""
    seen = []
    for r in np.asarray(rows, dtype=np.float64):
        if not any(np.array_equal(r, s) for s in seen):
            seen.append(r)
    return len(seen), np.array([s[list(KINDS[kind][4])] for s in seen]).ravel()


def _check_table(b, kind, base_len, rows):
    count, flat = _model(kind, rows)
    assert b.scenario_data_len(kind) == flat.size
    assert np.array_equal(b.get_scenario_data(kind), np.tile(flat, (B, 1)))
    b._refresh_con_len()
    assert b.con_len == base_len + b.p * (N - 1) * count


@pytest.mark.parametrize("kind", list(KINDS))
def test_identical_entries_are_shared(alg, kind):
    b = _batch(alg, kind)
    base = b.con_len
    e = _entries(kind, 3)
    _add(b, kind, [e[0], e[1], e[0]], player=0)            # one entry repeated within the call
    _check_table(b, kind, base, [e[0], e[1]])
    _add(b, kind, [e[1], e[2]], player=1)                  # e[1] shared between the two players
    _check_table(b, kind, base, [e[0], e[1], e[2]])


@pytest.mark.parametrize("kind", ["wall", "circle"])
def test_masks_become_explicit_after_an_all_player_set(alg, orc, kind):
    """Two entries for everybody, then a third for player 0 only: the third constrains nobody else."""
    model, p, d = KINDS[kind][:3]
    g, o = _batch(alg, kind), orc.OracleBatch(model, p, N, 0.1, B, d=d)
    rng = np.random.default_rng(3)
    e = _entries(kind, 3, seed=1)
    x0 = rng.random((B, g.n))
    z = rng.random((B, g.traj_len)); z[:, :g.n] = x0
    base = g.con_len
    for b in (g, o):
        b.set_x0(x0); b.set_lqr(np.ones((p, g.ni)), np.ones((p, g.mi)), np.zeros((p, g.ni)), np.zeros((p, g.mi)))
        _add(b, kind, e[:2])
        _add(b, kind, e[2:], player=0)
        b.set_traj(z)
    assert g.con_len == o.con_len == base + p * (N - 1) * 3
    vg, vo = g.dual_penalty_update(), o.dual_penalty_update()
    fin = np.isfinite(vo)
    print("max |vals - oracle| =", np.abs(vg[fin] - vo[fin]).max())
    assert np.array_equal(np.isfinite(vg), fin) and np.abs(vg[fin] - vo[fin]).max() < 1e-14
    rows = vg[:, base:].reshape(B, p, N - 1, 3)             # (game, player, step, table entry): the kind's block follows the base rows
    assert np.all(rows[:, 1:, :, 2] == 0.0)                 # third entry: players 1 and 2 are not constrained by it


@pytest.mark.parametrize("kind", ["wall", "cylinder"])
def test_a_call_that_does_not_fit_changes_nothing(alg, kind):
    b = _batch(alg, kind)
    e = _entries(kind, MAX_ENTRIES + 2)
    _add(b, kind, e[:5], player=0)
    before = (b.con_len, b.scenario_data_len(kind), b.get_scenario_data(kind))
    with pytest.raises(alg.AlgamesError, match="more distinct entries than the table holds"):
        _add(b, kind, e[4:9], player=1)                     # one shared entry and four new ones: a ninth
    b._refresh_con_len()
    assert (b.con_len, b.scenario_data_len(kind)) == before[:2] and np.array_equal(b.get_scenario_data(kind), before[2])
    _add(b, kind, e[4:8], player=1)                         # ... and the table still takes what fits
    _check_table(b, kind, before[0] - b.p * (N - 1) * 5, e[:8])


@pytest.mark.parametrize("kind", list(KINDS))
def test_an_all_player_set_overwrites_the_table(alg, kind):
    b = _batch(alg, kind)
    base = b.con_len
    e = _entries(kind, 5)
    _add(b, kind, e[:2], player=0)
    _add(b, kind, e[2:3], player=1)
    _check_table(b, kind, base, e[:3])
    _add(b, kind, e[3:])
    _check_table(b, kind, base, e[3:])


def _refused(b, name, *args):
    """The message of a raw ABI call that must be refused with ALG_ERR_ARG."""
    assert getattr(b.lib, name)(b.h, *args) == ALG_ERR_ARG, name
    msg = b.lib.last_error().decode()
    assert msg.startswith("alg_" + name + ":"), msg
    return msg


def test_refused_calls_name_their_entry_point(alg):
    planar, solid = _batch(alg, "wall"), _batch(alg, "wall3d")
    one = np.ones(3)
    d = one.ctypes.data_as(alg._abi._D)
    ax = np.array([3], dtype=np.int32).ctypes.data_as(alg._abi._I)
    fields = {"add_wall_constraint": 6, "add_circle_constraint": 3, "add_wall3d_constraint": 4, "add_cylinder_constraint": 4}
    for name, nf in fields.items():
        b = solid if "3d" in name or "cyl" in name else planar
        _refused(b, name, 1, *[None] * nf)                                       # null arrays with a positive count
        _refused(b, name + "_player", 0, 1, *[None] * nf)
        for player in (-1, b.p):
            assert "bad player index" in _refused(b, name + "_player", player, 0, *[None] * nf)
    # the 3-D adders on a planar model
    for msg in (_refused(planar, "add_wall3d_constraint", 1, d, d, d, d), _refused(planar, "add_wall3d_constraint_player", 0, 1, d, d, d, d),
                _refused(planar, "add_cylinder_constraint", 1, d, ax, d, d), _refused(planar, "add_cylinder_constraint_player", 0, 1, d, ax, d, d),
                _refused(planar, "add_spherical_collision_avoidance", d), _refused(planar, "add_spherical_collision_avoidance_pair", 0, 1, 0.5)):
        assert "three position dimensions" in msg
    assert "axis must be" in _refused(solid, "add_cylinder_constraint", 1, d, ax, d, d)
    assert "axis must be" in _refused(solid, "add_cylinder_constraint_player", 0, 1, d, ax, d, d)
    for b, kinds in ((planar, ("wall", "circle")), (solid, ("wall3d", "cylinder"))):    # none of it reached a table
        assert [b.scenario_data_len(k) for k in kinds] == [0, 0]


def test_kernel_choice_follows_the_compiled_lists(alg):
    uni3 = alg.Batch(alg.hip_lib(), UNI, 3, N, 0.1, B)
    uni3.set_waves_per_game(4)
    with pytest.raises(alg.AlgamesError, match="no team kernel of that width"):
        uni3.set_waves_per_game(2)                          # only the team of four is compiled for three unicycles
    assert uni3.get_waves_per_game() == 4
    uni3.set_handoff(5)
    assert uni3.get_handoff()[0] == 5
    uni2 = alg.Batch(alg.hip_lib(), UNI, 2, N, 0.1, B)
    with pytest.raises(alg.AlgamesError, match="no hand-off kernel pair"):
        uni2.set_handoff(5)
    assert uni2.get_handoff()[0] == 0
    di3 = alg.Batch(alg.hip_lib(), DI, 2, N, 0.1, B, d=3)   # a base configuration with an EXT twin: the first extended adder switches
    base = di3.con_len
    di3.add_state_bound(0, np.ones(di3.n), -np.ones(di3.n))
    assert di3.con_len == base + di3.p * 2 * di3.n * (N - 1) and di3.get_scenario_kernels()[1] == 1
