"""The KKT column kernel k_kkt_sens<C> on the GPU over ALL of its configurations, per-game numbers and partial pair tables: the entry points
alg_kkt_solve, alg_kkt_sensitivity and alg_kkt_normal_equations where their code differs per configuration -- the loader's flat loops
(e -> (k, q, i, s, a, j) with C::n, m, P, ni, mi, PD; con_col / con_ctl / pairq; A_entry of every model), the store's slices of C::b, and the
numbers ALG_SCEN_AT takes from the game's EXT block, the base twins' block or the handle.

  a. every configuration of tests/kkt_config_family.py (79: what the library instantiates, tests/test_kkt_config_family.py), N in {2, 3, 5},
     three games, on the random full-magnitude data of the parity tests;
  b. per-game collision cost, pair radii and control bounds, on the EXT kernels (the default after set_scenario_data) and on the base kernels'
     block-reading twins, four games, N in {3, 5}: every game against its own oracle, shuffled batches, sub-ranges, the normal equations.
     Two things the library decides: the spherical form is an extended ingredient, so its handle stays on the EXT kernels when asked for
     the base ones (the planar form reaches that twin), and one dimension has neither kind of kernel -- per-game numbers are refused there;
  c. partial, asymmetric pair tables (test_gpu_parity.PAIR_CASES), N = 5.

The reference is always the oracle's Jacobian and the right-hand side written down on the host (tests/param_reference.py), never the HIP
Jacobian; its own accuracy on every problem used here is held by tests/test_kkt_config_family.py on the CPU.  Bounds: test_gpu_kkt_solve's,
unchanged -- status 0, |X - X_ref| <= 1e-9 max |X_ref| per column, |J X - R| <= 1e-8 max(1, |R|_inf); a column whose right-hand side is
zero is exactly zero; everything said to be equal is equal bit for bit.

Measured on an MI355X (printed per case; worst per class of configurations, kkt_config_family.cfg_class): forward and backward figure of
the USER columns, parameter columns against USER, backward figure of the parameter columns --
    base (9)                7.3e-14  2.0e-13  5.3e-16  5.7e-14        block-reading twins (9)   7.3e-14  2.0e-13  5.3e-16  5.7e-14
    EXT, p <= 4 (13)        7.7e-14  1.3e-13  1.0e-15  8.4e-14        one dimension (4)         1.4e-13  1.7e-13  7.4e-16  5.7e-14
    quadrotor (8)           4.8e-14  5.4e-12  5.6e-14  2.6e-12        d = 3, p = 1, 3, 4 (6)    1.2e-13  1.5e-13  4.5e-16  5.7e-14
    5 and 6 players (10)    4.0e-13  2.5e-12  9.1e-16  4.3e-13        7 to 10 players (20)      7.4e-12  1.9e-11  2.7e-14  7.3e-12
against bounds of 1e-9 (forward, against USER) and 1e-8 (backward); per-game problems and pair tables: 1.4e-15 against USER, 7.9e-14
backward (both on the two quadrotors); the normal equations 0.072 of their bound at worst.  The slowest case, ten bicycles, takes 3.2 s."""
import ctypes

import numpy as np
import pytest

import kkt_config_family as F
import kkt_reference as K
import normal_reference as NR
import param_reference as PR
import test_gpu_horizon_shapes as HS
from test_gpu_kkt_solve import TOL_LIN, TOL_X, _check, _T
from test_gpu_parity import PAIR_CASES

pytestmark = pytest.mark.gpu

ERR_STATE = -3
_D, _I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def _backward(J, X, R):
    return float(np.abs(np.matmul(J, X) - R).max() / max(1.0, np.abs(R).max()))


def _refused(g, code, what):
    """a parameter whose ingredient is not on the handle: ALG_ERR_STATE, out and status untouched"""
    out = np.full((g.B, g._param_len(code), g.S), 7.0); st = np.full(g.B, 9, dtype=np.int32)
    rc = g.lib.kkt_sensitivity(g.h, 0.0, code, 0, None, 0, g.B, 0, 0, out.ctypes.data_as(_D), st.ctypes.data_as(_I))
    assert rc == ERR_STATE, (what, rc)
    assert np.all(out == 7.0) and np.all(st == 9), what


def _param_checks(g, tw, J, param, rng, what, tally, fig):
    """One parameter of a handle against its oracle twin (J: the oracle's Jacobians at reg = 0): the unit columns against USER columns on the
    host-written right-hand side and the backward bound, exact zeros, the lengths, x0 / xf against alg_kkt_solve's kinds, step slices, a game
    sub-range and one random direction.  Returns the unit columns."""
    N, o = g.N, tw[0][0]
    code = PR.PARAMS.index(param)
    R, act = PR.analytic_rhs(tw, param)
    ln = R.shape[2]
    assert g.param_len(param) == g.param_len(code) == ln == PR.param_len(o, param) == g._param_len(code), (what, param)
    X, st = g.kkt_sensitivity(param)
    XU, su = g.kkt_solve(_T(R))
    assert X.shape == XU.shape == (g.B, ln, g.S) and st.shape == (g.B,)
    assert np.all(st == 0) and np.all(su == 0), (what, param, st, su)
    assert np.all(np.isfinite(X)), (what, param)
    same, lin = K.col_err(_T(X), _T(XU)), _backward(J, _T(X), R)
    print(what, param, "against USER %.2e backward %.2e" % (same, lin))
    assert same <= TOL_X, (what, param, same)
    assert lin <= TOL_LIN, (what, param, lin)
    fig[2], fig[3] = max(fig[2], same), max(fig[3], lin)
    dead = ~np.any(R != 0, axis=1)                                       # (B, len): columns with a zero right-hand side
    assert np.all(X[dead] == 0), (what, param)
    tally["nonzero"][param] = tally["nonzero"].get(param, 0) + int((~dead).sum())
    if param in ("collision_radius", "control_bound"):
        r = tally["rows"].setdefault(param, [0, 0])                      # [inactive, active]
        r[0] += act.count(0.0); r[1] += act.count(1.0)
    if param in ("x0", "xf"):
        assert np.array_equal(X, g.kkt_solve(kind=param)[0]), (what, param)
    for s0, ns in {(0, 1), (N - 2, 1)} | ({(1, N - 2)} if N >= 3 else set()):
        Xs, ss = g.kkt_sensitivity(param, steps=(s0, ns))
        assert Xs.shape == (g.B, ln, ns * g.b) and np.all(ss == 0)
        assert np.array_equal(Xs, X[:, :, s0 * g.b:(s0 + ns) * g.b]), (what, param, s0, ns)
    assert np.array_equal(g.kkt_sensitivity(param, games=(1, 2))[0], X[1:3]), (what, param, "games")
    # one random direction against the combination of the unit columns: the statement and the bound of test_directions (reg = 1e-3)
    Xr, sr = g.kkt_sensitivity(param, reg=1e-3)
    V = rng.uniform(-1.0, 1.0, (g.B, 1, ln))
    XV, sv = g.kkt_sensitivity(param, reg=1e-3, dirs=V)
    assert XV.shape == (g.B, 1, g.S) and np.all(sr == 0) and np.all(sv == 0)
    want = np.einsum("bdc,bcs->bds", V, Xr)
    tol = 1e-9 * np.einsum("bdc,bc->bd", np.abs(V), np.abs(Xr).max(axis=2))
    err = np.abs(XV - want).max(axis=2)
    assert np.all(err <= tol), (what, param, "direction", err.max(), tol.min())
    assert np.all(XV[tol == 0] == 0), (what, param, "direction of zero columns")
    return X


def _tally_ok(tally, what):
    """the counting of the existing tests: every carried kind has a non-zero column, pair radii and control bounds see both kinds of rows"""
    assert all(v > 0 for v in tally["nonzero"].values()), (what, tally["nonzero"])
    for k, (off, on) in tally["rows"].items():
        assert off > 0 and on > 0, (what, k, off, on)


# ---- a. every configuration -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", F.CONFIGS, ids=F.IDS)
def test_every_configuration(alg, orc, cfg):
    """USER columns against the numpy solve on the oracle's J (reg = 0 and 1e-3), rhs = -res against alg_newton_direction bit for bit, and every
    parameter the handle carries (_param_checks); a parameter without its ingredient is refused."""
    name = F.cfg_id(cfg)
    tally, fig = dict(nonzero={}, rows={}), [0.0, 0.0, 0.0, 0.0]
    for N in F.HORIZONS:
        g, tw = F.pair_problem(alg, orc, cfg, N)
        assert F.runs_its_kernel(g, cfg), (name, g.desc.model, g.p, g.d, g.get_scenario_kernels())
        assert g.B == F.B == len(tw)
        R = K.user_columns(g.B, g.S, N)
        for reg in K.REGS[::-1]:                                         # (reg = 0 last: its J serves the parameters)
            J = K.jacobians(tw, reg)
            X, st = g.kkt_solve(_T(R), reg=reg)
            assert X.shape == (g.B, K.NCOL, g.S) and st.shape == (g.B,)
            f, l = _check(_T(X), st, J, R, K.solve_ref(J, R), (name, N, reg))
            fig[0], fig[1] = max(fig[0], f), max(fig[1], l)
            res = g.residual(0, reg)[0]
            X, st = g.kkt_solve(-res, reg=reg)
            d, sd = g.newton_direction(reg)
            assert np.all(st == 0) and np.all(sd == 0), (name, N, reg)
            assert np.array_equal(X[:, 0], d), (name, N, reg, "-res against the Newton direction")
        carried = PR.carried(tw[0][0])
        assert carried == (PR.PARAMS if cfg[1] > 1 else PR.PARAMS[:5] + ("control_bound",)), (name, carried)
        rng = np.random.default_rng([N, 5])
        for code, param in enumerate(PR.PARAMS):
            if param in carried:
                _param_checks(g, tw, J, param, rng, (name, N), tally, fig)
            else:
                _refused(g, code, (name, N, param))
        HS._guards_ok(g)
    _tally_ok(tally, name)
    assert set(tally["nonzero"]) == set(carried)
    print("figures", name, "class", F.cfg_class(cfg), "forward %.2e backward %.2e against USER %.2e parameter backward %.2e" % tuple(fig))


# ---- b. per-game numbers -----------------------------------------------------------------------------------------------------------------------------------------
def _normal_columns(g, X, want=12):
    """`want` columns spread over the per-game kinds the handle carries, live ones (a non-zero column in some game) first"""
    order = {}
    for k in F.PER_GAME_KINDS:
        if k in X:
            live = np.any(X[k] != 0, axis=(0, 2))
            order[k] = [(k, int(i)) for i in list(np.flatnonzero(live)) + list(np.flatnonzero(~live))]
    cols = []
    while len(cols) < want:                                              # one of each kind in turn (a kind with few entries runs out first)
        assert any(order.values())
        cols += [order[k].pop(0) for k in order if order[k]][:want - len(cols)]
    assert len({k for k, _ in cols}) == len(order)
    return cols


@pytest.mark.parametrize("case,mode", F.PER_GAME_CASES, ids=F.PER_GAME_IDS)
def test_per_game_numbers(alg, orc, case, mode):
    """Collision cost, pair radii and control bounds differ between the four games: every game's columns against ITS oracle (one
    OracleBatch(B = 1) per game), a shuffled batch gives the shuffled result, a sub-range its rows, and one alg_kkt_normal_equations call over
    twelve columns of the per-game kinds sits inside the derived bound of tests/normal_reference.py."""
    tally, fig = dict(nonzero={}, rows={}), [0.0, 0.0, 0.0, 0.0]
    perm = np.array([2, 0, 3, 1])
    for N in F.PER_GAME_HORIZONS:
        data = F.PerGame(orc, case, N)
        g, tw = data.device(alg, mode), data.twin(orc)
        assert (g.desc.model, g.p, g.d) == case[:3] and g.get_scenario_kernels() == F.per_game_kernels(case, mode), g.get_scenario_kernels()
        assert g.B == len(tw) == 4 and g.con_len == tw[0][0].con_len
        J = K.jacobians(tw, 0.0)
        carried = PR.carried(tw[0][0])
        rng = np.random.default_rng([N, 6])
        X = {}
        for param in ("Q",) + F.PER_GAME_KINDS:
            if param in carried:
                X[param] = _param_checks(g, tw, J, param, rng, (case, mode, N), tally, fig)
            else:
                assert case[0] == K.QUAD and param == "collision_radius"
                _refused(g, PR.PARAMS.index(param), (case, mode, N, param))
        h = data.device(alg, mode, perm)
        for param, Xp in X.items():
            assert np.array_equal(h.kkt_sensitivity(param)[0], Xp[perm]), (case, mode, N, param, "shuffled batch")
            assert np.array_equal(g.kkt_sensitivity(param, games=(2, 2))[0], Xp[2:4]), (case, mode, N, param, "sub-range")
        cols = _normal_columns(g, X)
        z = g.get_traj()[:, g.n:]
        rs = np.random.default_rng([N, 7])
        target, w = z + rs.uniform(-0.5, 0.5, z.shape), rs.uniform(0.0, 2.0, z.shape)
        w[..., ::7] = 0.0
        Hm, gv, loss, st = g.kkt_normal_equations(cols, target, w)
        assert np.all(st == 0), st
        ref = NR.gram(np.stack([X[k][:, i] for k, i in cols], axis=1), z, target, w)
        frac = NR.assert_parity((Hm, gv, loss), ref, (case, mode, N))
        assert np.array_equal(Hm, Hm.transpose(0, 2, 1))
        print((case, mode, N), "normal equations over", sorted({k for k, _ in cols}), "worst error %.3f of the bound" % frac)
        HS._guards_ok(g); HS._guards_ok(h)
    _tally_ok(tally, (case, mode))
    print("figures", (case, mode), "against USER %.2e parameter backward %.2e" % (fig[2], fig[3]))


def test_one_dimension_takes_no_per_game_numbers(alg, orc):
    """Two double integrators in one dimension: the library has neither an EXT kernel nor a block-reading twin for d = 1, so per-game numbers
    are refused in both modes (ALG_ERR_ARG) -- and the handle goes on answering with its shared numbers, bit for bit."""
    N = 5
    data = F.PerGame(orc, F.PER_GAME_REFUSED, N)
    g = data.device(alg, None)
    before = {param: g.kkt_sensitivity(param)[0] for param in F.PER_GAME_KINDS}
    for mode in ("ext", "base"):
        with pytest.raises(alg.AlgamesError, match=r"code -1"):
            data.upload(g, mode)
        assert g.get_scenario_kernels() == (0, 0), (mode, g.get_scenario_kernels())
        for param, X in before.items():
            Xa, st = g.kkt_sensitivity(param)
            assert np.all(st == 0) and np.array_equal(Xa, X), (mode, param)
    HS._guards_ok(g)


# ---- c. partial, asymmetric pair tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stale", [False, True], ids=["fresh", "stale"])
@pytest.mark.parametrize("case", PAIR_CASES, ids=["%s%d_d%d" % (("di", "uni")[c[0]], c[1], c[2]) for c in PAIR_CASES])
def test_partial_pair_tables(alg, orc, case, stale):
    """Collision avoidance on a subset of the ordered pairs, each with its own radius (the spherical case: distance over three position
    entries): the column of a never-added pair and of the diagonal is exactly zero although its rows carry multipliers; an added pair's
    column matches USER on the right-hand side written with that pair's radius.  stale: the handle carried the all-pairs form before, so
    its table holds a radius where no pair exists -- only the pair mask keeps those columns zero (on a fresh handle the radius is 0 too)."""
    N = 5
    g, tw, pairs = F.pair_table_problem(alg, orc, case, N, stale=stale)
    p = g.p
    on = np.zeros((p, p), dtype=bool)
    for i, j, _ in pairs:
        on[i, j] = True
    lam, mu = g.get_con_duals()
    for i in range(p):
        for j in range(p):
            if i != j and not on[i, j]:                                  # the premise: a loader without the mask would write these rows
                q = PR._pairq(p, i, j)
                assert np.any(lam[:, q * (N - 1):(q + 1) * (N - 1)] > 0) and np.all(mu[:, q * (N - 1):(q + 1) * (N - 1)] >= 1), (case[:3], i, j)
    J = K.jacobians(tw, 0.0)
    tally, fig = dict(nonzero={}, rows={}), [0.0, 0.0, 0.0, 0.0]
    X = _param_checks(g, tw, J, "collision_radius", np.random.default_rng([N, 8]), case[:3], tally, fig)
    assert X.shape[1] == p * p
    assert np.all(X[:, ~on.reshape(-1)] == 0), (case[:3], "never-added pairs and the diagonal")
    assert np.all(np.abs(X[:, on.reshape(-1)]).max(axis=(0, 2)) > 0), (case[:3], "added pairs")
    for param in ("collision_cost", "control_bound"):
        _param_checks(g, tw, J, param, np.random.default_rng([N, 9]), case[:3], tally, fig)
    HS._guards_ok(g)
    print("figures", case[:3], "against USER %.2e parameter backward %.2e" % (fig[2], fig[3]))
