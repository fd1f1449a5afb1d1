"""alg_kkt_sensitivity on the GPU: equilibrium sensitivities X = -J^-1 d res / d theta with the right-hand sides built on the device, directional
columns and the device-side step slice.

The reference of a right-hand side is the one written down on the host (tests/param_reference.py; held against central differences of the
oracle's residual by tests/test_param_reference.py on the CPU), evaluated at the oracle twin of the device's iterate; the reference of the
solve is alg_kkt_solve(ALG_KKT_RHS_USER) on that right-hand side and the oracle's Jacobian -- never the HIP Jacobian.  Shapes, horizons and
batch are test_gpu_kkt_solve's: the nine of kkt_reference.SHAPES over K.horizons(name), four games.  Bounds: status 0, |X - X_user| <= 1e-9
max |X_user| per column, |J X - R| <= 1e-8 max(1, |R|_inf); a column whose right-hand side is zero is exactly zero.  The nine shapes are
not the coverage of the kernel's configurations: all 79, per-game numbers and partial pair tables run in tests/test_gpu_kkt_configs.py."""
import ctypes

import numpy as np
import pytest

import kkt_reference as K
import param_reference as PR
import test_gpu_horizon_shapes as HS
from test_gpu_kkt_solve import BIT_SHAPES, TOL_LIN, TOL_X, _hip, _orc, _pair_data, _Prob, _T

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3


def _problems(alg, orc, name, N):
    """(what, device batch, oracle twin at the device's iterate): the solved family game and the random data of the parity tests"""
    g = PR.family_problem(_hip(alg), name, N)
    g.newton_solve(init=True, game_id0=HS.GID0)
    tw = K.twin_of(PR.family_problem(_orc(orc), name, N))
    K.copy_iterate(g, tw)
    yield "family", g, tw
    g, tw = PR.pair_problem(alg, orc, name, N)
    yield "pair", g, tw


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_unit_columns_against_user_columns_and_the_oracle(alg, orc, name):
    """Every parameter, unit columns: equal to alg_kkt_solve(USER) on the analytic right-hand side (1e-9 per column), backward bound against the
    oracle's J, status 0, zero right-hand sides give exactly zero columns; x0 and xf are alg_kkt_solve's own columns bit for bit; a step
    slice is those rows of the full call bit for bit; parameter_sensitivity and its accessors are the matching slices."""
    zero_cols = 0
    for N in K.horizons(name):
        for what, g, tw in _problems(alg, orc, name, N):
            J = K.jacobians(tw, 0.0)
            for code, param in enumerate(PR.PARAMS):
                R, _ = PR.analytic_rhs(tw, param)
                assert g.param_len(param) == g.param_len(code) == R.shape[2] == g._param_len(code)
                X, st = g.kkt_sensitivity(param)
                XU, su = g.kkt_solve(_T(R))
                assert X.shape == XU.shape == (g.B, R.shape[2], g.S) and st.shape == (g.B,)
                assert np.all(st == 0) and np.all(su == 0), (name, N, what, param, st, su)
                assert np.all(np.isfinite(X)), (name, N, what, param)
                same = K.col_err(_T(X), _T(XU))
                lin = np.abs(np.einsum("brc,bcq->brq", J, _T(X)) - R).max() / max(1.0, np.abs(R).max())
                print((name, N, what, param), "against USER %.2e backward %.2e" % (same, lin))
                assert same <= TOL_X, (name, N, what, param, same)
                assert lin <= TOL_LIN, (name, N, what, param, lin)
                dead = ~np.any(R != 0, axis=1)                                   # (B, len): columns with a zero right-hand side
                assert np.all(X[dead] == 0), (name, N, what, param)
                zero_cols += int(dead.sum()) if code >= 5 else 0
                if param in ("x0", "xf"):
                    assert np.array_equal(X, g.kkt_solve(kind=param)[0]), (name, N, what, param)
                if N >= 3:
                    for s0, ns in ((0, 1), (N - 2, 1), (1, N - 2), (0, N - 1)):
                        Xs, ss = g.kkt_sensitivity(param, steps=(s0, ns))
                        assert Xs.shape == (g.B, R.shape[2], ns * g.b) and np.all(ss == 0)
                        assert np.array_equal(Xs, X[:, :, s0 * g.b:(s0 + ns) * g.b]), (name, N, what, param, s0, ns)
            sens = alg.parameter_sensitivity(_Prob(g), "Q", steps=(N - 2, 1), games=(1, 2))
            XQ = g.kkt_sensitivity("Q")[0]
            assert np.array_equal(sens.dz, _T(XQ[1:3, :, (N - 2) * g.b:])) and np.array_equal(sens.dx(N), _T(XQ[1:3])[:, (N - 2) * g.b:(N - 2) * g.b + g.n])
            HS._guards_ok(g)
    assert zero_cols > 0, name             # the diagonal of the pair table, the infinite bound, the rows outside their active set


def test_pair_radii_of_the_spherical_form_use_the_distance_in_three_dimensions(alg, orc):
    """Two double integrators in three dimensions with add_spherical_collision_avoidance (EXT kernels, PD = 3): the pair-radius columns against
    USER columns on the host-written right-hand side, whose distance runs over x, y, z.  The solved games' multipliers are replaced by positive
    ones on both sides so that every row is active and the columns are not zero."""
    for N in (3, 6):
        with PR.recorded():
            g = HS.family(_hip(alg), K.DI, 2, 3, N, spherical=True)
            o = HS.family(_orc(orc), K.DI, 2, 3, N, spherical=True)
        g.newton_solve(init=True, game_id0=HS.GID0)
        lam, mu = g.get_con_duals()
        rng = np.random.default_rng(N)
        g.set_con_duals(lam + rng.uniform(0.1, 1.0, lam.shape), mu)
        tw = K.twin_of(o)
        K.copy_iterate(g, tw)
        J = K.jacobians(tw, 0.0)
        for param in ("collision_radius", "collision_cost", "control_bound"):
            R, _ = PR.analytic_rhs(tw, param)
            X, st = g.kkt_sensitivity(param)
            XU, su = g.kkt_solve(_T(R))
            assert np.all(st == 0) and np.all(su == 0)
            same = K.col_err(_T(X), _T(XU))
            lin = np.abs(np.einsum("brc,bcq->brq", J, _T(X)) - R).max() / max(1.0, np.abs(R).max())
            print(("di2_d3 spherical", N, param), "against USER %.2e backward %.2e" % (same, lin))
            assert same <= TOL_X and lin <= TOL_LIN, (N, param, same, lin)
            if param == "collision_radius":
                assert np.all(np.abs(X[:, [1, 2]]).max(axis=2) > 0) and np.all(X[:, [0, 3]] == 0)     # both ordered pairs live, the diagonal zero
        HS._guards_ok(g)


def test_a_missing_ingredient_is_a_state_error(alg):
    """ALG_ERR_STATE where the parameter's ingredient is not on the handle, with nothing written"""
    b = alg.Batch(alg.hip_lib(), K.DI, 3, 5, K.DT, 2)
    b.set_x0(np.zeros((2, b.n)))
    out = np.full((2, 2 * b.m, b.S), 7.0); st = np.full(2, 9, dtype=np.int32)
    D, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    call = lambda param: b.lib.kkt_sensitivity(b.h, 0.0, param, 0, None, 0, 2, 0, 0, out.ctypes.data_as(D), st.ctypes.data_as(I))
    for param in range(1, 8):
        assert call(param) == ERR_STATE, param
    b.set_lqr(np.ones((3, 4)), np.ones((3, 2)), np.zeros((3, 4)), np.zeros((3, 2)))
    for param in (5, 6, 7):
        assert call(param) == ERR_STATE, param
    assert np.all(out == 7.0) and np.all(st == 9)
    b.init_traj(1)
    for param in range(5):
        assert call(param) == 0 and np.all(st == 0), param
    HS._guards_ok(b)


@pytest.mark.parametrize("name", BIT_SHAPES)
def test_directions(alg, orc, name):
    """dirs = e_c is unit column c bit for bit; a random direction in [-1, 1] is the combination of the unit columns within 1e-9 sum |v_c| max |X_c|;
    also with two forced corrections per column (alg_set_refinement(2, 0.0)), which catches a block the loader left stale after a correction."""
    N = 7
    g, _ = PR.pair_problem(alg, orc, name, N)
    rng = np.random.default_rng([N, 5])
    for forced in (False, True):
        if forced:
            g.set_refinement(max_steps=2, tol=0.0)
        for param in PR.PARAMS:
            ln = g.param_len(param)
            X, st = g.kkt_sensitivity(param, reg=1e-3)
            E = np.broadcast_to(np.eye(ln), (g.B, ln, ln))
            XE, se = g.kkt_sensitivity(param, reg=1e-3, dirs=E)
            assert np.all(st == 0) and np.all(se == 0)
            assert np.array_equal(XE, X), (name, forced, param, "unit directions")
            one, _ = g.kkt_sensitivity(param, reg=1e-3, dirs=E[:, ln - 1])
            assert one.shape == (g.B, 1, g.S) and np.array_equal(one[:, 0], X[:, ln - 1]), (name, forced, param, "one direction")
            V = rng.uniform(-1.0, 1.0, (g.B, 3, ln))
            XV, sv = g.kkt_sensitivity(param, reg=1e-3, dirs=V)
            assert XV.shape == (g.B, 3, g.S) and np.all(sv == 0)
            want = np.einsum("bdc,bcs->bds", V, X)
            tol = 1e-9 * np.einsum("bdc,bc->bd", np.abs(V), np.abs(X).max(axis=2))
            err = np.abs(XV - want).max(axis=2)
            print((name, forced, param), "directions against combinations: %.2e of the bound" % (err / np.where(tol > 0, tol, 1)).max())
            assert np.all(err <= tol), (name, forced, param, err.max())
            assert np.array_equal(g.kkt_sensitivity(param, reg=1e-3, dirs=V[:, 1], steps=(2, 3))[0][:, 0], XV[:, 1, 2 * g.b:5 * g.b])
    HS._guards_ok(g)


@pytest.mark.parametrize("name", BIT_SHAPES)
def test_games_and_calls_are_independent_bit_for_bit(alg, orc, name):
    """A game sub-range equals those rows of the full call; a shuffled batch gives the shuffled result; two calls are identical."""
    N = 7
    g, _ = PR.pair_problem(alg, orc, name, N)
    g.set_refinement(max_steps=2, tol=0.0)
    full = {}
    for param in PR.PARAMS:
        X, st = g.kkt_sensitivity(param, reg=1e-3)
        assert np.all(st == 0)
        assert np.array_equal(g.kkt_sensitivity(param, reg=1e-3)[0], X), (name, param, "two calls")
        assert np.array_equal(g.kkt_sensitivity(param, reg=1e-3, games=(2, 2))[0], X[2:4]), (name, param, "sub-range")
        assert np.array_equal(g.kkt_sensitivity(param, reg=1e-3, games=(1, 1), steps=(3, 2))[0], X[1:2, :, 3 * g.b:5 * g.b]), (name, param, "sub-range of a slice")
        full[param] = X
    if K.SHAPES[name][3] == "base":
        perm = np.array([2, 0, 3, 1])
        h, _ = K.pair_problem(alg, orc, name, N)
        z, (lam, mu) = h.get_traj(), h.get_con_duals()
        h.set_x0(z[perm][:, :h.n]); h.set_lqr(*[v[perm] for v in _pair_data(name, N)])
        h.set_traj(z[perm]); h.set_con_duals(lam[perm], mu[perm])
        h.set_refinement(max_steps=2, tol=0.0)
        for param in PR.PARAMS:
            assert np.array_equal(h.kkt_sensitivity(param, reg=1e-3)[0], full[param][perm]), (name, param, "shuffled batch")
        HS._guards_ok(h)
    HS._guards_ok(g)


@pytest.mark.parametrize("name", ["di3", "uni4", "di5"])
def test_the_call_leaves_the_solver_state_alone(alg, orc, name):
    """Everything test_gpu_horizon_shapes._bits collects is unchanged by the calls, ALG_TRAJ_DELTA holds the last column, ALG_TRAJ_TRIAL keeps
    x_1, and a following newton_solve(init=False) matches, bit for bit, a handle that never made them."""
    N = 7
    a, b = K.family_problem(_hip(alg), name, N), K.family_problem(_hip(alg), name, N)
    for h in (a, b):
        h.newton_solve(init=True, game_id0=HS.GID0)
    before = HS._bits(a)
    x0 = a.get_x0()
    for param in PR.PARAMS:
        X, _ = a.kkt_sensitivity(param, reg=1e-3 if param == "R" else 0.0, steps=(1, 2))
    V = np.random.default_rng(3).uniform(-1.0, 1.0, (3, 2, 2 * a.m))
    X, _ = a.kkt_sensitivity("control_bound", dirs=V, games=(1, 3), steps=(0, 1))
    last = a.kkt_sensitivity("control_bound", dirs=V[:, 1], games=(1, 3))[0][:, 0]
    assert np.array_equal(a.get_traj(2)[1:4, a.n:], last)                   # the delta buffer holds all steps of the last column
    for i, (x, y) in enumerate(zip(before, HS._bits(a))):
        assert np.array_equal(x, y, equal_nan=True), (name, i)
    assert np.array_equal(x0, a.get_x0())
    assert np.array_equal(a.get_traj(1)[:, :a.n], a.get_traj(0)[:, :a.n])   # ALG_TRAJ_TRIAL is scratch with x_1 restored
    for h in (a, b):
        h.newton_solve(init=False, game_id0=HS.GID0)
    HS._same_bits(a, b, (name, "solve after the calls"))
    HS._guards_ok(a)


def test_refused_arguments(alg, orc):
    """Every refused argument returns ALG_ERR_ARG with nothing changed: a following solve matches a handle that never saw the calls."""
    N = 5
    a, b = K.family_problem(_hip(alg), "di3", N), K.family_problem(_hip(alg), "di3", N)
    for h in (a, b):
        h.newton_solve(init=True, game_id0=HS.GID0)
    S, B, n = a.S, a.B, a.n
    D, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    dirs = np.zeros((B, 2, n)); out = np.full((B, n, S), 7.0); st = np.full(B, 9, dtype=np.int32)
    pd, po, ps = dirs.ctypes.data_as(D), out.ctypes.data_as(D), st.ctypes.data_as(I)
    bad = dirs.copy(); bad[B - 1, 1, n - 1] = np.nan
    inf = dirs.copy(); inf[0, 0, 0] = -np.inf
    call = lambda *args: a.lib.kkt_sensitivity(a.h, *args)
    cases = {
        "param 8": (0.0, 8, 0, None, 0, B, 0, 0, po, ps), "param -1": (0.0, -1, 0, None, 0, B, 0, 0, po, ps),
        "ndir without dirs": (0.0, 2, 2, None, 0, B, 0, 0, po, ps), "dirs without ndir": (0.0, 2, 0, pd, 0, B, 0, 0, po, ps),
        "ndir -1": (0.0, 2, -1, pd, 0, B, 0, 0, po, ps), "nan": (0.0, 2, 2, bad.ctypes.data_as(D), 0, B, 0, 0, po, ps),
        "inf": (0.0, 2, 2, inf.ctypes.data_as(D), 0, B, 0, 0, po, ps), "null out": (0.0, 2, 0, None, 0, B, 0, 0, None, ps),
        "first < 0": (0.0, 2, 0, None, -1, 2, 0, 0, po, ps), "count 0": (0.0, 2, 0, None, 0, 0, 0, 0, po, ps),
        "past the batch": (0.0, 2, 0, None, B - 1, 2, 0, 0, po, ps), "first past the batch": (0.0, 2, 0, None, B, 1, 0, 0, po, ps),
        "step < 0": (0.0, 2, 0, None, 0, B, -1, 1, po, ps), "steps -1": (0.0, 2, 0, None, 0, B, 0, -1, po, ps),
        "past the horizon": (0.0, 2, 0, None, 0, B, N - 2, 2, po, ps), "first step past the horizon": (0.0, 2, 0, None, 0, B, N - 1, 1, po, ps),
        "all steps from step 1": (0.0, 2, 0, None, 0, B, 1, 0, po, ps),
    }
    for what, args in cases.items():
        assert call(*args) == ERR_ARG, what
        assert np.all(out == 7.0) and np.all(st == 9), what
    assert a.lib.kkt_sensitivity(None, 0.0, 2, 0, None, 0, B, 0, 0, po, ps) == ERR_ARG
    v = ctypes.c_int32(5)
    for param in (-1, 8):
        assert a.lib.param_len(a.h, param, ctypes.byref(v)) == ERR_ARG and v.value == 5
    assert a.lib.param_len(a.h, 2, None) == ERR_ARG
    # the accepted forms next to them: n_steps = 0 for all steps, a NULL status, the last step of the last game
    assert call(0.0, 2, 0, None, 0, B, 0, 0, po, None) == 0 and call(0.0, 2, 2, pd, B - 1, 1, N - 2, 1, po, ps) == 0 and st[0] == 0
    for h in (a, b):
        h.newton_solve(init=False, game_id0=HS.GID0)
    HS._same_bits(a, b, "solve after the refused calls")
    HS._guards_ok(a)
