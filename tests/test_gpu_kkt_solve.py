"""alg_kkt_solve on the GPU: KKT solves with many right-hand sides and the equilibrium sensitivities built on them.

The reference is always the oracle's Jacobian with numpy's LAPACK solve (tests/kkt_reference.py; its own accuracy on every problem used here
is held by tests/test_kkt_sensitivity_family.py on the CPU), never the HIP Jacobian.  One shape per kernel kind (kkt_reference.SHAPES: base
tile path, unicycle, d = 1, EXT by a wall, bicycle, the block-reading twin with per-game pair radii, three dense kinds), horizons N in
{2, 3, 5, 7, 9} and N - 1 = FT + 1 (dense kinds up to 7), four games.  Bounds: the direction test's -- status 0, |X - X_ref| <= 1e-9 max |X_ref|
per column, |J X - R| <= 1e-8 max(1, |R|_inf).  The nine shapes are not the coverage of the kernel's configurations: all 79 run in
tests/test_gpu_kkt_configs.py (the list: tests/kkt_config_family.py)."""
import ctypes

import numpy as np
import pytest

import kkt_reference as K
import test_gpu_horizon_shapes as HS

pytestmark = pytest.mark.gpu

ERR_ARG = -1
TOL_X, TOL_LIN = 1e-9, 1e-8
BIT_SHAPES = ["di3", "uni4", "di3_twin", "di5"]


def _T(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))


def _hip(alg):
    return lambda *a: alg.Batch(alg.hip_lib(), *a[:5], d=a[5])


def _orc(orc):
    return lambda *a: orc.OracleBatch(*a[:5], d=a[5])


class _Prob:
    """the part of a GameProblem the host functions touch"""

    def __init__(self, batch):
        self.batch = batch

    def _sync_options(self):
        pass


def _check(X, st, J, R, Xref, what):
    """X, R, Xref (B, S, q); the three bounds of the module docstring; returns (forward, backward) figures"""
    assert np.all(st == 0), (what, st)
    assert np.all(np.isfinite(X)), what
    fwd = K.col_err(X, Xref)
    lin = np.abs(np.einsum("brc,bcq->brq", J, X) - R).max() / max(1.0, np.abs(R).max())
    print(what, "forward %.2e backward %.2e" % (fwd, lin))
    assert fwd <= TOL_X, (what, fwd)
    assert lin <= TOL_LIN, (what, lin)
    return fwd, lin


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_user_columns_against_the_oracle(alg, orc, name):
    """Five random columns in [-1, 1] per game on the random full-magnitude data of the parity tests, reg = 0 and 1e-3."""
    for N in K.horizons(name):
        g, tw = K.pair_problem(alg, orc, name, N)
        R = K.user_columns(g.B, g.S, N)
        for reg in K.REGS:
            J = K.jacobians(tw, reg)
            X, st = g.kkt_solve(_T(R), reg=reg)
            assert X.shape == (g.B, K.NCOL, g.S) and st.shape == (g.B,)
            _check(_T(X), st, J, R, K.solve_ref(J, R), (name, N, reg))
        HS._guards_ok(g)


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_minus_the_residual_gives_the_newton_direction(alg, orc, name):
    """USER with rhs = -res (alg_residual, same reg) against alg_newton_direction's delta: 1e-12 relative, and the same bits in every call (the
    loader's sign flip of -res is exact, so the records hold what k_direction's hold)."""
    for N in K.horizons(name):
        g, _ = K.pair_problem(alg, orc, name, N)
        for reg in (1e-3, 0.0):
            res = g.residual(0, reg)[0]
            X, st = g.kkt_solve(-res, reg=reg)
            d, sd = g.newton_direction(reg)
            assert np.all(st == 0) and np.all(sd == 0), (name, N, reg)
            err = (np.abs(X[:, 0] - d) / np.abs(d).max(axis=1, keepdims=True)).max()
            assert err <= 1e-12, (name, N, reg, err)
            assert np.array_equal(X[:, 0], d), (name, N, reg)
        HS._guards_ok(g)


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_x0_and_xf_on_solved_family_games(alg, orc, name):
    """After newton_solve on the short-horizon family: each built-in kind equals USER with the host-built reference right-hand side (1e-9 per
    column), both meet the backward bound against the oracle's J at the oracle twin of the HIP iterate (its trajectory, multipliers and
    penalties copied over), and feedback_gains / equilibrium_sensitivity are the matching slices."""
    for N in K.horizons(name):
        g = K.family_problem(_hip(alg), name, N)
        g.newton_solve(init=True, game_id0=HS.GID0)
        o = K.family_problem(_orc(orc), name, N)
        tw = K.twin_of(o)
        K.copy_iterate(g, tw)
        J = K.jacobians(tw, 0.0)
        for kind, R in (("x0", K.rhs_x0(tw)), ("xf", K.rhs_xf(tw, [o._lqr] * o.B))):
            X, st = g.kkt_solve(kind=kind)
            XU, su = g.kkt_solve(_T(R))
            assert X.shape == XU.shape == (g.B, g.n, g.S)            # (n = p ni columns for both kinds)
            assert np.all(st == 0) and np.all(su == 0), (name, N, kind, st, su)
            same = K.col_err(_T(X), _T(XU))
            lin = np.abs(np.einsum("brc,bcq->brq", J, _T(X)) - R).max() / max(1.0, np.abs(R).max())
            print((name, N, kind), "against USER %.2e backward %.2e" % (same, lin))
            assert same <= TOL_X, (name, N, kind, same)
            assert lin <= TOL_LIN, (name, N, kind, lin)
            sens = alg.equilibrium_sensitivity(_Prob(g), wrt=kind)
            assert np.array_equal(sens.dz, _T(X)) and np.array_equal(sens.status, st)
            assert np.array_equal(g.kkt_solve(kind=kind, games=(1, 2))[0], X[1:3])
            if kind == "x0":
                gains = alg.feedback_gains(_Prob(g))
                assert gains.shape == (g.B, g.m, g.n) and np.array_equal(gains, _T(X)[:, g.n:g.n + g.m, :])
                assert np.array_equal(sens.du(1), gains) and np.array_equal(sens.dx(2), _T(X)[:, :g.n, :])
        HS._guards_ok(g)


def _pair_data(name, N, B=4):
    """the draws of test_gpu_parity._pair(seed = N), in its order"""
    model, p, d, _ = K.SHAPES[name]
    rng = np.random.default_rng(N)
    n = (2 * d if model == K.DI else 4) * p
    mi = d if model == K.DI else 2
    ni = n // p
    Q, R = 1 + rng.random((B, p, ni)), 0.5 + rng.random((B, p, mi))
    xf, uf = rng.random((B, p, ni)), rng.random((B, p, mi)) - 0.5
    return Q, R, xf, uf


@pytest.mark.parametrize("name", BIT_SHAPES)
def test_columns_games_and_calls_are_independent_bit_for_bit(alg, orc, name):
    """Columns solved together equal each column solved alone -- also with two forced corrections per column (alg_set_refinement(2, 0.0, ...)),
    which catches a stale rx / rd block after a correction; a game sub-range equals those rows of the full call; a shuffled batch gives the
    shuffled result; two calls are identical."""
    N = 7
    g, _ = K.pair_problem(alg, orc, name, N)
    R = _T(K.user_columns(g.B, g.S, N))
    for forced in (False, True):
        if forced:
            g.set_refinement(max_steps=2, tol=0.0)
        X, st = g.kkt_solve(R, reg=1e-3)
        assert np.all(st == 0)
        if forced:
            assert np.all(g.get_stats()["refinements"] == 0)          # the statistic belongs to the solver paths
        for c in (0, 2, K.NCOL - 1):
            Xc, sc = g.kkt_solve(R[:, c:c + 1], reg=1e-3)
            assert np.array_equal(Xc[:, 0], X[:, c]) and np.all(sc == 0), (name, forced, c)
        for kind in ("x0", "xf"):
            Xk, _ = g.kkt_solve(kind=kind, reg=1e-3)
            X2, _ = g.kkt_solve(kind=kind, reg=1e-3)
            assert np.array_equal(Xk, X2), (name, forced, kind, "two calls")
            assert np.array_equal(g.kkt_solve(kind=kind, reg=1e-3, games=(2, 2))[0], Xk[2:4]), (name, forced, kind, "sub-range")
        Xs, _ = g.kkt_solve(R[1:3], reg=1e-3, games=(1, 2))
        assert np.array_equal(Xs, X[1:3]), (name, forced, "sub-range")
        X2, _ = g.kkt_solve(R, reg=1e-3)
        assert np.array_equal(X2, X), (name, forced, "two calls")
    if K.SHAPES[name][3] == "base":
        perm = np.array([2, 0, 3, 1])
        h, _ = K.pair_problem(alg, orc, name, N)
        z, (lam, mu) = h.get_traj(), h.get_con_duals()
        h.set_x0(z[perm][:, :h.n]); h.set_lqr(*[v[perm] for v in _pair_data(name, N)])
        h.set_traj(z[perm]); h.set_con_duals(lam[perm], mu[perm])
        h.set_refinement(max_steps=2, tol=0.0)
        Xp, _ = h.kkt_solve(R[perm], reg=1e-3)
        assert np.array_equal(Xp, X[perm]), (name, "shuffled batch")
        HS._guards_ok(h)
    HS._guards_ok(g)


@pytest.mark.parametrize("name", ["di3", "uni4", "di5"])
def test_the_call_leaves_the_solver_state_alone(alg, orc, name):
    """Everything test_gpu_horizon_shapes._bits collects (trajectory, multipliers, penalties, statistics, histories) is unchanged by the call, and
    a following newton_solve(init=False) matches, bit for bit, a handle that never made it."""
    N = 7
    a, b = K.family_problem(_hip(alg), name, N), K.family_problem(_hip(alg), name, N)
    for h in (a, b):
        h.newton_solve(init=True, game_id0=HS.GID0)
    before = HS._bits(a)
    x0 = a.get_x0()
    a.kkt_solve(kind="x0"); a.kkt_solve(kind="xf", reg=1e-3)
    a.kkt_solve(_T(K.user_columns(a.B, a.S, N))[1:4], games=(1, 3))
    for i, (x, y) in enumerate(zip(before, HS._bits(a))):
        assert np.array_equal(x, y, equal_nan=True), (name, i)
    assert np.array_equal(x0, a.get_x0())
    zt = a.get_traj(1)
    assert np.array_equal(zt[:, :a.n], a.get_traj(0)[:, :a.n])             # ALG_TRAJ_TRIAL is scratch with x_1 restored
    for h in (a, b):
        h.newton_solve(init=False, game_id0=HS.GID0)
    HS._same_bits(a, b, (name, "solve after the call"))
    HS._guards_ok(a)


def test_refused_arguments(alg, orc):
    """Every refused argument returns ALG_ERR_ARG with nothing changed: a following solve matches a handle that never saw the calls."""
    N = 5
    a, b = K.family_problem(_hip(alg), "di3", N), K.family_problem(_hip(alg), "di3", N)
    for h in (a, b):
        h.newton_solve(init=True, game_id0=HS.GID0)
    S, B, n = a.S, a.B, a.n
    D, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    rhs = np.zeros((B, 2, S)); out = np.full((B, n, S), 7.0); st = np.full(B, 9, dtype=np.int32)
    pr, po, ps = rhs.ctypes.data_as(D), out.ctypes.data_as(D), st.ctypes.data_as(I)
    bad = rhs.copy(); bad[B - 1, 1, S - 1] = np.nan
    inf = rhs.copy(); inf[0, 0, 0] = np.inf
    call = lambda *args: a.lib.kkt_solve(a.h, *args)
    cases = {
        "kind 3": (0.0, 3, 2, pr, 0, B, po, ps), "kind -1": (0.0, -1, 2, pr, 0, B, po, ps),
        "user nrhs 0": (0.0, 0, 0, pr, 0, B, po, ps), "user nrhs -1": (0.0, 0, -1, pr, 0, B, po, ps), "user null rhs": (0.0, 0, 2, None, 0, B, po, ps),
        "user nan": (0.0, 0, 2, bad.ctypes.data_as(D), 0, B, po, ps), "user inf": (0.0, 0, 2, inf.ctypes.data_as(D), 0, B, po, ps),
        "x0 count": (0.0, 1, n - 1, None, 0, B, po, ps), "xf count": (0.0, 2, 1, None, 0, B, po, ps), "x0 with rhs": (0.0, 1, n, pr, 0, B, po, ps),
        "null out": (0.0, 1, 0, None, 0, B, None, ps),
        "first < 0": (0.0, 1, 0, None, -1, 2, po, ps), "count 0": (0.0, 1, 0, None, 0, 0, po, ps), "past the batch": (0.0, 1, 0, None, B - 1, 2, po, ps),
        "first past the batch": (0.0, 1, 0, None, B, 1, po, ps),
    }
    for what, args in cases.items():
        assert call(*args) == ERR_ARG, what
        assert np.all(out == 7.0) and np.all(st == 9), what
    assert a.lib.kkt_solve(None, 0.0, 1, 0, None, 0, B, po, ps) == ERR_ARG
    # the accepted forms next to them: a count of 0 or the full count, a NULL status
    assert call(0.0, 1, 0, None, 0, B, po, None) == 0 and call(0.0, 2, n, None, B - 1, 1, po, ps) == 0 and st[0] == 0
    for h in (a, b):
        h.newton_solve(init=False, game_id0=HS.GID0)
    HS._same_bits(a, b, "solve after the refused calls")
    HS._guards_ok(a)


@pytest.mark.parametrize("name", ["di3", "uni4", "di5"])
def test_interleaved_kinds_on_one_handle_equal_each_call_alone(alg, orc, name):
    """The three entry points run one kernel: on one handle USER, the unit columns of Q, x0, one direction of R, xf and USER again each equal,
    bit for bit, the same call made alone on a fresh handle of the same problem -- no len, dirs, step range or right-hand-side block of one
    kind reaches the next."""
    for N in (3, 7):
        g, _ = K.pair_problem(alg, orc, name, N)
        R = _T(K.user_columns(g.B, g.S, N))
        v = np.random.default_rng(100 + N).uniform(-1.0, 1.0, (g.B, g.p * g.mi))
        calls = [lambda h: h.kkt_solve(R, reg=1e-3), lambda h: h.kkt_sensitivity("Q", reg=1e-3), lambda h: h.kkt_solve(kind="x0", reg=1e-3),
                 lambda h: h.kkt_sensitivity("R", reg=1e-3, dirs=v), lambda h: h.kkt_solve(kind="xf", reg=1e-3), lambda h: h.kkt_solve(R, reg=1e-3)]
        together = [call(g) for call in calls]
        for c, (call, (X, st)) in enumerate(zip(calls, together)):
            Xa, sa = call(K.pair_problem(alg, orc, name, N)[0])
            assert np.all(st == 0) and np.array_equal(st, sa), (name, N, c)
            assert X.shape == Xa.shape and np.array_equal(X, Xa), (name, N, c)
        assert np.array_equal(together[0][0], together[-1][0]), (name, N, "USER twice")
        HS._guards_ok(g)
