"""The preconditions of tests/test_gpu_kkt_solve.py, on the CPU and about the REFERENCE only (oracle Jacobian + numpy):

  * on every problem the GPU tests use, np.linalg.solve on the oracle's J is within 1e-11 (relative, per column) of its own solution refined
    with long-double residuals -- the 1e-9 the device solve is held to leaves the reference 100 x room.  Measured: <= 7.4e-12 on the random
    USER problems (4-player unicycle, N = 9, reg = 0, cond 1.3e8).  That is where the GPU tests compare against the numpy solution; on
    the solved family games they use the oracle's J and right-hand sides only;
  * the X0 reference  -J^-1 [A_0 in the dyn_1 rows]  IS the derivative of the root of res(z; x0) = 0 with multipliers and penalties held where the
    dynamics are linear: on the double integrator (3 players N = 6, 2 players N = 4) it agrees with central differences (h = 1e-5) of polished
    re-solves to 1e-7 max |X| (measured: 3.4e-10 max |X|; the finite difference, not the solve, limits it);
  * on the unicycle (3 players, N = 6) the same quantity is NOT that derivative: the reference's Jacobian drops the second-order terms of the
    dynamics (global_quantities.jl:150-172), J^-1 is a Gauss-Newton sensitivity there.  The gap to the finite difference is asserted to be
    <= 0.15 max |X| (measured: 0.049 ... 0.071) and to be there at all (>= 1e-3), so that nobody documents it as exact;
  * the XF right-hand side from oracle residual differences is +w_k Q_i[a] in the opt_i,x rows, as the device builds it.

The GPU tests linearise at the device's own solves; here the oracle's solve of the same game stands in (they agree to 1e-8)."""
import numpy as np
import pytest

import kkt_reference as K
import test_gpu_horizon_shapes as HS

_ORC_ALG = {}


def _as_product(orc):
    if "a" not in _ORC_ALG:
        _ORC_ALG["a"] = K.OracleAsProduct(orc)
    return _ORC_ALG["a"]


def _make(orc):
    return lambda *a: orc.OracleBatch(*a[:5], d=a[5])


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_numpy_reference_on_the_user_problems(orc, name):
    worst = 0.0
    for N in K.horizons(name):
        _, tw = K.pair_problem(_as_product(orc), orc, name, N)
        R = K.user_columns(len(tw), tw[0][0].S, N)
        for reg in K.REGS:
            J = K.jacobians(tw, reg)
            X = K.solve_ref(J, R)
            err = K.col_err(X, K.refine_ld(J, R, X))
            worst = max(worst, err)
            assert err <= 1e-11, (name, N, reg, err)
    print("reference on USER problems", name, "worst relative distance to its long-double-refined solution %.2e" % worst)


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_reference_right_hand_sides_on_the_solved_family_games(orc, name):
    """On the solved family games the GPU tests use the oracle for J and the right-hand sides only (a backward bound, and device against device):
    the XF right-hand side from residual differences is the one written down, the X0 one sits in the dyn_1 rows alone.  The distance of the
    numpy solve to its refined solution is printed, not bounded: with penalties at their ceiling these J are far worse conditioned than the
    USER problems' (4-player unicycle, N = 9: 4.4e-11)."""
    worst = 0.0
    for N in K.horizons(name):
        o = K.family_problem(_make(orc), name, N)
        o.newton_solve(init=True, game_id0=HS.GID0)
        tw = K.twin_of(o)
        J = K.jacobians(tw, 0.0)
        Rxf, Rx0 = K.rhs_xf(tw, [o._lqr] * o.B), K.rhs_x0(tw)
        ana = K.rhs_xf_analytic(o, o._lqr[0])
        assert np.abs(Rxf - ana).max() <= 1e-12 * np.abs(ana).max(), (name, N, np.abs(Rxf - ana).max())
        rows = np.zeros(o.S, dtype=bool); rows[K.vd(o, 0):K.vd(o, 0) + o.n] = True
        assert np.all(Rx0[:, ~rows] == 0) and np.all(np.abs(Rx0[:, rows]).max(axis=(1, 2)) >= 1.0), (name, N)
        for R in (Rx0, Rxf):
            X = K.solve_ref(J, R)
            worst = max(worst, K.col_err(X, K.refine_ld(J, R, X)))
    print("reference on solved family games", name, "worst relative distance to its long-double-refined solution %.2e (not bounded)" % worst)


def _polish(o, tol=1e-13, iters=30):
    """Newton on res(z) = 0 at the batch's x0 with multipliers and penalties held (the oracle's J and LAPACK), to |res| <= tol"""
    for _ in range(iters):
        res = o.residual(0, 0.0)[0]
        if np.abs(res).max() <= tol:
            return
        J = o.residual_jacobian(0.0)
        z = o.get_traj()
        z[:, o.n:] += np.stack([np.linalg.solve(J[g], -res[g]) for g in range(o.B)])
        o.set_traj(z)
    raise AssertionError("polish did not converge: %.2e" % np.abs(o.residual(0, 0.0)[0]).max())


def _x0_gap(orc, model, p, d, N, h=1e-5):
    """max |X0 reference - central difference of polished re-solves| / max |X0 reference| over the games"""
    o = HS.family(lambda *a: K.recording(_make(orc)(*a)), model, p, d, N, **HS.TUNED.get((model, p, d), {}))
    o.newton_solve(init=True, game_id0=HS.GID0)
    _polish(o)
    tw = K.twin_of(o)
    X = K.solve_ref(K.jacobians(tw, 0.0), K.rhs_x0(tw))
    x0, z0 = o.get_traj()[:, :o.n].copy(), o.get_traj()
    fd = np.empty_like(X)
    for c in range(o.n):
        zz = []
        for s in (1.0, -1.0):
            x = x0.copy(); x[:, c] += s * h
            o.set_x0(x)
            z = z0.copy(); z[:, :o.n] = x
            o.set_traj(z)
            _polish(o)
            zz.append(o.get_traj()[:, o.n:])
        fd[:, :, c] = (zz[0] - zz[1]) / (2 * h)
    return np.abs(X - fd).max() / np.abs(X).max()


@pytest.mark.parametrize("cfg,N", [((K.DI, 3, 2), 6), ((K.DI, 2, 2), 4)], ids=["di3_N6", "di2_N4"])
def test_x0_reference_is_the_derivative_of_the_root_on_the_double_integrator(orc, cfg, N):
    gap = _x0_gap(orc, *cfg, N)
    print("X0 reference against central differences", cfg, N, "%.2e max|X|" % gap)
    assert gap <= 1e-7, (cfg, N, gap)


def test_x0_reference_is_a_gauss_newton_sensitivity_on_the_unicycle(orc):
    gap = _x0_gap(orc, K.UNI, 3, 2, 6)
    print("X0 reference against central differences, 3-player unicycle N = 6: %.3f max|X|" % gap)
    assert 1e-3 <= gap <= 0.15, gap
