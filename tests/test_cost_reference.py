"""Pins tests/cost_reference.py -- the numpy statement of the players' costs the device figures are held to -- on the CPU oracle.

The oracle has no cost VALUE, only the gradients the reference's tests pin (cost_grad_x / cost_grad_u behind orc.kat_cost; weights on
test/objective/objective.jl:52-64).  So the reference is differentiated: the central difference of J_i with respect to x_k (k >= 2) and
u_{i,k} must be the oracle's q and r.  Knots 2, N - 1 and N; 3-player double integrator and 3-player unicycle, N = 5; a collision cost whose
radii make at least one ordered pair active and one inactive at every knot checked (both asserted).

Tolerances, all computed here:
  * LQR part (state + control components): quadratics, whose central difference is exact -- what is left is the rounding of the two
    function values, 4 eps max |J| / h_q, at h_q = 1e-3.
  * collision part, at h_c = 1e-6: the distance of the central quotient from the derivative is bounded by the gap between the forward and the
    backward quotient, |f(x + h) - 2 f(x) + f(x - h)| / h (the printed second difference over h), plus the same rounding term; plus what the
    reference's own gradient leaves out of the derivative: it evaluates mu (r (eps + d) / (eps sqrt(n) + |d|) - d) with eps = 1e-10
    (objective.jl:134-173), at most w mu_i r_i eps (1 + sqrt(n)) / |d| away from the derivative per active pair.
  * the single-pair value is the oracle's own orc_kat_collision_cost, to rounding (4 eps of the value)."""
import numpy as np
import pytest

import cost_reference as CR

DI, UNI = 0, 1
N, DT, P = 5, 0.1, 3
EPS = np.finfo(float).eps
HQ, HC = 1e-3, 1e-6
KNOTS = (1, N - 2, N - 1)          # 0-based: knots 2, N - 1, N


def _problem(alg, orc, model_id, seed):
    rng = np.random.default_rng(seed)
    model = alg.DoubleIntegratorGame(p=P, d=2) if model_id == DI else alg.UnicycleGame(p=P)
    b = orc.OracleBatch(model_id, P, N, DT, 1)
    ni, mi = b.ni, b.mi
    Q, R = rng.uniform(0.5, 2.0, (P, ni)), rng.uniform(0.5, 2.0, (P, mi))
    xf, uf = rng.normal(size=(P, ni)), 0.3 * rng.normal(size=(P, mi))
    b.set_lqr(Q, R, xf, uf)
    # players 0 and 1 stay within 0.3 of each other, player 2 sits 5 away: with radii (1, 1, 1) the pairs (0,1), (1,0) are active and
    # every pair with player 2 is inactive at every knot
    rad, mu = np.array([1.0, 1.0, 1.0]), np.array([7.0, 11.0, 5.0])
    b.add_collision_cost(rad, mu)
    X = 0.1 * rng.normal(size=(N, b.n))
    _, _, px = CR.maps(model)
    X[:, px[2, 0]] += 5.0
    U = rng.normal(size=(N - 1, b.m))
    return model, b, (Q, R, xf, uf, rad, mu), X, U


def _J(model, X, U, nums, i):
    """(LQR part, collision part) of J_i"""
    tot, _ = CR.plan_cost(model, DT, X, U, *nums)
    return tot[i, 0] + tot[i, 1], tot[i, 2]


@pytest.mark.parametrize("model_id", [DI, UNI])
def test_the_reference_differentiates_to_the_oracles_cost_gradients(alg, orc, model_id):
    model, b, nums, X, U = _problem(alg, orc, model_id, 20 + model_id)
    Q, R, xf, uf, rad, mu = nums
    pz, pu, px = CR.maps(model)
    worst = dict(x=0.0, u=0.0, tol=0.0, second=0.0)
    for k in KNOTS:
        w = 1.0 if k == N - 1 else DT
        dist = lambda i, j: np.hypot(X[k, px[i, 0]] - X[k, px[j, 0]], X[k, px[i, 1]] - X[k, px[j, 1]])
        act = [(i, j) for i in range(P) for j in range(P) if i != j and dist(i, j) < rad[i]]
        assert len(act) >= 1 and len(act) < P * (P - 1), (k, act)          # at least one active and one inactive pair
        for i in range(P):
            q, r, _ = b.kat_cost(i, k, X[k], U[min(k, N - 2)])
            # what the reference's gradient formula leaves out of the derivative, per active pair of player i
            gform = sum(w * mu[i] * rad[i] * 1e-10 * (1 + np.sqrt(b.n)) / dist(i, j) for (a, j) in act if a == i)
            for c in range(b.n):
                def at(h):
                    Xh = X.copy(); Xh[k, c] += h
                    return _J(model, Xh, U, nums, i)
                (qp, _), (qm, _) = at(HQ), at(-HQ)
                (_, cp), (_, cm), (_, c0) = at(HC), at(-HC), at(0.0)
                fd = (qp - qm) / (2 * HQ) + (cp - cm) / (2 * HC)
                second = abs(cp - 2 * c0 + cm)
                tol = 4 * EPS * max(abs(qp), abs(qm)) / HQ + second / HC + 4 * EPS * max(abs(cp), abs(cm)) / HC + gform
                worst.update(x=max(worst["x"], abs(fd - q[c])), tol=max(worst["tol"], tol), second=max(worst["second"], second))
                assert abs(fd - q[c]) <= tol, (k, i, c, fd, q[c], tol, second)
            if k < N - 1:
                for a in range(b.mi):
                    def atu(h):
                        Uh = U.copy(); Uh[k, pu[i, a]] += h
                        return _J(model, X, Uh, nums, i)[0]
                    up, um = atu(HQ), atu(-HQ)
                    fd = (up - um) / (2 * HQ)
                    tol = 4 * EPS * max(abs(up), abs(um)) / HQ
                    worst["u"] = max(worst["u"], abs(fd - r[a]))
                    assert abs(fd - r[a]) <= tol, (k, i, a, fd, r[a], tol)
    print("model %d: worst |fd - q| %.3e, |fd - r| %.3e, largest tolerance %.3e, largest second difference %.3e (h_c = %g)"
          % (model_id, worst["x"], worst["u"], worst["tol"], worst["second"], HC))


def test_the_terminal_knot_has_no_control_term_and_the_weights_are_the_oracles(alg, orc):
    model, b, nums, X, U = _problem(alg, orc, DI, 3)
    tot, stage = CR.plan_cost(model, DT, X, U, *nums)
    assert np.all(stage[N - 1, :, 1] == 0.0) and np.all(stage[:N - 1, :, 1] > 0.0)
    un = np.stack([CR.stage_cost(model, X[k], None if k == N - 1 else U[k], *nums) for k in range(N)])
    assert np.array_equal(stage[:N - 1], DT * un[:N - 1]) and np.array_equal(stage[N - 1], un[N - 1])
    assert np.allclose(tot, stage.sum(axis=0), rtol=4 * EPS, atol=0)


def test_the_single_pair_value_is_the_oracles(alg, orc):
    model = alg.DoubleIntegratorGame(p=2, d=2)
    # test/objective/objective.jl:108-147: x = [1, 1.1, 2, 2, 0, 0, 0, 0], mu = 10, r = 0.2 -> 0.05
    x = np.array([1.0, 1.1, 2.0, 2.0, 0, 0, 0, 0])
    z = np.zeros((2, 4)); zu = np.zeros((2, 2))
    v = CR.stage_cost(model, x, None, z, zu, z, zu, np.array([0.2, 0.2]), np.array([10.0, 10.0]))
    ref = orc.collision_cost_value(10.0, 0.2, x[[0, 2]], x[[1, 3]])
    assert abs(ref - 0.05) < 1e-10
    assert abs(v[0, 2] - ref) <= 4 * EPS * ref and abs(v[1, 2] - ref) <= 4 * EPS * ref
    assert np.all(v[:, :2] == 0.0)
    rng = np.random.default_rng(8)
    for _ in range(20):
        x = rng.normal(size=8); r, m = rng.uniform(0.1, 3.0), rng.uniform(0.5, 20.0)
        v = CR.stage_cost(model, x, None, z, zu, z, zu, np.array([r, r]), np.array([m, m]))
        ref = orc.collision_cost_value(m, r, x[[0, 2]], x[[1, 3]])
        assert abs(v[0, 2] - ref) <= 4 * EPS * abs(ref)


def test_stored_controls_map_to_the_joint_order(alg):
    for model in (alg.DoubleIntegratorGame(p=3, d=2), alg.UnicycleGame(p=4), alg.QuadrotorGame(p=2)):
        mi = len(model.pu[0])
        stored = np.arange(model.m, dtype=float)
        joint = CR.stored_to_joint(model, stored)
        for i in range(model.p):
            for a in range(mi):
                assert joint[model.pu[i][a] - 1] == stored[i * mi + a]
