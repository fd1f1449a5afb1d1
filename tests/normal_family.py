"""The fit families of the normal-equation tests: small inverse games whose parameters the Levenberg-Marquardt loop must recover.  No test lives
here; tests/test_normal_reference.py holds the preconditions on the oracle, tests/test_gpu_normal_equations.py runs the fits on the device.

Both families are double integrators in the plane (d = 2) with a collision cost and NO inequality constraint: the held-multiplier derivative
is then the derivative of the solution map, and it is exact for the double integrator's linear dynamics.  N = 6, four games, each with its
own theta_true drawn from a fixed generator; the observation is the equilibrium at theta_true, and the fit starts from
    theta_0 = theta_true + REL u max(|theta_true|, FLOOR),   u uniform in [-1, 1] per entry.
  "xf2":  p = 2, fitting all of x_f (8 columns).
  "Q3":   p = 3, fitting the second player's Q (4 columns) with every R held.

COND and E_REF are what tests/test_normal_reference.py measured on the oracle (printed there): the largest condition number of X' W X at
theta_true over the games, and the final error max |theta - theta_true| of the reference loop.  The CPU test asserts the condition number
within a factor of 10 of COND and e_ref <= 1e-3 |theta_0 - theta_true|_inf; the GPU test asserts 10 E_REF."""
import numpy as np

N, B, DT = 6, 4, 0.1
REL, FLOOR = 0.2, 0.1
ITERS = 20
# solver options of the families: the solves are driven to rounding level so that the fit is limited by the loop, not by the solve tolerance
OPTS = dict(outer_iter=3, inner_iter=40, reg_0=1e-6, beta=0.2, eps_dyn=1e-9, eps_sta=1e-9, eps_con=1e-9, eps_opt=1e-9, delta_min=1e-13)
FAMILIES = {"xf2": dict(p=2, wrt=("xf",)), "Q3": dict(p=3, wrt=(("Q", (4, 5, 6, 7)),))}
COND = {"xf2": 25.1, "Q3": 2.19e3}
E_REF = {"xf2": 1.98e-9, "Q3": 1.16e-6}


def numbers(name):
    """x0 (B, n), Q, xf (B, p, 4), R, uf (B, p, 2), collision cost (radius, mu) (p,): the games at theta_true.  Players start on a circle of
    radius 0.4 and cross to the far side, so that their paths meet inside the collision cost's radius."""
    p = FAMILIES[name]["p"]
    rng = np.random.default_rng([11, p])
    ang = 2 * np.pi * np.arange(p) / p + rng.uniform(-0.3, 0.3, (B, p))
    rad = 0.4 + rng.uniform(-0.05, 0.05, (B, p))
    x0 = np.zeros((B, 4 * p)); xf = np.zeros((B, p, 4))
    x0[:, 0:p] = rad * np.cos(ang); x0[:, p:2 * p] = rad * np.sin(ang)
    xf[:, :, 0] = 0.6 * np.cos(ang + np.pi + 0.4); xf[:, :, 1] = 0.6 * np.sin(ang + np.pi + 0.4)
    xf[:, :, 2:] = rng.uniform(-0.2, 0.2, (B, p, 2))
    Q = rng.uniform(5.0, 15.0, (B, p, 4))
    R = rng.uniform(0.05, 0.2, (B, p, 2))
    return dict(x0=x0, Q=Q, xf=xf, R=R, uf=np.zeros((B, p, 2)), cc=(np.full(p, 1.0), np.full(p, 2.0)))


def columns(name):
    """the (kind, index) columns of the family, in the order of host.normal_columns"""
    p = FAMILIES[name]["p"]
    out = []
    for item in FAMILIES[name]["wrt"]:
        kind, idx = (item, range(4 * p)) if isinstance(item, str) else item
        out += [(kind, int(i)) for i in idx]
    return out


def theta_of(name, num):
    return np.stack([num[k].reshape(B, -1)[:, i] for k, i in columns(name)], axis=1)


def start(name):
    """(theta_true, theta_0), both (B, q)"""
    true = theta_of(name, numbers(name))
    u = np.random.default_rng([13, true.shape[1]]).uniform(-1.0, 1.0, true.shape)
    return true, true + REL * u * np.maximum(np.abs(true), FLOOR)


def with_theta(name, theta):
    """the family's numbers with the fitted entries replaced by theta (B, q)"""
    num = numbers(name)
    for c, (k, i) in enumerate(columns(name)):
        num[k].reshape(B, -1)[:, i] = theta[:, c]
    return num


def batch(make, name, num):
    """the family on make(model, p, N, dt, B, d) -> Batch / OracleBatch, with per-game LQR data"""
    p = FAMILIES[name]["p"]
    b = make(0, p, N, DT, B, 2)
    b.set_x0(num["x0"])
    b.set_lqr(num["Q"], num["R"], num["xf"], num["uf"])
    b.set_options(**OPTS)
    b.add_collision_cost(*num["cc"])
    return b


def problem(alg, name, num, backend=None):
    """the same games as a GameProblem (what host.fit_parameters takes): game_obj carries the per-game LQR data of `num`"""
    p = FAMILIES[name]["p"]
    model = alg.DoubleIntegratorGame(p=p, d=2)
    obj = alg.GameObjective([np.ones(4)] * p, [np.ones(2)] * p, [np.zeros(4)] * p, [np.zeros(2)] * p, N, model)
    obj.Qdiag, obj.Rdiag, obj.xf, obj.uf = num["Q"], num["R"], num["xf"], num["uf"]
    alg.add_collision_cost(obj, *num["cc"])
    opts = alg.Options(outer_iter=OPTS["outer_iter"], inner_iter=OPTS["inner_iter"], reg_0=OPTS["reg_0"], β=OPTS["beta"], ϵ_dyn=OPTS["eps_dyn"],
                       ϵ_sta=OPTS["eps_sta"], ϵ_con=OPTS["eps_con"], ϵ_opt=OPTS["eps_opt"], Δ_min=OPTS["delta_min"], inner_print=False, outer_print=False)
    return alg.GameProblem(N, DT, num["x0"], model, opts, obj, alg.GameConstraintValues(alg.ProblemSize(N, model)), backend=backend)
