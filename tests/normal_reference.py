"""Shared helpers of the normal-equation tests (tests/test_normal_reference.py on the CPU, tests/test_gpu_normal_equations.py on the GPU).  No
test lives here.

The statement.  With X (S, q) the sensitivity columns, z the S entries of pdtraj behind x_1, ẑ the target and w the weights,
    r = z - ẑ  (formed in float64: the device performs the same single subtraction),   Y = [X | r],   G = Y' diag(w) Y,
    H = G[:q, :q],   g = G[:q, q],   loss = G[q, q] / 2,
evaluated in np.longdouble.

The bound (derived, not measured).  Every entry of G is a sum of S terms w_e Y_ec Y_ed.  The device rounds w_e Y_ec once, forms the product
with Y_ed inside a fused multiply-add (one rounding together with the accumulation) and accumulates S times: to first order
    |device - exact| <= (S + 8) 2^-53 sum_e |w_e Y_ec Y_ed|,
the + 8 being headroom for the second-order terms and for the long-double reference's own error.  This is the tolerance of every parity
assertion; loss = G[q, q] / 2 takes half of its entry's bound (the halving is exact).

The Levenberg-Marquardt twin: host.fit_parameters restated over callbacks, so that the oracle backend -- which has no counterpart of the
reduction -- runs the same loop on normal equations built from its own Jacobian."""
import numpy as np

import kkt_reference as K
import param_reference as PR

LD = np.longdouble
DIAG_FLOOR = 1e-12


def gram(X, z, target, w):
    """X (B, q, S) columns in horizontal order, z, target (B, S), w (S,) or (B, S) -> (H, g, loss, tolH, tolg, tolloss): the long-double
    statement rounded to float64 and the derived bound of every entry"""
    B, q, S = X.shape
    r = np.asarray(z, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    Y = np.concatenate([X, r[:, None, :]], axis=1).astype(LD)
    W = np.broadcast_to(np.asarray(w, dtype=np.float64), (B, S)).astype(LD)
    G = np.einsum("bcs,bs,bds->bcd", Y, W, Y)
    A = np.einsum("bcs,bs,bds->bcd", np.abs(Y), W, np.abs(Y))
    tol = (LD(S + 8) * LD(2.0) ** -53 * A).astype(np.float64)
    G = G.astype(np.float64)
    return G[:, :q, :q], G[:, :q, q], 0.5 * G[:, q, q], tol[:, :q, :q], tol[:, :q, q], 0.5 * tol[:, q, q]


def assert_parity(dev, ref, what):
    """dev = (H, g, loss) of the device, ref = gram(...): every entry inside its bound; returns the worst error as a fraction of the bound"""
    worst = 0.0
    for name, d, r, t in zip(("H", "g", "loss"), dev, ref[:3], ref[3:]):
        err = np.abs(np.asarray(d, dtype=LD) - np.asarray(r, dtype=LD)).astype(np.float64)
        assert np.all(np.isfinite(d)), (what, name)
        bad = err > t
        frac = float((err[t > 0] / t[t > 0]).max()) if np.any(t > 0) else 0.0
        assert not bad.any(), (what, name, float(err[bad].max()), frac)
        worst = max(worst, frac)
    return worst


def lm_step(H, g, lam):
    """(H + lambda diag(H)) delta = -g per game, the diagonal floored at DIAG_FLOOR of its maximum; delta = 0 where the system is singular or
    not finite"""
    delta = np.zeros(g.shape)
    for k in range(g.shape[0]):
        d = np.diagonal(H[k])
        if not (np.all(np.isfinite(H[k])) and np.all(np.isfinite(g[k])) and d.max() > 0):
            continue
        try:
            s = np.linalg.solve(H[k] + lam[k] * np.diag(np.maximum(d, DIAG_FLOOR * d.max())), -g[k])
        except np.linalg.LinAlgError:
            continue
        if np.all(np.isfinite(s)):
            delta[k] = s
    return delta


def lm_twin(theta0, positive, evaluate, save, restore, iters=20, damping=1e-3):
    """The loop of host.fit_parameters over callbacks.  evaluate(theta, init) sets theta on every game, solves (warm unless init) and returns
    (H, g, loss, ok); save() keeps the games' state on the host; restore(mask, theta) puts the games of `mask` back to it, with theta set.
    positive: (q,) bool, the columns that must stay > 0.  Returns (theta, loss_history (iters + 1, B), accepted (iters, B))."""
    theta = np.array(theta0, dtype=np.float64)
    H, g, loss, _ = evaluate(theta, True)
    H, g, loss = H.copy(), g.copy(), loss.copy()
    lam = np.full(theta.shape[0], float(damping))
    history, accepted = [loss.copy()], np.zeros((iters, theta.shape[0]), dtype=bool)
    for it in range(iters):
        save()
        trial = theta + lm_step(H, g, lam)
        sane = np.all(np.isfinite(trial), axis=1) & np.all(trial[:, positive] > 0, axis=1)
        trial[~sane] = theta[~sane]
        Hn, gn, ln, ok = evaluate(trial, False)
        acc = sane & ok & (ln < loss)
        accepted[it] = acc
        theta[acc] = trial[acc]; H[acc] = Hn[acc]; g[acc] = gn[acc]; loss[acc] = ln[acc]
        lam = np.where(acc, lam / 10.0, lam * 10.0)
        if not acc.all():
            restore(~acc, theta)
        history.append(loss.copy())
    return theta, np.stack(history), accepted


def oracle_columns(o, cols):
    """X (B, q, S) in horizontal order of the (kind, index) columns at the oracle batch's iterate: X = -J^-1 d res / d theta with the oracle's
    Jacobian and the right-hand sides param_reference writes down (o carries its numbers in o._num: build it under PR.recorded())"""
    tw = K.twin_of(o)
    J = K.jacobians(tw, 0.0)
    # (param_reference.numbers reads every ingredient: a problem without collision avoidance or control bounds states them as absent)
    o._num.setdefault("add_collision_avoidance", (np.zeros(o.p),))
    o._num.setdefault("add_control_bound", (np.full(o.m, np.inf), np.full(o.m, -np.inf)))
    full = {}
    for kind in dict.fromkeys(k for k, _ in cols):
        R, _ = PR.analytic_rhs(tw, kind)
        full[kind] = np.linalg.solve(J, R)                                   # (B, S, len), rows in horizontal order
    return np.stack([full[k][:, :, i] for k, i in cols], axis=1)


class OracleFit:
    """The callbacks of lm_twin on an oracle batch whose games carry per-game LQR data: theta is written through set_lqr, the normal equations
    are gram() of oracle_columns()."""

    def __init__(self, o, lqr, cols, target, weight):
        self.o, self.cols, self.target, self.weight = o, cols, target, weight
        self.data = {k: np.array(v, dtype=np.float64) for k, v in zip(("Q", "R", "xf", "uf"), lqr)}

    def _set(self, theta):
        B = self.o.B
        for c, (k, i) in enumerate(self.cols):
            self.data[k].reshape(B, -1)[:, i] = theta[:, c]
        with PR.recorded():
            self.o.set_lqr(self.data["Q"], self.data["R"], self.data["xf"], self.data["uf"])

    def evaluate(self, theta, init):
        self._set(theta)
        st = self.o.newton_solve(init=init)
        X = oracle_columns(self.o, self.cols)
        H, g, loss = gram(X, self.o.get_traj()[:, self.o.n:], self.target, self.weight)[:3]
        return H, g, loss, (st["converged"] == 1) & (st["status"] == 0) & np.isfinite(loss)

    def save(self):
        self.z = self.o.get_traj()

    def restore(self, mask, theta):
        self._set(theta)
        z = self.o.get_traj(); z[mask] = self.z[mask]
        self.o.set_traj(z)
