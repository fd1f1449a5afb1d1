"""The players' costs in numpy: the definition alg_get_cost / alg_mpc_get_cost are held to (include/algames_hip.h), stated once and
independently of algames_jl_amd/host.py -- plain loops over knots, players and pairs, with index maps taken from the model objects' own
pz / pu / px lists (1-based there, as in the reference).

  J_i = sum_{k=1..N} w_k l_i(x_k, u_k),  w_k = dt for k < N, w_N = 1  (the weights of the oracle's cost_grad_x / cost_grad_u, pinned on
  test/objective/objective.jl:52-64; tests/test_cost_reference.py differentiates this file against them)
  l_i = [ 1/2 sum_a Q_i[a] (x[pz_i[a]] - xf_i[a])^2 | 1/2 sum_a R_i[a] (u[pu_i[a]] - uf_i[a])^2 (0 at k = N)
        | sum_{j != i} 1/2 mu_i max(0, r_i - |x[px_i] - x[px_j]|)^2 ]

Trajectories come as the joint vectors of Batch.split_traj: X (N, n), U (N - 1, m) with u[pu_i[a]] the player's a-th control; the closed-loop
log stores controls player-major, stored[i mi + a] = u[pu_i[a]] (stored_to_joint)."""
import numpy as np


def maps(model):
    """0-based (pz (p, ni), pu (p, mi), px (p, 2)) of a model object"""
    return (np.array(model.pz, dtype=int) - 1, np.array(model.pu, dtype=int) - 1, np.array(model.px, dtype=int) - 1)


def stored_to_joint(model, u):
    """controls (..., m) in the stored player-major order -> the joint order of the models"""
    _, pu, _ = maps(model)
    u = np.asarray(u, dtype=np.float64)
    out = np.empty_like(u)
    mi = pu.shape[1]
    for i in range(model.p):
        for a in range(mi):
            out[..., pu[i, a]] = u[..., i * mi + a]
    return out


def stage_cost(model, x, u, Q, R, xf, uf, rad=None, mu=None):
    """l_i(x, u) of one game at one knot, unweighted: (p, 3).  x (n,); u (m,) joint order, or None at the terminal knot; Q, xf (p, ni);
    R, uf (p, mi); rad, mu (p,), or None without a collision cost."""
    pz, pu, px = maps(model)
    p = model.p
    out = np.zeros((p, 3))
    for i in range(p):
        for a in range(pz.shape[1]):
            out[i, 0] += 0.5 * Q[i][a] * (x[pz[i, a]] - xf[i][a]) ** 2
        if u is not None:
            for a in range(pu.shape[1]):
                out[i, 1] += 0.5 * R[i][a] * (u[pu[i, a]] - uf[i][a]) ** 2
        if rad is not None:
            for j in range(p):
                if j != i:
                    dist = np.sqrt((x[px[i, 0]] - x[px[j, 0]]) ** 2 + (x[px[i, 1]] - x[px[j, 1]]) ** 2)
                    out[i, 2] += 0.5 * mu[i] * np.maximum(0.0, rad[i] - dist) ** 2
    return out


def plan_cost(model, dt, X, U, Q, R, xf, uf, rad=None, mu=None):
    """(total (p, 3), stage (N, p, 3), w_k applied) of one game's plan: X (N, n), U (N - 1, m) joint order"""
    N = X.shape[0]
    stage = np.zeros((N, model.p, 3))
    for k in range(N):
        last = k == N - 1
        stage[k] = (1.0 if last else dt) * stage_cost(model, X[k], None if last else U[k], Q, R, xf, uf, rad, mu)
    return stage.sum(axis=0), stage


def batch_plan_cost(model, dt, X, U, Q, R, xf, uf, rad=None, mu=None):
    """plan_cost over a batch: X (B, N, n), U (B, N - 1, m); every number either shared ((p, .) / (p,)) or per game (leading B)"""
    B = X.shape[0]
    pick = lambda a, g, nd: None if a is None else (np.asarray(a)[g] if np.ndim(a) == nd + 1 else np.asarray(a))
    tot, stg = [], []
    for g in range(B):
        t, s = plan_cost(model, dt, X[g], U[g], pick(Q, g, 2), pick(R, g, 2), pick(xf, g, 2), pick(uf, g, 2), pick(rad, g, 1), pick(mu, g, 1))
        tot.append(t); stg.append(s)
    return np.stack(tot), np.stack(stg)


def closed_loop_cost(model, dt, hold, states, controls, Q, R, xf, uf, rad=None, mu=None, target_rows=None, cost_rows=None):
    """(stage (knots, B, p, 3), total (B, p, 3)) of a closed-loop log: states (knots + 1, B, n), controls (knots, B, m) stored player-major.
    Knot q of solve t = q // hold costs dt l_i(states[q], controls[q]); no terminal term.  Q, R (B, p, .) as set; xf, uf (B, p, .) and rad,
    mu (B, p) are the handle's, replaced by row min(t, rows - 1) of target_rows (rows, B, p ni + p mi: xf | uf) / cost_rows (rows, B, 2 p:
    radius | mu) where a schedule is given."""
    knots, B = controls.shape[0], controls.shape[1]
    p, ni, mi = model.p, len(model.pz[0]), len(model.pu[0])
    U = stored_to_joint(model, controls)
    stage = np.zeros((knots, B, p, 3))
    for q in range(knots):
        t = q // hold
        for g in range(B):
            xf_g, uf_g = xf[g], uf[g]
            rad_g, mu_g = (None, None) if rad is None else (rad[g], mu[g])
            if target_rows is not None:
                row = target_rows[min(t, target_rows.shape[0] - 1)][g]
                xf_g, uf_g = row[:p * ni].reshape(p, ni), row[p * ni:].reshape(p, mi)
            if cost_rows is not None:
                row = cost_rows[min(t, cost_rows.shape[0] - 1)][g]
                rad_g, mu_g = row[:p], row[p:]
            stage[q, g] = dt * stage_cost(model, states[q, g], U[q, g], Q[g], R[g], xf_g, uf_g, rad_g, mu_g)
    return stage, stage.sum(axis=0)


def bound(ref, w_mu_r2_pairs=None):
    """The tolerance of the device figures against this file, per component: 1e-12 (ref + w mu_i r_i^2 x pair terms), the second term on the
    collision component only.  Derived, not measured: all summands are non-negative, a total takes fewer than 5 000 rounding operations at
    the shapes of tests/test_gpu_cost.py (5 000 x 2^-53 = 5.6e-13), and the cancellation in r - |.| is absolute in r.

    At the shapes of tests/test_gpu_log_configs.py the count of operations no longer serves (one quadrotor over 129 knots: about 6 200), and
    it is not what bounds the error either: a sum of non-negative terms is off by at most (depth of the longest addition chain + the
    roundings of one term) ulp, relative.  The chain of a device total: the terms of one item (at most the quadrotor's 12 state entries, or
    p - 1 <= 9 pair terms), the factor 1/2 and the weight (2), the trips of a lane (ceil(knots / KPT) = 3 at knots = 2 KPT + 1), the lanes of
    one player in cost_reduce (KPT <= 64); a term costs 3 roundings (difference, square, weight), a pair term a few more (two squares, a
    square root, the gap).  One player, 129 knots (KPT = 64): 12 + 2 + 3 + 64 + 3 = 84 ulp = 9.3e-15.  Two quadrotors, 65 knots (KPT = 32):
    12 + 2 + 3 + 32 + 3 = 52 ulp = 5.8e-15.  This file adds the same terms knot after knot: a chain of at most 130 knots + 15 = 1.6e-14.
    Device and reference together stay below 2.6e-14, a fortieth of the 1e-12: the constant stands."""
    tol = 1e-12 * np.abs(ref)
    if w_mu_r2_pairs is not None:
        tol[..., 2] = tol[..., 2] + 1e-12 * w_mu_r2_pairs
    return tol
