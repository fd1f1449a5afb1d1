"""The constraint values of a plan and of a closed-loop run, stated in numpy (a helper, no tests): what alg_get_con_values and alg_mpc_get_con
are held to (tests/test_gpu_con_log.py), pinned on the oracle's evaluate! by tests/test_con_reference.py.

One step k pairs the control u_k with the state x_{k+1} it reaches; its K1 rows, in the ABI's order within each block, are
  [ pair (i, j), j != i: R_ij^2 - |px_i - px_j|^2 (planar, or the first three entries with spherical pairs); 0 for a pair never added
  | u - u_max (m) | u_min - u (m), the control in joint order c = a p + i
  | per player i: x - x_max_i (n), x_min_i - x (n)
  | per player i, wall w:   ((px - x1) xv + (py - y1) yv) [left] [right]
  | per player i, circle c: r^2 - (px - xc)^2 - (py - yc)^2
  | per player i, 3-D wall: ((q - p1) . v) [left] [right] [bottom] [top]
  | per player i, cylinder: (r^2 - |q - p|^2 + (q - p)_axis^2) [0 < (q - p)_axis < l] ]
with a table row whose player bit is clear reporting 0.  c <= 0 is feasible; a row of an infinite bound is -inf.

Next to every value stands a scale s: the sum of the absolute values of the terms of the row's expression, differences of two inputs taken
as |a| + |b|.  Each finite row takes fewer than about 25 rounding operations on partial sums bounded by s, so two correct evaluations differ
by less than 25 * 2^-53 * s; TOL = 64 * 2^-53 covers contraction differences (fused multiply-adds on one side only).  And a margin: the
smallest distance of an indicator's argument from its switch (inf for a row without one) -- a test asserts that it stays above 1e-6, so that
the two sides cannot disagree about an indicator."""
import numpy as np

import algames_jl_amd as alg
from algames_jl_amd import host as H

TOL = 64 * 2.0 ** -53
KINDS = 7
(S_CAR, S_CC, S_CTL, S_SB, S_WALL, S_CIRC, S_WALL3, S_CYL) = range(8)


def tables(prob):
    """structure and numbers of the problem's constraints (host._con_tables: data only, no formulas)"""
    return H._con_tables(prob)


def tables_from_batch(b, spherical=False, axes=None):
    """the same for a handle built with the all-player adders of Batch (tests/ext_horizon_family.py): every pair, every table entry for
    every player; the numbers are read back from the handle (get_scenario_data: the caller's order, per game)"""
    nums = {k: b.get_scenario_data(k) for k in (S_CAR, S_CTL, S_SB, S_WALL, S_CIRC, S_WALL3, S_CYL) if b.scenario_data_len(k) > 0}
    masks = {k: np.ones((b.p, nums[k].shape[1] // w), dtype=bool) for k, w in ((S_WALL, 6), (S_CIRC, 3), (S_WALL3, 12), (S_CYL, 5)) if k in nums}
    return dict(nums=nums, pairs=~np.eye(b.p, dtype=bool), spherical=spherical, masks=masks, axes=None if axes is None else np.asarray(axes))


def rollout_problem(backend=None, B=2, N=6, seed=11):
    """(prob, rng): the 3-player double integrator with control bounds, a wall masked to player 2 and a circle for every player"""
    p = 3
    model = alg.DoubleIntegratorGame(p=p, d=2)
    rng = np.random.default_rng(seed)
    obj = alg.GameObjective([np.eye(4)] * p, [0.1 * np.eye(2)] * p, list(rng.normal(size=(p, 4))), [np.zeros(2)] * p, N, model)
    con = alg.GameConstraintValues(alg.ProblemSize(N, model))
    alg.add_control_bound(con, np.full(model.m, 0.3), np.full(model.m, -0.25))
    alg.add_wall_constraint(con, 2, [alg.Wall([-2.0, 0.1], [2.0, 0.1], [0.0, -1.0])])
    alg.add_circle_constraint(con, np.array([0.2]), np.array([-0.1]), np.array([0.6]))
    opts = alg.Options(); opts.outer_iter, opts.inner_iter = 2, 3
    x0 = 0.4 * rng.normal(size=(B, model.n))
    return alg.GameProblem(N, 0.1, x0, model, opts, obj, con, backend=backend), rng


def circle_rows(rng, B):
    """a schedule of two rows for rollout_problem's circle: (2, B, 3) [xc yc r]"""
    rows = np.empty((2, B, 3))
    rows[..., 0], rows[..., 1], rows[..., 2] = 0.2 + 0.3 * rng.random((2, B)), -0.1 + 0.3 * rng.random((2, B)), 0.5 + 0.4 * rng.random((2, B))
    return rows


def knot_rows(b, tab, nums, x, u):
    """x (B, n), u (B, m) stored player-major -> vals, scale, margin (B, K1 each), kinds (K1,) with -1 for a base block that was not added"""
    B, p, n, m, mi = x.shape[0], b.p, b.n, b.m, b.mi
    pos = lambda i, a: x[:, a * p + i]
    V, S, M, kinds = [], [], [], []
    inf = np.full(B, np.inf)

    def put(v, s, kind, margin=None):
        V.append(v); S.append(s); M.append(inf if margin is None else margin); kinds.append(kind)

    for i in range(p):
        for j in range(p):
            if j == i:
                continue
            if S_CAR in nums and tab["pairs"][i, j]:
                R = nums[S_CAR].reshape(B, p, p)[:, i, j]
                dims = 3 if tab["spherical"] else 2
                d2 = sum((pos(i, a) - pos(j, a)) ** 2 for a in range(dims))
                put(R * R - d2, R * R + sum((np.abs(pos(i, a)) + np.abs(pos(j, a))) ** 2 for a in range(dims)), 0)
            else:
                put(np.zeros(B), np.zeros(B), 0 if S_CAR in nums else -1)
    uj = u.reshape(B, p, mi).transpose(0, 2, 1).reshape(B, m)
    for c in range(2 * m):
        if S_CTL in nums:
            bd = nums[S_CTL][:, c]
            uc = uj[:, c % m]
            put(uc - bd if c < m else bd - uc, np.abs(uc) + np.abs(bd), 1)
        else:
            put(np.zeros(B), np.zeros(B), -1)
    if S_SB in nums:
        sb = nums[S_SB].reshape(B, 2, p, n)
        for i in range(p):
            for r in range(2 * n):
                xe, bd = x[:, r % n], sb[:, r // n, i, r % n]
                put(xe - bd if r < n else bd - xe, np.abs(xe) + np.abs(bd), 2)
    if S_WALL in nums:
        W = nums[S_WALL].reshape(B, -1, 6)
        for i in range(p):
            px, py = pos(i, 0), pos(i, 1)
            for w in range(W.shape[1]):
                x1, y1, x2, y2, xv, yv = W[:, w].T
                if not tab["masks"][S_WALL][i, w]:
                    put(np.zeros(B), np.zeros(B), 3)
                    continue
                left = (px - x1) * (x2 - x1) + (py - y1) * (y2 - y1)
                right = (px - x2) * (x1 - x2) + (py - y2) * (y1 - y2)
                v = np.where((left > 0) & (right > 0), (px - x1) * xv + (py - y1) * yv, 0.0)
                put(v, (np.abs(px) + np.abs(x1)) * np.abs(xv) + (np.abs(py) + np.abs(y1)) * np.abs(yv), 3, np.minimum(np.abs(left), np.abs(right)))
    if S_CIRC in nums:
        Cc = nums[S_CIRC].reshape(B, -1, 3)
        for i in range(p):
            px, py = pos(i, 0), pos(i, 1)
            for c in range(Cc.shape[1]):
                xc, yc, r = Cc[:, c].T
                if not tab["masks"][S_CIRC][i, c]:
                    put(np.zeros(B), np.zeros(B), 4)
                    continue
                put(r * r - (px - xc) ** 2 - (py - yc) ** 2, r * r + (np.abs(px) + np.abs(xc)) ** 2 + (np.abs(py) + np.abs(yc)) ** 2, 4)
    if S_WALL3 in nums:
        W = nums[S_WALL3].reshape(B, -1, 4, 3)
        for i in range(p):
            q = np.stack([pos(i, 0), pos(i, 1), pos(i, 2)], axis=1)
            for w in range(W.shape[1]):
                p1, p2, p3, v = (W[:, w, f] for f in range(4))
                if not tab["masks"][S_WALL3][i, w]:
                    put(np.zeros(B), np.zeros(B), 5)
                    continue
                dot = lambda a, e, c: np.sum((q - a) * (e - c), axis=1)
                flags = np.stack([dot(p1, p2, p1), dot(p2, p1, p2), dot(p3, p2, p3), dot(p2, p3, p2)])
                val = np.where(np.all(flags > 0, axis=0), np.sum((q - p1) * v, axis=1), 0.0)
                put(val, np.sum((np.abs(q) + np.abs(p1)) * np.abs(v), axis=1), 5, np.abs(flags).min(axis=0))
    if S_CYL in nums:
        Y = nums[S_CYL].reshape(B, -1, 5)
        for i in range(p):
            q = np.stack([pos(i, 0), pos(i, 1), pos(i, 2)], axis=1)
            for c in range(Y.shape[1]):
                if not tab["masks"][S_CYL][i, c]:
                    put(np.zeros(B), np.zeros(B), 6)
                    continue
                ax = int(tab["axes"][c])
                t0 = q - Y[:, c, :3]
                ta, l, r = t0[:, ax], Y[:, c, 3], Y[:, c, 4]
                val = np.where((ta > 0) & (ta < l), r * r - np.sum(t0 ** 2, axis=1) + ta ** 2, 0.0)
                mag = (np.abs(q) + np.abs(Y[:, c, :3])) ** 2
                put(val, r * r + mag.sum(axis=1) + mag[:, ax], 6, np.minimum(np.abs(ta), np.abs(ta - l)))
    return np.stack(V, axis=1), np.stack(S, axis=1), np.stack(M, axis=1), np.array(kinds)


def abi_index(b, tab, nums, N):
    """(N - 1, K1) int: the place of row r of step k in the ABI's constraint layout"""
    p, n, m, K = b.p, b.n, b.m, N - 1
    cols, base = [], 0
    k = np.arange(K)
    for q in range(p * (p - 1)):
        cols.append(q * K + k)
    base += p * (p - 1) * K
    for r in range(2 * m):
        cols.append(base + k * 2 * m + r)
    base += 2 * m * K

    def per_player(cnt):
        nonlocal base
        for i in range(p):
            for w in range(cnt):
                cols.append(base + (i * K + k) * cnt + w)
        base += p * cnt * K

    if S_SB in nums:
        per_player(2 * n)
    for kind, width in ((S_WALL, 6), (S_CIRC, 3), (S_WALL3, 12), (S_CYL, 5)):
        if kind in nums:
            per_player(nums[kind].shape[1] // width)
    idx = np.stack(cols, axis=1)
    assert sorted(idx.ravel().tolist()) == list(range(base)), "the map is a permutation of the constraint vector"
    return idx


def plan(b, tab, nums, z, N):
    """z (B, traj_len) as get_traj returns it -> vals, scale, margin (B, con_len each) in the ABI's layout, kinds (con_len,)"""
    n, m, blk = b.n, b.m, b.n + b.m + b.p * b.n
    idx = None
    out = None
    for k in range(N - 1):
        at = n + k * blk
        v, s, mg, kinds = knot_rows(b, tab, nums, z[:, at:at + n], z[:, at + n:at + n + m])
        if idx is None:
            idx = abi_index(b, tab, nums, N)
            out = [np.zeros((z.shape[0], idx.size)) for _ in range(3)] + [np.zeros(idx.size, dtype=int)]
        for o, a in zip(out[:3], (v, s, mg)):
            o[:, idx[k]] = a
        out[3][idx[k]] = kinds
    return tuple(out)


def closed_loop(b, tab, nums, states, controls, hold=1, sched=None):
    """states (knots + 1, B, n), controls (knots, B, m) of a rollout; sched {kind: (rows, B, len)}: knot q takes row min(q // hold, rows - 1)
    -> vals, scale, margin (knots, B, K1), kinds (K1,)"""
    V, S, M = [], [], []
    for q in range(controls.shape[0]):
        t = q // hold
        nq = dict(nums)
        for kind, a in (sched or {}).items():
            nq[kind] = a[min(t, a.shape[0] - 1)]
        v, s, mg, kinds = knot_rows(b, tab, nq, states[q + 1], controls[q])
        V.append(v); S.append(s); M.append(mg)
    return np.stack(V), np.stack(S), np.stack(M), kinds


def summary(vals, kinds):
    """worst (B, 7), first (B, 7) of a log vals (knots, B, K1): the maximum of every kind's rows (NaN if one is NaN, -inf if the kind is
    absent; -0 reads +0) and the first knot with a row that is not <= 0 (-1: none)"""
    B = vals.shape[1]
    worst = np.full((B, KINDS), -np.inf); first = np.full((B, KINDS), -1, dtype=np.int32)
    for c in range(KINDS):
        v = vals[:, :, kinds == c]
        if v.shape[2]:
            worst[:, c] = v.max(axis=(0, 2)) + 0.0
            hit = (~(v <= 0.0)).any(axis=2)
            first[:, c] = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
    return worst, first


def check(got, ref, scale, what=""):
    """got against ref within TOL * scale per row; rows of scale 0 (inert) and infinite rows exactly.  Returns the worst error over the
    tolerance among the finite rows."""
    fin = np.isfinite(ref) & (scale > 0)
    assert np.array_equal(got[~fin], ref[~fin]), f"{what}: an inert or infinite row differs"
    if not fin.any():
        return 0.0
    ratio = np.abs(got[fin] - ref[fin]) / (TOL * scale[fin])
    assert np.all(ratio <= 1.0), f"{what}: worst error / tolerance = {ratio.max():.3g}"
    return float(ratio.max())


# ---- the cases: problems whose data is drawn so that every kind has rows of both signs and no indicator sits on its switch ----------------
def _objective(model, N):
    p, ni, mi = model.p, model.n // model.p, model.m // model.p
    return alg.GameObjective([np.eye(ni)] * p, [0.1 * np.eye(mi)] * p, [np.zeros(ni)] * p, [np.zeros(mi)] * p, N, model)


def make_case(name, N, B, backend=None, seed=0, scenario_kernels="ext", per_game=False):
    """(prob, z): a problem of one of the shapes below and a random trajectory (B, traj_len) for set_traj.  per_game: every game its own
    numbers (a list of GameConstraintValues).  The draw is repeated with the next sub-seed until the data meets `preconditions` (a
    property of the data alone, decided here in numpy before any backend sees it; the tests assert it again)."""
    import types
    for attempt in range(50):
        model, con, x0, z = _draw_case(name, N, B, np.random.default_rng([1000 + seed, attempt]), per_game)
        stub = types.SimpleNamespace(B=B, p=model.p, n=model.n, m=model.m, mi=model.m // model.p)
        tab = H._con_tables(types.SimpleNamespace(batch=stub, game_con=con[0] if per_game else con, game_cons=con if per_game else None))
        try:
            preconditions(*plan(stub, tab, tab["nums"], z, N))
            break
        except AssertionError:
            continue
    prob = alg.GameProblem(N, 0.1, x0, model, alg.Options(), _objective(model, N), con, backend=backend, scenario_kernels=scenario_kernels)
    assert z.shape == (B, prob.batch.traj_len)
    return prob, z


def _draw_case(name, N, B, rng, per_game):
    model = {"di2_p3_base": lambda: alg.DoubleIntegratorGame(p=3, d=2), "di2_p3_ext": lambda: alg.DoubleIntegratorGame(p=3, d=2),
             "di2_p1": lambda: alg.DoubleIntegratorGame(p=1, d=2), "di1_p2": lambda: alg.DoubleIntegratorGame(p=2, d=1),
             "di3_p2": lambda: alg.DoubleIntegratorGame(p=2, d=3), "uni_p4": lambda: alg.UnicycleGame(p=4),
             "bic_p2": lambda: alg.BicycleGame(p=2), "quad_p2": lambda: alg.QuadrotorGame(p=2),
             "di2_p10_sb": lambda: alg.DoubleIntegratorGame(p=10, d=2)}[name]()
    p, n, m = model.p, model.n, model.m

    def one_con():
        con = alg.GameConstraintValues(alg.ProblemSize(N, model))
        jit = lambda a: np.asarray(a, dtype=float) * (1.0 + 0.2 * rng.random(np.shape(a)))
        umax, umin = jit(np.full(m, 0.6)), -jit(np.full(m, 0.5))
        if name != "di2_p10_sb":
            umax[0], umin[m - 1] = np.inf, -np.inf
        if name in ("di2_p3_base", "di1_p2", "uni_p4", "bic_p2", "quad_p2", "di2_p10_sb"):
            alg.add_collision_avoidance(con, jit(np.full(p, 0.8)))
            alg.add_control_bound(con, umax, umin)
        if name == "di2_p1":
            alg.add_control_bound(con, umax, umin)
        if name == "di2_p3_ext":
            alg.add_collision_avoidance(con, 1, 2, float(jit(1.5))); alg.add_collision_avoidance(con, 3, 1, float(jit(1.7)))     # a pair subset
            alg.add_control_bound(con, umax, umin)
            for i in (1, 2, 3):
                xm, xn = jit(np.full(n, 0.7)), -jit(np.full(n, 0.6))
                xm[i], xn[n - i] = np.inf, -np.inf
                alg.add_state_bound(con, i, xm, xn)
            walls = [alg.Wall(jit([-1.0, -3.0]), jit([-1.0, 3.0]), [1.0, 0.0]), alg.Wall(jit([-3.0, 0.5]), jit([3.0, 0.5]), [0.0, -1.0]),
                     alg.Wall(jit([0.3, 0.2]), jit([0.3, 0.9]), [-1.0, 0.0])]
            alg.add_wall_constraint(con, 1, walls[:2]); alg.add_wall_constraint(con, 3, walls[1:])           # masks: entry 1 shared
            alg.add_circle_constraint(con, 2, jit([0.4, -0.5]), jit([0.3, 0.6]), jit([0.9, 0.8]))
            alg.add_circle_constraint(con, 3, jit([1.0]), jit([-1.0]), jit([1.2]))
        if name in ("uni_p4", "bic_p2", "quad_p2"):
            xm, xn = jit(np.full(n, 0.7)), -jit(np.full(n, 0.6))
            xm[1], xn[2] = np.inf, -np.inf
            alg.add_state_bound(con, 1, xm, xn)
            if p > 1:
                alg.add_state_bound(con, p, jit(np.full(n, 0.5)), -jit(np.full(n, 0.9)))
        if name == "di2_p10_sb":
            xm, xn = jit(np.full(n, 0.7)), -jit(np.full(n, 0.6))
            xm[3], xn[5] = np.inf, -np.inf
            alg.add_state_bound(con, 4, xm, xn)
        if name == "di3_p2":
            alg.add_spherical_collision_avoidance(con, jit(np.full(p, 0.9)))
            alg.add_control_bound(con, umax, umin)
            alg.add_wall_constraint(con, [alg.Wall3D(jit([-3.0, -3.0, 0.2]), jit([3.0, -3.0, 0.2]), jit([3.0, 3.0, 0.2]), [0.0, 0.0, -1.0])])
            alg.add_wall_constraint(con, 2, [alg.CylinderWall(jit([0.2, -0.1, -1.5]), "z", 3.0, float(jit(1.1))),
                                             alg.CylinderWall(jit([-2.0, 0.1, 0.3]), "x", 4.0, float(jit(0.9)))])
        return con

    con = [one_con() for _ in range(B)] if per_game else one_con()
    x0 = 0.5 * rng.normal(size=(B, n))
    z = 0.8 * rng.normal(size=(B, n + (N - 1) * (n + m + p * n)))
    z[:, :n] = x0
    return model, con, x0, z


CASES = ("di2_p3_base", "di2_p3_ext", "di2_p1", "di1_p2", "di3_p2", "uni_p4", "bic_p2", "quad_p2", "di2_p10_sb")


def preconditions(vals, scale, margin, kinds, need_signs=True):
    """the data of a case is fit for a comparison: every indicator argument at least 1e-6 from its switch, every kind present with rows of
    both signs (among its live rows)"""
    assert margin.min() >= 1e-6, f"an indicator argument lies {margin.min():.2e} from its switch"
    if need_signs:
        for c in sorted(set(kinds.tolist()) - {-1}):
            v = vals[..., kinds == c]
            v = v[np.isfinite(v)]
            assert (v > 0).any() and (v < 0).any(), f"kind {c}: rows of one sign only"
