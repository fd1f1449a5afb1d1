"""Shared helpers of the parameter-sensitivity tests (tests/test_param_reference.py on the CPU, tests/test_gpu_param_sensitivity.py on the GPU),
built on tests/kkt_reference.py: the numbers a problem was assembled with, the right-hand sides R = -d res / d theta written down on the host,
and the same right-hand sides as central differences of the ORACLE's residual.  No test lives here.

theta is one of the parameter vectors of alg_kkt_sensitivity (PARAMS, in the ABI's order); a right-hand side is (B, S, len) in the vertical
order of the residual.  The numbers are recorded while the problem is built (`recorded()` wraps the setters of Batch for the duration of a
`with` block), because neither the oracle nor the ABI hands the handle's values back; an oracle twin entry (OracleBatch, game) then carries
its batch's numbers in `o._num`.

Central differences re-assemble the oracle batch with one entry of theta moved by +-h (all games of the batch at once: the numbers of the
constraints are shared by a batch, per-game LQR data moves the same entry of every game) and restore the batch afterwards.  The pair table is
rebuilt pair by pair (add_collision_avoidance_pair), which is the only way the oracle takes a radius of one ordered pair.

A handle need not carry every ingredient (one player has no collision terms), and its pair table may have been built pair by pair
(add_collision_avoidance_pair: a partial, asymmetric table).  `carried` names the parameters a handle has; `numbers` leaves an ingredient
that was never added out, and gives the pair table with the mask `on` of the ordered pairs that exist (a never-added pair: radius 0, off)."""
import contextlib

import numpy as np

import kkt_reference as K

PARAMS = ("x0", "xf", "Q", "R", "uf", "collision_cost", "collision_radius", "control_bound")
NEW = PARAMS[2:]                                   # what alg_kkt_solve has no kind for
H_AFFINE = 2.0 ** 10                               # step of the entries the residual is affine in everywhere (steps)
H_RADIUS_COST = 2.0 ** -11                         # step of the collision cost's r_i (steps)
H_RADIUS_PAIR = 2.0 ** -16                         # step of the pair radii R_ij (steps)
H_BOUND = 1.0                                      # step of the control bounds, placed at +-BOUND_AT for this check (move_bounds)
BOUND_AT = 3.0
EPS = 1e-10                                        # the eps of the CollisionCost gradient (objective.jl:134-149)
_SETTERS = ("set_lqr", "add_collision_cost", "add_collision_avoidance", "add_control_bound")


PAIRS = "add_collision_avoidance_pair"            # key of o._num of a table built pair by pair: ((p, p) radii, 0 where never added,)


@contextlib.contextmanager
def recorded():
    """while active, every Batch (oracle batches included) keeps the arguments of its last set_lqr / add_collision_cost /
    add_collision_avoidance / add_control_bound in self._num, and the ordered pairs of add_collision_avoidance_pair as one (p, p) table under
    PAIRS (the all-pairs form and the pair-by-pair form replace each other, as on the handle)"""
    import algames_jl_amd as A
    names = _SETTERS + ("add_spherical_collision_avoidance",)
    orig = {k: getattr(A.Batch, k) for k in names + (PAIRS,)}

    def wrap(k):
        def f(self, *a):
            num = self.__dict__.setdefault("_num", {})
            # (the spherical form: the same radii, the distance over three position entries -- analytic_rhs_game's `dims`)
            num["add_collision_avoidance" if k.startswith("add_spherical") else k] = tuple(np.array(v, dtype=np.float64) for v in a)
            if k.endswith("collision_avoidance"):
                self._dims = 3 if k.startswith("add_spherical") else 2
                num.pop(PAIRS, None)
            return orig[k](self, *a)
        return f

    def pair(self, i, j, radius, spherical=False):
        num = self.__dict__.setdefault("_num", {})
        num.pop("add_collision_avoidance", None)
        tab = num.get(PAIRS, (np.zeros((self.p, self.p)),))[0].copy()
        tab[i, j] = radius
        num[PAIRS] = (tab,)
        self._dims = 3 if spherical else 2
        return orig[PAIRS](self, i, j, radius, spherical=spherical)
    for k in names:
        setattr(A.Batch, k, wrap(k))
    setattr(A.Batch, PAIRS, pair)
    try:
        yield
    finally:
        for k in names + (PAIRS,):
            setattr(A.Batch, k, orig[k])


def pair_problem(alg, orc, name, N, B=4):
    with recorded():
        return K.pair_problem(alg, orc, name, N, B=B)


def family_problem(make, name, N, B=4):
    with recorded():
        return K.family_problem(make, name, N, B=B)


def _pair_table(o, num):
    """(pair (p, p), on (p, p) bool) of the recorded collision avoidance, or None: r_i + r_j on every ordered pair of the all-pairs form, the
    recorded radii of the pairs that were added one by one; the diagonal and a never-added pair are 0 and off"""
    p = o.p
    if "add_collision_avoidance" in num:
        r = np.broadcast_to(num["add_collision_avoidance"][0], (p,))
        return (r[:, None] + r[None, :]) * (1 - np.eye(p)), ~np.eye(p, dtype=bool)
    if PAIRS in num:
        tab = num[PAIRS][0] * (1 - np.eye(p))
        return tab, tab > 0
    return None


INGREDIENT = {"collision_cost": "add_collision_cost", "control_bound": "add_control_bound"}


def carried(o):
    """the parameters of PARAMS the handle has an ingredient for (alg_kkt_sensitivity answers ALG_ERR_STATE for the others)"""
    num = o._num
    have = lambda q: (_pair_table(o, num) is not None) if q == "collision_radius" else INGREDIENT.get(q, "set_lqr") in num
    return tuple(q for q in PARAMS if have(q))


def numbers(o, g):
    """the numbers of game g of batch o: Q, xf (p, ni), R, uf (p, mi), cc_r, cc_mu (p), pair (p, p) with a zero diagonal and its mask `on`
    (p, p) of the ordered pairs that exist, umax, umin (m); an ingredient that was never added is absent"""
    num = o._num
    Q, R, xf, uf = num["set_lqr"]
    ni = o.n // o.p
    pick = lambda v, w: np.broadcast_to(v[g] if v.ndim == 3 else v, (o.p, w)).copy()
    out = dict(Q=pick(Q, ni), xf=pick(xf, ni), R=pick(R, o.mi), uf=pick(uf, o.mi))
    if "add_collision_cost" in num:
        out.update(cc_r=num["add_collision_cost"][0].copy(), cc_mu=num["add_collision_cost"][1].copy())
    tab = _pair_table(o, num)
    if tab is not None:
        out.update(pair=tab[0], on=tab[1])
    if "add_control_bound" in num:
        out.update(umax=num["add_control_bound"][0].copy(), umin=num["add_control_bound"][1].copy())
    return out


def param_len(o, param):
    ni = o.n // o.p
    return dict(x0=o.n, xf=o.p * ni, Q=o.p * ni, R=o.p * o.mi, uf=o.p * o.mi, collision_cost=2 * o.p, collision_radius=o.p * o.p, control_bound=2 * o.m)[param]


def _game(o, g):
    """(z, lam, mu) of game g"""
    lam, mu = o.get_con_duals()
    return o.get_traj()[g], lam[g], mu[g]


def _active(c, lam):
    return 1.0 if (c >= 0.0 or lam > 0.0) else 0.0


def _pairq(p, i, j):
    return i * (p - 1) + (j if j < i else j - 1)


def analytic_rhs_game(o, g, param):
    """R = -d res / d theta of game g, (S, len), written down term by term from the oracle's residual (cost_grad_x / cost_grad_u and the
    collision-avoidance and control-bound blocks of `residual`, oracle/algames_oracle.cpp).  Also returns the activity of the rows the
    parameter enters: a list of 0 / 1 (collision_radius, control_bound: a = (c >= 0) | (lambda > 0) per finite row; collision_cost: the
    pairs' r_i - |d| > 0): what the test counts active and inactive rows with.  A parameter whose ingredient was never added is no parameter
    of this handle (`carried`): zeros and no rows; a never-added pair of a partial pair table has no row and a zero column."""
    z, lam, mu = _game(o, g)
    num = numbers(o, g)
    n, m, p, mi, N, dt = o.n, o.m, o.p, o.mi, o.N, o.dt
    ni = n // p
    L = param_len(o, param)
    R = np.zeros((o.S, L))
    act = []
    if param not in carried(o):
        return R, act
    eps_n = EPS * np.sqrt(float(n))
    for k in range(N - 1):
        w = dt if k + 1 < N - 1 else 1.0
        x = z[n + K.hx(o, k):n + K.hx(o, k) + n]
        for i in range(p):
            u = z[n + K.hu(o, k, i):n + K.hu(o, k, i) + mi]
            rx, ru = K.vx(o, i, k), K.vu(o, i, k)
            if param == "xf":
                for a in range(ni):
                    R[rx + a * p + i, i * ni + a] = w * num["Q"][i, a]
            elif param == "Q":
                for a in range(ni):
                    R[rx + a * p + i, i * ni + a] = -w * (x[a * p + i] - num["xf"][i, a])
            elif param == "R":
                for j in range(mi):
                    R[ru + j, i * mi + j] = -dt * (u[j] - num["uf"][i, j])
            elif param == "uf":
                for j in range(mi):
                    R[ru + j, i * mi + j] = dt * num["R"][i, j]
            elif param == "collision_cost":
                for j in range(p):
                    if j == i:
                        continue
                    dl = np.array([x[i] - x[j], x[p + i] - x[p + j]])
                    nrm = np.sqrt(dl[0] * dl[0] + dl[1] * dl[1])
                    on = max(0.0, num["cc_r"][i] - nrm) > 0.0
                    act.append(1.0 if on else 0.0)
                    if not on:
                        continue
                    for a in range(2):
                        f = (EPS + dl[a]) / (eps_n + nrm)
                        for col, dg in ((i, num["cc_mu"][i] * f), (p + i, num["cc_r"][i] * f - dl[a])):       # d gg / d r_i, d gg / d mu_i
                            R[rx + a * p + i, col] += w * dg                                              # res gets -w gg at i, +w gg at j
                            R[rx + a * p + j, col] -= w * dg
            elif param == "collision_radius":
                for j in range(p):
                    if j == i or not num["on"][i, j]:
                        continue
                    Rr = num["pair"][i, j]
                    dims = getattr(o, "_dims", 2)                                                             # 3: the spherical form
                    dl = np.array([x[a * p + i] - x[a * p + j] for a in range(dims)])
                    ci = _pairq(p, i, j) * (N - 1) + k
                    a_ = _active(Rr * Rr - dl @ dl, lam[ci])
                    act.append(a_)
                    for a in range(dims):
                        t = 2.0 * dl[a] * a_ * mu[ci] * 2.0 * Rr                                           # res gets -t at i, +t at j
                        R[rx + a * p + i, i * p + j] += t
                        R[rx + a * p + j, i * p + j] -= t
            elif param == "control_bound":
                for j in range(mi):
                    c = j * p + i
                    for half in range(2):
                        ci = p * (p - 1) * (N - 1) + k * 2 * m + half * m + c
                        cv = u[j] - num["umax"][c] if half == 0 else num["umin"][c] - u[j]
                        if not np.isfinite(cv):
                            continue
                        a_ = _active(cv, lam[ci])
                        act.append(a_)
                        R[ru + j, half * m + c] = a_ * mu[ci]                                                # res gets -a mu per half
    return R, act


def analytic_rhs(tw, param):
    """(B, S, len) and the concatenated activity list"""
    if param == "x0":
        return K.rhs_x0(tw), []
    out, act = [], []
    for o, g in tw:
        R, a = analytic_rhs_game(o, g, param)
        out.append(R); act += a
    return np.stack(out), act


def _set(o, name, *args, **kw):
    """Batch's own setter, past any wrapper that sits on the instance (kkt_reference.recording keeps the one it was given): o._num stays"""
    import algames_jl_amd as A
    return getattr(A.Batch, name)(o, *args, **kw)


def _set_pairs(o, pair, on):
    """the collision avoidance of batch o rebuilt pair by pair from the table `pair` over the ordered pairs of `on`, in the batch's own form
    (planar or spherical).  The spherical adders re-create the multipliers: they are put back."""
    sph = getattr(o, "_dims", 2) == 3
    lam, mu = o.get_con_duals()
    o.lib.check((o.lib.add_spherical_collision_avoidance if sph else o.lib.add_collision_avoidance)(o.h, None))
    for i in range(o.p):
        for j in range(o.p):
            if j != i and on[i, j]:
                _set(o, PAIRS, i, j, pair[i, j], spherical=sph)
    if sph:
        assert o.get_con_duals()[0].shape == lam.shape
        o.set_con_duals(lam, mu)


def _apply(o, num):
    """the batch's numbers as recorded in `num` (the layout of o._num)"""
    for name in _SETTERS:
        if name in num and name != "add_collision_avoidance":
            _set(o, name, *num[name])
    tab = _pair_table(o, num)
    if tab is not None:
        if "add_collision_avoidance" in num and getattr(o, "_dims", 2) == 2:
            _set(o, "add_collision_avoidance", *num["add_collision_avoidance"])
        else:
            _set_pairs(o, *tab)


def _moved(o, param, c, s):
    """assemble batch o with entry c of theta moved by s (every game's entry for per-game LQR data)"""
    num = {k: tuple(v.copy() for v in vs) for k, vs in o._num.items()}
    p, m = o.p, o.m
    if param in ("xf", "Q", "R", "uf"):
        w = o.mi if param in ("R", "uf") else o.n // o.p
        num["set_lqr"][("Q", "R", "xf", "uf").index(param)][..., c // w, c % w] += s
        _set(o, "set_lqr", *num["set_lqr"])
    elif param == "collision_cost":
        num["add_collision_cost"][c // p][c % p] += s
        _set(o, "add_collision_cost", *num["add_collision_cost"])
        o._cc_now = num["add_collision_cost"]                          # (the oracle hands no number back: _activity asks it pair by pair)
    elif param == "control_bound":
        num["add_control_bound"][c // m][c % m] += s
        _set(o, "add_control_bound", *num["add_control_bound"])
    else:
        pair, on = _pair_table(o, num)
        pair = pair.copy()
        pair[c // p, c % p] += s                                        # (the diagonal, a never-added pair: no parameter, nothing moves)
        _set_pairs(o, pair, on)


def _no_column(o, param, c):
    """collision_radius: the diagonal of the pair table and a never-added pair are no parameters of the oracle"""
    return param == "collision_radius" and not _pair_table(o, o._num)[1][c // o.p, c % o.p]


def fd_rhs(tw, param, h):
    """R = -(res(theta + h e_c) - res(theta - h e_c)) / (2 h) per game, (B, S, len), of the oracle's residual; h: one step or one per column.
    The diagonal of the pair table and a never-added pair are no parameters of the oracle: their columns stay zero."""
    out, done = [None] * len(tw), {}
    for k, (o, g) in enumerate(tw):
        if id(o) not in done:
            L = param_len(o, param)
            hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (L,))
            saved = {k2: tuple(v.copy() for v in vs) for k2, vs in o._num.items()}
            R = np.zeros((o.B, o.S, L))
            for c in range(L):
                if _no_column(o, param, c):
                    continue
                rr = []
                for s in (hs[c], -hs[c]):
                    _moved(o, param, c, s)
                    rr.append(o.residual(0, 0.0)[0])
                R[:, :, c] = -(rr[0] - rr[1]) / (2 * hs[c])
            _apply(o, saved)
            done[id(o)] = R
        out[k] = done[id(o)][g]
    return np.stack(out)


def steps(o, param):
    """the step of every column: one power of two per kind.
    H_AFFINE = 2^10 where the residual is affine in the entry everywhere (Q, R, uf, xf, the collision cost's mu), not the 1 of rhs_xf: the
    difference carries the rounding eps |terms of the row| of the oracle's residual whatever the step, and on solved games whose penalties
    sit at their ceiling those terms reach 1e4 -- 1e-12 absolute, the whole bound where max |R| is below 1 (measured with step 1: 1.0e-12
    against 0.84e-12 for Q on the 4-player unicycle at N = 9).  The quotient of an affine function is exact at any step, so the larger step
    only divides that rounding.
    The two radii: the residual is affine in r_i and quadratic in R_ij while no pair changes its activity, so the step only has to stay
    below the distance to the nearest change over all problems of the tests, and the larger it is the less of the rows' rounding remains.
    H_RADIUS_PAIR = 2^-16 for R_ij: the nearest change is 4.9e-5 away (random data of the 3-player double integrator), three steps.
    H_RADIUS_COST = 2^-11 for r_i: the nearest is 1.1e-3 away (solved two-player games in one dimension), two steps; at 2^-16 the rounding
    of the solved 4-player unicycle games' rows at N = 9 (penalties at their ceiling, terms of 1e4) is 7.8e-8 against a bound of 5.5e-8.
    H_BOUND = 1 for the control bounds, on problems whose bounds were moved to +-BOUND_AT (move_bounds)."""
    L = param_len(o, param)
    if param == "collision_radius":
        return np.full(L, H_RADIUS_PAIR)
    if param == "collision_cost":
        return np.concatenate([np.full(o.p, H_RADIUS_COST), np.full(o.p, H_AFFINE)])
    return np.full(L, H_BOUND if param == "control_bound" else H_AFFINE)


def bound(o, param, c):
    """relative bound (times max |R|) of column c: 1e-8 for the two radii, 1e-12 for every entry the residual is affine in"""
    return 1e-8 if param == "collision_radius" or (param == "collision_cost" and c < o.p) else 1e-12


def move_bounds(tw):
    """The control bounds of the twin's batches moved to +-BOUND_AT (an infinite bound stays infinite), recorded like the problem's own.  The
    residual is affine in a bound only while no row with lambda = 0 crosses c = 0; the problems' own bounds (0.6 / -0.4 on the random data,
    +-0.8 on the solved games, which hold saturated controls at violations of 1e-4 and less) leave rows closer to c = 0 than any step that
    meets the 1e-12 bound.  Every control of the problems lies in [-1, 1], so at +-3 a step of 1 crosses nothing: rows with lambda > 0 are
    active, rows with lambda = 0 inactive, on both sides of the difference.  The right-hand side written down on the host is evaluated at
    the same moved bounds -- the formula under test is the one the GPU tests use at the problems' own."""
    for o in {id(o): o for o, _ in tw}.values():
        umax, umin = o._num["add_control_bound"]
        with recorded():
            o.add_control_bound(np.where(np.isfinite(umax), BOUND_AT, umax), np.where(np.isfinite(umin), -BOUND_AT, umin))


def _activity(o, param):
    """what the oracle says about the rows the parameter enters, for every game of the batch: a = (c >= 0) | (lambda > 0) of the finite rows
    of orc_kat_evaluate_con's constraint values (collision_radius, control_bound), or which (game, step, i, j) carry a collision cost
    (orc_kat_collision_cost != 0)"""
    import oracle as orc
    if param != "collision_cost":
        v, lam = o.kat_evaluate_con(), o.get_con_duals()[0]
        return np.where(np.isfinite(v), (v >= 0.0) | (lam > 0.0), False)
    z, (r, mu) = o.get_traj(), o._cc_now
    p, n = o.p, o.n
    out = []
    for g in range(o.B):
        for k in range(o.N - 1):
            x = z[g, n + K.hx(o, k):n + K.hx(o, k) + n]
            out += [orc.collision_cost_value(1.0, r[i], x[[i, p + i]], x[[j, p + j]]) != 0.0 for i in range(p) for j in range(p) if j != i]
    return np.array(out)


def flips(tw, param, h):
    """rows whose activity (pairs whose collision cost) differs between theta + h e_c and theta - h e_c on the oracle, over every column and
    every game of the twin's batches; the batches get their numbers back"""
    bad = 0
    for o in {id(o): o for o, _ in tw}.values():
        hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (param_len(o, param),))
        for c in range(len(hs)):
            if _no_column(o, param, c):
                continue
            act = []
            for s in (hs[c], -hs[c]):
                _moved(o, param, c, s)
                act.append(_activity(o, param))
            bad += int(np.sum(act[0] != act[1]))
        _apply(o, o._num)
    return bad
