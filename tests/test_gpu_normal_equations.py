"""alg_kkt_normal_equations on the GPU: the normal equations of a parameter fit reduced on the device (k_sens_gram over the columns of
k_kkt_sens), and host.fit_parameters on top of them.

Parity is always against tests/normal_reference.py -- the long-double statement on the columns alg_kkt_sensitivity returns from the same
handle -- inside its derived bound (S + 8) 2^-53 sum |w Y Y|, for every entry of H, g and loss.  Every game is solved first and reports
status 0.  Every test here needs the entry point, which the commit before the feature does not have."""
import ctypes

import numpy as np
import pytest

import kkt_reference as K
import normal_family as F
import normal_reference as NR
import test_gpu_horizon_shapes as HS
from test_gpu_kkt_solve import _hip, _Prob

pytestmark = pytest.mark.gpu

ERR_ARG = -1
PROFILES = 64                                       # history profiles of the handles whose state is compared: records per game
KINDS = ("x0", "xf", "Q", "R", "uf", "collision_cost", "collision_radius", "control_bound")


def _solved(g, profiles=0):
    """solve every game; profiles: records per game whose violation profiles the solve stores next to the history"""
    if profiles:
        g.set_history_profiles(profiles)
    st = g.newton_solve(init=True, game_id0=HS.GID0)
    assert np.all(st["status"] == 0), st["status"]
    return g


def _state(g):
    """everything the call must leave alone, for bit-wise comparison: HS._bits (pdtraj, duals, penalties, alg_game_stats, history) and the
    per-record violation profiles of every game (the solve ran with history profiles on: no game's profiles are empty)"""
    out = HS._bits(g)
    assert g.get_history_profiles() > 0
    for game in range(g.B):
        vio = g.get_history_vio(game)
        assert all(vio[k].shape[0] >= 1 for k in ("dyn", "con", "sta", "opt")), game
        out += [vio[k] for k in ("dyn", "con", "sta", "opt")]
    return out


def _unchanged(before, g, what):
    after = _state(g)
    assert len(before) == len(after), what
    for i, (x, y) in enumerate(zip(before, after)):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, i)


def _wrt(cols):
    """columns one by one, so that host.normal_columns keeps their order"""
    return [(k, [i]) for k, i in cols]


def _data(g, seed, per_game=False):
    """a target near the plan and positive weights with zeros among them"""
    rng = np.random.default_rng(seed)
    z = g.get_traj()[:, g.n:]
    target = z + rng.uniform(-0.5, 0.5, z.shape)
    w = rng.uniform(0.0, 2.0, z.shape if per_game else g.S)
    w[..., ::7] = 0.0
    return target, w


def _reference(g, cols, target, w, reg=0.0):
    full = {}
    for kind in dict.fromkeys(k for k, _ in cols):
        X, st = g.kkt_sensitivity(kind, reg=reg)
        assert np.all(st == 0), (kind, st)
        full[kind] = X
    X = np.stack([full[k][:, i] for k, i in cols], axis=1)
    return NR.gram(X, g.get_traj()[:, g.n:], target, w)


def _parity(alg, g, cols, target, w, what, reg=0.0):
    ne = alg.normal_equations(_Prob(g), target, _wrt(cols), weight=w, reg=reg)
    assert ne.cols == list(cols) and np.all(ne.status == 0), (what, ne.status)
    q = len(cols)
    assert ne.H.shape == (g.B, q, q) and ne.g.shape == (g.B, q) and ne.loss.shape == (g.B,)
    frac = NR.assert_parity((ne.H, ne.g, ne.loss), _reference(g, cols, target, w, reg), what)
    assert np.array_equal(ne.H, ne.H.transpose(0, 2, 1)), what
    print(what, "q = %d, S = %d: worst error %.3f of the bound" % (q, g.S, frac))
    return ne


def _all_columns(g, kinds):
    return [(k, i) for k in kinds for i in range(g.param_len(k))]


def test_parity_over_the_ragged_row_tails(alg):
    """Double integrator d = 1, p = 3 (b = 27) at N = 3, 4, 5, 6: S mod 4 = 2, 1, 0, 3; wrt = ("xf", "Q"), shared and per-game weights"""
    seen = set()
    for N in (3, 4, 5, 6):
        g = _solved(HS.hip_family(alg, K.DI, 3, 1, N))
        assert g.b == 27
        seen.add(g.S % 4)
        cols = _all_columns(g, ("xf", "Q"))
        for per_game in (False, True):
            target, w = _data(g, N, per_game)
            ne = _parity(alg, g, cols, target, w, ("di3_d1", N, per_game))
        plain = alg.normal_equations(_Prob(g), target, ("xf", "Q"), weight=w)
        assert all(np.array_equal(a, b) for a, b in zip(plain[:4], ne[:4]))
        HS._guards_ok(g)
    assert seen == {0, 1, 2, 3}


def test_parity_over_the_column_tile_edges(alg):
    """Double integrator p = 3, d = 2 with collision cost, collision avoidance and control bounds: 75 columns to choose from; subsets of 1, 15,
    16, 31, 32, 47, 48 and 63 columns mixing the kinds in scrambled order; 64 and 0 columns are refused with the handle untouched."""
    g = _solved(HS.hip_family(alg, K.DI, 3, 2, 4), profiles=PROFILES)
    every = _all_columns(g, KINDS)
    assert len(every) == 75
    target, w = _data(g, 4)
    before = _state(g)
    for q in (1, 15, 16, 31, 32, 47, 48, 63):
        order = np.random.default_rng([4, q]).permutation(75)[:q]
        cols = [every[i] for i in order]
        assert q < 15 or len({k for k, _ in cols}) >= 3
        _parity(alg, g, cols, target, w, ("di3 tiles", q))
    _unchanged(before, g, "the accepted calls")
    D, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    cp = np.array([KINDS.index(k) for k, _ in every[:64]], dtype=np.int32); ci = np.array([i for _, i in every[:64]], dtype=np.int32)
    Hm = np.full((g.B, 64, 64), 7.0); gv = np.full((g.B, 64), 7.0); ls = np.full(g.B, 7.0); st = np.full(g.B, 9, dtype=np.int32)
    wf = np.ascontiguousarray(w)
    for ncol in (64, 0, -1):
        rc = g.lib.kkt_normal_equations(g.h, 0.0, ncol, cp.ctypes.data_as(I), ci.ctypes.data_as(I), target.ctypes.data_as(D), wf.ctypes.data_as(D), 0, 0, g.B,
                                        Hm.ctypes.data_as(D), gv.ctypes.data_as(D), ls.ctypes.data_as(D), st.ctypes.data_as(I))
        assert rc == ERR_ARG, ncol
        _unchanged(before, g, ("ncol", ncol))
    assert np.all(Hm == 7.0) and np.all(gv == 7.0) and np.all(ls == 7.0) and np.all(st == 9)
    HS._guards_ok(g)


@pytest.mark.parametrize("what", ["uni2", "di3_d3", "di3_twin"])
def test_parity_on_other_paths(alg, what):
    """A Gauss-Newton model (unicycle p = 2, N = 5, x0 and R), a dense-direction configuration (double integrator d = 3, p = 3, N = 4, x0) and a
    per-game scenario batch on the base kernels' block-reading twins (collision cost)."""
    if what == "uni2":
        g, kinds = HS.hip_family(alg, K.UNI, 2, 2, 5), ("x0", "R")
    elif what == "di3_d3":
        g, kinds = HS.hip_family(alg, K.DI, 3, 3, 4), ("x0",)
    else:
        g, kinds = K.family_problem(_hip(alg), "di3_twin", 5), ("collision_cost",)
        rad, mu = 1.0 + 0.1 * np.arange(g.B * 3).reshape(g.B, 3) / 12, 2.0 + 0.25 * np.arange(g.B * 3).reshape(g.B, 3)
        g.set_scenario_data(HS.K_COST, np.concatenate([rad, mu], axis=1))          # the games differ in their collision cost
        assert g.get_scenario_kernels() == (1, 2)
    _solved(g)
    target, w = _data(g, 3)
    _parity(alg, g, _all_columns(g, kinds), target, w, what)
    HS._guards_ok(g)


def test_bit_level_properties(alg):
    """A repeated call, sub-ranges of games, a shuffled batch and chunks of one and two games are bit-equal to the plain call; a shared weight
    equals the same weight per game; the target is not read where the weight is 0; a permuted column order stays inside the bound."""
    N = 4
    g = _solved(K.family_problem(_hip(alg), "di3", N))
    cols = _all_columns(g, ("xf", "control_bound", "Q"))[3:]            # 33 columns, the first kind not whole
    q = len(cols)
    target, w = _data(g, 9)
    P = _Prob(g)
    ne = _parity(alg, g, cols, target, w, "di3 bits")
    same = lambda a, b, what: [np.testing.assert_array_equal(x, y, err_msg=str(what)) for x, y in zip(a[:4], b[:4])]
    same(alg.normal_equations(P, target, _wrt(cols), weight=w), ne, "two calls")
    for first, cnt in ((0, 1), (1, 2), (3, 1), (2, 2)):
        part = alg.normal_equations(P, target[first:first + cnt], _wrt(cols), weight=w, games=(first, cnt))
        same(part, [v[first:first + cnt] for v in ne[:4]], ("sub-range", first, cnt))
    for games in (1, 2):
        limit = alg.normal_scratch_bytes(g, cols, games)
        assert limit < alg.normal_scratch_bytes(g, cols, games + 1) and limit > 8 * games * q * g.S
        same(alg.normal_equations(P, target, _wrt(cols), weight=w, max_scratch_bytes=limit), ne, ("chunks of", games))
    wg = np.ascontiguousarray(np.broadcast_to(w, (g.B, g.S)))
    same(alg.normal_equations(P, target, _wrt(cols), weight=wg), ne, "per-game weight")
    same(alg.normal_equations(P, target[2:], _wrt(cols), weight=wg[2:], games=(2, 2), max_scratch_bytes=1), [v[2:] for v in ne[:4]], "per-game weight, chunks, sub-range")
    moved = target.copy(); moved[:, w == 0] += 1e6
    assert (w == 0).sum() >= g.S // 7
    same(alg.normal_equations(P, moved, _wrt(cols), weight=w), ne, "target under zero weight")
    perm = np.random.default_rng(2).permutation(q)
    pe = _parity(alg, g, [cols[i] for i in perm], target, w, "di3 permuted columns")
    ref = _reference(g, cols, target, w)
    assert np.all(np.abs(pe.H - ne.H[:, perm][:, :, perm]) <= 2 * ref[3][:, perm][:, :, perm]) and np.array_equal(pe.loss, ne.loss)
    # a shuffled batch: the games' data, plans and multipliers in another order on a second handle
    order = np.array([2, 0, 3, 1])
    h = K.family_problem(_hip(alg), "di3", N)
    z, (lam, mu) = g.get_traj(), g.get_con_duals()
    h.set_x0(z[order][:, :h.n]); h.set_lqr(*[v[order] for v in g._lqr])
    h.set_traj(z[order]); h.set_con_duals(lam[order], mu[order])
    same(alg.normal_equations(_Prob(h), target[order], _wrt(cols), weight=w), [v[order] for v in ne[:4]], "shuffled batch")
    HS._guards_ok(g); HS._guards_ok(h)


def test_the_call_leaves_the_solver_state_alone(alg):
    """pdtraj, duals, penalties, alg_game_stats, history and the per-record violation profiles (the solve ran with history profiles on) are
    identical before and after a call and after every refused call; ALG_TRAJ_DELTA holds the last column; a following warm solve matches a
    handle that never made the calls."""
    N = 5
    a, b = K.family_problem(_hip(alg), "di3", N), K.family_problem(_hip(alg), "di3", N)
    for h in (a, b):
        _solved(h, profiles=PROFILES)
    before = _state(a)
    x0 = a.get_x0()
    target, w = _data(a, 1)
    cols = [("Q", 2), ("control_bound", 1), ("x0", 5), ("Q", 0)]
    ne = alg.normal_equations(_Prob(a), target, _wrt(cols), weight=w)
    assert np.all(ne.status == 0)
    _unchanged(before, a, "an accepted call")
    assert np.array_equal(a.get_traj(2)[:, a.n:], a.kkt_sensitivity("x0")[0][:, 5])       # kinds run in the order they first appear: x0 is last
    alg.normal_equations(_Prob(a), target, _wrt(cols), weight=w)
    D, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    B, S = a.B, a.S
    Hm = np.full((B, 4, 4), 7.0); gv = np.full((B, 4), 7.0); ls = np.full(B, 7.0); st = np.full(B, 9, dtype=np.int32)
    pH, pg, pl, ps = Hm.ctypes.data_as(D), gv.ctypes.data_as(D), ls.ctypes.data_as(D), st.ctypes.data_as(I)
    ints = lambda *v: np.array(v, dtype=np.int32)
    cp, ci = ints(2, 7, 0, 2), ints(2, 1, 5, 0)
    pt, pw = target.ctypes.data_as(D), w.ctypes.data_as(D)
    nan_t = target.copy(); nan_t[B - 1, S - 1] = np.nan
    inf_t = target.copy(); inf_t[0, 0] = np.inf
    bad_w = {k: w.copy() for k in ("nan", "inf", "neg")}
    bad_w["nan"][S - 1] = np.nan; bad_w["inf"][0] = np.inf; bad_w["neg"][1] = -1e-300
    I_ = lambda v: v.ctypes.data_as(I)
    D_ = lambda v: v.ctypes.data_as(D)
    cases = {
        "kind 8": (0.0, 4, I_(ints(2, 8, 0, 2)), I_(ci), pt, pw, 0, 0, B, pH, pg, pl, ps), "kind -1": (0.0, 4, I_(ints(2, -1, 0, 2)), I_(ci), pt, pw, 0, 0, B, pH, pg, pl, ps),
        "index past the kind": (0.0, 4, I_(cp), I_(ints(12, 1, 5, 0)), pt, pw, 0, 0, B, pH, pg, pl, ps), "index -1": (0.0, 4, I_(cp), I_(ints(2, 1, -1, 0)), pt, pw, 0, 0, B, pH, pg, pl, ps),
        "duplicate": (0.0, 4, I_(cp), I_(ints(2, 1, 5, 2)), pt, pw, 0, 0, B, pH, pg, pl, ps),
        "null kinds": (0.0, 4, None, I_(ci), pt, pw, 0, 0, B, pH, pg, pl, ps), "null indices": (0.0, 4, I_(cp), None, pt, pw, 0, 0, B, pH, pg, pl, ps),
        "null target": (0.0, 4, I_(cp), I_(ci), None, pw, 0, 0, B, pH, pg, pl, ps), "null weight": (0.0, 4, I_(cp), I_(ci), pt, None, 0, 0, B, pH, pg, pl, ps),
        "null H": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, B, None, pg, pl, ps), "null g": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, B, pH, None, pl, ps),
        "null loss": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, B, pH, pg, None, ps),
        "nan target": (0.0, 4, I_(cp), I_(ci), D_(nan_t), pw, 0, 0, B, pH, pg, pl, ps), "inf target": (0.0, 4, I_(cp), I_(ci), D_(inf_t), pw, 0, 0, B, pH, pg, pl, ps),
        "nan weight": (0.0, 4, I_(cp), I_(ci), pt, D_(bad_w["nan"]), 0, 0, B, pH, pg, pl, ps), "inf weight": (0.0, 4, I_(cp), I_(ci), pt, D_(bad_w["inf"]), 0, 0, B, pH, pg, pl, ps),
        "negative weight": (0.0, 4, I_(cp), I_(ci), pt, D_(bad_w["neg"]), 0, 0, B, pH, pg, pl, ps),
        "first < 0": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, -1, 2, pH, pg, pl, ps), "count 0": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, 0, pH, pg, pl, ps),
        "past the batch": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, B - 1, 2, pH, pg, pl, ps), "first past the batch": (0.0, 4, I_(cp), I_(ci), pt, pw, 0, B, 1, pH, pg, pl, ps),
    }
    for what, args in cases.items():
        assert a.lib.kkt_normal_equations(a.h, *args) == ERR_ARG, what
        assert np.all(Hm == 7.0) and np.all(gv == 7.0) and np.all(ls == 7.0) and np.all(st == 9), what
        _unchanged(before, a, what)
    assert a.lib.kkt_normal_equations(None, 0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, B, pH, pg, pl, ps) == ERR_ARG
    # the accepted forms next to them: a NULL status, the last game alone
    assert a.lib.kkt_normal_equations(a.h, 0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, B, pH, pg, pl, None) == 0 and np.all(st == 9)
    assert np.array_equal(Hm, ne.H) and np.array_equal(gv, ne.g) and np.array_equal(ls, ne.loss)
    assert a.lib.kkt_normal_equations(a.h, 0.0, 4, I_(cp), I_(ci), D_(np.ascontiguousarray(target[B - 1:])), pw, 0, B - 1, 1, pH, pg, pl, ps) == 0 and st[0] == 0
    _unchanged(before, a, "the accepted forms")
    assert np.array_equal(x0, a.get_x0())
    assert np.array_equal(a.get_traj(1)[:, :a.n], a.get_traj(0)[:, :a.n])
    # a handle without LQR data: ALG_ERR_STATE where alg_kkt_sensitivity returns it, nothing written
    c = alg.Batch(alg.hip_lib(), K.DI, 3, N, K.DT, B)
    c.set_x0(np.zeros((B, c.n)))
    Hm[:] = 7.0
    assert c.lib.kkt_normal_equations(c.h, 0.0, 4, I_(cp), I_(ci), pt, pw, 0, 0, B, pH, pg, pl, ps) == -3 and np.all(Hm == 7.0)
    assert c.lib.kkt_normal_equations(c.h, 0.0, 4, I_(cp), I_(ci), D_(nan_t), D_(bad_w["neg"]), 0, 0, B, pH, pg, pl, ps) == -3        # before target and weight are read
    assert c.lib.kkt_normal_equations(c.h, 0.0, 4, I_(cp), I_(ci), pt, pw, 0, B, 1, pH, pg, pl, ps) == ERR_ARG and np.all(Hm == 7.0)  # the game range comes first
    for h in (a, b):
        h.newton_solve(init=False, game_id0=HS.GID0)
    HS._same_bits(a, b, "solve after the calls")
    _unchanged(_state(b), a, "profiles of the solve after the calls")
    HS._guards_ok(a)


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_fit(alg, name):
    """fit_parameters on the families of tests/normal_family.py: per game the loss is non-increasing, theta ends within 10 E_REF of theta_true
    (measured on an MI355X: xf2 0.998, Q3 1.00 of E_REF); a game with an unreachable observation ends with a finite theta and leaves
    its neighbours' fits unchanged, bit for bit."""
    true, th0 = F.start(name)
    wrt = F.FAMILIES[name]["wrt"]
    seen = F.problem(alg, name, F.numbers(name))
    alg.newton_solve(seen)
    s = seen.stats.summary
    assert np.all(s["status"] == 0) and np.all(s["converged"] == 1), s
    observed = seen.pdtraj
    prob = F.problem(alg, name, F.with_theta(name, th0))
    fit = alg.fit_parameters(prob, observed, wrt, iters=F.ITERS)
    assert fit.theta.shape == true.shape and fit.loss_history.shape == (F.ITERS + 1, F.B) and fit.accepted.shape == (F.ITERS, F.B)
    assert np.all(fit.status == 0) and np.all(np.diff(fit.loss_history, axis=0) <= 0) and np.all(fit.accepted.sum(axis=0) >= 1)
    assert np.array_equal(np.diff(fit.loss_history, axis=0) < 0, fit.accepted)
    err = np.abs(fit.theta - true).max()
    print(name, "|theta - theta_true| = %.3g = %.3g E_REF; accepted steps %s; loss %s -> %s" % (
        err, err / F.E_REF[name], fit.accepted.sum(axis=0), fit.loss_history[0], fit.loss_history[-1]))
    assert err <= 10 * F.E_REF[name], (name, err)
    far = F.problem(alg, name, F.with_theta(name, th0))
    X, U = observed.states.copy(), observed.controls.copy()
    X[1] += 1e3; U[1] -= 1e3
    lost = alg.fit_parameters(far, (X, U), wrt, iters=F.ITERS)
    assert np.all(np.isfinite(lost.theta)) and np.all(np.isfinite(lost.loss_history))
    keep = np.array([0, 2, 3])
    assert np.array_equal(lost.theta[keep], fit.theta[keep]) and np.array_equal(lost.loss_history[:, keep], fit.loss_history[:, keep])
    assert np.array_equal(lost.accepted[:, keep], fit.accepted[:, keep])
