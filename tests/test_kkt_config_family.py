"""The preconditions of tests/test_gpu_kkt_configs.py, on the CPU and about the REFERENCE only (oracle + numpy), for every configuration of the KKT
column kernel (tests/kkt_config_family.py: 79), the per-game problems and the partial pair tables.  No GPU needed.

  * the k_kkt_sens<...> kernels of the built library map one to one onto kkt_config_family.CONFIGS: a configuration added to the library
    later cannot go untested, an entry without a kernel cannot pass vacuously;
  * on every problem the GPU tests use, np.linalg.solve on the oracle's J is within 1e-11 (relative, per column) of its own solution refined
    with long-double residuals (the rule of test_kkt_sensitivity_family), and the reference's own backward figure
    |J X_ref - R| / max(1, |R|_inf) is <= 1e-10 on USER columns and on the Q / collision_radius / control_bound columns: the device's 1e-8
    keeps 100 x room over it.  Both are printed per problem; the worst are quoted in kkt_config_family's docstring;
  * the right-hand sides written down on the host (param_reference.analytic_rhs) equal central differences of the oracle's residual at
    param_reference.steps / bound, column by column, with no row changing its activity between theta + h and theta - h (flips == 0, for the
    three constraint kinds, no column left out), control bounds after move_bounds -- the check of test_param_reference, on these problems;
  * on the per-game problems the check can fail: with game 0's numbers in place of game g's the analytic right-hand side of each of
    collision_cost, collision_radius and control_bound differs from game g's own by more than 1e-3 max |R| in some column, for every g >= 1."""
import re

import numpy as np
import pytest

import kkt_config_family as F
import kkt_reference as K
import param_reference as PR
from test_gpu_parity import PAIR_CASES
from test_kkt_sensitivity_family import _as_product
from test_kkt_solve_build import _resources

CHECKED = ("xf",) + PR.NEW
TOL_FORWARD, TOL_BACKWARD = 1e-11, 1e-10


def test_the_library_has_one_column_kernel_per_listed_configuration(alg):
    res = _resources(alg)
    names = sorted(k for k in res if k.startswith("k_kkt_sens<"))
    have = []
    for k in names:                                     # k_kkt_sens<Cfg<model, p, d, ext, wavefronts per game> >
        m = re.fullmatch(r"k_kkt_sens<Cfg<(\d+), (\d+), (\d+), (\d+), (\d+)> ?>", k)
        assert m and int(m.group(5)) == 1, k            # (one wavefront per game: no team shape has a column kernel)
        have.append(tuple(int(v) for v in m.groups()[:4]))
    print("k_kkt_sens kernels in the library: %d, configurations listed: %d" % (len(have), len(F.CONFIGS)))
    assert len(set(have)) == len(have) and len(set(F.CONFIGS)) == len(F.CONFIGS) == 79
    assert [c for c in have if c not in F.CONFIGS] == [], "a kernel without a list entry"
    assert [c for c in F.CONFIGS if c not in have] == [], "a list entry without a kernel"


def _backward(J, X, R):
    return float(np.abs(np.matmul(J, X) - R).max() / max(1.0, np.abs(R).max()))


def _accuracy(tw, seed, what):
    """(forward, backward) figures of the numpy reference on the twin's problem, asserted against TOL_FORWARD / TOL_BACKWARD"""
    o = tw[0][0]
    R = K.user_columns(len(tw), o.S, seed)
    fwd = bwd = 0.0
    for reg in K.REGS:
        J = K.jacobians(tw, reg)
        rhs = [R] + [PR.analytic_rhs(tw, param)[0] for param in ("Q", "collision_radius", "control_bound") if param in PR.carried(o)]
        sol = K.solve_ref(J, np.concatenate(rhs, axis=2))                # (one factorisation per game serves every column)
        X, at = sol[:, :, :R.shape[2]], 0
        fwd = max(fwd, K.col_err(X, K.refine_ld(J, R, X)))
        for Rp in rhs:                                                   # the backward figure of each kind against its own max |R|
            bwd = max(bwd, _backward(J, sol[:, :, at:at + Rp.shape[2]], Rp))
            at += Rp.shape[2]
    assert fwd <= TOL_FORWARD, (what, fwd)
    assert bwd <= TOL_BACKWARD, (what, bwd)
    return fwd, bwd


def _rhs_check(tw, what, tally):
    """every column of analytic_rhs against fd_rhs at PR.steps / PR.bound, flips == 0; tally: worst / nonzero / rows, added to"""
    o = tw[0][0]
    for param in CHECKED:                              # (control_bound is the last: it moves the batches' bounds)
        if param not in PR.carried(o):
            continue
        if param == "control_bound":
            PR.move_bounds(tw)
        h = PR.steps(o, param)
        if param in PR.PARAMS[5:]:
            assert PR.flips(tw, param, h) == 0, (what, param)
        ana, act = PR.analytic_rhs(tw, param)
        fd = PR.fd_rhs(tw, param, h)
        top = np.abs(ana).max()
        for c in range(ana.shape[2]):
            err = np.abs(fd[:, :, c] - ana[:, :, c]).max()
            tally["worst"][param] = max(tally["worst"].get(param, 0.0), err / top if top > 0 else err)
            assert err <= PR.bound(o, param, c) * top, (what, param, c, err, top)
        tally["nonzero"][param] = tally["nonzero"].get(param, 0) + int(np.any(ana != 0, axis=(0, 1)).sum())
        if param in ("collision_radius", "control_bound"):
            r = tally["rows"].setdefault(param, [0, 0])                # [inactive, active]
            r[0] += act.count(0.0); r[1] += act.count(1.0)


def _tally():
    return dict(worst={}, nonzero={}, rows={})


def _tally_ok(t, what):
    print(what, "worst |fd - analytic| / max |R|:", {k: "%.1e" % v for k, v in t["worst"].items()}, "rows [inactive, active]:", t["rows"])
    assert all(v > 0 for v in t["nonzero"].values()), (what, t["nonzero"])
    for k, (off, on) in t["rows"].items():
        assert off > 0 and on > 0, (what, k, off, on)


@pytest.mark.parametrize("cfg", F.CONFIGS, ids=F.IDS)
def test_numpy_reference_on_every_configuration(orc, cfg):
    worst = [0.0, 0.0]
    for N in F.HORIZONS:
        _, tw = F.pair_problem(_as_product(orc), orc, cfg, N)
        assert len(tw) == F.B
        f, b = _accuracy(tw, N, (cfg, N))
        worst = [max(worst[0], f), max(worst[1], b)]
    print("reference", F.cfg_id(cfg), "forward %.2e backward %.2e" % tuple(worst))


@pytest.mark.parametrize("cfg", F.CONFIGS, ids=F.IDS)
def test_analytic_right_hand_sides_on_every_configuration(orc, cfg):
    t = _tally()
    for N in F.HORIZONS:
        _, tw = F.pair_problem(_as_product(orc), orc, cfg, N)
        o = tw[0][0]
        assert PR.carried(o) == (PR.PARAMS if cfg[1] > 1 else PR.PARAMS[:5] + ("control_bound",)), (cfg, PR.carried(o))
        _rhs_check(tw, (cfg, N), t)
    _tally_ok(t, F.cfg_id(cfg))


@pytest.mark.parametrize("case", F.PER_GAME, ids=[F.per_game_id(c) for c in F.PER_GAME])
def test_per_game_problems(orc, case):
    """The oracle twins of the per-game problems (one OracleBatch(B = 1) per game; the same twin serves both kernel modes): the two checks
    above, and the check can fail -- another game's numbers give another right-hand side."""
    case = case[:4]
    t = _tally()
    for N in F.PER_GAME_HORIZONS:
        data = F.PerGame(orc, case, N)
        tw = data.twin(orc)
        assert len({id(o) for o, _ in tw}) == data.B and all(o.B == 1 for o, _ in tw)
        f, b = _accuracy(tw, N, (case, N))
        print("reference", case, N, "forward %.2e backward %.2e" % (f, b))
        for param in F.PER_GAME_KINDS:
            if param not in PR.carried(tw[0][0]):
                assert case[0] == F.QUAD and param == "collision_radius"
                continue
            for k in range(1, data.B):
                o = tw[k][0]
                own, _ = PR.analytic_rhs_game(o, 0, param)
                with F.with_numbers_of(o, tw[0][0], param):
                    other, _ = PR.analytic_rhs_game(o, 0, param)
                assert np.abs(own).max() > 0, (case, N, param, k, "the game has no term of this kind")
                gap = np.abs(own - other).max(axis=0) / np.abs(own).max()
                assert gap.max() > 1e-3, (case, N, param, k, gap.max())
        _rhs_check(tw, (case, N), t)
    _tally_ok(t, case)


@pytest.mark.parametrize("case", PAIR_CASES, ids=["%s%d_d%d" % (("di", "uni")[c[0]], c[1], c[2]) for c in PAIR_CASES])
def test_partial_pair_tables(orc, case):
    """The handles of test_gpu_parity.PAIR_CASES at N = 5: the two checks; the recorded table has the listed pairs and no other."""
    _, tw, pairs = F.pair_table_problem(_as_product(orc), orc, case)
    o = tw[0][0]
    num = PR.numbers(o, 0)
    assert {(i, j) for i, j in zip(*np.nonzero(num["on"]))} == {(i, j) for i, j, _ in pairs}
    assert all(num["pair"][i, j] == r for i, j, r in pairs) and np.all(num["pair"][~num["on"]] == 0)
    assert getattr(o, "_dims", 2) == (3 if case[5] else 2)
    f, b = _accuracy(tw, 5, case[:3])
    print("reference", case[:3], "forward %.2e backward %.2e" % (f, b))
    t = _tally()
    _rhs_check(tw, case[:3], t)
    R, _ = PR.analytic_rhs(tw, "collision_radius")
    live = np.any(R != 0, axis=(0, 1)).reshape(o.p, o.p)
    assert np.array_equal(live, num["on"]), (case[:3], live)           # every added pair has a non-zero column, no other has
    print(case[:3], "worst |fd - analytic| / max |R|:", {k: "%.1e" % v for k, v in t["worst"].items()})
