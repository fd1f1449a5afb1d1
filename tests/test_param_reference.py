"""The preconditions of tests/test_gpu_param_sensitivity.py, on the CPU: the REFERENCE of the parameter sensitivities (oracle + numpy), the C ABI
and the Python argument checks of alg_kkt_sensitivity (the metadata of its kernel: tests/test_kkt_solve_build.py).  No GPU needed.

  * the right-hand sides R = -d res / d theta written down on the host (param_reference.analytic_rhs) equal central differences of the
    oracle's residual, for xf and every new parameter, on the random data of the parity tests (pair_problem) and on solved family games, all
    nine shapes over their horizons, four games.  Bounds: 1e-12 max |R| where the residual is affine in the entry (the bound of the XF
    test), 1e-8 max |R| for the two radii (quadratic in R_ij, affine in r_i inside an active set: only the rounding eps |term| / h remains).
    Every column is held to these two bounds.  One power-of-two step per kind (param_reference.steps gives the reasons): 2^10 where the
    residual is affine everywhere (at step 1 the rounding of the oracle's residual on solved games with penalties at their ceiling is the
    whole bound), 2^-11 for r_i and 2^-16 for R_ij, 1 for the control bounds.  The control bounds are checked on both problem sets with the bounds
    moved to +-3 (param_reference.move_bounds): at the problems' own bounds rows with lambda = 0 sit closer to c = 0 than any step that
    meets 1e-12, at +-3 a step of 1 crosses none (every control lies in [-1, 1]); the host-written right-hand side is evaluated at the
    same moved bounds.
    Asserted, not measured: no row's activity and no pair's r_i - |d| > 0 differs between theta + h and theta - h, with no column left out;
    over a shape's problems every kind has a non-zero column, and the pair radii and the control bounds see active and inactive rows
    (both problem sets supply both: rows with lambda > 0 or c >= 0, and rows with lambda = 0 and c < 0).  The activity is the oracle's:
    orc_kat_evaluate_con's values with the multipliers, orc_kat_collision_cost per pair (param_reference.flips);
  * on the double integrator (3 players N = 6, 2 players N = 4) the reference X = J^-1 R of one column per new parameter is the derivative of
    the polished root, as test_kkt_sensitivity_family._x0_gap shows for x0: 1e-7 max |X|."""
import ctypes
import os
import re

import numpy as np
import pytest

import kkt_reference as K
import param_reference as PR
import test_gpu_horizon_shapes as HS
from test_kkt_sensitivity_family import _as_product, _make, _polish

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "algames_hip.h")
CHECKED = ("xf",) + PR.NEW


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_analytic_right_hand_sides_equal_oracle_differences(orc, name):
    nonzero = {k: 0 for k in CHECKED}
    rows = {k: [0, 0] for k in ("collision_radius", "control_bound")}          # [inactive, active]
    worst = {k: 0.0 for k in CHECKED}
    for N in K.horizons(name):
        _, tw_pair = PR.pair_problem(_as_product(orc), orc, name, N)
        fam = PR.family_problem(_make(orc), name, N)
        fam.newton_solve(init=True, game_id0=HS.GID0)
        for what, tw in (("pair", tw_pair), ("family", K.twin_of(fam))):
            o = tw[0][0]
            for param in CHECKED:                      # (control_bound is the last: it moves the batch's bounds)
                if param == "control_bound":
                    PR.move_bounds(tw)
                h = PR.steps(o, param)
                if param in PR.PARAMS[5:]:
                    assert PR.flips(tw, param, h) == 0, (name, N, what, param)
                ana, act = PR.analytic_rhs(tw, param)
                fd = PR.fd_rhs(tw, param, h)
                top = np.abs(ana).max()
                for c in range(ana.shape[2]):
                    err = np.abs(fd[:, :, c] - ana[:, :, c]).max()
                    worst[param] = max(worst[param], err / top if top > 0 else err)
                    assert err <= PR.bound(o, param, c) * top, (name, N, what, param, c, err, top)
                nonzero[param] += int(np.any(ana != 0, axis=(0, 1)).sum())
                if param in rows:
                    rows[param][0] += act.count(0.0); rows[param][1] += act.count(1.0)
    print(name, "worst |fd - analytic| / max |R|:", {k: "%.1e" % v for k, v in worst.items()}, "rows [inactive, active]:", rows)
    assert all(v > 0 for v in nonzero.values()), (name, nonzero)
    for k, (off, on) in rows.items():
        assert off > 0 and on > 0, (name, k, off, on)


def _root_gap(orc, model, p, d, N, param):
    """max |X reference - central difference of polished re-solves| / max |X reference| of one column of `param`: the first column whose
    right-hand side is not zero on some game (column 0 if there is none: reference and difference are then both exactly zero).  h = 1e-5 as
    in _x0_gap; uf takes 1e-3: with the active set held the root is affine in uf, so the quotient has no truncation error at any step, and
    what remains is the polish tolerance over h -- against sensitivities of 3e-4 (control targets weighted 0.1 barely move the plan) the
    step of 1e-5 leaves 2e-7 of it."""
    h = 1e-3 if param == "uf" else 1e-5
    with PR.recorded():
        o = HS.family(lambda *a: K.recording(_make(orc)(*a)), model, p, d, N, **HS.TUNED.get((model, p, d), {}))
    o.newton_solve(init=True, game_id0=HS.GID0)
    _polish(o)
    tw = K.twin_of(o)
    R, _ = PR.analytic_rhs(tw, param)
    live = np.flatnonzero(np.any(R != 0, axis=(0, 1)))
    c = int(live[0]) if len(live) else 0
    X = K.solve_ref(K.jacobians(tw, 0.0), R[:, :, c:c + 1])[:, :, 0]
    z0 = o.get_traj()
    zz = []
    for s in (h, -h):
        PR._moved(o, param, c, s)
        o.set_traj(z0)
        _polish(o)
        zz.append(o.get_traj()[:, o.n:])
    PR._apply(o, o._num)
    fd = (zz[0] - zz[1]) / (2 * h)
    top = np.abs(X).max()
    return (np.abs(X - fd).max() / top if top > 0 else np.abs(fd).max()), c, top


@pytest.mark.parametrize("param", PR.NEW)
@pytest.mark.parametrize("cfg,N", [((K.DI, 3, 2), 6), ((K.DI, 2, 2), 4)], ids=["di3_N6", "di2_N4"])
def test_reference_is_the_derivative_of_the_root_on_the_double_integrator(orc, cfg, N, param):
    gap, c, top = _root_gap(orc, *cfg, N, param)
    print("reference against central differences of polished roots", cfg, N, param, "column %d: %.2e max|X| (max |X| = %.2e)" % (c, gap, top))
    assert gap <= 1e-7, (cfg, N, param, c, gap)


# ---- the C ABI, the Python layers, the kernels ---------------------------------------------------------------------------------------------------------------
def _lib_path(alg):
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    return alg.HIP_LIB_PATH


def test_the_header_declares_and_the_library_exports_the_entry_points(alg):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = ("X0", "XF", "Q", "R", "UF", "COLLISION_COST", "COLLISION_RADIUS", "CONTROL_BOUND")
    for val, name in enumerate(names):
        assert re.search(r"#define\s+ALG_PARAM_%s\s+%d\b" % (name, val), txt)
        assert getattr(alg._abi, "ALG_PARAM_" + name) == val and getattr(alg, "ALG_PARAM_" + name) == val
    assert [k.upper() for k in alg._abi.PARAM_KINDS] == list(names)
    assert re.search(r"int\s+alg_param_len\s*\(\s*alg_handle\s*\*\s*h\s*,\s*int32_t\s+param\s*,\s*int32_t\s*\*\s*len\s*\)", txt)
    assert re.search(r"int\s+alg_kkt_sensitivity\s*\(\s*alg_handle\s*\*\s*h\s*,\s*double\s+reg\s*,\s*int32_t\s+param\s*,\s*int32_t\s+ndir\s*,\s*const\s+double\s*\*\s*dirs\s*,"
                     r"\s*int32_t\s+first_game\s*,\s*int32_t\s+n_games\s*,\s*int32_t\s+first_step\s*,\s*int32_t\s+n_steps\s*,\s*double\s*\*\s*out\s*,"
                     r"\s*int32_t\s*\*\s*status\s*\)", txt)
    dll = ctypes.CDLL(_lib_path(alg))                # loads without a GPU; no compute call is made
    for f in ("param_len", "kkt_sensitivity"):
        assert hasattr(dll, "alg_" + f)
        assert f in alg._abi.SIGNATURES and f in alg._abi.OPTIONAL and f not in alg.hip_lib().absent
        getattr(dll, "alg_" + f).argtypes = alg._abi.SIGNATURES[f][1]
    v = ctypes.c_int32(7)
    assert dll.alg_param_len(None, 0, ctypes.byref(v)) == alg._abi.ALG_ERR_ARG and v.value == 7       # a null handle is refused before any device call
    assert dll.alg_kkt_sensitivity(None, 0.0, 0, 0, None, 0, 1, 0, 0, None, None) == alg._abi.ALG_ERR_ARG
    for f in ("parameter_sensitivity", "EquilibriumSensitivity"):
        assert hasattr(alg, f), f


def test_python_argument_validation(alg, orc):
    """Batch.kkt_sensitivity and host.parameter_sensitivity refuse a wrong parameter, range, shape or value before any library call (on an
    oracle-backed batch, which needs no GPU: the oracle has no counterpart of the entry points, so a call that got through says so)."""
    b = orc.OracleBatch(0, 3, 6, 0.1, 2)
    for bad in ("radius", 8, -1, True, 1.5, None):
        with pytest.raises(ValueError, match="unknown parameter"):
            b.kkt_sensitivity(bad)
    for games in ((-1, 1), (0, 0), (1, 2), (2, 1)):
        with pytest.raises(ValueError, match="games"):
            b.kkt_sensitivity("Q", games=games)
    for steps in ((-1, 1), (0, 0), (0, 6), (4, 2), (5, 1)):
        with pytest.raises(ValueError, match="steps"):
            b.kkt_sensitivity("Q", steps=steps)
    ln = 3 * 4
    for bad in (np.zeros((3, 1, ln)), np.zeros((2, 1, ln + 1)), np.zeros((2, 0, ln)), np.zeros(ln), np.zeros((2, 1, 1, ln))):
        with pytest.raises(ValueError, match="expected shape"):
            b.kkt_sensitivity("Q", dirs=bad)
    for v in (np.nan, np.inf):
        d = np.zeros((2, 2, ln)); d[1, 1, ln - 1] = v
        with pytest.raises(ValueError, match="finite"):
            b.kkt_sensitivity("Q", dirs=d)
    for call in (lambda: b.kkt_sensitivity("Q"), lambda: b.kkt_sensitivity(7, steps=(4, 1), games=(1, 1)), lambda: b.kkt_sensitivity("xf", dirs=np.zeros((2, ln))),
                 lambda: b.param_len("uf")):
        with pytest.raises(alg.AlgamesError, match="no orc_(kkt_sensitivity|param_len)"):
            call()
    assert [b._param_len(c) for c in range(8)] == [12, 12, 12, 6, 6, 6, 9, 12]

    class P:                                          # the part of a GameProblem the host functions touch
        batch = b

        def _sync_options(self):
            pass
    with pytest.raises(ValueError, match="wrt must be"):
        alg.parameter_sensitivity(P(), wrt="radius")
    with pytest.raises(ValueError, match="wrt must be"):
        alg.parameter_sensitivity(P(), wrt=2)
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_sensitivity"):
        alg.parameter_sensitivity(P(), "collision_radius", steps=(0, 1))


def test_sliced_sensitivity_accessors(alg):
    """EquilibriumSensitivity over a step slice: the accessors address the rows of the steps it holds and raise IndexError outside them"""
    N, p, n, mi, q = 6, 3, 12, 2, 4
    bl = n + p * mi + p * n
    full = np.arange(2 * (N - 1) * bl * q, dtype=np.float64).reshape(2, (N - 1) * bl, q)
    whole = alg.EquilibriumSensitivity(full, np.zeros(2, dtype=np.int32), "Q", N, n, p, mi)
    s0, ns = 1, 2
    part = alg.EquilibriumSensitivity(full[:, s0 * bl:(s0 + ns) * bl], np.zeros(2, dtype=np.int32), "Q", N, n, p, mi, steps=(s0, ns))
    assert whole.steps == (0, N - 1) and part.steps == (s0, ns)
    for step in range(s0, s0 + ns):
        assert np.array_equal(part.dx(step + 2), whole.dx(step + 2)) and np.array_equal(part.du(step + 1), whole.du(step + 1))
        for i in range(1, p + 1):
            assert np.array_equal(part.du(step + 1, i), whole.du(step + 1, i)) and np.array_equal(part.dλ(step + 1, i), whole.dλ(step + 1, i))
    for bad in (lambda: part.dx(2), lambda: part.dx(5), lambda: part.du(1), lambda: part.du(4), lambda: part.dλ(1, 1), lambda: part.dλ(4, 2),
                lambda: part.dx(1), lambda: part.dx(N + 1), lambda: part.du(N), lambda: part.du(2, 4)):
        with pytest.raises(IndexError):
            bad()

