"""CPU-side checks of the normal equations of a fit (alg_kkt_normal_equations): the C ABI declares and exports the entry point, the Python layers
refuse wrong arguments before any device call, k_sens_gram uses no scratch and spills nothing, and the fit families of tests/normal_family.py
hold their preconditions on the oracle -- coupled players, a well-conditioned X' W X, and a reference Levenberg-Marquardt loop
(normal_reference.lm_twin) that recovers theta_true.  No GPU needed."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import normal_family as F
import normal_reference as NR
import param_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "algames_hip.h")


def _lib_path(alg):
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    return alg.HIP_LIB_PATH


def test_the_header_declares_and_the_library_exports_the_entry_point(alg):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+ALG_NORMAL_MAX_COLS\s+63\b", txt) and alg.ALG_NORMAL_MAX_COLS == 63
    sig = (r"int\s+alg_kkt_normal_equations\s*\(\s*alg_handle\s*\*\s*h\s*,\s*double\s+reg\s*,\s*int32_t\s+ncol\s*,\s*const\s+int32_t\s*\*\s*col_param\s*,"
           r"\s*const\s+int32_t\s*\*\s*col_index\s*,\s*const\s+double\s*\*\s*target\s*,\s*const\s+double\s*\*\s*weight\s*,\s*int32_t\s+per_game_weight\s*,"
           r"\s*int32_t\s+first_game\s*,\s*int32_t\s+n_games\s*,\s*double\s*\*\s*H\s*,\s*double\s*\*\s*g\s*,\s*double\s*\*\s*loss\s*,\s*int32_t\s*\*\s*status\s*\)")
    assert re.search(sig, txt)
    dll = ctypes.CDLL(_lib_path(alg))                # loads without a GPU; no compute call is made
    assert hasattr(dll, "alg_kkt_normal_equations")
    assert "kkt_normal_equations" in alg._abi.SIGNATURES and "kkt_normal_equations" in alg._abi.OPTIONAL and "kkt_normal_equations" not in alg.hip_lib().absent
    dll.alg_kkt_normal_equations.argtypes = alg._abi.SIGNATURES["kkt_normal_equations"][1]
    assert dll.alg_kkt_normal_equations(None, 0.0, 1, None, None, None, None, 0, 0, 1, None, None, None, None) == alg._abi.ALG_ERR_ARG
    for f in ("normal_equations", "fit_parameters", "normal_columns", "NormalEquations", "FitResult"):
        assert hasattr(alg, f), f


def test_python_argument_validation(alg, orc):
    """Batch.kkt_normal_equations, host.normal_equations and host.fit_parameters refuse wrong arguments before any library call (on an
    oracle-backed batch, which needs no GPU: the oracle has no counterpart of the entry point, so a call that got through says so)."""
    b = orc.OracleBatch(0, 3, 6, 0.1, 2)
    S = b.S
    t, w = np.zeros((2, S)), np.ones(S)
    ok = [("xf", 0), ("Q", 3)]
    with pytest.raises(ValueError, match="1 ... 63 columns"):
        b.kkt_normal_equations([], t, w)
    with pytest.raises(ValueError, match="1 ... 63 columns"):
        b.kkt_normal_equations([("x0", i % 12) for i in range(64)], t, w)
    with pytest.raises(ValueError, match="unknown parameter"):
        b.kkt_normal_equations([("goal", 0)], t, w)
    for bad in (("xf", 12), ("xf", -1), ("R", 6), ("collision_cost", 6), ("xf", 1.5), ("xf", True)):
        with pytest.raises(ValueError, match="index must be"):
            b.kkt_normal_equations([bad], t, w)
    with pytest.raises(ValueError, match="pair"):
        b.kkt_normal_equations(["xf"], t, w)
    with pytest.raises(ValueError, match="duplicate"):
        b.kkt_normal_equations([("xf", 1), ("Q", 1), (1, 1)], t, w)
    for bad in (np.zeros((3, S)), np.zeros((2, S + 1)), np.zeros(S)):
        with pytest.raises(ValueError, match="target: expected shape"):
            b.kkt_normal_equations(ok, bad, w)
    for bad in (np.nan, np.inf):
        tt = t.copy(); tt[1, S - 1] = bad
        with pytest.raises(ValueError, match="target must be finite"):
            b.kkt_normal_equations(ok, tt, w)
    for bad in (np.ones(S + 1), np.ones((3, S)), np.ones((2, 1, S))):
        with pytest.raises(ValueError, match="weight: expected shape"):
            b.kkt_normal_equations(ok, t, bad)
    for bad in (np.nan, np.inf, -1.0):
        ww = w.copy(); ww[0] = bad
        with pytest.raises(ValueError, match="weight must be finite"):
            b.kkt_normal_equations(ok, t, ww)
    for bad in ((-1, 1), (0, 0), (1, 2), (2, 1)):
        with pytest.raises(ValueError, match="inside the batch"):
            b.kkt_normal_equations(ok, t, w, games=bad)
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_normal_equations"):
        b.kkt_normal_equations(ok, t, w)
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_normal_equations"):
        b.kkt_normal_equations(ok, t[:1], np.ones((1, S)), games=(1, 1))

    class P:                                          # the part of a GameProblem the host functions touch
        batch = b

        def _sync_options(self):
            pass
    assert alg.normal_columns(b, "uf") == [("uf", i) for i in range(6)]
    assert alg.normal_columns(b, (("Q", (5, 2)), "x0", ("R", 1))) == [("Q", 5), ("Q", 2)] + [("x0", i) for i in range(12)] + [("R", 1)]
    with pytest.raises(ValueError, match="wrt must name"):
        alg.normal_equations(P(), t, ("goal",))
    with pytest.raises(ValueError, match="observed: expected"):
        alg.normal_equations(P(), np.zeros((2, S - 1)), ("xf",))
    with pytest.raises(ValueError, match="observed: expected"):
        alg.normal_equations(P(), (np.zeros((2, 6, 12)), np.zeros((2, 6, 6))), ("xf",))
    with pytest.raises(ValueError, match="weight: expected shape"):
        alg.normal_equations(P(), t, ("xf",), weight=np.ones((3, S)), max_scratch_bytes=1)
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_normal_equations"):
        alg.normal_equations(P(), (np.zeros((2, 6, 12)), np.zeros((2, 5, 6))), ("xf", ("Q", [0])), max_scratch_bytes=1)
    with pytest.raises(ValueError, match="fit_parameters: wrt must name"):
        alg.fit_parameters(P(), t, ("x0",))
    with pytest.raises(ValueError, match="iters must be"):
        alg.fit_parameters(P(), t, ("xf",), iters=-1)
    w0 = alg.default_fit_weight(b)
    X, U, L = b.split_traj(np.concatenate([np.zeros((1, b.n)), w0[None]], axis=1))
    assert np.all(X[:, 1:] == 1) and np.all(U == 1) and np.all(L == 0)


def test_the_reduction_kernel_uses_no_scratch_and_spills_nothing(alg):
    spec = importlib.util.spec_from_file_location("_resources", os.path.join(ROOT, "algames.jl_amd", "_resources.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.kernel_resources(_lib_path(alg))
    mine = {k: v for k, v in res.items() if k.startswith("k_sens_gram")}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    print(name, v)
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, v


def test_the_reference_statement_and_its_bound():
    """gram() against a plain float64 evaluation in another summation order: inside the derived bound (the bound covers any order of the S
    terms), and H symmetric"""
    rng = np.random.default_rng(5)
    B, q, S = 3, 7, 61
    X, z, t = rng.standard_normal((B, q, S)) * 10.0 ** rng.integers(-3, 4, (B, q, 1)), rng.standard_normal((B, S)), rng.standard_normal((B, S))
    w = rng.uniform(0.0, 2.0, S); w[::5] = 0.0
    ref = NR.gram(X, z, t, w)
    r = z - t
    H = np.einsum("bcs,bds->bcd", X[:, :, ::-1] * w[::-1], X[:, :, ::-1])
    g = np.einsum("bcs,bs->bc", X[:, :, ::-1] * w[::-1], r[:, ::-1])
    loss = 0.5 * np.einsum("bs,bs->b", r * w, r)
    frac = NR.assert_parity((H, g, loss), ref, "float64 in reverse order")
    print("float64 against long double: %.3f of the bound" % frac)
    assert np.array_equal(ref[0], ref[0].transpose(0, 2, 1))
    with pytest.raises(AssertionError):
        NR.assert_parity((H * (1 + 1e-12), g, loss), ref, "a relative error of 1e-12 is outside")


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_family_preconditions_and_the_reference_fit(alg, orc, name):
    """On the oracle: every game is solved, its players are coupled through the collision cost, X' W X at theta_true is well conditioned
    (COND, factor 10), and the reference loop from theta_0 has a non-increasing loss and ends within 1e-3 |theta_0 - theta_true|_inf of
    theta_true -- E_REF of the family, which the GPU test multiplies by 10."""
    make = lambda *a: orc.OracleBatch(*a[:5], d=a[5])
    num = F.numbers(name)
    with PR.recorded():
        o = F.batch(make, name, num)
    st = o.newton_solve(init=True)
    assert np.all(st["converged"] == 1) and np.all(st["status"] == 0), st
    z = o.get_traj()
    X, _, _ = o.split_traj(z)
    p, rad = o.p, num["cc"][0]
    for g in range(F.B):
        active = [rad[i] - np.hypot(X[g, k, i] - X[g, k, j], X[g, k, p + i] - X[g, k, p + j]) > 0 for k in range(1, F.N) for i in range(p) for j in range(p) if i != j]
        assert any(active), (name, g)
    cols = F.columns(name)
    assert cols == alg.normal_columns(o, F.FAMILIES[name]["wrt"])
    w = alg.default_fit_weight(o)
    target = z[:, o.n:].copy()
    H = NR.gram(NR.oracle_columns(o, cols), target, target, w)[0]
    cond = max(float(np.linalg.cond(h)) for h in H)
    print(name, "condition number of X' W X: %.3g (recorded %.3g)" % (cond, F.COND[name]))
    assert np.isfinite(cond) and F.COND[name] / 10 <= cond <= F.COND[name] * 10
    true, th0 = F.start(name)
    n0 = F.with_theta(name, th0)
    with PR.recorded():
        o2 = F.batch(make, name, n0)
    fit = NR.OracleFit(o2, (n0["Q"], n0["R"], n0["xf"], n0["uf"]), cols, target, w)
    positive = np.array([k in ("Q", "R") for k, _ in cols])
    th, hist, acc = NR.lm_twin(th0, positive, fit.evaluate, fit.save, fit.restore, iters=F.ITERS)
    e0, e_ref = np.abs(th0 - true).max(), np.abs(th - true).max()
    print(name, "e_0 %.3g e_ref %.3g (recorded %.3g) accepted steps %s" % (e0, e_ref, F.E_REF[name], acc.sum(axis=0)))
    assert np.all(np.diff(hist, axis=0) <= 0) and np.all(acc.sum(axis=0) >= 1)
    assert e_ref <= 1e-3 * e0, (name, e_ref, e0)
    assert e_ref <= F.E_REF[name] * 2, (name, e_ref)             # the recorded constant is this run's figure (2: another LAPACK build)
