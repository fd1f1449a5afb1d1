"""CPU-side checks of the KKT solves with many right-hand sides (alg_kkt_solve): the C ABI declares and exports the entry point, the Python
layers refuse wrong arguments before any device call, every configuration that has a k_direction<...> kernel has its KKT column kernel k_kkt_sens<...> (the one
kernel of alg_kkt_solve, alg_kkt_sensitivity and alg_kkt_normal_equations) with the resources of that k_direction, and the solver kernels k_newton_solve* / k_mpc_loop* keep the metadata they had before the feature, entry for
entry (tests/golden/solver_kernel_resources_parent.json: a build of the commit before it).  No GPU needed."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "algames_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "solver_kernel_resources_parent.json")
_RES = {}


def _lib_path(alg):
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    return alg.HIP_LIB_PATH


def _resources(alg):
    if not _RES:
        spec = importlib.util.spec_from_file_location("_resources", os.path.join(ROOT, "algames.jl_amd", "_resources.py"))
        mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
        _RES.update(mod.kernel_resources(_lib_path(alg)))
    return _RES


def test_the_header_declares_and_the_library_exports_the_entry_point(alg):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, val in (("ALG_KKT_RHS_USER", 0), ("ALG_KKT_RHS_X0", 1), ("ALG_KKT_RHS_XF", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt)
        assert getattr(alg._abi, name) == val and getattr(alg, name) == val
    assert re.search(r"int\s+alg_kkt_solve\s*\(\s*alg_handle\s*\*\s*h\s*,\s*double\s+reg\s*,\s*int32_t\s+kind\s*,\s*int32_t\s+nrhs\s*,\s*const\s+double\s*\*\s*rhs\s*,"
                     r"\s*int32_t\s+first_game\s*,\s*int32_t\s+n_games\s*,\s*double\s*\*\s*out\s*,\s*int32_t\s*\*\s*status\s*\)", txt)
    dll = ctypes.CDLL(_lib_path(alg))                # loads without a GPU; no compute call is made
    assert hasattr(dll, "alg_kkt_solve")
    assert "kkt_solve" in alg._abi.SIGNATURES and "kkt_solve" in alg._abi.OPTIONAL and "kkt_solve" not in alg.hip_lib().absent
    dll.alg_kkt_solve.argtypes = alg._abi.SIGNATURES["kkt_solve"][1]
    assert dll.alg_kkt_solve(None, 0.0, 0, 1, None, 0, 1, None, None) == alg._abi.ALG_ERR_ARG      # a null handle is refused before any device call
    for f in ("kkt_solve", "equilibrium_sensitivity", "feedback_gains", "EquilibriumSensitivity"):
        assert hasattr(alg, f), f


def test_python_argument_validation(alg, orc):
    """Batch.kkt_solve and host.equilibrium_sensitivity refuse a wrong kind, shape or combination before any library call (on an oracle-backed
    batch, which needs no GPU: the oracle has no counterpart of the entry point, so a call that got through says so)."""
    b = orc.OracleBatch(0, 3, 6, 0.1, 2)
    S = b.S
    with pytest.raises(ValueError, match="unknown right-hand-side kind"):
        b.kkt_solve(np.zeros((2, 1, S)), kind="uf")
    with pytest.raises(ValueError, match="needs rhs"):
        b.kkt_solve(None, kind="user")
    for bad in (np.zeros((3, 1, S)), np.zeros((2, 1, S + 1)), np.zeros((2, 0, S)), np.zeros(S)):
        with pytest.raises(ValueError, match="expected shape"):
            b.kkt_solve(bad)
    with pytest.raises(ValueError, match="only taken with kind='user'"):
        b.kkt_solve(np.zeros((2, 1, S)), kind="x0")
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_solve"):
        b.kkt_solve(np.zeros((2, 1, S)))
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_solve"):
        b.kkt_solve(kind="xf", games=(1, 1))

    class P:                                          # the part of a GameProblem the host functions touch
        batch = b

        def _sync_options(self):
            pass
    with pytest.raises(ValueError, match="wrt must be"):
        alg.equilibrium_sensitivity(P(), wrt="uf")
    with pytest.raises(alg.AlgamesError, match="no orc_kkt_solve"):
        alg.feedback_gains(P())


def test_sensitivity_accessors_follow_the_horizontal_index_maps(alg):
    """EquilibriumSensitivity.dx / du / dλ slice the rows horizontal_indices names (1-based stamps of the reference)."""
    N, p, n, mi, q = 4, 3, 12, [2, 2, 2], 5
    hor = alg.horizontal_indices(alg.ProblemSize(N, alg.DoubleIntegratorGame(p=p)))
    S = max(v[-1] for v in hor.values())
    dz = np.arange(2 * S * q, dtype=np.float64).reshape(2, S, q)
    s = alg.EquilibriumSensitivity(dz, np.zeros(2, dtype=np.int32), "x0", N, n, p, mi[0])
    rows = lambda st: np.array(hor[st]) - 1
    for k in range(2, N + 1):
        assert np.array_equal(s.dx(k), dz[:, rows(alg.stampify("x", 1, k))])
    for k in range(1, N):
        assert np.array_equal(s.du(k), dz[:, np.concatenate([rows(alg.stampify("u", i, k)) for i in range(1, p + 1)])])
        for i in range(1, p + 1):
            assert np.array_equal(s.du(k, i), dz[:, rows(alg.stampify("u", i, k))])
            assert np.array_equal(s.dλ(k, i), dz[:, rows(alg.stampify("λ", i, k))])
    for bad in (lambda: s.dx(1), lambda: s.dx(N + 1), lambda: s.du(N), lambda: s.du(1, 4), lambda: s.dλ(0, 1)):
        with pytest.raises(IndexError):
            bad()


def test_every_direction_kernel_has_its_kkt_solve_with_the_same_resources(alg):
    """k_kkt_sens<C>, the column kernel of all three KKT entry points, exists for every Cfg that has a k_direction<C> (base, EXT, the
    block-reading twins, the dense-direction configurations) and nowhere else (no team shape); it spills no VGPR, uses scratch only where its
    k_direction does, and has that kernel's LDS size: the loader and the sliced store add none.  No k_kkt_solve<C> is left beside it."""
    res = _resources(alg)
    dirs = {k[len("k_direction"):]: v for k, v in res.items() if k.startswith("k_direction<")}
    kkt = {k[len("k_kkt_sens"):]: v for k, v in res.items() if k.startswith("k_kkt_sens<")}
    assert len(dirs) >= 79 and sorted(kkt) == sorted(dirs)
    assert not [k for k in res if k.startswith("k_kkt_solve<")]
    for c, d in sorted(dirs.items()):
        v = kkt[c]
        print("k_kkt_sens%-24s vgpr %3d (direction %3d) sgpr %3d sgpr_spill %3d (%3d) scratch %4d (%4d) lds %6d" % (
            c, v["vgpr"], d["vgpr"], v["sgpr"], v["sgpr_spill"], d["sgpr_spill"], v["scratch"], d["scratch"], v["lds"]))
        assert v["vgpr_spill"] == 0, (c, v)
        assert v["scratch"] == 0 or d["scratch"] > 0, (c, v, d)
        assert v["lds"] == d["lds"], (c, v, d)


def test_the_solver_kernels_keep_the_parents_metadata(alg):
    """Every k_newton_solve* / k_mpc_loop* kernel of the library against a build of the commit before the feature: VGPRs, SGPRs, spills,
    scratch and LDS, entry for entry, and no kernel of these families added or gone."""
    res = _resources(alg)
    want = json.load(open(FIXTURE))
    have = {k: v for k, v in res.items() if k.startswith(("k_newton_solve", "k_mpc_loop"))}
    assert len(want) >= 290 and sorted(have) == sorted(want)
    for k, w in want.items():
        assert set(w) == {"vgpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "lds"}
        assert have[k] == w, (k, have[k], w)
