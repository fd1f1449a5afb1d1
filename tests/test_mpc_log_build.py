"""CPU-side checks of the closed-loop log and the plant disturbance of the fused receding-horizon loop (alg_mpc_solve_log,
ALG_SCHED_DISTURBANCE): the C ABI declares and exports them, the Python layers refuse wrong shapes and non-finite entries before any device
call, and the unscheduled loop kernels k_mpc_loop<...> keep the resources they had before the feature, entry for entry.  No GPU needed."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "algames_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "mpc_loop_resources_parent.json")


def _lib_path(alg):
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    return alg.HIP_LIB_PATH


def test_the_header_declares_and_the_library_exports_the_log_entry_point(alg):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+ALG_SCHED_DISTURBANCE\s+101\b", txt)
    assert re.search(r"int\s+alg_mpc_solve_log\s*\(\s*alg_handle\s*\*\s*h\s*,\s*int32_t\s+steps\s*,\s*int64_t\s+game_id0\s*,\s*double\s*\*\s*states\s*,"
                     r"\s*double\s*\*\s*controls\s*,\s*alg_game_stats\s*\*\s*stats\s*\)", txt)
    # alg_mpc_solve stays what it is
    assert re.search(r"int\s+alg_mpc_solve\s*\(\s*alg_handle\s*\*\s*h\s*,\s*int32_t\s+steps\s*,\s*int64_t\s+game_id0\s*,\s*double\s*\*\s*states\s*\)", txt)
    dll = ctypes.CDLL(_lib_path(alg))                # loads without a GPU; no compute call is made
    assert hasattr(dll, "alg_mpc_solve_log") and hasattr(dll, "alg_mpc_solve")
    assert alg._abi.ALG_SCHED_DISTURBANCE == 101 and alg.ALG_SCHED_DISTURBANCE == 101
    assert "mpc_solve_log" in alg._abi.SIGNATURES and "mpc_solve_log" not in alg.hip_lib().absent
    # a null handle is refused before any device call
    assert dll.alg_mpc_solve_log(None, 3, 0, None, None, None) == alg._abi.ALG_ERR_ARG
    assert dll.alg_mpc_set_schedule(None, 101, 1, None) == alg._abi.ALG_ERR_ARG
    assert dll.alg_mpc_get_schedule(None, 101, None) == alg._abi.ALG_ERR_ARG


def test_python_shape_and_finiteness_validation(alg, orc):
    """Batch.mpc_set_schedule("disturbance") and host.mpc_rollout refuse wrong shapes and non-finite entries before any library call (checked
    on an oracle-backed batch, which needs no GPU: the oracle has neither entry point, so a call that got through would say so)."""
    b = orc.OracleBatch(1, 3, 6, 0.1, 2)
    n = 12
    assert b._sched_kind("disturbance") == (101, n) and b._sched_kind(101) == (101, n)
    for bad in (np.zeros((2, n)), np.zeros((2, 3, n)), np.zeros((2, 2, n + 1)), np.zeros((0, 2, n))):
        with pytest.raises(ValueError, match="expected shape"):
            b.mpc_set_schedule("disturbance", bad)
    for v in (np.nan, np.inf, -np.inf):
        w = np.zeros((3, 2, n)); w[2, 1, 5] = v
        with pytest.raises(ValueError, match=r"finite \(row 2\)"):
            b.mpc_set_schedule("disturbance", w)
    with pytest.raises(alg.AlgamesError, match="no orc_mpc_set_schedule"):
        b.mpc_set_schedule("disturbance", np.zeros((3, 2, n)))
    with pytest.raises(alg.AlgamesError, match="no orc_mpc_solve_log"):
        b.mpc_solve_log(2)

    class P:                                          # the part of a GameProblem mpc_rollout touches before it validates
        batch = b
    with pytest.raises(ValueError, match="disturbance: expected shape"):
        alg.mpc_rollout(P, 3, disturbance=np.zeros((2, 5, n)))
    with pytest.raises(ValueError, match="disturbance: expected shape"):
        alg.mpc_rollout(P, 3, disturbance=np.zeros((2, n)))
    w = np.zeros((2, 2, n)); w[1, 0, 0] = np.nan
    with pytest.raises(ValueError, match="disturbance: every entry must be finite"):
        alg.mpc_rollout(P, 3, disturbance=w)
    with pytest.raises(ValueError, match="steps must be >= 1"):
        alg.mpc_rollout(P, 0)
    with pytest.raises(ValueError, match="unknown schedule kind"):
        alg.mpc_rollout(P, 3, schedule={"target": np.zeros((2, 2, 18))})
    with pytest.raises(ValueError, match="expected shape"):
        alg.mpc_rollout(P, 3, schedule={"lqr_target": np.zeros((2, 5, 18))})
    # the disturbance is no key of `schedule`, for mpc_rollout and mpc_solve alike
    for f in (alg.mpc_rollout, alg.mpc_solve):
        with pytest.raises(ValueError, match="`disturbance` argument"):
            f(P, 3, schedule={"disturbance": np.zeros((2, 2, n))})


def test_the_unscheduled_loop_kernels_keep_their_resources(alg):
    """Every k_mpc_loop<...> kernel of the library against tests/golden/mpc_loop_resources_parent.json, taken from a build of the commit
    before the feature: VGPRs, SGPRs, spills, scratch and LDS, entry for entry -- the per-step phases live in the siblings only."""
    spec = importlib.util.spec_from_file_location("_resources", os.path.join(ROOT, "algames.jl_amd", "_resources.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.kernel_resources(_lib_path(alg))
    want = json.load(open(FIXTURE))
    loops = {k: v for k, v in res.items() if k.startswith("k_mpc_loop<")}
    assert len(want) >= 97 and sorted(loops) == sorted(want)
    for k, w in want.items():
        assert set(w) == {"vgpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "lds"}
        assert {f: loops[k][f] for f in w} == w, (k, loops[k], w)
    # no third kernel family: the siblings carry the new phases
    assert len([k for k in res if k.startswith("k_mpc_loop_sched<")]) == len(loops)
    assert not [k for k in res if k.startswith("k_mpc_loop") and not k.startswith(("k_mpc_loop<", "k_mpc_loop_sched<"))]
    for k in sorted(loops):
        v = res[k.replace("k_mpc_loop<", "k_mpc_loop_sched<")]
        print("%-52s sgpr_spill %3d (unscheduled %3d) vgpr %3d scratch %3d" % (k.replace("k_mpc_loop<", "k_mpc_loop_sched<"), v["sgpr_spill"], loops[k]["sgpr_spill"],
                                                                               v["vgpr"], v["scratch"]))
