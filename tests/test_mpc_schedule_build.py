"""CPU-side checks of the schedules of the fused receding-horizon loop (alg_mpc_set_schedule): the C ABI declares and exports the entry
points, every loop kernel has its scheduled sibling within the resources of the unscheduled kernel (kernel metadata of the code objects
inside libalgames_hip.so), and the Python layers refuse wrong kinds and shapes.  No GPU needed."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "algames_hip.h")


def _lib_path(alg):
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    return alg.HIP_LIB_PATH


def test_the_header_declares_and_the_library_exports_the_schedule_entry_points(alg):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+ALG_SCHED_LQR_TARGET\s+100\b", txt)
    assert re.search(r"int\s+alg_mpc_set_schedule\s*\(\s*alg_handle\s*\*\s*h\s*,\s*int32_t\s+kind\s*,\s*int32_t\s+rows\s*,\s*const\s+double\s*\*\s*data\s*\)", txt)
    assert re.search(r"int\s+alg_mpc_get_schedule\s*\(\s*alg_handle\s*\*\s*h\s*,\s*int32_t\s+kind\s*,\s*int32_t\s*\*\s*rows\s*\)", txt)
    dll = ctypes.CDLL(_lib_path(alg))                # loads without a GPU; no compute call is made
    for name in ("alg_mpc_set_schedule", "alg_mpc_get_schedule"):
        assert hasattr(dll, name), name
    assert alg._abi.ALG_SCHED_LQR_TARGET == 100
    lib = alg.hip_lib()
    assert "mpc_set_schedule" not in lib.absent and "mpc_get_schedule" not in lib.absent
    # a null handle is refused before any device call
    assert dll.alg_mpc_set_schedule(None, 0, 1, None) == alg._abi.ALG_ERR_ARG
    assert dll.alg_mpc_get_schedule(None, 0, None) == alg._abi.ALG_ERR_ARG


def test_every_loop_kernel_has_a_scheduled_sibling_within_its_resources(alg):
    """k_mpc_loop_sched<C> for every k_mpc_loop<C> of the library -- one wavefront, teams, EXT, block-reading twins, dense direction: no VGPR
    spill, no scratch where the unscheduled kernel has none, the same LDS.  (The unscheduled kernels themselves: tests/test_abi.py.)"""
    spec = importlib.util.spec_from_file_location("_resources", os.path.join(ROOT, "algames.jl_amd", "_resources.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.kernel_resources(_lib_path(alg))
    loops = sorted(k for k in res if k.startswith("k_mpc_loop<"))
    assert len(loops) >= 97, len(loops)
    assert len([k for k in res if k.startswith("k_mpc_loop_sched<")]) == len(loops)
    for k in loops:
        ks = k.replace("k_mpc_loop<", "k_mpc_loop_sched<")
        assert ks in res, ks
        v, parent = res[ks], res[k]
        print("%-52s vgpr %3d sgpr_spill %3d scratch %3d lds %6d   (unscheduled: vgpr %3d sgpr_spill %3d scratch %3d)" %
              (ks, v["vgpr"], v["sgpr_spill"], v["scratch"], v["lds"], parent["vgpr"], parent["sgpr_spill"], parent["scratch"]))
        assert v["vgpr_spill"] == 0, (ks, v)
        assert v["scratch"] == 0 or parent["scratch"] > 0, (ks, v, parent)
        assert v["lds"] == parent["lds"], (ks, v, parent)
    # (SGPR spills: the phase costs the C5 loops 2 -- 13 against 11 in the team of four, 26 against 24 in the one-wavefront kernel, which is
    # why it lives in a sibling and not in k_mpc_loop itself: DESIGN.md 3.2 -- reported above, not bounded)
    assert res["k_mpc_loop_sched<Cfg<2, 4, 2, 1, 1> >"]["scratch"] == 0


def test_the_scheduled_units_are_registered_with_the_build():
    import __graft_entry__ as ge
    sched = ge.KERNEL_SETS["sched"]
    assert len(sched) == 21 and all(u in ge.HIP_UNITS and u[1].startswith("algames_sched_") for u in sched)
    assert all(os.path.exists(os.path.join(ge.CSRC, u[0])) for u in sched)
    # the scheduled loops take the flags of the unit that holds their unscheduled siblings: every family, every unit of it
    for f in ge.FAMILIES:
        mine, siblings = ge._sched_units(f), ge._kernel_units(f)
        assert mine and siblings and all(u in sched for u in mine), f.name
        for u in mine:
            for v in siblings:
                assert ge.unit_flags(u[1]) == ge.unit_flags(v[1]), (u[1], v[1])
    assert sum(len(ge._sched_units(f)) for f in ge.FAMILIES) == 21
    assert ge.unit_flags("algames_sched_mw") == ge.unit_flags("algames_mw") == ge.HIP_FLAGS_TILE
    assert ge.unit_flags("algames_sched_quad") == ge.unit_flags("algames_quad") == ge.HIP_FLAGS_DENSE + ge.HIP_FLAGS_NOLSO
    assert ge.unit_flags("algames_sched_p5") == ge.unit_flags("algames_p5") == ge.HIP_FLAGS_DENSE


def test_python_kind_and_shape_validation(alg, orc):
    """Batch.mpc_set_schedule / host.mpc_solve(schedule=...) refuse unknown kinds and wrong shapes before any library call (checked on an
    oracle-backed batch, which needs no GPU; the oracle has no schedule entry points)."""
    b = orc.OracleBatch(1, 3, 6, 0.1, 2)
    L = 3 * 4 + 3 * 2
    assert b._sched_kind("lqr_target") == (100, L) and b._sched_kind(100) == (100, L)
    for bad in (np.zeros((2, L)), np.zeros((2, 3, L)), np.zeros((2, 2, L + 1)), np.zeros((0, 2, L))):
        with pytest.raises(ValueError, match="expected shape"):
            b.mpc_set_schedule("lqr_target", bad)
    with pytest.raises(ValueError, match="unknown schedule kind"):
        b.mpc_set_schedule("lqr", np.zeros((2, 2, L)))
    with pytest.raises(ValueError):
        b.mpc_set_schedule(8, np.zeros((2, 2, L)))
    with pytest.raises(alg.AlgamesError, match="no orc_mpc_set_schedule"):
        b.mpc_set_schedule("lqr_target", np.zeros((2, 2, L)))

    class P:                                          # the part of a GameProblem mpc_solve touches before it validates
        batch = b
    with pytest.raises(ValueError, match="expected shape"):
        alg.mpc_solve(P, 3, schedule={"lqr_target": np.zeros((2, 5, L))})
    with pytest.raises(ValueError, match="unknown schedule kind"):
        alg.mpc_solve(P, 3, schedule={"target": np.zeros((2, 2, L))})


def test_the_scheduled_set_is_a_pure_function_of_the_scenario_ids(alg, orc):
    """scenarios.c5_scheduled: rows of the right shapes, row 0 = the problem's own values, low speeds, shards see the whole batch's numbers"""
    ids, rows = np.arange(40, 48), 12
    prob, S = alg.scenarios.c5_scheduled(ids, rows, backend=orc.lib())
    assert set(S) == {"circle", "lqr_target"} and S["circle"].shape == (rows, 8, 3) and S["lqr_target"].shape == (rows, 8, 18)
    assert np.array_equal(S["lqr_target"][0][:, :12], prob.game_obj.xf.reshape(8, 12))
    assert np.all(S["circle"][..., 2] == 0.1)
    step_c = np.linalg.norm(np.diff(S["circle"][..., :2], axis=0), axis=-1)
    assert step_c.max() <= 0.03 + 1e-12 and step_c.min() >= 0.02 - 1e-12                 # 0.2 ... 0.3 per unit time, dt = 0.1
    xy = S["lqr_target"][..., :12].reshape(rows, 8, 3, 4)[..., :2]
    assert np.allclose(np.linalg.norm(np.diff(xy, axis=0), axis=-1), alg.scenarios.GOAL_SPEED * 0.1) and alg.scenarios.GOAL_SPEED <= 0.05
    # no vehicle starts inside the circle
    x0 = prob.x0
    d0 = np.hypot(x0[:, 0:3] - S["circle"][0][:, None, 0], x0[:, 3:6] - S["circle"][0][:, None, 1])
    assert d0.min() > 0.2
    _, S2 = alg.scenarios.c5_scheduled(ids[3:6], rows, backend=orc.lib())
    assert np.array_equal(S2["circle"], S["circle"][:, 3:6]) and np.array_equal(S2["lqr_target"], S["lqr_target"][:, 3:6])
