"""Build check of the base kernels' twins that read per-game scenario blocks (Cfg<model, p, d, 2, waves>, alg_set_scenario_kernels): the
kernel metadata of the code objects inside libalgames_hip.so.  No GPU needed."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DI, UNI = 0, 1
TILE = [(DI, 1, 2), (DI, 2, 2), (DI, 3, 2), (DI, 4, 2), (DI, 2, 3), (UNI, 1, 2), (UNI, 2, 2), (UNI, 3, 2), (UNI, 4, 2)]    # ALG_CFGS_BASE
TEAMS = [(DI, 3, 2, 4), (UNI, 3, 2, 4), (UNI, 4, 2, 2), (UNI, 4, 2, 4)]                                                    # ALG_CFGS_MW
HANDOFF = [(DI, 3, 2, 4), (UNI, 3, 2, 4), (UNI, 4, 2, 4)]                                                                  # ALG_CFGS_HANDOFF


def _resources(alg):
    import __graft_entry__ as ge
    if not os.path.exists(alg.HIP_LIB_PATH):
        ge.build()
    spec = importlib.util.spec_from_file_location("_resources", os.path.join(ROOT, "algames.jl_amd", "_resources.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod.kernel_resources(alg.HIP_LIB_PATH)


def _name(kernel, model, p, d, e, w, ls=None):
    return "%s<Cfg<%d, %d, %d, %d, %d%s> >" % (kernel, model, p, d, e, w, "" if ls is None else ", %d" % ls)


def test_the_block_reading_twins_of_the_base_kernels_are_built_and_do_not_spill(alg):
    res = _resources(alg)
    twins = []                       # (kernel, model, p, d, waves, line-search staging)
    for (model, p, d) in TILE:
        twins += [(k, model, p, d, 1, None) for k in ("k_newton_solve", "k_mpc_loop")]
    for (model, p, d, w) in TEAMS:
        twins += [(k, model, p, d, w, None) for k in ("k_newton_solve", "k_mpc_loop")]
    for (model, p, d, w) in HANDOFF:
        twins += [("k_newton_solve_ho", model, p, d, 1, None), ("k_newton_resume", model, p, d, w, 0)]
    for (kern, model, p, d, w, ls) in twins:
        k, k0 = _name(kern, model, p, d, 2, w, ls), _name(kern, model, p, d, 0, w, ls)
        assert k in res, k
        v, parent = res[k], res[k0]
        print("%-52s vgpr %3d sgpr %3d scratch %3d sgpr_spill %3d lds %6d   (parent: vgpr %3d sgpr_spill %3d lds %6d)" %
              (k, v["vgpr"], v["sgpr"], v["scratch"], v["sgpr_spill"], v["lds"], parent["vgpr"], parent["sgpr_spill"], parent["lds"]))
        assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["lds"] == parent["lds"], (k, v, parent)                 # the same LDS layout as the base kernel
    # all 13 kernels of the tile-path twins exist (the step-wise entry points, IBR and the MPC loop honour the block too)
    for k in ("k_newton_step", "k_residual", "k_jacobian", "k_direction", "k_line_search", "k_update", "k_record", "k_dual_update", "k_init", "k_ibr",
              "k_mpc_advance"):
        for (model, p, d) in TILE:
            assert _name(k, model, p, d, 2, 1) in res, (k, model, p, d)
    # the C2 twin and its hand-off twin: sixteen games per CU (128 VGPRs, 160 KB / 16 = 10 240 bytes of LDS), the occupancy the headline rests on
    for k in (_name("k_newton_solve", DI, 3, 2, 2, 1), _name("k_newton_solve_ho", DI, 3, 2, 2, 1)):
        assert res[k]["vgpr"] <= 128 and res[k]["lds"] <= 10240, (k, res[k])
    # the team twins keep the LDS bounds tests/test_abi.py states for their parents
    assert res[_name("k_mpc_loop", UNI, 3, 2, 2, 4)]["lds"] <= 80 * 1024 and res[_name("k_newton_solve", DI, 3, 2, 2, 4)]["lds"] <= 80 * 1024
    assert res[_name("k_newton_solve", UNI, 3, 2, 2, 1)]["lds"] <= 13653
    assert res[_name("k_newton_solve", UNI, 4, 2, 2, 2)]["lds"] <= 40 * 1024


def test_the_new_units_are_registered_with_the_build():
    import __graft_entry__ as ge
    stems = [u[1] for u in ge.HIP_UNITS]
    assert [s for s in stems if s.startswith("algames_base_scen_")] == ["algames_base_scen_%d" % k for k in range(9)]
    # nine per-entry units with ext = 2, one per index, and the team unit with ext = 2
    per_entry = [u for u in ge.HIP_UNITS if u[0] == "algames_base.hip" and "-DALG_BASE_EXT=2" in u[2]]
    assert [u[1] for u in per_entry] == ["algames_base_scen_%d" % k for k in range(9)]
    assert [u[2] for u in per_entry] == [["-DALG_BASE_SEL=%d" % k, "-DALG_BASE_EXT=2"] for k in range(9)]
    assert ("algames_mw.hip", "algames_mw_scen", ["-DALG_MW_EXT=2"]) in ge.HIP_UNITS
    for src, stem, extra in ge.HIP_UNITS:
        assert os.path.exists(os.path.join(ge.CSRC, src)), src
