"""Players' costs (alg_get_cost, alg_mpc_set_cost_log / alg_mpc_get_cost_log / alg_mpc_get_cost), the parts that need no GPU: the header
declares and the library exports the four entry points, a null handle is refused before any device call, the ctypes table and the Julia shim
bind them, every one-wavefront configuration has its two cost kernels within the register budget, and the Python layer validates its
arguments -- on an oracle-backed batch, which has no such entry points and says so."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

DI, UNI = 0, 1
ENTRY = ("get_cost", "mpc_set_cost_log", "mpc_get_cost_log", "mpc_get_cost")
ALG_ERR_ARG = -1


def test_the_header_declares_and_the_library_exports_the_four_entry_points():
    ge.build()
    hdr = open(os.path.join(ge.ROOT, "include", "algames_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).replace(" ,", ",").replace(" )", ")")
    for proto in ("int alg_get_cost(alg_handle* h, int32_t which, double* total, double* stage);",
                  "int alg_mpc_set_cost_log(alg_handle* h, int32_t on);",
                  "int alg_mpc_get_cost_log(alg_handle* h, int32_t* on);",
                  "int alg_mpc_get_cost(alg_handle* h, int32_t max_knots, double* stage, double* total, int32_t* knots_out);"):
        assert proto in code, proto
    assert "objective.jl:12-35" in hdr and "objective.jl:122-131" in hdr
    dll = ctypes.CDLL(ge.HIP_LIB)
    for name in ENTRY:
        assert hasattr(dll, "alg_" + name), name


def test_the_ctypes_table_lists_them_as_optional_and_the_product_has_them():
    ge.build()
    import algames_jl_amd as alg
    for name in ENTRY:
        assert name in alg._abi.SIGNATURES and name in alg._abi.OPTIONAL and name not in alg.hip_lib().absent, name
    _P, _D, _I, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32
    assert alg._abi.SIGNATURES["get_cost"] == (ctypes.c_int, [_P, i32, _D, _D])
    assert alg._abi.SIGNATURES["mpc_set_cost_log"] == (ctypes.c_int, [_P, i32])
    assert alg._abi.SIGNATURES["mpc_get_cost_log"] == (ctypes.c_int, [_P, _I])
    assert alg._abi.SIGNATURES["mpc_get_cost"] == (ctypes.c_int, [_P, i32, _D, _D, _I])


def test_a_null_handle_is_refused_without_a_device_call():
    """the refusal comes first: ALG_ERR_ARG with a message, the outputs untouched -- where no device is present a device call would have come
    back as ALG_ERR_DEVICE instead"""
    ge.build()
    import algames_jl_amd as alg
    lib = alg.hip_lib()
    out = np.zeros(16); v = ctypes.c_int32(7)
    D = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for rc in (lib.get_cost(None, 0, D(out), None), lib.mpc_set_cost_log(None, 1), lib.mpc_get_cost_log(None, ctypes.byref(v)),
               lib.mpc_get_cost(None, 4, D(out), D(out), ctypes.byref(v))):
        assert rc == ALG_ERR_ARG
        assert b"null" in lib.last_error()
    assert v.value == 7 and np.all(out == 0.0)


def test_the_shim_binds_the_four_entry_points():
    txt = open(os.path.join(ge.PKG, "julia", "AlgamesHIP.jl")).read()
    for name, types in (("alg_get_cost", "(Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64})"), ("alg_mpc_set_cost_log", "(Ptr{Cvoid}, Int32)"),
                        ("alg_mpc_get_cost_log", "(Ptr{Cvoid}, Ref{Int32})"),
                        ("alg_mpc_get_cost", "(Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int32})")):
        assert "ccall((:%s, LIB), Cint, %s" % (name, types) in txt, name
    for fn in (r"^function player_costs\(bp::BatchedGameProblem", r"^set_mpc_cost_log!\(bp::BatchedGameProblem, on::Bool\)", r"^function mpc_costs\(bp::BatchedGameProblem\)"):
        assert re.search(fn, txt, flags=re.M), fn


def test_every_one_wavefront_configuration_has_its_two_cost_kernels_within_the_budget():
    ge.build()
    from algames_jl_amd import _resources
    res = {k.replace("> >", ">>"): v for k, v in _resources.kernel_resources(ge.HIP_LIB).items()}
    adv = sorted(k[len("k_mpc_advance"):] for k in res if k.startswith("k_mpc_advance<"))
    assert len(adv) >= 60 and len(set(adv)) == len(adv)
    for fam in ("k_player_cost", "k_closed_loop_cost"):
        assert sorted(k[len(fam):] for k in res if k.startswith(fam + "<")) == adv, fam
        for cfg in adv:
            r = res[fam + cfg]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["vgpr"] <= 128, (fam + cfg, r)
            assert r["lds"] <= 4096, (fam + cfg, r)        # a reduction buffer, nothing else


def test_python_argument_validation_on_an_oracle_backed_batch(orc):
    import algames_jl_amd as alg
    o = orc.OracleBatch(DI, 2, 5, 0.1, 2)
    for name in ENTRY:
        assert name in o.lib.absent
    # bad arguments are refused by the Python layer, before the backend is asked
    for bad in (2, -1, "pd", 0.0, True, None):
        with pytest.raises(ValueError):
            o.get_cost(which=bad)
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError):
            o.mpc_get_cost(max_knots=bad)
    with pytest.raises(ValueError):
        o.mpc_set_cost_log("yes")
    # good ones reach the backend, which has no such entry point
    for call in (lambda: o.get_cost(), lambda: o.get_cost(alg.ALG_TRAJ_TRIAL, stage=True), lambda: o.mpc_set_cost_log(True),
                 lambda: o.mpc_get_cost_log(), lambda: o.mpc_get_cost(), lambda: o.mpc_get_cost(max_knots=3)):
        with pytest.raises(alg.AlgamesError):
            call()
    prob = alg.scenarios.make_problem("C2", np.arange(2), N=6, backend=orc.lib())
    with pytest.raises(ValueError):
        alg.player_costs(prob, which="delta")
    with pytest.raises(alg.AlgamesError):
        alg.player_costs(prob)
    with pytest.raises(alg.AlgamesError):
        alg.player_costs(prob, which="trial", stage=True)
    with pytest.raises(alg.AlgamesError):
        alg.mpc_rollout(prob, steps=1, costs=True)


def test_the_step_wise_rollout_costs_are_the_reference_on_the_oracle(orc):
    """mpc_rollout(fused=False, costs=True) evaluates the definition in numpy (host.py's own statement of it): on an oracle-backed problem --
    the step-wise path needs no device entry point -- it must be tests/cost_reference.py on the rollout's own states and controls, with a
    target schedule of two rows over three steps (the oracle has no plant: a knot is a step)."""
    import algames_jl_amd as alg
    import cost_reference as CR
    B, N, p = 2, 6, 3
    model = alg.DoubleIntegratorGame(p=p, d=2)
    rng = np.random.default_rng(5)
    Q, R = 0.5 + rng.random((B, p, 4)), 0.5 + rng.random((B, p, 2))
    xf, uf = rng.normal(size=(B, p, 4)), 0.2 * rng.normal(size=(B, p, 2))
    obj = alg.GameObjective([np.diag(q) for q in Q[0]], [np.diag(r) for r in R[0]], list(xf[0]), list(uf[0]), N, model)
    obj.Qdiag, obj.Rdiag, obj.xf, obj.uf = Q, R, xf, uf
    rad, mu = np.array([0.9, 1.1, 1.0]), np.array([3.0, 5.0, 7.0])
    alg.add_collision_cost(obj, rad, mu)
    con = alg.GameConstraintValues(alg.ProblemSize(N, model))
    opts = alg.Options(); opts.outer_iter, opts.inner_iter = 2, 3
    x0 = 0.3 * rng.normal(size=(B, model.n))
    prob = alg.GameProblem(N, 0.1, x0, model, opts, obj, con, backend=orc.lib())
    rows = rng.normal(size=(2, B, p * 4 + p * 2))
    ro = alg.mpc_rollout(prob, steps=3, schedule={"lqr_target": rows}, fused=False, costs=True)
    assert ro.stage_cost.shape == (3, B, p, 3) and ro.cost.shape == (B, p, 3)
    stage, total = CR.closed_loop_cost(model, 0.1, 1, ro.states, ro.controls, Q, R, xf, uf, np.tile(rad, (B, 1)), np.tile(mu, (B, 1)), target_rows=rows)
    tol = CR.bound(stage, 0.1 * (mu * rad ** 2 * (p - 1))[None, None, :])
    assert np.all(np.abs(ro.stage_cost - stage) <= tol), np.abs(ro.stage_cost - stage).max()
    assert np.all(np.abs(ro.cost - total) <= CR.bound(total, 3 * 0.1 * (mu * rad ** 2 * (p - 1))[None, :]))
    assert np.all(ro.stage_cost[..., 2].sum(axis=0) >= 0) and np.all(ro.stage_cost[..., :2] > 0)
    plain = alg.mpc_rollout(prob, steps=1, fused=False)
    assert plain.stage_cost is None and plain.cost is None
