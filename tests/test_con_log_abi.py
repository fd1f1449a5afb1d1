"""Constraint values (alg_get_con_values, alg_con_knot_len, alg_mpc_set_con_log / alg_mpc_get_con_log / alg_mpc_get_con), the parts that need
no GPU: the header declares and the library exports the five entry points, a null handle is refused before any device call, the ctypes table
and the Julia shim bind them, every one-wavefront configuration has its two constraint kernels without scratch or spills, the Python layer
validates its arguments -- on an oracle-backed batch, which has no such entry points and says so -- and the step-wise rollout's numpy
evaluation is tests/con_reference.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

DI = 0
ENTRY = ("get_con_values", "con_knot_len", "mpc_set_con_log", "mpc_get_con_log", "mpc_get_con")
ALG_ERR_ARG = -1


def test_the_header_declares_and_the_library_exports_the_five_entry_points():
    ge.build()
    hdr = open(os.path.join(ge.ROOT, "include", "algames_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).replace(" ,", ",").replace(" )", ")")
    for proto in ("int alg_get_con_values(alg_handle* h, int32_t which, double* vals);",
                  "int alg_con_knot_len(alg_handle* h, int32_t* len);",
                  "int alg_mpc_set_con_log(alg_handle* h, int32_t on);",
                  "int alg_mpc_get_con_log(alg_handle* h, int32_t* on);",
                  "int alg_mpc_get_con(alg_handle* h, int32_t max_knots, double* vals, double* worst, int32_t* first, int32_t* knots_out);"):
        assert proto in code, proto
    for k, name in enumerate(("COLLISION", "CONTROL", "STATE", "WALL", "CIRCLE", "WALL3D", "CYLINDER", "KINDS")):
        assert re.search(r"#define ALG_CON_%s\s+%d\b" % (name, k), hdr), name
    assert "constraints_methods.jl:329-379" in hdr
    dll = ctypes.CDLL(ge.HIP_LIB)
    for name in ENTRY:
        assert hasattr(dll, "alg_" + name), name


def test_the_ctypes_table_lists_them_as_optional_and_only_the_product_has_them(orc):
    ge.build()
    import algames_jl_amd as alg
    for name in ENTRY:
        assert name in alg._abi.SIGNATURES and name in alg._abi.OPTIONAL and name not in alg.hip_lib().absent, name
        assert name in orc.lib().absent, name
    _P, _D, _I, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32
    assert alg._abi.SIGNATURES["get_con_values"] == (ctypes.c_int, [_P, i32, _D])
    assert alg._abi.SIGNATURES["con_knot_len"] == (ctypes.c_int, [_P, _I])
    assert alg._abi.SIGNATURES["mpc_set_con_log"] == (ctypes.c_int, [_P, i32])
    assert alg._abi.SIGNATURES["mpc_get_con_log"] == (ctypes.c_int, [_P, _I])
    assert alg._abi.SIGNATURES["mpc_get_con"] == (ctypes.c_int, [_P, i32, _D, _D, _I, _I])
    assert alg.ALG_CON_KINDS == 7 and (alg.ALG_CON_COLLISION, alg.ALG_CON_CYLINDER) == (0, 6)


def test_a_null_handle_is_refused_without_a_device_call():
    """the refusal comes first: ALG_ERR_ARG with a message, the outputs untouched -- where no device is present a device call would have come
    back as ALG_ERR_DEVICE instead"""
    ge.build()
    import algames_jl_amd as alg
    lib = alg.hip_lib()
    out = np.zeros(16); first = np.zeros(8, dtype=np.int32); v = ctypes.c_int32(7)
    D = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    I = first.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for rc in (lib.get_con_values(None, 0, D(out)), lib.con_knot_len(None, ctypes.byref(v)), lib.mpc_set_con_log(None, 1),
               lib.mpc_get_con_log(None, ctypes.byref(v)), lib.mpc_get_con(None, 4, D(out), D(out), I, ctypes.byref(v))):
        assert rc == ALG_ERR_ARG
        assert b"null" in lib.last_error()
    assert v.value == 7 and np.all(out == 0.0) and np.all(first == 0)


def test_the_shim_binds_the_five_entry_points():
    txt = open(os.path.join(ge.PKG, "julia", "AlgamesHIP.jl")).read()
    for name, types in (("alg_get_con_values", "(Ptr{Cvoid}, Int32, Ptr{Float64})"), ("alg_con_knot_len", "(Ptr{Cvoid}, Ref{Int32})"),
                        ("alg_mpc_set_con_log", "(Ptr{Cvoid}, Int32)"), ("alg_mpc_get_con_log", "(Ptr{Cvoid}, Ref{Int32})"),
                        ("alg_mpc_get_con", "(Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Int32})")):
        assert "ccall((:%s, LIB), Cint, %s" % (name, types) in txt, name
    for fn in (r"^function constraint_values\(bp::BatchedGameProblem", r"^set_mpc_con_log!\(bp::BatchedGameProblem, on::Bool\)",
               r"^function mpc_constraints\(bp::BatchedGameProblem\)", r"constraints::Bool=false"):
        assert re.search(fn, txt, flags=re.M), fn


def test_every_one_wavefront_configuration_has_its_two_constraint_kernels_without_scratch_or_spills():
    ge.build()
    from algames_jl_amd import _resources
    res = {k.replace("> >", ">>"): v for k, v in _resources.kernel_resources(ge.HIP_LIB).items()}
    adv = sorted(k[len("k_mpc_advance"):] for k in res if k.startswith("k_mpc_advance<"))
    assert len(adv) >= 60 and len(set(adv)) == len(adv)
    for fam in ("k_con_values", "k_closed_loop_con"):
        assert sorted(k[len(fam):] for k in res if k.startswith(fam + "<")) == adv, fam
        for cfg in adv:
            r = res[fam + cfg]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["vgpr"] <= 128, (fam + cfg, r)
            assert r["lds"] == 0, (fam + cfg, r)


def test_python_argument_validation_on_an_oracle_backed_batch(orc):
    import algames_jl_amd as alg
    o = orc.OracleBatch(DI, 2, 5, 0.1, 2)
    for name in ENTRY:
        assert name in o.lib.absent
    # bad arguments are refused by the Python layer, before the backend is asked
    for bad in (2, -1, "pd", 0.0, True, None):
        with pytest.raises(ValueError):
            o.get_con_values(which=bad)
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError):
            o.mpc_get_con(max_knots=bad)
    with pytest.raises(ValueError):
        o.mpc_set_con_log("yes")
    # good ones reach the backend, which has no such entry point
    for call in (lambda: o.get_con_values(), lambda: o.get_con_values(alg.ALG_TRAJ_TRIAL), lambda: o.con_knot_len(), lambda: o.mpc_set_con_log(True),
                 lambda: o.mpc_get_con_log(), lambda: o.mpc_get_con(), lambda: o.mpc_get_con(max_knots=3)):
        with pytest.raises(alg.AlgamesError):
            call()
    prob = alg.scenarios.make_problem("C2", np.arange(2), N=6, backend=orc.lib())
    with pytest.raises(ValueError):
        alg.constraint_values(prob, which="delta")
    with pytest.raises(alg.AlgamesError):
        alg.constraint_values(prob)
    with pytest.raises(alg.AlgamesError):
        alg.constraint_values(prob, which="trial")
    with pytest.raises(ValueError):
        alg.mpc_rollout(prob, steps=1, constraints=1)
    with pytest.raises(alg.AlgamesError):
        alg.mpc_rollout(prob, steps=1, constraints=True)


def test_the_step_wise_rollout_constraints_are_the_reference_on_the_oracle(orc):
    """mpc_rollout(fused=False, constraints=True) evaluates the definition in numpy (host.py's own statement of it): on an oracle-backed
    problem it must be tests/con_reference.py on the rollout's own states and controls, con_worst / con_first from the same values.
    Three steps, N = 6, a circle schedule of two rows (the last row held), a wall masked to one player, control bounds.  The oracle has no
    plant (a knot is a step) and no per-game scenario data: the step-wise loop cannot hand it a schedule row, so the rows are applied to
    the definition's numbers alone -- which is what this test is about -- through a backend wrapper that accepts set_scenario_data."""
    import algames_jl_amd as alg
    import con_reference as CR
    B = 2
    prob, rng = CR.rollout_problem(orc.lib(), B)
    b = prob.batch
    rows = CR.circle_rows(rng, B)
    applied = []
    b.scenario_data_len = lambda kind: 3
    b.set_scenario_data = lambda kind, data: applied.append((kind, np.array(data)))
    ro = alg.mpc_rollout(prob, steps=3, schedule={"circle": rows}, fused=False, constraints=True)
    assert len(applied) == 2 and np.array_equal(applied[0][1], rows[0]) and np.array_equal(applied[1][1], rows[1])
    tab = CR.tables(prob)
    K1 = 6 + 2 * b.m + 3 * 1 + 3 * 1                                  # the pair block (not added: zeros), control bounds, a wall and a circle per player
    assert ro.con.shape == (3, B, K1) and ro.con_worst.shape == (B, 7) and ro.con_first.shape == (B, 7) and ro.con_first.dtype == np.int32
    ref, scale, margin, kinds = CR.closed_loop(b, tab, tab["nums"], ro.states, ro.controls, 1, {CR.S_CIRC: rows})
    assert margin.min() >= 1e-6
    CR.check(ro.con, ref, scale, "step-wise rollout")
    worst, first = CR.summary(ro.con, kinds)
    assert np.array_equal(ro.con_worst, worst) and np.array_equal(ro.con_first, first)
    assert np.all(np.isneginf(ro.con_worst[:, [0, 2, 5, 6]])) and np.all(ro.con_first[:, [0, 2, 5, 6]] == -1)      # kinds that were not added
    assert np.all(ro.con[:, :, kinds == 3][:, :, [0, 2]] == 0.0)                                                   # the wall's rows of players 1 and 3: inert
    assert (ro.con_first[:, [1, 3, 4]] >= 0).any()
    plain = alg.mpc_rollout(prob, steps=1, fused=False)
    assert plain.con is None and plain.con_worst is None and plain.con_first is None
