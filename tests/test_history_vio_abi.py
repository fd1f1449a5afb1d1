"""Per-record violation profiles (alg_set_history_profiles), the parts that need no GPU: the library exports the entry points, every solve
kernel but those of seven to ten players has its sibling k_newton_solve_vio, the Julia shim binds the three calls, the oracle backend
refuses the setter -- and the oracle-side replay that tests/test_gpu_history_vio.py compares the device's profiles with reproduces the
oracle's own history (the replay loop itself is what this holds)."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

DI, UNI, BIC = 0, 1, 2
# the set-up of tests/test_gpu_parity.py::test_violation_profile_parity, and the 3-player double integrator at N - 1 in {1, 2, FT, FT + 1}, FT = 13
T1_CASES = [(DI, 3, 12, False), (UNI, 4, 9, False), (UNI, 3, 8, True), (BIC, 2, 7, True), (DI, 3, 2, False), (DI, 3, 3, False), (DI, 3, 14, False), (DI, 3, 15, False)]
T1_B, T1_GID0 = 3, 5
FIELDS = ("dyn", "con", "sta", "opt")


def t1_problem(make, model, p, N, ext):
    """test_violation_profile_parity's problem on make(model, p, N, dt, B) -> batch: seed 31, outer_iter = 2, inner_iter = 3"""
    b = make(model, p, N, 0.1, T1_B)
    rng = np.random.default_rng(31)
    ni = b.n // p
    Q, R = 1 + rng.random((T1_B, p, ni)), 0.5 + rng.random((T1_B, p, b.mi)); xf, uf = rng.random((T1_B, p, ni)), rng.random((T1_B, p, b.mi)) - 0.5
    x0 = rng.random((T1_B, b.n))
    b.set_x0(x0); b.set_lqr(Q, R, xf, uf); b.set_options(outer_iter=2, inner_iter=3)
    if p > 1:
        b.add_collision_avoidance(0.3 + 0.1 * np.arange(p))
    umax = np.full(b.m, 0.3); umax[0] = np.inf
    b.add_control_bound(umax, np.full(b.m, -0.2))
    if ext:
        xmax = np.full(b.n, np.inf); xmin = np.full(b.n, -np.inf); xmax[::3] = 0.6
        b.add_state_bound(0, xmax, xmin)
        b.add_wall_constraint([0.0], [0.5], [1.0], [0.5], [0.0], [1.0]); b.add_circle_constraint([0.5], [0.5], [0.3])
    return b


def oracle_replay(make_oracle, hist, game):
    """The profiles of every record of `hist` (the history of `game` from the oracle's own fused solve) by the oracle's step-wise entry
    points on a fresh batch: init_traj + rollout + reset_con, dual_penalty_update wherever the record's outer index advances,
    violation_profile() before each newton_step(k, l, delta), once more at the final iterate.  Every game of the fresh batch is driven by
    this game's history; only this game's rows are read.  Returns dict(dyn, con, sta, opt) of shape (records, N-1 | N)."""
    o = make_oracle()
    o.init_traj(game_id0=T1_GID0, use_shift=True); o.rollout(0); o.reset_con()
    rows = {f: [] for f in FIELDS}
    outer, l = 1, 0
    for r in range(len(hist)):
        k = int(hist["outer"][r])
        last = r == len(hist) - 1
        if k > outer and not last:                 # (the final record carries the outer index of the last iteration: no update precedes it)
            o.dual_penalty_update(); outer, l = k, 0
        v = o.violation_profile()
        for f in FIELDS:
            rows[f].append(v[f][game].copy())
        if not last:
            l += 1
            o.newton_step(k, l, delta=np.full(o.B, hist["delta"][r]))
    return {f: np.array(rows[f]) for f in FIELDS}


@pytest.mark.parametrize("model,p,N,ext", T1_CASES)
def test_the_oracle_replay_reproduces_the_oracles_own_history(orc, model, p, N, ext):
    """per-record maxima of the replayed profiles == the *_vio of the oracle's own history, exactly; sta[:, 0] == 0"""
    make = lambda: t1_problem(lambda *a: orc.OracleBatch(*a), model, p, N, ext)
    o = make()
    o.newton_solve(init=True, game_id0=T1_GID0)
    for game in range(T1_B):
        h = o.get_history(game)
        assert len(h) >= 2
        prof = oracle_replay(make, h, game)
        for f in FIELDS:
            assert prof[f].shape == (len(h), N - 1 if f in ("dyn", "con") else N)
            assert np.array_equal(prof[f].max(axis=1), h[f + "_vio"]), (game, f, prof[f].max(axis=1), h[f + "_vio"])
        assert np.all(prof["sta"][:, 0] == 0.0)


def test_the_library_exports_the_three_entry_points():
    ge.build()
    dll = ctypes.CDLL(ge.HIP_LIB)
    for name in ("alg_set_history_profiles", "alg_get_history_profiles", "alg_get_history_vio"):
        assert hasattr(dll, name), name
    import algames_jl_amd as alg
    for name in ("set_history_profiles", "get_history_profiles", "get_history_vio"):
        assert name in alg._abi.SIGNATURES and name in alg._abi.OPTIONAL and name not in alg.hip_lib().absent, name


def _header_list(name):
    """the entries (model, p, d, ext[, waves]) of one ALG_CFGS_* list of algames_kernels.hpp, lists inside lists expanded"""
    txt = open(os.path.join(ge.CSRC, "algames_kernels.hpp")).read().replace("\\\n", " ")
    defs = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"^#define\s+(ALG_CFGS_\w+)\(([^)]*)\)(.*)$", txt, flags=re.M)}
    models = {"ALG_MODEL_DOUBLE_INTEGRATOR": 0, "ALG_MODEL_UNICYCLE": 1, "ALG_MODEL_BICYCLE": 2, "ALG_MODEL_QUADROTOR": 3}

    def expand(n, args):
        params, body = defs[n]
        env = dict(zip([q.strip() for q in params.split(",")], args))
        out = []
        for m in re.finditer(r"(\w+)\(([^()]*)\)", body):
            a = [env.get(q.strip(), q.strip()) for q in m.group(2).split(",")]
            if m.group(1) in defs:
                out += expand(m.group(1), a)
            elif m.group(1) == env.get("X", "X"):
                out.append(tuple(models[v] if v in models else int(v) for v in a))
        return out
    return expand(name, ["X"])


def test_every_covered_solve_kernel_has_its_sibling_and_seven_to_ten_players_have_none():
    ge.build()
    from algames_jl_amd import _resources
    res = {k.replace("> >", ">>") for k in _resources.kernel_resources(ge.HIP_LIB)}      # (the demangler writes nested templates as `> >`)
    # the siblings are a kernel family of their own, history_vio::k_newton_solve_vio<C>: the k_newton_solve* / k_mpc_loop* families stay the
    # list tests/test_kkt_solve_build.py pins
    assert not any(k.startswith("k_newton_solve_vio") for k in res)
    vio = {k[len("history_vio::"):] for k in res if k.startswith("history_vio::k_newton_solve_vio<")}
    assert len(vio) == sum("k_newton_solve_vio<" in k for k in res)
    plain = {k for k in res if k.startswith("k_newton_solve<")}
    one = ["ALG_CFGS_BASE", "ALG_CFGS_BASE_SCEN", "ALG_CFGS_EXT", "ALG_CFGS_QUAD", "ALG_CFGS_QUAD_EXT", "ALG_CFGS_DI3D", "ALG_CFGS_P5", "ALG_CFGS_P6", "ALG_CFGS_DI1"]
    want = set()
    for name in one:
        entries = _header_list(name)
        assert entries, name
        want |= {"k_newton_solve_vio<Cfg<%d, %d, %d, %d, 1>>" % e for e in entries}
    for name in ("ALG_CFGS_MW", "ALG_CFGS_MW_SCEN", "ALG_CFGS_MW_DENSE"):
        entries = _header_list(name)
        assert entries, name
        want |= {"k_newton_solve_vio<Cfg<%d, %d, %d, %d, %d>>" % e for e in entries}
    assert vio == want, (sorted(want - vio), sorted(vio - want))
    # a sibling per solve kernel of at most six players, none beyond
    assert {k.replace("k_newton_solve<", "k_newton_solve_vio<") for k in plain if int(re.search(r"Cfg<\d+, (\d+),", k).group(1)) <= 6} == vio
    for name in ("ALG_CFGS_P7", "ALG_CFGS_P8", "ALG_CFGS_P9", "ALG_CFGS_P10"):
        for e in _header_list(name):
            assert "k_newton_solve<Cfg<%d, %d, %d, %d, 1>>" % e in plain and "k_newton_solve_vio<Cfg<%d, %d, %d, %d, 1>>" % e not in vio, e
    assert not any(re.search(r"Cfg<\d+, (7|8|9|10),", k) for k in vio)


def test_the_shim_binds_the_three_entry_points():
    txt = open(os.path.join(ge.PKG, "julia", "AlgamesHIP.jl")).read()
    for name, types in (("alg_set_history_profiles", "(Ptr{Cvoid}, Int32)"), ("alg_get_history_profiles", "(Ptr{Cvoid}, Ref{Int32})"),
                        ("alg_get_history_vio", "(Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32})")):
        assert "ccall((:%s, LIB), Cint, %s" % (name, types) in txt, name
    assert re.search(r"^set_history_profiles!\(bp::BatchedGameProblem, max_records::Integer\)", txt, flags=re.M)


def test_the_oracle_backend_refuses_the_setter(orc):
    import algames_jl_amd as alg
    o = orc.OracleBatch(DI, 2, 5, 0.1, 2)
    with pytest.raises(alg.AlgamesError):
        o.set_history_profiles(4)
    assert o.get_history_profiles() == 0
    prob = alg.scenarios.make_problem("C2", np.arange(2), N=6, backend=orc.lib())
    with pytest.raises(alg.AlgamesError):
        alg.newton_solve(prob, history_profiles=4)
    alg.newton_solve(prob)
    assert prob.stats.vio(0) is None
