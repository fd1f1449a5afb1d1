"""Shared helpers of the iterated-best-response horizon tests (tests/test_ibr_family.py on the CPU, tests/test_gpu_ibr_horizons.py on the GPU):
the configuration lists, the horizon rules, the cached reference solves and the comparison functions, which take the batch under test as an
argument so that the CPU file runs them with the oracle (or the long-double arbiter) in the device's place.  No test lives here.

A. STEP family: one best-response step of every player in turn (outer_iter = inner_iter = 1, no dual reset, reg_0 = 1e-3) on the random
   full-magnitude data of the parity tests -- test_gpu_parity._pair(seed = N) for the base instantiations, ext_horizon_family.pair for the
   extended ones -- at N = 2 ... 18 on the tile shapes, 2 ... 7 on the dense shapes, 2, 3, 4 with ten players.
B. SOLVE family: ibr_newton_solve(ibr_iter = 2, init = True, game_id0 = HS.GID0) on the short-horizon family of test_gpu_horizon_shapes
   (HS.family with its TUNED seeds and OPTS) at N in {2 ... 11} + {FT + 1, FT + 2} on the tile shapes and N = 2 ... 7 on the dense ones.  The
   far-away wall of HS.family (wall = True) switches DI3, UNI3 and UNI4 to their EXT instantiations; it is never active, so these share the
   cached reference of the wall-less problem.  The constrained family ext_horizon_family.ext_family is NOT solved whole under IBR: there the
   oracle and the long-double arbiter part ways themselves (DESIGN.md 2.1 has the figures); active extended rows under IBR are the step family's.
   The two-player bicycle (EXT by its model) takes other discrete paths in double and in long double at one horizon in ten on half of the
   seeds (seed 0 among them): BIC_SEED is the first seed of 1 ... 8 whose ten horizons N = 2 ... 11 all meet the preconditions, so no horizon
   is left out (BIC_SKIP is empty).
C. what IBR adds to the control flow (ordering, the round exit, init = False, ibr_solve_player after ibr_newton_solve) on DI3, UNI4 and (DI, 5, 2).

tests/test_ibr_family.py holds the preconditions: oracle and arbiter agree on every discrete outcome of every game of both families, to a
quarter of the bound the device is held to, and the families are not trivial."""
import numpy as np

import ext_horizon_family as EF
import test_gpu_fuzz as FZ
import test_gpu_horizon_shapes as HS
import test_gpu_parity as GP

DI, UNI, BIC, QUAD = HS.DI, HS.UNI, HS.BIC, HS.QUAD
B = 4
COUNTS = ("status", "outer_iters", "newton_iters", "records", "converged", "ls_failures")
VIO = ("res", "dyn_vio", "con_vio", "sta_vio", "opt_vio")
TOL_STEP, TOL_Z, TOL_LAM = 1e-9, 1e-8, 1e-6                   # test_ibr_best_response_step_parity; test_gpu_parity's docstring
WORST = {}                                                    # (part, shape) -> worst difference (printed by each test)


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))


class LibAsProduct:
    """stands in for the `alg` argument of the _pair helpers and of the families below: the "HIP" half is built on `lib` (the oracle's or
    the arbiter's library)"""

    def __init__(self, lib):
        import algames_jl_amd
        self._lib, self.Batch = lib, algames_jl_amd.Batch

    def hip_lib(self):
        return self._lib


def name(v):
    if isinstance(v, tuple) and len(v) == 2 and v[0] in ("base", "ext"):
        return "%s-%s" % (HS._name(v[1]), v[0])
    return HS._name(v)


# ---- A. the step family -----------------------------------------------------------------------------------------------------------------------------
STEP_OPTS = dict(outer_iter=1, inner_iter=1, dual_reset=0, reg_0=1e-3)
STEP_BASE = HS.BASE_CONFIGS + [(DI, 1, 1), (DI, 3, 1), (DI, 1, 3), (DI, 3, 3), (DI, 4, 3),
                               (DI, 5, 2), (UNI, 6, 2), (DI, 7, 2), (UNI, 8, 2), (UNI, 9, 2), (DI, 10, 2)]
STEP_EXT = EF.TILE_EXT + EF.DENSE_EXT + EF.DENSE_EXT_P10
STEP_PROBLEMS = [("base", cfg) for cfg in STEP_BASE] + [("ext", cfg) for cfg in STEP_EXT]


def step_horizons(kind, cfg):
    """N = 2 ... 18 on the tile shapes, 2 ... 7 on the dense shapes, 2, 3, 4 with ten players (ext_horizon_family.step_horizons)"""
    if kind == "ext":
        return EF.step_horizons(cfg)
    return range(2, 19) if cfg in HS.BASE_CONFIGS else ((2, 3, 4) if cfg[1] == 10 else range(2, 8))


# What the CPU preconditions made of the seed N: a lone player's best response is an all-but-quadratic problem whose full Newton step is
# accepted in every game of every seed-N batch; these are the first seeds of 100 k + N, k = 1 ... 599, with a step that backtracks.  The
# lone double integrator in three dimensions on the base set has none among 4000 seeds at any of its six horizons (NEVER_BACKTRACKS; its
# EXT instantiation backtracks at N = 3).
STEP_SEED = {("base", (DI, 1, 2), 2): 51002, ("base", (UNI, 1, 2), 2): 51002, ("base", (DI, 1, 1), 2): 1802,
             ("ext", (DI, 1, 2), 3): 1803, ("ext", (DI, 1, 3), 3): 803}
NEVER_BACKTRACKS = [("base", (DI, 1, 3))]


def step_pair(alg, orc, kind, cfg, N):
    """(batch on alg.hip_lib(), oracle batch) with the step family's data and options"""
    seed = STEP_SEED.get((kind, tuple(cfg), N))
    g, o = EF.pair(alg, orc, cfg, N, B=B, seed=seed)[:2] if kind == "ext" else GP._pair(alg, orc, *cfg, N, B=B, seed=N if seed is None else seed)
    for b in (g, o):
        b.set_options(**STEP_OPTS)
    return g, o


def others(b, player):
    """(controls (m,) bool, costates (p,) bool): what belongs to the OTHER players in split_traj's U (joint order: column c is player c % p's)
    and L"""
    return np.arange(b.m) % b.p != player, np.arange(b.p) != player


def assert_mask(b, player, z0, z1, dz, what):
    """The horizontal mask of a best response, exactly: the step buffer holds zeros in x_1 and in the other players' controls and costates,
    and the iterate keeps its bits there."""
    ou, ol = others(b, player)
    (X0, U0, L0), (X1, U1, L1), (Xd, Ud, Ld) = b.split_traj(z0), b.split_traj(z1), b.split_traj(dz)
    assert np.all(Xd[:, 0] == 0) and np.array_equal(X1[:, 0], X0[:, 0]), (what, player, "x_1")
    assert np.all(Ud[:, :, ou] == 0), (what, player, "step: another player's control", np.abs(Ud[:, :, ou]).max(initial=0.0))
    assert np.all(Ld[:, ol] == 0), (what, player, "step: another player's costate", np.abs(Ld[:, ol]).max(initial=0.0))
    assert np.array_equal(U1[:, :, ou], U0[:, :, ou]), (what, player, "iterate: another player's control")
    assert np.array_equal(L1[:, ol], L0[:, ol]), (what, player, "iterate: another player's costate")


def assert_same_histories(g, o, what, fields=("outer", "ls_j", "alpha"), rtol=None):
    """every game: the same number of records, `fields` equal; rtol: res, delta and the violations of every record within it"""
    so = o.get_stats()
    for game in range(o.B):
        hg, ho = g.get_history(game), o.get_history(game)
        assert len(hg) == len(ho) == so["records"][game], (what, game, len(hg), len(ho), so["records"][game])
        for f in fields:
            assert np.array_equal(hg[f], ho[f]), (what, game, f, hg[f], ho[f])
        if rtol is not None:
            for f in VIO + ("delta",):
                assert np.allclose(hg[f], ho[f], rtol=rtol, atol=1e-12), (what, game, f, hg[f], ho[f])


def has_profiles(b):
    """the handle can keep per-record violation profiles: not the CPU oracle, not seven to ten players"""
    return "set_history_profiles" not in b.lib.absent and "get_history_profiles" not in b.lib.absent and b.p < 7


def compare_step(g, o, what, key, tol=TOL_STEP):
    """One best-response step of every player in turn on a step_pair: what test_ibr_best_response_step_parity asserts, after every player and
    for every game, plus the mask, two records per call and no violation profile left behind.  Returns the ls_j of every step (a failed line
    search: ls_iter)."""
    profiles = has_profiles(g)
    if profiles:
        g.set_history_profiles(4)
    steps = []
    for player in range(o.p):
        before = [(b.get_traj(0), b.get_stats()["records"].copy()) for b in (g, o)]
        sg, so = g.ibr_solve_player(player), o.ibr_solve_player(player)
        for f in COUNTS:
            assert np.array_equal(sg[f], so[f]), (what, player, f, sg[f], so[f])
        for f in VIO:
            assert np.allclose(sg["last"][f], so["last"][f], rtol=tol, atol=1e-12), (what, player, f, sg["last"][f], so["last"][f])
        for b, s, (z0, r0) in ((g, sg, before[0]), (o, so, before[1])):
            assert np.array_equal(s["records"], r0 + 2), (what, player, "records", r0, s["records"])
            assert_mask(b, player, z0, b.get_traj(0), b.get_traj(2), what)
        for which in (0, 2):
            zg, zo = g.get_traj(which), o.get_traj(which)
            err = np.abs(zg - zo).max() / max(1.0, np.abs(zo).max())
            note(key, err)
            assert err <= tol, (what, player, ("z", None, "step")[which], err)
        assert_same_histories(g, o, (what, player), rtol=tol)
        if profiles:
            assert g.get_history_profiles() == 4, (what, player)
            for game in range(g.B):
                assert all(len(v) == 0 for v in g.get_history_vio(game).values()), (what, player, game, "a violation profile after a best response")
        steps += [int(o.get_history(game)["ls_j"][-2]) for game in range(o.B)]      # (the call's second record follows no line search)
    HS._guards_ok(g)
    return steps


# ---- B. the solve family ----------------------------------------------------------------------------------------------------------------------------
IBR_ITER = 2
SOLVE_SHORT = [(DI, 5, 2), (UNI, 5, 2), (DI, 6, 2), (DI, 7, 2), (DI, 3, 3), (DI, 4, 3), (DI, 3, 1)]           # N = 2 ... 7
SOLVE_TILE = [cfg for cfg in HS.BASE_CONFIGS]                                                                  # p >= 2 and the lone players
SOLVE_WALL = [HS.DI3, HS.UNI3, HS.UNI4]
BIC2 = (BIC, 2, 2)
# What the CPU preconditions made of the bicycle's seed (oracle against arbiter, N = 2 ... 11): seed 1 misses 2.5e-9 at N = 9 (3.4e-9), seeds 0, 3, 6
# and 7 take different discrete paths at N = 8, 10, 11 and 9; seeds 2, 4, 5 and 8 pass every horizon.
BIC_SEED = 2
BIC_SKIP = ()                                                # horizons left out of the bicycle's solves: none
BIC_SOLVE = [BIC2]
# on top of HS.TUNED: the bicycle's seed, and the first seed of 1 ... 8 at which a configuration whose seed-0 games never fail a line search
# under IBR at any of its horizons does so and meets the other preconditions
SEEDS = {BIC2: dict(seed=BIC_SEED), (DI, 3, 3): dict(seed=2), (DI, 4, 1): dict(seed=1), (DI, 3, 1): dict(seed=8)}
# (configuration, N) that stay in the solve family for the parity they check although every best response of every game converges in its
# first outer iteration there at every seed of 0 ... 8 (test_ibr_family.py asserts that it is trivial, so that the entry cannot outlive its reason)
TRIVIAL = [((DI, 1, 2), 3)]


def solve_horizons(cfg):
    if tuple(cfg) in SOLVE_SHORT:
        return list(range(2, 8))
    ft = HS.FT(*cfg)
    return [N for N in sorted(set(range(2, 12)) | {ft + 1, ft + 2}) if not (tuple(cfg) == BIC2 and N in BIC_SKIP)]


def solve_problems():
    """every (configuration, far-away wall) the solve family is run on"""
    return [(cfg, False) for cfg in SOLVE_TILE + SOLVE_SHORT + BIC_SOLVE] + [(cfg, True) for cfg in SOLVE_WALL]


def family_kw(cfg, **kw):
    return {**HS.TUNED.get(tuple(cfg), {}), **SEEDS.get(tuple(cfg), {}), **kw}


def make_of(alg):
    return lambda *a: alg.Batch(alg.hip_lib(), *a[:5], d=a[5])


def family(alg, cfg, N, **kw):
    """HS.family on alg.hip_lib() with the seeds of HS.TUNED and SEEDS"""
    return HS.family(make_of(alg), *cfg, N, B=B, **family_kw(cfg, **kw))


def ibr_solve(b, ibr_iter=IBR_ITER, ordering=None, delta_min=1e-9, init=True):
    return b.ibr_newton_solve(ibr_iter=ibr_iter, ordering=ordering, delta_min=delta_min, init=init, game_id0=HS.GID0)


class SolvedIBR(HS.Solved):
    """HS.Solved whose cached call is the IBR solve of the solve family"""

    def newton_solve(self, *a, **kw):
        raise AttributeError("a cached IBR reference solve has no newton_solve")

    def ibr_newton_solve(self, ibr_iter=IBR_ITER, ordering=None, delta_min=1e-9, init=True, game_id0=HS.GID0):
        assert (ibr_iter, ordering, delta_min, init, game_id0) == (IBR_ITER, None, 1e-9, True, HS.GID0)
        if self._st is None:
            self._st = ibr_solve(self._b)
        return self._st.copy()


_REF = {}


def reference(orc, cfg, N, kind=""):
    """The oracle's (kind "") or the arbiter's ("x") IBR solve of the wall-less family(cfg, N): built once per session, solved on first use."""
    k = (tuple(cfg), N, kind)
    if k not in _REF:
        _REF[k] = SolvedIBR(family(LibAsProduct(orc.lib(kind)), cfg, N))
    return _REF[k]


def compare_solve(g, orc, cfg, N, wall=False, tag=()):
    """ibr_solve(g) against the cached oracle: test_gpu_fuzz._compare_solve with the arbiter (discrete fields identical, z <= 1e-8 x scale,
    else |g - x| <= 4 |orc - x| + tol; its last-record rule), then mu bit-equal and lambda <= 1e-6 relative on the games the oracle converged
    (HS._compare), every game's history equal in outer / ls_j / alpha and in length, nothing in alg_game_stats.reserved.  wall: g carries the
    far-away wall, whose p (N - 1) rows close the constraint vector and never get a multiplier.  Returns the worst |g - oracle| over the
    games of status OK."""
    o, x = reference(orc, cfg, N), reference(orc, cfg, N, kind="x")
    what = (cfg[0], cfg[1], N, HS.DT) + tuple(tag)
    FZ._compare_solve(g, o, what, x=x, solve=ibr_solve)
    so = o.ibr_newton_solve()
    conv = so["converged"] == 1
    (lg, mg), (lo, mo) = g.get_con_duals(), o.get_con_duals()
    rows = lo.shape[1]
    assert lg.shape[1] == rows + (g.p * (N - 1) if wall else 0), (what, lg.shape, lo.shape)
    assert np.all(lg[:, rows:] == 0), (what, "a multiplier on the far-away wall")
    if conv.any():
        assert np.array_equal(mg[conv, :rows], mo[conv]), (what, "mu")
        dl = np.abs(lg[conv, :rows] - lo[conv]).max(initial=0.0)
        assert dl <= TOL_LAM * max(1.0, np.abs(lo[conv]).max(initial=0.0)), (what, "lambda", dl)
    assert_same_histories(g, o, what)
    assert np.all(g.get_stats()["reserved"] == 0), (what, "reserved")
    ok = so["status"] == 0
    return np.abs(g.get_traj(0) - o.get_traj(0))[ok].max(initial=0.0)


def solve_family(alg, orc, cfg, wall, horizons=None, prepare=None):
    """the solve family of one configuration on alg.hip_lib(): compare_solve at every horizon"""
    key = ("solve", tuple(cfg), wall)
    for N in solve_horizons(cfg) if horizons is None else horizons:
        g = family(alg, cfg, N, wall=wall)
        if prepare:
            prepare(g)
        note(key, compare_solve(g, orc, cfg, N, wall=wall, tag=("wall",) if wall else ()))
        HS._guards_ok(g)
    print("IBR solves", name(tuple(cfg)), "wall" if wall else "", "worst |hip - orc| %.2e" % WORST[key])


# ---- C. what IBR adds to the control flow -----------------------------------------------------------------------------------------------------------
FLOW_CONFIGS = [HS.DI3, HS.UNI4, (DI, 5, 2)]
ROUNDS = 5


def flow_horizons(cfg):
    return (3, 7) if tuple(cfg) in SOLVE_SHORT else (3, 7, HS.FT(*cfg) + 2)


def orderings(p):
    """reversed, and rotated by one"""
    return [list(range(p))[::-1], list(range(1, p)) + [0]]


def assert_flow_parity(g, o, what, tol=TOL_Z):
    """discrete against the oracle (statistics counters, every history's length, outer, ls_j, alpha), z <= tol"""
    sg, so = g.get_stats(), o.get_stats()
    for f in COUNTS:
        assert np.array_equal(sg[f], so[f]), (what, f, sg[f], so[f])
    assert_same_histories(g, o, what)
    zg, zo = g.get_traj(0), o.get_traj(0)
    err = np.abs(zg - zo).max() / max(1.0, np.abs(zo).max())
    note(("flow",) + tuple(what[1:2]), err)
    assert err <= tol, (what, err)


def differs(a, b):
    """per game: the iterates of two batches are not bit-equal"""
    return np.any(a.get_traj(0) != b.get_traj(0), axis=1)


def ordering_case(alg, ref, cfg, N, tol=TOL_Z, ordering_ref=None):
    """ordering reversed and rotated by one: the oracle with the same ordering agrees, and the result differs from the identity ordering's
    in at least one game.  ordering_ref: what the reference side is given instead (the mutation check of tests/test_ibr_family.py)."""
    ident = family(alg, cfg, N)
    ibr_solve(ident)
    for order in orderings(cfg[1]):
        what = ("ordering", name(tuple(cfg)), N, tuple(order))
        g, o = family(alg, cfg, N), family(ref, cfg, N)
        ibr_solve(g, ordering=order); ibr_solve(o, ordering=order if ordering_ref is None else ordering_ref(order))
        assert_flow_parity(g, o, what, tol)
        assert differs(g, ident).any(), (what, "the ordering changes nothing")
        HS._guards_ok(g)


def round_exit_case(alg, ref, cfg, N, tol=TOL_Z):
    """ibr_iter = 5 with delta_min = 1e3 ends after exactly one round: the bits of ibr_iter = 1, the oracle's records, fewer than the
    delta_min = 0 run's, which runs all five rounds (the oracle's records again)."""
    what = ("round exit", name(tuple(cfg)), N)
    one, g, o = family(alg, cfg, N), family(alg, cfg, N), family(ref, cfg, N)
    ibr_solve(one, ibr_iter=1)
    ibr_solve(g, ibr_iter=ROUNDS, delta_min=1e3); ibr_solve(o, ibr_iter=ROUNDS, delta_min=1e3)
    assert_flow_parity(g, o, what + ("delta_min 1e3",), tol)
    HS._same_bits(g, one, what + ("one round",))
    early = g.get_stats()["records"].copy()
    HS._guards_ok(g)
    g, o = family(alg, cfg, N), family(ref, cfg, N)
    ibr_solve(g, ibr_iter=ROUNDS, delta_min=0.0); ibr_solve(o, ibr_iter=ROUNDS, delta_min=0.0)
    assert_flow_parity(g, o, what + ("delta_min 0",), tol)
    ok = o.get_stats()["status"] == 0
    assert ok.any() and np.all(early[ok] < g.get_stats()["records"][ok]), (what, early, g.get_stats()["records"])
    HS._guards_ok(g)
    return early, g.get_stats()["records"]


def stored_plan(b):
    """a handle holding a stored plan whose x_1 is not x0: one round of IBR, x0 moved by 0.01 (alg_set_x0 writes x_1 too), the plan stored again"""
    ibr_solve(b, ibr_iter=1)
    z = b.get_traj(0)
    x0 = z[:, :b.n] + 0.01 * np.cos(np.arange(b.B * b.n)).reshape(b.B, b.n)
    b.set_x0(x0)
    b.set_traj(z)
    return x0


def stored_plan_case(alg, ref, cfg, N, tol=TOL_Z):
    """init = False on a handle holding a stored plan: x_1 becomes x0 (the copy branch of ibr_newton_solve), the bits of a second handle
    prepared the same way, parity with the oracle."""
    what = ("init = False", name(tuple(cfg)), N)
    g, g2, o = family(alg, cfg, N), family(alg, cfg, N), family(ref, cfg, N)
    for b in (g, g2, o):
        x0 = stored_plan(b)
        assert np.any(b.get_traj(0)[:, :b.n] != x0)
        ibr_solve(b, init=False)
        assert np.array_equal(b.get_traj(0)[:, :b.n], x0), (what, "x_1 is not x0")
    HS._same_bits(g, g2, what)
    assert_flow_parity(g, o, what, tol)
    HS._guards_ok(g)


def accumulate_case(alg, ref, cfg, N, tol=TOL_Z):
    """ibr_newton_solve, then ibr_solve_player(1): statistics and history accumulate, the earlier records keep their bits although the
    history buffer has grown, the total is the oracle's."""
    what = ("accumulate", name(tuple(cfg)), N)
    g, o = family(alg, cfg, N), family(ref, cfg, N)
    ibr_solve(g); ibr_solve(o)
    s0 = g.get_stats()
    h0 = [g.get_history(game) for game in range(g.B)]
    s1, so = g.ibr_solve_player(1), o.ibr_solve_player(1)
    assert np.all(s1["records"] >= s0["records"] + 2) and np.all(s1["newton_iters"] >= s0["newton_iters"]) and np.all(s1["ls_failures"] >= s0["ls_failures"]), (what, s0, s1)
    for game in range(g.B):
        h1 = g.get_history(game)
        assert len(h1) == s1["records"][game] > len(h0[game]), (what, game)
        for f in h1.dtype.names:
            assert np.array_equal(h1[f][:len(h0[game])], h0[game][f]), (what, game, f, "an earlier record changed")
    assert_flow_parity(g, o, what, tol)
    HS._guards_ok(g)
