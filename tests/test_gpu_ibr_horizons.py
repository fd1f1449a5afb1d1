"""Best-response steps and whole IBR solves over kernel shapes and horizons.

Iterated best response (alg_ibr_solve_player, alg_ibr_newton_solve, kernel k_ibr<C>) is compiled for every one-wavefront configuration and has
instantiations of its own: the masked assemble passes with the player-specific violations and the proximal term on one player's rows, the
Newton direction and the costate sweep with the horizontal mask INSIDE the sweeps (whose prefetch rings end in a clamped tail), the masked
line search, ibr_push_stats and the round exit.  The other solver paths are held over short and ring-edge horizons by
tests/test_gpu_horizon_shapes.py and tests/test_gpu_ext_horizons.py; here IBR is, on the families of tests/ibr_family.py, whose preconditions
tests/test_ibr_family.py holds on the CPU (oracle against the long-double arbiter).  B = 4 throughout, debug_check_guards after every handle.

  A. one best-response step of every player in turn on random full-magnitude data, every one-wavefront shape (base, EXT, dense, d = 1 and 3,
     five to ten players), N = 2 ... 18 / 2 ... 7 / 2, 3, 4: after every player the counts equal, the last record 1e-9, z and the step <= 1e-9
     relative, every game's history equal in length, outer, ls_j, alpha and within 1e-9 in its values; the step buffer EXACTLY zero in x_1 and in
     the other players' controls and costates and the iterate's bits kept there; two records per call; no violation profile;
  B. whole solves, ibr_iter = 2, on the short-horizon family at N in {2 ... 11} + {FT + 1, FT + 2} (dense shapes: 2 ... 7): the rule of
     test_gpu_fuzz._compare_solve with the arbiter, mu bit-equal and lambda <= 1e-6 relative on the games the oracle converged, every
     game's history equal in outer / ls_j / alpha, reserved == 0;
  C. what IBR adds to the control flow: `ordering`, the round exit, init = False on a stored plan, ibr_solve_player after ibr_newton_solve;
  D. bit-level properties that need no reference: a second solve on the handle, a permuted batch, the team's handle layout, the block-reading
     twins of the base kernels."""
import numpy as np
import pytest

import failure_family as FF
import ibr_family as IF
import test_gpu_horizon_shapes as HS
from test_gpu_horizon_shapes import DI3, UNI3, UNI4

pytestmark = pytest.mark.gpu


# ---- A. one best-response step of every player ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cfg", IF.STEP_PROBLEMS, ids=[IF.name(v) for v in IF.STEP_PROBLEMS])
def test_best_response_step_over_horizons(alg, orc, kind, cfg):
    key = ("step", kind, cfg)
    for N in IF.step_horizons(kind, cfg):
        g, o = IF.step_pair(alg, orc, kind, cfg, N)
        if kind == "ext" or cfg in HS.BASE_CONFIGS:
            assert g.get_scenario_kernels() == ((HS.EXT, 1) if kind == "ext" else (HS.EXT, 0))
        IF.compare_step(g, o, (kind, IF.name(cfg), N), key)
    print("best-response step", kind, cfg, "worst relative difference of z and of the step %.2e" % IF.WORST[key])


# ---- B. whole IBR solves ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,wall", IF.solve_problems(), ids=lambda v: IF.name(v) or ("wall" if v else "plain"))
def test_ibr_solve_over_horizons(alg, orc, cfg, wall):
    def prepare(g):
        if wall or cfg[0] == IF.BIC or cfg in HS.BASE_CONFIGS:
            assert g.get_scenario_kernels() == (HS.EXT, 1 if wall or cfg[0] == IF.BIC else 0)
    IF.solve_family(alg, orc, cfg, wall, prepare=prepare)


# ---- C. what IBR adds to the control flow -----------------------------------------------------------------------------------------------------------
def _oracle(orc):
    return IF.LibAsProduct(orc.lib())


@pytest.mark.parametrize("cfg", IF.FLOW_CONFIGS, ids=IF.name)
def test_ibr_ordering(alg, orc, cfg):
    """reversed and rotated by one: the oracle with the same ordering agrees, the result is not the identity ordering's"""
    for N in IF.flow_horizons(cfg):
        IF.ordering_case(alg, _oracle(orc), cfg, N)


@pytest.mark.parametrize("cfg", IF.FLOW_CONFIGS, ids=IF.name)
def test_ibr_round_exit(alg, orc, cfg):
    """ibr_iter = 5: delta_min = 1e3 ends after exactly one round (the bits of ibr_iter = 1), delta_min = 0 runs all five"""
    for N in IF.flow_horizons(cfg):
        IF.round_exit_case(alg, _oracle(orc), cfg, N)


@pytest.mark.parametrize("cfg", IF.FLOW_CONFIGS, ids=IF.name)
def test_ibr_solve_from_a_stored_plan(alg, orc, cfg):
    for N in IF.flow_horizons(cfg):
        IF.stored_plan_case(alg, _oracle(orc), cfg, N)


@pytest.mark.parametrize("cfg", IF.FLOW_CONFIGS, ids=IF.name)
def test_ibr_solve_player_after_ibr_newton_solve(alg, orc, cfg):
    for N in IF.flow_horizons(cfg):
        IF.accumulate_case(alg, _oracle(orc), cfg, N)
    print("IBR control flow", cfg, "worst relative difference %.2e" % IF.WORST[("flow", IF.name(tuple(cfg)))])


# ---- D. bit-level properties that need no reference ---------------------------------------------------------------------------------------------------
BIT_CONFIGS = [DI3, UNI3, UNI4]
PERM = [2, 0, 3, 1]


@pytest.mark.parametrize("cfg", BIT_CONFIGS, ids=IF.name)
def test_a_second_ibr_solve_gives_the_same_bits(alg, cfg):
    """nothing of a solve (maximum(stats.Δ_traj) in tc[6], LS_count, the trial and step buffers) reaches the next one on the handle"""
    for N in HS.handoff_horizons(cfg):
        g, fresh = IF.family(alg, cfg, N), IF.family(alg, cfg, N)
        IF.ibr_solve(g); IF.ibr_solve(fresh)
        st = IF.ibr_solve(g)
        assert st["newton_iters"].min() > 0, (cfg, N)
        HS._same_bits(g, fresh, (cfg, N, "second solve"))
        HS._guards_ok(g)


class _Permuted:
    """a batch whose per-game data (x0, LQR) arrive permuted: game q gets the data of game PERM[q]"""

    def __init__(self, b):
        self._b = b

    def set_x0(self, x0):
        self._b.set_x0(np.asarray(x0)[PERM])

    def set_lqr(self, *a):
        self._b.set_lqr(*(np.asarray(v)[PERM] for v in a))

    def __getattr__(self, k):
        return getattr(self._b, k)


@pytest.mark.parametrize("cfg", BIT_CONFIGS, ids=IF.name)
def test_a_permuted_batch_gives_the_permuted_bits(alg, cfg):
    """games are independent blocks: init = False on a stored plan (the initial draw of init = True depends on the game's id)"""
    make = IF.make_of(alg)
    for N in HS.handoff_horizons(cfg):
        a = IF.family(alg, cfg, N)
        b = HS.family(lambda *v: _Permuted(make(*v)), *cfg, N, B=IF.B, **IF.family_kw(cfg))._b
        z = 0.01 * np.random.default_rng([N, 3]).random((a.B, a.traj_len))
        a.set_traj(z); b.set_traj(z[PERM])
        sa, sb = IF.ibr_solve(a, init=False), IF.ibr_solve(b, init=False)
        assert sa["newton_iters"].min() > 0, (cfg, N)
        for q, game in enumerate(PERM):
            for i, (x, y) in enumerate(zip(FF.game_bits(a, game), FF.game_bits(b, q))):
                assert np.shape(x) == np.shape(y) and np.array_equal(x, y, equal_nan=True), (cfg, N, "permuted batch", q, i)
        HS._guards_ok(b)


@pytest.mark.parametrize("cfg", BIT_CONFIGS, ids=IF.name)
def test_ibr_on_a_teams_handle_layout(alg, cfg):
    """k_ibr always runs one wavefront per game, but the handle's layout is the team's: set_waves_per_game(4) (UNI4: also 2) before the
    solve gives the bits of set_waves_per_game(1)"""
    for N in HS.handoff_horizons(cfg):
        one = IF.family(alg, cfg, N)
        one.set_waves_per_game(1)
        IF.ibr_solve(one)
        for nw in ((2, 4) if cfg == UNI4 else (4,)):
            g = IF.family(alg, cfg, N)
            g.set_waves_per_game(nw)
            assert g.get_waves_per_game() == nw
            IF.ibr_solve(g)
            HS._same_bits(g, one, (cfg, N, nw))
            assert np.all(g.get_stats()["reserved"] == 0), (cfg, N, nw)
            HS._guards_ok(g)


@pytest.mark.parametrize("cfg", BIT_CONFIGS, ids=IF.name)
def test_ibr_on_the_block_reading_twins(alg, cfg):
    """alg_set_scenario_kernels(BASE) with every game's block a copy of the shared values: the base kernel's bits
    (test_block_reading_twins_give_the_base_kernels_bits for newton_solve)"""
    for N in HS.handoff_horizons(cfg):
        a, b = IF.family(alg, cfg, N), IF.family(alg, cfg, N)
        b.set_scenario_kernels(HS.BASE)
        kinds = [k for k in (HS.K_RAD, HS.K_COST, HS.K_CTL) if b.scenario_data_len(k)]
        assert kinds == [HS.K_RAD, HS.K_COST, HS.K_CTL]
        for k in kinds:
            b.set_scenario_data(k, b.get_scenario_data(k))
        assert a.get_scenario_kernels() == (HS.EXT, 0) and b.get_scenario_kernels() == (HS.BASE, 2)
        IF.ibr_solve(a); IF.ibr_solve(b)
        HS._same_bits(a, b, (cfg, N, "twins"))
        HS._guards_ok(b)
