"""The preconditions of tests/test_gpu_ibr_horizons.py, on the CPU: the two problem families of tests/ibr_family.py are well posed under
iterated best response -- the oracle (double) and the long-double arbiter agree on every discrete outcome of every game, to a quarter of
the bound the device is held to -- and the comparison functions of the GPU tests pass with the oracle's library in the device's place.

  1. step family, every (configuration, N): ibr_family.compare_step with the ARBITER in the device's place and a quarter of its bound --
     every discrete field and every history's ls_j / alpha equal, z, step and record fields <= 2.5e-10 relative; per configuration at least
     one accepted step has 1 < ls_j < ls_iter (ibr_family.STEP_SEED: the seeds of the lone players, whose seed-N steps never backtrack;
     NEVER_BACKTRACKS: the one configuration in which no seed was found, held here to be that);
  2. the mask: in the oracle (and in the arbiter) the step buffer holds exact zeros in x_1 and in the other players' controls and costates
     and the iterate keeps its bits there (compare_step asserts it on both of its batches): what entitles the GPU test to demand equality;
  3. solve family, every (configuration, N): every discrete field and every history's outer / ls_j / alpha equal in every game -- no game
     is left out of any configuration, the two-player bicycle at ibr_family.BIC_SEED included; |oracle - arbiter| <= 2.5e-9 relative per
     game (the rule of tests/test_horizon_family.py); from N = 3 on some game has a best response with at least two outer iterations and
     a multiplier above 1e-2 (ibr_family.TRIVIAL: the one (configuration, N) that has none at any seed, held here to be that); per configuration at least one failed line search and one backtracked step;
  4. the control-flow cases: a reversed and a rotated ordering change the result of at least one game, the fifth round of the
     delta_min = 0 run makes records; the bodies pass with the arbiter in the device's place at 2.5e-9
     (N = 3 and 7);
  5. the bodies of the GPU tests pass on the oracle, the EXT handles with the far-away wall against the wall-less reference among them;
  6. mutations: one other player's control entry of the step one ulp off zero fails the mask assertion; two entries of `ordering`
     swapped on one side only fail the ordering case.  (The third mutation one would like -- the last knot's row dropped from a player's
     masked norm, emulated by an oracle run at N - 1 -- is not practical: a record's `res` is the FULL residual norm, the masked norm only
     decides the line search, and the constraint rows of a problem at N - 1 are no prefix of those at N.)

A family that misses one of these is changed (seed, horizon list), not the condition."""
import numpy as np
import pytest

import ibr_family as IF
import test_gpu_horizon_shapes as HS


def _orc_as(orc, kind=""):
    return IF.LibAsProduct(orc.lib(kind))


@pytest.mark.parametrize("kind,cfg", IF.STEP_PROBLEMS, ids=[IF.name(v) for v in IF.STEP_PROBLEMS])
def test_step_family_is_exact_and_backtracks(orc, kind, cfg):
    steps, Ns = [], list(IF.step_horizons(kind, cfg))
    for N in Ns:
        x, o = IF.step_pair(_orc_as(orc, "x"), orc, kind, cfg, N)
        steps += IF.compare_step(x, o, (kind, IF.name(cfg), N, "arbiter"), ("step x", kind, cfg), tol=0.25 * IF.TOL_STEP)
        ls_iter = o.opts.ls_iter
        if N in (Ns[0], Ns[len(Ns) // 2], Ns[-1]):                       # (the same code as above at the bound of the GPU test: three horizons)
            a, o = IF.step_pair(_orc_as(orc), orc, kind, cfg, N)
            IF.compare_step(a, o, (kind, IF.name(cfg), N, "oracle in the device's place"), ("step o", kind, cfg))
    steps = np.array(steps)
    print(kind, cfg, "worst |orc - arbiter| %.2e relative;" % IF.WORST[("step x", kind, cfg)], len(steps), "steps,",
          int(((steps > 1) & (steps < ls_iter)).sum()), "backtracked,", int((steps == ls_iter).sum()), "failed line searches")
    assert np.any((steps > 1) & (steps < ls_iter)) != ((kind, cfg) in IF.NEVER_BACKTRACKS), (kind, cfg, steps)


def _best_responses(orc, cfg, N, o):
    """(outer iterations, largest multiplier), each (solves, B), after every best response of the cached solve `o`: every player's solve resets
    the multipliers, so the end of the solve shows the last one's only.  The solve is replayed on a second oracle batch, one
    ibr_solve_player after the other, and must end on the bits of `o`."""
    b = IF.family(_orc_as(orc), cfg, N)
    b.init_traj(game_id0=HS.GID0, use_shift=True)
    out = []
    for _ in range(IF.IBR_ITER):
        for player in range(b.p):
            st = b.ibr_solve_player(player)
            out.append((st["outer_iters"].copy(), b.get_con_duals()[0].max(axis=1, initial=0.0)))
    assert np.array_equal(b.get_traj(0), o.get_traj(0)) and np.array_equal(st["records"], o.get_stats()["records"]), (cfg, N, "the replay is not the solve")
    return np.array([a for a, _ in out]), np.array([l for _, l in out])


PROBLEMS = [cfg for cfg, wall in IF.solve_problems() if not wall]


@pytest.mark.parametrize("cfg", PROBLEMS, ids=IF.name)
def test_solve_family_is_neither_trivial_nor_amplifying(orc, cfg):
    backtracked = failed = False
    worst = 0.0
    assert not (tuple(cfg) == IF.BIC2 and len(IF.BIC_SKIP) > 2)
    for N in IF.solve_horizons(cfg):
        o, x = IF.reference(orc, cfg, N), IF.reference(orc, cfg, N, kind="x")
        so, sx = o.ibr_newton_solve(), x.ibr_newton_solve()
        ls_iter = o.opts.ls_iter
        for f in IF.COUNTS:
            assert np.array_equal(so[f], sx[f]), (cfg, N, f, so[f], sx[f])
        IF.assert_same_histories(x, o, (cfg, N))
        zo, zx = o.get_traj(0), x.get_traj(0)
        for game in range(o.B):
            err = np.abs(zo[game] - zx[game]).max() / max(1.0, np.abs(zx[game]).max())
            worst = max(worst, err)
            assert err <= 2.5e-9, (cfg, N, game, err)
            h = o.get_history(game)
            steps = h["ls_j"][h["ls_j"] > 0]                              # (the closing record of a best response follows no line search)
            backtracked |= bool(np.any((steps > 1) & (steps < ls_iter)))
        failed |= bool(so["ls_failures"].sum() > 0)
        if N >= 3:
            outer, lam = _best_responses(orc, cfg, N, o)
            assert np.any((outer >= 2) & (lam > 1e-2)) != ((tuple(cfg), N) in IF.TRIVIAL), (cfg, N, outer, lam)
    print(cfg, "IBR solves: worst |orc - arbiter| %.2e" % worst)
    assert backtracked and failed, (cfg, backtracked, failed)


@pytest.mark.parametrize("cfg,wall", IF.solve_problems(), ids=lambda v: IF.name(v) or ("wall" if v else "plain"))
def test_the_solve_comparison_passes_on_the_oracle(orc, cfg, wall):
    IF.solve_family(_orc_as(orc), orc, cfg, wall)


@pytest.mark.parametrize("cfg", IF.FLOW_CONFIGS, ids=IF.name)
def test_the_control_flow_cases_are_well_posed(orc, cfg):
    """every case of part C with the arbiter, then with the oracle, in the device's place; the rounds of the round-exit case really run"""
    a, x = _orc_as(orc), _orc_as(orc, "x")
    for N in IF.flow_horizons(cfg):
        for dev, tol in ((x, 0.25 * IF.TOL_Z), (a, IF.TOL_Z)):
            if dev is x and N > 7:                                        # (long double: at the two short horizons)
                continue
            IF.ordering_case(dev, a, cfg, N, tol)
            early, full = IF.round_exit_case(dev, a, cfg, N, tol)
            IF.stored_plan_case(dev, a, cfg, N, tol)
            IF.accumulate_case(dev, a, cfg, N, tol)
        four = IF.family(a, cfg, N)
        s4 = IF.ibr_solve(four, ibr_iter=IF.ROUNDS - 1, delta_min=0.0)
        ok = s4["status"] == 0
        assert ok.all() and np.all(s4["records"] < full), (cfg, N, "the fifth round made no record", s4["records"], full)
    print(cfg, "control flow: worst relative difference %.2e" % IF.WORST[("flow", IF.name(tuple(cfg)))])


def test_a_step_entry_one_ulp_off_zero_fails_the_mask_assertion(orc):
    kind, cfg, N = "base", HS.UNI3, 5
    a, o = IF.step_pair(_orc_as(orc), orc, kind, cfg, N)
    z0 = o.get_traj(0)
    o.ibr_solve_player(1)
    z1, dz = o.get_traj(0), o.get_traj(2)
    IF.assert_mask(o, 1, z0, z1, dz, "untouched")
    X, U, L = o.split_traj(dz)
    assert U[2, 3, 0] == 0.0 and U[2, 3, 1] != 0.0                         # player 0's first control, player 1's
    U[2, 3, 0] = np.nextafter(0.0, 1.0)
    with pytest.raises(AssertionError, match="another player's control"):
        IF.assert_mask(o, 1, z0, z1, o.join_traj(X, U, L), "step")
    X, U, L = o.split_traj(z1)
    L[1, 2, 0, 0] = np.nextafter(L[1, 2, 0, 0], np.inf)                    # player 2's costate in the iterate
    with pytest.raises(AssertionError, match="another player's costate"):
        IF.assert_mask(o, 1, z0, o.join_traj(X, U, L), dz, "iterate")


@pytest.mark.parametrize("cfg", IF.FLOW_CONFIGS, ids=IF.name)
def test_an_ordering_swapped_on_one_side_fails_the_ordering_case(orc, cfg):
    def swapped(order):
        return [order[1], order[0]] + order[2:]
    a = _orc_as(orc)
    with pytest.raises(AssertionError):
        IF.ordering_case(a, a, cfg, 7, ordering_ref=swapped)


def test_horizon_rules_and_lists():
    """part A's horizons are the lists of ext_horizon_family.step_horizons; part B's hold every ring depth (4, 6, 8) with both neighbours as
    N - 1 on the tile shapes; every IBR kernel family of the issue is in the step family"""
    for kind, cfg in IF.STEP_PROBLEMS:
        Ns = list(IF.step_horizons(kind, cfg))
        assert Ns in (list(range(2, 19)), list(range(2, 8)), [2, 3, 4]), (kind, cfg)
        assert (Ns == [2, 3, 4]) == (cfg[1] == 10), (kind, cfg)
    for cfg, wall in IF.solve_problems():
        Ns = IF.solve_horizons(cfg)
        if tuple(cfg) in IF.SOLVE_SHORT:
            assert Ns == list(range(2, 8))
        else:
            ft = HS.FT(*cfg)
            assert set(range(2, 12)) | {ft + 1, ft + 2} == set(Ns) | (set(IF.BIC_SKIP) if tuple(cfg) == IF.BIC2 else set()), (cfg, Ns)
            assert {d + k for d in (4, 6, 8) for k in (0, 1, 2)} <= set(range(2, 12))
    assert len(IF.BIC_SKIP) <= 2 and 1 <= IF.BIC_SEED <= 8
    assert (HS.UNI, 10, 2) not in [c for c, _ in IF.solve_problems()]
    assert {(IF.DI, 1, 1), (IF.DI, 3, 3), (IF.DI, 5, 2), (IF.DI, 10, 2), (IF.UNI, 9, 2)} <= set(IF.STEP_BASE)
