"""tests/con_reference.py, the numpy statement of the constraint rows, pinned on the oracle: random trajectories set on oracle-backed problems,
kat_evaluate_con() -- the oracle's evaluate!(game_con, traj) -- against con_reference.plan.

Tolerance.  A finite row is a sum of at most seven products of differences of two inputs (the cylinder: r r - t0^2 - t1^2 - t2^2 + ta^2 with
t = q - p): fewer than about 25 rounding operations, each on a partial sum bounded by the row's scale s = the sum of the absolute values of
its terms, so two correct evaluations differ by less than 25 * 2^-53 * s.  The bound held here is 64 * 2^-53 * s (con_reference.TOL): the
factor covers contraction differences, one side fusing a multiply into an add where the other rounds twice.  Inert rows and rows of
infinite bounds must be equal exactly.  The data is drawn so that no indicator argument (the walls' left / right, the 3-D walls' four flags,
the cylinders' axial range) lies within 1e-6 of its switch, and so that every kind has rows of both signs: both are asserted."""
import numpy as np
import pytest

import con_reference as CR


@pytest.mark.parametrize("N", [2, 3, 5])
@pytest.mark.parametrize("name", CR.CASES)
def test_the_statement_is_the_oracles_evaluate(orc, name, N):
    B = 3
    prob, z = CR.make_case(name, N, B, backend=orc.lib(), seed=N)
    b = prob.batch
    b.set_traj(z)
    got = orc.OracleBatch.kat_evaluate_con(b)          # (the problem holds a plain Batch on the oracle library: the hook is OracleBatch's)
    tab = CR.tables(prob)
    ref, scale, margin, kinds = CR.plan(b, tab, tab["nums"], z, N)
    assert got.shape == ref.shape == (B, b.con_len) and b.con_len == (N - 1) * (ref.shape[1] // (N - 1))
    CR.preconditions(ref, scale, margin, kinds)
    worst = CR.check(got, ref, scale, f"{name} N={N}")
    # the kinds the case is about are there, with inert and -inf rows where the case has masks, subsets and infinite bounds
    want = {"di2_p3_base": {0, 1}, "di2_p3_ext": {0, 1, 2, 3, 4}, "di2_p1": {1}, "di1_p2": {0, 1}, "di3_p2": {0, 1, 5, 6},
            "uni_p4": {0, 1, 2}, "bic_p2": {0, 1, 2}, "quad_p2": {0, 1, 2}, "di2_p10_sb": {0, 1, 2}}[name]
    assert set(kinds.tolist()) - {-1} == want
    if name != "di2_p10_sb":
        assert np.isneginf(ref).any()
    if name in ("di2_p3_ext", "di3_p2"):
        assert (scale == 0).any() and np.all(ref[scale == 0] == 0.0)
    print(f"{name} N={N}: worst error / tolerance {worst:.3g}")


def test_the_index_map_is_the_abis_layout(orc):
    """(knot, row) -> ABI index: a permutation, pair rows pair-major, control rows step-major, extended rows player-major"""
    prob, z = CR.make_case("di2_p3_ext", 4, 1, backend=orc.lib())
    b, tab = prob.batch, CR.tables(prob)
    idx = CR.abi_index(b, tab, tab["nums"], 4)
    K1 = idx.shape[1]
    assert idx.shape == (3, K1) and K1 * 3 == b.con_len and K1 > 64
    assert idx[0, 0] == 0 and idx[1, 0] == 1 and idx[0, 1] == 3                       # pair q: q (N - 1) + k
    assert idx[0, 6] == 6 * 3 and idx[1, 6] == 6 * 3 + 2 * b.m                        # control rows: one step after the other
    assert idx[0, 6 + 2 * b.m] == 6 * 3 + 2 * b.m * 3 and idx[0, 6 + 2 * b.m + 2 * b.n] == idx[0, 6 + 2 * b.m] + 3 * 2 * b.n   # players apart by (N - 1) rows
