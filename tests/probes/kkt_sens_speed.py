"""Cost of alg_kkt_sensitivity on the C2 shape (3-player DoubleIntegrator, N = 40, 4096 games, after one solve).

    python tests/probes/kkt_sens_speed.py [--games 4096] [--out FILE]

The method of kkt_solve_speed.py: HIP events on the launch stream, WARM warm-up calls, ROUNDS x CALLS calls, median over the rounds and every
round's figure.  The entry point is synchronous (launch, then the download of the slice), so the events measure kernel + download; with
steps = (0, 1) the download is 54 doubles per column and game (21 MB for 12 columns instead of 828), and the call's time is the kernel's to
within that copy -- the rows marked `slice` are read as kernel times.  Rows:
  alg_kkt_solve X0, all steps            the parent's entry point, 12 columns and the 828 MB download
  X0 / Q / R / uf, slice                 the unit columns of each parameter (12 / 12 / 6 / 6 eliminations), Q + R + uf against 2 x X0
  X0, all steps                          the new entry point with nothing sliced: equal work and download to alg_kkt_solve X0
  one direction of Q, slice              one elimination against the parameter's 12
  collision_cost / collision_radius      the loaders with the pair terms, per column against Q's
  C3 R / control_bound, slice            the control-bound loader on the C3 shape (C2 carries no control bound), per column against R's"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import algames_jl_amd as alg  # noqa: E402
from kkt_solve_speed import OUT, row, say, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT.append(open(a.out, "a"))
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    B = a.games
    prob = alg.scenarios.make_problem("C2", np.arange(B))
    b = prob.batch
    b.set_stream(stream.cuda_stream)
    alg.newton_solve(prob)
    say("# parameter sensitivities at C2 (%d games, N = %d, S = %d, b = %d) on %s" % (B, b.N, b.S, b.b, torch.cuda.get_device_name(0)))
    D, I = alg._abi._D, alg._abi._I
    st = np.empty(B, dtype=np.int32)
    full = np.empty((B, b.n, b.S))
    k_med, k_ms = timed(stream, lambda: b.lib.check(b.lib.kkt_solve(b.h, 0.0, alg.ALG_KKT_RHS_X0, 0, None, 0, B, full.ctypes.data_as(D), st.ctypes.data_as(I))), calls=1)
    row("alg_kkt_solve X0, all steps (%.0f MB)" % (full.nbytes / 1e6), k_med, k_ms)

    def sens(param, steps, out, dirs=None, ndir=0):
        s0, ns = steps
        return lambda: b.lib.check(b.lib.kkt_sensitivity(b.h, 0.0, param, ndir, None if dirs is None else dirs.ctypes.data_as(D), 0, B, s0, ns,
                                                         out.ctypes.data_as(D), st.ctypes.data_as(I)))
    med = {}
    for name in ("x0", "Q", "R", "uf"):
        code = alg._abi.PARAM_KINDS.index(name)
        out = np.empty((B, b.param_len(code), b.b))
        med[name], ms = timed(stream, sens(code, (0, 1), out))
        row("%s, %d unit columns, slice (0, 1) (%.1f MB)" % (name, out.shape[1], out.nbytes / 1e6), med[name], ms)
        assert np.all(st == 0)
    say("# Q + R + uf (24 columns) = %.3f ms; 2 x X0 (24 columns) = %.3f ms; ratio %.3f" % (med["Q"] + med["R"] + med["uf"], 2 * med["x0"],
                                                                                          (med["Q"] + med["R"] + med["uf"]) / (2 * med["x0"])))
    say("# d u_1 / d x0 through the slice: %.3f ms against %.3f ms for the full X0 call (%.1f x)" % (med["x0"], k_med, k_med / med["x0"]))
    f_med, f_ms = timed(stream, sens(alg.ALG_PARAM_X0, (0, 0), full), calls=1)
    row("x0, 12 unit columns, all steps (%.0f MB)" % (full.nbytes / 1e6), f_med, f_ms)
    V = np.random.default_rng(0).uniform(-1.0, 1.0, (B, 1, b.param_len("Q")))
    one = np.empty((B, 1, b.b))
    d_med, d_ms = timed(stream, sens(alg.ALG_PARAM_Q, (0, 1), one, V, 1))
    row("one direction of Q, slice (0, 1)", d_med, d_ms)
    say("# one direction / %d unit columns of Q = %.3f" % (V.shape[2], d_med / med["Q"]))
    # the loaders that read more per entry: the pair terms (positions of i and j, scenario numbers, lambda and mu of the pair's row) ...
    for name in ("collision_cost", "collision_radius"):
        code = alg._abi.PARAM_KINDS.index(name)
        out = np.empty((B, b.param_len(code), b.b))
        med[name], ms = timed(stream, sens(code, (0, 1), out))
        row("%s, %d unit columns, slice (0, 1)" % (name, out.shape[1]), med[name], ms)
        say("# %s: %.4f ms per column against %.4f for Q" % (name, med[name] / out.shape[1], med["Q"] / 12))
    # ... and the control bounds (lambda and mu of two rows per entry), on the C3 shape: C2 carries no control bound
    B3 = min(B, 1024)
    prob3 = alg.scenarios.make_problem("C3", np.arange(B3))
    b3 = prob3.batch
    b3.set_stream(stream.cuda_stream)
    alg.newton_solve(prob3)
    st3 = np.empty(B3, dtype=np.int32)
    say("# C3 shape (%d games, N = %d, n = %d, m = %d, b = %d)" % (B3, b3.N, b3.n, b3.m, b3.b))
    per = {}
    for name in ("R", "control_bound"):
        code = alg._abi.PARAM_KINDS.index(name)
        out = np.empty((B3, b3.param_len(code), b3.b))
        fn = lambda: b3.lib.check(b3.lib.kkt_sensitivity(b3.h, 0.0, code, 0, None, 0, B3, 0, 1, out.ctypes.data_as(D), st3.ctypes.data_as(I)))
        m3, ms = timed(stream, fn)
        per[name] = m3 / out.shape[1]
        row("C3 %s, %d unit columns, slice (0, 1)" % (name, out.shape[1]), m3, ms)
    say("# C3: control_bound %.4f ms per column against %.4f for R" % (per["control_bound"], per["R"]))


if __name__ == "__main__":
    main()
