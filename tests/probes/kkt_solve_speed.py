"""Cost of alg_kkt_solve on the C2 shape (3-player DoubleIntegrator, N = 40, 4096 games, after one solve).

    python tests/probes/kkt_solve_speed.py [--games 4096] [--lapack-games 8] [--out FILE]
    ALGAMES_HIP_LIB=<library of the parent commit> python tests/probes/kkt_solve_speed.py --parent [--out FILE]

HIP events on the launch stream (torch events on a torch stream handed to the handle), WARM warm-up calls, then ROUNDS x CALLS calls; median
over the rounds and every round's figure are printed.  alg_kkt_solve is a synchronous call -- launch, then the download of its columns (12
columns x 4096 games x 2106 doubles = 828 MB at C2) -- so the events around it measure kernel + download; the kernel alone is what a kernel trace
of this script shows (rocprofv3 --kernel-trace --stats -- python tests/probes/kkt_solve_speed.py: k_kkt_sens / k_direction rows; in the
trace the X0 calls come first, then the USER calls -- a library from before the one column kernel shows them as k_kkt_solve).
alg_newton_direction is called with NULL outputs through the raw ABI: launch and synchronisation only, its event time is its kernel time.
  --parent   the library is a build of the parent commit, alternated with runs of this build by the caller: k_direction, newton_solve and, when
             the library exports alg_kkt_solve, its X0 and USER rows; not the host route."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import algames_jl_amd as alg  # noqa: E402

WARM, ROUNDS, CALLS = 3, 7, 3
OUT = [sys.stdout]


def say(s):
    for f in OUT:
        print(s, file=f, flush=True)


def timed(stream, fn, calls=CALLS, rounds=ROUNDS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ms)), ms


def row(name, med, ms):
    say("%-44s median %9.3f ms   rounds %s" % (name, med, " ".join("%.3f" % v for v in ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--lapack-games", type=int, default=8)
    ap.add_argument("--parent", action="store_true")
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
    say("# KKT solves at C2 (%d games, N = %d, S = %d) on %s, library %s; %d warm-up calls, %d rounds x %d calls, HIP events on the launch stream"
        % (B, b.N, b.S, torch.cuda.get_device_name(0), "of the parent commit" if a.parent else "of this tree", WARM, ROUNDS, CALLS))
    d_med, d_ms = timed(stream, lambda: b.lib.check(b.lib.newton_direction(b.h, 0.0, None, None)))
    row("k_direction (alg_newton_direction, no download)", d_med, d_ms)
    say("# 12 x k_direction = %.3f ms" % (12 * d_med))
    s_med, s_ms = timed(stream, lambda: b.newton_solve_async(init=True, game_id0=0), calls=2)
    row("newton_solve of the batch", s_med, s_ms)
    if "kkt_solve" in b.lib.absent:
        return
    b.newton_solve(init=True, game_id0=0)
    X = np.empty((B, b.n, b.S)); st = np.empty(B, dtype=np.int32)
    xp, sp = X.ctypes.data_as(alg._abi._D), st.ctypes.data_as(alg._abi._I)
    k_med, k_ms = timed(stream, lambda: b.lib.check(b.lib.kkt_solve(b.h, 0.0, alg.ALG_KKT_RHS_X0, 0, None, 0, B, xp, sp)), calls=1)
    row("alg_kkt_solve X0, %d columns (+ %.0f MB download)" % (b.n, X.nbytes / 1e6), k_med, k_ms)
    assert np.all(st == 0)
    say("# X0 call / (12 x k_direction) = %.3f ; X0 call / newton_solve = %.3f" % (k_med / (12 * d_med), k_med / s_med))
    R = np.random.default_rng(0).uniform(-1.0, 1.0, (B, 12, b.S))
    XU = np.empty_like(R)
    rp, up = R.ctypes.data_as(alg._abi._D), XU.ctypes.data_as(alg._abi._D)
    u_med, u_ms = timed(stream, lambda: b.lib.check(b.lib.kkt_solve(b.h, 0.0, alg.ALG_KKT_RHS_USER, 12, rp, 0, B, up, sp)), calls=1)
    row("alg_kkt_solve USER, 12 columns (+ %.0f MB upload, %.0f MB download)" % (R.nbytes / 1e6, XU.nbytes / 1e6), u_med, u_ms)
    assert np.all(st == 0)
    if a.parent:
        return
    # the host route as context: dense Jacobians to the host, LAPACK there
    G = a.lapack_games
    t0 = time.perf_counter()
    J = b.residual_jacobian(0.0, games=(0, G))
    t1 = time.perf_counter()
    R = np.zeros((G, b.S, b.n))
    Xh = np.stack([np.linalg.solve(J[g], R[g]) for g in range(G)])
    t2 = time.perf_counter()
    say("# host route, %d games: dense Jacobians to the host %.1f ms (%.0f MB), numpy LAPACK solve %.1f ms  -> %.2f ms per game; device call: %.4f ms per game"
        % (G, 1e3 * (t1 - t0), J.nbytes / 1e6, 1e3 * (t2 - t1), 1e3 * (t2 - t0) / G, k_med / B))
    assert Xh.shape == (G, b.S, b.n)


if __name__ == "__main__":
    main()
