"""Scheduled receding-horizon loop: the fused launch (alg_mpc_set_schedule + alg_mpc_solve) against the step-wise loop of the same library
(per MPC step: the step's rows through alg_set_scenario_data / alg_set_lqr, one alg_newton_solve_async launch, one alg_mpc_advance launch)
-- all a caller could do before schedules existed.  The C5 shape: scenarios.c5_scheduled, 64 seeds x 200 MPC steps, one row per step.

    python tests/probes/mpc_schedule_speed.py [--seeds 64] [--steps 200] [--reps 5] [--out profiles/mpc_schedule_speed.txt]

Two sets: the moving circle and the moving goals (per-game obstacle data: the one-wavefront EXT kernels) and the moving goals alone (base
kernels, the team of four the library picks at 64 seeds -- the kernel bench.py --config C5 runs).  Wall time of the whole call including the
schedule's upload, median and extremes over the repetitions after one warm-up; the two ways alternate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import algames_jl_amd as alg  # noqa: E402


def run(name, seeds, steps, reps, **kw):
    ids = np.arange(128, 128 + seeds)
    probs = {}
    for way in ("fused", "step-wise"):
        probs[way], S = alg.scenarios.c5_scheduled(ids, steps, **kw)
    x0 = probs["fused"].x0.copy()
    times = {"fused": [], "step-wise": []}
    totals = {}
    for rep in range(reps + 1):
        for way, prob in probs.items():
            b = prob.batch
            b.set_x0(x0); b.set_traj(np.zeros((b.B, b.traj_len))); b.reset_con()
            b.synchronize()
            t0 = time.perf_counter()
            it, cv, _ = alg.mpc_solve(prob, steps, schedule=S, fused=(way == "fused"))      # (mpc_totals inside waits for the device)
            dt = time.perf_counter() - t0
            if rep > 0:
                times[way].append(dt)
            totals[way] = (int(it.sum()), int(cv.sum()))
    lines = ["%s: %d seeds x %d steps, %d wavefronts per game, kernels in use %d" % (name, seeds, steps, probs["fused"].batch.get_waves_per_game(),
                                                                                 probs["fused"].batch.get_scenario_kernels()[1])]
    for way in ("fused", "step-wise"):
        t = times[way]
        lines.append("  %-9s median %8.2f ms  (min %8.2f, max %8.2f over %d runs)  %9.1f solves/s   Newton iterations %d, converged solves %d"
                     % (way, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), len(t), seeds * steps / statistics.median(t), *totals[way]))
    lines.append("  step-wise / fused = %.2f" % (statistics.median(times["step-wise"]) / statistics.median(times["fused"])))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = run("moving circle + moving goals", a.seeds, a.steps, a.reps) + run("moving goals", a.seeds, a.steps, a.reps, circle=False)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
