"""Closed-loop log and plant disturbance of the fused receding-horizon loop: the fused launch with the full log (alg_mpc_solve_log with a
disturbance: host.mpc_rollout(fused=True)) against the step-wise definition of the same library (mpc_rollout(fused=False): per MPC step one
alg_newton_solve_async launch, alg_get_stats, alg_get_traj, one alg_mpc_advance launch, x_1 read back, alg_set_x0(x_1 + w_t)) -- all a caller
could do before the log existed -- and against the disturbed loop without a log (alg_mpc_solve on a handle that carries the disturbance).
The C5 shape under noise: scenarios.c5_disturbed, 64 seeds x 200 MPC steps, one row per step.

    python tests/probes/mpc_log_speed.py [--seeds 64] [--steps 200] [--sigma 0.002] [--reps 5] [--out profiles/mpc_log_speed.txt]

Wall time of the whole call including the upload of the disturbance and the copies back, median and extremes over the repetitions after
one warm-up; the three ways alternate.  The two logged ways must run the same number of Newton iterations (the probe says so)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import algames_jl_amd as alg  # noqa: E402

WAYS = ("fused + log", "fused, no log", "step-wise")


def run(seeds, steps, sigma, reps):
    ids = np.arange(128, 128 + seeds)
    probs = {}
    for way in WAYS:
        probs[way], W = alg.scenarios.c5_disturbed(ids, steps, sigma)
    x0 = probs[WAYS[0]].x0.copy()
    times = {way: [] for way in WAYS}
    totals, last = {}, {}
    for rep in range(reps + 1):
        for way, prob in probs.items():
            b = prob.batch
            b.set_traj(np.zeros((b.B, b.traj_len))); b.reset_con(); b.set_x0(x0)       # (x0 last: it is x_1 of the trajectory too)
            b.synchronize()
            t0 = time.perf_counter()
            if way == "fused, no log":
                b.mpc_set_schedule("disturbance", W)
                it, cv, _ = alg.mpc_solve(prob, steps)                  # (mpc_totals inside waits for the device)
                b.mpc_set_schedule("disturbance", None)
            else:
                out = alg.mpc_rollout(prob, steps, disturbance=W, fused=(way == "fused + log"))
                it, cv, last[way] = out.newton_iters, out.converged, out
            dt = time.perf_counter() - t0
            if rep > 0:
                times[way].append(dt)
            totals[way] = (int(it.sum()), int(cv.sum()))
    b = probs[WAYS[0]].batch
    lines = ["C5 under noise (sigma %g): %d seeds x %d steps, %d wavefronts per game, kernels in use %d" % (sigma, seeds, steps, b.get_waves_per_game(),
                                                                                                       b.get_scenario_kernels()[1])]
    for way in WAYS:
        t = times[way]
        lines.append("  %-13s median %8.2f ms  (min %8.2f, max %8.2f over %d runs)  %9.1f solves/s   Newton iterations %d, converged solves %d"
                     % (way, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), len(t), seeds * steps / statistics.median(t), *totals[way]))
    med = {way: statistics.median(times[way]) for way in WAYS}
    f, s = last["fused + log"], last["step-wise"]
    lines.append("  step-wise / fused + log = %.2f;  fused + log / fused, no log = %.3f" % (med["step-wise"] / med["fused + log"], med["fused + log"] / med["fused, no log"]))
    lines.append("  same Newton iterations fused + log and step-wise: %s (per game: %d of %d);  states bit-equal: %s, max diff %.3e"
                 % (totals["fused + log"][0] == totals["step-wise"][0], int((f.newton_iters == s.newton_iters).sum()), seeds,
                    np.array_equal(f.states, s.states), np.abs(f.states - s.states).max()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = run(a.seeds, a.steps, a.sigma, a.reps)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
