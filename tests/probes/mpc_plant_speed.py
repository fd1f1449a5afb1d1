"""The plant of the fused receding-horizon loop (alg_mpc_set_plant): what holding `hold` knots of a plan buys and costs.
The C5 shape under noise: scenarios.c5_disturbed, 64 seeds x 200 plant knots, one disturbance row per knot.

    python tests/probes/mpc_plant_speed.py [--seeds 64] [--knots 200] [--sigma 0.002] [--reps 3] [--out profiles/mpc_plant_speed.txt]

For hold = 1, 2, 4 (200, 100, 50 solves; one RK2 sub-step per knot): wall time of the fused launch with the full log (host.mpc_rollout,
fused=True) and of the step-wise definition beside it (fused=False), Newton iterations, converged solves, and the closed-loop cost from the
log: the distance of every vehicle to its target after the last knot and the smallest distance of two vehicles of one game over the loop.
Then the same loop with the plant (1, 4, rk4) against (1, 1, rk2) -- the second is the loop without a plant, the first pays the plant phase
and four RK4 sub-steps per knot.  Median and extremes over the repetitions after one warm-up; the ways alternate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import algames_jl_amd as alg  # noqa: E402

PLANTS = [(1, 1, "rk2"), (2, 1, "rk2"), (4, 1, "rk2"), (1, 4, "rk4")]


def closed_loop_cost(prob, states):
    """(mean, largest final distance to the targets; smallest pair distance over all knots and games)"""
    p = prob.batch.p
    xf = np.broadcast_to(np.asarray(prob.game_obj.xf, dtype=np.float64), (prob.batch.B, p, 4))
    px, py = states[..., 0:p], states[..., p:2 * p]
    dist = np.hypot(px[-1] - xf[:, :, 0], py[-1] - xf[:, :, 1])
    pair = min(np.hypot(px[..., i] - px[..., j], py[..., i] - py[..., j]).min() for i in range(p) for j in range(i + 1, p))
    return dist.mean(), dist.max(), pair


def run(seeds, knots, sigma, reps):
    ids = np.arange(128, 128 + seeds)
    prob, W = alg.scenarios.c5_disturbed(ids, knots, sigma)
    b = prob.batch
    x0 = prob.x0.copy()
    ways = [(c, f) for c in PLANTS for f in (True, False)]
    times = {w: [] for w in ways}
    last = {}
    for rep in range(reps + 1):
        for c, f in ways:
            plant = alg.Plant(*c)
            assert knots % plant.hold == 0
            b.set_traj(np.zeros((b.B, b.traj_len))); b.reset_con(); b.set_x0(x0)       # (x0 last: it is x_1 of the trajectory too)
            b.synchronize()
            t0 = time.perf_counter()
            out = alg.mpc_rollout(prob, knots // plant.hold, disturbance=W, fused=f, plant=plant)
            dt = time.perf_counter() - t0
            if rep > 0:
                times[(c, f)].append(dt)
            last[(c, f)] = out
    lines = ["C5 under noise (sigma %g): %d seeds x %d plant knots, %d wavefronts per game, kernels in use %d" % (sigma, seeds, knots, b.get_waves_per_game(),
                                                                                                             b.get_scenario_kernels()[1])]
    med = {w: statistics.median(t) for w, t in times.items()}
    for c in PLANTS:
        o, s = last[(c, True)], last[(c, False)]
        tf, ts = times[(c, True)], times[(c, False)]
        mean_d, max_d, pair = closed_loop_cost(prob, o.states)
        lines.append("  plant (hold %d, substeps %d, %s): %d solves per game" % (c + (knots // c[0],)))
        lines.append("    fused     median %8.2f ms  (min %8.2f, max %8.2f over %d runs)  Newton iterations %d (%.2f per solve, most in one solve %d, in one game %d), "
                     "converged solves %d of %d"
                     % (1e3 * med[(c, True)], 1e3 * min(tf), 1e3 * max(tf), len(tf), o.newton_iters.sum(), o.newton_iters.sum() / o.stats.size,
                        o.stats["newton_iters"].max(), o.newton_iters.max(), o.converged.sum(), o.stats.size))
        lines.append("    step-wise median %8.2f ms  (min %8.2f, max %8.2f over %d runs)  step-wise / fused = %.2f;  bit-equal states %s, controls %s, iterations %s"
                     % (1e3 * med[(c, False)], 1e3 * min(ts), 1e3 * max(ts), len(ts), med[(c, False)] / med[(c, True)],
                        np.array_equal(o.states, s.states), np.array_equal(o.controls, s.controls), np.array_equal(o.newton_iters, s.newton_iters)))
        lines.append("    closed loop: final distance to the targets mean %.4f, largest %.4f;  smallest pair distance over the loop %.4f" % (mean_d, max_d, pair))
    base = med[(PLANTS[0], True)]
    lines.append("  fused time against hold 1: hold 2 x %.3f, hold 4 x %.3f (solves: x 0.5, x 0.25);  Newton iterations: x %.3f, x %.3f"
                 % (med[(PLANTS[1], True)] / base, med[(PLANTS[2], True)] / base,
                    last[(PLANTS[1], True)].newton_iters.sum() / last[(PLANTS[0], True)].newton_iters.sum(),
                    last[(PLANTS[2], True)].newton_iters.sum() / last[(PLANTS[0], True)].newton_iters.sum()))
    lines.append("  the plant phase alone: (1, 4, rk4) / (1, 1, rk2) = %.4f fused -- the finer plant is another closed loop: Newton iterations %d against %d, "
                 "in the slowest game, which the launch waits for, %d against %d"
                 % (med[(PLANTS[3], True)] / base, last[(PLANTS[3], True)].newton_iters.sum(), last[(PLANTS[0], True)].newton_iters.sum(),
                    last[(PLANTS[3], True)].newton_iters.max(), last[(PLANTS[0], True)].newton_iters.max()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--knots", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = run(a.seeds, a.knots, a.sigma, a.reps)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
