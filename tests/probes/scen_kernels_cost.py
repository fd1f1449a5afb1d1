"""Cost and gain of per-game scenario data on the base kernels (alg_set_scenario_kernels).

    python tests/probes/scen_kernels_cost.py [--rows 1,2,3,4] [--out FILE]

Timing as bench.py does it: HIP events around the asynchronous solve on the launch stream, WARM warm-up solves per variant, then the variants
alternated ROUNDS times x SOLVES solves each; median over the rounds and every round's figure are printed.
  row 1  C2 shape (3-player DoubleIntegrator, N = 40, 4096 games, control bounds +-8..9), every block equal to the shared values:
         E = 0 shared | E = 2 | E = 1 per game -- the same iterates on every variant
  row 2  the same shape, pair radii in [0.2, 0.3] and control bounds per game: E = 2 | E = 1
  row 3  heterogeneous batch (x0 +- 0.3, radii and bounds per game; the hand-off test's inputs) at 4096 games:
         E = 1 | E = 2 | E = 2 + hand-off K = 16 | K = 24, ms per solve
  row 4  3-player unicycle, N = 30, 64 seeds x 50 MPC steps, per-game radii: E = 1 (one wavefront) | E = 2 (team of four)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import algames_jl_amd as alg  # noqa: E402

K_RAD, K_COST, K_CTL = 0, 1, 2
WARM, ROUNDS, SOLVES = 5, 7, 4
OUT = [sys.stdout]


def say(s):
    for f in OUT:
        print(s, file=f, flush=True)


class Variant:
    def __init__(self, name, batch, launch, iters):
        self.name, self.b, self.launch, self.iters = name, batch, launch, iters
        self.ms, self.it = [], 0


def measure(stream, variants):
    for v in variants:
        v.b.set_stream(stream.cuda_stream)
        for _ in range(WARM):
            v.launch()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(SOLVES):
                v.launch()
            e1.record(stream)
            torch.cuda.synchronize()
            v.ms.append(e0.elapsed_time(e1) / SOLVES)
            v.it = v.iters()
    say("# variant                  median game-iterations/s   game-iterations per solve   median ms per solve   rate of every round")
    for v in variants:
        rates = [v.it / (ms * 1e-3) for ms in v.ms]
        say("%-26s %12.0f %10d %10.3f    %s" % (v.name, np.median(rates), v.it, np.median(v.ms), " ".join("%.0f" % r for r in rates)))
    return {v.name: (float(np.median([v.it / (ms * 1e-3) for ms in v.ms])), [v.it / (ms * 1e-3) for ms in v.ms], float(np.median(v.ms))) for v in variants}


def c2_batch(B, mode, radii=None, umax=None, umin=None, x0=None, same_blocks=False):
    """the C2 problem on a bare handle; mode: None = shared values on the base kernels, "base" / "ext" = per-game blocks on those kernels"""
    model, N, dt, x0_, obj, con, opts = alg.scenarios.c2_double_integrator(np.arange(B))
    x0 = x0_ if x0 is None else x0
    b = alg.Batch(alg.hip_lib(), 0, 3, N, dt, B)
    if mode is not None:
        b.set_scenario_kernels(mode)
    b.set_options(**opts.to_abi())
    b.set_x0(x0); b.set_lqr(obj.Qdiag, obj.Rdiag, obj.xf, obj.uf)
    b.add_collision_cost(obj.collision_radius, obj.collision_μ)
    b.add_collision_avoidance(np.full(3, 0.25) if radii is None else radii[0])
    b.add_control_bound(umax[0], umin[0])
    b.set_waves_per_game(1)
    if mode is not None:
        if same_blocks:
            for k in (K_RAD, K_COST, K_CTL):
                b.set_scenario_data(k, b.get_scenario_data(k))
        else:
            b.set_scenario_data(K_RAD, ((radii[:, :, None] + radii[:, None, :]) * (1 - np.eye(3))).reshape(B, 9))
            b.set_scenario_data(K_CTL, np.concatenate([umax, umin], axis=1))
    return b


def solve_variant(name, b):
    return Variant(name, b, lambda: b.newton_solve_async(init=True, game_id0=0), lambda: int(b.get_stats()["newton_iters"].sum()))


def row1(stream, B=4096):
    rng = np.random.default_rng(3)
    umax = np.tile(8.0 + rng.random(6), (B, 1)); umin = np.tile(-8.0 - rng.random(6), (B, 1))
    say("# row 1: C2 shape, %d games, control bounds +-8..9, every block equal to the shared values (the same iterates on every variant)" % B)
    vs = [solve_variant("E0_shared", c2_batch(B, None, umax=umax, umin=umin)),
          solve_variant("E2_pergame_same", c2_batch(B, "base", umax=umax, umin=umin, same_blocks=True)),
          solve_variant("E1_pergame_same", c2_batch(B, "ext", umax=umax, umin=umin, same_blocks=True))]
    assert [v.b.get_scenario_kernels()[1] for v in vs] == [0, 2, 1]
    r = measure(stream, vs)
    z = [v.b.get_traj() for v in vs]
    say("# E = 2 trajectories bit-equal to E = 0: %s" % np.array_equal(z[0], z[1]))
    e0, e2, e1 = r["E0_shared"], r["E2_pergame_same"], r["E1_pergame_same"]
    say("# E = 2 / E = 0 = %.4f  (target >= 0.97); per round %s" % (e2[0] / e0[0], " ".join("%.4f" % (a / b) for a, b in zip(e2[1], e0[1]))))
    say("# E = 2 / E = 1 = %.4f; per round %s" % (e2[0] / e1[0], " ".join("%.4f" % (a / b) for a, b in zip(e2[1], e1[1]))))


def row2(stream, B=4096):
    rng = np.random.default_rng(12)
    r = 0.1 + 0.05 * rng.random((B, 3))
    umax = 8.0 + rng.random((B, 6)); umin = -8.0 - rng.random((B, 6))
    say("# row 2: C2 shape, %d games, pair radii in [0.2, 0.3] and control bounds per game (other iterates than row 1)" % B)
    vs = [solve_variant("E2_pergame", c2_batch(B, "base", r, umax, umin)), solve_variant("E1_pergame", c2_batch(B, "ext", r, umax, umin))]
    res = measure(stream, vs)
    say("# E = 2 / E = 1 = %.4f" % (res["E2_pergame"][0] / res["E1_pergame"][0]))


def row3(stream, B=4096):
    model, N, dt, x0, obj, con, opts = alg.scenarios.c2_double_integrator(np.arange(B))
    rng = np.random.default_rng(5)
    x0[:, :6] += rng.uniform(-0.3, 0.3, (B, 6))
    r = 0.2 + 0.1 * rng.random((B, 3))
    umax = 8.0 + rng.random((B, 6)); umin = -8.0 - rng.random((B, 6))
    say("# row 3: heterogeneous batch: C2 shape, %d games, x0 +- 0.3, radii r_i in [0.2, 0.3] and control bounds per game" % B)
    vs = []
    for name, mode, K in (("E1", "ext", 0), ("E2", "base", 0), ("E2_handoff_16", "base", 16), ("E2_handoff_24", "base", 24)):
        b = c2_batch(B, mode, r, umax, umin, x0=x0)
        if K:
            b.set_handoff(K)
        vs.append(solve_variant(name, b))
    res = measure(stream, vs)
    for v in vs[2:]:
        say("# %s: %d of %d games parked; ms per solve / E2 = %.4f, / E1 = %.4f" % (v.name, v.b.get_handoff()[1], B, res[v.name][2] / res["E2"][2], res[v.name][2] / res["E1"][2]))


def row4(stream, B=64, steps=50):
    model, N, dt, x0, obj, con, opts = alg.scenarios.c3_unicycle(np.arange(B), N=30, p=3)
    rng = np.random.default_rng(7)
    r = 0.04 + 0.02 * rng.random((B, 3))
    say("# row 4: 3-player unicycle, N = 30, %d seeds x %d MPC steps (alg_mpc_solve), per-game pair radii in [0.08, 0.12]" % (B, steps))
    vs = []
    for name, mode in (("E1_one_wavefront", "ext"), ("E2_team", "base")):
        b = alg.Batch(alg.hip_lib(), 1, 3, N, dt, B)
        b.set_scenario_kernels(mode)
        b.set_options(**opts.to_abi())
        b.set_x0(x0); b.set_lqr(obj.Qdiag, obj.Rdiag, obj.xf, obj.uf)
        b.add_collision_avoidance(r[0]); b.add_control_bound(con.u_max, con.u_min)
        b.set_scenario_data(K_RAD, ((r[:, :, None] + r[:, None, :]) * (1 - np.eye(3))).reshape(B, 9))

        def launch(b=b):
            b.set_x0(x0); b.mpc_totals(reset=True); b.mpc_solve(steps, game_id0=0)
        vs.append(Variant("%s_w%d" % (name, b.get_waves_per_game()), b, launch, lambda b=b: int(b.mpc_totals()[0].sum())))
    res = measure(stream, vs)
    say("# E = 2 (team) / E = 1 = %.4f" % (res[vs[1].name][0] / res[vs[0].name][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,2,3,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT.append(open(a.out, "a"))
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    say("# per-game scenario data on the base kernels: one device (%s), variants alternated %d times x %d solves, %d warm-up solves each, HIP events on the launch stream"
        % (torch.cuda.get_device_name(0), ROUNDS, SOLVES, WARM))
    for row in a.rows.split(","):
        {"1": row1, "2": row2, "3": row3, "4": row4}[row.strip()](stream)


if __name__ == "__main__":
    main()
