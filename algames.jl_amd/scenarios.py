"""Synthetic scenario sets of the BASELINE configurations.

All random numbers come from the same counter-based generator the library uses on the device
(SplitMix64 keyed by (seed, stream, counter)), so inputs depend only on the *global* scenario id:
sharding a batch over ranks does not change them.
"""
import numpy as np

from . import host

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def counter_uniform(seed, game, counter):
    """Bit-identical to alg::counter_uniform (algames_device.hpp) / the oracle's counter_uniform."""
    game = np.asarray(game, dtype=np.uint64)
    counter = np.asarray(counter, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _splitmix64(np.uint64(seed) ^ _splitmix64(game * np.uint64(0xD1B54A32D192ED03) + np.uint64(0x632BE59BD9B4E019)))
        h = _splitmix64(h + counter * np.uint64(0x9E3779B97F4A7C15))
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


SCENARIO_STREAM = 0x5CE7A210   # keeps scenario draws disjoint from the init_traj draws of the same game id


def shard_range(total, rank, world):
    """Contiguous shard [lo, hi) of `total` scenarios for `rank` of `world`."""
    per = (total + world - 1) // world
    lo = min(rank * per, total)
    return lo, min(lo + per, total)


def _uniform(seed, ids, count, lo, hi):
    ids = np.asarray(ids, dtype=np.uint64)
    u = counter_uniform(seed ^ SCENARIO_STREAM, ids[:, None], np.arange(count, dtype=np.uint64)[None, :])
    return lo + (hi - lo) * u


def c2_double_integrator(ids, N=40, seed=100, p=3):
    """C2 / C4: 3-player DoubleIntegrator (d=2), base = examples/ibr_example.jl:10-74 with N 20 -> 40.
    Returns (model, N, dt, x0 (B,n), game_obj, game_con, opts)."""
    ids = np.asarray(ids, dtype=np.int64)
    model = host.DoubleIntegratorGame(p=p, d=2)
    dt = 0.1
    Q = [50.0 * np.ones(4) for _ in range(p)]
    R = [0.01 * np.ones(2) for _ in range(p)]
    xf = [np.zeros(4) for _ in range(p)]
    uf = [np.zeros(2) for _ in range(p)]
    game_obj = host.GameObjective(Q, R, xf, uf, N, model)
    host.add_collision_cost(game_obj, 3.0 * np.ones(p), 2.0 * np.ones(p))          # ibr_example.jl:44-46
    game_con = host.GameConstraintValues(host.ProblemSize(N, model))
    host.add_collision_avoidance(game_con, 0.25)                                      # ibr_example.jl:51-52
    # spiral start, ibr_example.jl:67-70
    th = np.linspace(0.0, 2 * np.pi * (1 - 1 / p), p)
    rad = 0.5
    base = np.zeros(model.n)
    base[0:p] = (rad + th / 10) * np.cos(th)
    base[p:2 * p] = (rad + th / 10) * np.sin(th)
    x0 = np.tile(base, (len(ids), 1))
    x0[:, :2 * p] += _uniform(seed, ids, 2 * p, -0.05, 0.05)
    opts = host.Options(Δ_min=1e-9, inner_print=False, seed=seed)                    # ibr_example.jl:74
    return model, N, dt, x0, game_obj, game_con, opts


def c3_unicycle(ids, N=50, seed=100, p=4, target_offset=0.1):
    """C3 (p=4, N=50) / C5 (p=3, N=30): Unicycle, costs of test/problem/solver_methods.jl:141-144 (Q_i = I, R_i = 0.5 I)
    with uf = 0; collision avoidance radius 0.05 (pair radius 0.1) and control bounds +-1 (:150-155); the effective
    options of that test (outer 7, inner 20, ls 25, reg_0 1e-7) with eps = 1e-3.
    Players start on the unit circle at angles 2 pi i/p + U(-0.1, 0.1) with speed 0.5, heading to their target.
    SURVEY 8(d) puts the target at the antipode, which makes all p paths meet at one point at one time: the
    reference algorithm itself then stalls (the collision-constraint Jacobian vanishes at coincidence; the CPU oracle
    does not converge either).  The target is therefore the antipode rotated by `target_offset` = 0.1 rad -- the
    constraints stay active (multipliers ~0.5) and every scenario converges in 4 outer iterations."""
    ids = np.asarray(ids, dtype=np.int64)
    model = host.UnicycleGame(p=p)
    dt = 0.1
    B = len(ids)
    ang = 2 * np.pi * np.arange(p) / p + _uniform(seed, ids, p, -0.1, 0.1)            # (B,p)
    x0 = np.zeros((B, model.n))
    x0[:, 0:p] = np.cos(ang)
    x0[:, p:2 * p] = np.sin(ang)
    tx, ty = np.cos(ang + np.pi + target_offset), np.sin(ang + np.pi + target_offset)
    head = np.arctan2(ty - x0[:, p:2 * p], tx - x0[:, 0:p])
    x0[:, 2 * p:3 * p] = head
    x0[:, 3 * p:4 * p] = 0.5
    Q = [np.ones(4) for _ in range(p)]
    R = [0.5 * np.ones(2) for _ in range(p)]
    uf = [np.zeros(2) for _ in range(p)]
    game_obj = host.GameObjective(Q, R, [np.zeros(4)] * p, uf, N, model)
    xf = np.zeros((B, p, 4))
    xf[:, :, 0], xf[:, :, 1], xf[:, :, 2] = tx, ty, head                             # stop at the target
    game_obj.xf = xf                                                                # per-game targets
    game_obj.Qdiag = np.broadcast_to(game_obj.Qdiag, (B, p, 4)).copy()
    game_obj.Rdiag = np.broadcast_to(game_obj.Rdiag, (B, p, 2)).copy()
    game_obj.uf = np.broadcast_to(game_obj.uf, (B, p, 2)).copy()
    game_con = host.GameConstraintValues(host.ProblemSize(N, model))
    host.add_collision_avoidance(game_con, 0.05)
    host.add_control_bound(game_con, np.ones(model.m), -np.ones(model.m))
    opts = host.Options(inner_print=False, outer_print=False, outer_iter=7, inner_iter=20, ls_iter=25,
                        reg_0=1e-7, seed=seed)
    return model, N, dt, x0, game_obj, game_con, opts


def quadrotor_crossing(ids, N=20, seed=100, p=2):
    """'Q' (not a BASELINE configuration): p quadrotors (src/dynamics/quadrotor.jl) start at rest on a circle of
    radius 0.6 m at height 0.5 m, +- 5 cm, and fly to the opposite side rotated by 0.3 rad while holding height: hover thrust
    reference uf = m g / (4 kf), planar collision avoidance on px[i] = (x, y) (quadrotor.jl:34) with radius 0.1 m, rotor
    commands bounded to [0, 3]."""
    ids = np.asarray(ids, dtype=np.int64)
    model = host.QuadrotorGame(p=p)
    dt = 0.1
    B = len(ids)
    hover = 0.5 * 9.81 / 4 / 1.245
    ang = 2 * np.pi * np.arange(p) / p + _uniform(seed, ids, p, -0.1, 0.1)
    jit = _uniform(seed + 1, ids, 3 * p, -0.05, 0.05).reshape(B, 3, p)
    x0 = np.zeros((B, model.n))
    x0[:, 0:p] = 0.6 * np.cos(ang) + jit[:, 0]
    x0[:, p:2 * p] = 0.6 * np.sin(ang) + jit[:, 1]
    x0[:, 2 * p:3 * p] = 0.5 + jit[:, 2]
    Q = [np.concatenate([np.ones(3), 0.5 * np.ones(3), 0.2 * np.ones(3), 0.2 * np.ones(3)]) for _ in range(p)]
    R = [0.1 * np.ones(4) for _ in range(p)]
    game_obj = host.GameObjective(Q, R, [np.zeros(12)] * p, [hover * np.ones(4)] * p, N, model)
    xf = np.zeros((B, p, 12))
    xf[:, :, 0], xf[:, :, 1], xf[:, :, 2] = 0.6 * np.cos(ang + np.pi + 0.3), 0.6 * np.sin(ang + np.pi + 0.3), 0.5
    game_obj.xf = xf
    game_obj.Qdiag = np.broadcast_to(game_obj.Qdiag, (B, p, 12)).copy()
    game_obj.Rdiag = np.broadcast_to(game_obj.Rdiag, (B, p, 4)).copy()
    game_obj.uf = np.broadcast_to(game_obj.uf, (B, p, 4)).copy()
    game_con = host.GameConstraintValues(host.ProblemSize(N, model))
    if p > 1:
        host.add_collision_avoidance(game_con, 0.1)
    host.add_control_bound(game_con, 3.0 * np.ones(model.m), np.zeros(model.m))
    # reg_0 = 1e-5: with the default 1e-3 the proximal term reg_0 l^4 of the later inner iterations holds the attitude states back
    # and the optimality test is not met within the default iteration limits (the CPU oracle behaves the same way)
    opts = host.Options(inner_print=False, outer_print=False, seed=seed, reg_0=1e-5)
    return model, N, dt, x0, game_obj, game_con, opts


GOAL_SPEED = 0.04     # of the moving targets of c5_scheduled, per unit time (the vehicles drive at 0.5)


def c5_scheduled(ids, rows, N=30, seed=100, circle=True, goals=True, backend=None, device=0, scenario_kernels="ext"):
    """The scheduled C5 set: the 3-player unicycle problem of C5 with a world that moves over the receding-horizon loop.
    Returns (problem, schedule): schedule = {kind: (rows, B, len)} for mpc_solve(problem, steps, schedule=...), row t = the world at
    MPC step t (time t dt), the last row held.

    circle: one circle per game (every player must stay outside it) crosses the vehicles' paths along a straight line.  It starts
      0.35 beside the point at radius 0.6 of player 0's way to the centre and moves at 0.2 ... 0.3 per unit time across that way, on a
      line turned by up to 0.3 rad, both by the seed: it reaches the way about when the vehicle does.  Radius 0.1.  The problem is built
      with the circle of row 0.
    goals: every target moves along a line of its own -- direction by the seed -- at GOAL_SPEED per unit time, the heading of the target with it.
    The speeds are low against the vehicles' 0.5, so every solve of the loop stays a warm-started one."""
    ids = np.asarray(ids, dtype=np.int64)
    model, N, dt, x0, obj, con, opts = c3_unicycle(ids, N=N, seed=seed, p=3)
    B, p = len(ids), 3
    t = dt * np.arange(rows)[:, None, None]                                             # (rows, 1, 1)
    u = _uniform(seed + 7, ids, 3 + p, 0.0, 1.0)                                         # (B, 3 + p)
    schedule = {}
    if circle:
        a0 = np.arctan2(x0[:, p], x0[:, 0])                                              # player 0 starts at (cos a0, sin a0) and heads for the centre
        side = np.where(u[:, 0] < 0.5, -1.0, 1.0)
        nrm = a0 + side * (0.5 * np.pi + 0.6 * (u[:, 1] - 0.5))                          # from the way to the circle's start
        c0 = 0.6 * np.stack([np.cos(a0), np.sin(a0)], axis=1) + 0.35 * np.stack([np.cos(nrm), np.sin(nrm)], axis=1)
        vel = -(0.2 + 0.1 * u[:, 2])[:, None] * np.stack([np.cos(nrm), np.sin(nrm)], axis=1)
        c = c0[None] + t * vel[None]                                                     # (rows, B, 2)
        schedule["circle"] = np.concatenate([c, np.full((rows, B, 1), 0.1)], axis=2)     # xc yc r
        host.add_circle_constraint(con, c0[:1, 0].copy(), c0[:1, 1].copy(), np.array([0.1]))
    if goals:
        xf = np.broadcast_to(obj.xf, (rows, B, p, 4)).copy()
        dirn = 2 * np.pi * u[:, 3:3 + p]                                                 # (B, p)
        xf[..., 0] += GOAL_SPEED * t * np.cos(dirn)[None]
        xf[..., 1] += GOAL_SPEED * t * np.sin(dirn)[None]
        xf[..., 2] = np.arctan2(xf[..., 1] - x0[None, :, p:2 * p], xf[..., 0] - x0[None, :, 0:p])
        uf = np.broadcast_to(obj.uf, (rows, B, p, 2))
        schedule["lqr_target"] = np.concatenate([xf.reshape(rows, B, -1), uf.reshape(rows, B, -1)], axis=2)
    prob = host.GameProblem(N, dt, x0, model, opts, obj, con, backend=backend, device=device, game_id0=int(ids[0]), scenario_kernels=scenario_kernels)
    return prob, schedule


DISTURBANCE_STREAM = 0x0D157A2B   # keeps the disturbance draws disjoint from the scenario draws of the same id


def c5_disturbed(ids, steps, sigma, N=30, seed=100, backend=None, device=0):
    """The C5 set under plant noise: the 3-player unicycle problem of C5 plus a disturbance for mpc_rollout(problem, steps,
    disturbance=...).  Returns (problem, disturbance (steps, B, n)): entry e of game g at MPC step t is uniform with mean 0 and standard
    deviation sigma (in +-sqrt(3) sigma), drawn from the counter-based generator keyed by (global scenario id, t * n + e) -- a pure
    function of the ids, so the shards of a batch see the numbers of the whole batch."""
    ids = np.asarray(ids, dtype=np.int64)
    prob = make_problem("C5", ids, backend=backend, device=device, N=N, seed=seed)
    n = prob.probsize.n
    u = counter_uniform((seed + 11) ^ DISTURBANCE_STREAM, ids.astype(np.uint64)[None, :, None],
                        (np.arange(steps, dtype=np.uint64)[:, None, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, None, :]))
    return prob, np.ascontiguousarray(float(sigma) * np.sqrt(3.0) * (2.0 * u - 1.0))


def make_problem(cfg, ids, backend=None, device=0, devices=None, **kw):
    """cfg in {'C2','C3','C4','C5'} (BASELINE configurations) or 'Q' (quadrotors) -> GameProblem over the scenarios `ids`
    (global scenario ids).  devices=[...]: a sharding.ShardedGameProblem, the batch split contiguously over those devices."""
    ids = np.asarray(ids, dtype=np.int64)
    if cfg in ("C2", "C4"):                      # C4 = the C2 problem, 65 536 scenarios sharded over 8 GPUs
        model, N, dt, x0, obj, con, opts = c2_double_integrator(ids, **kw)
    elif cfg == "C3":
        model, N, dt, x0, obj, con, opts = c3_unicycle(ids, **{"N": 50, "p": 4, **kw})
    elif cfg == "C5":
        model, N, dt, x0, obj, con, opts = c3_unicycle(ids, **{"N": 30, "p": 3, **kw})
    elif cfg == "Q":
        model, N, dt, x0, obj, con, opts = quadrotor_crossing(ids, **kw)
    else:
        raise ValueError(cfg)
    contiguous = len(ids) > 0 and np.array_equal(ids, ids[0] + np.arange(len(ids)))
    if not contiguous:
        raise ValueError("scenario ids of one problem must be contiguous (the device RNG is keyed by game_id0 + g)")
    if devices is not None:
        from . import sharding
        return sharding.ShardedGameProblem(N, dt, x0, model, opts, obj, con, devices=devices, backend=backend, game_id0=int(ids[0]))
    return host.GameProblem(N, dt, x0, model, opts, obj, con, backend=backend, device=device, game_id0=int(ids[0]))
