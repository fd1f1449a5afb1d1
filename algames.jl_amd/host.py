"""Host-side mirror of the Algames.jl API surface for the Newton / augmented-Lagrangian hot path.

Same names, argument meaning and error behaviour as the reference (Julia `f!` -> Python `f`), but a
`GameProblem` owns a *batch* of B games (x0 of shape (B, n)) that are solved together on one MI355X
through the C ABI of include/algames_hip.h.  Index sets / stamps are kept 1-based like the reference
so that its tests' literal values can be quoted unchanged.

Reference: src/Algames.jl:19-165 (exports), src/problem/problem.jl, src/problem/solver_methods.jl,
src/struct/*.jl, src/dynamics/{double_integrator,unicycle}.jl, src/objective/objective.jl,
src/constraints/{game_constraints,constraints_methods}.jl.
"""
import collections
import contextlib
import dataclasses
import os

import numpy as np

from . import _abi
from ._abi import (ALG_MODEL_BICYCLE, ALG_MODEL_DOUBLE_INTEGRATOR, ALG_MODEL_QUADROTOR, ALG_MODEL_UNICYCLE, ALG_TRAJ_PD, ALG_TRAJ_TRIAL,
                   ALG_TRAJ_DELTA, ALG_SCEN_COLLISION_COST, ALG_SCHED_LQR_TARGET, ALG_SCHED_DISTURBANCE, ALG_CON_KINDS, AlgamesError, Batch, CLib, Plant)

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("ALGAMES_HIP_LIB", os.path.join(_HERE, "lib", "libalgames_hip.so"))
_hip = None


def hip_lib():
    """The product backend.  Fails loudly when the HIP extension is missing -- there is no CPU fallback."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise AlgamesError(
                f"{HIP_LIB_PATH} is not built. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
        _hip = CLib(HIP_LIB_PATH, "alg_")
    return _hip


# --------------------------------------------------------------------------------------------------
# Models (src/dynamics/double_integrator.jl:2-25, src/dynamics/unicycle.jl:2-25)
# --------------------------------------------------------------------------------------------------
class AbstractGameModel:
    pass


class DoubleIntegratorGame(AbstractGameModel):
    model_id = ALG_MODEL_DOUBLE_INTEGRATOR

    def __init__(self, p=2, d=2):
        self.p, self.d = p, d
        self.n, self.m = 2 * d * p, d * p
        self.pu = [[i + (j - 1) * p for j in range(1, d + 1)] for i in range(1, p + 1)]
        self.px = [[i + (j - 1) * p for j in range(1, 3)] for i in range(1, p + 1)]
        self.pz = [[i + (j - 1) * p for j in range(1, 2 * d + 1)] for i in range(1, p + 1)]
        self.ni = [2 * d] * p
        self.mi = [d] * p


class UnicycleGame(AbstractGameModel):
    model_id = ALG_MODEL_UNICYCLE

    def __init__(self, p=2):
        self.p, self.d = p, 2
        self.n, self.m = 4 * p, 2 * p
        self.pu = [[i + (j - 1) * p for j in range(1, 3)] for i in range(1, p + 1)]
        self.px = [[i + (j - 1) * p for j in range(1, 3)] for i in range(1, p + 1)]
        self.pz = [[i + (j - 1) * p for j in range(1, 5)] for i in range(1, p + 1)]
        self.ni = [4] * p
        self.mi = [2] * p


class BicycleGame(AbstractGameModel):
    """BicycleGame(p; lf, lr), src/dynamics/bicycle.jl:2-27: X = [x, y, v, psi], U = [a, delta]."""
    model_id = ALG_MODEL_BICYCLE

    def __init__(self, p=2, lf=0.05, lr=0.05):
        self.p, self.d = p, 2
        self.lf, self.lr = float(lf), float(lr)
        self.n, self.m = 4 * p, 2 * p
        self.pu = [[i + (j - 1) * p for j in range(1, 3)] for i in range(1, p + 1)]
        self.px = [[i + (j - 1) * p for j in range(1, 3)] for i in range(1, p + 1)]
        self.pz = [[i + (j - 1) * p for j in range(1, 5)] for i in range(1, p + 1)]
        self.ni = [4] * p
        self.mi = [2] * p


class QuadrotorGame(AbstractGameModel):
    """QuadrotorGame(; p, mass), src/dynamics/quadrotor.jl:3-46: per player 12 states [x, y, z | MRP q1 q2 q3 | vx vy vz | wx wy wz]
    and 4 rotor commands; the constructor's constants (J, gravity, motor_dist, kf, km) are fixed in the reference."""
    model_id = ALG_MODEL_QUADROTOR

    def __init__(self, p=2, mass=0.5):
        assert p <= 4                      # quadrotor.jl:22
        if not mass > 0:
            raise AlgamesError("QuadrotorGame: mass must be positive")
        self.p, self.d, self.mass = p, 3, float(mass)
        self.n, self.m = 12 * p, 4 * p
        self.pu = [[i + (j - 1) * p for j in range(1, 5)] for i in range(1, p + 1)]
        self.px = [[i + (j - 1) * p for j in range(1, 3)] for i in range(1, p + 1)]
        self.pz = [[i + (j - 1) * p for j in range(1, 13)] for i in range(1, p + 1)]
        self.ni = [12] * p
        self.mi = [4] * p


def dim(model):
    if isinstance(model, QuadrotorGame):
        return 3                           # quadrotor.jl:208
    return model.mi[0] if isinstance(model, DoubleIntegratorGame) else 2


# --------------------------------------------------------------------------------------------------
# ProblemSize (src/struct/problem_size.jl:5-35) and index maps (src/core/newton_core.jl:40-89)
# --------------------------------------------------------------------------------------------------
class ProblemSize:
    def __init__(self, N, model):
        self.N, self.n, self.m, self.p = N, model.n, model.m, model.p
        self.ni, self.mi = list(model.ni), list(model.mi)
        self.pu, self.px, self.pz = model.pu, model.px, model.pz
        self.S = self.n * self.p * (N - 1) + self.m * (N - 1) + self.n * (N - 1)

    def __eq__(self, o):
        return all(getattr(self, f) == getattr(o, f) for f in ("N", "n", "m", "p", "ni", "mi", "pu", "px", "pz", "S"))


def stampify(*a):
    """Stamps are plain tuples: VStamp (prob,i0,n1,i1,v1), HStamp (n2,i2,v2), Stamp = V + H."""
    return tuple(a)


def valid(stamp, N, p):
    """Stamp validity rules, src/core/stamp.jl:167-229."""
    def v1(prob, i0, n1, i1, k):
        if prob == "opt" and 1 <= i0 <= p:
            if n1 == "u" and i1 == i0 and 1 <= k <= N - 1:
                return True
            if n1 == "x" and i1 == 1 and 2 <= k <= N:
                return True
        if prob == "dyn" and i0 == 1:
            if n1 == "x" and i1 == 1 and 1 <= k <= N - 1:
                return True
        return False

    def v2(n2, i2, k, prob=None, i0=None):
        if n2 == "u" and 1 <= i2 <= p and 1 <= k <= N - 1:
            return True
        if n2 == "λ" and 1 <= k <= N - 1 and ((prob is None and 1 <= i2 <= p) or (prob == "opt" and i2 == i0)):
            return True
        if n2 == "x" and i2 == 1 and 2 <= k <= N:
            return True
        return False

    if len(stamp) == 5:
        return v1(*stamp)
    if len(stamp) == 3:
        return v2(*stamp)
    prob, i0 = stamp[0], stamp[1]
    if prob == "opt" and not (1 <= i0 <= p):
        return False
    if prob == "dyn" and i0 != 1:
        return False
    if prob not in ("opt", "dyn"):
        return False
    return v1(*stamp[:5]) and v2(*stamp[5:], prob=prob, i0=i0)


def vertical_indices(probsize):
    """Row ("vertical") 1-based index ranges of `core.res`, src/core/newton_core.jl:40-63."""
    N, n, p, mi = probsize.N, probsize.n, probsize.p, probsize.mi
    out, off = {}, 0
    for i in range(1, p + 1):
        for k in range(1, N):
            out[stampify("opt", i, "x", 1, k + 1)] = list(range(off + 1, off + n + 1)); off += n
            out[stampify("opt", i, "u", i, k)] = list(range(off + 1, off + mi[i - 1] + 1)); off += mi[i - 1]
    for k in range(1, N):
        out[stampify("dyn", 1, "x", 1, k)] = list(range(off + 1, off + n + 1)); off += n
    return out


def horizontal_indices(probsize):
    """Column ("horizontal") 1-based index ranges of `Δtraj`, src/core/newton_core.jl:65-89."""
    N, n, p, mi = probsize.N, probsize.n, probsize.p, probsize.mi
    out, off = {}, 0
    for k in range(1, N):
        out[stampify("x", 1, k + 1)] = list(range(off + 1, off + n + 1)); off += n
        for i in range(1, p + 1):
            out[stampify("u", i, k)] = list(range(off + 1, off + mi[i - 1] + 1)); off += mi[i - 1]
        for i in range(1, p + 1):
            out[stampify("λ", i, k)] = list(range(off + 1, off + n + 1)); off += n
    return out


# --------------------------------------------------------------------------------------------------
# Options / Regularizer (src/struct/options.jl:5-116, src/struct/regularizer.jl:5-35)
# --------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Regularizer:
    x: float = 1e-3
    u: float = 1e-3
    λ: float = 1e-3


def _ones10():
    return [1.0] * 10


@dataclasses.dataclass
class Options:
    θ: float = 1e-2
    f_init: object = "rand"          # "rand": counter-based generator on the device (alg_init_traj); a callable f(size): init_traj_host
    amplitude_init: float = 1e-8
    shift: int = 2 ** 10
    regularize: bool = True
    reg: Regularizer = dataclasses.field(default_factory=Regularizer)
    reg_0: float = 1e-3
    α_0: float = 1.0
    α_increase: float = 1.2
    α_decrease: float = 0.5
    β: float = 0.01
    ls_iter: int = 25
    Δ_min: float = 1e-9
    ρ_0: float = 1.0
    ρ_trial: float = 1.0
    ρ_increase: float = 10.0
    ρ_max: float = 1e7
    λ_max: float = 1e7
    α_dual: float = 1.0
    αx_dual: list = dataclasses.field(default_factory=_ones10)
    active_set_tolerance: float = 1e-4
    ϵ_dyn: float = 1e-3
    ϵ_sta: float = 1e-3
    ϵ_con: float = 1e-3
    ϵ_opt: float = 1e-3
    outer_iter: int = 7
    inner_iter: int = 20
    γ: float = 1.0
    mpc_horizon: int = 20
    upsampling: int = 2
    inner_print: bool = True
    outer_print: bool = True
    seed: int = 100
    dual_reset: bool = True

    def to_abi(self):
        return dict(amplitude_init=self.amplitude_init, shift=int(min(self.shift, 2 ** 30)),
                    regularize=int(self.regularize), reg_0=self.reg_0, alpha_decrease=self.α_decrease,
                    beta=self.β, ls_iter=self.ls_iter, dual_reset=int(self.dual_reset),
                    delta_min=self.Δ_min, rho_0=self.ρ_0, rho_increase=self.ρ_increase,
                    rho_max=self.ρ_max, lambda_max=self.λ_max, alpha_dual=self.α_dual,
                    alphax_dual=list(self.αx_dual)[:10], eps_dyn=self.ϵ_dyn, eps_sta=self.ϵ_sta,
                    eps_con=self.ϵ_con, eps_opt=self.ϵ_opt, outer_iter=self.outer_iter,
                    inner_iter=self.inner_iter, seed=self.seed)


# --------------------------------------------------------------------------------------------------
# GameObjective (src/objective/objective.jl:6-100)
# --------------------------------------------------------------------------------------------------
def _diag(M):
    M = np.asarray(M, dtype=np.float64)
    return np.diag(M).copy() if M.ndim == 2 else M.copy()


def expand_vector(v, inds, n):
    V = np.zeros(n)
    V[np.asarray(inds) - 1] = v
    return V


class GameObjective:
    def __init__(self, Q, R, xf, uf, N, model):
        p = model.p
        assert len(Q) == len(R) == len(xf) == len(uf) == p
        self.probsize = ProblemSize(N, model)
        self.Qdiag = np.stack([_diag(Q[i]) for i in range(p)])          # (p, ni)
        self.Rdiag = np.stack([_diag(R[i]) for i in range(p)])          # (p, mi)
        self.xf = np.stack([np.asarray(xf[i], dtype=np.float64) for i in range(p)])
        self.uf = np.stack([np.asarray(uf[i], dtype=np.float64) for i in range(p)])
        self.collision_radius = None
        self.collision_μ = None


def add_collision_cost(game_obj, radius, μ):
    """add_collision_cost!(game_obj, radius, μ), objective.jl:84-100 (one set per objective).  `radius` and `μ` are (p,) or, for
    a batch whose games differ in them, (B, p) like the per-game LQR data of GameObjective."""
    p = game_obj.probsize.p
    radius, μ = np.asarray(radius, dtype=np.float64), np.asarray(μ, dtype=np.float64)
    if radius.shape != μ.shape or radius.ndim not in (1, 2) or radius.shape[-1] != p:
        raise ValueError(f"add_collision_cost: radius and μ must both be (p,) or (B, p) with p = {p}")
    if game_obj.collision_radius is not None:
        raise AlgamesError("only one collision-cost set per GameObjective is supported")
    game_obj.collision_radius = radius
    game_obj.collision_μ = μ


# --------------------------------------------------------------------------------------------------
# GameConstraintValues (src/constraints/game_constraints.jl, constraints_methods.jl)
# --------------------------------------------------------------------------------------------------
class GameConstraintValues:
    def __init__(self, probsize):
        self.probsize = probsize
        self.α_dual = 1.0
        self.αx_dual = [1.0] * probsize.p
        self.active_set_tolerance = 0.0  # game_constraints.jl:23; set_constraint_params! copies opts.active_set_tolerance (:37)
        self.collision_radius = None     # per player, pair radius = r_i + r_j
        self.collision_pairs = {}        # (i, j) 1-based ordered pair -> radius of its own CollisionConstraint (the per-pair adders)
        self.u_max = None
        self.u_min = None
        self.state_bounds = {}           # player (1-based) -> merged (x_max, x_min) on the joint state
        self.state_conval = [[] for _ in range(probsize.p)]   # per player: the state-bound sets in the order they were added
        self.walls = None
        self.circles = None
        self.player_walls = {}           # player (1-based) -> list of Wall (add_wall_constraint!(game_con, i, walls))
        self.player_circles = {}         # player (1-based) -> (xc, yc, radius) (add_circle_constraint!(game_con, i, ...))
        self.spherical = False           # collision_radius applies to the 3-D distance (add_spherical_collision_avoidance!)
        self.walls3d = None
        self.cylinders = None
        self.player_walls3d = {}         # player (1-based) -> list of Wall3D (add_wall_constraint!(game_con, i, walls::Vector{Wall3D}))
        self.player_cylinders = {}       # player (1-based) -> list of CylinderWall


def add_collision_avoidance(game_con, *args):
    """add_collision_avoidance!(game_con, radius) (constraints_methods.jl:21-39: every ordered pair, r_i + r_j) or
    add_collision_avoidance!(game_con, i, j, radius) (:5-19: ONE CollisionConstraint of player i against player j, 1-based, with
    its own radius)."""
    p = game_con.probsize.p
    if len(args) == 3:
        i, j, radius = int(args[0]), int(args[1]), float(args[2])
        if not (1 <= i <= p and 1 <= j <= p and i != j):
            raise AlgamesError("add_collision_avoidance!(game_con, i, j, radius): players i != j in 1..p")
        if game_con.collision_radius is not None or (i, j) in game_con.collision_pairs:
            raise AlgamesError("one collision-avoidance constraint per ordered pair is supported")
        game_con.collision_pairs[(i, j)] = radius
        return
    (radius,) = args
    r = np.asarray(radius, dtype=np.float64)
    if r.ndim == 0:
        r = r * np.ones(p)
    assert p == len(r)
    if game_con.collision_radius is not None or game_con.collision_pairs:
        raise AlgamesError("only one collision-avoidance set per GameConstraintValues is supported")
    game_con.collision_radius = r


def add_spherical_collision_avoidance(game_con, *args):
    """add_spherical_collision_avoidance!(game_con, radius) / (game_con, i, j, radius), constraints_methods.jl:45-81:
    CollisionConstraint on pz[i][1:3] (the x, y, z positions of a DoubleIntegratorGame with d = 3 or a Quadrotor; other models
    are rejected when the problem is built)."""
    if (game_con.collision_radius is not None or game_con.collision_pairs) and not game_con.spherical:
        raise AlgamesError("planar and spherical collision avoidance cannot be mixed")
    add_collision_avoidance(game_con, *args)
    game_con.spherical = True


def add_control_bound(game_con, u_max, u_min):
    """add_control_bound!(game_con, u_max, u_min), constraints_methods.jl:104-115."""
    u_max = np.asarray(u_max, dtype=np.float64); u_min = np.asarray(u_min, dtype=np.float64)
    if not np.all(u_max >= u_min):
        raise ValueError("Upper bounds must be greater than or equal to lower bounds")   # control_bound_constraint.jl:69-75
    if game_con.u_max is not None:
        raise AlgamesError("only one control-bound set per GameConstraintValues is supported")
    game_con.u_max, game_con.u_min = u_max, u_min


def add_state_bound(game_con, i, x_max, x_min):
    """add_state_bound!(game_con, i, x_max, x_min), constraints_methods.jl:87-98 (player i is 1-based; bounds on the
    joint state, +-inf allowed).  The reference appends one StateBoundConstraint per call; the rows of several calls for
    the same player are independent scalar constraints, so they are kept as one merged (x_max, x_min) pair -- which
    requires that no state entry is bounded on the same side by two calls."""
    n, p = game_con.probsize.n, game_con.probsize.p
    x_max = np.array(x_max, dtype=np.float64); x_min = np.array(x_min, dtype=np.float64)
    if x_max.shape != (n,) or x_min.shape != (n,):
        raise ValueError("state bounds must have length n")
    if not (1 <= i <= p):
        raise ValueError("player index out of range")
    if not np.all(x_max >= x_min):
        raise ValueError("Upper bounds must be greater than or equal to lower bounds")   # checkBounds
    game_con.state_conval[i - 1].append((x_max.copy(), x_min.copy()))
    if i in game_con.state_bounds:
        mx, mn = game_con.state_bounds[i]
        if np.any(np.isfinite(mx) & np.isfinite(x_max)) or np.any(np.isfinite(mn) & np.isfinite(x_min)):
            raise AlgamesError("a state entry of one player can carry only one upper and one lower bound")
        x_max, x_min = np.minimum(mx, x_max), np.maximum(mn, x_min)
    game_con.state_bounds[i] = (x_max, x_min)


def velocity_index(model, i):
    """velocity_index(model, i), velocity_constraint.jl:30-43 (1-based)."""
    assert 1 <= i <= model.p
    if isinstance(model, UnicycleGame):
        return model.pz[i - 1][3]
    if isinstance(model, BicycleGame):
        return model.pz[i - 1][2]
    raise AlgamesError("Velocity Index is not implemented for DoubleIntegratorGame.")


def add_velocity_bound(model, game_con, v_max, v_min):
    """add_velocity_bound!(model, game_con, v_max, v_min), velocity_constraint.jl:1-28: the bound on player i's speed is a
    state bound added to every player's constraint list."""
    n, p = model.n, model.p
    v_max, v_min = np.asarray(v_max, dtype=np.float64), np.asarray(v_min, dtype=np.float64)
    assert len(v_max) == len(v_min) == p
    for i in range(1, p + 1):
        if v_max[i - 1] != np.inf or v_min[i - 1] != -np.inf:
            x_max = np.full(n, np.inf); x_min = np.full(n, -np.inf)
            x_max[velocity_index(model, i) - 1] = v_max[i - 1]
            x_min[velocity_index(model, i) - 1] = v_min[i - 1]
            for j in range(1, p + 1):
                add_state_bound(game_con, j, x_max, x_min)


class Wall:
    """Wall(p1, p2, v), constraints_methods.jl:155-159: segment p1-p2, v orthogonal to it pointing into the forbidden half space."""

    def __init__(self, p1, p2, v):
        self.p1, self.p2, self.v = (np.asarray(a, dtype=np.float64) for a in (p1, p2, v))


class Wall3D:
    """Wall3D(p1, p2, p3, v), constraints_methods.jl:201-206: parallelogram corners p1, p2, p3 and the normal v of its plane
    pointing into the forbidden half space."""

    def __init__(self, p1, p2, p3, v):
        self.p1, self.p2, self.p3, self.v = (np.asarray(a, dtype=np.float64) for a in (p1, p2, p3, v))


class CylinderWall:
    """CylinderWall(p, v, l, r), constraints_methods.jl:249-254: axis-aligned cylinder with origin p, axis v in (:x, :y, :z)
    (also accepted: "x"/"y"/"z" or 0/1/2), length l, radius r."""

    def __init__(self, p, v, l, r):
        self.p = np.asarray(p, dtype=np.float64)
        self.v = {"x": 0, "y": 1, "z": 2, ":x": 0, ":y": 1, ":z": 2, 0: 0, 1: 1, 2: 2}[v]
        self.l, self.r = float(l), float(r)


def add_wall_constraint(game_con, *args):
    """add_wall_constraint!(game_con, walls) (constraints_methods.jl:189-195, every player) or add_wall_constraint!(game_con, i, walls)
    (:161-187, player i only, 1-based); dispatches on the wall type like the reference's methods for Vector{Wall} (:161),
    Vector{Wall3D} (:208) and Vector{CylinderWall} (:256)."""
    if len(args) == 2:
        i, walls = int(args[0]), list(args[1])
        if not 1 <= i <= game_con.probsize.p:
            raise ValueError("add_wall_constraint: player index out of range")
        kinds = {type(w) for w in walls}
        if len(kinds) != 1 or not kinds <= {Wall, Wall3D, CylinderWall}:
            raise TypeError("add_wall_constraint(game_con, i, walls): walls must all be Wall, all Wall3D or all CylinderWall")
        kind = kinds.pop()                         # the reference's three methods: Vector{Wall} (:161), Vector{Wall3D} (:208), Vector{CylinderWall} (:256)
        shared, own = {Wall: ("walls", "player_walls"), Wall3D: ("walls3d", "player_walls3d"), CylinderWall: ("cylinders", "player_cylinders")}[kind]
        if getattr(game_con, shared) is not None:
            raise AlgamesError("per-player walls cannot be combined with an all-player wall set")
        getattr(game_con, own).setdefault(i, []).extend(walls)
        return
    (walls,) = args
    walls = list(walls)
    kinds = {type(w) for w in walls}
    if len(kinds) != 1:
        raise TypeError("add_wall_constraint: walls must all be Wall, all Wall3D or all CylinderWall")
    slot = {Wall: "walls", Wall3D: "walls3d", CylinderWall: "cylinders"}[kinds.pop()]
    if getattr(game_con, slot) is not None or getattr(game_con, {"walls": "player_walls", "walls3d": "player_walls3d", "cylinders": "player_cylinders"}[slot]):
        raise AlgamesError("only one wall set of each kind per GameConstraintValues is supported")
    setattr(game_con, slot, walls)


def add_circle_constraint(game_con, *args):
    """add_circle_constraint!(game_con, xc, yc, radius) (constraints_methods.jl:141-148, every player) or
    add_circle_constraint!(game_con, i, xc, yc, radius) (:121-139, player i only, 1-based)."""
    player = None
    if len(args) == 4:
        player, args = int(args[0]), args[1:]
        if not 1 <= player <= game_con.probsize.p:
            raise ValueError("add_circle_constraint: player index out of range")
    xc, yc, radius = (np.asarray(a, dtype=np.float64) for a in args)
    if not (xc.shape == yc.shape == radius.shape and xc.ndim == 1):
        raise ValueError("xc, yc, radius must be vectors of equal length")
    if player is not None:
        if game_con.circles is not None:
            raise AlgamesError("per-player circles cannot be combined with an all-player circle set")
        old = game_con.player_circles.get(player)
        game_con.player_circles[player] = (xc, yc, radius) if old is None else tuple(np.concatenate([o, a]) for o, a in zip(old, (xc, yc, radius)))
        return
    if game_con.circles is not None or game_con.player_circles:
        raise AlgamesError("only one circle set per GameConstraintValues is supported")
    game_con.circles = (xc, yc, radius)


# --------------------------------------------------------------------------------------------------
# PrimalDualTraj / Statistics views
# --------------------------------------------------------------------------------------------------
class PrimalDualTraj:
    """Batched view of a primal-dual trajectory (src/struct/primal_dual_traj.jl:5-23).
    states (B,N,n), controls (B,N-1,m) in joint order, duals (B,p,N-1,n)."""

    def __init__(self, states, controls, duals):
        self.states, self.controls, self.duals = states, controls, duals


class Statistics:
    """Per-game `Statistics` history (src/struct/statistics.jl:5-15) as numpy record arrays; the reference's field names
    (`outer_iter`, `res`, `Δ_traj`, `dyn_vio`, `con_vio`, `sta_vio`, `opt_vio`) are views of game 0's history, the `*_vio`
    entries being the `.max` of the reference's violation objects.  `t_elap[r]` is the duration (seconds) of the inner iteration
    that preceded record r, measured on the device with the 100 MHz real-time counter (0 for the first record of a solve).
    `vio(game)` are the `.vio` vectors of the same records when the solve ran with history profiles on (`history_profiles=`)."""

    def __init__(self, summary, history_fn, vio_fn=None):
        self.summary = summary
        self._history_fn = history_fn
        self._vio_fn = vio_fn

    def history(self, game=0):
        return self._history_fn(game)

    def vio(self, game=0):
        """dict(dyn, con, sta, opt) of shape (records, N-1 | N): the per-knot profiles of every stored record of `game`, row r next to
        record r of history(game); None when the solve ran with history profiles off."""
        return None if self._vio_fn is None else self._vio_fn(game)

    @property
    def iter(self):
        return self.summary["records"]

    def _col(self, name, game=0):
        return np.array(self.history(game)[name])

    outer_iter = property(lambda self: self._col("outer"))
    res = property(lambda self: self._col("res"))
    Δ_traj = property(lambda self: self._col("delta"))
    dyn_vio = property(lambda self: self._col("dyn_vio"))
    con_vio = property(lambda self: self._col("con_vio"))
    sta_vio = property(lambda self: self._col("sta_vio"))
    opt_vio = property(lambda self: self._col("opt_vio"))
    t_elap = property(lambda self: self._col("t_elap"))


# --------------------------------------------------------------------------------------------------
# Printers (src/utils.jl:37-84).  The solver runs on the device, so the per-iteration table of `opts.inner_print` is printed
# from the recorded history after the solve (game 0), one line per Newton iteration as solver_methods.jl:100 prints them.
# --------------------------------------------------------------------------------------------------
def scn(a, digits=1):
    """scn(a; digits), utils.jl:63-84: mantissa/exponent string such as ' 1.2e+3'."""
    assert digits >= 0
    if a == 0:
        e, m = 0, 0.0
    else:
        e = int(np.floor(np.log(abs(a)) / np.log(10)))
        m = a * np.exp(-e * np.log(10))
    m = round(m, digits)
    if digits == 0:
        strm = str(int(np.floor(m)))
    else:
        strm = str(float(m))
        strm = strm + "0" * abs(2 + digits + (m < 0) - len(strm))
    return f"{' ' if a >= 0 else ''}{strm}e{'+' if e >= 0 else ''}{e}"


def display_solver_header():
    print("%-3s %-2s %-2s %-6s %-6s %-6s " % ("out", "in", "α", "Δ", "res", "reg"))


def display_solver_data(k, l, j, Δ, res_norm, reg):
    reg_x = reg.x if hasattr(reg, "x") else reg
    print("%-3s %-2s %-2s %-6s %-6s %-6s " % (k, l, j, "%.0e" % Δ, "%.0e" % res_norm, "%.0e" % reg_x))


# Plot recipes (src/plots/solver_plots.jl:18-37,83-125) as plain data: what the recipes hand to Plots.jl, no drawing here.
def recipe_traj(model, states):
    """recipe_traj(model, traj): per player the x and y series (state entries pz[i][1], pz[i][2]) of a (N, n) state array;
    returned twice like the recipe (scatter + path series)."""
    states = np.asarray(states)
    x = [states[:, i] for i in range(model.p)]
    y = [states[:, model.p + i] for i in range(model.p)]
    return [x, x], [y, y]


def recipe_violation(stats, game=0):
    """recipe_violation(stats): log10 of the four violation histories clipped at 1e-10 and the outer-iteration epochs; returns
    (series_x, series_y, labels) with one shaded band per outer iteration followed by dyn / con / sta / opt."""
    h = stats.history(game)
    it = len(h)
    ser = {k: np.log10(np.maximum(1e-10, h[k + "_vio"])) for k in ("dyn", "con", "sta", "opt")}
    y_max = max(v.max() for v in ser.values())
    epochs = np.asarray(h["outer"])
    xs, ys, labels, i_start = [], [], [], 1
    for k in range(1, int(epochs[-1]) + 1):
        i_end = int(np.nonzero(epochs == k)[0][-1]) + 1
        xs.append(np.linspace(i_start, i_end, it)); ys.append(np.full(it, y_max)); labels.append("")
        i_start = i_end + 1
    x = np.arange(1, it + 1)
    for k in ("dyn", "con", "sta", "opt"):
        xs.append(x); ys.append(ser[k]); labels.append(k)
    return xs, ys, labels


def _print_history(prob):
    """What `opts.inner_print` shows (solver_methods.jl:36,100), replayed from game 0's history: a record is written at the
    top of every inner iteration; the line of an iteration carries that iteration's step (Δ is the next record's Δ_traj)."""
    h = prob.stats.history(0)
    display_solver_header()
    l = 0
    for idx in range(len(h) - 1):
        l = l + 1 if idx > 0 and h["outer"][idx] == h["outer"][idx - 1] else 1
        if h["ls_j"][idx] == 0:
            continue                                       # a record without a Newton step (gate / final record)
        display_solver_data(int(h["outer"][idx]), l, int(h["ls_j"][idx]), h["delta"][idx + 1], h["res"][idx], prob.opts.reg_0 * l ** 4)


# --------------------------------------------------------------------------------------------------
# GameProblem (src/problem/problem.jl:19-53)
# --------------------------------------------------------------------------------------------------
# --------------------------------------------------------------------------------------------------
# Batches of differing scenarios: per-game constraint / collision-cost numbers (alg_set_scenario_data)
# --------------------------------------------------------------------------------------------------
def _inf_pattern(a):
    a = np.asarray(a, dtype=np.float64)
    return tuple(np.where(np.isinf(a), np.sign(a), 0.0).tolist())


def scenario_structure(game_con):
    """What a batch's games must share: the (field, value) list of one GameConstraintValues, in a fixed order.  The numbers (radii,
    bounds, wall / circle / cylinder data) are not part of it, except the +-inf pattern of the bounds and the cylinder axes."""
    gc = game_con
    plen = lambda d: tuple((i, len(d[i]) if not isinstance(d[i], tuple) else len(d[i][0])) for i in sorted(d))
    return [
        ("collision avoidance (all pairs)", gc.collision_radius is not None),
        ("collision avoidance pairs", tuple(sorted(gc.collision_pairs))),
        ("spherical collision avoidance", bool(gc.spherical)),
        ("control bound", gc.u_max is not None),
        ("control bound +-inf pattern", None if gc.u_max is None else (_inf_pattern(gc.u_max), _inf_pattern(gc.u_min))),
        ("state bound players", tuple(sorted(gc.state_bounds))),
        ("state bound +-inf pattern", tuple((_inf_pattern(gc.state_bounds[i][0]), _inf_pattern(gc.state_bounds[i][1])) for i in sorted(gc.state_bounds))),
        ("walls", None if not gc.walls else len(gc.walls)),
        ("circles", None if gc.circles is None else len(gc.circles[0])),
        ("player walls", plen(gc.player_walls)),
        ("player circles", plen(gc.player_circles)),
        ("walls3d", None if not gc.walls3d else len(gc.walls3d)),
        ("cylinders", None if not gc.cylinders else tuple(c.v for c in gc.cylinders)),
        ("player walls3d", plen(gc.player_walls3d)),
        ("player cylinders", tuple((i, tuple(c.v for c in gc.player_cylinders[i])) for i in sorted(gc.player_cylinders))),
    ]


def _player_table(per_player):
    """The handle's table of distinct entries built from per-player lists the way alg_add_*_player builds it (players in increasing
    order, an identical entry shared): (table rows, [(player, index in that player's list) of every row's first occurrence, ...])."""
    rows, owners = [], []
    for i in sorted(per_player):
        for k, r in enumerate(per_player[i]):
            r = tuple(r)
            at = next((e for e, t in enumerate(rows) if t == r), None)
            if at is None:
                rows.append(r); owners.append([])
                at = len(rows) - 1
            owners[at].append((i, k))
    return rows, owners


def _wall_rows(ws):
    return [(w.p1[0], w.p1[1], w.p2[0], w.p2[1], w.v[0], w.v[1]) for w in ws]


def _wall3_rows(ws):
    return [tuple(np.concatenate([w.p1, w.p2, w.p3, w.v]).tolist()) for w in ws]


def _cyl_rows(cs):      # dedup key of the handle's table (p, axis, l, r); the per-game values drop the axis
    return [(c.p[0], c.p[1], c.p[2], float(c.v), c.l, c.r) for c in cs]


def _circle_rows(circ):
    xc, yc, r = circ
    return [(xc[k], yc[k], r[k]) for k in range(len(xc))]


def scenario_data(game_cons, game_obj=None, every_kind=False):
    """Per-game scenario data of a batch of GameConstraintValues (one per game) and an optional GameObjective whose collision
    cost may be (B, p).  Checks that every game has game 0's structure (AlgamesError naming the first game and field that differ)
    and returns {ALG_SCEN_* kind: (B, len) array} for the kinds whose numbers differ between the games; kinds equal for all games
    are left out (the handle's shared values, from game 0, hold for them) unless `every_kind` is set.  GameProblem sets it: a
    problem given per-game data runs on the kernels that read per-game blocks (EXT, or the base kernels' twins with
    scenario_kernels="base") whatever its games' numbers happen to be, so the arithmetic a game gets does
    not depend on how a batch is split into shards.  Per-player walls / circles / 3-D walls / cylinders map
    onto game 0's deduplicated table: a game that gives two players different values where game 0 shares one entry is rejected."""
    from ._abi import (ALG_SCEN_COLLISION_RADIUS, ALG_SCEN_COLLISION_COST, ALG_SCEN_CONTROL_BOUND, ALG_SCEN_STATE_BOUND,
                       ALG_SCEN_WALL, ALG_SCEN_CIRCLE, ALG_SCEN_WALL3D, ALG_SCEN_CYLINDER)
    cons = list(game_cons)
    B = len(cons)
    g0 = cons[0]
    p, n = g0.probsize.p, g0.probsize.n
    s0 = scenario_structure(g0)
    for g in range(1, B):
        for (field, v0), (_, v) in zip(s0, scenario_structure(cons[g])):
            if v != v0:
                raise AlgamesError(f"game_con[{g}] differs from game_con[0] in its structure: {field} ({v} vs {v0}); "
                                   "only the numbers may differ between the games of one batch")
    out = {}

    def table_values(get_rows, per_player_attr, all_attr, drop=None):
        """(B, entries x fields) values of one table kind for every game, or None if the kind is absent"""
        if getattr(g0, all_attr):
            vals = [get_rows(getattr(gc, all_attr)) for gc in cons]
        elif getattr(g0, per_player_attr):
            rows0, owners = _player_table({i: get_rows(v) for i, v in getattr(g0, per_player_attr).items()})
            vals = []
            for g, gc in enumerate(cons):
                pp = {i: get_rows(v) for i, v in getattr(gc, per_player_attr).items()}
                rows = []
                for e, own in enumerate(owners):
                    r = tuple(pp[own[0][0]][own[0][1]])
                    for (i, k) in own[1:]:
                        if tuple(pp[i][k]) != r:
                            raise AlgamesError(f"game_con[{g}]: players {own[0][0]} and {i} share entry {e} of the {per_player_attr} table "
                                               "in game_con[0] but have different values here")
                    rows.append(r)
                vals.append(rows)
        else:
            return None
        a = np.asarray(vals, dtype=np.float64)
        if drop is not None:
            a = np.delete(a, drop, axis=2)
        return a.reshape(B, -1)

    data = {}
    if g0.collision_radius is not None or g0.collision_pairs:
        a = np.zeros((B, p, p))
        for g, gc in enumerate(cons):
            if gc.collision_radius is not None:
                r = np.broadcast_to(np.asarray(gc.collision_radius, dtype=np.float64), (p,))
                a[g] = r[:, None] + r[None, :]
                np.fill_diagonal(a[g], 0.0)
            for (i, j), rad in gc.collision_pairs.items():
                a[g, i - 1, j - 1] = rad
        data[ALG_SCEN_COLLISION_RADIUS] = a.reshape(B, p * p)
    if game_obj is not None and game_obj.collision_radius is not None:
        r = np.broadcast_to(game_obj.collision_radius, (B, p)); mu = np.broadcast_to(game_obj.collision_μ, (B, p))
        data[ALG_SCEN_COLLISION_COST] = np.concatenate([r, mu], axis=1)
    if g0.u_max is not None:
        data[ALG_SCEN_CONTROL_BOUND] = np.stack([np.concatenate([np.asarray(gc.u_max, dtype=np.float64), np.asarray(gc.u_min, dtype=np.float64)]) for gc in cons])
    if g0.state_bounds:
        a = np.empty((B, 2, p, n))
        a[:, 0], a[:, 1] = np.inf, -np.inf
        for g, gc in enumerate(cons):
            for i, (mx, mn) in gc.state_bounds.items():
                a[g, 0, i - 1], a[g, 1, i - 1] = mx, mn
        data[ALG_SCEN_STATE_BOUND] = a.reshape(B, -1)
    for kind, rows_fn, own, shared, drop in ((ALG_SCEN_WALL, _wall_rows, "player_walls", "walls", None),
                                              (ALG_SCEN_CIRCLE, _circle_rows, "player_circles", "circles", None),
                                              (ALG_SCEN_WALL3D, _wall3_rows, "player_walls3d", "walls3d", None),
                                              (ALG_SCEN_CYLINDER, _cyl_rows, "player_cylinders", "cylinders", 3)):
        a = table_values(rows_fn, own, shared, drop)
        if a is not None:
            data[kind] = a
    for kind, a in data.items():
        if every_kind or not all(np.array_equal(a[g], a[0]) for g in range(1, B)):
            out[kind] = np.ascontiguousarray(a, dtype=np.float64)
    return out


def _obj_row(game_obj, g):
    """game_obj with its (B, p) collision cost reduced to game g's row (the handle's shared values)"""
    if game_obj.collision_radius is None or np.ndim(game_obj.collision_radius) == 1:
        return game_obj
    import copy
    o = copy.copy(game_obj)
    o.collision_radius, o.collision_μ = game_obj.collision_radius[g], game_obj.collision_μ[g]
    return o


class GameProblem:
    def __init__(self, N, dt, x0, model, opts, game_obj, game_con, backend=None, device=0, game_id0=0, scenario_kernels="ext",
                 history_profiles=0):
        """history_profiles: records per game whose `.vio` vectors newton_solve stores next to the history (Statistics.vio; 0 = off,
        the default; Batch.set_history_profiles -- the CPU oracle has no such entry point and raises AlgamesError).
        scenario_kernels: "ext" (default) or "base" -- which kernels per-game data of the base kinds runs on
        (Batch.set_scenario_kernels).  With "base" a problem that carries only the base constraint set keeps the base kernels (fused
        pass, teams, hand-off); every base kind the problem carries is still uploaded, so every shard takes the whole batch's path."""
        if scenario_kernels not in ("ext", "base"):
            raise ValueError(f"GameProblem: scenario_kernels must be 'ext' or 'base', got {scenario_kernels!r}")
        self.scenario_kernels = scenario_kernels
        self.probsize = ProblemSize(N, model)
        x0 = np.asarray(x0, dtype=np.float64)
        self.single = x0.ndim == 1
        self.x0 = np.ascontiguousarray(x0.reshape(-1, model.n))
        self.B = self.x0.shape[0]
        # game_con: one GameConstraintValues for every game, or a sequence of B of them (same structure, numbers may differ)
        self.game_cons = None
        if not isinstance(game_con, GameConstraintValues):
            self.game_cons = list(game_con)
            if len(self.game_cons) != self.B:
                raise ValueError(f"GameProblem: {len(self.game_cons)} game_con for a batch of {self.B} games")
            game_con = self.game_cons[0]
        cc = game_obj.collision_radius
        if cc is not None and np.ndim(cc) == 2 and np.shape(cc)[0] != self.B:
            raise ValueError(f"GameProblem: collision cost of {np.shape(cc)[0]} games for a batch of {self.B} games")
        # per-game data given: every kind goes to the device, so any shard of the batch runs the EXT kernels like the whole batch
        scen = scenario_data(self.game_cons or [game_con] * self.B, game_obj, every_kind=True) \
            if (self.game_cons or (cc is not None and np.ndim(cc) == 2)) else {}
        self.model, self.opts, self.game_obj, self.game_con = model, opts, game_obj, game_con
        game_obj = _obj_row(game_obj, 0)
        self.dt = dt
        self.game_id0 = game_id0
        lib = backend if backend is not None else hip_lib()
        self.batch = Batch(lib, model.model_id, model.p, N, dt, self.B, d=model.d, device=device)
        if isinstance(model, BicycleGame):
            self.batch.set_bicycle(model.lf, model.lr)
        if isinstance(model, QuadrotorGame) and model.mass != 0.5:
            self.batch.set_quadrotor(model.mass)
        if scenario_kernels == "base":       # before the adders (the default is not sent: a backend without the entry point keeps working)
            self.batch.set_scenario_kernels("base")
        self.batch.set_x0(self.x0)
        self.batch.set_lqr(game_obj.Qdiag, game_obj.Rdiag, game_obj.xf, game_obj.uf)
        if game_obj.collision_radius is not None:
            self.batch.add_collision_cost(game_obj.collision_radius, game_obj.collision_μ)
        if game_con.collision_radius is not None:
            if game_con.spherical:
                self.batch.add_spherical_collision_avoidance(game_con.collision_radius)
            else:
                self.batch.add_collision_avoidance(game_con.collision_radius)
        for (i, j) in sorted(game_con.collision_pairs):
            self.batch.add_collision_avoidance_pair(i - 1, j - 1, game_con.collision_pairs[(i, j)], spherical=game_con.spherical)
        if game_con.u_max is not None:
            self.batch.add_control_bound(game_con.u_max, game_con.u_min)
        for i in sorted(game_con.state_bounds):
            self.batch.add_state_bound(i - 1, *game_con.state_bounds[i])
        if game_con.walls:
            w = game_con.walls
            self.batch.add_wall_constraint([a.p1[0] for a in w], [a.p1[1] for a in w], [a.p2[0] for a in w],
                                           [a.p2[1] for a in w], [a.v[0] for a in w], [a.v[1] for a in w])
        if game_con.circles is not None:
            self.batch.add_circle_constraint(*game_con.circles)
        for i in sorted(game_con.player_walls):
            w = game_con.player_walls[i]
            self.batch.add_wall_constraint_player(i - 1, [a.p1[0] for a in w], [a.p1[1] for a in w], [a.p2[0] for a in w],
                                                  [a.p2[1] for a in w], [a.v[0] for a in w], [a.v[1] for a in w])
        for i in sorted(game_con.player_circles):
            self.batch.add_circle_constraint_player(i - 1, *game_con.player_circles[i])
        if game_con.walls3d:
            w = game_con.walls3d
            self.batch.add_wall3d_constraint([a.p1 for a in w], [a.p2 for a in w], [a.p3 for a in w], [a.v for a in w])
        if game_con.cylinders:
            c = game_con.cylinders
            self.batch.add_cylinder_constraint([a.p for a in c], [a.v for a in c], [a.l for a in c], [a.r for a in c])
        for i in sorted(game_con.player_walls3d):
            w = game_con.player_walls3d[i]
            self.batch.add_wall3d_constraint_player(i - 1, [a.p1 for a in w], [a.p2 for a in w], [a.p3 for a in w], [a.v for a in w])
        for i in sorted(game_con.player_cylinders):
            c = game_con.player_cylinders[i]
            self.batch.add_cylinder_constraint_player(i - 1, [a.p for a in c], [a.v for a in c], [a.l for a in c], [a.r for a in c])
        for kind in sorted(scen):       # after every adder: an adder drops per-game data
            self.batch.set_scenario_data(kind, scen[kind])
        self.stats = None
        for gc in (self.game_cons or [game_con]):
            gc.active_set_tolerance = opts.active_set_tolerance        # set_constraint_params!, game_constraints.jl:37
        self._sync_options()       # set_constraint_params!(game_con, opts), problem.jl:49
        if history_profiles:
            self.set_history_profiles(history_profiles)

    def set_history_profiles(self, max_records):
        """Per-record violation profiles of newton_solve (Batch.set_history_profiles): capacity in records per game, 0 = off."""
        self.batch.set_history_profiles(max_records)

    def _sync_options(self):
        # `opts` is shared by reference in Julia and read at solve time (tests mutate it after construction)
        self.batch.set_options(**self.opts.to_abi())

    def _traj(self, which):
        X, U, L = self.batch.split_traj(self.batch.get_traj(which))
        return PrimalDualTraj(X, U, L)

    @property
    def pdtraj(self):
        return self._traj(ALG_TRAJ_PD)

    @property
    def pdtraj_trial(self):
        return self._traj(ALG_TRAJ_TRIAL)

    @property
    def Δpdtraj(self):
        return self._traj(ALG_TRAJ_DELTA)

    def set_pdtraj(self, states=None, controls=None, duals=None):
        cur = self.pdtraj
        X = cur.states if states is None else np.broadcast_to(np.asarray(states, dtype=np.float64), cur.states.shape)
        U = cur.controls if controls is None else np.broadcast_to(np.asarray(controls, dtype=np.float64), cur.controls.shape)
        L = cur.duals if duals is None else np.broadcast_to(np.asarray(duals, dtype=np.float64), cur.duals.shape)
        self.batch.set_traj(self.batch.join_traj(np.array(X), np.array(U), np.array(L)))


# --------------------------------------------------------------------------------------------------
# Solver methods (src/problem/solver_methods.jl:5-125, src/problem/global_quantities.jl:1-193)
# --------------------------------------------------------------------------------------------------
def init_traj_host(prob):
    """init_traj!(prob.pdtraj; x0, f = opts.f_init, amplitude = opts.amplitude_init, s = opts.shift) (primal_dual_traj.jl:29-44,
    called at solver_methods.jl:13) for a CALLER-SUPPLIED generator: `opts.f_init` is a callable `f(size) -> array of that size`
    (the reference calls `f(SVector{n+m,T})` per knot and `f(SVector{n,T})` per player and step; `zeros`, `ones`, `randn` are the
    usual choices).  Calls are made game by game in the reference's order: knots k = 1..N (those with k + s > N), then players i,
    steps k = 1..N-1 (those with k + s > N-1).  The default `"rand"` never comes here: the device generates it (alg_init_traj).
    The result is stored as the handle's pdtraj; the solve then runs with init = 0, which still rolls the states out
    (solver_methods.jl:17), so only x_1 = x0, the controls and the duals of this guess matter.  The layout keeps no control at knot
    N (the reference's `pr[N]` carries one that nothing reads): when the shift copies knot N, its control is set to zero -- no draw
    is consumed for it, so a stateful generator stays aligned with the reference's call sequence.
    Every game is one `newton_solve!` of the reference, which calls `Random.seed!(opts.seed)` first (solver_methods.jl:9): NumPy's
    global generator is seeded the same way before each game's draws, so `f_init = np.random.randn` gives every game the stream the
    Julia shim gives it (generators that carry their own state, e.g. a `default_rng(...)` method, are not touched by this).  The
    caller's global NumPy generator state is saved before the loop and restored after it: the seeding is a detail of this call, not a
    side effect on the caller's stream.  (Deliberate deviation, stated: where the shift copies knot N the reference copies the STALE
    control `pr[N]` carries, primal_dual_traj.jl:35; the layout here has no such slot and stores zero.)"""
    b, o = prob.batch, prob.opts
    f, a, s = o.f_init, float(o.amplitude_init), int(min(o.shift, 2 ** 30))
    X, U, L = b.split_traj(b.get_traj(0))
    B, N, n, m, p = X.shape[0], b.N, b.n, b.m, b.p
    draw = lambda size: a * np.asarray(f(size), dtype=np.float64).reshape(size)
    rng_state = np.random.get_state()
    try:
        _init_traj_host_fill(o, X, U, L, B, N, n, m, p, s, draw)
    finally:
        np.random.set_state(rng_state)
    X[:, 0] = b.get_x0()
    b.set_traj(b.join_traj(X, U, L))


def _init_traj_host_fill(o, X, U, L, B, N, n, m, p, s, draw):
    for g in range(B):
        np.random.seed(int(o.seed) % (2 ** 32))                     # Random.seed!(opts.seed), solver_methods.jl:9
        for k in range(1, N + 1):                                   # 1-based like the reference
            if k + s <= N:
                X[g, k - 1] = X[g, k + s - 1]
                if k <= N - 1:
                    U[g, k - 1] = U[g, k + s - 1] if k + s <= N - 1 else 0.0
            else:
                z = draw(n + m)
                X[g, k - 1] = z[:n]
                if k <= N - 1:
                    U[g, k - 1] = z[n:]
        for i in range(p):
            for k in range(1, N):
                L[g, i, k - 1] = L[g, i, k + s - 1] if k + s <= N - 1 else draw(n)


def newton_solve(prob, init=True, history_profiles=None):
    """newton_solve!(prob) for every game of the batch (solver_methods.jl:5-65).
    init=False keeps the stored controls/duals as the initial guess (explicit warm start).
    history_profiles: None keeps the problem's setting; a count sets it first (prob.set_history_profiles; 0 = off) -- with profiles on,
    prob.stats.vio(game) returns the `.vio` vectors of every stored record.
    A `sharding.ShardedGameProblem` (batch split over several devices) is solved on all of its devices concurrently."""
    if history_profiles is not None:
        prob.set_history_profiles(history_profiles)
    if hasattr(prob, "shards"):
        from . import sharding
        if init and any(callable(q.opts.f_init) for q in prob.shards):
            for q in prob.shards:
                init_traj_host(q)
            init = False
        return sharding.newton_solve_sharded(prob, init=init)
    prob._sync_options()
    if init and callable(prob.opts.f_init):
        init_traj_host(prob)
        init = False
    summary = prob.batch.newton_solve(init=init, game_id0=prob.game_id0)
    prob.stats = Statistics(summary, prob.batch.get_history, prob.batch.get_history_vio if prob.batch.get_history_profiles() > 0 else None)
    if prob.opts.inner_print:
        _print_history(prob)
    return None


def residual(prob, which=ALG_TRAJ_PD, reg=0.0):
    """residual!(prob, pdtraj) (+ regularize_residual!): returns core.res, shape (B, S), vertical order."""
    prob._sync_options()
    return prob.batch.residual(which, reg)[0]


def residual_norm(prob, which=ALG_TRAJ_PD):
    """residual_norm(prob, pdtraj), global_quantities.jl:88-97."""
    prob._sync_options()
    return prob.batch.residual(which, 0.0, want_res=False)[1]


def residual_jacobian(prob, reg=0.0, games=None):
    """residual_jacobian! + regularize_residual_jacobian!: dense (B, S, S), [row vertical, col horizontal]; games = (first, count)
    builds only that range of the batch ((count, S, S))."""
    prob._sync_options()
    return prob.batch.residual_jacobian(reg, games)


class EquilibriumSensitivity:
    """d z* / d theta of a batch of games: `dz` is (cnt, S, q) in the horizontal order of Δtraj (rows) by the q entries of theta (columns);
    `status` (cnt,) is the per-game status of the solves (0 = every column solved).  The accessors slice rows by the index maps of
    horizontal_indices: knots and steps are 1-based like the reference's stamps.  steps = (first, count), 0-based: `dz` holds the rows of
    those steps only (parameter_sensitivity(steps=...)), count * b of them, and the accessors raise IndexError outside the slice."""

    def __init__(self, dz, status, wrt, N, n, p, mi, steps=None):
        self.dz, self.status, self.wrt = dz, status, wrt
        self.N, self.n, self.p, self.mi = N, n, p, mi
        self._b = n + p * mi + p * n
        self.steps = (0, N - 1) if steps is None else (int(steps[0]), int(steps[1]))

    def _row(self, step, what):
        """first row of the block of 0-based step `step` inside dz"""
        s0, ns = self.steps
        if not s0 <= step < s0 + ns:
            raise IndexError(f"{what}: the sensitivity holds steps {s0 + 1} ... {s0 + ns} only")
        return (step - s0) * self._b

    def dx(self, k):
        """d x_k / d theta, (cnt, n, q), knots k = 2 ... N (x_1 is the initial state itself)."""
        if not 2 <= k <= self.N:
            raise IndexError(f"state knot {k}: 2 ... {self.N}")
        o = self._row(k - 2, f"state knot {k}")
        return self.dz[:, o:o + self.n, :]

    def du(self, k, i=None):
        """d u_k / d theta, steps k = 1 ... N - 1: (cnt, m, q) in the stored order of get_traj (player by player), or player i's (cnt, mi, q)."""
        if not 1 <= k <= self.N - 1:
            raise IndexError(f"control step {k}: 1 ... {self.N - 1}")
        o = self._row(k - 1, f"control step {k}") + self.n
        if i is None:
            return self.dz[:, o:o + self.p * self.mi, :]
        if not 1 <= i <= self.p:
            raise IndexError(f"player {i}: 1 ... {self.p}")
        return self.dz[:, o + (i - 1) * self.mi:o + i * self.mi, :]

    def dλ(self, k, i):
        """d lambda_{i,k} / d theta (player i's multiplier of the dynamics of step k = 1 ... N - 1), (cnt, n, q)."""
        if not 1 <= k <= self.N - 1 or not 1 <= i <= self.p:
            raise IndexError(f"multiplier (player {i}, step {k}): players 1 ... {self.p}, steps 1 ... {self.N - 1}")
        o = self._row(k - 1, f"multiplier step {k}") + self.n + self.p * self.mi + (i - 1) * self.n
        return self.dz[:, o:o + self.n, :]

    dlam = dλ


def kkt_solve(prob, rhs=None, kind="user", reg=0.0, games=None):
    """J X = R at pdtraj on the device (Batch.kkt_solve): X (cnt, nrhs, S) in horizontal order and the per-game status."""
    prob._sync_options()
    return prob.batch.kkt_solve(rhs, kind, reg, games)


def equilibrium_sensitivity(prob, wrt="x0", reg=0.0, games=None):
    """How the equilibrium at pdtraj moves with the problem: d z* / d theta = -J^-1 d res / d theta for theta = the initial state (wrt = "x0",
    q = n columns) or the players' LQR targets x_f (wrt = "xf", q = p ni columns in the xf order of set_lqr), solved on the device in one
    launch (alg_kkt_solve).  Returns an EquilibriumSensitivity; `.dz` is (cnt, S, q) in horizontal order.

    Meaning: the derivative of the root z*(theta) of res(z; theta) = 0 -- the system newton_solve solves in its inner loop -- with the
    multipliers lambda and penalties mu of the constraints (and the active sets behind them) HELD at their current values.  J is the
    reference's residual Jacobian, which drops the second-order terms of the dynamics (global_quantities.jl:150-172): the result is exact
    for the double integrator (linear dynamics) and the Gauss-Newton sensitivity of that Jacobian for the unicycle, bicycle and quadrotor.
    A non-zero `reg` solves the regularised system (regularize_residual_jacobian!) instead.  Call it on a solved problem: away from a root the
    linearisation is still that of the current iterate.  games = (first, count)."""
    if wrt not in ("x0", "xf"):
        raise ValueError(f"wrt must be 'x0' or 'xf', got {wrt!r}")
    prob._sync_options()
    b = prob.batch
    X, st = b.kkt_solve(None, wrt, reg, games)
    return EquilibriumSensitivity(np.ascontiguousarray(X.transpose(0, 2, 1)), st, wrt, b.N, b.n, b.p, b.mi)


def feedback_gains(prob, games=None):
    """The local feedback policy around the plan at pdtraj: d u_1 / d x0, (cnt, m, n), rows in the stored order of get_traj (the order of the
    `controls` log of mpc_rollout), columns the entries of the initial state.  u_1(x0 + e) = u_1 + K e to first order, with multipliers and
    penalties held; exact for the double integrator, Gauss-Newton for the other models (equilibrium_sensitivity)."""
    return np.ascontiguousarray(equilibrium_sensitivity(prob, "x0", 0.0, games).du(1))


def parameter_sensitivity(prob, wrt, reg=0.0, games=None, steps=None, directions=None):
    """How the equilibrium at pdtraj moves with a parameter of the objectives or the constraints: d z* / d theta = -J^-1 d res / d theta with
    the right-hand sides built on the device (alg_kkt_sensitivity), one launch.  wrt: "x0", "xf", "Q", "R", "uf" (the orders of set_lqr),
    "collision_cost" (radius (p) | mu (p)), "collision_radius" (p x p ordered pairs), "control_bound" (u_max (m) | u_min (m)) -- the numbers a
    game was assembled with: per-game LQR data, its scenario block, else the handle's values.  The meaning is equilibrium_sensitivity's:
    multipliers, penalties and active sets are HELD, J is the reference's Jacobian (exact for the double integrator, Gauss-Newton otherwise).
    directions = None: one column per entry of theta.  directions[cnt, ndir, len] (or [cnt, len]): the columns are the directional
    derivatives along those vectors of parameter space, one elimination each.  steps = (first, count), 0-based steps: only their rows are
    computed into the output and downloaded (steps=(0, 1) with wrt="x0" is the feedback gain and the first state's sensitivity alone).
    games = (first, count).  Returns an EquilibriumSensitivity over the slice; `.dz` is (cnt, count * b, q)."""
    if wrt not in _abi.PARAM_KINDS:
        raise ValueError(f"wrt must be one of {_abi.PARAM_KINDS}, got {wrt!r}")
    prob._sync_options()
    b = prob.batch
    X, st = b.kkt_sensitivity(wrt, reg, games, steps, directions)
    return EquilibriumSensitivity(np.ascontiguousarray(X.transpose(0, 2, 1)), st, wrt, b.N, b.n, b.p, b.mi, steps)


NormalEquations = collections.namedtuple("NormalEquations", "H g loss status cols")
FitResult = collections.namedtuple("FitResult", "theta loss_history accepted status")
FIT_KINDS = ("xf", "Q", "R", "uf")            # what fit_parameters writes back through per-game set_lqr
FIT_DIAG_FLOOR = 1e-12                        # fit_parameters: the damping diagonal is max(diag H, FIT_DIAG_FLOOR max diag H)


def normal_columns(batch, wrt):
    """The (kind, index) columns `wrt` names: a sequence of kinds of PARAM_KINDS ("xf": every entry of it, in order) or (kind, indices) pairs;
    a single kind may be given as a string."""
    if isinstance(wrt, str):
        wrt = (wrt,)
    cols = []
    for item in wrt:
        kind, idx = (item, None) if isinstance(item, str) else (item[0], item[1])
        if kind not in _abi.PARAM_KINDS:
            raise ValueError(f"wrt must name kinds of {_abi.PARAM_KINDS}, got {kind!r}")
        ln = batch._param_len(_abi.PARAM_KINDS.index(kind))
        cols += [(kind, int(i)) for i in (range(ln) if idx is None else np.atleast_1d(idx))]
    return cols


def _observed_rows(b, observed, cnt):
    """the observation as (cnt, S) in horizontal order: an array of that shape, or states (cnt, N, n) and controls (cnt, N - 1, m) -- a
    PrimalDualTraj or a pair; the multiplier rows are zero (the default weight ignores them)"""
    if hasattr(observed, "states"):
        observed = (observed.states, observed.controls)
    if isinstance(observed, (tuple, list)) and len(observed) == 2 and np.ndim(observed[0]) == 3:
        X, U = (np.asarray(v, dtype=np.float64) for v in observed)
        if X.shape != (cnt, b.N, b.n) or U.shape != (cnt, b.N - 1, b.m):
            raise ValueError(f"observed: expected states {(cnt, b.N, b.n)} and controls {(cnt, b.N - 1, b.m)}, got {X.shape} and {U.shape}")
        return np.ascontiguousarray(b.join_traj(X, U, np.zeros((cnt, b.p, b.N - 1, b.n)))[:, b.n:])
    t = np.asarray(observed, dtype=np.float64)
    if t.shape != (cnt, b.S):
        raise ValueError(f"observed: expected shape {(cnt, b.S)} or a states / controls pair, got {t.shape}")
    return t


def default_fit_weight(b):
    """1 on the rows of states and controls, 0 on the rows of the dynamics multipliers: (S,) in horizontal order"""
    return np.ascontiguousarray(b.join_traj(np.ones((1, b.N, b.n)), np.ones((1, b.N - 1, b.m)), np.zeros((1, b.p, b.N - 1, b.n)))[0, b.n:])


def normal_scratch_bytes(batch, cols, games, per_game_weight=False):
    """Bytes of device scratch one alg_kkt_normal_equations call over `games` games takes: the column table, per kind the unit directions
    and the columns, target, weight, H, g, loss and the status words."""
    q, S = len(cols), batch.S
    kinds = collections.Counter(k for k, _ in cols)
    dirs = sum(c * batch._param_len(_abi.PARAM_KINDS.index(k)) for k, c in kinds.items())
    per_game = 8 * (dirs + q * S + S + (S if per_game_weight else 0) + q * q + q + 1) + 4 * (len(kinds) + 1)
    return 1024 + (0 if per_game_weight else 8 * S) + games * per_game


def normal_equations(prob, observed, wrt, weight=None, reg=0.0, games=None, max_scratch_bytes=1 << 30):
    """The normal equations of fitting the parameters `wrt` to an observed trajectory, reduced on the device (alg_kkt_normal_equations): with
    X the columns d z* / d theta of parameter_sensitivity (multipliers, penalties and active sets held; exact for the double integrator,
    Gauss-Newton otherwise) and r = z - observed over the S rows of pdtraj behind x_1, per game
        loss = 1/2 sum w r^2,    g = X' W r,    H = X' W X.
    wrt: kinds ("xf") or (kind, indices) pairs, up to 63 columns in all, in any mix and order (normal_columns).  observed: (cnt, S) in
    horizontal order, or a PrimalDualTraj-shaped states / controls pair.  weight: (S,) or (cnt, S), finite and >= 0; None is 1 on states and
    controls and 0 on the dynamics multipliers.  games = (first, count).  The game range is cut into chunks whose device scratch
    (normal_scratch_bytes: columns, directions, target, weight and results) stays under max_scratch_bytes -- one game at a time if even that
    is more; a game's numbers do not depend on the cut, bit for bit.  Call it on a solved problem.
    Returns NormalEquations(H (cnt, q, q), g (cnt, q), loss (cnt,), status (cnt,), cols); no column is downloaded."""
    prob._sync_options()
    b = prob.batch
    first, cnt = (0, b.B) if games is None else (int(games[0]), int(games[1]))
    if first < 0 or cnt < 1 or first + cnt > b.B:
        raise ValueError(f"games = (first, count) must lie inside the batch of {b.B}, got {games!r}")
    cols = normal_columns(b, wrt)
    t = _observed_rows(b, observed, cnt)
    w = default_fit_weight(b) if weight is None else np.asarray(weight, dtype=np.float64)
    fixed = normal_scratch_bytes(b, cols, 0, w.ndim == 2)
    step = max(1, (int(max_scratch_bytes) - fixed) // (normal_scratch_bytes(b, cols, 1, w.ndim == 2) - fixed))
    if step >= cnt:
        return NormalEquations(*b.kkt_normal_equations(cols, t, w, reg, (first, cnt)), cols)
    if w.shape not in ((b.S,), (cnt, b.S)):
        raise ValueError(f"weight: expected shape {(b.S,)} or {(cnt, b.S)}, got {w.shape}")
    parts = [b.kkt_normal_equations(cols, t[a:a + step], w if w.ndim == 1 else w[a:a + step], reg, (first + a, min(step, cnt - a))) for a in range(0, cnt, step)]
    return NormalEquations(*(np.concatenate([part[k] for part in parts]) for k in range(4)), cols)


def fit_parameters(prob, observed, wrt, weight=None, iters=20, damping=1e-3, reg=0.0):
    """Fit LQR parameters of every game of the batch to an observed play: a batched Levenberg-Marquardt loop on the device's normal equations,
    one damping lambda_g per game.  wrt: kinds of FIT_KINDS ("xf", "Q", "R", "uf") or (kind, indices) pairs; theta_0 is prob.game_obj's data.
    The loop writes theta_0 per game (set_lqr), solves (newton_solve) and forms the normal equations; then, `iters` times:
        solve (H + lambda_g diag(H)) delta = -g per game (the diagonal floored at FIT_DIAG_FLOOR of its maximum), set theta + delta on every
        game, run one warm-started newton_solve of the batch and one normal_equations call;
        game g accepts, with lambda_g /= 10, if its solve converged with status 0, the normal equations' status is 0, the loss fell and every
        fitted Q and R entry stays > 0; else its theta, pdtraj and constraint duals are put back from host copies and lambda_g *= 10.
    One solve and one reduction call per iteration; no sensitivity column leaves the device.
    Scale freedom: multiplying ALL of one player's Q and R by one factor moves no trajectory, so Q and R of a player cannot be fitted
    together -- fit Q with R held, or R with Q held.
    Returns FitResult(theta (B, q) in the order of normal_columns(wrt), loss_history (iters + 1, B) -- the loss of the accepted state after
    every iteration, non-increasing --, accepted (iters, B) bool, status (B,) of the accepted state's normal equations).  The handle is left
    with the fitted values as per-game LQR data and each game's accepted plan in pdtraj; prob.game_obj is not modified."""
    b = prob.batch
    cols = normal_columns(b, wrt)
    if any(k not in FIT_KINDS for k, _ in cols):
        raise ValueError(f"fit_parameters: wrt must name kinds of {FIT_KINDS}")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0 or not (np.isfinite(damping) and damping > 0):
        raise ValueError("fit_parameters: iters must be an integer >= 0 and damping a positive number")
    B, q, o = b.B, len(cols), prob.game_obj
    t = _observed_rows(b, observed, B)
    data = {"Q": np.array(np.broadcast_to(o.Qdiag, (B, b.p, b.ni)), dtype=np.float64), "xf": np.array(np.broadcast_to(o.xf, (B, b.p, b.ni)), dtype=np.float64),
            "R": np.array(np.broadcast_to(o.Rdiag, (B, b.p, b.mi)), dtype=np.float64), "uf": np.array(np.broadcast_to(o.uf, (B, b.p, b.mi)), dtype=np.float64)}
    positive = np.array([k in ("Q", "R") for k, _ in cols])

    def gather():
        return np.stack([data[k].reshape(B, -1)[:, i] for k, i in cols], axis=1)

    def scatter(theta):
        for c, (k, i) in enumerate(cols):
            data[k].reshape(B, -1)[:, i] = theta[:, c]
        b.set_lqr(data["Q"], data["R"], data["xf"], data["uf"])

    def solve_and_reduce(init):
        newton_solve(prob, init=init)
        s = prob.stats.summary
        ne = normal_equations(prob, t, cols, weight, reg)
        ok = (s["converged"] == 1) & (s["status"] == 0) & (ne.status == 0) & np.isfinite(ne.loss)
        return ne, ok

    theta = gather()
    scatter(theta)
    ne, _ = solve_and_reduce(True)
    Hm, g, loss, status = ne.H.copy(), ne.g.copy(), ne.loss.copy(), ne.status.copy()
    lam = np.full(B, float(damping))
    history, accepted = [loss.copy()], np.zeros((iters, B), dtype=bool)
    for it in range(iters):
        z = b.get_traj()
        duals = b.get_con_duals() if b.con_len else None
        delta = lm_step(Hm, g, lam)
        trial = theta + delta
        sane = np.all(np.isfinite(trial), axis=1) & np.all(trial[:, positive] > 0, axis=1)
        trial[~sane] = theta[~sane]
        scatter(trial)
        ne, ok = solve_and_reduce(False)
        acc = sane & ok & (ne.loss < loss)
        accepted[it] = acc
        theta[acc] = trial[acc]; Hm[acc] = ne.H[acc]; g[acc] = ne.g[acc]; loss[acc] = ne.loss[acc]; status[acc] = ne.status[acc]
        lam = np.where(acc, lam / 10.0, lam * 10.0)
        if not acc.all():                                     # the rejected games go back to their accepted state
            scatter(theta)
            z2 = b.get_traj(); z2[~acc] = z[~acc]
            b.set_traj(z2)
            if duals is not None:
                l2, m2 = b.get_con_duals(); l2[~acc] = duals[0][~acc]; m2[~acc] = duals[1][~acc]
                b.set_con_duals(l2, m2)
        history.append(loss.copy())
    return FitResult(theta, np.stack(history), accepted, status)


def lm_step(Hm, g, lam):
    """delta of (H + lambda diag(H)) delta = -g per game, the diagonal floored at FIT_DIAG_FLOOR of its maximum; a game whose system is
    singular or not finite gets delta = 0"""
    B, q = g.shape
    delta = np.zeros((B, q))
    for k in range(B):
        d = np.diagonal(Hm[k])
        if not (np.all(np.isfinite(Hm[k])) and np.all(np.isfinite(g[k])) and d.max() > 0):
            continue
        A = Hm[k] + lam[k] * np.diag(np.maximum(d, FIT_DIAG_FLOOR * d.max()))
        try:
            s = np.linalg.solve(A, -g[k])
        except np.linalg.LinAlgError:
            continue
        if np.all(np.isfinite(s)):
            delta[k] = s
    return delta


def inner_iteration(prob, LS_count, t_elap, Δ, k, l):
    """inner_iteration(prob, LS_count, t_elap, Δ, k, l) (solver_methods.jl:67-103).
    Returns (LS_count (B,), control_flow (B,) of 'continue'/'break', Δ (B,), info)."""
    prob._sync_options()
    info = prob.batch.newton_step(k, l, delta=Δ)
    LS = np.where(info["ls_failed"] == 1, np.asarray(LS_count) + 1, 0)
    LS = np.where(info["ls_j"] == 0, np.asarray(LS_count), LS)
    flow = np.where(info["control_flow"] == 1, "break", "continue")
    return LS, flow, info["delta"], info


def line_search(prob, res_norm, reg=0.0):
    """line_search(prob, res_norm) (solver_methods.jl:105-125) -> (α, j)."""
    prob._sync_options()
    return prob.batch.line_search(res_norm, reg)


def violation_profile(prob):
    """The `.vio` vectors of dynamics_violation / control_violation / state_violation / optimality_violation at pdtraj
    (violations.jl:5-26, 41-67, 86-114, 140-168): dict(dyn (B, N-1), con (B, N-1), sta (B, N), opt (B, N)); their maxima over the knots
    are the `*_vio` entries record! stores."""
    prob._sync_options()
    return prob.batch.violation_profile()


def player_costs(prob, which="pd", stage=False):
    """What the plan costs each player, evaluated on the device (alg_get_cost): (B, p, 3) with the components [state, control, collision]
    of J_i = sum_k w_k l_i(x_k, u_k) -- the LQRCost objectives (objective.jl:12-35) and the CollisionCost's stage_cost (objective.jl:122-131)
    with the weights of the cost gradients, w_k = dt for k < N and w_N = 1; constraints, multipliers and penalties do not enter.
    which: "pd" (prob.pdtraj) or "trial" (prob.pdtraj_trial).  stage=True also returns the summands per knot: (total, stage (B, N, p, 3))."""
    code = {"pd": ALG_TRAJ_PD, "trial": ALG_TRAJ_TRIAL}.get(which, which) if isinstance(which, str) else which
    if isinstance(code, str):
        raise ValueError(f"player_costs: which must be 'pd' or 'trial', got {which!r}")
    return prob.batch.get_cost(code, stage=stage)


def _stage_cost(b, x, u, Q, R, xf, uf, rad, mu):
    """l_i of the cost definition (alg_get_cost) in numpy, unweighted: x (B, n); u (B, m) player-major, or None at a terminal knot; Q, xf
    (B, p, ni); R, uf (B, p, mi); rad, mu (B, p), or None without a collision cost.  Returns (B, p, 3) [state, control, collision]."""
    p = b.p
    xi = x.reshape(-1, b.ni, p).transpose(0, 2, 1)                  # pz_i[a] = a p + i
    out = np.zeros((x.shape[0], p, 3))
    out[..., 0] = 0.5 * np.sum(Q * (xi - xf) ** 2, axis=-1)
    if u is not None:
        out[..., 1] = 0.5 * np.sum(R * (u.reshape(-1, p, b.mi) - uf) ** 2, axis=-1)
    if rad is not None and p > 1:
        pos = xi[..., :2]                                           # px_i: entries i and p + i of the joint state
        dist = np.linalg.norm(pos[:, :, None, :] - pos[:, None, :, :], axis=-1)
        pen = np.maximum(0.0, rad[:, :, None] - dist) ** 2
        pen[:, np.arange(p), np.arange(p)] = 0.0
        out[..., 2] = 0.5 * mu * pen.sum(axis=-1)
    return out


def _cost_numbers(prob, sched, t):
    """the numbers the running cost of solve t's knots is taken with (alg_mpc_get_cost): Q, R as set; xf, uf and the collision cost's
    radius, mu from row min(t, rows - 1) of their schedules where scheduled, else the problem's"""
    b, obj = prob.batch, prob.game_obj
    full = lambda a, w: np.broadcast_to(np.asarray(a, dtype=np.float64), (b.B, b.p, w))
    Q, R, xf, uf = full(obj.Qdiag, b.ni), full(obj.Rdiag, b.mi), full(obj.xf, b.ni), full(obj.uf, b.mi)
    rad = mu = None
    if obj.collision_radius is not None:
        if "get_scenario_data" not in getattr(b.lib, "absent", ()):
            cc = b.get_scenario_data(ALG_SCEN_COLLISION_COST)       # what the handle holds: the games' blocks or the shared values
            rad, mu = cc[:, :b.p], cc[:, b.p:]
        else:
            rad = np.broadcast_to(np.asarray(obj.collision_radius, dtype=np.float64), (b.B, b.p))
            mu = np.broadcast_to(np.asarray(obj.collision_μ, dtype=np.float64), (b.B, b.p))
    for k, a in sched:
        row = a[min(t, a.shape[0] - 1)]
        if k == ALG_SCHED_LQR_TARGET:
            w = b.p * b.ni
            xf, uf = row[:, :w].reshape(b.B, b.p, b.ni), row[:, w:].reshape(b.B, b.p, b.mi)
        elif k == ALG_SCEN_COLLISION_COST:
            rad, mu = row[:, :b.p], row[:, b.p:]
    return Q, R, xf, uf, rad, mu


def constraint_values(prob, which="pd"):
    """The constraint values of the plan, read-only, evaluated on the device (alg_get_con_values): (B, con_len) in the ABI's constraint
    layout -- evaluate!(game_con, traj) (constraints_methods.jl:329-379) without the dual and penalty update; c <= 0 is feasible, a row of
    an infinite bound reports -inf, an inert row 0.  which: "pd" (prob.pdtraj) or "trial" (prob.pdtraj_trial)."""
    code = {"pd": ALG_TRAJ_PD, "trial": ALG_TRAJ_TRIAL}.get(which, which) if isinstance(which, str) else which
    if isinstance(code, str):
        raise ValueError(f"constraint_values: which must be 'pd' or 'trial', got {which!r}")
    return prob.batch.get_con_values(code)


def _con_tables(prob):
    """What the constraint rows of a knot are built from, host side: {ALG_SCEN_* kind: (B, len) numbers in the caller's order} of every
    constraint kind the problem carries (scenario_data's arrays: a schedule row of the kind has the same layout) and the structure the
    handle keeps -- pair mask (p, p), spherical, per-player masks (p, entries) of the four tables, cylinder axes."""
    from ._abi import ALG_SCEN_WALL, ALG_SCEN_CIRCLE, ALG_SCEN_WALL3D, ALG_SCEN_CYLINDER
    b = prob.batch
    cons = prob.game_cons or [prob.game_con] * b.B
    gc, p = cons[0], b.p
    nums = scenario_data(cons, None, every_kind=True)
    pairs = np.zeros((p, p), dtype=bool)
    if gc.collision_radius is not None:
        pairs[:] = ~np.eye(p, dtype=bool)
    for (i, j) in gc.collision_pairs:
        pairs[i - 1, j - 1] = True
    masks = {}
    for kind, rows_fn, own, shared in ((ALG_SCEN_WALL, _wall_rows, "player_walls", "walls"), (ALG_SCEN_CIRCLE, _circle_rows, "player_circles", "circles"),
                                       (ALG_SCEN_WALL3D, _wall3_rows, "player_walls3d", "walls3d"), (ALG_SCEN_CYLINDER, _cyl_rows, "player_cylinders", "cylinders")):
        if getattr(gc, shared):
            masks[kind] = np.ones((p, len(rows_fn(getattr(gc, shared)))), dtype=bool)
        elif getattr(gc, own):
            rows, owners = _player_table({i: rows_fn(v) for i, v in getattr(gc, own).items()})
            masks[kind] = np.zeros((p, len(rows)), dtype=bool)
            for e, own_e in enumerate(owners):
                for (i, _) in own_e:
                    masks[kind][i - 1, e] = True
    axes = None
    if gc.cylinders:
        axes = np.array([c.v for c in gc.cylinders])
    elif gc.player_cylinders:
        axes = np.array([int(r[3]) for r in _player_table({i: _cyl_rows(v) for i, v in gc.player_cylinders.items()})[0]])
    return dict(nums=nums, pairs=pairs, spherical=bool(gc.spherical), masks=masks, axes=axes)


def _con_knot(b, tab, nums, x, u):
    """The K1 constraint rows of one step in numpy (alg_get_con_values' knot layout): x (B, n) the state the step reaches, u (B, m) its
    control in the stored player-major order, nums {kind: (B, len)} the numbers in force.  Returns (vals (B, K1), kind of every row (K1,):
    an ALG_CON_* value, -1 for the rows of a base block that was not added)."""
    from ._abi import (ALG_SCEN_COLLISION_RADIUS, ALG_SCEN_CONTROL_BOUND, ALG_SCEN_STATE_BOUND, ALG_SCEN_WALL, ALG_SCEN_CIRCLE,
                       ALG_SCEN_WALL3D, ALG_SCEN_CYLINDER)
    B, p, n, m = x.shape[0], b.p, b.n, b.m
    pos = lambda i, a: x[:, a * p + i]                              # pz_i[a] = a p + i
    out, kinds = [], []
    for i in range(p):
        for j in range(p):
            if j == i:
                continue
            if ALG_SCEN_COLLISION_RADIUS in nums and tab["pairs"][i, j]:
                R = nums[ALG_SCEN_COLLISION_RADIUS].reshape(B, p, p)[:, i, j]
                d2 = sum((pos(i, a) - pos(j, a)) ** 2 for a in range(3 if tab["spherical"] else 2))
                out.append(R * R - d2)
            else:
                out.append(np.zeros(B))
            kinds.append(0 if ALG_SCEN_COLLISION_RADIUS in nums else -1)
    uj = u.reshape(B, p, b.mi).transpose(0, 2, 1).reshape(B, m)     # joint order c = a p + i
    if ALG_SCEN_CONTROL_BOUND in nums:
        bd = nums[ALG_SCEN_CONTROL_BOUND]
        out += list((uj - bd[:, :m]).T) + list((bd[:, m:] - uj).T)
        kinds += [1] * (2 * m)
    else:
        out += [np.zeros(B)] * (2 * m)
        kinds += [-1] * (2 * m)
    if ALG_SCEN_STATE_BOUND in nums:
        sb = nums[ALG_SCEN_STATE_BOUND].reshape(B, 2, p, n)
        for i in range(p):
            out += list((x - sb[:, 0, i]).T) + list((sb[:, 1, i] - x).T)
            kinds += [2] * (2 * n)
    if ALG_SCEN_WALL in nums:
        W = nums[ALG_SCEN_WALL].reshape(B, -1, 6)
        for i in range(p):
            for w in range(W.shape[1]):
                x1, y1, x2, y2, xv, yv = W[:, w].T
                px, py = pos(i, 0), pos(i, 1)
                inside = ((px - x1) * (x2 - x1) + (py - y1) * (y2 - y1) > 0) & ((px - x2) * (x1 - x2) + (py - y2) * (y1 - y2) > 0)
                out.append(np.where(inside & tab["masks"][ALG_SCEN_WALL][i, w], (px - x1) * xv + (py - y1) * yv, 0.0))
                kinds.append(3)
    if ALG_SCEN_CIRCLE in nums:
        Cc = nums[ALG_SCEN_CIRCLE].reshape(B, -1, 3)
        for i in range(p):
            for c in range(Cc.shape[1]):
                v = Cc[:, c, 2] ** 2 - (pos(i, 0) - Cc[:, c, 0]) ** 2 - (pos(i, 1) - Cc[:, c, 1]) ** 2
                out.append(np.where(tab["masks"][ALG_SCEN_CIRCLE][i, c], v, 0.0))
                kinds.append(4)
    if ALG_SCEN_WALL3D in nums:
        W = nums[ALG_SCEN_WALL3D].reshape(B, -1, 4, 3)
        for i in range(p):
            q = np.stack([pos(i, 0), pos(i, 1), pos(i, 2)], axis=1)
            for w in range(W.shape[1]):
                p1, p2, p3, v = (W[:, w, f] for f in range(4))
                dot = lambda a, e, c: np.sum((q - a) * (e - c), axis=1)
                inside = (dot(p1, p2, p1) > 0) & (dot(p2, p1, p2) > 0) & (dot(p3, p2, p3) > 0) & (dot(p2, p3, p2) > 0)
                out.append(np.where(inside & tab["masks"][ALG_SCEN_WALL3D][i, w], np.sum((q - p1) * v, axis=1), 0.0))
                kinds.append(5)
    if ALG_SCEN_CYLINDER in nums:
        Y = nums[ALG_SCEN_CYLINDER].reshape(B, -1, 5)
        for i in range(p):
            q = np.stack([pos(i, 0), pos(i, 1), pos(i, 2)], axis=1)
            for c in range(Y.shape[1]):
                t0 = q - Y[:, c, :3]
                ta = t0[:, tab["axes"][c]]
                v = Y[:, c, 4] ** 2 - np.sum(t0 ** 2, axis=1) + ta ** 2
                out.append(np.where((ta > 0) & (ta < Y[:, c, 3]) & tab["masks"][ALG_SCEN_CYLINDER][i, c], v, 0.0))
                kinds.append(6)
    return np.stack(out, axis=1), np.array(kinds)


def _con_summary(con, kinds):
    """worst (B, 7) and first (B, 7) of a constraint log con (knots, B, K1): alg_mpc_get_con's summary"""
    B = con.shape[1]
    worst = np.full((B, ALG_CON_KINDS), -np.inf); first = np.full((B, ALG_CON_KINDS), -1, dtype=np.int32)
    for c in range(ALG_CON_KINDS):
        v = con[:, :, kinds == c]
        if v.shape[2] == 0:
            continue
        worst[:, c] = v.max(axis=(0, 2)) + 0.0                      # (a NaN propagates; + 0.0: -0 reads +0)
        bad = ~(v <= 0.0)
        hit = bad.any(axis=2)
        first[:, c] = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
    return worst, first


def dynamics_violation(prob):
    return prob.batch.record()["dyn_vio"]


def control_violation(prob):
    return prob.batch.record()["con_vio"]


def state_violation(prob):
    return prob.batch.record()["sta_vio"]


def optimality_violation(prob):
    return prob.batch.record()["opt_vio"]


# --------------------------------------------------------------------------------------------------
# Iterated best response (src/struct/options.jl:123-136, src/problem/solver_methods.jl:133-289)
# --------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class IBROptions:
    ibr_iter: int = 100
    ordering: list = dataclasses.field(default_factory=lambda: list(range(1, 101)))   # 1-based player ids, like the reference
    Δ_min: float = 1e-9
    live_plotting: bool = False


def ibr_newton_solve(prob, i=None, ibr_opts=None, init=True):
    """ibr_newton_solve!(prob; ibr_opts) (solver_methods.jl:133-169), or with a 1-based player index `i`
    ibr_newton_solve!(prob, i) (:171-228) on the stored trajectory."""
    prob._sync_options()
    if i is not None:
        summary = prob.batch.ibr_solve_player(i - 1)
    else:
        o = ibr_opts if ibr_opts is not None else IBROptions()
        order = [j - 1 for j in list(o.ordering)[:prob.probsize.p]]
        if init and callable(prob.opts.f_init):
            init_traj_host(prob)
            init = False
        summary = prob.batch.ibr_newton_solve(o.ibr_iter, order, o.Δ_min, init=init, game_id0=prob.game_id0)
    prob.stats = Statistics(summary, prob.batch.get_history)
    return None


# --------------------------------------------------------------------------------------------------
# Receding-horizon loop (BASELINE config 5).  Not in the reference: Algames.jl v0.1.6 only has the warm-start hooks
# `opts.shift` / `opts.dual_reset` (options.jl:16-17, primal_dual_traj.jl:35-39, solver_methods.jl:25).  Builder-defined
# (SURVEY.md 8(d) C5): solve; x0 <- RK2(x_1, u_1); next solve warm-started with shift = 1 and dual_reset = false.
# --------------------------------------------------------------------------------------------------
def _mpc_schedule(b, schedule):
    """{kind: array (rows, B, len)} -> [(ABI kind, array)] in kind order, shapes checked before any library call"""
    sched = []
    for kind in (schedule or {}):
        k, L = b._sched_kind(kind)
        if k == ALG_SCHED_DISTURBANCE:
            raise ValueError(f"schedule of kind {kind!r}: the disturbance is no entry of `schedule`: it is the `disturbance` argument of mpc_rollout; "
                             "for mpc_solve upload it with Batch.mpc_set_schedule('disturbance', w) before the call")
        a = np.ascontiguousarray(np.asarray(schedule[kind], dtype=np.float64))
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (b.B, L):
            raise ValueError(f"schedule of kind {kind!r}: expected shape (rows >= 1, {b.B}, {L}), got {a.shape}")
        sched.append((k, a))
    sched.sort(key=lambda ka: ka[0])
    return sched


def _apply_schedule_rows(prob, sched, t):
    """the step-wise definition of the schedule: row min(t, rows - 1) of every kind through set_scenario_data / set_lqr"""
    b = prob.batch
    for k, a in sched:
        r = min(t, a.shape[0] - 1)
        if t > 0 and r == min(t - 1, a.shape[0] - 1):
            continue                            # the last row is held: nothing to upload
        if k == ALG_SCHED_LQR_TARGET:
            obj = prob.game_obj
            if np.ndim(obj.Qdiag) != 3:
                raise AlgamesError("mpc_solve: a target schedule needs per-game LQR data (Qdiag, Rdiag of shape (B, p, .))")
            w = b.p * b.ni
            b.set_lqr(obj.Qdiag, obj.Rdiag, a[r][:, :w].reshape(b.B, b.p, b.ni), a[r][:, w:].reshape(b.B, b.p, b.mi))
        else:
            b.set_scenario_data(k, a[r])


@contextlib.contextmanager
def _with_plant(b, plant):
    """the handle's plant for one call: `plant` is set and the previous one restored; None leaves the handle alone.  Yields the plant in force."""
    if plant is None:
        yield b.mpc_get_plant()
        return
    if not isinstance(plant, Plant):
        raise ValueError(f"plant: expected a Plant or None, got {type(plant).__name__}")
    old = b.mpc_get_plant()
    b.mpc_set_plant(plant)
    try:
        yield plant
    finally:
        b.mpc_set_plant(old)


def mpc_solve(prob, steps, record_states=False, fused=True, schedule=None, plant=None):
    """Runs `steps` receding-horizon solves for every game of the batch.  Returns (newton_iters (B,), converged (B,),
    states (steps * hold + 1, B, n) or None).  fused=True: one launch, every game runs its own loop (alg_mpc_solve); fused=False:
    one newton_solve! launch + one advance launch per plant knot (the batch waits for its slowest game at every step).
    No host synchronisation happens inside the loop unless record_states is set.

    schedule: {kind: array (rows, B, len)} -- values per MPC step and game of the numbers that may differ per game; kind is a scenario
    kind (Batch.set_scenario_data) or "lqr_target" (xf (p, ni) | uf (p, mi) of every game; the problem needs per-game LQR data).  Step t
    solves with row min(t, rows - 1) of every kind.  fused=True uploads the schedule (Batch.mpc_set_schedule), launches once and drops it
    again; fused=False applies the step's rows through set_scenario_data / set_lqr before each step's solve -- the definition the fused
    path is held to.  Either way the handle keeps the rows the last step used.

    plant: a Plant -- every solve is followed by plant.hold plant knots, each integrated in plant.substeps sub-steps (see mpc_rollout);
    set on the handle for the call and restored afterwards.  None: the handle's own plant, by default the loop without one."""
    b = prob.batch
    sched = _mpc_schedule(b, schedule)
    with _with_plant(b, plant) as pl:
        b.mpc_totals(reset=True)
        prob._sync_options()
        if fused:
            for k, a in sched:
                b.mpc_set_schedule(k, a)
            try:
                states = b.mpc_solve(steps, prob.game_id0, record_states)
                it, cv = b.mpc_totals()
            finally:
                for k, a in sched:
                    b.mpc_set_schedule(k, None)
            return it, cv, states
        shift0, reset0 = prob.opts.shift, prob.opts.dual_reset
        states = [b.get_x0()] if record_states else None
        stepwise_plant = plant is not None or not pl.is_default

        try:
            for t in range(steps):
                if t == 1:
                    prob.opts.shift, prob.opts.dual_reset = pl.hold, False
                    prob._sync_options()
                _apply_schedule_rows(prob, sched, t)
                b.newton_solve_async(init=True, game_id0=prob.game_id0 + t * 1000003)
                for j in range(pl.hold):
                    if stepwise_plant:
                        b.mpc_plant_advance(j)
                    else:
                        b.mpc_advance()
                    if record_states:
                        states.append(b.get_x0())
            it, cv = b.mpc_totals()
        finally:
            prob.opts.shift, prob.opts.dual_reset = shift0, reset0
            prob._sync_options()
        return it, cv, (np.stack(states) if record_states else None)


@dataclasses.dataclass
class MpcRollout:
    """Closed-loop log of mpc_rollout over steps solves and knots = steps * hold plant knots (hold = 1 without a plant): states
    (knots+1, B, n) -- x0 before the loop and after every knot, disturbed where a disturbance acts --, controls (knots, B, m) -- the joint
    control every knot held, player-major --, stats (steps, B) of game_stats_dtype -- every step's solve as get_stats reports it --, and the
    totals newton_iters (B,), converged (B,), which gain every solve once.  With costs=True also stage_cost (knots, B, p, 3) -- the running
    cost dt l_i(states[q], controls[q]) of every knot and player in the components [state, control, collision] of player_costs, taken with
    the schedule rows the knot's solve used -- and cost (B, p, 3), its sum over the knots (no terminal term); None otherwise.  With
    constraints=True also con (knots, B, K1) -- the constraint rows of every knot in the knot layout of alg_get_con_values: the control-bound
    rows on controls[q], every other row on states[q + 1], with the schedule rows the knot's solve used --, con_worst (B, 7) -- the maximum
    of every ALG_CON_* kind's rows over the run, -inf for a kind that was not added -- and con_first (B, 7) int32 -- the first knot with a
    row that is not <= 0, -1 if none; None otherwise."""
    states: np.ndarray
    controls: np.ndarray
    stats: np.ndarray
    newton_iters: np.ndarray
    converged: np.ndarray
    stage_cost: np.ndarray = None
    cost: np.ndarray = None
    con: np.ndarray = None
    con_worst: np.ndarray = None
    con_first: np.ndarray = None


def mpc_rollout(prob, steps=None, schedule=None, disturbance=None, fused=True, plant=None, costs=False, constraints=False):
    """The receding-horizon loop as a closed-loop simulation: mpc_solve's loop with every step observable and a disturbed plant.  Returns
    an MpcRollout.  steps=None takes prob.opts.mpc_horizon.

    schedule: as for mpc_solve.  disturbance: (rows, B, n), finite -- after plant knot q the state becomes
    x0 + disturbance[min(q, rows - 1)] (the last row is held); states[q + 1] is the disturbed state.
    plant: a Plant(hold, substeps, integrator), set on the handle for the call and restored afterwards (None: the handle's own, by default
    Plant()).  Solve t is followed by the knots q = t * hold + j, j < hold: knot j holds u_{1+j} of the solve's plan and integrates the state
    over dt in `substeps` sub-steps of the model's own RK2 step ("rk2") or the classical RK4 on its continuous dynamics ("rk4"); the next
    solve is warm-started with shift = hold.  Without a plant a knot is a step: q = t.
    fused=True: one launch (alg_mpc_solve_log; schedule and disturbance are uploaded and dropped again); fused=False: the definition --
    per step the schedule rows, newton_solve_async, get_stats and the controls of get_traj, then per knot mpc_plant_advance(j) (mpc_advance
    without a plant), x0 read back, set_x0(x0 + w_q).
    costs=True: what the run cost each player (MpcRollout.stage_cost, .cost).  fused=True takes them from the device's cost log
    (Batch.mpc_set_cost_log, switched on for the call); fused=False evaluates the definition in numpy on the states and controls of the log
    with the rows _apply_schedule_rows applied.
    constraints=True: did the run stay feasible (MpcRollout.con, .con_worst, .con_first)?  fused=True reads the device's constraint log
    (Batch.mpc_set_con_log, switched on for the call); fused=False evaluates the definition in numpy the same way."""
    b = prob.batch
    if not isinstance(constraints, (bool, np.bool_)):
        raise ValueError(f"mpc_rollout: constraints must be a bool, got {constraints!r}")
    if steps is None:
        steps = prob.opts.mpc_horizon
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"mpc_rollout: steps must be >= 1, got {steps}")
    sched = _mpc_schedule(b, schedule)
    w = None
    if disturbance is not None:
        w = np.ascontiguousarray(np.asarray(disturbance, dtype=np.float64))
        if w.ndim != 3 or w.shape[0] < 1 or w.shape[1:] != (b.B, b.n):
            raise ValueError(f"disturbance: expected shape (rows >= 1, {b.B}, {b.n}), got {w.shape}")
        if not np.all(np.isfinite(w)):
            raise ValueError(f"disturbance: every entry must be finite (row {int(np.argwhere(~np.isfinite(w))[0][0])})")
    with _with_plant(b, plant) as pl:
        b.mpc_totals(reset=True)
        prob._sync_options()
        if fused:
            up = sched + ([(ALG_SCHED_DISTURBANCE, w)] if w is not None else [])
            done = []
            log0 = b.mpc_get_cost_log() if costs else None
            klog0 = b.mpc_get_con_log() if constraints else None
            stage_cost = cost = None
            con = (None, None, None)
            try:
                if costs:
                    b.mpc_set_cost_log(True)
                if constraints:
                    b.mpc_set_con_log(True)
                for k, a in up:
                    b.mpc_set_schedule(k, a)
                    done.append(k)
                states, controls, stats = b.mpc_solve_log(steps, prob.game_id0)
                it, cv = b.mpc_totals()
                if costs:
                    stage_cost, cost = b.mpc_get_cost()             # before the schedules go: dropping one invalidates the log
                if constraints:
                    con = b.mpc_get_con()
            finally:
                for k in done:
                    b.mpc_set_schedule(k, None)
                if costs and not log0:
                    b.mpc_set_cost_log(False)
                if constraints and not klog0:
                    b.mpc_set_con_log(False)
            return MpcRollout(states, controls, stats, it, cv, stage_cost, cost, *con)
        shift0, reset0 = prob.opts.shift, prob.opts.dual_reset
        n, m = b.n, b.m
        states, controls, stats, stage_cost, con = [b.get_x0()], [], [], [], []
        tab = _con_tables(prob) if constraints else None
        stepwise_plant = plant is not None or not pl.is_default
        try:
            for t in range(steps):
                if t == 1:
                    prob.opts.shift, prob.opts.dual_reset = pl.hold, False
                    prob._sync_options()
                _apply_schedule_rows(prob, sched, t)
                b.newton_solve_async(init=True, game_id0=prob.game_id0 + t * 1000003)
                stats.append(b.get_stats())
                z = b.get_traj()
                nums = _cost_numbers(prob, sched, t) if costs else None
                if constraints:                                     # the problem's numbers, row min(t, rows - 1) of a scheduled kind in their place
                    knums = dict(tab["nums"])
                    knums.update({k: a[min(t, a.shape[0] - 1)] for k, a in sched if k in knums})
                for j in range(pl.hold):
                    q = t * pl.hold + j
                    controls.append(z[:, 2 * n + j * b.b:2 * n + j * b.b + m].copy())
                    if costs:
                        stage_cost.append(prob.dt * _stage_cost(b, states[-1], controls[-1], *nums))
                    if stepwise_plant:
                        b.mpc_plant_advance(j)
                    else:
                        b.mpc_advance()
                    x1 = b.get_x0()
                    if w is not None:
                        x1 = x1 + w[min(q, w.shape[0] - 1)]
                        b.set_x0(x1)
                    states.append(x1)
                    if constraints:
                        con.append(_con_knot(b, tab, knums, x1, controls[-1]))
            it, cv = b.mpc_totals()
        finally:
            prob.opts.shift, prob.opts.dual_reset = shift0, reset0
            prob._sync_options()
        ro = MpcRollout(np.stack(states), np.stack(controls), np.stack(stats), it, cv)
        if costs:
            ro.stage_cost = np.stack(stage_cost)
            ro.cost = ro.stage_cost.sum(axis=0)
        if constraints:
            ro.con = np.stack([v for v, _ in con])
            ro.con_worst, ro.con_first = _con_summary(ro.con, con[0][1])
        return ro
