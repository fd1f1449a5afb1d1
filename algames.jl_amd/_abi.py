"""ctypes mirror of include/algames_hip.h.

`CLib(path, prefix)` binds every entry point the header declares.  The product binds
libalgames_hip.so with prefix ``alg_``; the CPU oracle (oracle/, test infrastructure) exports the
same signatures with prefix ``orc_`` and is bound by oracle/oracle.py through this same class.
"""
import ctypes as C
import dataclasses
import numpy as np

ALG_OK = 0
ALG_MODEL_DOUBLE_INTEGRATOR = 0
ALG_MODEL_UNICYCLE = 1
ALG_MODEL_BICYCLE = 2
ALG_MODEL_QUADROTOR = 3
ALG_TRAJ_PD, ALG_TRAJ_TRIAL, ALG_TRAJ_DELTA = 0, 1, 2
ALG_STATUS_OK, ALG_STATUS_SINGULAR, ALG_STATUS_NAN = 0, 1, 2
ALG_ERR_ARG, ALG_ERR_DEVICE, ALG_ERR_STATE = -1, -2, -3
# kinds of per-game scenario data (alg_set_scenario_data)
(ALG_SCEN_COLLISION_RADIUS, ALG_SCEN_COLLISION_COST, ALG_SCEN_CONTROL_BOUND, ALG_SCEN_STATE_BOUND,
 ALG_SCEN_WALL, ALG_SCEN_CIRCLE, ALG_SCEN_WALL3D, ALG_SCEN_CYLINDER) = range(8)
# which kernels per-game data of the base kinds runs on (alg_set_scenario_kernels)
ALG_SCEN_KERNELS_EXT, ALG_SCEN_KERNELS_BASE = 0, 1
SCEN_KERNELS = ("ext", "base")
ALG_SCHED_LQR_TARGET = 100      # alg_mpc_set_schedule: xf (p, ni) | uf (p, mi) per MPC step and game
ALG_SCHED_DISTURBANCE = 101     # alg_mpc_set_schedule: w (n) per MPC step and game, added to the advanced state
ALG_PLANT_RK2, ALG_PLANT_RK4 = 0, 1    # alg_mpc_set_plant: the plant's integrator
PLANT_INTEGRATORS = ("rk2", "rk4")
ALG_KKT_RHS_USER, ALG_KKT_RHS_X0, ALG_KKT_RHS_XF = 0, 1, 2    # alg_kkt_solve: the right-hand sides' kind
# alg_kkt_sensitivity: the parameter vector theta of X = -J^-1 d res / d theta
(ALG_PARAM_X0, ALG_PARAM_XF, ALG_PARAM_Q, ALG_PARAM_R, ALG_PARAM_UF, ALG_PARAM_COLLISION_COST, ALG_PARAM_COLLISION_RADIUS,
 ALG_PARAM_CONTROL_BOUND) = range(8)
PARAM_KINDS = ("x0", "xf", "Q", "R", "uf", "collision_cost", "collision_radius", "control_bound")
ALG_NORMAL_MAX_COLS = 63    # alg_kkt_normal_equations: columns of one call
SCEN_KINDS = ("collision_radius", "collision_cost", "control_bound", "state_bound", "wall", "circle", "wall3d", "cylinder")
# kinds of constraint rows, in the order of the knot layout (alg_get_con_values, alg_mpc_get_con: the columns of worst / first)
(ALG_CON_COLLISION, ALG_CON_CONTROL, ALG_CON_STATE, ALG_CON_WALL, ALG_CON_CIRCLE, ALG_CON_WALL3D, ALG_CON_CYLINDER) = range(7)
ALG_CON_KINDS = 7
CON_KINDS = ("collision", "control", "state", "wall", "circle", "wall3d", "cylinder")


class alg_desc(C.Structure):
    _fields_ = [("model", C.c_int32), ("p", C.c_int32), ("d", C.c_int32), ("N", C.c_int32),
                ("dt", C.c_double), ("batch", C.c_int32), ("device", C.c_int32)]


class alg_options(C.Structure):
    _fields_ = [("amplitude_init", C.c_double), ("shift", C.c_int32), ("regularize", C.c_int32),
                ("reg_0", C.c_double), ("alpha_decrease", C.c_double), ("beta", C.c_double),
                ("ls_iter", C.c_int32), ("dual_reset", C.c_int32), ("delta_min", C.c_double),
                ("rho_0", C.c_double), ("rho_increase", C.c_double), ("rho_max", C.c_double),
                ("lambda_max", C.c_double), ("alpha_dual", C.c_double),
                ("alphax_dual", C.c_double * 10),
                ("eps_dyn", C.c_double), ("eps_sta", C.c_double), ("eps_con", C.c_double),
                ("eps_opt", C.c_double), ("outer_iter", C.c_int32), ("inner_iter", C.c_int32),
                ("seed", C.c_int64)]


class alg_mpc_plant(C.Structure):
    _fields_ = [("hold", C.c_int32), ("substeps", C.c_int32), ("integrator", C.c_int32), ("reserved", C.c_int32)]


class alg_record(C.Structure):
    _fields_ = [("outer", C.c_int32), ("ls_j", C.c_int32), ("alpha", C.c_double),
                ("res", C.c_double), ("delta", C.c_double), ("dyn_vio", C.c_double),
                ("con_vio", C.c_double), ("sta_vio", C.c_double), ("opt_vio", C.c_double), ("t_elap", C.c_double)]


class alg_game_stats(C.Structure):
    _fields_ = [("status", C.c_int32), ("outer_iters", C.c_int32), ("newton_iters", C.c_int32),
                ("records", C.c_int32), ("converged", C.c_int32), ("ls_failures", C.c_int32),
                ("refinements", C.c_int32), ("reserved", C.c_int32), ("last", alg_record)]


class alg_step_info(C.Structure):
    _fields_ = [("status", C.c_int32), ("control_flow", C.c_int32), ("ls_j", C.c_int32),
                ("ls_failed", C.c_int32), ("alpha", C.c_double), ("delta", C.c_double),
                ("rec", alg_record)]


record_dtype = np.dtype([("outer", "<i4"), ("ls_j", "<i4"), ("alpha", "<f8"), ("res", "<f8"),
                         ("delta", "<f8"), ("dyn_vio", "<f8"), ("con_vio", "<f8"),
                         ("sta_vio", "<f8"), ("opt_vio", "<f8"), ("t_elap", "<f8")])
game_stats_dtype = np.dtype([("status", "<i4"), ("outer_iters", "<i4"), ("newton_iters", "<i4"),
                             ("records", "<i4"), ("converged", "<i4"), ("ls_failures", "<i4"),
                             ("refinements", "<i4"), ("reserved", "<i4"), ("last", record_dtype)])
step_info_dtype = np.dtype([("status", "<i4"), ("control_flow", "<i4"), ("ls_j", "<i4"),
                            ("ls_failed", "<i4"), ("alpha", "<f8"), ("delta", "<f8"),
                            ("rec", record_dtype)])
assert record_dtype.itemsize == C.sizeof(alg_record)
assert game_stats_dtype.itemsize == C.sizeof(alg_game_stats)
assert step_info_dtype.itemsize == C.sizeof(alg_step_info)

_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int32)

# name -> (restype, argtypes); exactly the functions declared in include/algames_hip.h
SIGNATURES = {
    "last_error": (C.c_char_p, []),
    "default_options": (None, [C.POINTER(alg_options)]),
    "dims": (C.c_int, [C.POINTER(alg_desc), _I, _I, _I, _I, _I, _I]),
    "create": (C.c_int, [C.POINTER(alg_desc), C.POINTER(_P)]),
    "destroy": (None, [_P]),
    "set_options": (C.c_int, [_P, C.POINTER(alg_options)]),
    "get_options": (C.c_int, [_P, C.POINTER(alg_options)]),
    "set_stream": (C.c_int, [_P, _P]),
    "set_waves_per_game": (C.c_int, [_P, C.c_int32]),
    "get_waves_per_game": (C.c_int, [_P, _I]),
    "set_refinement": (C.c_int, [_P, C.c_int32, C.c_double, C.c_double]),
    "get_refinement": (C.c_int, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "get_direction_gate": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "set_line_search_groups": (C.c_int, [_P, C.c_int32]),
    "get_line_search_groups": (C.c_int, [_P, _I]),
    "set_handoff": (C.c_int, [_P, C.c_int32]),
    "get_handoff": (C.c_int, [_P, _I, _I]),
    "set_x0": (C.c_int, [_P, _D]),
    "set_lqr": (C.c_int, [_P, _D, _D, _D, _D, C.c_int32]),
    "add_collision_cost": (C.c_int, [_P, _D, _D]),
    "add_collision_avoidance": (C.c_int, [_P, _D]),
    "add_collision_avoidance_pair": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_double]),
    "add_spherical_collision_avoidance_pair": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_double]),
    "add_control_bound": (C.c_int, [_P, _D, _D]),
    "set_bicycle": (C.c_int, [_P, C.c_double, C.c_double]),
    "set_quadrotor": (C.c_int, [_P, C.c_double]),
    "add_state_bound": (C.c_int, [_P, C.c_int32, _D, _D]),
    "add_wall_constraint": (C.c_int, [_P, C.c_int32, _D, _D, _D, _D, _D, _D]),
    "add_circle_constraint": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "add_wall_constraint_player": (C.c_int, [_P, C.c_int32, C.c_int32, _D, _D, _D, _D, _D, _D]),
    "add_circle_constraint_player": (C.c_int, [_P, C.c_int32, C.c_int32, _D, _D, _D]),
    "add_spherical_collision_avoidance": (C.c_int, [_P, _D]),
    "add_wall3d_constraint": (C.c_int, [_P, C.c_int32, _D, _D, _D, _D]),
    "add_cylinder_constraint": (C.c_int, [_P, C.c_int32, _D, _I, _D, _D]),
    "add_wall3d_constraint_player": (C.c_int, [_P, C.c_int32, C.c_int32, _D, _D, _D, _D]),
    "add_cylinder_constraint_player": (C.c_int, [_P, C.c_int32, C.c_int32, _D, _I, _D, _D]),
    "get_con_len": (C.c_int, [_P, _I]),
    "set_traj": (C.c_int, [_P, C.c_int32, _D]),
    "get_traj": (C.c_int, [_P, C.c_int32, _D]),
    "set_con_duals": (C.c_int, [_P, _D, _D]),
    "get_con_duals": (C.c_int, [_P, _D, _D]),
    "init_traj": (C.c_int, [_P, C.c_int64, C.c_int32]),
    "rollout": (C.c_int, [_P, C.c_int32]),
    "residual": (C.c_int, [_P, C.c_int32, C.c_double, _D, _D]),
    "residual_jacobian": (C.c_int, [_P, C.c_double, _D]),
    "residual_jacobian_games": (C.c_int, [_P, C.c_double, C.c_int32, C.c_int32, _D]),
    "release_scratch": (C.c_int, [_P]),
    "get_violation_profile": (C.c_int, [_P, _D, _D, _D, _D]),
    "newton_direction": (C.c_int, [_P, C.c_double, _D, _I]),
    "kkt_solve": (C.c_int, [_P, C.c_double, C.c_int32, C.c_int32, _D, C.c_int32, C.c_int32, _D, _I]),
    "param_len": (C.c_int, [_P, C.c_int32, _I]),
    "kkt_sensitivity": (C.c_int, [_P, C.c_double, C.c_int32, C.c_int32, _D, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _D, _I]),
    "kkt_normal_equations": (C.c_int, [_P, C.c_double, C.c_int32, _I, _I, _D, _D, C.c_int32, C.c_int32, C.c_int32, _D, _D, _D, _I]),
    "line_search": (C.c_int, [_P, C.c_double, _D, _D, _I]),
    "update_traj": (C.c_int, [_P, C.c_int32, C.c_int32, _D]),
    "record_stats": (C.c_int, [_P, _P]),
    "reset_con": (C.c_int, [_P]),
    "dual_penalty_update": (C.c_int, [_P, _D]),
    "newton_step": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    "newton_solve": (C.c_int, [_P, C.c_int32, C.c_int64, _P]),
    "newton_solve_async": (C.c_int, [_P, C.c_int32, C.c_int64]),
    "get_stats": (C.c_int, [_P, _P]),
    "get_history": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _I]),
    "set_history_profiles": (C.c_int, [_P, C.c_int32]),
    "get_history_profiles": (C.c_int, [_P, _I]),
    "get_history_vio": (C.c_int, [_P, C.c_int32, C.c_int32, _D, _D, _D, _D, _I]),
    "synchronize": (C.c_int, [_P]),
    "debug_check_guards": (C.c_int, [_P]),
    "ibr_solve_player": (C.c_int, [_P, C.c_int32, _P]),
    "ibr_newton_solve": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, _I, C.c_double, _P]),
    "mpc_advance": (C.c_int, [_P]),
    "mpc_totals": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "mpc_solve": (C.c_int, [_P, C.c_int32, C.c_int64, _D]),
    "scenario_data_len": (C.c_int, [_P, C.c_int32, _I]),
    "set_scenario_data": (C.c_int, [_P, C.c_int32, _D]),
    "get_scenario_data": (C.c_int, [_P, C.c_int32, _D]),
    "set_scenario_kernels": (C.c_int, [_P, C.c_int32]),
    "get_scenario_kernels": (C.c_int, [_P, _I, _I]),
    "mpc_set_schedule": (C.c_int, [_P, C.c_int32, C.c_int32, _D]),
    "mpc_get_schedule": (C.c_int, [_P, C.c_int32, _I]),
    "mpc_solve_log": (C.c_int, [_P, C.c_int32, C.c_int64, _D, _D, _P]),
    "mpc_set_plant": (C.c_int, [_P, C.POINTER(alg_mpc_plant)]),
    "mpc_get_plant": (C.c_int, [_P, C.POINTER(alg_mpc_plant)]),
    "mpc_plant_advance": (C.c_int, [_P, C.c_int32]),
    "get_cost": (C.c_int, [_P, C.c_int32, _D, _D]),
    "mpc_set_cost_log": (C.c_int, [_P, C.c_int32]),
    "mpc_get_cost_log": (C.c_int, [_P, _I]),
    "mpc_get_cost": (C.c_int, [_P, C.c_int32, _D, _D, _I]),
    "get_con_values": (C.c_int, [_P, C.c_int32, _D]),
    "con_knot_len": (C.c_int, [_P, _I]),
    "mpc_set_con_log": (C.c_int, [_P, C.c_int32]),
    "mpc_get_con_log": (C.c_int, [_P, _I]),
    "mpc_get_con": (C.c_int, [_P, C.c_int32, _D, _D, _I, _I]),
}
# Entry points a backend may lack (the CPU oracle has no per-game scenario data): bound when present; calling one that is absent
# raises AlgamesError naming the backend.
OPTIONAL = frozenset({"scenario_data_len", "set_scenario_data", "get_scenario_data", "set_scenario_kernels", "get_scenario_kernels",
                      "mpc_set_schedule", "mpc_get_schedule", "mpc_solve_log", "mpc_set_plant", "mpc_get_plant", "mpc_plant_advance", "kkt_solve",
                      "param_len", "kkt_sensitivity", "kkt_normal_equations",
                      "set_history_profiles", "get_history_profiles", "get_history_vio",
                      "get_cost", "mpc_set_cost_log", "mpc_get_cost_log", "mpc_get_cost",
                      "get_con_values", "con_knot_len", "mpc_set_con_log", "mpc_get_con_log", "mpc_get_con"})


class AlgamesError(RuntimeError):
    pass


@dataclasses.dataclass(frozen=True)
class Plant:
    """The plant of the receding-horizon loop (alg_mpc_set_plant): every solve is followed by `hold` plant knots; knot j holds u_{1+j} of the
    plan and integrates the state over dt in `substeps` sub-steps with `integrator` -- "rk2", the model's own discrete step, or "rk4", the
    classical method on the model's continuous dynamics.  Plant() is the loop without a plant: one RK2 step of length dt per solve."""
    hold: int = 1
    substeps: int = 1
    integrator: str = "rk2"

    def __post_init__(self):
        if isinstance(self.integrator, (int, np.integer)) and not isinstance(self.integrator, bool) and 0 <= int(self.integrator) < len(PLANT_INTEGRATORS):
            object.__setattr__(self, "integrator", PLANT_INTEGRATORS[int(self.integrator)])
        if self.integrator not in PLANT_INTEGRATORS:
            raise ValueError(f"Plant: integrator must be one of {PLANT_INTEGRATORS}, got {self.integrator!r}")
        for name, hi in (("hold", None), ("substeps", 256)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or (hi is not None and v > hi):
                raise ValueError(f"Plant: {name} must be an integer in 1 ... {hi if hi is not None else 'N - 1'}, got {v!r}")
            object.__setattr__(self, name, int(v))

    @classmethod
    def from_options(cls, opts):
        """The plant the reference's Options ask for: substeps = opts.upsampling, one knot per solve, the model's own step."""
        return cls(substeps=int(opts.upsampling))

    @property
    def is_default(self):
        return self == Plant()


def _dptr(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_D)


def _iptr(a):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_I)


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


class CLib:
    """A loaded shared library exporting the ABI of include/algames_hip.h under `prefix`."""

    def __init__(self, path, prefix):
        self.path, self.prefix = path, prefix
        self.dll = C.CDLL(path)
        self.missing = []
        self.absent = []        # optional entry points this backend does not export
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(self.dll, prefix + name)
            except AttributeError:
                if name in OPTIONAL:
                    self.absent.append(name)
                    setattr(self, name, self._absent_fn(name))
                else:
                    self.missing.append(prefix + name)
                continue
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)
        if self.missing:
            raise AlgamesError(f"{path}: missing ABI symbols {self.missing}")

    def _absent_fn(self, name):
        def absent(*args):
            raise AlgamesError(f"{self.path}: this backend has no {self.prefix}{name} (per-game scenario data is not supported by it)")
        return absent

    def check(self, rc):
        if rc != ALG_OK:
            msg = self.last_error()
            raise AlgamesError((msg or b"").decode() + f" (code {rc})")

    def default_opts(self):
        o = alg_options()
        self.default_options(C.byref(o))
        return o

    def sizes(self, desc):
        v = [C.c_int32() for _ in range(6)]
        self.check(self.dims(C.byref(desc), *[C.byref(x) for x in v]))
        n, m, mi, S, traj_len, con_len = [x.value for x in v]
        return dict(n=n, m=m, mi=mi, S=S, traj_len=traj_len, con_len=con_len)


class Batch:
    """Thin object wrapper over one alg_handle: a batch of B games sharing structure.

    This is the level the Julia shim binds; the reference-shaped host API
    (GameProblem, newton_solve, ...) in algames_jl_amd/__init__.py is built on it.
    """

    def __init__(self, lib, model, p, N, dt, batch, d=2, device=0):
        self.lib = lib
        self.desc = alg_desc(model, p, d, N, dt, batch, device)
        sz = lib.sizes(self.desc)
        self.n, self.m, self.mi, self.S = sz["n"], sz["m"], sz["mi"], sz["S"]
        self.traj_len, self.con_len = sz["traj_len"], sz["con_len"]
        self.ni = self.n // p
        self.p, self.N, self.dt, self.B, self.d = p, N, dt, batch, d
        self.b = self.n + self.m + p * self.n
        h = _P()
        lib.check(lib.create(C.byref(self.desc), C.byref(h)))
        self.h = h
        self.opts = lib.default_opts()

    def close(self):
        if getattr(self, "h", None):
            self.lib.destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup -------------------------------------------------------------------------------
    def set_options(self, **kw):
        for k, v in kw.items():
            if k == "alphax_dual":
                for i, x in enumerate(v):
                    self.opts.alphax_dual[i] = x
            else:
                if not hasattr(self.opts, k):
                    raise AttributeError(k)
                setattr(self.opts, k, v)
        self.lib.check(self.lib.set_options(self.h, C.byref(self.opts)))

    def set_waves_per_game(self, nw):
        """0 = automatic, 1 = one game per wavefront, 2 / 4 = a team of wavefronts per game (fused solver kernels)."""
        self.lib.check(self.lib.set_waves_per_game(self.h, int(nw)))

    def get_waves_per_game(self):
        v = C.c_int32()
        self.lib.check(self.lib.get_waves_per_game(self.h, C.byref(v)))
        return v.value

    def set_refinement(self, max_steps=None, tol=None, mu_tight=None):
        """Iterative refinement of the Newton direction (alg_set_refinement): the opt-u rows of every direction are evaluated and the
        direction is corrected (at most `max_steps` correction solves) while their row-wise backward error exceeds `tol` (relaxed up to
        256 x while the game's largest penalty is below `mu_tight`); max_steps = 0 switches gate and refinement off.  None keeps a value."""
        ms0, tol0, mu0 = self.get_refinement()
        self.lib.check(self.lib.set_refinement(self.h, int(ms0 if max_steps is None else max_steps), float(tol0 if tol is None else tol),
                                               float(mu0 if mu_tight is None else mu_tight)))

    def get_refinement(self):
        ms = C.c_int32(); tol = C.c_double(); mu = C.c_double()
        self.lib.check(self.lib.get_refinement(self.h, C.byref(ms), C.byref(tol), C.byref(mu)))
        return ms.value, tol.value, mu.value

    def set_line_search_groups(self, on):
        """Line search of the team / one-wavefront unicycle kernels: step sizes tried four at a time once the first one was rejected (True,
        default) or one after another (False); bit-identical norms either way (alg_set_line_search_groups)."""
        self.lib.check(self.lib.set_line_search_groups(self.h, 1 if on else 0))

    def get_line_search_groups(self):
        v = C.c_int32()
        self.lib.check(self.lib.get_line_search_groups(self.h, C.byref(v)))
        return bool(v.value)

    def set_handoff(self, iters):
        """Straggler hand-off for heterogeneous batches (alg_set_handoff): games that need more than `iters` inner iterations in the
        one-wavefront kernel park and a second launch finishes them with the team kernel; 0 = off (default)."""
        self.lib.check(self.lib.set_handoff(self.h, int(iters)))

    def get_handoff(self):
        """(budget, number of games the most recent solve handed over)"""
        k = C.c_int32(); n = C.c_int32()
        self.lib.check(self.lib.get_handoff(self.h, C.byref(k), C.byref(n)))
        return k.value, n.value

    def get_direction_gate(self):
        """(B, 3): [max |rho|, row-wise backward error omega, largest row scale] of the opt-u rows of the last Newton direction
        (alg_get_direction_gate)."""
        out = np.zeros((self.B, 3))
        self.lib.check(self.lib.get_direction_gate(self.h, _dptr(out)))
        return out

    def set_stream(self, stream_ptr):
        self.lib.check(self.lib.set_stream(self.h, _P(stream_ptr)))

    def set_x0(self, x0):
        x0 = _f64(x0)
        if x0.ndim == 1:
            x0 = np.ascontiguousarray(np.broadcast_to(x0, (self.B, self.n)))
        x0 = _f64(x0, (self.B, self.n))
        self.lib.check(self.lib.set_x0(self.h, _dptr(x0)))

    def set_lqr(self, Qdiag, Rdiag, xf, uf):
        Qdiag, Rdiag, xf, uf = _f64(Qdiag), _f64(Rdiag), _f64(xf), _f64(uf)
        per_game = int(Qdiag.ndim == 3)
        lead = (self.B,) if per_game else ()
        Qdiag = _f64(Qdiag, lead + (self.p, self.ni)); xf = _f64(np.broadcast_to(xf, lead + (self.p, self.ni)))
        Rdiag = _f64(Rdiag, lead + (self.p, self.mi)); uf = _f64(np.broadcast_to(uf, lead + (self.p, self.mi)))
        self.lib.check(self.lib.set_lqr(self.h, _dptr(Qdiag), _dptr(Rdiag), _dptr(xf), _dptr(uf), per_game))

    def add_collision_cost(self, radius, mu):
        self.lib.check(self.lib.add_collision_cost(self.h, _dptr(_f64(radius, (self.p,))), _dptr(_f64(mu, (self.p,)))))

    def add_collision_avoidance(self, radius):
        r = _f64(np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.p,)))
        self.lib.check(self.lib.add_collision_avoidance(self.h, _dptr(r)))

    def add_control_bound(self, u_max, u_min):
        self.lib.check(self.lib.add_control_bound(self.h, _dptr(_f64(u_max, (self.m,))), _dptr(_f64(u_min, (self.m,)))))

    def _refresh_con_len(self):
        v = C.c_int32()
        self.lib.check(self.lib.get_con_len(self.h, C.byref(v)))
        self.con_len = v.value

    def set_bicycle(self, lf, lr):
        self.lib.check(self.lib.set_bicycle(self.h, float(lf), float(lr)))

    def set_quadrotor(self, mass):
        self.lib.check(self.lib.set_quadrotor(self.h, float(mass)))

    def add_state_bound(self, player, x_max, x_min):
        self.lib.check(self.lib.add_state_bound(self.h, int(player), _dptr(_f64(x_max, (self.n,))), _dptr(_f64(x_min, (self.n,)))))
        self._refresh_con_len()

    def add_wall_constraint(self, x1, y1, x2, y2, xv, yv):
        arrs = [_f64(a) for a in (x1, y1, x2, y2, xv, yv)]
        self.lib.check(self.lib.add_wall_constraint(self.h, len(arrs[0]), *[_dptr(a) for a in arrs]))
        self._refresh_con_len()

    def add_circle_constraint(self, xc, yc, radius):
        arrs = [_f64(a) for a in (xc, yc, radius)]
        self.lib.check(self.lib.add_circle_constraint(self.h, len(arrs[0]), *[_dptr(a) for a in arrs]))
        self._refresh_con_len()

    def add_wall_constraint_player(self, player, x1, y1, x2, y2, xv, yv):
        arrs = [_f64(a) for a in (x1, y1, x2, y2, xv, yv)]
        self.lib.check(self.lib.add_wall_constraint_player(self.h, int(player), len(arrs[0]), *[_dptr(a) for a in arrs]))
        self._refresh_con_len()

    def add_circle_constraint_player(self, player, xc, yc, radius):
        arrs = [_f64(a) for a in (xc, yc, radius)]
        self.lib.check(self.lib.add_circle_constraint_player(self.h, int(player), len(arrs[0]), *[_dptr(a) for a in arrs]))
        self._refresh_con_len()

    def add_collision_avoidance_pair(self, i, j, radius, spherical=False):
        """One ordered pair (0-based players), own radius: add_collision_avoidance!(game_con, i, j, radius)."""
        fn = self.lib.add_spherical_collision_avoidance_pair if spherical else self.lib.add_collision_avoidance_pair
        self.lib.check(fn(self.h, int(i), int(j), float(radius)))
        if spherical:
            self._refresh_con_len()

    def add_spherical_collision_avoidance(self, radius):
        r = _f64(np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.p,)))
        self.lib.check(self.lib.add_spherical_collision_avoidance(self.h, _dptr(r)))

    def add_wall3d_constraint(self, p1, p2, p3, v):
        arrs = [_f64(np.asarray(a, dtype=np.float64).reshape(-1, 3)) for a in (p1, p2, p3, v)]
        self.lib.check(self.lib.add_wall3d_constraint(self.h, len(arrs[0]), *[_dptr(a) for a in arrs]))
        self._refresh_con_len()

    def add_cylinder_constraint(self, p, axis, l, r):
        p = _f64(np.asarray(p, dtype=np.float64).reshape(-1, 3))
        ax = np.ascontiguousarray(axis, dtype=np.int32)
        self.lib.check(self.lib.add_cylinder_constraint(self.h, len(p), _dptr(p), ax.ctypes.data_as(_I), _dptr(_f64(l, (len(p),))), _dptr(_f64(r, (len(p),)))))
        self._refresh_con_len()

    def add_wall3d_constraint_player(self, player, p1, p2, p3, v):
        """add_wall_constraint!(game_con, i, walls::Vector{Wall3D}): player i (0-based) only."""
        arrs = [_f64(np.asarray(a, dtype=np.float64).reshape(-1, 3)) for a in (p1, p2, p3, v)]
        self.lib.check(self.lib.add_wall3d_constraint_player(self.h, int(player), len(arrs[0]), *[_dptr(a) for a in arrs]))
        self._refresh_con_len()

    def add_cylinder_constraint_player(self, player, p, axis, l, r):
        """add_wall_constraint!(game_con, i, walls::Vector{CylinderWall}): player i (0-based) only."""
        p = _f64(np.asarray(p, dtype=np.float64).reshape(-1, 3))
        ax = np.ascontiguousarray(axis, dtype=np.int32)
        self.lib.check(self.lib.add_cylinder_constraint_player(self.h, int(player), len(p), _dptr(p), ax.ctypes.data_as(_I), _dptr(_f64(l, (len(p),))), _dptr(_f64(r, (len(p),)))))
        self._refresh_con_len()

    # ---- per-game scenario data ----------------------------------------------------------------
    @staticmethod
    def _kind(kind):
        if isinstance(kind, str):
            if kind not in SCEN_KINDS:
                raise ValueError(f"unknown scenario kind {kind!r}; one of {SCEN_KINDS}")
            return SCEN_KINDS.index(kind)
        k = int(kind)
        if not 0 <= k < len(SCEN_KINDS):
            raise ValueError(f"unknown scenario kind {kind!r}")
        return k

    def scenario_data_len(self, kind):
        """Doubles per game of `kind` (an ALG_SCEN_* value or its name in SCEN_KINDS); 0 if that kind was not added."""
        v = C.c_int32()
        self.lib.check(self.lib.scenario_data_len(self.h, self._kind(kind), C.byref(v)))
        return v.value

    def set_scenario_data(self, kind, data):
        """Per-game values of one kind (B x scenario_data_len(kind)); None = back to the handle's shared values.  See
        alg_set_scenario_data for what is checked and when the multipliers are re-created."""
        k = self._kind(kind)
        if data is None:
            self.lib.check(self.lib.set_scenario_data(self.h, k, None))
            return
        L = self.scenario_data_len(k)
        a = np.ascontiguousarray(np.asarray(data, dtype=np.float64))
        if a.shape != (self.B, L):
            raise ValueError(f"scenario data of kind {SCEN_KINDS[k]!r}: expected shape {(self.B, L)}, got {a.shape}")
        self.lib.check(self.lib.set_scenario_data(self.h, k, _dptr(a)))
        self._refresh_con_len()

    def get_scenario_data(self, kind):
        k = self._kind(kind)
        L = self.scenario_data_len(k)
        out = np.empty((self.B, L))
        self.lib.check(self.lib.get_scenario_data(self.h, k, _dptr(out)))
        return out

    def set_scenario_kernels(self, which):
        """Which kernels per-game data of the base kinds (pair radii, collision cost, control bounds) runs on: "ext" / ALG_SCEN_KERNELS_EXT
        (default: the first set_scenario_data switches the handle to the EXT kernels and re-creates the multipliers) or "base" /
        ALG_SCEN_KERNELS_BASE (a handle with the base constraint set keeps the base kernels -- fused pass, teams, hand-off -- and its
        multipliers).  Only while the handle carries no per-game data; see alg_set_scenario_kernels."""
        if isinstance(which, str):
            if which not in SCEN_KERNELS:
                raise ValueError(f"scenario_kernels: one of {SCEN_KERNELS}, got {which!r}")
            which = SCEN_KERNELS.index(which)
        self.lib.check(self.lib.set_scenario_kernels(self.h, int(which)))

    def get_scenario_kernels(self):
        """(setting, in_use): the ALG_SCEN_KERNELS_* value and the kernels the next launch takes -- 0 base, 1 EXT, 2 base kernels
        reading per-game blocks."""
        w, u = C.c_int32(), C.c_int32()
        self.lib.check(self.lib.get_scenario_kernels(self.h, C.byref(w), C.byref(u)))
        return w.value, u.value

    # ---- data movement -----------------------------------------------------------------------
    def set_traj(self, z, which=ALG_TRAJ_PD):
        z = _f64(z, (self.B, self.traj_len))
        self.lib.check(self.lib.set_traj(self.h, which, _dptr(z)))

    def get_traj(self, which=ALG_TRAJ_PD):
        z = np.empty((self.B, self.traj_len))
        self.lib.check(self.lib.get_traj(self.h, which, _dptr(z)))
        return z

    def set_con_duals(self, lam=None, mu=None):
        lam = None if lam is None else _f64(lam, (self.B, self.con_len))
        mu = None if mu is None else _f64(mu, (self.B, self.con_len))
        self.lib.check(self.lib.set_con_duals(self.h, _dptr(lam), _dptr(mu)))

    def get_con_duals(self):
        lam = np.empty((self.B, self.con_len)); mu = np.empty((self.B, self.con_len))
        self.lib.check(self.lib.get_con_duals(self.h, _dptr(lam), _dptr(mu)))
        return lam, mu

    # ---- the path ----------------------------------------------------------------------------
    def init_traj(self, game_id0=0, use_shift=False):
        self.lib.check(self.lib.init_traj(self.h, game_id0, int(use_shift)))

    def rollout(self, which=ALG_TRAJ_PD):
        self.lib.check(self.lib.rollout(self.h, which))

    def residual(self, which=ALG_TRAJ_PD, reg=0.0, want_res=True):
        res = np.empty((self.B, self.S)) if want_res else None
        rn = np.empty(self.B)
        self.lib.check(self.lib.residual(self.h, which, reg, _dptr(res), _dptr(rn)))
        return res, rn

    def residual_jacobian(self, reg=0.0, games=None):
        """Dense KKT Jacobians [g, row, col]; games = (first, count) restricts the work and the memory to that range."""
        first, cnt = (0, self.B) if games is None else (int(games[0]), int(games[1]))
        jac = np.empty((cnt, self.S, self.S))
        self.lib.check(self.lib.residual_jacobian_games(self.h, reg, first, cnt, _dptr(jac)))
        return jac.transpose(0, 2, 1)     # column-major S x S per game -> [g, row, col]

    def release_scratch(self):
        self.lib.check(self.lib.release_scratch(self.h))

    def violation_profile(self):
        """Per-knot .vio vectors at pdtraj: dict(dyn (B, N-1), con (B, N-1), sta (B, N), opt (B, N))."""
        out = dict(dyn=np.empty((self.B, self.N - 1)), con=np.empty((self.B, self.N - 1)), sta=np.empty((self.B, self.N)), opt=np.empty((self.B, self.N)))
        self.lib.check(self.lib.get_violation_profile(self.h, _dptr(out["dyn"]), _dptr(out["con"]), _dptr(out["sta"]), _dptr(out["opt"])))
        return out

    def get_cost(self, which=ALG_TRAJ_PD, stage=False):
        """What the plan costs each player (alg_get_cost): total (B, p, 3) with the components [state, control, collision] of
        J_i = sum_k w_k l_i(x_k, u_k), w_k = dt for k < N and w_N = 1 -- the objective, without constraints, multipliers or penalties.
        which: ALG_TRAJ_PD or ALG_TRAJ_TRIAL.  stage=True returns (total, stage (B, N, p, 3)), the summands w_k l_i per knot.
        Changes nothing on the handle; a backend without the entry point (the CPU oracle) raises AlgamesError."""
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or int(which) not in (ALG_TRAJ_PD, ALG_TRAJ_TRIAL):
            raise ValueError(f"get_cost: which must be ALG_TRAJ_PD (0) or ALG_TRAJ_TRIAL (1), got {which!r}")
        total = np.empty((self.B, self.p, 3))
        st = np.empty((self.B, self.N, self.p, 3)) if stage else None
        self.lib.check(self.lib.get_cost(self.h, int(which), _dptr(total), _dptr(st)))
        return (total, st) if stage else total

    def get_con_values(self, which=ALG_TRAJ_PD):
        """The constraint values of the plan, read-only (alg_get_con_values): (B, con_len) in the ABI's constraint layout, the rows of
        dual_penalty_update's vals -- c <= 0 feasible, -inf for a row of an infinite bound, 0 for an inert row -- without its dual and
        penalty update.  which: ALG_TRAJ_PD or ALG_TRAJ_TRIAL.  Changes nothing on the handle; a backend without the entry point (the CPU
        oracle) raises AlgamesError."""
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or int(which) not in (ALG_TRAJ_PD, ALG_TRAJ_TRIAL):
            raise ValueError(f"get_con_values: which must be ALG_TRAJ_PD (0) or ALG_TRAJ_TRIAL (1), got {which!r}")
        vals = np.empty((self.B, self.con_len))
        self.lib.check(self.lib.get_con_values(self.h, int(which), _dptr(vals)))
        return vals

    def con_knot_len(self):
        """K1, the constraint rows of one step (alg_con_knot_len): con_len = (N - 1) K1"""
        v = C.c_int32()
        self.lib.check(self.lib.con_knot_len(self.h, C.byref(v)))
        return v.value

    def newton_direction(self, reg=0.0):
        delta = np.empty((self.B, self.S)); st = np.empty(self.B, dtype=np.int32)
        self.lib.check(self.lib.newton_direction(self.h, reg, _dptr(delta), _iptr(st)))
        return delta, st

    def kkt_solve(self, rhs=None, kind="user", reg=0.0, games=None):
        """J X = R at the current iterate (alg_kkt_solve): J is the residual Jacobian of residual_jacobian(reg) at pdtraj, solved on the device
        by the structured elimination of newton_direction (refinement gate included), one elimination per column.
        kind = "user": rhs[cnt, nrhs, S] (or [cnt, S]: one column) in the VERTICAL order of residual(); rhs = -res gives the Newton direction.
        kind = "x0":   R = -d res / d x_1, n columns: X = d z* / d x0.     kind = "xf": R = -d res / d x_f, p ni columns in the xf order of set_lqr.
        The derivative is that of the root of res(z; theta) = 0 with the multipliers and penalties held; exact for the double integrator, the
        Gauss-Newton sensitivity of the reference's Jacobian (no second-order dynamics terms) for the other models; reg != 0 solves the
        regularised system.  games = (first, count).  Returns (X[cnt, nrhs, S] in horizontal order, status[cnt])."""
        first, cnt = (0, self.B) if games is None else (int(games[0]), int(games[1]))
        code = {"user": ALG_KKT_RHS_USER, "x0": ALG_KKT_RHS_X0, "xf": ALG_KKT_RHS_XF}.get(kind, kind)
        if code not in (ALG_KKT_RHS_USER, ALG_KKT_RHS_X0, ALG_KKT_RHS_XF):
            raise ValueError(f"unknown right-hand-side kind {kind!r}: 'user', 'x0' or 'xf'")
        if code == ALG_KKT_RHS_USER:
            if rhs is None:
                raise ValueError("kind='user' needs rhs")
            r = np.asarray(rhs, dtype=np.float64)
            if r.ndim == 2:
                r = r[:, None, :]
            if r.ndim != 3 or r.shape[0] != cnt or r.shape[1] < 1 or r.shape[2] != self.S:
                raise ValueError(f"expected shape {(cnt, 'nrhs', self.S)}, got {tuple(np.shape(rhs))}")
            r = _f64(r, r.shape); nrhs = r.shape[1]
        else:
            if rhs is not None:
                raise ValueError("rhs is only taken with kind='user'")
            r = None; nrhs = self.n if code == ALG_KKT_RHS_X0 else self.p * self.ni
        X = np.empty((max(cnt, 0), nrhs, self.S)); st = np.empty(max(cnt, 0), dtype=np.int32)
        self.lib.check(self.lib.kkt_solve(self.h, float(reg), code, nrhs, _dptr(r), first, cnt, _dptr(X), _iptr(st)))
        return X, st

    @staticmethod
    def _param_code(param):
        code = PARAM_KINDS.index(param) if isinstance(param, str) and param in PARAM_KINDS else param
        if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or not 0 <= int(code) < len(PARAM_KINDS):
            raise ValueError(f"unknown parameter {param!r}: one of {PARAM_KINDS} or its ALG_PARAM_* code")
        return int(code)

    def param_len(self, param):
        """entries of the parameter vector `param` (a name of PARAM_KINDS or an ALG_PARAM_* code), in the order of its setter (alg_param_len)"""
        v = C.c_int32()
        self.lib.check(self.lib.param_len(self.h, self._param_code(param), C.byref(v)))
        return v.value

    def _param_len(self, code):
        """the same count from the problem sizes: what the argument checks use before any library call"""
        return (self.n, self.p * self.ni, self.p * self.ni, self.p * self.mi, self.p * self.mi, 2 * self.p, self.p * self.p, 2 * self.m)[code]

    def kkt_sensitivity(self, param, reg=0.0, games=None, steps=None, dirs=None):
        """X = -J^-1 d res / d theta at the current iterate with the right-hand sides built on the device (alg_kkt_sensitivity): theta = `param`
        (PARAM_KINDS: "x0", "xf", "Q", "R", "uf" in the orders of set_lqr, "collision_cost" / "collision_radius" / "control_bound" in the orders of
        set_scenario_data), multipliers, penalties and active sets held, J and reg as in kkt_solve.
        dirs = None: the param_len(param) unit columns.  dirs[cnt, ndir, len] (or [cnt, len]: one direction): column c is the directional
        derivative X dirs[g, c], one elimination each.  games = (first, count).  steps = (first, count), 0-based: only those steps' blocks
        of b = n + m + n p rows are stored and downloaded.  Returns (X[cnt, ncol, count * b] in horizontal order, status[cnt])."""
        code = self._param_code(param)
        ln = self._param_len(code)
        first, cnt = (0, self.B) if games is None else (int(games[0]), int(games[1]))
        if first < 0 or cnt < 1 or first + cnt > self.B:
            raise ValueError(f"games = (first, count) must lie inside the batch of {self.B}, got {games!r}")
        s0, ns = (0, self.N - 1) if steps is None else (int(steps[0]), int(steps[1]))
        if s0 < 0 or ns < 1 or s0 + ns > self.N - 1:
            raise ValueError(f"steps = (first, count) must lie inside 0 ... {self.N - 2}, got {steps!r}")
        if dirs is None:
            v = None; ndir = 0; ncol = ln
        else:
            v = np.asarray(dirs, dtype=np.float64)
            if v.ndim == 2:
                v = v[:, None, :]
            if v.ndim != 3 or v.shape[0] != cnt or v.shape[1] < 1 or v.shape[2] != ln:
                raise ValueError(f"expected shape {(cnt, 'ndir', ln)}, got {tuple(np.shape(dirs))}")
            if not np.isfinite(v).all():
                raise ValueError("dirs must be finite")
            v = _f64(v, v.shape); ndir = ncol = v.shape[1]
        X = np.empty((cnt, ncol, ns * self.b)); st = np.empty(cnt, dtype=np.int32)
        self.lib.check(self.lib.kkt_sensitivity(self.h, float(reg), code, ndir, _dptr(v), first, cnt, s0, ns, _dptr(X), _iptr(st)))
        return X, st

    def kkt_normal_equations(self, cols, target, weight, reg=0.0, games=None):
        """The normal equations of fitting parameters to an observed trajectory, reduced on the device (alg_kkt_normal_equations).  cols: up to
        ALG_NORMAL_MAX_COLS distinct (param, index) pairs, param a name of PARAM_KINDS or its code, index an entry of that parameter vector;
        column c is the unit column kkt_sensitivity returns for it.  target[cnt, S]: the observed z in horizontal order; weight[S] (shared) or
        weight[cnt, S]: finite and >= 0.  With r = z - target over the S entries of pdtraj behind x_1, per game: loss = 1/2 sum w r^2,
        g = X' W r, H = X' W X (both triangles, symmetric bit for bit).  games = (first, count).  Returns (H[cnt, q, q], g[cnt, q], loss[cnt],
        status[cnt]); no column is downloaded."""
        first, cnt = (0, self.B) if games is None else (int(games[0]), int(games[1]))
        if first < 0 or cnt < 1 or first + cnt > self.B:
            raise ValueError(f"games = (first, count) must lie inside the batch of {self.B}, got {games!r}")
        cols = list(cols)
        if not 1 <= len(cols) <= ALG_NORMAL_MAX_COLS:
            raise ValueError(f"cols must name 1 ... {ALG_NORMAL_MAX_COLS} columns, got {len(cols)}")
        cp = np.empty(len(cols), dtype=np.int32); ci = np.empty(len(cols), dtype=np.int32)
        seen = set()
        for c, col in enumerate(cols):
            try:
                if isinstance(col, str):
                    raise TypeError
                param, index = col
            except (TypeError, ValueError):
                raise ValueError(f"column {c}: expected a (param, index) pair, got {col!r}") from None
            code = self._param_code(param)
            if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or not 0 <= int(index) < self._param_len(code):
                raise ValueError(f"column {c}: index must be an integer in 0 ... {self._param_len(code) - 1} for {PARAM_KINDS[code]!r}, got {index!r}")
            if (code, int(index)) in seen:
                raise ValueError(f"column {c}: duplicate column ({PARAM_KINDS[code]!r}, {int(index)})")
            seen.add((code, int(index)))
            cp[c], ci[c] = code, int(index)
        t = np.asarray(target, dtype=np.float64)
        if t.shape != (cnt, self.S):
            raise ValueError(f"target: expected shape {(cnt, self.S)}, got {t.shape}")
        if not np.isfinite(t).all():
            raise ValueError("target must be finite")
        w = np.asarray(weight, dtype=np.float64)
        if w.shape not in ((self.S,), (cnt, self.S)):
            raise ValueError(f"weight: expected shape {(self.S,)} or {(cnt, self.S)}, got {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("weight must be finite and >= 0")
        t, w = _f64(t), _f64(w)
        q = len(cols)
        Hm = np.empty((cnt, q, q)); g = np.empty((cnt, q)); loss = np.empty(cnt); st = np.empty(cnt, dtype=np.int32)
        self.lib.check(self.lib.kkt_normal_equations(self.h, float(reg), q, _iptr(cp), _iptr(ci), _dptr(t), _dptr(w), int(w.ndim == 2), first, cnt,
                                                     _dptr(Hm), _dptr(g), _dptr(loss), _iptr(st)))
        return Hm, g, loss, st

    def line_search(self, res_norm, reg=0.0):
        rn = _f64(res_norm, (self.B,)); a = np.empty(self.B); j = np.empty(self.B, dtype=np.int32)
        self.lib.check(self.lib.line_search(self.h, reg, _dptr(rn), _dptr(a), _iptr(j)))
        return a, j

    def update_traj(self, alpha, target=ALG_TRAJ_PD, source=ALG_TRAJ_PD):
        a = _f64(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.B,)))
        self.lib.check(self.lib.update_traj(self.h, target, source, _dptr(a)))

    def record(self):
        rec = np.zeros(self.B, dtype=record_dtype)
        self.lib.check(self.lib.record_stats(self.h, rec.ctypes.data_as(_P)))
        return rec

    def reset_con(self):
        self.lib.check(self.lib.reset_con(self.h))

    def dual_penalty_update(self):
        vals = np.empty((self.B, self.con_len))
        self.lib.check(self.lib.dual_penalty_update(self.h, _dptr(vals)))
        return vals

    def newton_step(self, k_outer=1, l_inner=1, delta=None):
        """inner_iteration for every game; `delta` (B,) is the caller's Δ that record! stores (solver_methods.jl:75), default 0."""
        info = np.zeros(self.B, dtype=step_info_dtype)
        d = None if delta is None else _f64(np.broadcast_to(np.asarray(delta, dtype=np.float64), (self.B,)))
        self.lib.check(self.lib.newton_step(self.h, k_outer, l_inner, None if d is None else _dptr(d), info.ctypes.data_as(_P)))
        return info

    def newton_solve(self, init=True, game_id0=0):
        st = np.zeros(self.B, dtype=game_stats_dtype)
        self.lib.check(self.lib.newton_solve(self.h, int(init), game_id0, st.ctypes.data_as(_P)))
        return st

    def newton_solve_async(self, init=True, game_id0=0):
        self.lib.check(self.lib.newton_solve_async(self.h, int(init), game_id0))

    def get_stats(self):
        st = np.zeros(self.B, dtype=game_stats_dtype)
        self.lib.check(self.lib.get_stats(self.h, st.ctypes.data_as(_P)))
        return st

    def get_history(self, game, max_records=None):
        """Statistics history of one game.  max_records=None: everything the game recorded (alg_get_stats first); a history
        the device buffer could not hold completely raises a warning (alg_get_history returns fewer records than were made)."""
        made = None
        if max_records is None:
            made = int(self.get_stats()["records"][game])
            max_records = max(made, 1)
        out = np.zeros(max_records, dtype=record_dtype); cnt = C.c_int32()
        self.lib.check(self.lib.get_history(self.h, game, max_records, out.ctypes.data_as(_P), C.byref(cnt)))
        if made is not None and cnt.value < made:
            import warnings
            warnings.warn(f"alg_get_history: game {game} made {made} records, the device history holds {cnt.value} (truncated)")
        return out[:cnt.value]

    # ---- per-record violation profiles of the fused solve (alg_set_history_profiles) ---------
    def set_history_profiles(self, max_records):
        """newton_solve / newton_solve_async also store the four .vio vectors of every record they push, up to `max_records` records per
        game (0 = off, the default: the buffer is freed).  Refused (AlgamesError) for seven to ten players, while a hand-off budget is
        set, and for a buffer beyond 1 GiB; a backend without the entry point (the CPU oracle) raises AlgamesError."""
        self.lib.check(self.lib.set_history_profiles(self.h, int(max_records)))

    def get_history_profiles(self):
        """Capacity in records per game (0 = off; also 0 on a backend without the entry point)."""
        if "get_history_profiles" in self.lib.absent:
            return 0
        v = C.c_int32()
        self.lib.check(self.lib.get_history_profiles(self.h, C.byref(v)))
        return v.value

    def get_history_vio(self, game, max_records=None):
        """dict(dyn, con, sta, opt): the profiles of the records of one game's history, shapes (records, N-1 | N); row r belongs to record
        r of get_history.  Zero rows with profiles off, and after any entry point other than newton_solve* has pushed records."""
        cap = self.get_history_profiles() if max_records is None else int(max_records)
        if cap > 0:                                 # (host arrays for the records the game made, not for the whole capacity)
            cap = min(cap, max(int(self.get_stats()["records"][game]), 1))
        K, N = self.N - 1, self.N
        out = dict(dyn=np.zeros((cap, K)), con=np.zeros((cap, K)), sta=np.zeros((cap, N)), opt=np.zeros((cap, N)))
        cnt = C.c_int32()
        self.lib.check(self.lib.get_history_vio(self.h, int(game), cap, _dptr(out["dyn"]), _dptr(out["con"]), _dptr(out["sta"]), _dptr(out["opt"]), C.byref(cnt)))
        return {k: v[:cnt.value] for k, v in out.items()}

    def synchronize(self):
        self.lib.check(self.lib.synchronize(self.h))

    def ibr_solve_player(self, player):
        st = np.zeros(self.B, dtype=game_stats_dtype)
        self.lib.check(self.lib.ibr_solve_player(self.h, int(player), st.ctypes.data_as(_P)))
        return st

    def ibr_newton_solve(self, ibr_iter=100, ordering=None, delta_min=1e-9, init=True, game_id0=0):
        order = np.ascontiguousarray(np.arange(self.p) if ordering is None else np.asarray(ordering)[:self.p], dtype=np.int32)
        st = np.zeros(self.B, dtype=game_stats_dtype)
        self.lib.check(self.lib.ibr_newton_solve(self.h, int(init), game_id0, int(ibr_iter), _iptr(order), float(delta_min), st.ctypes.data_as(_P)))
        return st

    def mpc_advance(self):
        self.lib.check(self.lib.mpc_advance(self.h))

    # ---- the plant of the fused loop (alg_mpc_set_plant) ------------------------------------
    def mpc_set_plant(self, plant=None):
        """Sets the handle's plant (a Plant; None = the default, the loop without a plant).  hold must not exceed N - 1."""
        if plant is None:
            self.lib.check(self.lib.mpc_set_plant(self.h, None))
            return
        if not isinstance(plant, Plant):
            raise ValueError(f"mpc_set_plant: expected a Plant or None, got {type(plant).__name__}")
        if plant.hold > self.N - 1:
            raise ValueError(f"mpc_set_plant: hold must be in 1 ... N - 1 = {self.N - 1}, got {plant.hold}")
        c = alg_mpc_plant(plant.hold, plant.substeps, PLANT_INTEGRATORS.index(plant.integrator), 0)
        self.lib.check(self.lib.mpc_set_plant(self.h, C.byref(c)))

    def mpc_get_plant(self):
        """The handle's plant (Plant() on a backend without the entry point: such a backend runs the loop without a plant)."""
        if "mpc_get_plant" in self.lib.absent:
            return Plant()
        c = alg_mpc_plant()
        self.lib.check(self.lib.mpc_get_plant(self.h, C.byref(c)))
        return Plant(c.hold, c.substeps, PLANT_INTEGRATORS[c.integrator])

    def mpc_plant_advance(self, knot=0):
        """alg_mpc_plant_advance: one plant knot for every game -- x0 <- Phi(x0, u_{1+knot} of pdtraj) with the handle's plant (asynchronous)."""
        knot = int(knot)
        if not 0 <= knot <= self.N - 2:
            raise ValueError(f"mpc_plant_advance: knot must be in 0 ... N - 2 = {self.N - 2}, got {knot}")
        self.lib.check(self.lib.mpc_plant_advance(self.h, knot))

    def mpc_solve(self, steps, game_id0=0, record_states=False):
        """The whole receding-horizon loop in one call; returns the states (steps * hold + 1, B, n) -- hold: the handle's plant, 1 without
        one -- or None (asynchronous)."""
        states = np.empty((steps * self.mpc_get_plant().hold + 1, self.B, self.n)) if record_states else None
        self.lib.check(self.lib.mpc_solve(self.h, int(steps), int(game_id0), _dptr(states)))
        return states

    def mpc_solve_log(self, steps, game_id0=0, states=True, controls=True, stats=True):
        """alg_mpc_solve_log: the loop of mpc_solve with the closed-loop log.  Returns (states (knots+1, B, n), controls (knots, B, m),
        stats (steps, B) of game_stats_dtype), None for every part not asked for; asynchronous if none is.  knots = steps * hold of the
        handle's plant (mpc_set_plant), = steps without one."""
        steps = int(steps)
        knots = steps * self.mpc_get_plant().hold
        st = np.empty((knots + 1, self.B, self.n)) if states else None
        uc = np.empty((knots, self.B, self.m)) if controls else None
        gs = np.zeros((steps, self.B), dtype=game_stats_dtype) if stats else None
        self.lib.check(self.lib.mpc_solve_log(self.h, steps, int(game_id0), _dptr(st), _dptr(uc), None if gs is None else gs.ctypes.data_as(_P)))
        return st, uc, gs

    def mpc_set_cost_log(self, on=True):
        """Closed-loop cost log of mpc_solve / mpc_solve_log (alg_mpc_set_cost_log; off by default): with it on the loop also leaves the
        running cost of every plant knot and player on the device (mpc_get_cost).  A backend without it (the CPU oracle) raises AlgamesError."""
        if not isinstance(on, (bool, int, np.integer)):
            raise ValueError(f"mpc_set_cost_log: on must be a bool, got {on!r}")
        self.lib.check(self.lib.mpc_set_cost_log(self.h, int(bool(on))))

    def mpc_get_cost_log(self):
        v = C.c_int32()
        self.lib.check(self.lib.mpc_get_cost_log(self.h, C.byref(v)))
        return bool(v.value)

    def mpc_get_cost(self, max_knots=None):
        """The cost log of the most recent mpc_solve / mpc_solve_log (alg_mpc_get_cost; waits for the stream): (stage (k, B, p, 3), total
        (B, p, 3)) -- stage[q, g, i] = dt l_i(states[q], controls[q]) in the components [state, control, collision] with the schedule rows
        the knot's solve used, total their sum over ALL knots of the run, k = min(max_knots, knots).  (None, None) while there is none:
        log off, no loop yet, or invalidated by an adder, set_lqr, set_scenario_data or mpc_set_schedule."""
        if max_knots is not None and (isinstance(max_knots, bool) or not isinstance(max_knots, (int, np.integer)) or max_knots < 0):
            raise ValueError(f"mpc_get_cost: max_knots must be a non-negative integer or None, got {max_knots!r}")
        v = C.c_int32()
        self.lib.check(self.lib.mpc_get_cost(self.h, 0, None, None, C.byref(v)))
        if v.value == 0:
            return None, None
        k = v.value if max_knots is None else min(int(max_knots), v.value)
        stage = np.empty((k, self.B, self.p, 3)); total = np.empty((self.B, self.p, 3))
        self.lib.check(self.lib.mpc_get_cost(self.h, k, _dptr(stage), _dptr(total), C.byref(v)))
        return stage, total

    def mpc_set_con_log(self, on=True):
        """Closed-loop constraint log of mpc_solve / mpc_solve_log (alg_mpc_set_con_log; off by default): with it on the loop also leaves
        the constraint values of every plant knot on the device (mpc_get_con).  A backend without it (the CPU oracle) raises AlgamesError."""
        if not isinstance(on, (bool, int, np.integer)):
            raise ValueError(f"mpc_set_con_log: on must be a bool, got {on!r}")
        self.lib.check(self.lib.mpc_set_con_log(self.h, int(bool(on))))

    def mpc_get_con_log(self):
        v = C.c_int32()
        self.lib.check(self.lib.mpc_get_con_log(self.h, C.byref(v)))
        return bool(v.value)

    def mpc_get_con(self, max_knots=None):
        """The constraint log of the most recent mpc_solve / mpc_solve_log (alg_mpc_get_con; waits for the stream): (vals (k, B, K1), worst
        (B, 7), first (B, 7) int32), k = min(max_knots, knots).  vals[q, g] are the rows of one step in the knot layout (con_knot_len): the
        control-bound rows on controls[q], every other row on states[q + 1], with the schedule rows the knot's solve used.  worst: the
        maximum of every ALG_CON_* kind's rows over ALL knots (-inf: kind not added, NaN: a row is NaN); first: the first knot with a row
        that is not <= 0, -1 if none.  (None, None, None) while there is no log: log off, no loop yet, or invalidated by an adder, set_lqr,
        set_scenario_data or mpc_set_schedule."""
        if max_knots is not None and (isinstance(max_knots, bool) or not isinstance(max_knots, (int, np.integer)) or max_knots < 0):
            raise ValueError(f"mpc_get_con: max_knots must be a non-negative integer or None, got {max_knots!r}")
        v = C.c_int32()
        self.lib.check(self.lib.mpc_get_con(self.h, 0, None, None, None, C.byref(v)))
        if v.value == 0:
            return None, None, None
        k = v.value if max_knots is None else min(int(max_knots), v.value)
        vals = np.empty((k, self.B, self.con_knot_len())); worst = np.empty((self.B, ALG_CON_KINDS)); first = np.empty((self.B, ALG_CON_KINDS), dtype=np.int32)
        self.lib.check(self.lib.mpc_get_con(self.h, k, _dptr(vals), _dptr(worst), _iptr(first), C.byref(v)))
        return vals, worst, first

    # ---- schedules of the fused loop (alg_mpc_set_schedule) ----------------------------------
    def _sched_kind(self, kind):
        """(ABI kind, doubles per game and row) of a schedule kind: "lqr_target" / ALG_SCHED_LQR_TARGET, "disturbance" /
        ALG_SCHED_DISTURBANCE or a scenario kind."""
        if kind == "disturbance" or (not isinstance(kind, str) and int(kind) == ALG_SCHED_DISTURBANCE):
            return ALG_SCHED_DISTURBANCE, self.n
        if kind == "lqr_target" or (not isinstance(kind, str) and int(kind) == ALG_SCHED_LQR_TARGET):
            return ALG_SCHED_LQR_TARGET, self.p * self.ni + self.p * self.mi
        if isinstance(kind, str) and kind not in SCEN_KINDS:
            raise ValueError(f"unknown schedule kind {kind!r}; 'lqr_target', 'disturbance' or one of {SCEN_KINDS}")
        k = self._kind(kind)
        return k, self.scenario_data_len(k)

    def mpc_set_schedule(self, kind, data):
        """Values per MPC step and game of one kind for mpc_solve: data (rows, B, len), step t of the loop takes row min(t, rows - 1);
        None drops the kind's schedule.  kind: a scenario kind (name in SCEN_KINDS or ALG_SCEN_* value; len = scenario_data_len(kind)) or
        "lqr_target" (len = p ni + p mi: xf (p, ni) | uf (p, mi) of every game) or "disturbance" (len = n: added to the advanced state of
        every step, finite).  See alg_mpc_set_schedule."""
        k, L = self._sched_kind(kind)
        if data is None:
            self.lib.check(self.lib.mpc_set_schedule(self.h, k, 0, None))
            return
        a = np.ascontiguousarray(np.asarray(data, dtype=np.float64))
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (self.B, L):
            raise ValueError(f"schedule of kind {kind!r}: expected shape (rows >= 1, {self.B}, {L}), got {a.shape}")
        if k == ALG_SCHED_DISTURBANCE and not np.all(np.isfinite(a)):
            raise ValueError(f"schedule of kind {kind!r}: every entry must be finite (row {int(np.argwhere(~np.isfinite(a))[0][0])})")
        self.lib.check(self.lib.mpc_set_schedule(self.h, k, a.shape[0], _dptr(a)))
        if k != ALG_SCHED_DISTURBANCE:
            self._refresh_con_len()

    def mpc_get_schedule(self, kind):
        """Rows of the kind's schedule, 0 = none."""
        k, _ = self._sched_kind(kind)
        v = C.c_int32()
        self.lib.check(self.lib.mpc_get_schedule(self.h, k, C.byref(v)))
        return v.value

    def mpc_totals(self, reset=False):
        it = np.zeros(self.B, dtype=np.int64); cv = np.zeros(self.B, dtype=np.int64)
        self.lib.check(self.lib.mpc_totals(self.h, it.ctypes.data_as(C.POINTER(C.c_int64)), cv.ctypes.data_as(C.POINTER(C.c_int64)), int(reset)))
        return it, cv

    def get_x0(self):
        return self.get_traj(ALG_TRAJ_PD)[:, :self.n].copy()

    # ---- views of a traj buffer (primal_dual_traj.jl layout) ----------------------------------
    def split_traj(self, z):
        """z: (B, n+S) -> states (B,N,n), controls (B,N-1,m) joint order, duals (B,p,N-1,n)."""
        B, n, m, p, N, mi = z.shape[0], self.n, self.m, self.p, self.N, self.mi
        blk = z[:, n:].reshape(B, N - 1, self.b)
        X = np.concatenate([z[:, None, :n], blk[:, :, :n]], axis=1)
        ug = blk[:, :, n:n + m].reshape(B, N - 1, p, mi)         # [player, j] -> joint index i + j*p
        U = ug.transpose(0, 1, 3, 2).reshape(B, N - 1, m)
        L = blk[:, :, n + m:].reshape(B, N - 1, p, n).transpose(0, 2, 1, 3)
        return X, U, L

    def join_traj(self, X, U, L):
        B, n, m, p, N, mi = X.shape[0], self.n, self.m, self.p, self.N, self.mi
        z = np.zeros((B, self.traj_len))
        z[:, :n] = X[:, 0]
        blk = z[:, n:].reshape(B, N - 1, self.b)
        blk[:, :, :n] = X[:, 1:]
        blk[:, :, n:n + m] = U.reshape(B, N - 1, mi, p).transpose(0, 1, 3, 2).reshape(B, N - 1, m)
        blk[:, :, n + m:] = L.transpose(0, 2, 1, 3).reshape(B, N - 1, p * n)
        return z
