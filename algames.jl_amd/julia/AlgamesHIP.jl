# AlgamesHIP.jl -- Julia host shim over the C ABI of libalgames_hip.so (include/algames_hip.h).
#
# UNTESTED IN THIS ENVIRONMENT: neither the build container nor the GPU box has a `julia` binary (SURVEY.md section 0), so
# this file is the binding a maintainer of Algames.jl would add.  Every ABI call it makes, in the order it makes them, is
# mirrored through the identical ctypes binding by tests/test_gpu_boundary.py (same layouts, same write-back arithmetic).
#
# It keeps the reference API surface for the hot path.  `GameProblem` / `Options` are the reference's own types;
#   bp = BatchedGameProblem(probs; device=0)          one device handle for a batch of structurally identical problems
#   newton_solve!(bp)                                 src/problem/solver_methods.jl:5-65 for every problem of the batch
#   ibr_newton_solve!(bp; ibr_opts), ibr_newton_solve!(bp, i)     solver_methods.jl:133-228
#   mpc_solve!(bp, steps; schedule)                   receding-horizon loop of BASELINE config 5 (opts.shift / opts.dual_reset), with per-step values of targets / obstacles
#   mpc_solve_log!(bp, steps; disturbance)            the same loop with the closed-loop log (controls and statistics of every step) and a plant disturbance
#   player_costs(bp), set_mpc_cost_log!(bp, on), mpc_costs(bp)    what a plan / a closed-loop run costs each player, evaluated on the device
#   constraint_values(bp), set_mpc_con_log!(bp, on), mpc_constraints(bp)    the constraint rows of a plan / a closed-loop run, read-only, evaluated on the device
#   newton_solve!(probs::Vector{<:GameProblem})       convenience: build a handle, solve, release
#   sp = ShardedGameProblem(probs; devices=0:7); newton_solve!(sp)     the batch split over several devices (one handle each)
# After a solve every `prob.pdtraj`, the multipliers / penalties / values of every constraint (`conval.λ`, `.μ`, `.vals`,
# constraints_methods.jl:329-379) and `prob.stats` (struct/statistics.jl:5-57) hold what the reference's solver would have left.
module AlgamesHIP

using Algames
using LinearAlgebra
using StaticArrays
import Algames: newton_solve!, ibr_newton_solve!

const TO = Algames.TrajectoryOptimization
const LIB = get(ENV, "ALGAMES_HIP_LIB", joinpath(@__DIR__, "..", "lib", "libalgames_hip.so"))

struct AlgDesc
    model::Int32; p::Int32; d::Int32; N::Int32
    dt::Float64
    batch::Int32; device::Int32
end

struct AlgOptions                      # POD mirror of include/algames_hip.h: alg_options
    amplitude_init::Float64; shift::Int32; regularize::Int32
    reg_0::Float64; alpha_decrease::Float64; beta::Float64
    ls_iter::Int32; dual_reset::Int32; delta_min::Float64
    rho_0::Float64; rho_increase::Float64; rho_max::Float64; lambda_max::Float64; alpha_dual::Float64
    alphax_dual::NTuple{10,Float64}
    eps_dyn::Float64; eps_sta::Float64; eps_con::Float64; eps_opt::Float64
    outer_iter::Int32; inner_iter::Int32
    seed::Int64
end

struct AlgRecord
    outer::Int32; ls_j::Int32
    alpha::Float64; res::Float64; delta::Float64
    dyn_vio::Float64; con_vio::Float64; sta_vio::Float64; opt_vio::Float64
    t_elap::Float64
end

struct AlgGameStats
    status::Int32; outer_iters::Int32; newton_iters::Int32; records::Int32; converged::Int32; ls_failures::Int32
    refinements::Int32; reserved::Int32
    last::AlgRecord
end

check(rc) = rc == 0 || error(unsafe_string(ccall((:alg_last_error, LIB), Cstring, ())))

model_id(::DoubleIntegratorGame) = Int32(0)
model_id(::UnicycleGame) = Int32(1)
model_id(::BicycleGame) = Int32(2)
model_id(::QuadrotorGame) = Int32(3)      # src/dynamics/quadrotor.jl (the constructor's constants; mass through alg_set_quadrotor)

function abi_options(o::Options)
    ax = ntuple(i -> i <= length(o.αx_dual) ? Float64(o.αx_dual[i]) : 1.0, 10)
    AlgOptions(o.amplitude_init, min(o.shift, 2^30), o.regularize, o.reg_0, o.α_decrease, o.β, o.ls_iter,
               o.dual_reset, o.Δ_min, o.ρ_0, o.ρ_increase, o.ρ_max, o.λ_max, o.α_dual, ax,
               o.ϵ_dyn, o.ϵ_sta, o.ϵ_con, o.ϵ_opt, o.outer_iter, o.inner_iter, o.seed)
end

"""
A batch of structurally identical `GameProblem`s bound to one device handle (`alg_create` ... `alg_destroy`).
All problems must share model, N, dt, options and constraint structure (which constraints exist, the number of walls / circles /
pairs, per-player sets, cylinder axes, the +-inf pattern of the bounds; `setup!` checks it and errors naming the first problem that
differs); they may differ in x0, in the LQR data and in the constraint and collision-cost numbers (radii, bounds, obstacle positions),
which are uploaded per game (`alg_set_scenario_data`) where they differ.  The handle lives until `close(bp)` or finalisation,
so repeated solves (warm starts with `opts.dual_reset = false`, MPC loops) reuse the device buffers.
`scenario_kernels = :base` (default `:ext`): problems that carry only the base constraint set (pair radii, collision cost, control
bounds) keep the base kernels -- fused pass, team kernels, straggler hand-off -- when their numbers differ per game
(`alg_set_scenario_kernels`); `scenario_kernels(bp)` reports the setting and the kernels in use.
"""
mutable struct BatchedGameProblem{P<:GameProblem}
    probs::Vector{P}
    h::Ptr{Cvoid}
    con_len::Int
    function BatchedGameProblem(probs::Vector{P}; device::Integer=0, scenario_kernels::Symbol=:ext) where {P<:GameProblem}
        bp = new{P}(probs, C_NULL, 0)
        finalizer(close, bp)                                        # registered first: a failing setup! must not leak the handle
        try
            setup!(bp, device; scenario_kernels=scenario_kernels)
        catch
            close(bp)
            rethrow()
        end
        return bp
    end
end

function Base.close(bp::BatchedGameProblem)
    if bp.h != C_NULL
        ccall((:alg_destroy, LIB), Cvoid, (Ptr{Cvoid},), bp.h)
        bp.h = C_NULL
    end
    return nothing
end

sync_options!(bp::BatchedGameProblem) =       # `opts` is shared by reference and read at solve time, like the reference does
    check(ccall((:alg_set_options, LIB), Cint, (Ptr{Cvoid}, Ref{AlgOptions}), bp.h, Ref(abi_options(bp.probs[1].opts))))

function setup!(bp::BatchedGameProblem, device; scenario_kernels::Symbol = :ext)
    scenario_kernels in (:ext, :base) || error("setup!: scenario_kernels must be :ext or :base")
    probs = bp.probs; prob = probs[1]; ps = prob.probsize; B = length(probs)
    N, n, m, p = ps.N, ps.n, ps.m, ps.p
    ni, mi = ps.ni[1], ps.mi[1]
    d = prob.model isa DoubleIntegratorGame ? mi : (prob.model isa QuadrotorGame ? 3 : 2)
    dt = prob.pdtraj.pr[1].dt
    desc = Ref(AlgDesc(model_id(prob.model), p, d, N, dt, B, device))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:alg_create, LIB), Cint, (Ref{AlgDesc}, Ref{Ptr{Cvoid}}), desc, h))
    bp.h = h[]
    # before the adders (ALG_SCEN_KERNELS_BASE = 1; the default is the handle's own)
    scenario_kernels == :base && check(ccall((:alg_set_scenario_kernels, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, 1))
    sync_options!(bp)
    # x0: B x n, game-major (Julia is column-major: build n x B)
    x0 = hcat([Vector(pr.x0) for pr in probs]...)
    check(ccall((:alg_set_x0, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), bp.h, x0))
    # LQR data from game_obj.obj[i][1] (LQRCost: Q diagonal, q = -Q xf), per game: (ni x p x B) in memory order
    Qd = zeros(ni, p, B); Rd = zeros(mi, p, B); xf = zeros(ni, p, B); uf = zeros(mi, p, B)
    for (g, pr) in enumerate(probs), i in 1:p
        c = pr.game_obj.obj[i][1].cost[1]
        Qfull = diag(c.Q); Rfull = diag(c.R)
        Qd[:, i, g] = Qfull[ps.pz[i]]; Rd[:, i, g] = Rfull[ps.pu[i]]
        xf[:, i, g] = -(c.q ./ map(x -> x == 0 ? 1.0 : x, Qfull))[ps.pz[i]]
        uf[:, i, g] = -(c.r ./ map(x -> x == 0 ? 1.0 : x, Rfull))[ps.pu[i]]
    end
    check(ccall((:alg_set_lqr, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32),
                bp.h, Qd, Rd, xf, uf, 1))
    # collision costs: game_obj.obj[i][2:end] are CollisionCost objectives (objective.jl:84-100)
    if length(prob.game_obj.obj[1]) > 1
        rad = [prob.game_obj.obj[i][2].cost[1].r for i in 1:p]
        mu = [prob.game_obj.obj[i][2].cost[1].μ for i in 1:p]
        check(ccall((:alg_add_collision_cost, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), bp.h, rad, mu))
    end
    # state constraints of player i, in the order they were added (constraints_methods.jl): dispatch on the type
    # collision avoidance: every CollisionConstraint of player i's state constraints is ONE ordered pair (i, j) with its own radius
    # (add_collision_avoidance!(game_con, i, j, radius), constraints_methods.jl:5-19; the vector form adds all pairs with r_i + r_j,
    # :21-33).  add_spherical_collision_avoidance! builds the constraint on pz[i][1:3] (three indices) instead of px[i] (two).
    for i in 1:p, cv in prob.game_con.state_conval[i]
        con = cv.con
        con isa TO.CollisionConstraint || continue
        j = partner_of(ps, con)
        fn = length(con.x1) == 3 ? :alg_add_spherical_collision_avoidance_pair : :alg_add_collision_avoidance_pair
        check(fn === :alg_add_collision_avoidance_pair ?
              ccall((:alg_add_collision_avoidance_pair, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Float64), bp.h, i - 1, j - 1, con.radius) :
              ccall((:alg_add_spherical_collision_avoidance_pair, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Float64), bp.h, i - 1, j - 1, con.radius))
    end
    if prob.model isa BicycleGame
        check(ccall((:alg_set_bicycle, LIB), Cint, (Ptr{Cvoid}, Float64, Float64), bp.h, prob.model.lf, prob.model.lr))
    elseif prob.model isa QuadrotorGame
        check(ccall((:alg_set_quadrotor, LIB), Cint, (Ptr{Cvoid}, Float64), bp.h, prob.model.mass))
    end
    pts(a, b, c) = Vector{Float64}(vec(permutedims(hcat(Vector(a), Vector(b), Vector(c)))))      # n x 3, row-major
    for i in 1:p, cv in prob.game_con.state_conval[i]
        con = cv.con
        if con isa Algames.StateBoundConstraint                      # add_state_bound!(game_con, i, x_max, x_min)
            check(ccall((:alg_add_state_bound, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), bp.h, i - 1,
                        Vector{Float64}(con.x_max), Vector{Float64}(con.x_min)))
        elseif con isa Algames.WallConstraint                        # add_wall_constraint!(game_con, walls) / (game_con, i, walls)
            check(ccall((:alg_add_wall_constraint_player, LIB), Cint,
                        (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), bp.h, i - 1, length(con),
                        Vector{Float64}(con.x1), Vector{Float64}(con.y1), Vector{Float64}(con.x2), Vector{Float64}(con.y2),
                        Vector{Float64}(con.xv), Vector{Float64}(con.yv)))
        elseif con isa TO.CircleConstraint                           # add_circle_constraint!(game_con, xc, yc, radius) / (game_con, i, ...)
            check(ccall((:alg_add_circle_constraint_player, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), bp.h, i - 1, length(con),
                        Vector{Float64}(con.x), Vector{Float64}(con.y), Vector{Float64}(con.radius)))
        elseif con isa Algames.Wall3DConstraint                      # add_wall_constraint!(game_con, walls::Vector{Wall3D}) / (game_con, i, walls) (constraints_methods.jl:208-247)
            check(ccall((:alg_add_wall3d_constraint_player, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), bp.h, i - 1, length(con),
                        pts(con.x1, con.y1, con.z1), pts(con.x2, con.y2, con.z2), pts(con.x3, con.y3, con.z3), pts(con.xv, con.yv, con.zv)))
        elseif con isa Algames.CylinderConstraint                    # add_wall_constraint!(game_con, walls::Vector{CylinderWall}) / (game_con, i, walls) (:256-299)
            axis = Int32[s == :x ? 0 : s == :y ? 1 : 2 for s in con.v]
            check(ccall((:alg_add_cylinder_constraint_player, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}), bp.h, i - 1, length(con),
                        pts(con.p1, con.p2, con.p3), axis, Vector{Float64}(con.l), Vector{Float64}(con.r)))
        end
    end
    if !isempty(prob.game_con.control_conval)
        con = prob.game_con.control_conval[1].con
        check(ccall((:alg_add_control_bound, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), bp.h,
                    Vector(con.u_max), Vector(con.u_min)))
    end
    # batches of differing scenarios: every problem must have problem 1's constraint structure; the numbers may differ per game
    s1 = scenario_structure(prob)
    for g in 2:B
        sg = scenario_structure(probs[g])
        sg == s1 || error("BatchedGameProblem: problem $g differs from problem 1 in its constraint structure (first difference: " *
                          "$(first_difference(sg, s1))); only the numbers may differ between the games of one batch")
    end
    upload_scenarios!(bp)
    cl = Ref{Int32}(0)
    check(ccall((:alg_get_con_len, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), bp.h, cl))
    bp.con_len = cl[]
    return bp
end

# What the problems of one batch must share: the kinds of constraint per player and their counts, pair partners, cylinder axes, and
# the +-inf pattern of the bounds (it decides which rows count).  The numbers themselves are not part of it.
infpattern(v) = Tuple(isinf(x) ? sign(x) : 0.0 for x in v)
function scenario_structure(prob)
    ps = prob.probsize
    s = Any[("collision cost", length(prob.game_obj.obj[1]) > 1)]
    for i in 1:ps.p, cv in prob.game_con.state_conval[i]
        con = cv.con
        if con isa TO.CollisionConstraint
            push!(s, ("collision avoidance", i, partner_of(ps, con), length(con.x1)))
        elseif con isa Algames.StateBoundConstraint
            push!(s, ("state bound", i, infpattern(con.x_max), infpattern(con.x_min)))
        elseif con isa Algames.WallConstraint
            push!(s, ("walls", i, length(con)))
        elseif con isa TO.CircleConstraint
            push!(s, ("circles", i, length(con)))
        elseif con isa Algames.Wall3DConstraint
            push!(s, ("3-D walls", i, length(con)))
        elseif con isa Algames.CylinderConstraint
            push!(s, ("cylinders", i, Tuple(con.v)))
        end
    end
    if !isempty(prob.game_con.control_conval)
        con = prob.game_con.control_conval[1].con
        push!(s, ("control bound", infpattern(con.u_max), infpattern(con.u_min)))
    end
    return s
end
function first_difference(a, b)
    length(a) == length(b) || return "number of constraint sets"
    k = findfirst(q -> a[q] != b[q], eachindex(a))
    return string(a[k][1], a[k] isa Tuple && length(a[k]) > 1 && a[k][2] isa Integer ? " of player $(a[k][2])" : "")
end

# Per-game values of one ALG_SCEN_* kind (include/algames_hip.h) for problem `pr`, laid out on problem 1's tables
const SCEN_WALL, SCEN_CIRCLE, SCEN_WALL3D, SCEN_CYLINDER = 4, 5, 6, 7
function scenario_values(bp::BatchedGameProblem, pr, kind::Integer, len::Integer)
    prob1 = bp.probs[1]; ps = prob1.probsize; p, n, m = ps.p, ps.n, ps.m
    v = zeros(len)
    if kind == 0                                     # collision radius of ordered pair (i, j) at (i-1) p + j
        for i in 1:p, cv in pr.game_con.state_conval[i]
            cv.con isa TO.CollisionConstraint && (v[(i - 1) * p + partner_of(ps, cv.con)] = cv.con.radius)
        end
    elseif kind == 1                                 # collision cost: radius (p) | mu (p)
        for i in 1:p
            c = pr.game_obj.obj[i][2].cost[1]; v[i] = c.r; v[p + i] = c.μ
        end
    elseif kind == 2                                 # control bound: u_max (m) | u_min (m)
        con = pr.game_con.control_conval[1].con
        v[1:m] = con.u_max; v[m+1:2m] = con.u_min
    elseif kind == 3                                 # state bound: x_max (p x n) | x_min (p x n); players without one: +-inf
        v[1:p*n] .= Inf; v[p*n+1:2p*n] .= -Inf
        for i in 1:p, cv in pr.game_con.state_conval[i]
            cv.con isa Algames.StateBoundConstraint || continue
            v[(i - 1) * n .+ (1:n)] = cv.con.x_max; v[p * n + (i - 1) * n .+ (1:n)] = cv.con.x_min
        end
    else                                             # tables: problem 1's entry of each conval row, pr's values of that row
        walls, circs, walls3, cyls = constraint_tables(prob1)
        T, key, tab, keep = kind == SCEN_WALL ? (Algames.WallConstraint, wall_key, walls, 1:6) :
                            kind == SCEN_CIRCLE ? (TO.CircleConstraint, circ_key, circs, 1:3) :
                            kind == SCEN_WALL3D ? (Algames.Wall3DConstraint, wall3_key, walls3, 1:12) :
                            (Algames.CylinderConstraint, cyl_key, cyls, [1, 2, 3, 5, 6])      # the axis stays handle-wide
        F = length(keep); seen = falses(length(tab))
        for i in 1:p, (cv1, cvg) in zip(prob1.game_con.state_conval[i], pr.game_con.state_conval[i])
            cv1.con isa T || continue
            for r in 1:length(cv1.con)
                t = findfirst(==(key(cv1.con, r)), tab)
                val = Float64[key(cvg.con, r)[f] for f in keep]
                if seen[t]
                    v[(t - 1) * F .+ (1:F)] == val || error("BatchedGameProblem: problem 1 shares one table entry between players " *
                                                            "that another problem gives different values")
                end
                v[(t - 1) * F .+ (1:F)] = val; seen[t] = true
            end
        end
    end
    return v
end

"(setting, in_use) of alg_get_scenario_kernels: `:ext` / `:base`, and the kernels the next launch takes -- 0 base, 1 EXT, 2 base kernels reading per-game blocks"
function scenario_kernels(bp::BatchedGameProblem)
    w = Ref{Int32}(0); u = Ref{Int32}(0)
    check(ccall((:alg_get_scenario_kernels, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), bp.h, w, u))
    return (w[] == 1 ? :base : :ext), Int(u[])
end
# Upload the kinds whose numbers differ between the problems (the handle holds problem 1's values for the others)
function upload_scenarios!(bp::BatchedGameProblem)
    B = length(bp.probs)
    B > 1 || return nothing
    for kind in 0:7
        len = Ref{Int32}(0)
        check(ccall((:alg_scenario_data_len, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}), bp.h, kind, len))
        len[] == 0 && continue
        V = reduce(hcat, [scenario_values(bp, pr, kind, len[]) for pr in bp.probs])      # len x B = B x len game-major
        all(g -> isequal(V[:, g], V[:, 1]), 2:B) && continue
        check(ccall((:alg_set_scenario_data, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), bp.h, kind, V))
    end
    return nothing
end

# player j whose position indices a CollisionConstraint of player i points at (x2 = px[j] or pz[j][1:3])
partner_of(ps, con) = findfirst(q -> all(con.x2 .== ps.px[q][1:length(con.x2)]) || all(con.x2 .== ps.pz[q][1:length(con.x2)]), 1:ps.p)

# The library keeps ONE table of distinct walls (circles) per handle; alg_add_wall_constraint_player appends the entries it has not
# seen, in call order, and row w of the ABI's wall block is table entry w for every player (include/algames_hip.h).  The same
# table is rebuilt here from the constraint objects, in the order setup! made the calls (players 1..p, their convals in order), so
# that a conval's row r maps to its table index.
wall_key(con, r) = (con.x1[r], con.y1[r], con.x2[r], con.y2[r], con.xv[r], con.yv[r])
circ_key(con, r) = (con.x[r], con.y[r], con.radius[r])
wall3_key(con, r) = (con.x1[r], con.y1[r], con.z1[r], con.x2[r], con.y2[r], con.z2[r], con.x3[r], con.y3[r], con.z3[r], con.xv[r], con.yv[r], con.zv[r])
cyl_key(con, r) = (con.p1[r], con.p2[r], con.p3[r], con.v[r], con.l[r], con.r[r])
function constraint_tables(prob)
    walls = Tuple[]; circs = Tuple[]; walls3 = Tuple[]; cyls = Tuple[]
    for i in 1:prob.probsize.p, cv in prob.game_con.state_conval[i]
        con = cv.con
        if con isa Algames.WallConstraint
            for r in 1:length(con); k = wall_key(con, r); k in walls || push!(walls, k); end
        elseif con isa TO.CircleConstraint
            for r in 1:length(con); k = circ_key(con, r); k in circs || push!(circs, k); end
        elseif con isa Algames.Wall3DConstraint
            for r in 1:length(con); k = wall3_key(con, r); k in walls3 || push!(walls3, k); end
        elseif con isa Algames.CylinderConstraint
            for r in 1:length(con); k = cyl_key(con, r); k in cyls || push!(cyls, k); end
        end
    end
    return walls, circs, walls3, cyls
end

# ---- layout of the ABI's constraint vectors (include/algames_hip.h "Layouts") -----------------------------------------------
# Returns, for constraint value object `cv` of player i (0 = shared control constraint), a function (l, r) -> 1-based position in
# the ABI vector of row r (1-based, in the conval's own row numbering) at the l-th knot index of the conval.
function abi_position(bp::BatchedGameProblem, cv, i::Int)
    prob = bp.probs[1]; ps = prob.probsize; N, n, m, p = ps.N, ps.n, ps.m, ps.p
    K = N - 1
    con = cv.con
    col_len = p * (p - 1) * K                                        # the ABI always carries the collision-avoidance and control-bound rows
    ctl_len = 2m * K                                                # (include/algames_hip.h "Layouts"); rows that were never added are inert
    has_sb = any(c -> c.con isa Algames.StateBoundConstraint, vcat(prob.game_con.state_conval...))
    sb_len = has_sb ? p * 2n * K : 0
    walls, circs, walls3, cyls = constraint_tables(prob)             # distinct entries in call order = the library's tables
    nwall, ncirc = length(walls), length(circs)
    if con isa TO.CollisionConstraint                               # rows: pair q = (i, j), knot k = 2..N
        j = partner_of(ps, con)
        q = (i - 1) * (p - 1) + (j < i ? j : j - 1) - 1
        return (l, r) -> q * K + (cv.inds[l] - 2) + 1
    elseif con isa Algames.ControlBoundConstraint                   # knot k = 1..N-1: (u - u_max)(m) then (u_min - u)(m); the reference keeps finite rows only
        fin = con.inds                                              # control_bound_constraint.jl:35-38
        return (l, r) -> col_len + (cv.inds[l] - 1) * 2m + fin[r]
    elseif con isa Algames.StateBoundConstraint                     # player i, knot k = 2..N: (x - x_max)(n) then (x_min - x)(n), finite rows
        fin = con.inds
        return (l, r) -> col_len + ctl_len + ((i - 1) * K + (cv.inds[l] - 2)) * 2n + fin[r]
    elseif con isa Algames.WallConstraint                           # row r of the conval = table entry w(r)
        tw = [findfirst(==(wall_key(con, r)), walls) for r in 1:length(con)]
        return (l, r) -> col_len + ctl_len + sb_len + ((i - 1) * K + (cv.inds[l] - 2)) * nwall + tw[r]
    elseif con isa TO.CircleConstraint
        tc = [findfirst(==(circ_key(con, r)), circs) for r in 1:length(con)]
        return (l, r) -> col_len + ctl_len + sb_len + p * nwall * K + ((i - 1) * K + (cv.inds[l] - 2)) * ncirc + tc[r]
    elseif con isa Algames.Wall3DConstraint || con isa Algames.CylinderConstraint
        nw3, ncy = length(walls3), length(cyls)                      # row r of the conval = table entry t(r), as for the planar walls
        base = col_len + ctl_len + sb_len + p * nwall * K + p * ncirc * K
        if con isa Algames.Wall3DConstraint
            t3 = [findfirst(==(wall3_key(con, r)), walls3) for r in 1:length(con)]
            return (l, r) -> base + ((i - 1) * K + (cv.inds[l] - 2)) * nw3 + t3[r]
        end
        ty = [findfirst(==(cyl_key(con, r)), cyls) for r in 1:length(con)]
        return (l, r) -> base + p * nw3 * K + ((i - 1) * K + (cv.inds[l] - 2)) * ncy + ty[r]
    end
    error("AlgamesHIP: constraint type $(typeof(con)) is not bound")
end

each_conval(f, game_con) = begin
    for (i, list) in enumerate(game_con.state_conval), cv in list; f(cv, i); end
    for cv in game_con.control_conval; f(cv, 0); end
end

"Push the multipliers / penalties the Julia side holds to the device (warm starts with opts.dual_reset = false)."
function push_duals!(bp::BatchedGameProblem)
    bp.con_len == 0 && return
    B = length(bp.probs)
    lam = zeros(bp.con_len, B); mu = fill(Float64(bp.probs[1].opts.ρ_0), bp.con_len, B)
    for (g, pr) in enumerate(bp.probs)
        each_conval(pr.game_con) do cv, i
            pos = abi_position(bp, cv, i)
            for l in eachindex(cv.inds), r in eachindex(cv.λ[l])
                lam[pos(l, r), g] = cv.λ[l][r]; mu[pos(l, r), g] = cv.μ[l][r]
            end
        end
    end
    check(ccall((:alg_set_con_duals, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), bp.h, lam, mu))
end

"Write back what a solve left on the device: pdtraj, constraint values / multipliers / penalties, Statistics."
function pull_results!(bp::BatchedGameProblem, stats::Vector{AlgGameStats})
    prob = bp.probs[1]; ps = prob.probsize; B = length(bp.probs)
    N, n, S = ps.N, ps.n, ps.S
    # pdtraj: [x_1 | horizontal-order vector] per game (primal_dual_traj.jl:46-75)
    z = zeros(n + S, B)
    check(ccall((:alg_get_traj, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), bp.h, 0, z))
    for (g, pr) in enumerate(bp.probs)
        Algames.set_traj!(pr.core, pr.pdtraj, view(z, n+1:n+S, g))
        Algames.RobotDynamics.set_state!(pr.pdtraj.pr[1], SVector{n}(z[1:n, g]))
    end
    # constraint multipliers and penalties (dual_update!, penalty_update!, constraints_methods.jl:329-379, 421-440)
    if bp.con_len > 0
        lam = zeros(bp.con_len, B); mu = zeros(bp.con_len, B)
        check(ccall((:alg_get_con_duals, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), bp.h, lam, mu))
        for (g, pr) in enumerate(bp.probs)
            each_conval(pr.game_con) do cv, i
                pos = abi_position(bp, cv, i)
                for l in eachindex(cv.inds)
                    cv.λ[l] .= [lam[pos(l, r), g] for r in eachindex(cv.λ[l])]
                    cv.μ[l] .= [mu[pos(l, r), g] for r in eachindex(cv.μ[l])]
                end
            end
            Algames.evaluate!(pr.game_con, pr.pdtraj.pr)             # conval.vals at the final iterate, as solver_methods.jl:57 leaves them
        end
    end
    # prob.stats: one record! per stored record (statistics.jl:30-57); the violation objects carry the recorded maxima (what the
    # solver's exit test and the plot recipes read, solver_plots.jl:83-125); the final record also gets its per-knot profiles --
    # with history profiles on (set_history_profiles!) EVERY stored record gets the .vio vectors the solve stored next to it
    pcap = Ref{Int32}(0)
    check(ccall((:alg_get_history_profiles, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), bp.h, pcap))
    cap = max(Int(maximum(s.records for s in stats)), 1)
    rec = Vector{AlgRecord}(undef, cap); cnt = Ref{Int32}(0)
    # the .vio vectors of the four violation objects at the final iterate (violations.jl), all games in one call
    vdyn = zeros(N - 1, B); vcon = zeros(N - 1, B); vsta = zeros(N, B); vopt = zeros(N, B)
    check(ccall((:alg_get_violation_profile, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), bp.h, vdyn, vcon, vsta, vopt))
    for (g, pr) in enumerate(bp.probs)
        check(ccall((:alg_get_history, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{AlgRecord}, Ref{Int32}), bp.h, g - 1, cap, rec, cnt))
        cnt[] < stats[g].records && @warn "AlgamesHIP: Statistics history truncated" game = g kept = cnt[] records = stats[g].records
        Algames.reset!(pr.stats)
        for t in 1:cnt[]
            r = rec[t]
            dv = Algames.DynamicsViolation(N); dv.max = r.dyn_vio
            cvv = Algames.ControlViolation(N); cvv.max = r.con_vio
            sv = Algames.StateViolation(N); sv.max = r.sta_vio
            ov = Algames.OptimalityViolation(N); ov.max = r.opt_vio
            Algames.record!(pr.stats, r.t_elap, r.res, r.delta, dv, cvv, sv, ov, Int(r.outer))      # t_elap: device real-time counter
        end
        nvio = Ref{Int32}(0)
        if pcap[] > 0 && cnt[] > 0                                  # row-major n x (N-1 | N) of the ABI = column t of these matrices is record t
            hdyn = zeros(N - 1, cnt[]); hcon = zeros(N - 1, cnt[]); hsta = zeros(N, cnt[]); hopt = zeros(N, cnt[])
            check(ccall((:alg_get_history_vio, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                        bp.h, g - 1, cnt[], hdyn, hcon, hsta, hopt, nvio))
            for t in 1:nvio[]
                pr.stats.dyn_vio[t].vio .= view(hdyn, :, t); pr.stats.con_vio[t].vio .= view(hcon, :, t)
                pr.stats.sta_vio[t].vio .= view(hsta, :, t); pr.stats.opt_vio[t].vio .= view(hopt, :, t)
            end
        end
        if cnt[] > 0 && nvio[] < cnt[]                              # final record (solver_methods.jl:63): per-knot profiles from the device
            pr.stats.dyn_vio[end].vio .= view(vdyn, :, g); pr.stats.con_vio[end].vio .= view(vcon, :, g)
            pr.stats.sta_vio[end].vio .= view(vsta, :, g); pr.stats.opt_vio[end].vio .= view(vopt, :, g)
        end
    end
    return stats
end

"""
    newton_solve!(bp::BatchedGameProblem; game_id0=0, init=true)

Batched drop-in for `newton_solve!(prob)` (src/problem/solver_methods.jl:5-65).  `init=false` keeps the controls / duals the
problems currently hold as the initial guess (`alg_set_traj`); with `opts.dual_reset == false` the constraint multipliers and
penalties the problems hold are pushed first (warm start).  An `opts.f_init` other than `rand` is honoured through the reference's
own `init_traj!` on the host followed by a solve with `init = 0`.  Returns the per-game `AlgGameStats`.
"""
function newton_solve!(bp::BatchedGameProblem; game_id0::Integer=0, init::Bool=true, async::Bool=false)
    sync_options!(bp)
    B = length(bp.probs); ps = bp.probs[1].probsize
    bp.probs[1].opts.dual_reset || push_duals!(bp)
    if init && bp.probs[1].opts.f_init !== rand                     # caller-supplied generator (options.jl:11): the reference's own
        for pr in bp.probs                                          # init_traj! makes the guess (solver_methods.jl:12-13), the device
            o = pr.opts                                             # generates only the default `rand`
            Algames.Random.seed!(o.seed)
            Algames.init_traj!(pr.pdtraj; x0=pr.x0, f=o.f_init, amplitude=o.amplitude_init, s=o.shift)
        end
        init = false
    end
    if !init || bp.probs[1].opts.shift < ps.N                       # explicit initial guess / shifted warm start: upload pdtraj
        z = zeros(ps.n + ps.S, B)
        for (g, pr) in enumerate(bp.probs)
            z[1:ps.n, g] = Vector(Algames.RobotDynamics.state(pr.pdtraj.pr[1]))
            Algames.get_traj!(pr.core, view(z, ps.n+1:ps.n+ps.S, g), pr.pdtraj)
        end
        check(ccall((:alg_set_traj, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), bp.h, 0, z))
    end
    stats = Vector{AlgGameStats}(undef, B)
    if async                                                        # ShardedGameProblem: every device is launched before the first wait
        check(ccall((:alg_newton_solve_async, LIB), Cint, (Ptr{Cvoid}, Int32, Int64), bp.h, init ? 1 : 0, game_id0))
        return nothing
    end
    check(ccall((:alg_newton_solve, LIB), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{AlgGameStats}), bp.h, init ? 1 : 0, game_id0, stats))
    return pull_results!(bp, stats)
end

"Waits for an asynchronous solve of the handle and writes the results back into its problems."
function finish!(bp::BatchedGameProblem)
    check(ccall((:alg_synchronize, LIB), Cint, (Ptr{Cvoid},), bp.h))
    stats = Vector{AlgGameStats}(undef, length(bp.probs))
    check(ccall((:alg_get_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{AlgGameStats}), bp.h, stats))
    return pull_results!(bp, stats)
end

"""
    ShardedGameProblem(probs; devices=0:7)

The batch split over several devices (BASELINE north_star: "the batch shards naturally across the 8 GPUs"; SURVEY.md 8(e)): shard r
owns the contiguous problems `cuts[r]` and the global scenario ids `game_id0 + first(cuts[r]) - 1 ...`, one `BatchedGameProblem`
(device handle + stream) per entry of `devices`.  `newton_solve!` launches every shard (`alg_newton_solve_async`) before it waits
for the first one; there is no data-path collective.  Python twin: `algames.jl_amd/sharding.py` (`ShardedGameProblem`,
tests/test_gpu_boundary.py::test_multi_device_solve_behind_the_boundary_two_handles_on_one_gpu).
"""
struct ShardedGameProblem{P<:GameProblem}
    shards::Vector{BatchedGameProblem{P}}
    cuts::Vector{UnitRange{Int}}
end
function ShardedGameProblem(probs::Vector{P}; devices=0:0, scenario_kernels::Symbol=:ext) where {P<:GameProblem}
    B, W = length(probs), length(devices)
    per = cld(B, W)                                                 # scenarios.shard_range: ceil(B / W) games per shard, last ones shorter
    cuts = [min((r - 1) * per, B)+1:min(r * per, B) for r in 1:W]
    keep = [r for r in 1:W if !isempty(cuts[r])]
    shards = [BatchedGameProblem(probs[cuts[r]]; device=collect(devices)[r], scenario_kernels=scenario_kernels) for r in keep]
    # one kernel shape for all shards (the automatic choice depends on a handle's batch size; the shapes differ at rounding level)
    w = Ref{Int32}(0)
    check(ccall((:alg_get_waves_per_game, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), shards[1].h, w))
    for bp in shards
        check(ccall((:alg_set_waves_per_game, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, w[]))
    end
    ShardedGameProblem{P}(shards, cuts[keep])
end
Base.close(sp::ShardedGameProblem) = foreach(close, sp.shards)
function newton_solve!(sp::ShardedGameProblem; game_id0::Integer=0, init::Bool=true)
    for (bp, r) in zip(sp.shards, sp.cuts)
        newton_solve!(bp; game_id0=game_id0 + first(r) - 1, init=init, async=true)
    end
    return vcat([finish!(bp) for bp in sp.shards]...)
end

function newton_solve!(probs::Vector{<:GameProblem}; device::Integer=0, game_id0::Integer=0)
    bp = BatchedGameProblem(probs; device=device)
    try
        return newton_solve!(bp; game_id0=game_id0)
    finally
        close(bp)
    end
end

"ibr_newton_solve!(prob; ibr_opts) (solver_methods.jl:133-169) for every problem of the batch."
function ibr_newton_solve!(bp::BatchedGameProblem; ibr_opts::IBROptions=IBROptions(), game_id0::Integer=0)
    sync_options!(bp)
    p = bp.probs[1].probsize.p
    ordering = Int32.(ibr_opts.ordering[1:p] .- 1)
    stats = Vector{AlgGameStats}(undef, length(bp.probs))
    check(ccall((:alg_ibr_newton_solve, LIB), Cint, (Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Int32}, Float64, Ptr{AlgGameStats}),
                bp.h, 1, game_id0, ibr_opts.ibr_iter, ordering, ibr_opts.Δ_min, stats))
    return pull_results!(bp, stats)
end

"ibr_newton_solve!(prob, i) (solver_methods.jl:171-228): player i best-responds on the stored trajectories."
function ibr_newton_solve!(bp::BatchedGameProblem, i::Int)
    sync_options!(bp)
    stats = Vector{AlgGameStats}(undef, length(bp.probs))
    check(ccall((:alg_ibr_solve_player, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{AlgGameStats}), bp.h, i - 1, stats))
    return pull_results!(bp, stats)
end

const SCHED_LQR_TARGET = 100       # ALG_SCHED_LQR_TARGET: xf (p x ni) | uf (p x mi) of every game and MPC step
const SCHED_DISTURBANCE = 101      # ALG_SCHED_DISTURBANCE: w (n) of every game and MPC step, added to the advanced state
"ABI kind of a schedule key: an ALG_SCEN_* value (0 .. 7), `SCHED_DISTURBANCE` or `:lqr_target`"
sched_kind(k::Integer) = Int32(k)
sched_kind(k::Symbol) = k == :lqr_target ? Int32(SCHED_LQR_TARGET) : error("mpc_solve!: unknown schedule kind $k (:lqr_target or an ALG_SCEN_* value)")
"rows of the kind's schedule on the handle, 0 = none (alg_mpc_get_schedule)"
function mpc_schedule_rows(bp::BatchedGameProblem, kind)
    rows = Ref{Int32}(0)
    check(ccall((:alg_mpc_get_schedule, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}), bp.h, sched_kind(kind), rows))
    return Int(rows[])
end

"""
    with_schedules(f, bp, who, schedule)

Uploads every entry of `schedule` (`nothing` or a `Dict` kind => `len x B x rows` array; `alg_mpc_set_schedule`), runs `f()` and drops
the uploaded kinds again, also when an upload or `f` throws.  Shared by `mpc_solve!` and `mpc_solve_log!`.
"""
function with_schedules(f, bp::BatchedGameProblem, who::String, schedule)
    B = length(bp.probs)
    done = Int32[]
    try
        if schedule !== nothing
            for (k, V) in schedule
                A = Array{Float64, 3}(V)
                size(A, 2) == B && size(A, 3) >= 1 || error("$who: schedule of kind $k must be len x $B x rows")
                check(ccall((:alg_mpc_set_schedule, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}), bp.h, sched_kind(k), size(A, 3), A))
                push!(done, sched_kind(k))
            end
        end
        return f()
    finally
        for k in sort!(done)
            check(ccall((:alg_mpc_set_schedule, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}), bp.h, k, 0, C_NULL))
        end
    end
end

"""
    mpc_solve!(bp, steps; game_id0=0, schedule=nothing) -> (newton_iters, converged, states)

Receding-horizon loop of BASELINE config 5, one launch: `steps` x (newton_solve! from the shifted warm start, x0 <- RK2(x_1, u_1)),
first solve with the handle's shift / dual_reset, later ones with shift = 1 and dual_reset = false (the reference's hooks,
options.jl:16-17, primal_dual_traj.jl:29-44, solver_methods.jl:25).  `states` is n x B x (steps + 1).

`schedule`: a `Dict` kind => `len x B x rows` array (column-major: the ABI's rows x B x len, step-major) of values per MPC step and game --
kind an ALG_SCEN_* value or `:lqr_target` (xf | uf of every game; needs per-game LQR data).  The step-th solve (1-based) takes slice min(step, rows) of every
kind; the schedule is uploaded (`alg_mpc_set_schedule`), applied inside the single launch and dropped again, the handle keeps the rows
the last step used.
"""
function mpc_solve!(bp::BatchedGameProblem, steps::Integer; game_id0::Integer=0, schedule=nothing)
    sync_options!(bp)
    B = length(bp.probs); n = bp.probs[1].probsize.n
    iters = zeros(Int64, B); conv = zeros(Int64, B)
    check(ccall((:alg_mpc_totals, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int32), bp.h, iters, conv, 1))      # reset the totals
    states = zeros(n, B, steps + 1)
    with_schedules(bp, "mpc_solve!", schedule) do
        check(ccall((:alg_mpc_solve, LIB), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}), bp.h, steps, game_id0, states))
    end
    check(ccall((:alg_mpc_totals, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int32), bp.h, iters, conv, 0))
    stats = Vector{AlgGameStats}(undef, B)
    check(ccall((:alg_get_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{AlgGameStats}), bp.h, stats))
    pull_results!(bp, stats)                                        # the last solve's iterate, multipliers and statistics
    for (g, pr) in enumerate(bp.probs)
        pr.x0 = SVector{n}(states[:, g, end])
    end
    return iters, conv, states
end

"""
    mpc_solve_log!(bp, steps; game_id0=0, schedule=nothing, disturbance=nothing, costs=false, constraints=false) -> (newton_iters, converged, states, controls, stats[, costs][, constraints])

The loop of `mpc_solve!` with the closed-loop log (`alg_mpc_solve_log`): `controls` is m x B x steps (the joint control every advance
applied, player-major), `stats` a B x steps matrix of `AlgGameStats` (every step's solve as `alg_get_stats` reports it).
`schedule`: as for `mpc_solve!`.  `disturbance`: n x B x rows, finite -- after the advance of the step-th solve the state becomes
x0 + slice min(step, rows); `states` holds the disturbed states.  It travels as one more schedule kind (`SCHED_DISTURBANCE`): uploaded
and dropped again with the others.  `costs=true` switches the cost log on for the call (`set_mpc_cost_log!`) and appends `mpc_costs(bp)`,
read before the schedules are dropped, to the result.  `constraints=true` does the same with the constraint log (`set_mpc_con_log!`) and
appends `mpc_constraints(bp)` behind it.
"""
function mpc_solve_log!(bp::BatchedGameProblem, steps::Integer; game_id0::Integer=0, schedule=nothing, disturbance=nothing, costs::Bool=false, constraints::Bool=false)
    sync_options!(bp)
    B = length(bp.probs); n = bp.probs[1].probsize.n; m = bp.probs[1].probsize.m
    iters = zeros(Int64, B); conv = zeros(Int64, B)
    check(ccall((:alg_mpc_totals, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int32), bp.h, iters, conv, 1))      # reset the totals
    states = zeros(n, B, steps + 1); controls = zeros(m, B, steps)
    stats = Matrix{AlgGameStats}(undef, B, steps)
    up = Dict{Any, Any}()
    schedule === nothing || merge!(up, schedule)
    if disturbance !== nothing
        W = Array{Float64, 3}(disturbance)
        size(W, 1) == n && size(W, 2) == B && size(W, 3) >= 1 || error("mpc_solve_log!: the disturbance must be $n x $B x rows")
        up[SCHED_DISTURBANCE] = W
    end
    cost = nothing
    log0 = costs && mpc_cost_log(bp)
    costs && set_mpc_cost_log!(bp, true)
    con = nothing
    klog0 = constraints && mpc_con_log(bp)
    constraints && set_mpc_con_log!(bp, true)
    try
        with_schedules(bp, "mpc_solve_log!", up) do
            check(ccall((:alg_mpc_solve_log, LIB), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{AlgGameStats}),
                        bp.h, steps, game_id0, states, controls, stats))
            costs && (cost = mpc_costs(bp))
            constraints && (con = mpc_constraints(bp))
        end
    finally
        costs && !log0 && set_mpc_cost_log!(bp, false)
        constraints && !klog0 && set_mpc_con_log!(bp, false)
    end
    check(ccall((:alg_mpc_totals, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int32), bp.h, iters, conv, 0))
    pull_results!(bp, stats[:, end])                                # the last solve's iterate, multipliers and statistics
    for (g, pr) in enumerate(bp.probs)
        pr.x0 = SVector{n}(states[:, g, end])
    end
    out = (iters, conv, states, controls, stats)
    costs && (out = (out..., cost))
    constraints && (out = (out..., con))
    return out
end

# ---- step-wise entry points on a handle (same names as the reference's functions they batch) ------------------------------------
"residual!(prob, pdtraj) + residual_norm (global_quantities.jl:9-97): S x B residuals in vertical order and ||res||_1 / S per game."
function residual(bp::BatchedGameProblem; reg::Float64=0.0)
    S = bp.probs[1].probsize.S; B = length(bp.probs)
    res = zeros(S, B); rn = zeros(B)
    check(ccall((:alg_residual, LIB), Cint, (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}), bp.h, 0, reg, res, rn))
    return res, rn
end
"residual_jacobian! + regularisation (global_quantities.jl:109-193): S x S x B dense, rows vertical order, columns horizontal order."
function residual_jacobian(bp::BatchedGameProblem; reg::Float64=0.0, games::UnitRange{Int}=1:length(bp.probs))
    S = bp.probs[1].probsize.S
    jac = zeros(S, S, length(games))      # only the requested games are built on the device and copied
    check(ccall((:alg_residual_jacobian_games, LIB), Cint, (Ptr{Cvoid}, Float64, Int32, Int32, Ptr{Float64}),
                bp.h, reg, Int32(first(games) - 1), Int32(length(games)), jac))
    return jac
end
"""
    set_refinement!(bp; max_steps = 2, tol = 2.0^-34, mu_tight = 1.6e5)

Iterative refinement of the Newton direction (alg_set_refinement): the stand-in for the backward stability of `lu(core.jac) \\ core.res`
(solver_methods.jl:87).  After every structured solve the opt-u rows of `J d = -res` are evaluated; while their row-wise backward error exceeds `tol`
the direction is corrected by one more elimination on the residual (at most `max_steps` times); below `mu_tight` (largest penalty of the game)
the tolerance is relaxed in proportion, at most 256 x.  `max_steps = 0` switches both off.
"""
set_refinement!(bp::BatchedGameProblem; max_steps::Integer=2, tol::Float64=2.0^-34, mu_tight::Float64=1.6e5) =
    check(ccall((:alg_set_refinement, LIB), Cint, (Ptr{Cvoid}, Int32, Float64, Float64), bp.h, max_steps, tol, mu_tight))

"""
    set_handoff!(bp, iters)

Straggler hand-off for heterogeneous batches (alg_set_handoff): games that need more than `iters` inner iterations in the one-wavefront kernel
park and a second launch finishes them with the team kernel; `0` switches it off (the default).  `handoff(bp)` returns the budget and the
number of games the most recent solve handed over.
"""
set_handoff!(bp::BatchedGameProblem, iters::Integer) = check(ccall((:alg_set_handoff, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, iters))
"""
    set_history_profiles!(bp, max_records)

Per-record violation profiles (alg_set_history_profiles): with `max_records > 0` `newton_solve!` stores the `.vio` vectors of every record it pushes,
up to `max_records` records per game, and `pull_results!` fills `.vio` of every stored record of `prob.stats` from them; `0` switches it off (the
default: only the final record carries its profiles).  Refused for seven to ten players and while a hand-off budget is set.
"""
set_history_profiles!(bp::BatchedGameProblem, max_records::Integer) = check(ccall((:alg_set_history_profiles, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, max_records))
function handoff(bp::BatchedGameProblem)
    k = Ref{Int32}(0); n = Ref{Int32}(0)
    check(ccall((:alg_get_handoff, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), bp.h, k, n))
    return Int(k[]), Int(n[])
end
"Line search with the step sizes tried in groups (`true`, default) or one after another (`false`): bit-identical norms (alg_set_line_search_groups)."
set_line_search_groups!(bp::BatchedGameProblem, on::Bool) = check(ccall((:alg_set_line_search_groups, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, on ? 1 : 0))

"3 x B: [max |rho|, row-wise backward error, largest row scale] of the opt-u rows of every game's last Newton direction (alg_get_direction_gate)."
function direction_gate(bp::BatchedGameProblem)
    out = zeros(3, length(bp.probs))
    check(ccall((:alg_get_direction_gate, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), bp.h, out))
    return out
end

"""
    player_costs(bp; trial=false, stage=false) -> total [, stage]

What the plan costs each player, evaluated on the device (alg_get_cost): `total` is 3 x p x B -- the components [state, control, collision]
of J_i = sum_k w_k l_i(x_k, u_k), the values of the `LQRCost` objectives (objective.jl:12-35) and of `stage_cost(::CollisionCost, x)`
(objective.jl:122-131) with w_k = dt for k < N and w_N = 1; constraints, multipliers and penalties do not enter.  `trial=true` evaluates
`pdtraj_trial`; `stage=true` also returns the summands per knot, 3 x p x N x B.  Nothing on the handle changes.
"""
function player_costs(bp::BatchedGameProblem; trial::Bool=false, stage::Bool=false)
    B = length(bp.probs); p = bp.probs[1].probsize.p; N = bp.probs[1].probsize.N
    total = zeros(3, p, B)
    stg = stage ? zeros(3, p, N, B) : nothing
    check(ccall((:alg_get_cost, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), bp.h, trial ? 1 : 0, total, stage ? stg : C_NULL))
    return stage ? (total, stg) : total
end
"""
    set_mpc_cost_log!(bp, on)

The closed-loop cost log of `mpc_solve!` / `mpc_solve_log!` (alg_mpc_set_cost_log; off by default): with it on the loop also evaluates, on the
device, what every plant knot cost every player -- with the schedule rows the knot's solve used.  `mpc_costs(bp)` reads it.
"""
set_mpc_cost_log!(bp::BatchedGameProblem, on::Bool) = check(ccall((:alg_mpc_set_cost_log, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, on ? 1 : 0))
function mpc_cost_log(bp::BatchedGameProblem)
    on = Ref{Int32}(0)
    check(ccall((:alg_mpc_get_cost_log, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), bp.h, on))
    return on[] != 0
end
"""
    mpc_costs(bp) -> (stage, total) or nothing

The cost log of the most recent `mpc_solve!` / `mpc_solve_log!` (alg_mpc_get_cost): `stage` is 3 x p x B x knots -- the running cost
dt l_i(states[q], controls[q]) in the components [state, control, collision] --, `total` 3 x p x B its sum over the knots (no terminal term).
`nothing` while there is none: log off, no loop yet, or invalidated by an adder, new LQR or scenario data, or a schedule call.  (The loop
entry points drop their schedules when they return, which invalidates the log: `mpc_solve_log!(...; costs=true)` reads it before that.)
"""
function mpc_costs(bp::BatchedGameProblem)
    B = length(bp.probs); p = bp.probs[1].probsize.p
    knots = Ref{Int32}(0)
    check(ccall((:alg_mpc_get_cost, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int32}), bp.h, 0, C_NULL, C_NULL, knots))
    knots[] == 0 && return nothing
    stage = zeros(3, p, B, Int(knots[])); total = zeros(3, p, B)
    check(ccall((:alg_mpc_get_cost, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int32}), bp.h, knots[], stage, total, knots))
    return stage, total
end

"""
    constraint_values(bp; trial=false) -> vals

The constraint values of the plan, read-only, evaluated on the device (alg_get_con_values): con_len x B in the ABI's constraint layout --
`evaluate!(game_con, traj)` (constraints_methods.jl:329-379) without the dual and penalty update; c <= 0 is feasible, a row of an infinite
bound reports -Inf, an inert row 0.  `trial=true` evaluates `pdtraj_trial`.  Nothing on the handle changes.  `con_knot_len(bp)` is K1, the
rows of one step: con_len = (N - 1) K1.
"""
function constraint_values(bp::BatchedGameProblem; trial::Bool=false)
    len = Ref{Int32}(0)
    check(ccall((:alg_get_con_len, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), bp.h, len))
    vals = zeros(Int(len[]), length(bp.probs))
    check(ccall((:alg_get_con_values, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), bp.h, trial ? 1 : 0, vals))
    return vals
end
function con_knot_len(bp::BatchedGameProblem)
    len = Ref{Int32}(0)
    check(ccall((:alg_con_knot_len, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), bp.h, len))
    return Int(len[])
end
"""
    set_mpc_con_log!(bp, on)

The closed-loop constraint log of `mpc_solve!` / `mpc_solve_log!` (alg_mpc_set_con_log; off by default): with it on the loop also evaluates,
on the device, the constraint rows of every plant knot -- with the schedule rows the knot's solve used.  `mpc_constraints(bp)` reads it.
"""
set_mpc_con_log!(bp::BatchedGameProblem, on::Bool) = check(ccall((:alg_mpc_set_con_log, LIB), Cint, (Ptr{Cvoid}, Int32), bp.h, on ? 1 : 0))
function mpc_con_log(bp::BatchedGameProblem)
    on = Ref{Int32}(0)
    check(ccall((:alg_mpc_get_con_log, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), bp.h, on))
    return on[] != 0
end
"""
    mpc_constraints(bp) -> (vals, worst, first) or nothing

The constraint log of the most recent `mpc_solve!` / `mpc_solve_log!` (alg_mpc_get_con): `vals` is K1 x B x knots -- the rows of one step
in the knot layout, the control-bound rows on the control applied over the knot, every other row on the state the knot reaches --, `worst`
7 x B the maximum of every ALG_CON_* kind's rows over the run (-Inf: kind not added), `first` 7 x B the first knot (0-based, as the ABI
counts) with a row that is not <= 0, -1 if none.  `nothing` while there is no log (see `mpc_costs`).
"""
function mpc_constraints(bp::BatchedGameProblem)
    B = length(bp.probs); K1 = con_knot_len(bp)
    knots = Ref{Int32}(0)
    check(ccall((:alg_mpc_get_con, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Int32}), bp.h, 0, C_NULL, C_NULL, C_NULL, knots))
    knots[] == 0 && return nothing
    vals = zeros(K1, B, Int(knots[])); worst = zeros(7, B); first = zeros(Int32, 7, B)
    check(ccall((:alg_mpc_get_con, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Int32}), bp.h, knots[], vals, worst, first, knots))
    return vals, worst, first
end

const PARAM_KINDS = (:x0, :xf, :Q, :R, :uf, :collision_cost, :collision_radius, :control_bound)     # ALG_PARAM_* = index - 1
function param_code(wrt::Symbol)
    k = findfirst(==(wrt), PARAM_KINDS)
    k === nothing && throw(ArgumentError("wrt must be one of $(PARAM_KINDS), got $(wrt)"))
    return Int32(k - 1)
end
"Entries of the parameter vector `wrt` (alg_param_len), in the order of its setter."
function param_len(bp::BatchedGameProblem, wrt::Symbol)
    len = Ref{Int32}(0)
    check(ccall((:alg_param_len, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}), bp.h, param_code(wrt), len))
    return Int(len[])
end
"""
    parameter_sensitivity(bp, wrt; reg=0.0, games=nothing, steps=nothing, directions=nothing) -> (X, status)

d z* / d theta = -J^-1 d res / d theta at `pdtraj` with the right-hand sides built on the device (alg_kkt_sensitivity): theta is the initial
state (`:x0`), the LQR data (`:xf`, `:Q`, `:R`, `:uf`, the orders of the `LQRCost` diagonals), the collision cost (`:collision_cost`, radius
(p) | mu (p)), the pair radii (`:collision_radius`, p x p ordered pairs) or the control bounds (`:control_bound`, u_max (m) | u_min (m)) --
the numbers each game was assembled with; multipliers, penalties and active sets are held.  `X` is (count b) x ncol x B in the horizontal
order of the Newton direction, b = n + m + n p rows per step.  `steps = (first, count)` (0-based steps) stores and downloads those steps'
rows only.  `directions` (len x ndir x B): the columns are the directional derivatives along those vectors, one elimination each; without
it there is one column per entry of theta.  `games = (first, count)` (0-based) restricts work, `X`, `directions` and `status` to those games
(B = count).  `status` (B): 0 where every column was solved.  The raw arrays of the ABI come back: the row of (step k, entry e) of a
slice starting at step s0 is (k - s0) b + e + 1.
"""
function parameter_sensitivity(bp::BatchedGameProblem, wrt::Symbol; reg::Float64=0.0, games=nothing, steps=nothing, directions=nothing)
    ps = bp.probs[1].probsize
    b = ps.n + ps.m + ps.n * ps.p
    g0, B = games === nothing ? (0, length(bp.probs)) : (Int(games[1]), Int(games[2]))
    (g0 >= 0 && B >= 1 && g0 + B <= length(bp.probs)) || throw(ArgumentError("games = (first, count) must lie inside the batch of $(length(bp.probs))"))
    len = param_len(bp, wrt)
    s0, ns = steps === nothing ? (0, ps.N - 1) : (Int(steps[1]), Int(steps[2]))
    (s0 >= 0 && ns >= 1 && s0 + ns <= ps.N - 1) || throw(ArgumentError("steps = (first, count) must lie inside 0 ... $(ps.N - 2)"))
    ndir = directions === nothing ? 0 : size(directions, 2)
    directions === nothing || size(directions) == (len, ndir, B) || throw(ArgumentError("directions must be $(len) x ndir x $(B)"))
    dirs = directions === nothing ? C_NULL : Array{Float64}(directions)
    X = zeros(ns * b, directions === nothing ? len : ndir, B); status = zeros(Int32, B)
    check(ccall((:alg_kkt_sensitivity, LIB), Cint, (Ptr{Cvoid}, Float64, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Int32}),
                bp.h, reg, param_code(wrt), ndir, dirs, g0, B, s0, ns, X, status))
    return X, status
end

"""
    normal_equations(bp, cols, target, weight; reg=0.0, games=nothing) -> (H, g, loss, status)

The normal equations of fitting parameters to an observed trajectory, reduced on the device (alg_kkt_normal_equations).  `cols` is a vector of
`(wrt, index)` pairs, `wrt` a symbol of `parameter_sensitivity` and `index` the 1-based entry of that parameter vector: up to 63 distinct
columns, kinds mixed in any order; column c is the unit column `parameter_sensitivity` returns for it.  `target` is S x B, the observed
trajectory in the horizontal order of the Newton direction; `weight` is S (shared) or S x B, finite and >= 0.  With r = z - target over
the S entries of `pdtraj` behind x_1, per game: `loss` = 1/2 sum w r^2, `g` = X' W r (q x B), `H` = X' W X (q x q x B, both triangles,
symmetric bit for bit).  `status` (B): 0 where every column was solved.  `games = (first, count)` (0-based) restricts the call to those
games (B = count).  No sensitivity column is downloaded.
"""
function normal_equations(bp::BatchedGameProblem, cols::AbstractVector, target::AbstractMatrix, weight::AbstractVecOrMat; reg::Float64=0.0, games=nothing)
    ps = bp.probs[1].probsize
    S = ps.S
    g0, B = games === nothing ? (0, length(bp.probs)) : (Int(games[1]), Int(games[2]))
    (g0 >= 0 && B >= 1 && g0 + B <= length(bp.probs)) || throw(ArgumentError("games = (first, count) must lie inside the batch of $(length(bp.probs))"))
    q = length(cols)
    1 <= q <= 63 || throw(ArgumentError("cols must name 1 ... 63 columns"))
    size(target) == (S, B) || throw(ArgumentError("target must be $(S) x $(B)"))
    (size(weight) == (S,) || size(weight) == (S, B)) || throw(ArgumentError("weight must be $(S) or $(S) x $(B)"))
    cp = Int32[param_code(c[1]) for c in cols]; ci = Int32[Int(c[2]) - 1 for c in cols]
    H = zeros(q, q, B); g = zeros(q, B); loss = zeros(B); status = zeros(Int32, B)
    check(ccall((:alg_kkt_normal_equations, LIB), Cint,
                (Ptr{Cvoid}, Float64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                bp.h, reg, q, cp, ci, Array{Float64}(target), Array{Float64}(weight), ndims(weight) == 2 ? 1 : 0, g0, B, H, g, loss, status))
    return H, g, loss, status
end

"Give the inspection entry points' device scratch (dense Jacobians, MPC state logs) back to the allocator."
release_scratch!(bp::BatchedGameProblem) = check(ccall((:alg_release_scratch, LIB), Cint, (Ptr{Cvoid},), bp.h))

end # module
