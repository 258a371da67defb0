# QOCMI355X.jl — ccall shim that routes QuantumOptimalControl.jl's PWC GRAPE hot path to
# libqoc_mi355x.so (C ABI: include/qoc.h).  Nothing else in the reference changes: the Ipopt
# callbacks (examples/ipopt_callbacks_exp.jl) keep calling `QuantumOptimalControl.propagate`
# and `grape_sensitivity`; only the `setup_grape_cache` line constructs an `MI355XCache`.
#
#   cache = QOCMI355X.setup_grape_cache(A0Δt, complex(x0), (2, segment_count))
#   x     = QuantumOptimalControl.propagate(A0Δt, [A1Δt, A2Δt], u, x0, cache)      # method below
#   dJdu  = QuantumOptimalControl.grape_sensitivity(A0Δt, [A1Δt, A2Δt], dJfinal_dx, cache.u, x0, cache;
#                                                   dUkdp_order=3, dL_dx=dL_dx)
#
# Memory layout needs no conversion: Matrix{ComplexF64} is column-major interleaved (re, im),
# exactly the ABI's layout; u / dJdu are Matrix{Float64} (nu x Nt).
module QOCMI355X

import QuantumOptimalControl
using LinearAlgebra: tr
const QOC = QuantumOptimalControl

const libqoc = get(ENV, "QOC_MI355X_LIB", joinpath(@__DIR__, "..", "qoc_amd", "libqoc_mi355x.so"))

const QOC_FP64 = Cint(0)
const QOC_COST_TRACE = Cint(0)
const QOC_COST_ZCAL = Cint(1)
const QOC_COST_EXTERNAL = Cint(2)
const QOC_ERR_STALE = Cint(-3)

qoc_error(ctx) = unsafe_string(ccall((:qoc_last_error, libqoc), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, ctx)
    rc == 0 && return nothing
    # the reference raises error(...) at src/gradient_computations.jl:37-39 and :84-87
    error(qoc_error(ctx))
end

mutable struct MI355XCache
    ctx::Ptr{Cvoid}
    N::Int
    m::Int
    nu::Int
    Nt::Int
    u::Matrix{Float64}
    dJdu::Matrix{Float64}
    gen::UInt64        # hash of the generators last uploaded
    x0::UInt64
    function MI355XCache(ctx, N, m, nu, Nt)
        c = new(ctx, N, m, nu, Nt, zeros(nu, Nt), zeros(nu, Nt), 0, 0)
        finalizer(c) do c
            c.ctx != C_NULL && ccall((:qoc_destroy, libqoc), Cvoid, (Ptr{Cvoid},), c.ctx)
            c.ctx = C_NULL
        end
        return c
    end
end

"""
    setup_grape_cache(A0, x0, u_size; device=0, compress=nothing)

GPU-resident replacement of `QuantumOptimalControl.setup_grape_cache`
(src/gradient_computations.jl:79-96).  Errors on a dimension mismatch like the reference.
`compress = v` takes the reference's `compress_states` spec (src/utils.jl:96-109, 1-based, e.g.
`((1:2:27, [1,4]), (2:2:26, [2,3]))`): the kernels then run on the packed columns while `x`, `dJfinal_dx`
and `dL_dx` keep the caller's N x m layout (qoc_set_compression).
"""
function setup_grape_cache(A0, x0, u_size; device::Integer=0, compress=nothing)
    size(x0, 1) == size(A0, 1) || error("Error when creating cache, A0 and x0 have incompatiable dimensions")
    nu, Nt = u_size
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:qoc_create, libqoc), Cint,
               (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, Cint, Cint),
               ref, device, size(A0, 1), size(x0, 2), nu, Nt, 1, QOC_FP64)
    check(rc, C_NULL)
    c = MI355XCache(ref[], size(A0, 1), size(x0, 2), nu, Nt)
    check(ccall((:qoc_set_cost, libqoc), Cint, (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Cdouble),
                c.ctx, QOC_COST_EXTERNAL, C_NULL, 1.0), c.ctx)
    compress === nothing || set_compression!(c, compress)
    return c
end

function set_compression!(c::MI355XCache, v)
    (r1, c1), (r2, c2) = v
    l = [Cint.(collect(a) .- 1) for a in (r1, c1, r2, c2)]   # 0-based
    check(ccall((:qoc_set_compression, libqoc), Cint,
                (Ptr{Cvoid}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Ptr{Cint}, Cint),
                c.ctx, l[1], length(l[1]), l[2], length(l[2]), l[3], length(l[3]), l[4], length(l[4])), c.ctx)
end

function upload!(c::MI355XCache, A0, A, x0)
    h = hash((A0, A))
    if h != c.gen
        A0c = Matrix{ComplexF64}(A0)
        Ac = [Matrix{ComplexF64}(a) for a in A]
        ptrs = [pointer(a) for a in Ac]
        GC.@preserve A0c Ac ptrs begin
            check(ccall((:qoc_set_generators, libqoc), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{Ptr{ComplexF64}}),
                        c.ctx, A0c, ptrs), c.ctx)
        end
        c.gen = h
    end
    hx = hash(x0)
    if hx != c.x0
        x0c = Matrix{ComplexF64}(reshape(x0, size(x0, 1), :))
        GC.@preserve x0c check(ccall((:qoc_set_x0, libqoc), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Cint),
                                     c.ctx, x0c, 0), c.ctx)
        c.x0 = hx
    end
end

"""
    set_generator_ensemble!(cache, A0s, As, weights=nothing)

Robust control (include/qoc.h `qoc_set_generator_ensemble`): `A0s[e]` and `As[j][e]` are member e's Δt-prescaled
generators (E members, the layout of `upload!`'s arguments per member); `weights` E values used as given (`nothing`:
1/E each); an empty `A0s` clears the ensemble.  The generators of the last `propagate` (the nominal set) fix the block
layout, so call it after one.  With an ensemble set the library evaluates J̄ = Σ_e w_e J(u; member e) in
`qoc_eval_dev` / `qoc_eval_spline` (built-in costs: set one with `qoc_set_cost`, this cache's default is the external
cost of the reference's closures) and refuses `propagate` / `grape_sensitivity`, whose states are per member.
`upload!` of other generators (any later `propagate` after clearing) drops it.  Like the rest of this shim it is
written against the ABI and has not been run (no `julia` where the library is built and tested).
"""
function set_generator_ensemble!(c::MI355XCache, A0s::Vector{<:AbstractMatrix}, As::Vector{<:Vector},
                                 weights::Union{Nothing,AbstractVector}=nothing)
    E = length(A0s)
    if E == 0
        check(ccall((:qoc_set_generator_ensemble, libqoc), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Ptr{Ptr{ComplexF64}}, Ptr{Cdouble}),
                    c.ctx, 0, C_NULL, C_NULL, C_NULL), c.ctx)
        return nothing
    end
    length(As) == c.nu || error("expected $(c.nu) stacks of control generators, got $(length(As))")
    all(length(a) == E for a in As) || error("every stack of control generators needs $E members")
    # members contiguous: N x N x E column-major is E matrices of N x N one after the other
    A0c = cat((Matrix{ComplexF64}(a) for a in A0s)...; dims=3)
    Ac = [cat((Matrix{ComplexF64}(a) for a in stack)...; dims=3) for stack in As]
    ptrs = [pointer(a) for a in Ac]
    w = weights === nothing ? nothing : Vector{Float64}(weights)
    w === nothing || length(w) == E || error("weights needs $E entries")
    GC.@preserve A0c Ac ptrs w begin
        check(ccall((:qoc_set_generator_ensemble, libqoc), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Ptr{Ptr{ComplexF64}}, Ptr{Cdouble}),
                    c.ctx, E, A0c, ptrs, w === nothing ? C_NULL : pointer(w)), c.ctx)
    end
    c.gen = 0   # the next upload! reaches qoc_set_generators (which clears the ensemble) whatever its generators
    return nothing
end

"""Members of the generator ensemble (0: none)."""
ensemble_size(c::MI355XCache) = Int(ccall((:qoc_ensemble_size, libqoc), Cint, (Ptr{Cvoid},), c.ctx))

"""J of every member for the cache's one pulse at the last ensemble eval (`qoc_get_member_costs`); not run, see above."""
function member_costs(c::MI355XCache)
    Jm = zeros(max(ensemble_size(c), 1))
    check(ccall((:qoc_get_member_costs, libqoc), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), c.ctx, Jm), c.ctx)
    return Jm
end

"""
    set_ensemble_objective!(cache, kind, param=0.0)

What the ensemble evals minimise over the members (include/qoc.h `qoc_set_ensemble_objective`): `kind` one of `:mean`
(default, J̄ = Σ_e w_e J_e), `:max` (the worst member), `:cvar` with `param` = α in (0, 1] (the mean of the worst
α-fraction) or `:lse` with `param` = β > 0 (the smooth maximum).  A setting of the context: it holds with or without an
ensemble and survives `set_generator_ensemble!` and `upload!`.  Not run, like the shim's other ensemble calls.
"""
function set_ensemble_objective!(c::MI355XCache, kind::Symbol, param::Real=0.0)
    k = findfirst(==(kind), (:mean, :max, :cvar, :lse))
    k === nothing && error("kind must be :mean, :max, :cvar or :lse, got $kind")
    check(ccall((:qoc_set_ensemble_objective, libqoc), Cint, (Ptr{Cvoid}, Cint, Cdouble), c.ctx, k - 1, Float64(param)),
          c.ctx)
    return nothing
end

"""The member weights ω of the cache's one pulse at the last ensemble eval (`qoc_get_member_weights`; Σ ω = Σ w, and
dJ̄/du = Σ_e ω_e dJ_e/du); not run, see above."""
function member_weights(c::MI355XCache)
    om = zeros(max(ensemble_size(c), 1))
    check(ccall((:qoc_get_member_weights, libqoc), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), c.ctx, om), c.ctx)
    return om
end

"""
    set_time_scale!(cache, tau)

Gate duration as a variable (include/qoc.h `qoc_set_time_scale`): the cache's pulse evolves under τ (A0 + Σ_j u_jk A_j),
so its gate lasts τ times the nominal duration; `tau` finite and > 0, `nothing` clears it.  With it set the library
evaluates J and dJ/du at that duration in `qoc_eval_dev` / `qoc_eval_spline` (built-in costs, as for the ensemble),
leaves dJ/dτ at fixed u for `time_scale_grad`, and refuses `propagate` / `grape_sensitivity`.  It survives `upload!`.
Like the rest of this shim the four wrappers are written against the ABI and have not been run (no `julia` where the
library is built and tested).
"""
function set_time_scale!(c::MI355XCache, tau::Union{Nothing,Real})
    if tau === nothing
        check(ccall((:qoc_set_time_scale, libqoc), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), c.ctx, C_NULL), c.ctx)
    else
        t = [Float64(tau)]   # B = 1
        check(ccall((:qoc_set_time_scale, libqoc), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), c.ctx, t), c.ctx)
    end
    return nothing
end

"""dJ/dτ of the last eval under the time scale (`qoc_get_time_scale_grad`); not run, see above."""
function time_scale_grad(c::MI355XCache)
    d = zeros(1)
    check(ccall((:qoc_get_time_scale_grad, libqoc), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), c.ctx, d), c.ctx)
    return d[1]
end

"""Device pointers of τ and of dJ/dτ (`qoc_time_scale_dev`, `qoc_time_scale_grad_dev`; `C_NULL` when none is set), for
callers that write τ on the library's stream between evals; not run, see above."""
time_scale_device(c::MI355XCache) = ccall((:qoc_time_scale_dev, libqoc), Ptr{Cdouble}, (Ptr{Cvoid},), c.ctx)
time_scale_grad_device(c::MI355XCache) = ccall((:qoc_time_scale_grad_dev, libqoc), Ptr{Cdouble}, (Ptr{Cvoid},), c.ctx)

# qoc_opt_params and qoc_opt_duration (include/qoc.h), field for field
struct OptParams
    n::Cint; ns::Cint; nu::Cint
    lower::Cdouble; upper::Cdouble
    g_upper::NTuple{2,Cdouble}
    max_iter::Cint; memory::Cint; outer_iters::Cint; max_ls::Cint
    rho0::Cdouble; gtol::Cdouble
    order::Cint
end
struct OptDuration
    tau_lower::Cdouble; tau_upper::Cdouble; time_weight::Cdouble
end

"""
    opt_create_duration(B, params::OptParams, dur::OptDuration; device=0) -> Ptr{Cvoid}

The device optimiser with the gate duration as every seed's last variable (`qoc_opt_create_duration`): z = [c, τ],
`params.n == ns * nu + 1`, `params.lower / upper` bound c and `dur.tau_lower / tau_upper` bound τ.  Free the handle with
`ccall((:qoc_opt_destroy, libqoc), Cvoid, (Ptr{Cvoid},), opt)`.  Not run, see `set_time_scale!`.
"""
function opt_create_duration(B::Integer, params::OptParams, dur::OptDuration; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:qoc_opt_create_duration, libqoc), Cint, (Ptr{Ptr{Cvoid}}, Cint, Cint, Ref{OptParams}, Ref{OptDuration}),
                h, device, B, params, dur), C_NULL)
    return h[]
end

"""
    minimize_spline_duration!(cache, opt, d_z, max_ticks; poll_every=16) -> ticks

Time-optimal control on the device from start to finish (`qoc_minimize_spline_duration_dev`): minimises
f = J + time_weight τ over z = [c, τ] for every seed of the cache's context.  `d_z` is a device pointer to
B x (ns * nu + 1) doubles, the starts in and the final iterates out; the spline basis and a time scale
(`set_time_scale!`) must be set, and the time scale holds the final τ on return.  Not run, see `set_time_scale!`.
"""
function minimize_spline_duration!(c::MI355XCache, opt::Ptr{Cvoid}, d_z::Ptr{Cdouble}, max_ticks::Integer;
                                   poll_every::Integer=16)
    ticks = Ref{Clonglong}(0)
    check(ccall((:qoc_minimize_spline_duration_dev, libqoc), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Clonglong}),
                c.ctx, opt, d_z, max_ticks, poll_every, ticks), c.ctx)
    return Int(ticks[])
end

"""States of the last propagate, fetched lazily (the reference returns cache.x, Nt+1 matrices)."""
struct LazyStates <: AbstractVector{Matrix{ComplexF64}}
    c::MI355XCache
end
Base.size(s::LazyStates) = (s.c.Nt + 1,)
function Base.getindex(s::LazyStates, k::Int)
    out = Matrix{ComplexF64}(undef, s.c.N, s.c.m)
    check(ccall((:qoc_get_states, libqoc), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{ComplexF64}),
                s.c.ctx, 0, k - 1, out), s.c.ctx)
    return out
end

function Base.getproperty(c::MI355XCache, s::Symbol)
    s === :x && return LazyStates(c)
    return getfield(c, s)
end

# propagate (src/gradient_computations.jl:2-32) on the GPU
function QOC.propagate(A0, A::Vector{<:AbstractMatrix}, u, x0, cache::MI355XCache)
    upload!(cache, A0, A, x0)
    cache.u .= u                              # :12, kept for the stale-u check
    J = Ref{Cdouble}(0.0)
    check(ccall((:qoc_propagate, libqoc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Cdouble}),
                cache.ctx, cache.u, J), cache.ctx)
    return cache.x
end

const ENVELOPE_KINDS = Dict(:tunable_bus => Cint(0), :drag => Cint(1), :sinebasis => Cint(2))

"""
    eval_envelope(A0, A, kind, p, x0, tgate, dt, dJfinal_dx, cache) -> (dJdp, x)

Gradient of a terminal cost with respect to the parameters `p` of a parameterised pulse (src/parameterized_pulses.jl;
`kind` is `:drag`, `:sinebasis` or `:tunable_bus`) for dx/dt = (A0 + Σ_j c_j(t; p) A_j) x integrated with fixed-step
Tsit5 on [0, tgate] (wrap_envelope, src/QuantumOptimalControl.jl:43-54): the discrete adjoint of that scheme
(qoc_eval_envelope), i.e. the derivative of the cost of the `x` returned.  The generators are used as given (not
Δt-scaled).  The closure `dJfinal_dx` is evaluated here at x(tgate) (one forward run, qoc_propagate_envelope) and
handed over as λ (dJ = Re<λ, dx>).  ∂/∂p[1] of `:drag` / `:sinebasis` holds the horizon `tgate` fixed.
"""
function eval_envelope(A0, A::Vector{<:AbstractMatrix}, kind::Symbol, p::AbstractVector, x0, tgate, dt, dJfinal_dx,
                       cache::MI355XCache)
    upload!(cache, A0, A, x0)
    pv = Vector{Float64}(p)
    x = Matrix{ComplexF64}(undef, cache.N, cache.m)
    check(ccall((:qoc_propagate_envelope, libqoc), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Cdouble, Cdouble, Ptr{Float64}, Ptr{ComplexF64}),
                cache.ctx, ENVELOPE_KINDS[kind], pv, length(pv), tgate, dt, C_NULL, x), cache.ctx)
    λf = Matrix{ComplexF64}(dJfinal_dx(x))
    dJdp = zeros(length(pv))
    check(ccall((:qoc_eval_envelope, libqoc), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Cdouble, Cdouble, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{ComplexF64}),
                cache.ctx, ENVELOPE_KINDS[kind], pv, length(pv), tgate, dt, λf, C_NULL, dJdp, x), cache.ctx)
    return dJdp, x
end

# grape_sensitivity (src/gradient_computations.jl:35-77) on the GPU; the closure dJfinal_dx is
# evaluated here at x[end] and handed over as λ_{Nt+1} (QOC_COST_EXTERNAL).  dUkdp_order = 0 (QOC_DUKDP_EXACT) is the
# exact Fréchet gradient; with this external cost it runs the dense route (the segmented eval and the interpolating
# block propagators of blocks of 5..16 rows take it with the built-in costs, qoc_eval_dev): on generators without
# invariant blocks that the fused gradient kernels fit (N <= 48, m in {1, 2, 4, 8, 16}, nu <= 2) the series kernels,
# one 16-byte readback of the term counts per call, and the block exponentials when the largest count exceeds 48 or
# with QOC_GRAD_EXACT_SERIES=0 (read at qoc_create); exact_series_stats(cache) tells which ran.
function QOC.grape_sensitivity(A0, A::Vector{<:AbstractMatrix}, dJfinal_dx, u, x0, cache::MI355XCache;
                               dUkdp_order=3, dL_dx=nothing)
    # setup_state_penalty's gradient runs on the GPU; nothing clears a penalty left by an earlier call
    # (:47-57 add nothing then); any other closure is evaluated here on every state and the GPU adds
    # dL_dx(x[k]) to λ[k] (qoc_set_costate_source)
    set_penalty!(cache, dL_dx isa PenaltyGrad ? dL_dx : nothing)
    src = nothing
    if !(dL_dx === nothing || dL_dx isa PenaltyGrad)
        xs = cache.x
        src = Array{ComplexF64}(undef, cache.N, cache.m, cache.Nt + 1)
        for k in 1:cache.Nt+1
            src[:, :, k] .= dL_dx(xs[k])
        end
        GC.@preserve src check(ccall((:qoc_set_costate_source, libqoc), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}),
                                     cache.ctx, src), cache.ctx)
    end
    λf = Matrix{ComplexF64}(dJfinal_dx(cache.x[end]))
    rc = ccall((:qoc_grape_sensitivity, libqoc), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{ComplexF64}, Ptr{Float64}),
               cache.ctx, Matrix{Float64}(u), dUkdp_order, λf, cache.dJdu)
    src === nothing || ccall((:qoc_set_costate_source, libqoc), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), cache.ctx, C_NULL)
    check(rc, cache.ctx)   # QOC_ERR_STALE -> "Cache data from other control signal u"
    return cache.dJdu
end

"""What the exact gradient's series route did since the last reset (qoc_exact_series_stats): units processed,
the sum and the largest of their term counts, and the calls that fell back to the block exponential."""
function exact_series_stats(cache::MI355XCache; reset::Bool=false)
    v = zeros(Clonglong, 4)
    check(ccall((:qoc_exact_series_stats, libqoc), Cint, (Ptr{Cvoid}, Ptr{Clonglong}, Cint), cache.ctx, v, reset),
          cache.ctx)
    return (units=v[1], terms=v[2], n_max=v[3], fallbacks=v[4])
end

function set_penalty!(cache::MI355XCache, dL_dx)
    if dL_dx isa PenaltyGrad
        P = Cint.(dL_dx.P .- 1); C = Cint.(dL_dx.C .- 1)
        check(ccall((:qoc_set_state_penalty, libqoc), Cint,
                    (Ptr{Cvoid}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Cdouble),
                    cache.ctx, P, length(P), C, length(C), dL_dx.μ), cache.ctx)
    else
        check(ccall((:qoc_set_state_penalty, libqoc), Cint,
                    (Ptr{Cvoid}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Cdouble),
                    cache.ctx, C_NULL, 0, C_NULL, 0, 0.0), cache.ctx)
    end
end

"""Trace infidelity J = 1 - |tr(X'x)|^2/n^2 and its gradient (src/penalty_fcns.jl:15-24), tagged so that the
GPU path can evaluate them on the device; on host they behave like the reference's closures."""
struct TraceJ
    Xt::Matrix{ComplexF64}
    n::Float64
end
struct TraceGrad
    Xt::Matrix{ComplexF64}
    n::Float64
end
(f::TraceJ)(x) = 1 - abs2(tr(f.Xt' * x)) / f.n^2
(g::TraceGrad)(x) = (-2 * tr(g.Xt' * x) / g.n^2) .* g.Xt
tr(A) = sum(A[i, i] for i in 1:minimum(size(A)))
setup_infidelity(x_target, n=size(x_target, 2)) =
    (TraceJ(Matrix{ComplexF64}(x_target), n), TraceGrad(Matrix{ComplexF64}(x_target), n))

"""z-calibrated infidelity (src/penalty_fcns.jl:27-42): the reference's closures, tagged for the device."""
struct ZCalJ
    Xt::Matrix{ComplexF64}
    J::Any
end
struct ZCalGrad
    Xt::Matrix{ComplexF64}
    dJ::Any
end
(f::ZCalJ)(x) = f.J(x)
(g::ZCalGrad)(x) = g.dJ(x)
function setup_infidelity_zcalibrated(x_target)
    J, dJ = QOC.setup_infidelity_zcalibrated(x_target)
    return ZCalJ(Matrix{ComplexF64}(x_target), J), ZCalGrad(Matrix{ComplexF64}(x_target), dJ)
end

# the reference's "no penalty" pair (examples/zz_coupling_ipopt_exp.jl:46: Returns(0), x -> 0*x)
no_penalty(L) = L === nothing || (L isa Base.Returns && iszero(L.value))

"""Guard-state penalty whose gradient the GPU applies at every slice (src/penalty_fcns.jl:1-11)."""
struct PenaltyGrad
    P::Vector{Int}
    C::Vector{Int}
    μ::Float64
end
(g::PenaltyGrad)(x) = (d = zeros(eltype(x), size(x)); d[g.P, g.C] .= 2g.μ .* x[g.P, g.C]; d)
function setup_state_penalty(inds_penalty, inds_css, μ)
    L, _ = QOC.setup_state_penalty(inds_penalty, inds_css, μ)
    return L, PenaltyGrad(collect(inds_penalty), collect(inds_css), Float64(μ))
end

# x_target / n given with untagged closures: they must be the trace infidelity of x_target (the reference's
# setup_infidelity(x_target, n), src/penalty_fcns.jl:15-24), checked on a probe state.
function check_trace_closures(Jfinal, dJfinal_dx, Xt, nn)
    xp = Xt .+ 0.1 .* cis.(reshape(1:length(Xt), size(Xt)))
    Ω = tr(Xt' * xp)
    Jw, dJw = 1 - abs2(Ω) / nn^2, -2Ω / nn^2 .* Xt
    ok = isapprox(Jfinal(xp), Jw; rtol=1e-12, atol=1e-14) &&
         isapprox(dJfinal_dx(xp), dJw; rtol=1e-12, atol=1e-14)
    ok || error("x_target given but (Jfinal, dJfinal_dx) are not setup_infidelity(x_target, n): pass the " *
                "closures without x_target (host-evaluated cost) or use QOCMI355X.setup_infidelity")
    return nothing
end

"""
    setup_ipopt_callbacks(A0Δt, A1Δt, A2Δt, x0, u_prototype, (Jfinal, dJfinal_dx), (L, dL_dx), B; x_target, n)

GPU version of examples/ipopt_callbacks_exp.jl:1-54: f = Jfinal(x[end]) + sum(L, x) and f_grad = B' dJdu'.
As in the reference, f only propagates (Ipopt's line-search evaluations pay no gradient) and f_grad runs the
sensitivity of the coefficients f last saw, re-propagating first if Ipopt asks for the gradient of new ones.
With the tagged costs of this module (setup_infidelity / setup_infidelity_zcalibrated) and penalty
(setup_state_penalty, or the reference's disabled Returns(0) pair) both run on the device
(`qoc_propagate_spline`, `qoc_sensitivity_spline`).  Any other cost closure is evaluated on
the host at x[end] and handed over as λ_{Nt+1} (QOC_COST_EXTERNAL), exactly as the reference's f / f_grad do;
any other penalty pair is evaluated on the host too: sum(L, x) in f, and dL_dx(x[k]) for every slice added to
the co-states on the device (qoc_set_costate_source).  g / g_jac are the reference's norm constraints.
Returns the same tuple.
"""
function setup_ipopt_callbacks(A0Δt, A1Δt, A2Δt, x0, u_prototype, (Jfinal, dJfinal_dx), (L, dL_dx), B;
                               x_target=nothing, n=nothing)
    nu = size(u_prototype, 1)
    ng = 2
    nx = length(x0)
    nsplines = size(B, 2)
    nc = nu * nsplines
    Nt = size(B, 1)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:qoc_create, libqoc), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, Cint, Cint),
                ref, 0, size(A0Δt, 1), size(x0, 2), nu, Nt, 1, QOC_FP64), C_NULL)
    cache = MI355XCache(ref[], size(A0Δt, 1), size(x0, 2), nu, Nt)
    A = [A1Δt, A2Δt][1:nu]
    upload!(cache, A0Δt, A, complex(x0))
    # penalty: the device applies setup_state_penalty's; the reference's disabled pair adds nothing; any
    # other (L, dL_dx) takes the host path below (sum(L, x) on the host, dL_dx through the co-state source)
    device_penalty = dL_dx isa PenaltyGrad || no_penalty(L)
    set_penalty!(cache, dL_dx isa PenaltyGrad ? dL_dx : nothing)
    # cost: on the device when tagged, else the caller's closures on the host.  The x_target / n keywords name the
    # trace infidelity for callers that pass the reference's own (untagged) setup_infidelity(x_target, n)
    # closures; closures that are not that cost are an error rather than silently replaced by it.
    if Jfinal isa TraceJ || (x_target !== nothing && !(Jfinal isa ZCalJ))
        Xt = Jfinal isa TraceJ ? Jfinal.Xt : Matrix{ComplexF64}(x_target)
        nn = Jfinal isa TraceJ ? Jfinal.n : (n === nothing ? size(Xt, 2) : n)
        Jfinal isa TraceJ || check_trace_closures(Jfinal, dJfinal_dx, Xt, nn)
        kind = QOC_COST_TRACE
    elseif Jfinal isa ZCalJ
        Xt, nn, kind = Jfinal.Xt, 4.0, QOC_COST_ZCAL
    else
        Xt, nn, kind = Matrix{ComplexF64}(undef, 0, 0), 1.0, QOC_COST_EXTERNAL
    end
    check(ccall((:qoc_set_cost, libqoc), Cint, (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Cdouble),
                cache.ctx, kind, kind == QOC_COST_EXTERNAL ? C_NULL : Xt, nn), cache.ctx)
    Bm = Matrix{Float64}(B)
    check(ccall((:qoc_set_spline_basis, libqoc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint),
                cache.ctx, Bm, nsplines), cache.ctx)
    c_prev = fill(NaN, nc)
    J = Ref{Cdouble}(0.0)
    dJdc = zeros(nc)
    on_device = kind != QOC_COST_EXTERNAL && device_penalty
    # f: examples/ipopt_callbacks_exp.jl:11-19 — spline map, propagate, cost; no sensitivity
    propagate!(c) = if on_device
        check(ccall((:qoc_propagate_spline, libqoc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Cdouble}),
                    cache.ctx, c, J), cache.ctx)
    else
        u = Matrix(transpose(Bm * reshape(c, nsplines, nu)))
        x = QOC.propagate(A0Δt, A, u, x0, cache)
        J[] = Jfinal(x[end]) + (no_penalty(L) ? 0.0 : sum(L, x))
    end
    # f_grad: :21-31 — the sensitivity of the last propagated c, mapped to the coefficients (B' dJdu')
    sensitivity!(c) = if on_device
        check(ccall((:qoc_sensitivity_spline, libqoc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Float64}),
                    cache.ctx, c, 3, dJdc), cache.ctx)
    else
        dJdu = QOC.grape_sensitivity(A0Δt, A, dJfinal_dx, cache.u, x0, cache; dUkdp_order=3, dL_dx=dL_dx)
        dJdc .= (Bm' * transpose(dJdu))[:]
    end
    f = function (c::Vector{Float64})
        c_prev .= c
        propagate!(c)
        J[]
    end
    f_grad = function (c, f_grad_out)
        if c_prev != c  # Ipopt asked for the gradient first (:22-25)
            c_prev .= c
            propagate!(c)
        end
        sensitivity!(c)
        f_grad_out .= dJdc
    end
    g_oop = function (c)
        cm = reshape(c, nsplines, nu)
        [sqrt(sum(abs2, cm)); sqrt(sum(abs2, diff(cm, dims=1)))]
    end
    g = (c, g_out) -> (g_out .= g_oop(c))
    function g_jac(c, mode, rows, cols, g_jac_out)
        if mode == :Structure
            cols .= kron(ones(ng), 1:nc)
            rows .= kron(1:ng, ones(nc))
        else
            cm = reshape(c, nsplines, nu)
            g0, g1 = g_oop(c)
            D = zeros(nsplines + 1, nu)
            D[2:nsplines, :] .= diff(cm, dims=1)
            j1 = (D[1:nsplines, :] .- D[2:end, :])[:]
            g_jac_out .= [g0 > 0 ? c ./ g0 : zero(c); g1 > 0 ? j1 ./ g1 : zero(j1)]
        end
    end
    f, g, f_grad, g_jac, nu, ng, nx, nc, cache
end

end # module
