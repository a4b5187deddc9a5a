# HipGPs.jl — Julia host shim: keeps the AbstractGP / FiniteGP / PosteriorGP surface of AbstractGPs.jl
# and routes the logpdf / posterior hot path through `ccall` into libgpmi355.so (include/gpmi355.h, ABI v4).
#
# NOT EXECUTED in the build container (Julia is not installed there — SURVEY.md §0 F3); it is the
# reference-side binding a maintainer adds (INTEGRATION.md).  abstractgps.jl_amd/api.py is its ctypes
# mirror (same entry points, argument meaning and errors) and is what tests/ run.  Reference plug-in point:
# "subtype AbstractGP and implement the FiniteGP primary API" (docs/src/api.md:18-30, 49-73).
#
#   f   = HipGP(GP(SqExponentialKernel()))          # wraps a stock GP              src/base_gp.jl:57-64
#   f8  = HipGP(GP(k), HipContext([0,1,2,3,4,5,6,7])) # same API, fits partitioned over 8 devices inside the library
#   fx  = f(x, 0.01)                                # stock FiniteGP ctor           src/finite_gp_projection.jl:13-37
#   logpdf(fx, y)                                   # -> gp_logpdf                  src/finite_gp_projection.jl:306-311
#   Zygote.gradient(θ -> logpdf(build(θ)(x, σ²), y), θ)   # -> rrule below -> gp_logpdf_grad
#   p   = posterior(fx, y)                          # -> gp_posterior_fit           src/exact_gpr_posterior.jl:29-35
#   mean_and_var(p(xs)); cov(p(xs))                 # -> gp_posterior_predict       src/exact_gpr_posterior.jl:60-90
#   Zygote.gradient(x -> sum(mean(p, x) .+ 2 .* sqrt.(var(p, x))), xs)   # -> rrules -> gp_posterior_predict_grad / gp_vfe_predict_grad
#   logpdf(p(xs, σ²), ys); rand(rng, p(xs, σ²), 3)  # -> gp_posterior_logpdf / gp_posterior_rand   (device, no refit)
#   posterior(VFE(f(z, 1e-6)), fx, y); elbo(...)    # -> gp_vfe_fit / gp_vfe_predict src/sparse_approximations.jl:58-75,248-254
#   Zygote.gradient(θ -> elbo(VFE(build(θ)(z(θ), 1e-6)), build(θ)(x, σ²), y), θ)   # -> rrule -> gp_vfe_fit + gp_vfe_grad
#   update_posterior(pa, fx2, y2); update_posterior(pa, f(z2, 1e-6))   # -> gp_vfe_update / gp_vfe_append   :87-176
module HipGPs

using AbstractGPs
using AbstractGPs: AbstractGP, FiniteGP, GP, ZeroMean, ConstMean, CustomMean, VFE, DTC, mean_vector
using KernelFunctions
using KernelFunctions: SqExponentialKernel, Matern12Kernel, ExponentialKernel, Matern32Kernel, Matern52Kernel,
    TransformedKernel, ScaledKernel, ScaleTransform, ARDTransform, ColVecs, RowVecs
using LinearAlgebra, FillArrays, Statistics, StatsBase, Distributions, Random
using ChainRulesCore

export HipGP, HipPosteriorGP, HipColumnsPosteriorGP, HipApproxPosteriorGP, HipContext, logpdf_and_grad, loo_mean_and_var, loo_logpdf, loo_logpdf_and_grad, loo_logpdf_batch, loo_mean_and_var_batch, loo_logpdf_and_grad_batch, posterior_columns, logpdf_and_grad_columns, elbo_and_grad, HipApproxColumnsPosteriorGP, elbo_columns, approx_log_evidence_columns, elbo_and_grad_columns, objective_grad, columns_data, logpdf_batch, mean_and_var_batch, mean_and_var_grad_batch, joint_batch, mean_and_cov_batch, logpdf_heldout_batch, rand_batch, logpdf_and_grad_batch, BatchPosDefException

const libgpmi355 = get(ENV, "GPMI355_LIB", joinpath(@__DIR__, "..", "csrc", "libgpmi355.so"))

# ---- C structs (include/gpmi355.h) ---------------------------------------------------------------
struct CKernel          # gp_kernel
    kind::Int32
    dtype::Int32
    variance::Float64
    nscale::Int32
    scale::Ptr{Float64}
end
struct CKFactor         # gp_kfactor
    kind::Int32
    nscale::Int32
    scale::Ptr{Float64}
    nparam::Int32
    param::Ptr{Float64}
end
struct CKTerm           # gp_kterm
    variance::Float64
    nfactors::Int32
    factors::Ptr{CKFactor}
end
struct CKSum            # gp_ksum
    dtype::Int32
    nterms::Int32
    terms::Ptr{CKTerm}
end
struct CPoints          # gp_points
    data::Ptr{Cvoid}
    n::Int64
    d::Int32
    layout::Int32
end
struct CNoise           # gp_noise
    kind::Int32
    s::Float64
    diag::Ptr{Cvoid}
end

struct GpmiError <: Exception
    status::Int32
    msg::String
end

# status convention of the ABI: 0 ok; k>0 LAPACK info -> PosDefException(k) exactly like `cholesky`
# at src/finite_gp_projection.jl:308; <0 argument / HIP error with text in gp_last_error().
function check(rc::Int32)
    rc == 0 && return nothing
    rc > 0 && throw(LinearAlgebra.PosDefException(rc))
    msg = unsafe_string(ccall((:gp_last_error, libgpmi355), Cstring, ()))
    rc > -1000 ? throw(ArgumentError(msg)) : throw(GpmiError(rc, msg))
end

# ---- context ---------------------------------------------------------------------------------------
# HipContext(device)                 one GPU
# HipContext(devices; P, Q, nb)      several GPUs of the node driven from this one Julia process (gp_ctx_create_multi):
#                                    fp64 logpdf / posterior fits are partitioned 2D block-cyclically inside the library
mutable struct HipContext
    handle::Ptr{Cvoid}
    function HipContext(device::Integer=0)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:gp_ctx_create, libgpmi355), Int32, (Ref{Ptr{Cvoid}}, Int32, Ptr{Cvoid}), h, device, C_NULL))
        c = new(h[])
        finalizer(c -> ccall((:gp_ctx_destroy, libgpmi355), Int32, (Ptr{Cvoid},), c.handle), c)
        return c
    end
    function HipContext(devices::AbstractVector{<:Integer}; P::Integer=0, Q::Integer=0, nb::Integer=0)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        devs = Vector{Int32}(devices)
        check(ccall((:gp_ctx_create_multi, libgpmi355), Int32, (Ref{Ptr{Cvoid}}, Ptr{Int32}, Int32, Int32, Int32, Int32),
            h, devs, length(devs), P, Q, nb))
        c = new(h[])
        finalizer(c -> ccall((:gp_ctx_destroy, libgpmi355), Int32, (Ptr{Cvoid},), c.handle), c)
        return c
    end
end
const _default_ctx = Ref{Union{Nothing,HipContext}}(nothing)
default_context() = something(_default_ctx[], (_default_ctx[] = HipContext(0)))
set_param!(c::HipContext, name::AbstractString, v::Integer) =
    check(ccall((:gp_ctx_set_param, libgpmi355), Int32, (Ptr{Cvoid}, Cstring, Int64), c.handle, name, v))
function get_param(c::HipContext, name::AbstractString)
    v = Ref{Int64}(0)
    check(ccall((:gp_ctx_get_param, libgpmi355), Int32, (Ptr{Cvoid}, Cstring, Ref{Int64}), c.handle, name, v))
    return v[]
end
trim!(c::HipContext) = check(ccall((:gp_ctx_trim, libgpmi355), Int32, (Ptr{Cvoid},), c.handle))
# multi-device contexts: fit attempts, repetitions after a failed self-check, forward solves on the distributed factor
function multi_stats(c::HipContext)
    f = Ref{Int64}(0); r = Ref{Int64}(0); s = Ref{Int64}(0)
    check(ccall((:gp_ctx_multi_stats, libgpmi355), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), c.handle, f, r, s))
    return (fits=f[], retries=r[], solves=s[])
end

# ---- the GP wrapper -------------------------------------------------------------------------------
struct HipGP{Tg<:GP} <: AbstractGP
    gp::Tg
    ctx::HipContext
end
HipGP(gp::GP) = HipGP(gp, default_context())

# internal AbstractGP API delegates to the wrapped GP (src/base_gp.jl:68-74) so that everything that is not
# accelerated (dense Σy, kernels outside the composite limits, exotic input containers) keeps working through the stock methods.
Statistics.mean(f::HipGP, x::AbstractVector) = mean(f.gp, x)
Statistics.cov(f::HipGP, x::AbstractVector) = cov(f.gp, x)
Statistics.var(f::HipGP, x::AbstractVector) = var(f.gp, x)
Statistics.cov(f::HipGP, x::AbstractVector, y::AbstractVector) = cov(f.gp, x, y)

# ---- kernel -> descriptor (dispatch; anything else falls back) ------------------------------------
kind_of(::SqExponentialKernel) = Int32(0)
kind_of(::ExponentialKernel) = Int32(1)       # Matern12Kernel is an alias
kind_of(::Matern32Kernel) = Int32(2)
kind_of(::Matern52Kernel) = Int32(3)
kind_of(::Any) = nothing

# returns (kind, variance, scales::Vector{Float64}) or nothing if the kernel is not accelerated
descriptor(k) = (kd = kind_of(k); kd === nothing ? nothing : (kd, 1.0, Float64[]))
function descriptor(k::ScaledKernel)
    d = descriptor(k.kernel)
    return d === nothing ? nothing : (d[1], d[2] * only(k.σ²), d[3])
end
function descriptor(k::TransformedKernel{<:Any,<:ScaleTransform})
    d = descriptor(k.kernel)
    (d === nothing || !isempty(d[3])) && return nothing
    return (d[1], d[2], Float64[only(k.transform.s)])
end
function descriptor(k::TransformedKernel{<:Any,<:ARDTransform})
    d = descriptor(k.kernel)
    (d === nothing || !isempty(d[3])) && return nothing
    return (d[1], d[2], Vector{Float64}(k.transform.v))
end

# ---- composite kernels -> normal form Σ_t σ_t² Π_f κ_f (include/gpmi355.h gp_ksum) ------------------------------------
# sum_walk pushes the tree's own parameters into P, depth-first and left to right (ScaledKernel σ², Periodic r, RationalQuadratic α, then the
# transform's s / v), and returns the terms as (variance slots, [(kind, scale slots, param slots)]) — products distributed over sums share
# their slots — or `nothing` for anything the device does not evaluate (the caller then takes the stock path).
kind_of_sum(k) = kind_of(k)
kind_of_sum(::PeriodicKernel) = Int32(4)
kind_of_sum(::RationalQuadraticKernel) = Int32(5)
kind_of_sum(::WhiteKernel) = Int32(6)
base_params(k) = Float64[]
base_params(k::PeriodicKernel) = Vector{Float64}(k.r)
base_params(k::RationalQuadraticKernel) = Float64[only(k.α)]
function sum_walk(k, P)
    kd = kind_of_sum(k)
    kd === nothing && return nothing
    pi = [(push!(P, v); length(P)) for v in base_params(k)]
    return [(Int[], [(kd, Int[], pi)])]
end
function sum_walk(k::ScaledKernel, P)
    push!(P, only(k.σ²)); vi = length(P)
    t = sum_walk(k.kernel, P)
    return t === nothing ? nothing : [([vi; v], f) for (v, f) in t]
end
function sum_walk(k::TransformedKernel{<:Any,<:Union{ScaleTransform,ARDTransform}}, P)
    k.kernel isa WhiteKernel && return sum_walk(k.kernel, P)  # δ(x, x') is unchanged by a nonzero scale: the transform is dropped
    kd = kind_of_sum(k.kernel)
    kd === nothing && return nothing                          # a transform around a sum or product is not accelerated
    pi = [(push!(P, v); length(P)) for v in base_params(k.kernel)]
    sv = k.transform isa ScaleTransform ? Float64[only(k.transform.s)] : Vector{Float64}(k.transform.v)
    si = [(push!(P, v); length(P)) for v in sv]
    return [(Int[], [(kd, si, pi)])]
end
function sum_walk(k::KernelSum, P)
    out = []
    for c in k.kernels
        t = sum_walk(c, P)
        t === nothing && return nothing
        append!(out, t)
    end
    return out
end
function sum_walk(k::KernelProduct, P)
    out = [(Int[], [])]
    for c in k.kernels
        t = sum_walk(c, P)
        t === nothing && return nothing
        out = [([v1; v2], [f1; f2]) for (v1, f1) in out for (v2, f2) in t]
    end
    return out
end
# (P, terms) or nothing (beyond the limits of gp_ksum: the stock path); single-kind kernels keep `descriptor`, which marshal asks first
function sum_descriptor(k)
    P = Float64[]
    t = sum_walk(k, P)
    t === nothing && return nothing
    (length(t) > 8 || any(((_, f),) -> length(f) > 4, t) || sum(((_, f),) -> length(f), t) > 16) && return nothing
    return (P, t)
end
# θ of the C ABI (term by term σ_t², then per factor scale, then param) and the chain rule ∂/∂θ -> ∂/∂P
function sum_theta(P, terms)
    θ = Float64[]
    for (v, f) in terms
        push!(θ, prod(P[v]; init=1.0))
        for (_, s, q) in f
            append!(θ, P[s]); append!(θ, P[q])
        end
    end
    return θ
end
function sum_chain(P, terms, gθ)
    g = zeros(length(P)); j = 1
    for (v, f) in terms
        for a in eachindex(v)
            g[v[a]] += gθ[j] * prod((P[v[b]] for b in eachindex(v) if b != a); init=1.0)
        end
        j += 1
        for (_, s, q) in f, i in [s; q]
            g[i] += gθ[j]; j += 1
        end
    end
    return g
end

# ---- input / noise marshalling ---------------------------------------------------------------------
# layout 0 Vector{T}; 1 ColVecs (D×N column-major); 2 RowVecs (N×D column-major)   src/finite_gp_projection.jl:32-37
# points(x, T) returns (buffer kept alive by the caller, CPoints) in eltype T, converting when needed; `nothing` for
# containers the ABI has no layout for (vector of vectors, ...): the caller then takes the stock path.
const HipFloat = Union{Float32,Float64}
points(x::AbstractVector{<:Real}, ::Type{T}) where {T<:HipFloat} = (b = convert(Vector{T}, x); (b, CPoints(pointer(b), length(b), 1, 0)))
function points(x::ColVecs, ::Type{T}) where {T<:HipFloat}
    b = convert(Matrix{T}, x.X)
    return (b, CPoints(pointer(b), size(b, 2), size(b, 1), 1))
end
function points(x::RowVecs, ::Type{T}) where {T<:HipFloat}
    b = convert(Matrix{T}, x.X)
    return (b, CPoints(pointer(b), size(b, 1), size(b, 2), 2))
end
points(::Any, ::Type) = nothing
# element type of an input container (Float32 in -> Float32 out is a tested reference property,
# test/finite_gp_projection.jl:180-191); anything that is not Float32 computes in Float64
input_eltype(x::AbstractVector{<:Real}) = eltype(x)
input_eltype(x::Union{ColVecs,RowVecs}) = eltype(x.X)
input_eltype(::Any) = Float64
hip_eltype(Ts...) = (T = promote_type(map(t -> t <: AbstractFloat ? t : Float64, Ts)...); T === Float32 ? Float32 : Float64)

noise(Σ::Diagonal{<:Any,<:Fill}, ::Type{T}) where {T} = (nothing, CNoise(0, Float64(FillArrays.getindex_value(Σ.diag)), C_NULL))
function noise(Σ::Diagonal, ::Type{T}) where {T}
    v = Vector{T}(Σ.diag)
    return (v, CNoise(1, 0.0, pointer(v)))
end
# dense Σy (gp_noise kind 2 / 3: ONE triangle of an n×n column-major array is read — include/gpmi355.h): a Matrix{T} goes out as it lies with kind 2
# (its upper triangle, what _symmetric reads, src/util/common_covmat_ops.jl:5); anything else is converted once; the buffer is kept alive across the ccall
# by the callers' GC.@preserve of `nbuf`.  Symmetric(A, uplo): its parent with the triangle it names.
dense_buffer(Σ::Matrix{T}, ::Type{T}) where {T} = Σ
dense_buffer(Σ::AbstractMatrix, ::Type{T}) where {T} = Matrix{T}(Σ)
function noise(Σ::AbstractMatrix{<:Real}, ::Type{T}) where {T}
    size(Σ, 1) == size(Σ, 2) || throw(DimensionMismatch("Σy is $(size(Σ, 1))×$(size(Σ, 2))"))
    b = dense_buffer(Σ, T)
    return (b, CNoise(2, 0.0, pointer(b)))
end
function noise(Σ::Symmetric{<:Real}, ::Type{T}) where {T}
    b = dense_buffer(parent(Σ), T)
    return (b, CNoise(Σ.uplo == 'U' ? 2 : 3, 0.0, pointer(b)))
end
noise(::Any, ::Type) = nothing
is_dense(cn::CNoise) = cn.kind >= 2
# dnoise_out of gp_logpdf_grad / _sum: 1 entry (Fill), n (Diagonal), n×n (dense: G = ½(ααᵀ − C⁻¹), symmetric)
dnoise_buffer(cn::CNoise, ::Type{T}, n) where {T} = cn.kind == 0 ? Vector{T}(undef, 1) : (cn.kind == 1 ? Vector{T}(undef, n) : Matrix{T}(undef, n, n))

prior_mean(f::GP{<:ZeroMean}, x, ::Type{T}) where {T} = nothing
prior_mean(f::GP, x, ::Type{T}) where {T} = Vector{T}(mean_vector(f.mean, x))

# everything one call needs, or `nothing` => use the stock AbstractGPs path.  The compute type follows the reference's
# promotion (src/finite_gp_projection.jl:309): T = promote_type(eltype(x), eltype(Y)), restricted to Float32 / Float64.
function marshal(fx::FiniteGP{<:HipGP}, Ty::Type=input_eltype(fx.x))
    desc = descriptor(fx.f.gp.kernel)
    desc === nothing && return marshal_sum(fx, Ty)
    T = hip_eltype(input_eltype(fx.x), Ty)
    px = points(fx.x, T)
    px === nothing && return nothing
    xbuf, cx = px
    nz = noise(fx.Σy, T)
    nz === nothing && return nothing
    kind, variance, scales = desc
    (length(scales) > 1 && length(scales) != cx.d) &&
        throw(DimensionMismatch("ARDTransform has $(length(scales)) scales, inputs have D=$(cx.d)"))
    ck = CKernel(kind, T === Float64 ? 0 : 1, variance, length(scales), isempty(scales) ? C_NULL : pointer(scales))
    return (; T, xbuf, cx, scales, ck, nbuf=nz[1], cn=nz[2], m=prior_mean(fx.f.gp, fx.x, T))
end
# the same for a composite kernel: `ks` (a CKSum) in place of `ck`, the descriptor's buffers kept alive in `kbuf`
function marshal_sum(fx::FiniteGP{<:HipGP}, Ty::Type)
    sd = sum_descriptor(fx.f.gp.kernel)
    sd === nothing && return nothing
    T = hip_eltype(input_eltype(fx.x), Ty)
    px = points(fx.x, T)
    px === nothing && return nothing
    xbuf, cx = px
    nz = noise(fx.Σy, T)
    nz === nothing && return nothing
    P, terms = sd
    (cx.d > 16 || length(sum_theta(P, terms)) > 64) && return nothing
    kbuf = Any[]
    cterms = CKTerm[]
    for (v, f) in terms
        facs = CKFactor[]
        for (kind, s, q) in f
            sv, qv = P[s], P[q]
            (length(sv) > 1 && length(sv) != cx.d) && throw(DimensionMismatch("ARDTransform has $(length(sv)) scales, inputs have D=$(cx.d)"))
            push!(kbuf, sv, qv)
            push!(facs, CKFactor(kind, length(sv), isempty(sv) ? C_NULL : pointer(sv), length(qv), isempty(qv) ? C_NULL : pointer(qv)))
        end
        push!(kbuf, facs)
        push!(cterms, CKTerm(prod(P[v]; init=1.0), length(facs), pointer(facs)))
    end
    push!(kbuf, cterms)
    ks = CKSum(T === Float64 ? 0 : 1, length(cterms), pointer(cterms))
    return (; T, xbuf, cx, ks, kbuf, P, terms, nbuf=nz[1], cn=nz[2], m=prior_mean(fx.f.gp, fx.x, T))
end
stock(fx::FiniteGP{<:HipGP}) = FiniteGP(fx.f.gp, fx.x, fx.Σy)

# ---- logpdf (src/finite_gp_projection.jl:306-311) -------------------------------------------------
function Distributions.logpdf(fx::FiniteGP{<:HipGP}, Y::AbstractVecOrMat{<:Real})
    a = marshal(fx, eltype(Y))
    a === nothing && return logpdf(stock(fx), Y)
    size(Y, 1) == length(fx) || throw(DimensionMismatch("length(fx) = $(length(fx)) but Y has $(size(Y, 1)) rows"))
    T = a.T
    Yd = Matrix{T}(reshape(Y, size(Y, 1), :))
    out = Vector{T}(undef, size(Yd, 2))
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a Yd out begin
        if haskey(a, :ks)
            check(ccall((:gp_logpdf_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, Yd, size(Yd, 1), size(Yd, 2), out))
        else
            check(ccall((:gp_logpdf, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, Yd, size(Yd, 1), size(Yd, 2), out))
        end
    end
    return Y isa AbstractVector ? out[1] : out
end

# ---- the two terms of logpdf on their own (src/finite_gp_projection.jl:313-337): sqmahal, logdetcov, gradlogpdf ----------------
# ---- many small problems in one call: gp_logpdf_batch / gp_logpdf_batch_sum ---------------------------------------------------
# logpdf_batch(fxs, ys): logpdf(fxs[b], ys[b]) (src/finite_gp_projection.jl:306-311, once per problem) of independent exact GPs — the chains of a
# sampler over hyper-parameters, the starts of a multi-start optimiser, cross-validation folds — in ONE library call per (context, eltype,
# single-kind / composite) group; `ys` is a vector of vectors, or ONE vector shared by all.  The same `x` / `y` object in every entry is sent
# once (nx / ny = 1).  return_alpha = true also returns α_b = C_b \ (y_b − m_b) (src/exact_gpr_posterior.jl:29-35).  on_error = :raise throws the
# PosDefException of the first failing problem (BatchPosDefException carries its index as well); :nan leaves NaN in its place.  A problem the
# ABI has no layout for takes the stock path.
struct BatchPosDefException <: Exception
    info::Int
    index::Int
end
Base.showerror(io::IO, e::BatchPosDefException) =
    print(io, "PosDefException: problem ", e.index, " of the batch is not positive definite; leading minor of order ", e.info)

function logpdf_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys; return_alpha::Bool=false, on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    T = (nb > 0 && all(a -> a !== nothing && a.T === Float32, args)) ? Float32 : Float64
    lp = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    alphas = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        a = args[b]
        if a === nothing  # stock path, one problem at a time
            try
                lp[b] = logpdf(stock(fxs[b]), yv[b])
                return_alpha && (alphas[b] = cholesky(Symmetric(cov(stock(fxs[b])))) \ (yv[b] .- mean(stock(fxs[b]))))
            catch e
                e isa PosDefException || rethrow()
                lp[b] = NaN
                info[b] = e.info
            end
        else
            push!(get!(groups, (fxs[b].f.ctx, a.T, haskey(a, :ks)), Int[]), b)
        end
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        abufs = return_alpha ? [Vector{Tg}(undef, length(fxs[b])) for b in idx] : Vector{Tg}[]
        aptrs = Ptr{Cvoid}[pointer(v) for v in abufs]
        GC.@preserve args ybufs abufs cxs cns yptrs mptrs out inf aptrs begin
            if composite
                ks = [args[b].ks for b in idx]
                GC.@preserve ks check(ccall((:gp_logpdf_batch_sum, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                    ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, return_alpha ? pointer(aptrs) : C_NULL))
            else
                cks = [args[b].ck for b in idx]
                GC.@preserve cks check(ccall((:gp_logpdf_batch, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                    ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, return_alpha ? pointer(aptrs) : C_NULL))
            end
        end
        for (j, b) in enumerate(idx)
            lp[b] = out[j]
            info[b] = inf[j]
            return_alpha && (alphas[b] = abufs[j])
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    return return_alpha ? (lp, alphas) : lp
end

# ---- the predictive half: gp_predict_batch / gp_predict_batch_sum ------------------------------------------------------------------
# mean_and_var_batch(fxs, ys, xs): mean_and_var(posterior(fxs[b], ys[b]), xs[b]) (src/exact_gpr_posterior.jl:29-35, 85-90, once per problem) in ONE
# library call per (context, eltype, single-kind / composite) group.  `xs` is a vector of input containers, one per problem (each with its own
# number of test points, none included), or ONE container shared by all; the same `x` / `y` / `xs` object in every entry is sent once.  what: 1 the
# mean, 2 the variance, 3 both.  Returns the vector of (mean, var) tuples in the caller's order, `nothing` in place of a side that was not asked
# for (with return_logpdf = true: that vector and the logpdfs).  on_error as in logpdf_batch.  A problem the ABI has no layout for takes the stock path.
function mean_and_var_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys, xs; what::Integer=3, return_logpdf::Bool=false, on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    what in (1, 2, 3) || throw(ArgumentError("what must be 1 (mean), 2 (var) or 3 (both)"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    xv = (xs isa ColVecs || xs isa RowVecs || xs isa AbstractVector{<:Real}) ? fill(xs, nb) : collect(xs)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    length(xv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(xv)) sets of test points"))
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    T = (nb > 0 && all(a -> a !== nothing && a.T === Float32, args)) ? Float32 : Float64
    lp = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    means = Vector{Any}(nothing, nb)
    vars = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        a = args[b]
        if a === nothing || points(xv[b], a.T) === nothing  # stock path, one problem at a time
            try
                lp[b] = logpdf(stock(fxs[b]), yv[b])
                m, v = mean_and_var(posterior(stock(fxs[b]), yv[b]), xv[b])
                (what & 1) != 0 && (means[b] = m)
                (what & 2) != 0 && (vars[b] = v)
            catch e
                e isa PosDefException || rethrow()
                lp[b] = NaN
                info[b] = e.info
                (what & 1) != 0 && (means[b] = fill(NaN, length(xv[b])))
                (what & 2) != 0 && (vars[b] = fill(NaN, length(xv[b])))
            end
        else
            push!(get!(groups, (fxs[b].f.ctx, a.T, haskey(a, :ks)), Int[]), b)
        end
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        nxs = all(b -> xv[b] === xv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        xsp = [points(xv[b], Tg) for b in idx[1:nxs]]  # (buffer, CPoints)
        cxss = [p[2] for p in xsp]
        pms = [prior_mean(fxs[b].f.gp, xv[b], Tg) for b in idx]  # m(x*) on the host; nothing = ZeroMean
        pmptrs = Ptr{Cvoid}[m === nothing ? C_NULL : pointer(m) for m in pms]
        mbufs = [Vector{Tg}(undef, (what & 1) != 0 ? length(xv[b]) : 0) for b in idx]
        vbufs = [Vector{Tg}(undef, (what & 2) != 0 ? length(xv[b]) : 0) for b in idx]
        moptrs = Ptr{Cvoid}[pointer(v) for v in mbufs]
        voptrs = Ptr{Cvoid}[pointer(v) for v in vbufs]
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        GC.@preserve args ybufs cxs cns yptrs mptrs xsp cxss pms pmptrs mbufs vbufs moptrs voptrs out inf begin
            if composite
                ks = [args[b].ks for b in idx]
                GC.@preserve ks check(ccall((:gp_predict_batch_sum, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Int32, Ptr{CPoints},
                     Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32}),
                    ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, nxs, cxss, pmptrs, what, (what & 1) != 0 ? pointer(moptrs) : C_NULL,
                    (what & 2) != 0 ? pointer(voptrs) : C_NULL, out, inf))
            else
                cks = [args[b].ck for b in idx]
                GC.@preserve cks check(ccall((:gp_predict_batch, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Int32, Ptr{CPoints},
                     Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32}),
                    ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, nxs, cxss, pmptrs, what, (what & 1) != 0 ? pointer(moptrs) : C_NULL,
                    (what & 2) != 0 ? pointer(voptrs) : C_NULL, out, inf))
            end
        end
        for (j, b) in enumerate(idx)
            lp[b] = out[j]
            info[b] = inf[j]
            (what & 1) != 0 && (means[b] = mbufs[j])
            (what & 2) != 0 && (vars[b] = vbufs[j])
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    pairs = [(means[b], vars[b]) for b in 1:nb]
    return return_logpdf ? (pairs, lp) : pairs
end

# ---- the joint predictive distribution: gp_joint_batch / gp_joint_batch_sum --------------------------------------------------------
# joint_batch(fxs, ys, xs; noise, ys_heldout, xi, what): per problem what posterior(fxs[b], ys[b])(xs[b], noise[b]) answers (src/exact_gpr_posterior.jl:78-83,
# src/finite_gp_projection.jl:133-136, 233-237, 306-311) in ONE library call per (context, eltype, single-kind / composite) group: what bit 1 the mean,
# 4 the latent covariance (mean_and_cov(post, xs[b]): no Σy* added), 8 logpdf(post(xs[b], noise[b]), ys_heldout[b]), 16 the samples
# mean .+ cholesky(cov + noise[b]).L * xi[b] with the caller's standard normals (ns_b × nsamp, one nsamp per call).  noise: nothing (zero), one Real for all,
# or one entry per problem (nothing, a Real, or a covariance matrix over the test points as a FiniteGP holds it).  Returns the vector of
# (mean, cov, heldout_logpdf, samples) tuples in the caller's order, `nothing` for what was not asked for (with return_logpdf = true: that vector and the
# logpdfs).  on_error as in logpdf_batch; a joint covariance that is not positive definite counts as that problem's failure, with mean and cov left valid.
# A problem the ABI has no layout for takes the stock path.
joint_noise(::Nothing, n, ::Type{T}) where {T} = (nothing, CNoise(0, 0.0, C_NULL))
joint_noise(s::Real, n, ::Type{T}) where {T} = (nothing, CNoise(0, Float64(s), C_NULL))
joint_noise(Σ::AbstractMatrix, n, ::Type{T}) where {T} = noise(Σ, T)
stock_noise(::Nothing) = 0.0
stock_noise(s) = s
function joint_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys, xs; noise=nothing, ys_heldout=nothing, xi=nothing,
                     what::Integer=1 | 4 | (ys_heldout === nothing ? 0 : 8) | (xi === nothing ? 0 : 16), return_logpdf::Bool=false, on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    (what > 0 && (what & ~29) == 0) || throw(ArgumentError("what must be a combination of 1 (mean), 4 (cov), 8 (held-out logpdf) and 16 (samples)"))
    ((what & 8) == 0 || ys_heldout !== nothing) || throw(ArgumentError("the held-out logpdf needs ys_heldout"))
    ((what & 16) == 0 || xi !== nothing) || throw(ArgumentError("samples need xi, the standard normals of every problem"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    xv = (xs isa ColVecs || xs isa RowVecs || xs isa AbstractVector{<:Real}) ? fill(xs, nb) : collect(xs)
    nzv = (noise === nothing || noise isa Real) ? fill(noise, nb) : collect(noise)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    length(xv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(xv)) sets of test points"))
    length(nzv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(nzv)) entries of noise"))
    nsamp = (what & 16) != 0 && nb > 0 ? size(xi[1], 2) : 0
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    T = (nb > 0 && all(a -> a !== nothing && a.T === Float32, args)) ? Float32 : Float64
    lp = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    infoj = zeros(Int32, nb)
    means = Vector{Any}(nothing, nb)
    covs = Vector{Any}(nothing, nb)
    hls = Vector{Any}(nothing, nb)
    draws = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        a = args[b]
        ns = length(xv[b])
        if a === nothing || points(xv[b], a.T) === nothing || joint_noise(nzv[b], ns, a.T) === nothing  # stock path, one problem at a time
            try
                lp[b] = logpdf(stock(fxs[b]), yv[b])
                post = posterior(stock(fxs[b]), yv[b])
                m, Cs = mean_and_cov(post, xv[b])
                (what & 1) != 0 && (means[b] = m)
                (what & 4) != 0 && (covs[b] = Cs)
                try
                    fs = post(xv[b], stock_noise(nzv[b]))
                    (what & 8) != 0 && (hls[b] = logpdf(fs, ys_heldout[b]))
                    (what & 16) != 0 && (draws[b] = mean(fs) .+ cholesky(Symmetric(cov(fs))).L * xi[b])
                catch e
                    e isa PosDefException || rethrow()
                    infoj[b] = e.info
                    (what & 8) != 0 && (hls[b] = NaN)
                    (what & 16) != 0 && (draws[b] = fill(NaN, ns, nsamp))
                end
            catch e
                e isa PosDefException || rethrow()
                lp[b] = NaN
                info[b] = e.info
                (what & 1) != 0 && (means[b] = fill(NaN, ns))
                (what & 4) != 0 && (covs[b] = fill(NaN, ns, ns))
                (what & 8) != 0 && (hls[b] = NaN)
                (what & 16) != 0 && (draws[b] = fill(NaN, ns, nsamp))
            end
        else
            push!(get!(groups, (fxs[b].f.ctx, a.T, haskey(a, :ks)), Int[]), b)
        end
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        nxs = all(b -> xv[b] === xv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        xsp = [points(xv[b], Tg) for b in idx[1:nxs]]  # (buffer, CPoints)
        cxss = [p[2] for p in xsp]
        pms = [prior_mean(fxs[b].f.gp, xv[b], Tg) for b in idx]  # m(x*) on the host; nothing = ZeroMean
        pmptrs = Ptr{Cvoid}[m === nothing ? C_NULL : pointer(m) for m in pms]
        nzs = [joint_noise(nzv[b], length(xv[b]), Tg) for b in idx]  # (buffer, CNoise)
        cnzs = [p[2] for p in nzs]
        mbufs = [Vector{Tg}(undef, (what & 1) != 0 ? length(xv[b]) : 0) for b in idx]
        cbufs = [Matrix{Tg}(undef, ((what & 4) != 0 ? (length(xv[b]), length(xv[b])) : (0, 0))...) for b in idx]
        ysbufs = [(what & 8) != 0 ? Vector{Tg}(ys_heldout[b]) : Tg[] for b in idx]
        xibufs = [(what & 16) != 0 ? Matrix{Tg}(reshape(xi[b], length(xv[b]), nsamp)) : Matrix{Tg}(undef, 0, 0) for b in idx]
        sbufs = [Matrix{Tg}(undef, ((what & 16) != 0 ? (length(xv[b]), nsamp) : (0, 0))...) for b in idx]
        for (j, b) in enumerate(idx)
            ((what & 8) == 0 || length(ysbufs[j]) == length(xv[b])) || throw(DimensionMismatch("problem $(b): $(length(xv[b])) test points but ys_heldout has $(length(ysbufs[j])) entries"))
        end
        moptrs = Ptr{Cvoid}[pointer(v) for v in mbufs]
        coptrs = Ptr{Cvoid}[pointer(v) for v in cbufs]
        ysptrs = Ptr{Cvoid}[pointer(v) for v in ysbufs]
        xiptrs = Ptr{Cvoid}[pointer(v) for v in xibufs]
        soptrs = Ptr{Cvoid}[pointer(v) for v in sbufs]
        hl = zeros(Tg, g)
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        infj = zeros(Int32, g)
        GC.@preserve args ybufs cxs cns yptrs mptrs xsp cxss pms pmptrs nzs cnzs mbufs cbufs ysbufs xibufs sbufs moptrs coptrs ysptrs xiptrs soptrs hl out inf infj begin
            if composite
                ks = [args[b].ks for b in idx]
                GC.@preserve ks check(ccall((:gp_joint_batch_sum, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Int32, Ptr{CPoints},
                     Ptr{Ptr{Cvoid}}, Ptr{CNoise}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
                     Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}),
                    ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, nxs, cxss, pmptrs, cnzs, what, (what & 1) != 0 ? pointer(moptrs) : C_NULL,
                    (what & 4) != 0 ? pointer(coptrs) : C_NULL, (what & 8) != 0 ? pointer(ysptrs) : C_NULL, (what & 8) != 0 ? pointer(hl) : C_NULL, nsamp,
                    (what & 16) != 0 ? pointer(xiptrs) : C_NULL, (what & 16) != 0 ? pointer(soptrs) : C_NULL, out, inf, infj))
            else
                cks = [args[b].ck for b in idx]
                GC.@preserve cks check(ccall((:gp_joint_batch, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Int32, Ptr{CPoints},
                     Ptr{Ptr{Cvoid}}, Ptr{CNoise}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
                     Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}),
                    ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, nxs, cxss, pmptrs, cnzs, what, (what & 1) != 0 ? pointer(moptrs) : C_NULL,
                    (what & 4) != 0 ? pointer(coptrs) : C_NULL, (what & 8) != 0 ? pointer(ysptrs) : C_NULL, (what & 8) != 0 ? pointer(hl) : C_NULL, nsamp,
                    (what & 16) != 0 ? pointer(xiptrs) : C_NULL, (what & 16) != 0 ? pointer(soptrs) : C_NULL, out, inf, infj))
            end
        end
        for (j, b) in enumerate(idx)
            lp[b] = out[j]
            info[b] = inf[j]
            infoj[b] = infj[j]
            (what & 1) != 0 && (means[b] = mbufs[j])
            (what & 4) != 0 && (covs[b] = cbufs[j])
            (what & 8) != 0 && (hls[b] = hl[j])
            (what & 16) != 0 && (draws[b] = sbufs[j])
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    badj = findfirst(!=(0), infoj)
    (on_error === :raise && badj !== nothing) && throw(BatchPosDefException(Int(infoj[badj]), badj))
    quads = [(means[b], covs[b], hls[b], draws[b]) for b in 1:nb]
    return return_logpdf ? (quads, lp) : quads
end
mean_and_cov_batch(fxs, ys, xs; kw...) = (r = joint_batch(fxs, ys, xs; what=5, kw...); q = r isa Tuple ? r[1] : r; p = [(t[1], t[2]) for t in q]; r isa Tuple ? (p, r[2]) : p)
logpdf_heldout_batch(fxs, ys, xs, ys_heldout; kw...) = (r = joint_batch(fxs, ys, xs; ys_heldout=ys_heldout, what=8, kw...); q = r isa Tuple ? r[1] : r; p = [t[3] for t in q]; r isa Tuple ? (p, r[2]) : p)
rand_batch(fxs, ys, xs, xi; kw...) = (r = joint_batch(fxs, ys, xs; xi=xi, what=16, kw...); q = r isa Tuple ? r[1] : r; p = [t[4] for t in q]; r isa Tuple ? (p, r[2]) : p)

# ---- gradients of the batched predictions w.r.t. the test inputs: gp_predict_grad_batch / gp_predict_grad_batch_sum ----------------
# mean_and_var_grad_batch(fxs, ys, xs): what mean_and_var_batch returns AND the gradients of both sides w.r.t. the test inputs — a gradient-based
# acquisition step over many independent surrogates — in ONE library call per (context, eltype, single-kind / composite) group.  Arguments as in
# mean_and_var_batch.  Returns the vector of (mean, var, dmean, dvar) tuples in the caller's order, `nothing` for whatever was not asked for; a gradient
# lies in the container layout of its xs (Vector / D×N of ColVecs / N×D of RowVecs), as predict_grad returns it.  The device takes the prior mean as
# constant in x*: the mean side of a CustomMean prior needs its entry of `mean_grads` (a vector with one entry per problem, `nothing` where not needed):
# a function x -> the ns × d derivative of the mean function, which is added to dmean (ArgumentError without it).  Every problem must be one the ABI has
# a layout for (as logpdf_and_grad_batch demands).
grad_plus(x::AbstractVector{<:Real}, dm, g) = dm .+ vec(g)
grad_plus(x::ColVecs, dm, g) = dm .+ permutedims(g)
grad_plus(x::RowVecs, dm, g) = dm .+ g
function mean_and_var_grad_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys, xs; what::Integer=3, mean_grads=nothing, return_logpdf::Bool=false,
                                 on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    what in (1, 2, 3) || throw(ArgumentError("what must be 1 (mean), 2 (var) or 3 (both)"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    xv = (xs isa ColVecs || xs isa RowVecs || xs isa AbstractVector{<:Real}) ? fill(xs, nb) : collect(xs)
    mg = mean_grads === nothing ? fill(nothing, nb) : collect(Any, mean_grads)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    length(xv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(xv)) sets of test points"))
    length(mg) == nb || throw(DimensionMismatch("$(nb) problems but $(length(mg)) entries of mean_grads"))
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    any(a -> a === nothing, args) && throw(ArgumentError("kernel / noise form is not accelerated"))
    T = (nb > 0 && all(a -> a.T === Float32, args)) ? Float32 : Float64
    lp = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    quads = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        points(xv[b], args[b].T) === nothing && throw(ArgumentError("unsupported input container for the test points of problem $(b) (use a Vector, ColVecs or RowVecs)"))
        ((what & 1) != 0 && fxs[b].f.gp.mean isa CustomMean && mg[b] === nothing) &&
            throw(ArgumentError("problem $(b): the prior mean is a CustomMean: pass mean_grads[$(b)] = function returning its ns × d derivative at xs"))
        push!(get!(groups, (fxs[b].f.ctx, args[b].T, haskey(args[b], :ks)), Int[]), b)
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        nxs = all(b -> xv[b] === xv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        xsp = [points(xv[b], Tg) for b in idx[1:nxs]]  # (buffer, CPoints)
        cxss = [p[2] for p in xsp]
        pms = [prior_mean(fxs[b].f.gp, xv[b], Tg) for b in idx]  # m(x*) on the host; nothing = ZeroMean
        pmptrs = Ptr{Cvoid}[m === nothing ? C_NULL : pointer(m) for m in pms]
        mbufs = [Vector{Tg}(undef, (what & 1) != 0 ? length(xv[b]) : 0) for b in idx]
        vbufs = [Vector{Tg}(undef, (what & 2) != 0 ? length(xv[b]) : 0) for b in idx]
        dmbufs = [(what & 1) != 0 ? similar(xsp[nxs == 1 ? 1 : j][1]) : Tg[] for j in 1:g]  # in the container layout of xs
        dvbufs = [(what & 2) != 0 ? similar(xsp[nxs == 1 ? 1 : j][1]) : Tg[] for j in 1:g]
        moptrs = Ptr{Cvoid}[pointer(v) for v in mbufs]
        voptrs = Ptr{Cvoid}[pointer(v) for v in vbufs]
        dmptrs = Ptr{Cvoid}[pointer(v) for v in dmbufs]
        dvptrs = Ptr{Cvoid}[pointer(v) for v in dvbufs]
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        GC.@preserve args ybufs cxs cns yptrs mptrs xsp cxss pms pmptrs mbufs vbufs dmbufs dvbufs moptrs voptrs dmptrs dvptrs out inf begin
            if composite
                ks = [args[b].ks for b in idx]
                GC.@preserve ks check(ccall((:gp_predict_grad_batch_sum, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Int32, Ptr{CPoints},
                     Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32}),
                    ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, nxs, cxss, pmptrs, what, (what & 1) != 0 ? pointer(moptrs) : C_NULL,
                    (what & 2) != 0 ? pointer(voptrs) : C_NULL, (what & 1) != 0 ? pointer(dmptrs) : C_NULL, (what & 2) != 0 ? pointer(dvptrs) : C_NULL,
                    out, inf))
            else
                cks = [args[b].ck for b in idx]
                GC.@preserve cks check(ccall((:gp_predict_grad_batch, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Int32, Ptr{CPoints},
                     Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32}),
                    ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, nxs, cxss, pmptrs, what, (what & 1) != 0 ? pointer(moptrs) : C_NULL,
                    (what & 2) != 0 ? pointer(voptrs) : C_NULL, (what & 1) != 0 ? pointer(dmptrs) : C_NULL, (what & 2) != 0 ? pointer(dvptrs) : C_NULL,
                    out, inf))
            end
        end
        for (j, b) in enumerate(idx)
            lp[b] = out[j]
            info[b] = inf[j]
            dm = (what & 1) != 0 ? dmbufs[j] : nothing
            (dm !== nothing && fxs[b].f.gp.mean isa CustomMean) && (dm = grad_plus(xv[b], dm, Tg.(mg[b](xv[b]))))
            quads[b] = ((what & 1) != 0 ? mbufs[j] : nothing, (what & 2) != 0 ? vbufs[j] : nothing, dm, (what & 2) != 0 ? dvbufs[j] : nothing)
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    return return_logpdf ? (quads, lp) : quads
end

# ---- the training half: gp_logpdf_grad_batch / gp_logpdf_grad_batch_sum ------------------------------------------------------------
# logpdf_and_grad_batch(fxs, ys): value and gradient of logpdf(fxs[b], ys[b]) of independent exact GPs — the starts of a multi-start optimiser, the
# chains of a gradient-based sampler over hyper-parameters, per-fold training — in ONE library call per (context, eltype, single-kind / composite)
# group.  Returns (logpdfs, gradients in the caller's order); a gradient is the named tuple of logpdf_and_grad without `x`: (variance, scale, noise,
# y, mean) for a single-kind kernel, (theta, kernel, noise, y, mean) for a composite one.  on_error as in logpdf_batch; :nan leaves NaN in the logpdf
# and in every gradient entry of a failing problem.  Every problem must be one the ABI has a layout for (as logpdf_and_grad demands).
# wrt_x = true (gp_logpdf_grad_batch_x / gp_logpdf_grad_batch_sum_x): every gradient also carries `x`, ∂/∂x in the container layout of that problem's inputs
# as logpdf_and_grad returns it — what a deep-kernel model behind many small GPs back-propagates; problems sharing one x each get their own gradient.
function logpdf_and_grad_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys; wrt_x::Bool=false, on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    any(a -> a === nothing, args) && throw(ArgumentError("kernel / noise form is not accelerated"))
    T = (nb > 0 && all(a -> a.T === Float32, args)) ? Float32 : Float64
    lp = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    grads = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        push!(get!(groups, (fxs[b].f.ctx, args[b].T, haskey(args[b], :ks)), Int[]), b)
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        dnbufs = [dnoise_buffer(args[b].cn, Tg, length(fxs[b])) for b in idx]
        dybufs = [Vector{Tg}(undef, length(fxs[b])) for b in idx]
        dnptrs = Ptr{Cvoid}[pointer(v) for v in dnbufs]
        dyptrs = Ptr{Cvoid}[pointer(v) for v in dybufs]
        dxbufs = wrt_x ? [similar(args[b].xbuf) for b in idx] : []   # same container layout as the inputs (Vector / D×N / N×D), one per problem
        dxptrs = Ptr{Cvoid}[pointer(v) for v in dxbufs]
        GC.@preserve args ybufs cxs cns yptrs mptrs out inf dnbufs dybufs dnptrs dyptrs dxbufs dxptrs begin
            if composite
                ks = [args[b].ks for b in idx]
                dθs = [zeros(Float64, length(sum_theta(args[b].P, args[b].terms))) for b in idx]
                dθptrs = Ptr{Float64}[pointer(v) for v in dθs]
                if wrt_x
                    GC.@preserve ks dθs dθptrs check(ccall((:gp_logpdf_grad_batch_sum_x, libgpmi355), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                         Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                        ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, dθptrs, dnptrs, dyptrs, dxptrs))
                else
                    GC.@preserve ks dθs dθptrs check(ccall((:gp_logpdf_grad_batch_sum, libgpmi355), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                         Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                        ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, dθptrs, dnptrs, dyptrs))
                end
                for (j, b) in enumerate(idx)
                    grads[b] = (theta=dθs[j], kernel=sum_chain(args[b].P, args[b].terms, dθs[j]), noise=cns[j].kind == 0 ? dnbufs[j][1] : dnbufs[j],
                        y=dybufs[j], mean=-dybufs[j])
                end
            else
                cks = [args[b].ck for b in idx]
                dvars = zeros(Float64, g)
                dss = [zeros(Float64, length(args[b].scales)) for b in idx]
                dsptrs = Ptr{Float64}[isempty(v) ? Ptr{Float64}(C_NULL) : pointer(v) for v in dss]  # NULL where the kernel has no transform
                if wrt_x
                    GC.@preserve cks dvars dss dsptrs check(ccall((:gp_logpdf_grad_batch_x, libgpmi355), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                         Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                        ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, dvars, dsptrs, dnptrs, dyptrs, dxptrs))
                else
                    GC.@preserve cks dvars dss dsptrs check(ccall((:gp_logpdf_grad_batch, libgpmi355), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                         Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                        ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, dvars, dsptrs, dnptrs, dyptrs))
                end
                for (j, b) in enumerate(idx)
                    grads[b] = (variance=dvars[j], scale=dss[j], noise=cns[j].kind == 0 ? dnbufs[j][1] : dnbufs[j], y=dybufs[j], mean=-dybufs[j])
                end
            end
            if wrt_x
                for (j, b) in enumerate(idx)
                    grads[b] = merge(grads[b], (x=dxbufs[j],))
                end
            end
        end
        for (j, b) in enumerate(idx)
            lp[b] = out[j]
            info[b] = inf[j]
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    return lp, grads
end

function logpdf_terms(fx::FiniteGP{<:HipGP}, Y::Union{Nothing,AbstractVecOrMat{<:Real}}; logdet::Bool, sq::Bool)
    a = marshal(fx, Y === nothing ? input_eltype(fx.x) : eltype(Y))
    a === nothing && return nothing
    T = a.T
    Yd = Y === nothing ? nothing : Matrix{T}(reshape(Y, size(Y, 1), :))
    Yd === nothing || size(Yd, 1) == length(fx) || throw(DimensionMismatch("length(fx) = $(length(fx)) but Y has $(size(Yd, 1)) rows"))
    ld = Ref{T}(zero(T))
    out = Vector{T}(undef, Yd === nothing ? 1 : size(Yd, 2))
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a Yd out begin
        if haskey(a, :ks)   # composite kernel
            check(ccall((:gp_logpdf_terms_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, Yd === nothing ? C_NULL : pointer(Yd), length(fx),
                Yd === nothing ? 0 : size(Yd, 2), logdet ? Base.unsafe_convert(Ptr{Cvoid}, ld) : C_NULL, sq ? pointer(out) : C_NULL))
        else
            check(ccall((:gp_logpdf_terms, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, Yd === nothing ? C_NULL : pointer(Yd), length(fx),
                Yd === nothing ? 0 : size(Yd, 2), logdet ? Base.unsafe_convert(Ptr{Cvoid}, ld) : C_NULL, sq ? pointer(out) : C_NULL))
        end
    end
    return (ld[], out)
end
function Distributions.logdetcov(fx::FiniteGP{<:HipGP})                                  # :313
    r = logpdf_terms(fx, nothing; logdet=true, sq=false)
    return r === nothing ? logdetcov(stock(fx)) : r[1]
end
function Distributions.sqmahal(fx::FiniteGP{<:HipGP}, x::AbstractVector)                 # :315-318
    r = logpdf_terms(fx, x; logdet=false, sq=true)
    return r === nothing ? sqmahal(stock(fx), x) : r[2][1]
end
function Distributions.sqmahal(fx::FiniteGP{<:HipGP}, X::AbstractMatrix)                 # :320-323
    r = logpdf_terms(fx, X; logdet=false, sq=true)
    return r === nothing ? sqmahal(stock(fx), X) : r[2]
end
# gradlogpdf(f, x) = C \ (m .- x) (:328-337): −α of the posterior fit; further columns reuse that fit's resident factor
function Distributions.gradlogpdf(fx::FiniteGP{<:HipGP}, x::AbstractVector)
    marshal(fx, eltype(x)) === nothing && return gradlogpdf(stock(fx), x)
    return -posterior(fx, x).data.α
end
function Distributions.gradlogpdf(fx::FiniteGP{<:HipGP}, X::AbstractMatrix)
    a = marshal(fx, eltype(X))
    a === nothing && return gradlogpdf(stock(fx), X)
    post = posterior(fx, X[:, 1])
    T = a.T
    D = a.m === nothing ? Matrix{T}(X) : Matrix{T}(X) .- a.m
    out = similar(D)
    # `post` must outlive the call: its finalizer frees the device factor the solve reads
    GC.@preserve post D out check(ccall((:gp_posterior_solve, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
        getfield(post.data.C, :handle), D, size(D, 2), out))
    finalize(post.data.C)   # an O(n²) device factor: release it now instead of leaving it to the GC
    return -out
end

# ---- value + gradient: one factorisation, C⁻¹ by blocked TRSM + MFMA SYRK, one fused ½Σ(αᵢαⱼ − C⁻¹ᵢⱼ)∂Cᵢⱼ pass ----------
function logpdf_and_grad(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}; wrt_x::Bool=true)
    a = marshal(fx, eltype(y))
    a === nothing && throw(ArgumentError("kernel / noise form is not accelerated"))
    haskey(a, :ks) && return logpdf_and_grad_sum(fx, y, a; wrt_x=wrt_x)
    T = a.T
    yv = Vector{T}(y)
    lp = Ref{T}(zero(T)); dvar = Ref{Float64}(0.0)
    dscale = zeros(Float64, max(length(a.scales), 1))
    dnoise = dnoise_buffer(a.cn, T, length(yv))
    dy = Vector{T}(undef, length(yv))
    dx = wrt_x ? similar(a.xbuf) : T[]                  # same container layout as the inputs (Vector / D×N / N×D)
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a yv dscale dnoise dy dx begin
        check(ccall((:gp_logpdf_grad, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ref{Float64}, Ptr{Float64},
                Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, yv, lp, dvar, dscale, dnoise, dy, wrt_x ? pointer(dx) : C_NULL))
    end
    return lp[], (variance=dvar[], scale=dscale[1:length(a.scales)], noise=a.cn.kind == 0 ? dnoise[1] : dnoise, y=dy, mean=-dy,
        x=wrt_x ? dx : nothing)
end

# composite kernel: `theta` = ∂/∂θ of the C ABI, `kernel` = ∂/∂(the tree's own parameters) in sum_walk's order; with wrt_x the call is
# gp_logpdf_grad_sum_x and `x` = ∂/∂x in the container layout of the inputs, otherwise gp_logpdf_grad_sum
function logpdf_and_grad_sum(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}, a; wrt_x::Bool=true)
    T = a.T
    yv = Vector{T}(y)
    lp = Ref{T}(zero(T))
    dθ = zeros(Float64, length(sum_theta(a.P, a.terms)))
    dnoise = dnoise_buffer(a.cn, T, length(yv))
    dy = Vector{T}(undef, length(yv))
    dx = wrt_x ? similar(a.xbuf) : T[]
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a yv dθ dnoise dy dx begin
        if wrt_x
            check(ccall((:gp_logpdf_grad_sum_x, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, yv, lp, dθ, dnoise, dy, pointer(dx)))
        else
            check(ccall((:gp_logpdf_grad_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, yv, lp, dθ, dnoise, dy))
        end
    end
    return lp[], (theta=dθ, kernel=sum_chain(a.P, a.terms, dθ), noise=a.cn.kind == 0 ? dnoise[1] : dnoise, y=dy, mean=-dy, x=wrt_x ? dx : nothing)
end

# ---- leave-one-out cross-validation (Rasmussen & Williams §5.4.2): gp_loo / gp_loo_grad and their *_sum forms ----------------------------
# loo_terms: (L, ℓ, μ, v) from ONE fit — μ_i, v_i the predictive mean and variance of y_i (its own noise included) given every other
# observation, ℓ_i = log p(y_i | y_−i), L = Σ ℓ_i.
function loo_terms(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real})
    a = marshal(fx, eltype(y))
    a === nothing && throw(ArgumentError("kernel / noise form is not accelerated"))
    T = a.T
    yv = Vector{T}(y)
    n = length(yv)
    val = Ref{T}(zero(T))
    lp = Vector{T}(undef, n); mu = Vector{T}(undef, n); v = Vector{T}(undef, n)
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a yv lp mu v begin
        if haskey(a, :ks)
            check(ccall((:gp_loo_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, yv, val, lp, mu, v))
        else
            check(ccall((:gp_loo, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, yv, val, lp, mu, v))
        end
    end
    return val[], lp, mu, v
end
loo_mean_and_var(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}) = loo_terms(fx, y)[3:4]
function loo_logpdf(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}; pointwise::Bool=false)
    r = loo_terms(fx, y)
    return pointwise ? r[2] : r[1]
end
# value and gradient of loo_logpdf as a training objective: the named tuple of logpdf_and_grad (of logpdf_and_grad_sum for a composite kernel)
function loo_logpdf_and_grad(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}; wrt_x::Bool=false)
    a = marshal(fx, eltype(y))
    a === nothing && throw(ArgumentError("kernel / noise form is not accelerated"))
    T = a.T
    yv = Vector{T}(y)
    val = Ref{T}(zero(T))
    dnoise = dnoise_buffer(a.cn, T, length(yv))
    dy = Vector{T}(undef, length(yv))
    dx = wrt_x ? similar(a.xbuf) : T[]
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    if haskey(a, :ks)
        dθ = zeros(Float64, length(sum_theta(a.P, a.terms)))
        GC.@preserve a yv dθ dnoise dy dx begin
            check(ccall((:gp_loo_grad_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, yv, val, dθ, dnoise, dy, wrt_x ? pointer(dx) : C_NULL))
        end
        return val[], (theta=dθ, kernel=sum_chain(a.P, a.terms, dθ), noise=a.cn.kind == 0 ? dnoise[1] : dnoise, y=dy, mean=-dy, x=wrt_x ? dx : nothing)
    end
    dvar = Ref{Float64}(0.0)
    dscale = zeros(Float64, max(length(a.scales), 1))
    GC.@preserve a yv dscale dnoise dy dx begin
        check(ccall((:gp_loo_grad, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ref{Float64}, Ptr{Float64},
                Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, yv, val, dvar, dscale, dnoise, dy, wrt_x ? pointer(dx) : C_NULL))
    end
    return val[], (variance=dvar[], scale=dscale[1:length(a.scales)], noise=a.cn.kind == 0 ? dnoise[1] : dnoise, y=dy, mean=-dy,
        x=wrt_x ? dx : nothing)
end

# ---- leave-one-out cross-validation of many small problems in one call: gp_loo_batch / gp_loo_grad_batch and their *_sum forms -------
# loo_terms_batch: (L, ℓ, μ, v) of loo_terms for every problem, in ONE library call per (context, eltype, single-kind / composite) group — a grid of
# hyper-parameters scored by its leave-one-out log predictive density.  fxs, ys and on_error as in logpdf_batch; :nan leaves NaN in every output of a
# failing problem.  Every problem must be one the ABI has a layout for.
function loo_terms_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys; on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    any(a -> a === nothing, args) && throw(ArgumentError("kernel / noise form is not accelerated"))
    T = (nb > 0 && all(a -> a.T === Float32, args)) ? Float32 : Float64
    L = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    lps = Vector{Any}(nothing, nb); mus = Vector{Any}(nothing, nb); vs = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        push!(get!(groups, (fxs[b].f.ctx, args[b].T, haskey(args[b], :ks)), Int[]), b)
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        lpbufs = [Vector{Tg}(undef, length(fxs[b])) for b in idx]
        mubufs = [Vector{Tg}(undef, length(fxs[b])) for b in idx]
        vbufs = [Vector{Tg}(undef, length(fxs[b])) for b in idx]
        lpptrs = Ptr{Cvoid}[pointer(v) for v in lpbufs]
        muptrs = Ptr{Cvoid}[pointer(v) for v in mubufs]
        vptrs = Ptr{Cvoid}[pointer(v) for v in vbufs]
        GC.@preserve args ybufs cxs cns yptrs mptrs out inf lpbufs mubufs vbufs lpptrs muptrs vptrs begin
            if composite
                ks = [args[b].ks for b in idx]
                GC.@preserve ks check(ccall((:gp_loo_batch_sum, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                     Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                    ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, lpptrs, muptrs, vptrs))
            else
                cks = [args[b].ck for b in idx]
                GC.@preserve cks check(ccall((:gp_loo_batch, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                     Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                    ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, lpptrs, muptrs, vptrs))
            end
        end
        for (j, b) in enumerate(idx)
            L[b] = out[j]
            info[b] = inf[j]
            lps[b] = lpbufs[j]; mus[b] = mubufs[j]; vs[b] = vbufs[j]
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    return L, lps, mus, vs
end
loo_mean_and_var_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys; on_error::Symbol=:raise) = loo_terms_batch(fxs, ys; on_error=on_error)[3:4]
function loo_logpdf_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys; pointwise::Bool=false, on_error::Symbol=:raise)
    r = loo_terms_batch(fxs, ys; on_error=on_error)
    return pointwise ? (r[1], r[2]) : r[1]
end

# loo_logpdf_and_grad_batch(fxs, ys): value and gradient of loo_logpdf(fxs[b], ys[b]) in ONE library call per group; arguments and result as
# logpdf_and_grad_batch, the gradients those of loo_logpdf_and_grad.  With wrt_x = true every problem of the call runs on the single path inside the
# library (the batch kernels have no ∂/∂x yet).
function loo_logpdf_and_grad_batch(fxs::AbstractVector{<:FiniteGP{<:HipGP}}, ys; wrt_x::Bool=false, on_error::Symbol=:raise)
    on_error in (:raise, :nan) || throw(ArgumentError("on_error must be :raise or :nan"))
    nb = length(fxs)
    yv = (ys isa AbstractVector{<:Real}) ? fill(ys, nb) : collect(ys)
    length(yv) == nb || throw(DimensionMismatch("$(nb) problems but $(length(yv)) observation vectors"))
    args = [marshal(fxs[b], eltype(yv[b])) for b in 1:nb]
    any(a -> a === nothing, args) && throw(ArgumentError("kernel / noise form is not accelerated"))
    T = (nb > 0 && all(a -> a.T === Float32, args)) ? Float32 : Float64
    L = Vector{T}(undef, nb)
    info = zeros(Int32, nb)
    grads = Vector{Any}(nothing, nb)
    groups = Dict{Any,Vector{Int}}()
    for b in 1:nb
        length(yv[b]) == length(fxs[b]) || throw(DimensionMismatch("problem $(b): length(fx) = $(length(fxs[b])) but y has $(length(yv[b])) entries"))
        push!(get!(groups, (fxs[b].f.ctx, args[b].T, haskey(args[b], :ks)), Int[]), b)
    end
    for ((ctx, Tg, composite), idx) in groups
        g = length(idx)
        nx = all(b -> fxs[b].x === fxs[idx[1]].x, idx) ? 1 : g
        ny = all(b -> yv[b] === yv[idx[1]], idx) ? 1 : g
        cxs = [args[b].cx for b in idx[1:nx]]
        cns = [args[b].cn for b in idx]
        ybufs = [Vector{Tg}(yv[b]) for b in idx[1:ny]]
        yptrs = Ptr{Cvoid}[pointer(v) for v in ybufs]
        mptrs = Ptr{Cvoid}[args[b].m === nothing ? C_NULL : pointer(args[b].m) for b in idx]
        out = Vector{Tg}(undef, g)
        inf = zeros(Int32, g)
        dnbufs = [dnoise_buffer(args[b].cn, Tg, length(fxs[b])) for b in idx]
        dybufs = [Vector{Tg}(undef, length(fxs[b])) for b in idx]
        dnptrs = Ptr{Cvoid}[pointer(v) for v in dnbufs]
        dyptrs = Ptr{Cvoid}[pointer(v) for v in dybufs]
        dxbufs = wrt_x ? [similar(args[b].xbuf) for b in idx] : []   # same container layout as the inputs (Vector / D×N / N×D), one per problem
        dxptrs = Ptr{Cvoid}[pointer(v) for v in dxbufs]
        GC.@preserve args ybufs cxs cns yptrs mptrs out inf dnbufs dybufs dnptrs dyptrs dxbufs dxptrs begin
            if composite
                ks = [args[b].ks for b in idx]
                dθs = [zeros(Float64, length(sum_theta(args[b].P, args[b].terms))) for b in idx]
                dθptrs = Ptr{Float64}[pointer(v) for v in dθs]
                GC.@preserve ks dθs dθptrs check(ccall((:gp_loo_grad_batch_sum, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKSum}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                     Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                    ctx.handle, g, ks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, dθptrs, dnptrs, dyptrs, wrt_x ? pointer(dxptrs) : C_NULL))
                for (j, b) in enumerate(idx)
                    grads[b] = (theta=dθs[j], kernel=sum_chain(args[b].P, args[b].terms, dθs[j]), noise=cns[j].kind == 0 ? dnbufs[j][1] : dnbufs[j],
                        y=dybufs[j], mean=-dybufs[j], x=wrt_x ? dxbufs[j] : nothing)
                end
            else
                cks = [args[b].ck for b in idx]
                dvars = zeros(Float64, g)
                dss = [zeros(Float64, length(args[b].scales)) for b in idx]
                dsptrs = Ptr{Float64}[isempty(v) ? Ptr{Float64}(C_NULL) : pointer(v) for v in dss]  # NULL where the kernel has no transform
                GC.@preserve cks dvars dss dsptrs check(ccall((:gp_loo_grad_batch, libgpmi355), Int32,
                    (Ptr{Cvoid}, Int32, Ptr{CKernel}, Int32, Ptr{CPoints}, Ptr{CNoise}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Int32},
                     Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                    ctx.handle, g, cks, nx, cxs, cns, mptrs, ny, yptrs, out, inf, dvars, dsptrs, dnptrs, dyptrs, wrt_x ? pointer(dxptrs) : C_NULL))
                for (j, b) in enumerate(idx)
                    grads[b] = (variance=dvars[j], scale=dss[j], noise=cns[j].kind == 0 ? dnbufs[j][1] : dnbufs[j], y=dybufs[j], mean=-dybufs[j],
                        x=wrt_x ? dxbufs[j] : nothing)
                end
            end
        end
        for (j, b) in enumerate(idx)
            L[b] = out[j]
            info[b] = inf[j]
        end
    end
    bad = findfirst(!=(0), info)
    (on_error === :raise && bad !== nothing) && throw(BatchPosDefException(Int(info[bad]), bad))
    return L, grads
end

# ---- reverse-mode rule: Zygote / any ChainRules-based AD differentiates THROUGH the ccall -----------------------------------
# The reference's users differentiate logpdf by AD (test/finite_gp_projection.jl:152-178, test/mean_function.jl:38-56,
# examples/1-mauna-loa/script.jl:201-240); a ccall is opaque to AD, so the accelerated logpdf carries its own pullback built
# from gp_logpdf_grad (gp_logpdf_grad_sum_x for a composite kernel).  Tangents are structural, mirroring how `descriptor` walks the kernel:
#   ScaledKernel.σ²  (1-vector)  <- ∂/∂variance · (total variance / σ²)      TransformedKernel.transform.s / .v  <- ∂/∂scale
#   ConstMean.c <- Σ_i α_i        FiniteGP.Σy (Diagonal{Fill} value / Diagonal diag) <- ∂/∂σ² / ½(α_i² − C⁻¹_ii)        y <- −α
#   x (Vector / ColVecs.X / RowVecs.X) <- ∂/∂x, the input gradient a deep-kernel model back-propagates into its feature map
# CustomMean parameters are not differentiated here (@not_implemented); the prior mean is taken as constant in x.
kernel_tangent(k, dvar, variance, dscale) = NoTangent()
function kernel_tangent(k::ScaledKernel, dvar, variance, dscale)
    σ² = only(k.σ²)
    return Tangent{typeof(k)}(; kernel=kernel_tangent(k.kernel, dvar, variance, dscale), σ²=[dvar * variance / σ²])
end
function kernel_tangent(k::TransformedKernel{<:Any,<:ScaleTransform}, dvar, variance, dscale)
    return Tangent{typeof(k)}(; kernel=kernel_tangent(k.kernel, dvar, variance, dscale),
        transform=Tangent{typeof(k.transform)}(; s=[dscale[1]]))
end
function kernel_tangent(k::TransformedKernel{<:Any,<:ARDTransform}, dvar, variance, dscale)
    return Tangent{typeof(k)}(; kernel=kernel_tangent(k.kernel, dvar, variance, dscale),
        transform=Tangent{typeof(k.transform)}(; v=collect(dscale)))
end
# composite kernels: ∂/∂(the tree's own parameters) handed out node by node, in sum_walk's order (KernelSum / KernelProduct: a tuple of tangents)
sum_tangent(k, g, pos) = NoTangent()
function sum_tangent(k::ScaledKernel, g, pos)
    d = g[pos[]]; pos[] += 1
    return Tangent{typeof(k)}(; kernel=sum_tangent(k.kernel, g, pos), σ²=[d])
end
function sum_tangent(k::PeriodicKernel, g, pos)
    n = length(k.r); d = g[pos[]:pos[]+n-1]; pos[] += n
    return Tangent{typeof(k)}(; r=d)
end
function sum_tangent(k::RationalQuadraticKernel, g, pos)
    d = g[pos[]]; pos[] += 1
    return Tangent{typeof(k)}(; α=[d])
end
sum_tangent(k::WhiteKernel, g, pos) = NoTangent()
function sum_tangent(k::TransformedKernel{<:Any,<:Union{ScaleTransform,ARDTransform}}, g, pos)
    k.kernel isa WhiteKernel && return NoTangent()
    dk = sum_tangent(k.kernel, g, pos)
    if k.transform isa ScaleTransform
        dt = Tangent{typeof(k.transform)}(; s=[g[pos[]]]); pos[] += 1
    else
        n = length(k.transform.v); dt = Tangent{typeof(k.transform)}(; v=g[pos[]:pos[]+n-1]); pos[] += n
    end
    return Tangent{typeof(k)}(; kernel=dk, transform=dt)
end
sum_tangent(k::Union{KernelSum,KernelProduct}, g, pos) = Tangent{typeof(k)}(; kernels=Tuple(sum_tangent(c, g, pos) for c in k.kernels))
mean_tangent(::ZeroMean, dm) = NoTangent()
mean_tangent(m::ConstMean, dm) = Tangent{typeof(m)}(; c=sum(dm))
mean_tangent(m, dm) = ChainRulesCore.@not_implemented("HipGPs: gradients w.r.t. CustomMean parameters go through the stock path")
input_tangent(x::AbstractVector{<:Real}, dx, Δ) = Δ .* dx
input_tangent(x::ColVecs, dx, Δ) = Tangent{typeof(x)}(; X=Δ .* dx)
input_tangent(x::RowVecs, dx, Δ) = Tangent{typeof(x)}(; X=Δ .* dx)
noise_tangent(Σ::Diagonal{<:Any,<:Fill}, dn) = Tangent{typeof(Σ)}(; diag=Tangent{typeof(Σ.diag)}(; value=dn))
noise_tangent(Σ::Diagonal, dn) = Tangent{typeof(Σ)}(; diag=dn)
# dense Σy: the library returns G = ½(ααᵀ − C⁻¹) with d logpdf = ⟨G, dΣy⟩ for symmetric dΣy — the natural tangent of a matrix that is read through Symmetric
noise_tangent(Σ::Matrix, dn) = dn
noise_tangent(Σ::Symmetric, dn) = Tangent{typeof(Σ)}(; data=dn)
noise_tangent(Σ::AbstractMatrix, dn) = dn

function ChainRulesCore.rrule(config::RuleConfig{>:HasReverseMode}, ::typeof(Distributions.logpdf), fx::FiniteGP{<:HipGP},
    y::AbstractVector{<:Real})
    desc = descriptor(fx.f.gp.kernel)
    if marshal(fx, eltype(y)) === nothing   # not accelerated: the stock path keeps its own AD (composite kernels: sum_tangent below)
        lp0, back = rrule_via_ad(config, (g_, x_, Σ_, y_) -> logpdf(FiniteGP(g_, x_, Σ_), y_), fx.f.gp, fx.x, fx.Σy, y)
        return lp0, function (Δ)
            _, dg, dx, dΣ, dy = back(Δ)
            return NoTangent(), Tangent{typeof(fx)}(; f=Tangent{typeof(fx.f)}(; gp=dg, ctx=NoTangent()), x=dx, Σy=dΣ), dy
        end
    end
    lp, g = logpdf_and_grad(fx, y)
    function logpdf_hip_pullback(Δ)
        Δr = unthunk(Δ)
        gp = fx.f.gp
        dk = desc === nothing ? sum_tangent(gp.kernel, Δr .* g.kernel, Ref(1)) : kernel_tangent(gp.kernel, Δr * g.variance, desc[2], Δr .* g.scale)
        dgp = Tangent{typeof(gp)}(; mean=mean_tangent(gp.mean, Δr .* g.mean), kernel=dk)
        df = Tangent{typeof(fx.f)}(; gp=dgp, ctx=NoTangent())
        dfx = Tangent{typeof(fx)}(; f=df, x=input_tangent(fx.x, g.x, Δr), Σy=noise_tangent(fx.Σy, Δr .* g.noise))
        return NoTangent(), dfx, Δr .* g.y
    end
    return lp, logpdf_hip_pullback
end

# ---- posterior (src/exact_gpr_posterior.jl:29-35) -------------------------------------------------
mutable struct DeviceCholesky          # stands where `C::Cholesky` sits in PosteriorGP.data (:34)
    handle::Ptr{Cvoid}
    n::Int
    T::DataType
end
# C.U on the host (parity / debugging): N×N copy
function Base.getproperty(C::DeviceCholesky, s::Symbol)
    s === :U || return getfield(C, s)
    U = Matrix{C.T}(undef, C.n, C.n)
    check(ccall((:gp_posterior_get_factor, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), getfield(C, :handle), U))
    return UpperTriangular(U)
end
# `C \ B` of user code (what `post.data.C \ v` does on a LinearAlgebra.Cholesky): forward + backward sweeps over the resident factor —
# on the block-cyclic pieces when the factor comes from a multi-device fit (gp_posterior_solve)
function Base.:\(C::DeviceCholesky, B::AbstractVecOrMat{<:Real})
    size(B, 1) == getfield(C, :n) || throw(DimensionMismatch("C is $(getfield(C, :n))×$(getfield(C, :n)), B has $(size(B, 1)) rows"))
    T = getfield(C, :T)
    D = Matrix{T}(reshape(B, size(B, 1), :))
    out = similar(D)
    GC.@preserve D out check(ccall((:gp_posterior_solve, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
        getfield(C, :handle), D, size(D, 2), out))
    return B isa AbstractVector ? vec(out) : out
end
# logdet(post.data.C) (what src/finite_gp_projection.jl:310 does with its Cholesky): kept from the fit, no sweep over the factor
function LinearAlgebra.logdet(C::DeviceCholesky)
    out = Ref{Float64}(0.0)
    GC.@preserve C check(ccall((:gp_posterior_logdet, libgpmi355), Int32, (Ptr{Cvoid}, Ref{Float64}), getfield(C, :handle), out))
    return convert(getfield(C, :T), out[])
end
function device_cholesky(h::Ptr{Cvoid}, n::Int, ::Type{T}) where {T}
    C = DeviceCholesky(h, n, T)
    finalizer(c -> ccall((:gp_posterior_free, libgpmi355), Int32, (Ptr{Cvoid},), getfield(c, :handle)), C)
    return C
end

struct HipPosteriorGP{Tprior<:HipGP,Tdata} <: AbstractGP
    prior::Tprior
    data::Tdata                        # (α, C::DeviceCholesky, x, δ) — same field names as the reference (:34)
    logpdf_value::Float64              # logpdf(fx, y) from the same factorisation
end

function AbstractGPs.posterior(fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real})
    a = marshal(fx, eltype(y))
    a === nothing && return posterior(stock(fx), y)
    length(y) == length(fx) || throw(DimensionMismatch("length(fx) != length(y)"))
    T = a.T
    yv = Vector{T}(y)
    δ = a.m === nothing ? copy(yv) : yv - a.m
    α = Vector{T}(undef, length(yv))
    lp = Ref{T}(zero(T))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a yv α begin
        if haskey(a, :ks)   # a composite kernel: the handle keeps it, every posterior method below works on it unchanged
            check(ccall((:gp_posterior_fit_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ref{T}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, yv, h, α, lp))
        else
            check(ccall((:gp_posterior_fit, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ref{T}),
                fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, yv, h, α, lp))
        end
    end
    return HipPosteriorGP(fx.f, (α=α, C=device_cholesky(h[], length(yv), T), x=fx.x, δ=δ), Float64(lp[]))
end

# inputs / noise of a FiniteGP over one of the posterior types, in the posterior's element type
function joint_args(fx::FiniteGP, gp::GP, ::Type{T}) where {T}
    px = points(fx.x, T)
    px === nothing && throw(ArgumentError("unsupported input container for the accelerated posterior (use a Vector, ColVecs or RowVecs)"))
    nz = noise(fx.Σy, T)
    nz === nothing && throw(ArgumentError("this form of Σy is not accelerated"))
    return px[1], px[2], nz[1], nz[2], prior_mean(gp, fx.x, T)
end

# ---- sequential conditioning (src/exact_gpr_posterior.jl:46-56; update_chol src/util/common_covmat_ops.jl:38-42) ----
function AbstractGPs.posterior(fx::FiniteGP{<:HipPosteriorGP}, y::AbstractVector{<:Real})
    post = fx.f
    T = getfield(post.data.C, :T)
    xbuf, cx, nbuf, cn, m2 = joint_args(fx, post.prior.gp, T)
    δ2 = m2 === nothing ? Vector{T}(y) : Vector{T}(y) - m2                 # :48-49
    δ = vcat(post.data.δ, δ2)                                              # :52
    α = Vector{T}(undef, length(δ))
    lp = Ref{T}(zero(T))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve xbuf nbuf δ α begin
        check(ccall((:gp_posterior_update, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ref{T}),
            getfield(post.data.C, :handle), cx, cn, δ, h, α, lp))
    end
    return HipPosteriorGP(post.prior, (α=α, C=device_cholesky(h[], length(δ), T), x=vcat(post.data.x, fx.x), δ=δ), Float64(lp[]))   # :54-55
end

# ---- sampling (src/finite_gp_projection.jl:233-237, 271-277): m .+ C.U' * randn(rng, n, N), factor and product on the device ----
function Random.rand(rng::Random.AbstractRNG, fx::FiniteGP{<:HipGP}, N::Int)
    a = marshal(fx)
    a === nothing && return rand(rng, stock(fx), N)
    T = a.T
    p0 = posterior(FiniteGP(HipGP(GP(fx.f.gp.kernel), fx.f.ctx), fx.x, fx.Σy), zeros(T, length(fx)))   # factor of cov(fx)
    ξ = randn(rng, T, length(fx), N)
    out = similar(ξ)
    GC.@preserve ξ out check(ccall((:gp_posterior_factor_mul, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
        getfield(p0.data.C, :handle), ξ, N, out))
    return mean(fx) .+ out
end
Random.rand(rng::Random.AbstractRNG, fx::FiniteGP{<:HipGP}) = vec(rand(rng, fx, 1))
Random.rand(fx::FiniteGP{<:HipGP}, N::Int) = rand(Random.default_rng(), fx, N)
Random.rand(fx::FiniteGP{<:HipGP}) = rand(Random.default_rng(), fx)

post_handle(f::HipPosteriorGP) = (getfield(f.data.C, :handle), getfield(f.data.C, :T), :gp_posterior_logpdf, :gp_posterior_rand)

# logpdf(post(x*, Σy*), Y*) and rand(post(x*, Σy*)) — the FiniteGP-over-posterior path of the reference (mean_and_cov of the
# posterior + Σy*, cholesky, logdet/_sqmahal or m + U'ξ) as ONE device call each; nothing is refitted
function joint_logpdf(f, fx::FiniteGP, Y::AbstractVecOrMat{<:Real})
    h, T, sym_lp, _ = post_handle(f)
    size(Y, 1) == length(fx) || throw(DimensionMismatch("length(fx) = $(length(fx)) but Y has $(size(Y, 1)) rows"))
    xbuf, cx, nbuf, cn, pm = joint_args(fx, f.prior.gp, T)
    Yd = Matrix{T}(reshape(Y, size(Y, 1), :))
    out = Vector{T}(undef, size(Yd, 2))
    GC.@preserve xbuf nbuf pm Yd out begin
        rc = sym_lp === :gp_posterior_logpdf ?
            ccall((:gp_posterior_logpdf, libgpmi355), Int32, (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Ref{CNoise}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}),
                h, cx, pm === nothing ? C_NULL : pointer(pm), cn, Yd, size(Yd, 1), size(Yd, 2), out) :
            ccall((:gp_vfe_logpdf, libgpmi355), Int32, (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Ref{CNoise}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}),
                h, cx, pm === nothing ? C_NULL : pointer(pm), cn, Yd, size(Yd, 1), size(Yd, 2), out)
        check(rc)
    end
    return Y isa AbstractVector ? out[1] : out
end
function joint_rand!(rng::Random.AbstractRNG, f, fx::FiniteGP, out::AbstractVecOrMat{<:Real})
    h, T, _, sym_r = post_handle(f)
    size(out, 1) == length(fx) || throw(DimensionMismatch("length(fx) = $(length(fx)) but the output has $(size(out, 1)) rows"))
    xbuf, cx, nbuf, cn, pm = joint_args(fx, f.prior.gp, T)
    N = size(out, 2)
    ξ = randn(rng, T, length(fx), N)
    res = Matrix{T}(undef, length(fx), N)
    GC.@preserve xbuf nbuf pm ξ res begin
        rc = sym_r === :gp_posterior_rand ?
            ccall((:gp_posterior_rand, libgpmi355), Int32, (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Ref{CNoise}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
                h, cx, pm === nothing ? C_NULL : pointer(pm), cn, ξ, N, res) :
            ccall((:gp_vfe_rand, libgpmi355), Int32, (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Ref{CNoise}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
                h, cx, pm === nothing ? C_NULL : pointer(pm), cn, ξ, N, res)
        check(rc)
    end
    out .= reshape(res, size(out))
    return out
end

# ---- predictive methods (src/exact_gpr_posterior.jl:60-90) ----------------------------------------
function predict(f::HipPosteriorGP, x::AbstractVector, what::Integer)
    T = getfield(f.data.C, :T)
    px = points(x, T)
    px === nothing && throw(ArgumentError("unsupported input container for the accelerated posterior (use a Vector, ColVecs or RowVecs)"))
    xbuf, cx = px
    ns = length(x)
    pm = prior_mean(f.prior.gp, x, T)
    m = (what & 1) != 0 ? Vector{T}(undef, ns) : T[]
    v = (what & 2) != 0 ? Vector{T}(undef, ns) : T[]
    c = (what & 4) != 0 ? Matrix{T}(undef, ns, ns) : Matrix{T}(undef, 0, 0)
    GC.@preserve xbuf pm m v c begin
        check(ccall((:gp_posterior_predict, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            getfield(f.data.C, :handle), cx, pm === nothing ? C_NULL : pointer(pm), what, m, v, c))
    end
    return m, v, c
end
Statistics.mean(f::HipPosteriorGP, x::AbstractVector) = predict(f, x, 1)[1]            # :60-62
Statistics.var(f::HipPosteriorGP, x::AbstractVector) = predict(f, x, 2)[2]             # :68-70
Statistics.cov(f::HipPosteriorGP, x::AbstractVector) = predict(f, x, 4)[3]             # :64-66
StatsBase.mean_and_var(f::HipPosteriorGP, x::AbstractVector) = predict(f, x, 3)[1:2]   # :85-90
function StatsBase.mean_and_cov(f::HipPosteriorGP, x::AbstractVector)                  # :78-83
    m, _, c = predict(f, x, 5)
    return m, c
end
function Statistics.cov(f::HipPosteriorGP, x::AbstractVector, z::AbstractVector)       # :72-76
    c = predict(f, vcat(x, z), 4)[3]
    return c[1:length(x), (length(x) + 1):end]
end

# ---- one factorisation for a matrix of observations (include/gpmi355.h "columns") ------------------
# S = size(Y, 2) <= 128 GPs that share x, kernel, Σy and the prior mean and differ in y: posterior_columns(fx, Y) fits them with ONE Gram assembly and ONE
# factorisation (gp_posterior_fit_cols), mean(f, x) is length(x)×S from ONE kernel launch (gp_posterior_predict_cols: K_*x evaluated once for all columns),
# var / cov do not depend on y.  logpdf_and_grad_columns(fx, Y) returns logpdf(fx, Y) (length S) and the gradient of its SUM (gp_logpdf_grad_cols).
const COLS_MAX = 128                   # GPMI355_COLS_MAX
struct HipColumnsPosteriorGP{Tprior<:HipGP,Tdata} <: AbstractGP
    prior::Tprior
    data::Tdata                        # (α (n×S), C::DeviceCholesky, x, δ (n×S))
    logpdf_values::Vector{Float64}     # logpdf(fx, Y) from the same factorisation
end

function columns_args(fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real})
    a = marshal(fx, eltype(Y))
    a === nothing && throw(ArgumentError("kernel / noise form is not accelerated"))
    size(Y, 1) == length(fx) || throw(DimensionMismatch("length(fx) = $(length(fx)) but Y has $(size(Y, 1)) rows"))
    1 <= size(Y, 2) <= COLS_MAX || throw(ArgumentError("$(size(Y, 2)) columns: 1..$COLS_MAX fit one call, split them into groups"))
    return a, Matrix{a.T}(Y)
end

function posterior_columns(fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real})
    a, Yv = columns_args(fx, Y)
    T = a.T
    n, S = size(Yv)
    δ = a.m === nothing ? copy(Yv) : Yv .- a.m
    α = Matrix{T}(undef, n, S)
    lp = Vector{T}(undef, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a Yv α lp begin
        if haskey(a, :ks)
            check(ccall((:gp_posterior_fit_cols_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, Yv, n, S, h, α, lp))
        else
            check(ccall((:gp_posterior_fit_cols, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}),
                fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, Yv, n, S, h, α, lp))
        end
    end
    return HipColumnsPosteriorGP(fx.f, (α=α, C=device_cholesky(h[], n, T), x=fx.x, δ=δ), Vector{Float64}(lp))
end

function ncolumns(f::HipColumnsPosteriorGP)
    out = Ref{Int32}(0)
    check(ccall((:gp_posterior_ncols, libgpmi355), Int32, (Ptr{Cvoid}, Ref{Int32}), getfield(f.data.C, :handle), out))
    return Int(out[])
end

function predict(f::HipColumnsPosteriorGP, x::AbstractVector, what::Integer)
    T = getfield(f.data.C, :T)
    px = points(x, T)
    px === nothing && throw(ArgumentError("unsupported input container for the accelerated posterior (use a Vector, ColVecs or RowVecs)"))
    xbuf, cx = px
    ns = length(x)
    pm = prior_mean(f.prior.gp, x, T)
    m = (what & 1) != 0 ? Matrix{T}(undef, ns, size(f.data.α, 2)) : Matrix{T}(undef, 0, 0)
    v = (what & 2) != 0 ? Vector{T}(undef, ns) : T[]
    c = (what & 4) != 0 ? Matrix{T}(undef, ns, ns) : Matrix{T}(undef, 0, 0)
    GC.@preserve xbuf pm m v c begin
        check(ccall((:gp_posterior_predict_cols, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            getfield(f.data.C, :handle), cx, pm === nothing ? C_NULL : pointer(pm), what, m, v, c))
    end
    return m, v, c
end
Statistics.mean(f::HipColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 1)[1]            # length(x)×S
Statistics.var(f::HipColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 2)[2]
Statistics.cov(f::HipColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 4)[3]
StatsBase.mean_and_var(f::HipColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 3)[1:2]
function StatsBase.mean_and_cov(f::HipColumnsPosteriorGP, x::AbstractVector)
    m, _, c = predict(f, x, 5)
    return m, c
end
# one mean per column: a FiniteGP over a column posterior (held-out logpdf, samples, sequential conditioning) is not offered
(f::HipColumnsPosteriorGP)(x...) = throw(ArgumentError("a FiniteGP over a column posterior is not offered: use posterior(fx, Y[:, s])"))

function logpdf_and_grad_columns(fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real}; wrt_x::Bool=false)
    a, Yv = columns_args(fx, Y)
    T = a.T
    n, S = size(Yv)
    lp = Vector{T}(undef, S)
    dnoise = dnoise_buffer(a.cn, T, n)
    dY = Matrix{T}(undef, n, S)
    dx = wrt_x ? similar(a.xbuf) : T[]
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    if haskey(a, :ks)
        dθ = zeros(Float64, length(sum_theta(a.P, a.terms)))
        GC.@preserve a Yv lp dθ dnoise dY dx begin
            check(ccall((:gp_logpdf_grad_cols_sum, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CKSum}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid},
                    Ptr{Cvoid}),
                fx.f.ctx.handle, a.ks, a.cx, a.cn, mptr, Yv, n, S, lp, dθ, dnoise, dY, wrt_x ? pointer(dx) : C_NULL))
        end
        return lp, (theta=dθ, kernel=sum_chain(a.P, a.terms, dθ), noise=a.cn.kind == 0 ? dnoise[1] : dnoise, y=dY, mean=-dY, x=wrt_x ? dx : nothing)
    end
    dvar = Ref{Float64}(0.0)
    dscale = zeros(Float64, max(length(a.scales), 1))
    GC.@preserve a Yv lp dscale dnoise dY dx begin
        check(ccall((:gp_logpdf_grad_cols, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ptr{Cvoid},
                Ptr{Cvoid}, Ptr{Cvoid}),
            fx.f.ctx.handle, a.ck, a.cx, a.cn, mptr, Yv, n, S, lp, dvar, dscale, dnoise, dY, wrt_x ? pointer(dx) : C_NULL))
    end
    return lp, (variance=dvar[], scale=dscale[1:length(a.scales)], noise=a.cn.kind == 0 ? dnoise[1] : dnoise, y=dY, mean=-dY, x=wrt_x ? dx : nothing)
end

# ---- VFE / DTC (src/sparse_approximations.jl:58-75, 183-217, 248-254, 282-286) ---------------------
struct HipApproxPosteriorGP{Tapprox,Tprior<:HipGP,Tx,TΣ} <: AbstractGP
    approx::Tapprox
    prior::Tprior
    handle::Base.RefValue{Ptr{Cvoid}}
    T::DataType
    objective::Float64                 # ELBO / DTC evidence from the same streamed pass
    x::Tx                              # cache.x  (src/sparse_approximations.jl:73, :115): every observation input seen so far
    Σy::TΣ                             # cache.Σy (:73, :100): Diagonal over every observation seen so far
end
post_handle(f::HipApproxPosteriorGP) = (getfield(f, :handle)[], getfield(f, :T), :gp_vfe_logpdf, :gp_vfe_rand)
function approx_posterior(approx, prior, h::Base.RefValue{Ptr{Cvoid}}, ::Type{T}, obj, x, Σy) where {T}
    finalizer(hh -> ccall((:gp_vfe_free, libgpmi355), Int32, (Ptr{Cvoid},), hh[]), h)
    return HipApproxPosteriorGP(approx, prior, h, T, Float64(obj), x, Σy)
end
# `post.data` — the cache of the reference (src/sparse_approximations.jl:73), read field by field by its tests
# (test/sparse_approximations.jl:48-55, 76-83): m_ε, Λ_ε (a LinearAlgebra.Cholesky, so Λ_ε.U works), U, α, b_y from the device
# (gp_vfe_get, gp_vfe_get_factors, gp_vfe_get_by), x and Σy from the host side.  B_εf (M×N) is never materialised and is not a field.
# The view is LAZY: `post.data` costs nothing, `post.data.α` moves M numbers, `post.data.U` one M×M factor — a NamedTuple built on every
# access would download both factors and the N-vector b_y each time (256 MB per `post.data.α` at M = 4 096, N = 262 144).
struct HipVfeCache{Tf}
    f::Tf
end
Base.propertynames(::HipVfeCache) = (:m_ε, :Λ_ε, :U, :α, :b_y, :x, :Σy)
function Base.getproperty(c::HipVfeCache, s::Symbol)
    f = getfield(c, :f)
    h, T = getfield(f, :handle), getfield(f, :T)
    s === :x && return getfield(f, :x)
    s === :Σy && return getfield(f, :Σy)
    m = Int(ccall((:gp_vfe_m, libgpmi355), Int64, (Ptr{Cvoid},), h[]))
    if s === :α || s === :m_ε
        v = Vector{T}(undef, m)
        GC.@preserve f v begin
            p = convert(Ptr{Cvoid}, pointer(v))
            check(ccall((:gp_vfe_get, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], s === :α ? p : C_NULL, s === :m_ε ? p : C_NULL))
        end
        return v
    elseif s === :U || s === :Λ_ε
        A = Matrix{T}(undef, m, m)
        GC.@preserve f A begin
            p = convert(Ptr{Cvoid}, pointer(A))
            check(ccall((:gp_vfe_get_factors, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], s === :U ? p : C_NULL, s === :Λ_ε ? p : C_NULL))
        end
        return s === :U ? UpperTriangular(A) : Cholesky(A, 'U', 0)
    elseif s === :b_y
        n = Int(ccall((:gp_vfe_n, libgpmi355), Int64, (Ptr{Cvoid},), h[]))
        b_y = Vector{T}(undef, n)
        GC.@preserve f b_y check(ccall((:gp_vfe_get_by, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h[], b_y))
        return b_y
    end
    throw(ArgumentError("the VFE cache has no field $s (fields: $(propertynames(c)); B_εf is never materialised)"))
end
Base.getproperty(f::HipApproxPosteriorGP, s::Symbol) = s === :data ? HipVfeCache(f) : getfield(f, s)
Base.propertynames(::HipApproxPosteriorGP) = (:approx, :prior, :data, :objective)

# FiniteGP API of the two posterior types on the device
for PT in (:HipPosteriorGP, :HipApproxPosteriorGP)
    @eval begin
        Distributions.logpdf(fx::FiniteGP{<:$PT}, Y::AbstractVecOrMat{<:Real}) = joint_logpdf(fx.f, fx, Y)
        Random.rand(rng::Random.AbstractRNG, fx::FiniteGP{<:$PT}, N::Int) =
            joint_rand!(rng, fx.f, fx, Matrix{post_handle(fx.f)[2]}(undef, length(fx), N))
        Random.rand(rng::Random.AbstractRNG, fx::FiniteGP{<:$PT}) = joint_rand!(rng, fx.f, fx, Vector{post_handle(fx.f)[2]}(undef, length(fx)))
        Random.rand!(rng::Random.AbstractRNG, fx::FiniteGP{<:$PT}, y::AbstractVecOrMat{<:Real}) = joint_rand!(rng, fx.f, fx, y)   # :271-277
    end
end
function Random.rand!(rng::Random.AbstractRNG, fx::FiniteGP{<:HipGP}, y::AbstractVecOrMat{<:Real})            # :271-277
    y .= y isa AbstractVector ? rand(rng, fx) : rand(rng, fx, size(y, 2))
    return y
end

function vfe_call(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}, want_post::Bool)
    @assert approx.fz.f === fx.f                                                       # :59, :249, :283
    length(fx) == length(y) || throw(DimensionMismatch("length(fx) != length(y)"))    # :290-294
    a = marshal(fx, eltype(y))
    (a === nothing || haskey(a, :ks)) && return nothing   # VFE / DTC are single-kind: composite kernels take the stock path
    is_dense(a.cn) && return nothing                      # dense Σy: the sparse fits need cholesky(Σy) (src/sparse_approximations.jl:61) — stock path
    T = a.T
    pz = points(approx.fz.x, T)
    pz === nothing && return nothing
    jit = approx.fz.Σy
    jit isa Diagonal{<:Any,<:Fill} || return nothing
    jitter = Float64(FillArrays.getindex_value(jit.diag))
    zbuf, cz = pz
    yv = Vector{T}(y)
    obj = Ref{T}(zero(T))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a zbuf yv h begin
        check(ccall((:gp_vfe_fit, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CPoints}, Ref{CNoise}, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Int32,
                Ptr{Ptr{Cvoid}}, Ref{T}),
            fx.f.ctx.handle, a.ck, a.cx, cz, a.cn, jitter, mptr, yv, approx isa VFE ? 0 : 1,
            want_post ? h : Ptr{Ptr{Cvoid}}(C_NULL), obj))
    end
    return (h, Float64(obj[]), T)
end

function AbstractGPs.posterior(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real})
    r = vfe_call(approx, fx, y, true)
    r === nothing && return posterior(typeof(approx)(FiniteGP(fx.f.gp, approx.fz.x, approx.fz.Σy)), stock(fx), y)
    return approx_posterior(approx, fx.f, r[1], r[3], r[2], fx.x, Diagonal(collect(diag(fx.Σy))))
end
function AbstractGPs.approx_log_evidence(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real})
    r = vfe_call(approx, fx, y, false)
    r === nothing &&
        return approx_log_evidence(typeof(approx)(FiniteGP(fx.f.gp, approx.fz.x, approx.fz.Σy)), stock(fx), y)
    return r[2]
end
AbstractGPs.elbo(vfe::VFE, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}) = approx_log_evidence(vfe, fx, y)  # :254

# ---- value + gradient of the sparse objective: one fit + one backward pass over the retained observations (gp_vfe_grad) ------------------
# The reference's users maximise `elbo(VFE(f(z, jitter)), f(x, Σy), y)` over kernel parameters and pseudo-points by AD / finite differences
# (examples/0-intro-1d/script.jl:385-394); the ccall is opaque to AD, so the accelerated objective carries its own pullback.
# ∂/∂z needs an fp64 fit (an fp32 fit's streamed B Bᵀ does not carry it: the library returns −7), so fp32 inputs get no z-tangent.
function elbo_and_grad(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}; wrt_x::Bool=false)
    r = vfe_call(approx, fx, y, true)
    r === nothing && throw(ArgumentError("kernel / noise / pseudo-input form is not accelerated"))
    h, obj, T = r
    a = marshal(fx, eltype(y))
    zbuf, cz = points(approx.fz.x, T)
    n = length(y)
    dvar = Ref{Float64}(0.0); dns = Ref{Float64}(0.0)
    dscale = zeros(Float64, max(length(a.scales), 1))
    dnoise = Vector{T}(undef, n); dy = Vector{T}(undef, n)
    dz = T === Float64 ? similar(zbuf, Float64) : Float64[]             # the container layout of the pseudo-inputs
    dx = wrt_x ? similar(a.xbuf) : T[]
    try
        GC.@preserve dscale dnoise dy dz dx check(ccall((:gp_vfe_grad, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ref{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Cvoid}, Int32),
            h[], dvar, dscale, dns, dnoise, dy, T === Float64 ? pointer(dz) : Ptr{Float64}(C_NULL), cz.layout,
            wrt_x ? pointer(dx) : C_NULL, a.cx.layout))
    finally
        ccall((:gp_vfe_free, libgpmi355), Int32, (Ptr{Cvoid},), h[])
    end
    return obj, (variance=dvar[], scale=dscale[1:length(a.scales)], noise=a.cn.kind == 0 ? dns[] : dnoise, y=dy, mean=-dy,
        z=T === Float64 ? dz : nothing, x=wrt_x ? dx : nothing)
end

function ChainRulesCore.rrule(config::RuleConfig{>:HasReverseMode}, ::typeof(AbstractGPs.approx_log_evidence), approx::Union{VFE,DTC},
    fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real})
    desc = descriptor(fx.f.gp.kernel)
    if desc === nothing || marshal(fx, eltype(y)) === nothing || !(approx.fz.Σy isa Diagonal{<:Any,<:Fill})   # stock path keeps its own AD
        v0, back = rrule_via_ad(config, (g_, z_, J_, x_, Σ_, y_) -> approx_log_evidence(typeof(approx)(FiniteGP(g_, z_, J_)), FiniteGP(g_, x_, Σ_), y_),
            fx.f.gp, approx.fz.x, approx.fz.Σy, fx.x, fx.Σy, y)
        return v0, function (Δ)
            _, dg, dzz, dJ, dx, dΣ, dy = back(Δ)
            dfz = Tangent{typeof(approx.fz)}(; f=Tangent{typeof(fx.f)}(; gp=dg, ctx=NoTangent()), x=dzz, Σy=dJ)
            return NoTangent(), Tangent{typeof(approx)}(; fz=dfz), Tangent{typeof(fx)}(; f=Tangent{typeof(fx.f)}(; gp=dg, ctx=NoTangent()), x=dx, Σy=dΣ), dy
        end
    end
    v, g = elbo_and_grad(approx, fx, y; wrt_x=true)
    function sparse_objective_pullback(Δ)
        Δr = unthunk(Δ)
        gp = fx.f.gp
        dk = kernel_tangent(gp.kernel, Δr * g.variance, desc[2], Δr .* g.scale)
        dgp = Tangent{typeof(gp)}(; mean=mean_tangent(gp.mean, Δr .* g.mean), kernel=dk)
        df = Tangent{typeof(fx.f)}(; gp=dgp, ctx=NoTangent())
        dfx = Tangent{typeof(fx)}(; f=df, x=input_tangent(fx.x, g.x, Δr), Σy=noise_tangent(fx.Σy, Δr .* g.noise))
        # the prior is shared (approx.fz.f === fx.f): its tangent travels with fx; the pseudo-inputs get theirs, the jitter is a constant of the fit
        dzt = g.z === nothing ? ChainRulesCore.@not_implemented("HipGPs: ∂/∂z needs Float64 inputs") : input_tangent(approx.fz.x, g.z, Δr)
        dfz = Tangent{typeof(approx.fz)}(; f=ZeroTangent(), x=dzt, Σy=ZeroTangent())
        return NoTangent(), Tangent{typeof(approx)}(; fz=dfz), dfx, Δr .* g.y
    end
    return v, sparse_objective_pullback
end
ChainRulesCore.rrule(config::RuleConfig{>:HasReverseMode}, ::typeof(AbstractGPs.elbo), vfe::VFE, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real}) =
    ChainRulesCore.rrule(config, AbstractGPs.approx_log_evidence, vfe, fx, y)

function vfe_predict(f::HipApproxPosteriorGP, x::AbstractVector, what::Integer)
    T = getfield(f, :T)
    px = points(x, T)
    px === nothing && throw(ArgumentError("unsupported input container for the accelerated posterior (use a Vector, ColVecs or RowVecs)"))
    xbuf, cx = px
    ns = length(x)
    pm = prior_mean(f.prior.gp, x, T)
    m = (what & 1) != 0 ? Vector{T}(undef, ns) : T[]
    v = (what & 2) != 0 ? Vector{T}(undef, ns) : T[]
    c = (what & 4) != 0 ? Matrix{T}(undef, ns, ns) : Matrix{T}(undef, 0, 0)
    GC.@preserve f xbuf pm m v c begin
        check(ccall((:gp_vfe_predict, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            getfield(f, :handle)[], cx, pm === nothing ? C_NULL : pointer(pm), what, m, v, c))
    end
    return m, v, c
end
Statistics.mean(f::HipApproxPosteriorGP, x::AbstractVector) = vfe_predict(f, x, 1)[1]          # :183-185
Statistics.cov(f::HipApproxPosteriorGP, x::AbstractVector) = vfe_predict(f, x, 4)[3]           # :187-190
Statistics.var(f::HipApproxPosteriorGP, x::AbstractVector) = vfe_predict(f, x, 2)[2]           # :192-195
function Statistics.cov(f::HipApproxPosteriorGP, x::AbstractVector, z::AbstractVector)         # :197-203
    c = vfe_predict(f, vcat(x, z), 4)[3]
    return c[1:length(x), (length(x) + 1):end]
end
function StatsBase.mean_and_cov(f::HipApproxPosteriorGP, x::AbstractVector)                    # :205-210
    m, _, c = vfe_predict(f, x, 5)
    return m, c
end
StatsBase.mean_and_var(f::HipApproxPosteriorGP, x::AbstractVector) = vfe_predict(f, x, 3)[1:2] # :212-217
AbstractGPs.inducing_points(f::HipApproxPosteriorGP) = f.approx.fz.x                            # :219

# ---- gradients of the predictive mean / variance w.r.t. the test inputs ---------------------------------
# What an AD backend computes when it differentiates mean(f_post, x) / var(f_post, x) / mean_and_var(f_post, x) of the stock posteriors
# (src/exact_gpr_posterior.jl:60-90, src/sparse_approximations.jl:183-217): acquisition functions over x*, the test-time half of a deep kernel.
# gp_posterior_predict_grad / gp_vfe_predict_grad return values and gradients from ONE call; dm / dv lie in the container layout of x
# (Vector / D×N of ColVecs / N×D of RowVecs).  The device takes the prior mean as constant in x — exact for ZeroMean / ConstMean; the mean side of a
# CustomMean prior is refused here (never a silently incomplete gradient: such a model differentiates the stock path).
grad_entry(::HipPosteriorGP) = :exact
grad_entry(::HipApproxPosteriorGP) = :sparse
grad_eltype(f::HipPosteriorGP) = getfield(f.data.C, :T)
grad_eltype(f::HipApproxPosteriorGP) = getfield(f, :T)
grad_handle(f::HipPosteriorGP) = getfield(f.data.C, :handle)
grad_handle(f::HipApproxPosteriorGP) = getfield(f, :handle)[]
function predict_grad(f::Union{HipPosteriorGP,HipApproxPosteriorGP}, x::AbstractVector, what::Integer)
    T = grad_eltype(f)
    px = points(x, T)
    px === nothing && throw(ArgumentError("unsupported input container for the accelerated posterior (use a Vector, ColVecs or RowVecs)"))
    (what & 1) != 0 && f.prior.gp.mean isa CustomMean &&
        throw(ArgumentError("HipGPs: the gradient of the predictive mean under a CustomMean needs the mean function's own derivative; differentiate the stock path"))
    xbuf, cx = px
    ns = length(x)
    pm = prior_mean(f.prior.gp, x, T)
    m = (what & 1) != 0 ? Vector{T}(undef, ns) : T[]
    v = (what & 2) != 0 ? Vector{T}(undef, ns) : T[]
    dm = (what & 1) != 0 ? similar(xbuf) : T[]
    dv = (what & 2) != 0 ? similar(xbuf) : T[]
    h = grad_handle(f)
    GC.@preserve f xbuf pm m v dm dv begin
        if grad_entry(f) === :exact
            check(ccall((:gp_posterior_predict_grad, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                h, cx, pm === nothing ? C_NULL : pointer(pm), what, m, v, dm, dv))
        else
            check(ccall((:gp_vfe_predict_grad, libgpmi355), Int32,
                (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                h, cx, pm === nothing ? C_NULL : pointer(pm), what, m, v, dm, dv))
        end
    end
    return m, v, dm, dv
end
# Δ_j · g[j, :] in the layout of the container, and the tangent of the container around it
rows_times(x::AbstractVector{<:Real}, g, Δ) = Δ .* g
rows_times(x::ColVecs, g, Δ) = g .* reshape(Δ, 1, :)
rows_times(x::RowVecs, g, Δ) = g .* reshape(Δ, :, 1)
# a zero cotangent of one side (m, v = mean_and_var(p, x); sum(m) delivers (Δm, ZeroTangent)): one method per container, so that none is ambiguous with the three above
rows_times(x::AbstractVector{<:Real}, g, ::ChainRulesCore.AbstractZero) = zero(g)
rows_times(x::ColVecs, g, ::ChainRulesCore.AbstractZero) = zero(g)
rows_times(x::RowVecs, g, ::ChainRulesCore.AbstractZero) = zero(g)
points_tangent(x::AbstractVector{<:Real}, G) = G
points_tangent(x::Union{ColVecs,RowVecs}, G) = Tangent{typeof(x)}(; X=G)
posterior_tangent() = ChainRulesCore.@not_implemented("HipGPs: the device posterior is a constant of mean / var (gradients w.r.t. the fit go through logpdf / elbo)")

function ChainRulesCore.rrule(::typeof(Statistics.mean), f::Union{HipPosteriorGP,HipApproxPosteriorGP}, x::AbstractVector)
    m, _, dm, _ = predict_grad(f, x, 1)
    predictive_mean_pullback(Δ) = (NoTangent(), posterior_tangent(), points_tangent(x, rows_times(x, dm, unthunk(Δ))))
    return m, predictive_mean_pullback
end
function ChainRulesCore.rrule(::typeof(Statistics.var), f::Union{HipPosteriorGP,HipApproxPosteriorGP}, x::AbstractVector)
    _, v, _, dv = predict_grad(f, x, 2)
    predictive_var_pullback(Δ) = (NoTangent(), posterior_tangent(), points_tangent(x, rows_times(x, dv, unthunk(Δ))))
    return v, predictive_var_pullback
end
function ChainRulesCore.rrule(::typeof(StatsBase.mean_and_var), f::Union{HipPosteriorGP,HipApproxPosteriorGP}, x::AbstractVector)
    m, v, dm, dv = predict_grad(f, x, 3)
    function predictive_mean_and_var_pullback(Δ)
        Δm, Δv = unthunk(Δ)
        return NoTangent(), posterior_tangent(), points_tangent(x, rows_times(x, dm, unthunk(Δm)) .+ rows_times(x, dv, unthunk(Δv)))
    end
    return (m, v), predictive_mean_and_var_pullback
end

# update_posterior with new observations, same pseudo-points (src/sparse_approximations.jl:87-121)
function AbstractGPs.update_posterior(f::HipApproxPosteriorGP, fx::FiniteGP{<:HipGP}, y::AbstractVector{<:Real})
    @assert f.prior === fx.f
    T = getfield(f, :T)
    xbuf, cx, nbuf, cn, m2 = joint_args(fx, f.prior.gp, T)
    is_dense(cn) && throw(ArgumentError("update_posterior of a VFE / DTC posterior with a dense Σy is not accelerated (the reference factors Σy there)"))
    yv = Vector{T}(y)
    obj = Ref{T}(zero(T))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve f xbuf nbuf m2 yv begin
        check(ccall((:gp_vfe_update, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{T}),
            getfield(f, :handle)[], cx, cn, m2 === nothing ? C_NULL : pointer(m2), yv, h, obj))
    end
    Σy = Diagonal(vcat(diag(getfield(f, :Σy)), diag(fx.Σy)))                                   # :99-100 (block-diagonal of two Diagonals)
    return approx_posterior(f.approx, f.prior, h, T, obj[], vcat(getfield(f, :x), fx.x), Σy)   # :115
end

# update_posterior with new pseudo-points (src/sparse_approximations.jl:131-176): bordered K_zz factor + re-streamed new block
# rows on the device; the approximation object is rebuilt with z = vcat(z_old, z_new) like _update_approx (:178-179)
function AbstractGPs.update_posterior(f::HipApproxPosteriorGP, fz::FiniteGP{<:HipGP})
    @assert f.prior === fz.f                                                                   # :132
    T = getfield(f, :T)
    pz = points(fz.x, T)
    pz === nothing && throw(ArgumentError("unsupported container for the new pseudo-points"))
    zbuf, cz = pz
    obj = Ref{T}(zero(T))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve f zbuf begin
        check(ccall((:gp_vfe_append, libgpmi355), Int32, (Ptr{Cvoid}, Ref{CPoints}, Ref{Ptr{Cvoid}}, Ref{T}), getfield(f, :handle)[], cz, h, obj))
    end
    fz_new = f.approx.fz.f(vcat(f.approx.fz.x, fz.x), f.approx.fz.Σy)                         # :160-162
    return approx_posterior(typeof(f.approx)(fz_new), f.prior, h, T, obj[], getfield(f, :x), getfield(f, :Σy))
end

# ---- VFE / DTC for a matrix of observations (include/gpmi355.h "VFE / DTC for a matrix of observations") ------------------
# S = size(Y, 2) <= 128 sparse GPs that share x, z, kernel, jitter, Σy and the prior mean and differ in y: posterior_columns(approx, fx, Y) fits them from ONE
# streamed pass (gp_vfe_fit_cols), mean(f, x) is length(x)×S from ONE kernel launch over the pseudo-points (gp_vfe_predict_cols), var / cov do not depend
# on y; update_posterior continues all columns (gp_vfe_update_cols / gp_vfe_append_cols); elbo_and_grad_columns returns the objectives (length S) and the
# gradient of their SUM (gp_vfe_grad_cols).  Single-kind kernels with a scalar / diagonal Σy, as the single-column sparse calls.
struct HipApproxColumnsPosteriorGP{Tapprox,Tprior<:HipGP} <: AbstractGP
    approx::Tapprox
    prior::Tprior
    handle::Base.RefValue{Ptr{Cvoid}}
    T::DataType
    ncols::Int
    objective::Vector{Float64}         # ELBO / DTC evidence of every column from the same streamed pass
end
function approx_columns_posterior(approx, prior, h::Base.RefValue{Ptr{Cvoid}}, ::Type{T}, S, obj) where {T}
    finalizer(hh -> ccall((:gp_vfe_free, libgpmi355), Int32, (Ptr{Cvoid},), hh[]), h)
    return HipApproxColumnsPosteriorGP(approx, prior, h, T, Int(S), Vector{Float64}(obj))
end

function vfe_cols_call(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real}, want_post::Bool)
    @assert approx.fz.f === fx.f
    a, Yv = columns_args(fx, Y)
    (haskey(a, :ks) || is_dense(a.cn)) && throw(ArgumentError("VFE / DTC columns: composite kernels and a dense Σy are not accelerated"))
    T = a.T
    pz = points(approx.fz.x, T)
    pz === nothing && throw(ArgumentError("unsupported container for the pseudo-points"))
    jit = approx.fz.Σy
    jit isa Diagonal{<:Any,<:Fill} || throw(ArgumentError("inducing-point noise must be a scalar jitter"))
    jitter = Float64(FillArrays.getindex_value(jit.diag))
    zbuf, cz = pz
    n, S = size(Yv)
    obj = Vector{T}(undef, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = a.m === nothing ? C_NULL : pointer(a.m)
    GC.@preserve a zbuf Yv obj h begin
        check(ccall((:gp_vfe_fit_cols, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CKernel}, Ref{CPoints}, Ref{CPoints}, Ref{CNoise}, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32,
                Ptr{Ptr{Cvoid}}, Ptr{Cvoid}),
            fx.f.ctx.handle, a.ck, a.cx, cz, a.cn, jitter, mptr, Yv, max(n, 1), S, approx isa VFE ? 0 : 1,
            want_post ? h : Ptr{Ptr{Cvoid}}(C_NULL), obj))
    end
    return (h, Vector{Float64}(obj), T, S)
end

function posterior_columns(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real})
    h, obj, T, S = vfe_cols_call(approx, fx, Y, true)
    return approx_columns_posterior(approx, fx.f, h, T, S, obj)
end
approx_log_evidence_columns(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real}) = vfe_cols_call(approx, fx, Y, false)[2]
elbo_columns(vfe::VFE, fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real}) = approx_log_evidence_columns(vfe, fx, Y)

function ncolumns(f::HipApproxColumnsPosteriorGP)
    out = Ref{Int32}(0)
    check(ccall((:gp_vfe_ncols, libgpmi355), Int32, (Ptr{Cvoid}, Ref{Int32}), getfield(f, :handle)[], out))
    return Int(out[])
end

# (α, m_ε) of every column, both M×S, and b_y, n×S: the y-dependent cache fields (src/sparse_approximations.jl:73) column by column
function columns_data(f::HipApproxColumnsPosteriorGP)
    T = getfield(f, :T)
    h = getfield(f, :handle)
    S = getfield(f, :ncols)
    m = Int(ccall((:gp_vfe_m, libgpmi355), Int64, (Ptr{Cvoid},), h[]))
    n = Int(ccall((:gp_vfe_n, libgpmi355), Int64, (Ptr{Cvoid},), h[]))
    α = Matrix{T}(undef, m, S); m_ε = Matrix{T}(undef, m, S); b_y = Matrix{T}(undef, n, S)
    GC.@preserve f α m_ε b_y begin
        check(ccall((:gp_vfe_get_cols, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], α, m_ε))
        check(ccall((:gp_vfe_get_by_cols, libgpmi355), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h[], b_y))
    end
    return (α=α, m_ε=m_ε, b_y=b_y)
end

function predict(f::HipApproxColumnsPosteriorGP, x::AbstractVector, what::Integer)
    T = getfield(f, :T)
    px = points(x, T)
    px === nothing && throw(ArgumentError("unsupported input container for the accelerated posterior (use a Vector, ColVecs or RowVecs)"))
    xbuf, cx = px
    ns = length(x)
    pm = prior_mean(f.prior.gp, x, T)
    m = (what & 1) != 0 ? Matrix{T}(undef, ns, getfield(f, :ncols)) : Matrix{T}(undef, 0, 0)
    v = (what & 2) != 0 ? Vector{T}(undef, ns) : T[]
    c = (what & 4) != 0 ? Matrix{T}(undef, ns, ns) : Matrix{T}(undef, 0, 0)
    GC.@preserve f xbuf pm m v c begin
        check(ccall((:gp_vfe_predict_cols, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            getfield(f, :handle)[], cx, pm === nothing ? C_NULL : pointer(pm), what, m, v, c))
    end
    return m, v, c
end
Statistics.mean(f::HipApproxColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 1)[1]            # length(x)×S
Statistics.var(f::HipApproxColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 2)[2]
Statistics.cov(f::HipApproxColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 4)[3]
StatsBase.mean_and_var(f::HipApproxColumnsPosteriorGP, x::AbstractVector) = predict(f, x, 3)[1:2]
function StatsBase.mean_and_cov(f::HipApproxColumnsPosteriorGP, x::AbstractVector)
    m, _, c = predict(f, x, 5)
    return m, c
end
(f::HipApproxColumnsPosteriorGP)(x...) = throw(ArgumentError("a FiniteGP over a column posterior is not offered: use posterior(approx, fx, Y[:, s])"))

function AbstractGPs.update_posterior(f::HipApproxColumnsPosteriorGP, fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real})
    @assert f.prior === fx.f
    T = getfield(f, :T)
    S = getfield(f, :ncols)
    size(Y, 1) == length(fx) || throw(DimensionMismatch("length(fx) = $(length(fx)) but Y has $(size(Y, 1)) rows"))
    size(Y, 2) == S || throw(DimensionMismatch("Y has $(size(Y, 2)) columns but the posterior holds $S"))
    xbuf, cx, nbuf, cn, m2 = joint_args(fx, f.prior.gp, T)
    is_dense(cn) && throw(ArgumentError("update_posterior of a VFE / DTC posterior with a dense Σy is not accelerated (the reference factors Σy there)"))
    Yv = Matrix{T}(Y)
    obj = Vector{T}(undef, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve f xbuf nbuf m2 Yv obj begin
        check(ccall((:gp_vfe_update_cols, libgpmi355), Int32,
            (Ptr{Cvoid}, Ref{CPoints}, Ref{CNoise}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}, Ptr{Cvoid}),
            getfield(f, :handle)[], cx, cn, m2 === nothing ? C_NULL : pointer(m2), Yv, max(size(Yv, 1), 1), h, obj))
    end
    return approx_columns_posterior(f.approx, f.prior, h, T, S, obj)
end

function AbstractGPs.update_posterior(f::HipApproxColumnsPosteriorGP, fz::FiniteGP{<:HipGP})
    @assert f.prior === fz.f
    T = getfield(f, :T)
    S = getfield(f, :ncols)
    pz = points(fz.x, T)
    pz === nothing && throw(ArgumentError("unsupported container for the new pseudo-points"))
    zbuf, cz = pz
    obj = Vector{T}(undef, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve f zbuf obj begin
        check(ccall((:gp_vfe_append_cols, libgpmi355), Int32, (Ptr{Cvoid}, Ref{CPoints}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}), getfield(f, :handle)[], cz, h, obj))
    end
    fz_new = f.approx.fz.f(vcat(f.approx.fz.x, fz.x), f.approx.fz.Σy)
    return approx_columns_posterior(typeof(f.approx)(fz_new), f.prior, h, T, S, obj)
end

# the objectives of every column and the gradient of their SUM at the posterior's own parameters; y / mean are n×S
function objective_grad(f::HipApproxColumnsPosteriorGP, fx::FiniteGP{<:HipGP}; wrt_x::Bool=false)
    T = getfield(f, :T)
    S = getfield(f, :ncols)
    h = getfield(f, :handle)
    a = marshal(fx, T)
    zbuf, cz = points(f.approx.fz.x, T)
    n = Int(ccall((:gp_vfe_n, libgpmi355), Int64, (Ptr{Cvoid},), h[]))
    (!wrt_x || length(fx) == n) || throw(ArgumentError("wrt_x: fx must hold every observation of the posterior ($n)"))
    dvar = Ref{Float64}(0.0); dns = Ref{Float64}(0.0)
    dscale = zeros(Float64, max(length(a.scales), 1))
    dnoise = Vector{T}(undef, n); dY = Matrix{T}(undef, n, S)
    dz = T === Float64 ? similar(zbuf, Float64) : Float64[]
    dx = wrt_x ? similar(a.xbuf) : T[]
    GC.@preserve f dscale dnoise dY dz dx check(ccall((:gp_vfe_grad_cols, libgpmi355), Int32,
        (Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ref{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Cvoid}, Int32),
        h[], dvar, dscale, dns, dnoise, dY, T === Float64 ? pointer(dz) : Ptr{Float64}(C_NULL), cz.layout,
        wrt_x ? pointer(dx) : C_NULL, a.cx.layout))
    return (variance=dvar[], scale=dscale[1:length(a.scales)], noise=a.cn.kind == 0 ? dns[] : dnoise, y=dY, mean=-dY,
        z=T === Float64 ? dz : nothing, x=wrt_x ? dx : nothing)
end
function elbo_and_grad_columns(approx::Union{VFE,DTC}, fx::FiniteGP{<:HipGP}, Y::AbstractMatrix{<:Real}; wrt_x::Bool=false)
    post = posterior_columns(approx, fx, Y)
    return post.objective, objective_grad(post, fx; wrt_x=wrt_x)
end

end # module
