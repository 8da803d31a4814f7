# AutoBZCoreHIP.jl -- reference-side binding of libabzhip.so (include/abzhip.h).
#
# UNTESTED SOURCE: there is no Julia toolchain in the build pipeline (SURVEY.md section 8c), so this
# file shows the shim a maintainer of AutoBZCore.jl v0.3.8 would add; the same C ABI is exercised
# by the Python ctypes mirror in autobzcore.jl_amd/ and by tests/.
#
# What it plugs into (file:line in lxvm/AutoBZCore.jl v0.3.8):
#   * the dispatch pair init_cacheval / do_solve          src/interfaces.jl:59-62,116-118
#   * FourierIntegrand / FourierValue                     src/fourier.jl:22-58,111-118
#   * PTR / AutoPTR / IAI on a SymmetricBZ                src/brillouin.jl:337-444, src/fourier.jl:338-389,488-510
#   * BatchIntegrand f!(y, x, p)                          src/batch.jl:1-38
#   * batchsolve                                          src/interfaces.jl:199-243
#   * DOSProblem + GGR                                    src/dos_ggr.jl:1-104
#   * DOSProblem + LTM (planned there)                    src/dos_algorithms.jl:1-7
module AutoBZCoreHIP

using AutoBZCore
using AutoBZCore: FourierIntegrand, FourierValue, ParameterIntegrand, MixedParameters, SymmetricBZ,
    IntegralSolution, IntegralSolver, nsyms, PTR, AutoPTR, IAI, CubicLimits, TetrahedralLimits
using FourierSeriesEvaluators: FourierSeries, period
using LinearAlgebra, StaticArrays

const libabz = "libabzhip"   # autobzcore.jl_amd/libabzhip.so on the loader path

# ---------------------------------------------------------------- constants of abzhip.h
const WANT_H, WANT_EIG, WANT_VEL = Cint(1), Cint(2), Cint(4)
# rules of a Hermitian series (n <= 4) keep H(k) as its upper triangle: n^2 value planes instead of 2 n^2; ignored otherwise.
# Device integrands read those planes, abz_rule_export still returns full matrices (abzhip.h).
const WANT_H_COMPACT = Cint(8)
const WANT_H_ROW_MAJOR = Cint(16)  # abz_eval_nodes: row-major matrices (not for Julia arrays; listed for completeness)
const WANT_HC = WANT_H | WANT_H_COMPACT
const F_ONE, F_LINEAR, F_LINEAR_X, F_DOS, F_TRGLOC, F_GLOC, F_DOS_EIG = Cint.(0:6)
const LIMS_CUBIC, LIMS_TETRAHEDRAL, LIMS_POLYHEDRAL, LIMS_POLYGON = Cint(0), Cint(1), Cint(2), Cint(3)
const LTM_DOS, LTM_STATES, LTM_STATES_CORRECTED = Cint(0), Cint(1), Cint(2)  # `what` of abz_rule_ltm / abz_rule_ltm_weighted
const LTM_A_ELEMENTS, LTM_A_ENERGY, LTM_A_ONE = Cint(0), Cint(1), Cint(2)    # `source`; LTM_A_ONE: abz_rule_ltm_pairs_occupied and abz_rule_ltm_optimized

# (kind, lim_a, lim_b) of the reference's limits types for abz_iai_solve(_many); the SymmetryReduceBZ
# extension's Polyhedron3 travels as packed faces [nv, x y z ...] with lim_b = [length(lim_a)]
function pack_limits(l)
    l isa CubicLimits && return (LIMS_CUBIC, Float64[l.a...], Float64[l.b...])
    hasproperty(l, :face_coord) || return (LIMS_TETRAHEDRAL, Float64[l.a...], Float64[])
    a = Float64[]
    for f in l.face_coord            # nv x 3 matrices, vertices in order around the face
        push!(a, size(f, 1)); append!(a, vec(permutedims(f)))
    end
    return (LIMS_POLYHEDRAL, a, Float64[length(a)])
end

function check(rc::Cint)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:abz_last_error, libabz), Cstring, ()))
    rc == -1 && throw(ArgumentError(msg))        # ABZ_ERR_ARG <-> the reference's ArgumentError sites
    rc == -5 && throw(OutOfMemoryError())          # ABZ_ERR_NOMEM (device allocation, or std::bad_alloc caught at the boundary)
    error("libabzhip error $rc: $msg")             # -2 HIP, -3 no GPU, -4 unsupported, -6 a C++ exception caught at the boundary
end

# ---------------------------------------------------------------- handles
# Lifetimes: the library reference-counts context <- series <- rule, so these finalizers may run in any order
# (abz_*_destroy only marks a handle closed while dependants still use the object).
mutable struct HIPContext
    h::Ptr{Cvoid}
    HIPContext(h::Ptr{Cvoid}, ::Val{:adopt}) = new(h)
    function HIPContext(device::Integer=0)
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:abz_ctx_create, libabz), Cint, (Cint, Ptr{Ptr{Cvoid}}), device, ref))
        ctx = new(ref[])
        finalizer(c -> ccall((:abz_ctx_destroy, libabz), Cint, (Ptr{Cvoid},), c.h), ctx)
    end
end
const CTX = Ref{HIPContext}()           # one context per Julia thread in a threaded build
context() = isassigned(CTX) ? CTX[] : (CTX[] = HIPContext())

"Device-resident coefficients: replaces workspace_allocate_vec (src/fourier.jl:61-86)."
mutable struct HIPSeries{N}
    h::Ptr{Cvoid}
    n::Int
    rules::Dict{Tuple{Int,UInt,Cint},Any}
    exchange::Any                             # the @cfunction of shard_iai! (kept alive with the series)
end
function HIPSeries(s::FourierSeries{S,N}) where {S,N}
    c = s.c                                   # Array{SMatrix{n,n,ComplexF64}} or Array{<:Number}
    n = eltype(c) <: Number ? 1 : size(eltype(c), 1)
    coef = reinterpret(Float64, vec(c))       # Julia memory order == the ABI's order
    dims = Cint[size(c)...]
    first = Cint[(1 .+ s.o)...]               # frequency of c[1]: offset + 1 (OffsetArray axes fold into s.o)
    per = Float64[period(s)...]
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve coef dims first per begin
        check(ccall((:abz_series_create, libabz), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Cint, Ptr{Ptr{Cvoid}}),
            context().h, coef, N, dims, first, per, n, ref))
    end
    hs = HIPSeries{N}(ref[], n, Dict(), nothing)
    finalizer(x -> ccall((:abz_series_destroy, libabz), Cint, (Ptr{Cvoid},), x.h), hs)
end

"Cached PTR rule: replaces FourierPTR / FourierMonkhorstPack (src/fourier.jl:127-174,210-277)."
mutable struct HIPRule
    h::Ptr{Cvoid}
    nk::Int
    npt::Int
    nsyms::Int
end
function symptr_rule(npt, ::Val{d}, syms) where {d}   # replaces AutoSymPTR.symptr_rule (src/fourier.jl:271)
    S = Cint[round(Int, M[a, b]) for M in syms for a in 1:d for b in 1:d]   # row-major per matrix
    n = Ref{Int64}(0)
    check(ccall((:abz_symptr_rule, libabz), Cint, (Cint, Cint, Ptr{Cint}, Cint, Ptr{Int64}, Ptr{Cint}, Ptr{Int64}),
        npt, d, S, length(syms), n, C_NULL, C_NULL))
    idx = Matrix{Cint}(undef, d, n[]); w = Vector{Int64}(undef, n[])
    check(ccall((:abz_symptr_rule, libabz), Cint, (Cint, Cint, Ptr{Cint}, Cint, Ptr{Int64}, Ptr{Cint}, Ptr{Int64}),
        npt, d, S, length(syms), n, idx, w))
    return idx, w
end
function rule!(hs::HIPSeries{d}, npt::Integer, syms, want::Cint) where {d}
    key = (Int(npt), hash(syms), want)
    get!(hs.rules, key) do
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        if syms === nothing
            check(ccall((:abz_ptr_rule_build, libabz), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cint}, Ptr{Int64}, Cint, Ptr{Ptr{Cvoid}}),
                hs.h, npt, 0, C_NULL, C_NULL, want, ref))
            nk, ns = npt^d, 1
        elseif length(syms) <= 48
            # orbit tables, contraction plan and values on the device: the node list never visits the host
            S = Cint[round(Int, M[a, b]) for M in syms for a in 1:d for b in 1:d]   # row-major per matrix
            check(ccall((:abz_ptr_rule_build_sym, libabz), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cint}, Cint, Cint, Ptr{Ptr{Cvoid}}), hs.h, npt, S, length(syms), want, ref))
            n = Ref{Int64}(0)
            check(ccall((:abz_rule_info, libabz), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
                ref[], n, C_NULL, C_NULL, C_NULL, C_NULL))
            nk, ns = Int(n[]), length(syms)
        else
            idx, w = symptr_rule(npt, Val(d), syms)
            check(ccall((:abz_ptr_rule_build, libabz), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cint}, Ptr{Int64}, Cint, Ptr{Ptr{Cvoid}}),
                hs.h, npt, length(w), idx, w, want, ref))
            nk, ns = length(w), length(syms)
        end
        r = HIPRule(ref[], nk, npt, ns)
        finalizer(x -> ccall((:abz_rule_destroy, libabz), Cint, (Ptr{Cvoid},), x.h), r)
    end
end

# ---------------------------------------------------------------- device integrands
"Integrands evaluated on the GPU; everything else goes through `FourierValue` batches."
abstract type HIPIntegrand end
struct DOSIntegrand <: HIPIntegrand end       # (h_k, eta, omega) -> -imag(tr(inv((omega+im*eta)I - h_k.s)))/pi
struct TrGlocIntegrand <: HIPIntegrand end    # (h_k; eta, omega) -> tr(inv(complex(omega,eta)I - h_k.s))
struct GlocIntegrand <: HIPIntegrand end      # (h_k; eta, omega) -> inv(complex(omega,eta)I - h_k.s)
struct LinearIntegrand <: HIPIntegrand end    # (x, a; b) -> a*x.s + b
struct UnitIntegrand <: HIPIntegrand end
fid(::DOSIntegrand) = F_DOS; fid(::TrGlocIntegrand) = F_TRGLOC; fid(::GlocIntegrand) = F_GLOC
fid(::LinearIntegrand) = F_LINEAR; fid(::UnitIntegrand) = F_ONE
# host fall-backs keep the objects usable with every other AutoBZCore algorithm
(::DOSIntegrand)(h::FourierValue, eta, omega) = -imag(tr(inv((omega + im * eta) * I - h.s))) / pi
(::LinearIntegrand)(x::FourierValue, a; b) = a * x.s + b
bind(::Union{DOSIntegrand,TrGlocIntegrand,GlocIntegrand}, p::MixedParameters) =
    (Float64[get(getfield(p, :kwargs), :eta, p[1])], Float64(get(getfield(p, :kwargs), :omega, p[end])))
bind(::LinearIntegrand, p::MixedParameters) = (Float64[p[1], getfield(p, :kwargs).b], 0.0)
bind(::UnitIntegrand, p) = (Float64[], 0.0)

"Components of a device integrand's value (the library's integrand_ncomp): the buffers below are sized with it."
ncomp(::GlocIntegrand, n::Int, d::Int) = n * n
ncomp(::HIPIntegrand, n::Int, d::Int) = 1
"complex [ncomp] from the device -> the value the reference integrand returns (real only where the integrand is real)."
shape_value(::Union{DOSIntegrand,UnitIntegrand}, v::AbstractVector{ComplexF64}, n::Int) = real(v[1])
shape_value(::GlocIntegrand, v::AbstractVector{ComplexF64}, n::Int) = n == 1 ? v[1] : SMatrix{n,n,ComplexF64,n * n}(v)  # column-major block
shape_value(::HIPIntegrand, v::AbstractVector{ComplexF64}, n::Int) = v[1]          # TrGloc, Linear: complex scalars

const HIPFourierIntegrand = FourierIntegrand{<:HIPIntegrand}

"rule(f, B) = quadsum(...) (src/fourier.jl:204-207,289-292) for all sweep values in one pass."
function reduce_rule(r::HIPRule, f::HIPIntegrand, params::Vector{Float64}, sweep::Vector{Float64}, ncomp::Int)
    out = Vector{ComplexF64}(undef, ncomp * length(sweep))
    GC.@preserve params sweep out begin
        check(ccall((:abz_rule_reduce, libabz), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint, Ptr{ComplexF64}),
            r.h, fid(f), params, length(params), sweep, length(sweep), r.nsyms, out))
    end
    return reshape(out, ncomp, :)
end

# ---------------------------------------------------------------- the dispatch pair
# cacheval = the device series; rules are cached inside it by (npt, syms, want), so unlike
# src/interfaces.jl:174-179 nothing is rebuilt per solver call.
AutoBZCore.init_cacheval(f::HIPFourierIntegrand, bz::SymmetricBZ, p, ::Union{PTR,AutoPTR,IAI}) = HIPSeries(f.w.series)

function AutoBZCore.do_solve(f::HIPFourierIntegrand, bz::SymmetricBZ, p, alg::PTR, hs::HIPSeries{d};
    abstol=nothing, reltol=nothing, maxiters=typemax(Int)) where {d}
    j = abs(det(bz.B))                                   # src/brillouin.jl:340
    r = rule!(hs, alg.npt, bz.syms, WANT_HC)
    params, omega = bind(f.f.f, merge(f.f.p, p))
    u = reduce_rule(r, f.f.f, params, [omega], ncomp(f.f.f, hs.n, d))
    return IntegralSolution(j * nsyms(bz) * shape_value(f.f.f, view(u, :, 1), hs.n), nothing, true, r.nk)   # TrivialRep: src/brillouin.jl:107
end

"""
The p-adaptive loop of `AutoPTR` runs inside the library (`abz_autoptr_solve_many`: grid sequence, rules kept by the series,
store-free sums for grids used once, error test, `numevals`) -- the ONE implementation the Python mirror and its tests
drive as well (round 3 had a second, untested copy of the loop here).  `omegas`: one solve per swept value, in lock-step.
"""
function autoptr_solve(hs::HIPSeries{d}, f::HIPIntegrand, params::Vector{Float64}, omegas::Vector{Float64}, bz::SymmetricBZ,
    alg::AutoPTR; abstol=nothing, reltol=nothing, maxiters=typemax(Int)) where {d}
    j = abs(det(bz.B))
    n0 = clamp(round(Int, alg.n₀ / alg.a), alg.nmin, alg.nmax)       # MonkhorstPackRule's integers, src/fourier.jl:301-321
    dn = clamp(round(Int, alg.Δn / alg.a), alg.nmin, alg.nmax)
    syms = bz.syms === nothing ? Cint[] : Cint[round(Int, M[a, b]) for M in bz.syms for a in 1:d for b in 1:d]
    ns = bz.syms === nothing ? 0 : length(bz.syms)
    nsolve = length(omegas); nc = ncomp(f, hs.n, d)
    out = Vector{ComplexF64}(undef, nc * nsolve); err = Vector{Float64}(undef, nsolve)   # the library writes nc values per solve
    nev = Vector{Int64}(undef, nsolve); npt = Vector{Cint}(undef, nsolve)
    GC.@preserve syms params omegas out err nev npt begin
        check(ccall((:abz_autoptr_solve_many, libabz), Cint,
            (Ptr{Cvoid}, Ptr{Cint}, Cint, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint, Cint, Float64, Float64, Int64, Cint,
             Float64, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cint}),
            hs.h, ns == 0 ? C_NULL : pointer(syms), ns, fid(f), params, length(params), omegas, nsolve, n0, dn,
            abstol === nothing ? -1.0 : abstol / j,                  # src/brillouin.jl:433
            reltol === nothing ? -1.0 : reltol, min(maxiters, typemax(Int64) >> 1), alg.keepmost,
            Float64(nsyms(bz)),                                      # TrivialRep inside every rule: src/brillouin.jl:127-130
            out, err, nev, npt))
    end
    vals = reshape(out, nc, nsolve)
    return [IntegralSolution(shape_value(f, view(vals, :, i), hs.n) * j, err[i] * j, true, Int(nev[i])) for i in 1:nsolve]
end

"One AutoPTR solve through the single-value entry point (abz_autoptr_solve): what `do_solve(::AutoPTR)` calls."
function autoptr_solve(hs::HIPSeries{d}, f::HIPIntegrand, params::Vector{Float64}, omega::Float64, bz::SymmetricBZ,
    alg::AutoPTR; abstol=nothing, reltol=nothing, maxiters=typemax(Int)) where {d}
    j = abs(det(bz.B))
    n0 = clamp(round(Int, alg.n₀ / alg.a), alg.nmin, alg.nmax)
    dn = clamp(round(Int, alg.Δn / alg.a), alg.nmin, alg.nmax)
    syms = bz.syms === nothing ? Cint[] : Cint[round(Int, M[a, b]) for M in bz.syms for a in 1:d for b in 1:d]
    ns = bz.syms === nothing ? 0 : length(bz.syms)
    out = Vector{ComplexF64}(undef, ncomp(f, hs.n, d)); err = Ref{Float64}(0); nev = Ref{Int64}(0); npt = Ref{Cint}(0)
    GC.@preserve syms params out begin
        check(ccall((:abz_autoptr_solve, libabz), Cint,
            (Ptr{Cvoid}, Ptr{Cint}, Cint, Cint, Ptr{Float64}, Cint, Float64, Cint, Cint, Float64, Float64, Int64, Cint,
             Float64, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cint}),
            hs.h, ns == 0 ? C_NULL : pointer(syms), ns, fid(f), params, length(params), omega, n0, dn,
            abstol === nothing ? -1.0 : abstol / j, reltol === nothing ? -1.0 : reltol,
            min(maxiters, typemax(Int64) >> 1), alg.keepmost, Float64(nsyms(bz)), out, err, nev, npt))
    end
    return IntegralSolution(shape_value(f, out, hs.n) * j, err[] * j, true, Int(nev[]))
end

function AutoBZCore.do_solve(f::HIPFourierIntegrand, bz::SymmetricBZ, p, alg::AutoPTR, hs::HIPSeries;
    abstol=nothing, reltol=nothing, maxiters=typemax(Int))
    params, omega = bind(f.f.f, merge(f.f.p, p))
    return autoptr_solve(hs, f.f.f, params, omega, bz, alg; abstol, reltol, maxiters)
end

function AutoBZCore.do_solve(f::HIPFourierIntegrand, bz::SymmetricBZ, p, alg::IAI, hs::HIPSeries{d};
    abstol=nothing, reltol=nothing, maxiters=typemax(Int)) where {d}
    j = abs(det(bz.B)); ns = nsyms(bz)
    params, omega = bind(f.f.f, merge(f.f.p, p))
    kind, a, b = pack_limits(bz.lims)
    out = Vector{ComplexF64}(undef, ncomp(f.f.f, hs.n, d)); err = Ref{Float64}(0); nev = Ref{Int64}(0); npan = Ref{Int64}(0)
    GC.@preserve params a b out begin
        check(ccall((:abz_iai_solve, libabz), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Float64, Float64, Float64, Int64, Int64,
             Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
            hs.h, kind, a, isempty(b) ? C_NULL : pointer(b), fid(f.f.f), params, length(params), omega,
            abstol === nothing ? -1.0 : abstol / (j * ns),        # src/brillouin.jl:342
            reltol === nothing ? -1.0 : Float64(reltol), min(maxiters, typemax(Int64) >> 1), 0,
            out, err, nev, C_NULL, 0, npan))
    end
    return IntegralSolution(j * ns * shape_value(f.f.f, out, hs.n), j * ns * err[], true, nev[])
end

# ---------------------------------------------------------------- BatchIntegrand body for user closures
"""
    fourier_batch(g, s::FourierSeries)

`BatchIntegrand` whose body evaluates H(k) for all nodes of a batch on the GPU and applies the user
closure `g(FourierValue(k, H_k), p)` on the host (src/batch.jl:4-6 names this as the GPU hook).
"""
function fourier_batch(g, s::FourierSeries{S,N}, ::Type{Y}=ComplexF64) where {S,N,Y}
    hs = HIPSeries(s); n = hs.n
    return AutoBZCore.BatchIntegrand(Y, SVector{N,Float64}) do y, x, p
        k = reinterpret(Float64, x); H = Vector{ComplexF64}(undef, n * n * length(x))
        GC.@preserve k H check(ccall((:abz_eval_nodes, libabz), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Cint, Ptr{ComplexF64}, Ptr{Float64}),
            hs.h, k, length(x), WANT_H, H, C_NULL))
        Hs = reinterpret(SMatrix{n,n,ComplexF64,n * n}, H)
        @inbounds for i in eachindex(x)
            y[i] = g(FourierValue(x[i], Hs[i]), p)
        end
        return nothing
    end
end

# ---------------------------------------------------------------- fused parameter sweep
"batchsolve for a HIP integrand under PTR: one pass over the cached rule for all parameters."
function AutoBZCore.batchsolve(s::IntegralSolver{<:HIPFourierIntegrand,<:SymmetricBZ,<:PTR}, omegas::AbstractVector{<:Real})
    f, bz = s.f, s.dom
    hs = HIPSeries(f.w.series)
    r = rule!(hs, s.alg.npt, bz.syms, WANT_HC)
    params, _ = bind(f.f.f, merge(f.f.p, MixedParameters(first(omegas))))
    u = reduce_rule(r, f.f.f, params, Float64.(omegas), ncomp(f.f.f, hs.n, ndims(f.w.series.c)))
    return [abs(det(bz.B)) * nsyms(bz) * shape_value(f.f.f, view(u, :, i), hs.n) for i in axes(u, 2)]
end

"batchsolve for a HIP integrand under AutoPTR: the solves refine in lock-step, every grid is visited once for all that are still active."
function AutoBZCore.batchsolve(s::IntegralSolver{<:HIPFourierIntegrand,<:SymmetricBZ,<:AutoPTR}, omegas::AbstractVector{<:Real})
    f, bz = s.f, s.dom
    hs = HIPSeries(f.w.series)
    params, _ = bind(f.f.f, merge(f.f.p, MixedParameters(first(omegas))))
    sols = autoptr_solve(hs, f.f.f, params, Float64.(omegas), bz, s.alg; abstol=get(s.kwargs, :abstol, nothing),
        reltol=get(s.kwargs, :reltol, nothing), maxiters=get(s.kwargs, :maxiters, typemax(Int)))
    return [sol.u for sol in sols]
end

"batchsolve for a HIP integrand under IAI: all solves advance in lock-step and share their launches."
function AutoBZCore.batchsolve(s::IntegralSolver{<:HIPFourierIntegrand,<:SymmetricBZ,<:IAI}, omegas::AbstractVector{<:Real})
    f, bz = s.f, s.dom
    hs = HIPSeries(f.w.series)
    j = abs(det(bz.B)); ns = nsyms(bz); m = length(omegas)
    params, _ = bind(f.f.f, merge(f.f.p, MixedParameters(first(omegas))))
    kind, a, b = pack_limits(bz.lims)
    abstol = get(s.kwargs, :abstol, nothing); reltol = get(s.kwargs, :reltol, nothing)
    nc = ncomp(f.f.f, hs.n, ndims(f.w.series.c))
    sw = Float64.(omegas); out = Vector{ComplexF64}(undef, nc * m); err = Vector{Float64}(undef, m); nev = Vector{Int64}(undef, m)
    npan = Ref{Int64}(0)
    GC.@preserve params a b sw out err nev begin
        check(ccall((:abz_iai_solve_many, libabz), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Float64, Float64,
             Int64, Int64, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
            hs.h, kind, a, isempty(b) ? C_NULL : pointer(b), fid(f.f.f), params, length(params), sw, m,
            abstol === nothing ? -1.0 : abstol / (j * ns), reltol === nothing ? -1.0 : Float64(reltol),
            typemax(Int64) >> 1, 0, out, err, nev, C_NULL, 0, npan))
    end
    vals = reshape(out, nc, m)
    return [j * ns * shape_value(f.f.f, view(vals, :, i), hs.n) for i in 1:m]
end

# ---------------------------------------------------------------- store-free rule value
"rule(f, B) on the full npt^d grid without materialising FourierPTR (abz_ptr_sum): grids used once or beyond HBM."
function ptr_sum(hs::HIPSeries{d}, npt::Integer, f::HIPIntegrand, params::Vector{Float64}, omegas::Vector{Float64};
    z0=0, z1=npt, nsyms::Integer=1) where {d}
    nc = ncomp(f, hs.n, d)
    out = Vector{ComplexF64}(undef, nc * length(omegas))                 # [ncomp, n_sweep] like reduce_rule
    GC.@preserve params omegas out check(ccall((:abz_ptr_sum, libabz), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint, Ptr{ComplexF64}),
        hs.h, npt, z0, z1, fid(f), params, length(params), omegas, length(omegas), nsyms, out))
    return nc == 1 ? out : reshape(out, nc, :)
end

# ---------------------------------------------------------------- k-sharded rules (one solve on several GPUs)
"""
    slab_rule(hs, npt, rank, world, want)

This rank's slab of the full PTR grid (outermost index in `[z0, z1)`), for a solve sharded over k: sum
the `reduce_rule` results of all ranks (e.g. `MPI.Allreduce` / RCCL) to obtain the rule value.
"""
function slab_rule(hs::HIPSeries{N}, npt::Integer, rank::Integer, world::Integer, want::Integer=WANT_H) where {N}
    z0 = (npt * rank) ÷ world; z1 = (npt * (rank + 1)) ÷ world
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:abz_ptr_rule_build_slab, libabz), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Ptr{Cvoid}}),
        hs.h, npt, z0, z1, want, h))
    return HIPRule(h[], (z1 - z0) * npt^(N - 1), npt, 1)
end

# ---------------------------------------------------------------- GGR
"get_ggr_data + sum_ggr on the GPU (src/dos_ggr.jl:14-65)."
function ggr(h::FourierSeries{S,N}, bz::SymmetricBZ, Es::Vector{Float64}; npt=50) where {S,N}
    hs = HIPSeries(h)
    r = rule!(hs, npt, bz.syms, WANT_EIG | WANT_VEL)
    out = similar(Es)
    check(ccall((:abz_rule_ggr, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Float64}), r.h, Es, length(Es), out))
    return out
end

# ---------------------------------------------------------------- LTM
"""
    ltm(h, Es; npt=50, cumulative=false)

Linear tetrahedron DOS g(E) (or, with `cumulative`, the number of states N(E)) from the eigenvalues of the FULL `npt^d`
grid (`abz_rule_ltm`); the reference plans this method (src/dos_algorithms.jl:1-7).
"""
function ltm(h::FourierSeries{S,N}, Es::Vector{Float64}; npt=50, cumulative::Bool=false) where {S,N}
    hs = HIPSeries(h)
    r = rule!(hs, npt, nothing, WANT_EIG)
    out = similar(Es)
    check(ccall((:abz_rule_ltm, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}), r.h, Es, length(Es),
        cumulative ? 1 : 0, out))
    return out
end

"""
    ltm_elements!(r, A)

Attach matrix elements `A[b, k, c]` (band, node, component: the memory order of the C array `[ncomp][nk][n]`, nodes and
bands as `export_rule` orders the eigenvalues) to a full-grid rule with eigenvalues (`abz_rule_ltm_elements`);
`nothing` drops them.  A rebuild of the rule drops them too.
"""
function ltm_elements!(r::HIPRule, A::Union{Nothing,Array{Float64,3}})
    if A === nothing
        check(ccall((:abz_rule_ltm_elements, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), r.h, C_NULL, 0))
    else
        check(ccall((:abz_rule_ltm_elements, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), r.h, A, size(A, 3)))
    end
    return r
end

"""
    ltm_orbitals!(r; orbitals=nothing)        -> number of components

Attach the orbital weights `|U[a, b](k)|^2` of the listed orbitals (1-based; `nothing`: all `n <= 16`) as matrix elements,
computed on the device from `H(k)` (`abz_rule_ltm_orbitals`): the orbital-projected DOS is then `ltm_weighted(r, Es; ncomp)`.
"""
function ltm_orbitals!(r::HIPRule; orbitals::Union{Nothing,AbstractVector{<:Integer}}=nothing)
    if orbitals === nothing
        check(ccall((:abz_rule_ltm_orbitals, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint), r.h, C_NULL, 0))
    else
        o = Cint[a - 1 for a in orbitals]
        check(ccall((:abz_rule_ltm_orbitals, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint), r.h, o, length(o)))
    end
    nc = Ref{Cint}(0)
    check(ccall((:abz_rule_ltm_elements_export, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Float64}), r.h, nc, C_NULL))
    return Int(nc[])
end

"""
    ltm_expectation!(r, ops; components=nothing)   -> number of components

Attach the band expectation values `q_i = Re u_b' * Hermitian(O_i(k)) * u_b` of the operator rules `ops` (1 to 8 rules of the
same grid that hold `H` planes, in the Wannier basis of `r`'s series) as matrix elements, computed on the device
(`abz_rule_ltm_expectation`).  `components`: `nothing` for the expectations in order, or a vector of at most 16 entries, each an
operator index `i` (1-based: `q_i`) or a pair `(i, j)` (the product `q_i q_j`).  At a degenerate level only the sum of single
expectations over the level is defined.
"""
function ltm_expectation!(r::HIPRule, ops::AbstractVector{HIPRule}; components=nothing)
    hs = Ptr{Cvoid}[o.h for o in ops]
    if components === nothing
        GC.@preserve ops check(ccall((:abz_rule_ltm_expectation, libabz), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Ptr{Cint}, Cint),
                                     r.h, hs, length(hs), C_NULL, 0))
        return length(hs)
    end
    comps = Cint[]
    for c in components
        i, j = c isa Integer ? (c, 0) : (c[1], c[2])
        push!(comps, i - 1, j - 1)
    end
    GC.@preserve ops check(ccall((:abz_rule_ltm_expectation, libabz), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Ptr{Cint}, Cint),
                                 r.h, hs, length(hs), comps, length(comps) ÷ 2))
    return length(comps) ÷ 2
end

"""
    ltm_elements_export(r, n)                 -> A[b, k, c] or nothing

The attached matrix elements back on the host, in the order `ltm_elements!` takes them (`abz_rule_ltm_elements_export`);
`n`: the number of bands.
"""
function ltm_elements_export(r::HIPRule, n::Integer)
    nc = Ref{Cint}(0)
    check(ccall((:abz_rule_ltm_elements_export, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Float64}), r.h, nc, C_NULL))
    nc[] == 0 && return nothing
    A = Array{Float64,3}(undef, n, r.nk, Int(nc[]))
    check(ccall((:abz_rule_ltm_elements_export, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Float64}), r.h, nc, A))
    return A
end

"""
    ltm_weighted(r, Es; ncomp, energy=false, cumulative=false, correction=false)

`g_A(E)` (or `N_A(E)` with `cumulative`) of the attached elements, `ncomp` of them, or with `energy` of `A = e` itself
(`abz_rule_ltm_weighted`): a matrix `[ncomp, nE]`.  `correction` (with `cumulative`): `N_A` with Bloechl's curvature
correction (`LTM_STATES_CORRECTED`), which removes the leading `O(1/npt^2)` error of a sum taken at fixed filling, i.e.
at the level `ltm_fermi` finds on the same grid; at a fixed energy an error of that order remains.
"""
function ltm_weighted(r::HIPRule, Es::Vector{Float64}; ncomp::Integer=1, energy::Bool=false, cumulative::Bool=false,
        correction::Bool=false)
    correction && !cumulative && throw(ArgumentError("ltm_weighted: correction corrects N_A: it needs cumulative=true"))
    out = Matrix{Float64}(undef, energy ? 1 : ncomp, length(Es))
    check(ccall((:abz_rule_ltm_weighted, libabz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Cint, Ptr{Float64}), r.h,
        energy ? 1 : 0, Es, length(Es), correction ? LTM_STATES_CORRECTED : (cumulative ? 1 : 0), out))
    return out
end

"""
    ltm_optimized(r, Es; ncomp=0, energy=false, cumulative=false)

The sums of `ltm` / `ltm_weighted` by the optimized tetrahedron method of Kawamura, Gohda and Tsuneyuki, PRB 89, 094515
(`abz_rule_ltm_optimized`, `d = 3`): every simplex takes the band and the elements at its 4 corners and 16 neighbouring grid
points, and the closed forms run on the corner values of the linear function closest to the cubic through the 20 values.
`ncomp = 0`: `g(E)` or `N(E)` (`LTM_A_ONE`); `energy`: `A = e`; `ncomp > 0`: the attached elements.  A matrix
`[max(ncomp, 1), nE]`.  There is no correction: this rule replaces it.
"""
function ltm_optimized(r::HIPRule, Es::Vector{Float64}; ncomp::Integer=0, energy::Bool=false, cumulative::Bool=false)
    source = energy ? LTM_A_ENERGY : (ncomp > 0 ? LTM_A_ELEMENTS : LTM_A_ONE)
    out = Matrix{Float64}(undef, source == LTM_A_ELEMENTS ? ncomp : 1, length(Es))
    check(ccall((:abz_rule_ltm_optimized, libabz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Cint, Ptr{Float64}), r.h,
        source, Es, length(Es), cumulative ? LTM_STATES : LTM_DOS, out))
    return out
end

"""
    ltm_fermi(r, nstates; tol=1e-10)

`(E_F, N(E_F))` of `nstates` states per unit cell, `0 < nstates < n`, to within `tol` (`abz_rule_ltm_fermi`).
"""
function ltm_fermi(r::HIPRule, nstates::Real; tol::Real=1e-10)
    ef = Ref{Float64}(0.0); nf = Ref{Float64}(0.0)
    check(ccall((:abz_rule_ltm_fermi, libabz), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}), r.h,
        Float64(nstates), Float64(tol), ef, nf))
    return ef[], nf[]
end

"""
    ltm_unfold(r, syms, ::Val{d})            -> HIPRule
    ltm_unfold!(u, r, syms, ::Val{d})        -> u

Full-grid eigenvalue rule filled from the irreducible nodes of the symmetric rule `r` (built with `WANT_EIG` under `syms`) by a
gather on the device, `e_b(S k) = e_b(k)` (`abz_rule_ltm_unfold`); the symmetries must be symmetries of `H`.  The result serves
`ltm_weighted`, `ltm_elements!`, `ltm_fermi` and `export_rule` like a rule of `rule!(hs, npt, nothing, WANT_EIG)`.  After new
coefficients and a rebuild of `r`, `ltm_unfold!` gathers again into `u` through the orbit map it already holds.
"""
function ltm_unfold(r::HIPRule, syms, ::Val{d}) where {d}
    S = Cint[round(Int, M[a, b]) for M in syms for a in 1:d for b in 1:d]   # row-major per matrix
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:abz_rule_ltm_unfold, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint, Ptr{Ptr{Cvoid}}), r.h, S, length(syms), ref))
    u = HIPRule(ref[], r.npt^d, r.npt, 1)
    finalizer(x -> ccall((:abz_rule_destroy, libabz), Cint, (Ptr{Cvoid},), x.h), u)
end
function ltm_unfold!(u::HIPRule, r::HIPRule, syms, ::Val{d}) where {d}
    S = Cint[round(Int, M[a, b]) for M in syms for a in 1:d for b in 1:d]
    ref = Ref{Ptr{Cvoid}}(u.h)
    check(ccall((:abz_rule_ltm_unfold, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint, Ptr{Ptr{Cvoid}}), r.h, S, length(syms), ref))
    return u
end

function _pair_comps(components)
    components === nothing && return (C_NULL, 0, Cint[])
    flat = Cint[]
    for (i, j, part) in components
        push!(flat, i - 1, j - 1, part)
    end
    return (pointer(flat), length(components), flat)
end
function _ltm_pairs(ref, r::HIPRule, lower::UnitRange, upper::UnitRange, ops::AbstractVector{HIPRule}, components)
    hs = Ptr{Cvoid}[o.h for o in ops]
    pc, nc, keep = _pair_comps(components)
    GC.@preserve ops hs keep check(ccall((:abz_rule_ltm_pairs, libabz), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Ptr{Cvoid}}, Cint, Ptr{Cint}, Cint, Ptr{Ptr{Cvoid}}),
        r.h, first(lower) - 1, length(lower), first(upper) - 1, length(upper), isempty(hs) ? C_NULL : pointer(hs), length(hs), pc, nc, ref))
end
"""
    ltm_pairs(r, lower, upper; ops=HIPRule[], components=nothing)        -> HIPRule
    ltm_pairs!(p, r, lower, upper; ops=HIPRule[], components=nothing)    -> p
    ltm_bands(r)                                                         -> Int

Pair rule of the band ranges `lower` and `upper` (`UnitRange`s of 1-based ascending bands, `lower` below `upper`, at most 64 pairs)
of the whole-grid rule `r` (`abz_rule_ltm_pairs`): its eigenvalue planes are the differences `e_c(k) - e_v(k)`, pseudo-band
`(v - v0) nc + (c - c0)`, so `ltm_weighted` and the other tetrahedron scans on it give the joint density of states.  With `ops`
(1..4 rules that hold H planes of operator series on the same grid, as for `ltm_expectation!`) it carries the interband products of
`M^i_vc = u_v' Hermitian(O_i) u_c` as attached elements; `components`: `nothing` for `|M^i|^2` of every operator, or at most 16
entries `(i, j, part)`, 1-based operators, `part` 0 for `Re` and 1 for `Im` of `M^i_vc conj(M^j_vc)`.  At a degenerate level only
the sum of a component over all pairs between two levels is defined; the ranges are whole bands (no occupation factors).
`ltm_pairs!` fills `p` again after `r` was rebuilt; `ltm_bands` is the number of bands a rule's planes hold (`nv nc` here).
"""
function ltm_pairs(r::HIPRule, lower::UnitRange, upper::UnitRange; ops::AbstractVector{HIPRule}=HIPRule[], components=nothing)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    _ltm_pairs(ref, r, lower, upper, ops, components)
    p = HIPRule(ref[], r.nk, r.npt, 1)
    finalizer(x -> ccall((:abz_rule_destroy, libabz), Cint, (Ptr{Cvoid},), x.h), p)
end
function ltm_pairs!(p::HIPRule, r::HIPRule, lower::UnitRange, upper::UnitRange; ops::AbstractVector{HIPRule}=HIPRule[], components=nothing)
    ref = Ref{Ptr{Cvoid}}(p.h)
    _ltm_pairs(ref, r, lower, upper, ops, components)
    return p
end
"""
    ltm_pairs_occupied(r, p, ws, fermi; ncomp=0, cumulative=false)       -> Matrix [max(ncomp, 1), nw]

The scans of the pair rule `p` of the whole-grid rule `r` with the T = 0 occupations of a metal inside every simplex
(`abz_rule_ltm_pairs_occupied`): `theta(fermi - e_v) theta(e_c - fermi)` restricts each simplex to its occupied part, which is cut
into sub-simplices and goes through the closed forms of `ltm_weighted`.  `ncomp = 0`: the occupied joint density of states
(`A = 1`, `LTM_A_ONE`); `ncomp > 0`: the `ncomp` attached interband products of `p`.  `cumulative`: `theta(w - Delta)` in place of
`delta`.  A corner is occupied iff `e_v <= fermi` and empty iff `e_c > fermi`; `ltm_fermi(r, nstates)` gives the grid's own level.
"""
function ltm_pairs_occupied(r::HIPRule, p::HIPRule, ws::Vector{Float64}, fermi::Real; ncomp::Integer=0, cumulative::Bool=false)
    out = Matrix{Float64}(undef, max(ncomp, 1), length(ws))
    check(ccall((:abz_rule_ltm_pairs_occupied, libabz), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Ptr{Float64}, Cint, Cint, Ptr{Float64}),
        r.h, p.h, Float64(fermi), ncomp > 0 ? LTM_A_ELEMENTS : LTM_A_ONE, ws, length(ws), cumulative ? LTM_STATES : LTM_DOS, out))
    return out
end
"""
    ltm_elements_ptr(r) -> (base::Ptr{Cvoid}, nbytes::Int, ncomp::Int)

The resident element block of `r` as it lies on the device (`abz_rule_ltm_elements_ptr`): `[nk / npt][ncomp * ltm_bands(r)][row]`
doubles, `row` = `npt` rounded up to a multiple of 16, zeros in the padding columns; `(C_NULL, 0, 0)` when nothing is attached.
"""
function ltm_elements_ptr(r::HIPRule)
    base = Ref{Ptr{Cvoid}}(C_NULL); nb = Ref{Int64}(0); nc = Ref{Cint}(0)
    check(ccall((:abz_rule_ltm_elements_ptr, libabz), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Cint}), r.h, base, nb, nc))
    return base[], Int(nb[]), Int(nc[])
end
function ltm_bands(r::HIPRule)
    nb = Ref{Cint}(0)
    check(ccall((:abz_rule_ltm_bands, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}), r.h, nb))
    return Int(nb[])
end

"""
    ltm_halo!(r)                              -> r

Attach the halo plane to a slab rule with eigenvalues (`abz_rule_ltm_halo`): the one plane behind the slab, built by the
slab's own builder and owned by `r`.  `ltm_weighted(r, Es; energy=true, ...)` and `abz_rule_ltm` then return the slab's
partial sum, with the whole grid's weights; the slabs of a partition of the outermost variable add up to the grid's value.
"""
function ltm_halo!(r::HIPRule)
    check(ccall((:abz_rule_ltm_halo, libabz), Cint, (Ptr{Cvoid},), r.h))
    return r
end

"""
    ltm_green(r, zs)                          -> Vector{ComplexF64}

Trace of the Green's function `tr G(z) = sum_b int dk / (z - e_b(k))` at the complex energies `zs` (`Im z != 0`), per unit
cell, by the tetrahedron method on the eigenvalues of a whole-grid rule (`abz_rule_ltm_green`): `-imag(tr G(E + im*eta)) / pi`
is the DOS broadened by `eta`, with the interpolation error `O(1/npt^2)` whatever `eta` is.
"""
function ltm_green(r::HIPRule, zs::Vector{ComplexF64})
    out = Vector{ComplexF64}(undef, length(zs))
    check(ccall((:abz_rule_ltm_green, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Float64}), r.h, zs, length(zs), out))
    return out
end

"""
    ltm_green_weighted(r, zs; ncomp, energy=false)   -> Matrix{ComplexF64} [ncomp, nz]

The Green's function with matrix elements, `G_A,c(z) = sum_b int dk A_cb(k) / (z - e_b(k))`, of the attached elements, `ncomp`
of them, or with `energy` of `A = e` itself (`abz_rule_ltm_green_weighted`).  With the orbital weights of `ltm_orbitals!`
attached it is the diagonal `G_aa(z)` of the local Green's function; `-imag(G_aa(E + im*eta)) / pi` is the projected DOS
broadened by `eta`.
"""
function ltm_green_weighted(r::HIPRule, zs::Vector{ComplexF64}; ncomp::Integer=1, energy::Bool=false)
    out = Matrix{ComplexF64}(undef, energy ? 1 : ncomp, length(zs))
    check(ccall((:abz_rule_ltm_green_weighted, libabz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}), r.h,
        energy ? 1 : 0, zs, length(zs), out))
    return out
end

"""
    ltm_green_optimized(r, zs; ncomp=0, energy=false)   -> Matrix{ComplexF64} [max(ncomp, 1), nz]

`ltm_green` / `ltm_green_weighted` by the optimized tetrahedron method (`abz_rule_ltm_green_optimized`, `d = 3`): the closed
forms of the Green's function on the effective corner values of `ltm_optimized`, so that `-imag(G(E + im*eta)) / pi` tends to
`ltm_optimized(r, [E])` as `eta -> 0`.  `ncomp = 0`: the trace (`LTM_A_ONE`); `energy`: `A = e`; `ncomp > 0`: the attached
elements.
"""
function ltm_green_optimized(r::HIPRule, zs::Vector{ComplexF64}; ncomp::Integer=0, energy::Bool=false)
    source = energy ? LTM_A_ENERGY : (ncomp > 0 ? LTM_A_ELEMENTS : LTM_A_ONE)
    out = Matrix{ComplexF64}(undef, source == LTM_A_ELEMENTS ? ncomp : 1, length(zs))
    check(ccall((:abz_rule_ltm_green_optimized, libabz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}), r.h,
        source, zs, length(zs), out))
    return out
end

"""
    ltm_projectors!(r, pairs)                 -> number of components

Attach the band projectors `P^b[p, q](k) = U[p, b] * conj(U[q, b])` of the orbital pairs `pairs` (1-based tuples `(p, q)`) as
matrix elements, computed on the device from `H(k)` (`abz_rule_ltm_projectors`): one component `|U[p, b]|^2` for `p == q`,
two (`real`, then `imag`) for `p != q`, at most 16 in all, in the order of the pairs.
"""
function ltm_projectors!(r::HIPRule, pairs::AbstractVector{<:Tuple{Integer,Integer}})
    pq = Cint[x - 1 for pr in pairs for x in pr]
    check(ccall((:abz_rule_ltm_projectors, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint), r.h, pq, length(pairs)))
    return sum(p == q ? 1 : 2 for (p, q) in pairs)
end

"""
    ltm_green_matrix(r, zs, n; orbitals=1:n)   -> Array{ComplexF64,3} [m, m, nz]

The local Green's function `G[p, q](z) = sum_b int dk U[p, b] conj(U[q, b]) / (z - e_b(k))` on the listed orbitals of an
`n`-band rule: the diagonal pairs and the pairs `p < q` are dealt into groups of at most 16 components, each attached with
`ltm_projectors!` and scanned with `ltm_green_weighted`; `G[p, q] = G_ReP + im * G_ImP`, `G[q, p] = G_ReP - im * G_ImP`.
Each group repeats the eigen-solve of the grid; the last group stays attached.
"""
function ltm_green_matrix(r::HIPRule, zs::Vector{ComplexF64}, n::Integer; orbitals::AbstractVector{<:Integer}=1:n)
    allunique(orbitals) || throw(ArgumentError("ltm_green_matrix: orbitals names an orbital twice"))
    m = length(orbitals)
    todo = vcat([(a, a) for a in 1:m], [(a, b) for a in 1:m for b in a+1:m])
    groups = [Tuple{Int,Int}[]]
    ncomp = 0
    for (a, b) in todo
        need = a == b ? 1 : 2
        if ncomp + need > 16
            push!(groups, Tuple{Int,Int}[])
            ncomp = 0
        end
        push!(groups[end], (a, b))
        ncomp += need
    end
    G = zeros(ComplexF64, m, m, length(zs))
    for group in groups
        nc = ltm_projectors!(r, [(orbitals[a], orbitals[b]) for (a, b) in group])
        g = ltm_green_weighted(r, zs; ncomp=nc)
        c = 1
        for (a, b) in group
            if a == b
                G[a, a, :] = g[c, :]
                c += 1
            else
                G[a, b, :] = g[c, :] .+ im .* g[c+1, :]
                G[b, a, :] = g[c, :] .- im .* g[c+1, :]
                c += 2
            end
        end
    end
    return G
end

"""
    ltm_node_weights_optimized(r, Es, n; cumulative=true, export_weights=true)  -> Array{Float64,3} [n, nk, nE] or nothing

The integration weights `W[b, k, i] = w_b(k; E_i)` of the optimized tetrahedron rule on an `n`-band whole-grid rule, `d = 3`
(`abz_rule_ltm_node_weights_optimized`): `sum_k sum_b w_b(k; E) A_b(k)` is the `N_A` (`cumulative`) or `g_A` of `ltm_optimized`
for any `A`.  Every simplex scatters the corner weights of the linear rule on its effective corner energies onto its 20 stencil
points, so the weights are not confined to `[0, 1 / nk]`: a node next to the Fermi surface can weigh negative.  At most 16
energies.  The weights stay resident on the rule, in the block that `ltm_density_matrix` reads.
"""
function ltm_node_weights_optimized(r::HIPRule, Es::Vector{Float64}, n::Integer; cumulative::Bool=true, export_weights::Bool=true)
    1 <= length(Es) <= 16 || throw(ArgumentError("ltm_node_weights_optimized: $(length(Es)) energies, a call takes 1..16"))
    out = export_weights ? Array{Float64}(undef, n, r.nk, length(Es)) : nothing
    GC.@preserve Es out check(ccall((:abz_rule_ltm_node_weights_optimized, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}),
                                    r.h, Es, length(Es), cumulative ? LTM_STATES : LTM_DOS, export_weights ? pointer(out) : C_NULL))
    return out
end

"""
    ltm_density_matrix(r, n; orbitals=1:n)     -> Array{ComplexF64,3} [m, m, nE]

The density matrix `rho[p, q](E) = sum_k sum_b w_b(k; E) U[p, b](k) conj(U[q, b](k))` on the listed orbitals of an `n`-band rule,
per unit cell, at the energies of the rule's resident integration weights (`abz_rule_ltm_density_matrix`): the weights of the
last `abz_rule_ltm_node_weights` call contracted with the eigenvectors inside one eigen-solve of the grid.  Those weights say
what `rho` is: occupations, corrected occupations or the spectral-density matrix.  Hermitian to the bit; nothing is attached.
"""
function ltm_density_matrix(r::HIPRule, n::Integer; orbitals::AbstractVector{<:Integer}=1:n)
    allunique(orbitals) || throw(ArgumentError("ltm_density_matrix: orbitals names an orbital twice"))
    all(o -> 1 <= o <= n, orbitals) || throw(ArgumentError("ltm_density_matrix: orbitals outside 1:$n"))
    nE = Ref{Cint}(0)
    check(ccall((:abz_rule_ltm_node_weights_ptr, libabz), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Cint}), r.h, C_NULL, C_NULL, nE))
    nE[] >= 1 || throw(ArgumentError("ltm_density_matrix: the rule holds no integration weights (abz_rule_ltm_node_weights)"))
    out = Array{ComplexF64}(undef, n, n, nE[])  # the library's [nE][p][q] is column-major [q, p, iE]
    GC.@preserve out check(ccall((:abz_rule_ltm_density_matrix, libabz), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), r.h, out))
    rho = permutedims(out, (2, 1, 3))
    return rho[orbitals, orbitals, :]
end

# values of z of the rule's resident complex weights (0: none)
function ltm_green_node_weights_nz(r::HIPRule)
    nz = Ref{Cint}(0)
    check(ccall((:abz_rule_ltm_green_node_weights_ptr, libabz), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Cint}), r.h, C_NULL, C_NULL, nz))
    return Int(nz[])
end

"""
    ltm_green_node_weights!(r, zs, n; export_weights=true)  -> Array{ComplexF64,3} [n, nk, nz] or nothing

The complex integration weights `W[b, k, i] = W_b(k; z_i)` of the Green's function of an `n`-band whole-grid rule
(`abz_rule_ltm_green_node_weights`): `G_A(z) = sum_k sum_b W_b(k; z) A_b(k)` for any `A`.  At most 8 values, `imag(z) != 0`.  The
weights stay resident on the rule for `ltm_green_node_weights_dot`, `_fold` and `_matrix`.
"""
function ltm_green_node_weights!(r::HIPRule, zs::Vector{ComplexF64}, n::Integer; export_weights::Bool=true)
    1 <= length(zs) <= 8 || throw(ArgumentError("ltm_green_node_weights!: $(length(zs)) values of z, a call takes 1..8"))
    out = export_weights ? Array{ComplexF64}(undef, n, r.nk, length(zs)) : nothing
    GC.@preserve zs out check(ccall((:abz_rule_ltm_green_node_weights, libabz), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Cint, Ptr{ComplexF64}),
                                    r.h, zs, length(zs), export_weights ? pointer(out) : C_NULL))
    return out
end

"""
    ltm_green_node_weights_optimized(r, zs, n; export_weights=true)  -> Array{ComplexF64,3} [n, nk, nz] or nothing

The complex integration weights of the optimized tetrahedron rule, `d = 3` (`abz_rule_ltm_green_node_weights_optimized`):
`sum_k sum_b W_b(k; z) A_b(k)` is the `G_A(z)` of `abz_rule_ltm_green_optimized` for any `A`.  At most 8 values, `imag(z) != 0`.
The weights fill the same resident block as those of `ltm_green_node_weights!`: `ltm_green_node_weights_dot`, `_fold` and
`_matrix` work on them as they are.  (Written after the Python binding; not run.)
"""
function ltm_green_node_weights_optimized(r::HIPRule, zs::Vector{ComplexF64}, n::Integer; export_weights::Bool=true)
    1 <= length(zs) <= 8 || throw(ArgumentError("ltm_green_node_weights_optimized: $(length(zs)) values of z, a call takes 1..8"))
    out = export_weights ? Array{ComplexF64}(undef, n, r.nk, length(zs)) : nothing
    GC.@preserve zs out check(ccall((:abz_rule_ltm_green_node_weights_optimized, libabz), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Cint, Ptr{ComplexF64}),
                                    r.h, zs, length(zs), export_weights ? pointer(out) : C_NULL))
    return out
end

"""
    ltm_green_node_weights_dot(r, ncomp)  -> Matrix{ComplexF64} [ncomp, nz]

The resident complex weights against the `ncomp` attached element components (`abz_rule_ltm_green_node_weights_dot`).
"""
function ltm_green_node_weights_dot(r::HIPRule, ncomp::Integer)
    nz = ltm_green_node_weights_nz(r)
    nz >= 1 || throw(ArgumentError("ltm_green_node_weights_dot: the rule holds no complex weights (ltm_green_node_weights!)"))
    out = Matrix{ComplexF64}(undef, ncomp, nz)
    GC.@preserve out check(ccall((:abz_rule_ltm_green_node_weights_dot, libabz), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), r.h, out))
    return out
end

"""
    ltm_green_node_weights_fold(r, n, nirr)  -> Array{ComplexF64,3} [n, nirr, nz]

For a rule of `abz_rule_ltm_unfold`: the resident complex weights summed over each orbit onto the `nirr` nodes of the source rule
(`abz_rule_ltm_green_node_weights_fold`).
"""
function ltm_green_node_weights_fold(r::HIPRule, n::Integer, nirr::Integer)
    nz = ltm_green_node_weights_nz(r)
    nz >= 1 || throw(ArgumentError("ltm_green_node_weights_fold: the rule holds no complex weights (ltm_green_node_weights!)"))
    out = Array{ComplexF64}(undef, n, nirr, nz)
    GC.@preserve out check(ccall((:abz_rule_ltm_green_node_weights_fold, libabz), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), r.h, out))
    return out
end

"""
    ltm_green_node_weights_matrix(r, n; orbitals=1:n)  -> Array{ComplexF64,3} [m, m, nz]

The local Green's function `G[p, q](z) = sum_k sum_b W_b(k; z) U[p, b](k) conj(U[q, b](k))` from the resident complex weights and
the eigenvectors (`abz_rule_ltm_green_node_weights_matrix`); nothing is attached.  `G(z)' == G(conj(z))`.
"""
function ltm_green_node_weights_matrix(r::HIPRule, n::Integer; orbitals::AbstractVector{<:Integer}=1:n)
    allunique(orbitals) || throw(ArgumentError("ltm_green_node_weights_matrix: orbitals names an orbital twice"))
    all(o -> 1 <= o <= n, orbitals) || throw(ArgumentError("ltm_green_node_weights_matrix: orbitals outside 1:$n"))
    nz = ltm_green_node_weights_nz(r)
    nz >= 1 || throw(ArgumentError("ltm_green_node_weights_matrix: the rule holds no complex weights (ltm_green_node_weights!)"))
    out = Array{ComplexF64}(undef, n, n, nz)  # the library's [nz][p][q] is column-major [q, p, iz]
    GC.@preserve out check(ccall((:abz_rule_ltm_green_node_weights_matrix, libabz), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), r.h, out))
    G = permutedims(out, (2, 1, 3))
    return G[orbitals, orbitals, :]
end

# ---------------------------------------------------------------- cached rule -> the reference's own containers
"""
    export_rule(r, hs; H=true, eig=false, vel=false)

Host copies of a cached rule in the reference's layout -- `(x, w, H, eig, vel)` with `x :: Vector{SVector{d}}`, integer-valued
weights `w`, `H :: Vector{SMatrix{n,n,ComplexF64}}` -- i.e. what iterating a `FourierPTR` / `FourierMonkhorstPack` yields
(src/fourier.jl:177-207,279-292).  A user closure under `PTR` is fed from the cached rule through this:
`sum(w[i] * f(FourierValue(x[i], H[i]), p...) for i in eachindex(x)) / (npt^d * nsyms)`.
"""
function export_rule(r::HIPRule, hs::HIPSeries{d}; H::Bool=true, eig::Bool=false, vel::Bool=false) where {d}
    n = hs.n
    x = Matrix{Float64}(undef, d, r.nk); w = Vector{Float64}(undef, r.nk)
    Hb = H ? Array{ComplexF64}(undef, n, n, r.nk) : ComplexF64[]
    Eb = eig ? Matrix{Float64}(undef, n, r.nk) : Float64[]
    Vb = vel ? Array{Float64}(undef, n, d, r.nk) : Float64[]
    GC.@preserve x w Hb Eb Vb begin
        check(ccall((:abz_rule_export, libabz), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Float64}),
            r.h, x, w, H ? pointer(Hb) : C_NULL, eig ? pointer(Eb) : C_NULL, vel ? pointer(Vb) : C_NULL))
    end
    xs = [SVector{d,Float64}(view(x, :, k)) for k in 1:r.nk]
    Hs = H ? [SMatrix{n,n,ComplexF64}(view(Hb, :, :, k)) for k in 1:r.nk] : nothing
    return (x=xs, w=w, H=Hs, eig=eig ? Eb : nothing, vel=vel ? Vb : nothing)
end

"A plain-function integrand under `PTR` fed from the cached rule (src/fourier.jl:204-207): `rule(f, B)`."
function rule_sum(f, r::HIPRule, hs::HIPSeries{d}, args...; kws...) where {d}
    ex = export_rule(r, hs)
    acc = sum(ex.w[i] * f(FourierValue(ex.x[i], ex.H[i]), args...; kws...) for i in eachindex(ex.x))
    return acc / (r.npt^d * r.nsyms)
end

"Drop the rules the library keeps with the series for `abz_autoptr_solve*`."
drop_rules!(hs::HIPSeries) = check(ccall((:abz_series_drop_rules, libabz), Cint, (Ptr{Cvoid},), hs.h))

# ---------------------------------------------------------------- IAI building blocks (a host-language adaptive loop)
# What `abz_iai_solve*` is built from, for a client that keeps its own heaps (e.g. a custom error norm or termination):
# contract the outermost remaining variable at a batch of nodes, evaluate the integrand on innermost lines, apply the
# GK(7,15) rule to batches of panels.  Replaces workspace_contract! / workspace_evaluate! (src/fourier.jl:445-478) and
# QuadGK.evalrule on a batch.
"15 Kronrod nodes of the panel `(a, b)` in the library's (and the reference's) order."
function gk15_nodes(a::Real, b::Real)
    x = Vector{Float64}(undef, 15)
    check(ccall((:abz_gk15_nodes, libabz), Cint, (Cdouble, Cdouble, Ptr{Float64}), a, b, x))
    return x
end

"GK(7,15) on `npanels` panels: `ab` is 2 x npanels, `values` ncomp x 15 x npanels -> `(I :: ncomp x npanels, E)`."
function gk15_batch(ab::Matrix{Float64}, values::Array{ComplexF64,3})
    ncomp, np = size(values, 1), size(values, 3)
    (size(ab) == (2, np) && size(values, 2) == 15) || throw(ArgumentError("gk15_batch: ab is 2 x npanels, values ncomp x 15 x npanels"))
    I = Matrix{ComplexF64}(undef, ncomp, np); E = Vector{Float64}(undef, np)
    GC.@preserve ab values I E check(ccall((:abz_gk15_batch, libabz), Cint,
        (Ptr{Float64}, Ptr{ComplexF64}, Int64, Cint, Ptr{ComplexF64}, Ptr{Float64}), ab, values, np, ncomp, I, E))
    return I, E
end

"""
Contract the outermost remaining variable of the level-`src_level` sets `parents` (slot 0 at level d = the series) at `x`: slots of the new sets.
Slots are numbered consecutively per level from the level's current count and stay valid until `release_level!`, an IAI solve or
`update!` of the series; a parent that is not a live slot is an `ArgumentError` (checked by the library before any device work).
"""
function contract_nodes(hs::HIPSeries, src_level::Integer, parents::Vector{Int64}, x::Vector{Float64})
    length(parents) == length(x) || throw(ArgumentError("contract_nodes: one parent per node"))
    slots = Vector{Int64}(undef, length(x))
    GC.@preserve parents x slots check(ccall((:abz_contract_nodes, libabz), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}), hs.h, src_level, parents, x, length(x), slots))
    return slots
end

"Integrand values at innermost nodes `x` of the level-1 sets `parents` (`tail`: (d-1) x nnodes outer coordinates, for `F_LINEAR_X` only)."
function eval_line_nodes(hs::HIPSeries, parents::Vector{Int64}, x::Vector{Float64}, f::HIPIntegrand, params::Vector{Float64}, sweep::Real,
                         ncomp::Integer; tail::Union{Nothing,Matrix{Float64}}=nothing)
    vals = Matrix{ComplexF64}(undef, ncomp, length(x))
    tp = tail === nothing ? Ptr{Float64}(C_NULL) : pointer(tail)
    GC.@preserve parents x params vals tail check(ccall((:abz_eval_line_nodes, libabz), Cint,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int64, Cint, Ptr{Float64}, Cint, Cdouble, Ptr{ComplexF64}),
        hs.h, parents, x, tp, length(x), fid(f), params, length(params), sweep, vals))
    return vals
end

"Drop every contracted set below `level` (the client's loop is done with them)."
release_level!(hs::HIPSeries, level::Integer) = check(ccall((:abz_release_level, libabz), Cint, (Ptr{Cvoid}, Cint), hs.h, level))

# ---------------------------------------------------------------- the rest of abzhip.h (housekeeping)
"""(live device bytes, cached device bytes, this context's scratch bytes, its pinned host bytes, live blocks)"""
function mem_info(; ctx::HIPContext=context())
    info = zeros(Int64, 5)
    check(ccall((:abz_mem_info, libabz), Cint, (Ptr{Cvoid}, Ptr{Int64}), ctx.h, info))
    return Tuple(info)
end

version() = Int(ccall((:abz_version, libabz), Cint, ()))
function device_count()
    n = Ref{Cint}(0)
    check(ccall((:abz_device_count, libabz), Cint, (Ptr{Cint},), n))
    return Int(n[])
end
synchronize(ctx::HIPContext=context()) = check(ccall((:abz_ctx_sync, libabz), Cint, (Ptr{Cvoid},), ctx.h))

"New coefficients of the same shape (mutating `h.c`, test/dos.jl:122-129); cached rules go stale until `rebuild!`."
function update!(hs::HIPSeries, s::FourierSeries)
    coef = reinterpret(Float64, vec(s.c))
    GC.@preserve coef check(ccall((:abz_series_update, libabz), Cint, (Ptr{Cvoid}, Ptr{Float64}), hs.h, coef))
    try
        foreach(rebuild!, values(hs.rules))   # cached rule values follow the coefficients (the reference rebuilds its rule per solve)
    catch err
        # an upper-triangle (WANT_H_COMPACT) rule cannot be refilled from a series that stopped being Hermitian
        # (ABZ_ERR_ARG -> ArgumentError): drop the cache, the next solve builds full-layout rules
        err isa ArgumentError || rethrow()
        empty!(hs.rules)
    end
    return hs
end
const PIVOT_NONE = Cint(0)
const PIVOT_PARTIAL = Cint(1)
"""
`:none` (the default routes) or `:partial`: every inverse of (omega + i eta) I - H(k) taken for this series -- rule scans,
store-free sums, AutoPTR and IAI solves -- pivots by rows like LAPACK's `inv` (abz_series_set_pivoting).  Read at launch
time: rules built before the call follow it, `update!` keeps it.
"""
function set_pivoting!(hs::HIPSeries, mode::Symbol)
    mode in (:none, :partial) || throw(ArgumentError("pivoting must be :none or :partial, not $(repr(mode))"))
    check(ccall((:abz_series_set_pivoting, libabz), Cint, (Ptr{Cvoid}, Cint), hs.h, mode === :partial ? PIVOT_PARTIAL : PIVOT_NONE))
    return hs
end
function pivoting(hs::HIPSeries)
    m = Ref{Cint}(0)
    check(ccall((:abz_series_get_pivoting, libabz), Cint, (Ptr{Cvoid}, Ptr{Cint}), hs.h, m))
    return m[] == PIVOT_PARTIAL ? :partial : :none
end
"Context on a stream the caller owns (e.g. AMDGPU.jl's task-local HIP stream): launches are ordered with the caller's work."
function HIPContext(device::Integer, stream::Ptr{Cvoid})
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:abz_ctx_create_on_stream, libabz), Cint, (Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), device, stream, ref))
    ctx = HIPContext(ref[], Val(:adopt))
    finalizer(c -> ccall((:abz_ctx_destroy, libabz), Cint, (Ptr{Cvoid},), c.h), ctx)
end
"abz_rule_reduce with device-resident sweep values and sums (both `Ptr{Cvoid}` device addresses): no host round trip."
function reduce_rule_device!(out_dev::Ptr{Cvoid}, r::HIPRule, f::HIPIntegrand, params::Vector{Float64}, sweep_dev::Ptr{Cvoid}, nsweep::Integer, nsyms::Integer=r.nsyms)
    GC.@preserve params check(ccall((:abz_rule_reduce_device, libabz), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}),
        r.h, fid(f), params, length(params), sweep_dev, nsweep, nsyms, out_dev))
    return out_dev
end
"""
    shard_iai!(hs, allgather!, rank, world)

One IAI solve on several GPUs (`abz_iai_set_exchange`): `allgather!(buf::Vector{Float64}, per_rank::Int)` must fill every
rank's segment of `buf` (MPI.Allgather!(MPI.IN_PLACE, UBuffer(buf, per_rank), comm) does).  All ranks then call the solver
with the same arguments and get the single-GPU result bit for bit.  Pass `nothing` to switch it off.
"""
function shard_iai!(hs::HIPSeries, allgather!, rank::Integer, world::Integer)
    if allgather! === nothing
        check(ccall((:abz_iai_set_exchange, libabz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), hs.h, C_NULL, C_NULL, 0, 1))
        return hs
    end
    cb = (user::Ptr{Cvoid}, buf::Ptr{Float64}, per::Int64) -> begin
        try
            allgather!(unsafe_wrap(Array, buf, Int(per) * Int(world)), Int(per)); Cint(0)
        catch
            Cint(1)
        end
    end
    fptr = @cfunction($cb, Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64))
    hs.exchange = fptr                                   # keep the closure alive with the series
    check(ccall((:abz_iai_set_exchange, libabz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
                hs.h, Base.unsafe_convert(Ptr{Cvoid}, fptr), C_NULL, rank, world))
    return hs
end
"Device address and size of the rule's value block (tiled planar layout, DESIGN.md section 3)."
function values_ptr(r::HIPRule)
    base = Ref{Ptr{Cvoid}}(C_NULL); nb = Ref{Int64}(0)
    check(ccall((:abz_rule_values_ptr, libabz), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Int64}), r.h, base, nb))
    return base[], nb[]
end
rebuild!(r::HIPRule) = (check(ccall((:abz_rule_rebuild, libabz), Cint, (Ptr{Cvoid},), r.h)); r)

function rule_info(r::HIPRule)
    nk = Ref{Int64}(0); n = Ref{Cint}(0); d = Ref{Cint}(0); npt = Ref{Cint}(0); want = Ref{Cint}(0)
    check(ccall((:abz_rule_info, libabz), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
                r.h, nk, n, d, npt, want))
    return (nk=nk[], n=Int(n[]), d=Int(d[]), npt=Int(npt[]), want=want[])
end

"`symptr_rule` with the orbit tables computed on the GPU (bit-identical to the host version, ~50x faster on large grids)."
function symptr_rule_device(npt, ::Val{d}, syms; ctx::HIPContext=context()) where {d}
    S = Cint[round(Int, M[a, b]) for M in syms for a in 1:d for b in 1:d]   # row-major per matrix
    nirr = Ref{Int64}(0)
    check(ccall((:abz_symptr_rule_device, libabz), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cint}, Cint, Ptr{Int64}, Ptr{Cint}, Ptr{Int64}),
                ctx.h, npt, d, S, length(syms), nirr, C_NULL, C_NULL))   # first call: count
    idx = Matrix{Cint}(undef, d, nirr[]); w = Vector{Int64}(undef, nirr[])
    check(ccall((:abz_symptr_rule_device, libabz), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cint}, Cint, Ptr{Int64}, Ptr{Cint}, Ptr{Int64}),
                ctx.h, npt, d, S, length(syms), nirr, idx, w))
    return idx, w
end

"HIP-event timing of the library's own launches: `prof_enable(true)`, run, `prof_read(K_EVAL)` -> (ms, launches)."
const K_CONTRACT, K_EVAL, K_REDUCE, K_GGR, K_EIG, K_GGRBUILD = Cint.(0:5)
prof_enable(on::Bool=true; ctx::HIPContext=context()) =
    check(ccall((:abz_prof_enable, libabz), Cint, (Ptr{Cvoid}, Cint), ctx.h, on ? 1 : 0))
prof_reset(; ctx::HIPContext=context()) = check(ccall((:abz_prof_reset, libabz), Cint, (Ptr{Cvoid},), ctx.h))
function prof_read(kernel::Cint; ctx::HIPContext=context())
    ms = Ref{Float64}(0.0); n = Ref{Int64}(0)
    check(ccall((:abz_prof_read, libabz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Int64}), ctx.h, kernel, ms, n))
    return ms[], n[]
end

end # module
