# LevenbergMarquardtHIP.jl -- drop-in for src/LevenbergMarquardt.jl (4 positional arguments, what src/solve_ba.jl:26
# calls) AND src/lm.jl (5 positional arguments with `linesearch`: src/main.jl:30, src/diffprecsions.jl:41,
# src/benchmark_diffprec.jl:42-89).  Same function name, keywords and return type (GenericExecutionStats); the loop
# itself runs in libba_hip.so (ba_lm_solve), which follows the two reference loops line by line.
using NLPModels
using SolverTools
include("BALHIP.jl")

_tol(v) = v === nothing ? -1.0 : Float64(v)   # negative = "the variant's eps-derived default" (include/ba_hip.h)

# robust loss (an extension, scipy's least_squares names): f = 1/2 sum_i c^2 rho(|r_i|^2 / c^2), c = f_scale (pixels);
# include/ba_hip.h, ba_lm_set_loss.  Set on the handle at every call: a call without `loss` runs the plain objective.
const BA_LOSSES = (:linear, :huber, :soft_l1, :cauchy, :arctan)
function _ba_set_loss(nlp, loss :: Symbol, f_scale :: Real)
  k = findfirst(==(loss), BA_LOSSES)
  k === nothing && error("loss must be one of $(BA_LOSSES)")
  (isfinite(f_scale) && f_scale > 0) || error("f_scale must be finite and > 0")
  bacheck(ccall((:ba_lm_set_loss, libba), Cint, (Ptr{Cvoid}, Cint, Cdouble), nlp.handle, Cint(k - 1), Float64(f_scale)))
end

# fixed parameters (an extension): include/ba_hip.h, ba_lm_set_fixed.  fixed_cameras / fixed_points: 1-based indices or a
# Bool vector of length ncams / npnts; fixed_camera_params: names among (:r, :t, :k1, :k2, :f) applied to every camera, or a
# Bool (ncams, 9) matrix in block order r1 r2 r3 t1 t2 t3 k1 k2 f.  OR-ed.  Set on the handle at every call.
const BA_CAMERA_PARAMS = Dict(:r => 0x0007, :t => 0x0038, :k1 => 0x0040, :k2 => 0x0080, :f => 0x0100)
function _ba_fixed_set(v, n :: Int, what)
  v === nothing && return falses(n)
  if eltype(v) == Bool
    length(v) == n || error("$what: a Bool vector must have length $n")
    return collect(v)
  end
  out = falses(n)
  for i in v
    (1 <= i <= n) || error("$what: 1-based indices must lie in 1..$n, got $i")
    out[i] = true
  end
  return out
end
function _ba_set_fixed(nlp, fixed_cameras, fixed_points, fixed_camera_params, ft :: Int)
  cam = zeros(UInt16, nlp.ncams)
  cam[_ba_fixed_set(fixed_cameras, nlp.ncams, "fixed_cameras")] .= 0x01ff
  if fixed_camera_params isa AbstractMatrix{Bool}
    size(fixed_camera_params) == (nlp.ncams, 9) || error("fixed_camera_params: a Bool matrix must be ($(nlp.ncams), 9)")
    for c in 1:nlp.ncams, b in 1:9
      fixed_camera_params[c, b] && (cam[c] |= UInt16(1) << (b - 1))
    end
  elseif fixed_camera_params !== nothing
    for name in fixed_camera_params
      haskey(BA_CAMERA_PARAMS, name) || error("fixed_camera_params: names among $(keys(BA_CAMERA_PARAMS))")
      cam .|= BA_CAMERA_PARAMS[name]
    end
  end
  pnt = UInt8.(_ba_fixed_set(fixed_points, nlp.npnts, "fixed_points"))
  masked = any(!=(0), cam) || any(!=(0), pnt)
  (masked && ft == 2) && error("fixed parameters are not supported with facto_type = Float16")
  GC.@preserve cam pnt begin
    bacheck(ccall((:ba_lm_set_fixed, libba), Cint, (Ptr{Cvoid}, Ptr{UInt16}, Ptr{UInt8}), nlp.handle,
                  any(!=(0), cam) ? pointer(cam) : Ptr{UInt16}(C_NULL), any(!=(0), pnt) ? pointer(pnt) : Ptr{UInt8}(C_NULL)))
  end
end

# Gaussian priors (an extension): include/ba_hip.h, ba_lm_set_priors.  Each of point_priors / camera_priors / centre_priors is
# nothing or a tuple (index, mu, info): 1-based indices (each at most once), mu a (n, d) matrix (d = 3 / 9 / 3: a point, a camera
# block r t k1 k2 f, a camera centre -R(r)'t), info either n symmetric positive semi-definite d x d matrices as a (d, d, n) array
# or standard deviations as a (n, d) matrix (diag(1 / sigma^2), Inf = unconstrained).  Set on the handle at every call.
function _ba_prior_lists(v, d :: Int, n :: Int, what)
  v === nothing && return Int64[], Float64[], Float64[]
  idx, mu, info = v
  m = length(idx)
  (all(i -> 1 <= i <= n, idx) && allunique(idx)) || error("$what: 1-based indices in 1..$n, each at most once")
  size(mu) == (m, d) || error("$what: mu must be ($m, $d)")
  all(isfinite, mu) || error("$what: mu must be finite")
  full = zeros(Float64, d, d, m)
  if ndims(info) == 3
    size(info) == (d, d, m) || error("$what: info must be ($d, $d, $m)")
    all(isfinite, info) || error("$what: info must be finite")
    for k in 1:m
      info[:, :, k] == transpose(info[:, :, k]) || error("$what: the information blocks must be symmetric")
      full[:, :, k] .= info[:, :, k]
    end
  else
    size(info) == (m, d) || error("$what: info must be ($d, $d, $m) blocks or ($m, $d) standard deviations")
    all(s -> s > 0, info) || error("$what: standard deviations must be > 0 (Inf: unconstrained)")
    for k in 1:m, i in 1:d
      full[i, i, k] = 1.0 / info[k, i]^2
    end
  end
  packed = Float64[]                    # lower triangle, row-major: the C layout
  for k in 1:m, i in 1:d, j in 1:i
    push!(packed, full[i, j, k])
  end
  return collect(Int64, idx), vec(permutedims(Float64.(mu))), packed
end
function _ba_set_priors(nlp, point_priors, camera_priors, centre_priors, linesearch :: Bool, ft :: Int, T :: DataType)
  pi, pm, pl = _ba_prior_lists(point_priors, 3, nlp.npnts, "point_priors")
  ci, cm, cl = _ba_prior_lists(camera_priors, 9, nlp.ncams, "camera_priors")
  ti, tm, tl = _ba_prior_lists(centre_priors, 3, nlp.ncams, "centre_priors")
  if length(pi) + length(ci) + length(ti) > 0
    linesearch && error("priors are not supported with linesearch = true")
    ft == 2 && error("priors are not supported with facto_type = Float16")
    T == Float32 && error("priors are not supported for a Float32 model")
  end
  GC.@preserve pi pm pl ci cm cl ti tm tl begin
    bacheck(ccall((:ba_lm_set_priors, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble},
                   Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}),
                  nlp.handle, length(pi), pi, pm, pl, length(ci), ci, cm, cl, length(ti), ti, tm, tl))
  end
end

"(point, camera, centre) prior counts the handle holds (ba_lm_get_priors)"
function prior_counts(nlp)
  a, b, c = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
  bacheck(ccall((:ba_lm_get_priors, libba), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), nlp.handle, a, b, c))
  return a[], b[], c[]
end

"""
    prior_eval(nlp, x; point_priors = nothing, camera_priors = nothing, centre_priors = nothing)

`(cost, chi2_points, chi2_cameras, chi2_centres)` at `x` (ba_prior_eval): chi2[k] = d_k' info_k d_k of every prior in the order
given, cost = half their sum, the priors' part of the LM objective.  Sets the handle's priors, as every LM call does.
"""
function prior_eval(nlp, x :: AbstractVector; point_priors = nothing, camera_priors = nothing, centre_priors = nothing)
  _ba_set_priors(nlp, point_priors, camera_priors, centre_priors, false, 0, Float64)
  np, nc, nt = prior_counts(nlp)
  cp, cc, ct = zeros(np), zeros(nc), zeros(nt)
  cost = Ref{Cdouble}(0.0)
  xv = Vector{Float64}(x)
  bacheck(ccall((:ba_prior_eval, libba), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                nlp.handle, xv, cost, cp, cc, ct))
  return cost[], cp, cc, ct
end

# per-observation information (an extension): include/ba_hip.h, ba_lm_set_obs_info.  obs_info: nothing, standard deviations in
# pixels -- a vector (nobs, isotropic) or an (nobs, 2) matrix (sigma_x, sigma_y), Inf = information 0 -- or 2 x 2 x nobs symmetric
# positive semi-definite information matrices.  Packed to the 3 x nobs (xx, xy, yy) layout of set_obs_info (julia/BALHIP.jl).  Set
# on the handle at every call: a call without `obs_info` runs the unweighted path.
function _ba_obs_info(obs_info, nobs :: Int)
  obs_info === nothing && return nothing
  a = Array{Float64}(obs_info)
  out = zeros(Float64, 3, nobs)
  if ndims(a) == 3 && size(a) == (2, 2, nobs)
    all(isfinite, a) || error("obs_info: the information matrices must be finite")
    a[1, 2, :] == a[2, 1, :] || error("obs_info: the information matrices must be symmetric")
    out[1, :] = a[1, 1, :]; out[2, :] = a[1, 2, :]; out[3, :] = a[2, 2, :]
    (any(out[1, :] .< 0) || any(out[3, :] .< 0) || any(out[2, :] .^ 2 .> out[1, :] .* out[3, :])) &&
      error("obs_info: the information matrices must be positive semi-definite")
  elseif (ndims(a) == 1 && length(a) == nobs) || (ndims(a) == 2 && size(a) == (nobs, 2))
    (any(isnan, a) || any(a .<= 0)) && error("obs_info: standard deviations must be > 0 (Inf: dropped)")
    out[1, :] = 1.0 ./ a[:, 1] .^ 2
    out[3, :] = 1.0 ./ a[:, ndims(a)] .^ 2
  else
    error("obs_info: standard deviations (nobs) or (nobs, 2), or information matrices (2, 2, nobs), got $(size(a))")
  end
  return out
end

function _ba_set_obs_info(nlp, obs_info, linesearch :: Bool, ft :: Int, T :: DataType)
  info3 = _ba_obs_info(obs_info, nlp.nobs)
  if info3 !== nothing
    linesearch && error("obs_info is not supported with linesearch = true")
    ft == 2 && error("obs_info is not supported with facto_type = Float16")
    T == Float32 && error("obs_info is not supported for a Float32 model")
  end
  set_obs_info(nlp, info3)
end

# one log row per iteration, the reference's columns (src/lm.jl:120-121,304)
function _ba_log_row(ctx :: Ptr{Cvoid}, iter :: Cint, f :: Cdouble, df :: Cdouble, njtr :: Cdouble, lambda :: Cdouble,
                     ndelta :: Cdouble, rho :: Cdouble, acc :: Cint) :: Cvoid
  @info log_row(Any[Int(iter), f, df, njtr, lambda, ndelta, rho, acc != 0 ? "acc" : "rej"])
  return nothing
end

function _ba_lm(model, variant :: Int, facto :: Symbol, perm :: Symbol, normalize :: Symbol, linesearch :: Bool,
                x :: AbstractVector, facto_type :: DataType, restol, satol, srtol, oatol, ortol, atol, rtol, νd, νm, λ, δd,
                ite_max :: Int, max_time :: Real, pcg_tol :: Real = -1.0, pcg_max_iter :: Int = -1,
                loss :: Symbol = :linear, f_scale :: Real = 1.0, fixed_cameras = nothing, fixed_points = nothing,
                fixed_camera_params = nothing, point_priors = nothing, camera_priors = nothing, centre_priors = nothing,
                obs_info = nothing)
  # :PCG is an extension of the HIP path (no counterpart in the reference): matrix-free conjugate gradients on the reduced
  # camera system, include/ba_hip.h, ba_lm_opts.facto
  facto in (:QR, :LDL, :PCG) || error("facto must be :QR, :LDL or :PCG")
  (facto == :PCG && normalize != :None) && error("facto = :PCG has its own scaling (block-Jacobi preconditioner): normalize must be :None")
  (facto == :PCG && facto_type == Float32 && T != Float32) && error("facto = :PCG runs in Float64: facto_type = Float32 belongs to the direct branches")
  perm in (:AMD, :Metis) || error("perm must be :AMD or :Metis")   # src/lm.jl:84-88: orders the cameras of the reduced system (ba_lm_opts.perm)
  normalize in (:None, :J, :A) || error("normalize must be :None, :J or :A")
  nlp = model.nlp                       # the BALNLPModel inside FeasibilityResidual (src/solve_ba.jl:25)
  T = eltype(x)
  T in (Float64, Float32) || error("the HIP path iterates in Float64 or Float32")
  ft = facto_type == T ? 0 : facto_type == Float32 ? 1 : facto_type == Float16 ? 2 : error("facto_type must be Float64, Float32 or Float16")
  (T == Float32 && ft == 0 && variant == 1) && (ft = 1)   # eltype(x) = Float32: facto_type defaults to it (src/lm.jl:20)
  o = BaLmOpts(variant, facto == :QR ? 1 : facto == :PCG ? 2 : 0, normalize == :None ? 0 : normalize == :J ? 1 : 2, linesearch ? 1 : 0, ft,
               ite_max, 0, T == Float32 ? 1 : 0, _tol(restol), _tol(satol), _tol(srtol), _tol(oatol), _tol(ortol),
               _tol(atol), _tol(rtol), _tol(νd), _tol(νm), _tol(λ), _tol(δd), Float64(max_time), Float64(pcg_tol),
               Cint(pcg_max_iter), Cint(perm == :Metis ? 1 : 0))
  (loss != :linear && linesearch) && error("a robust loss is not supported with linesearch = true")
  _ba_set_loss(nlp, loss, f_scale)
  _ba_set_fixed(nlp, fixed_cameras, fixed_points, fixed_camera_params, ft)
  _ba_set_priors(nlp, point_priors, camera_priors, centre_priors, linesearch, ft, T)
  _ba_set_obs_info(nlp, obs_info, linesearch, ft, T)
  st = BaLmStats()
  xd = Vector{Float64}(x)               # the ABI carries the iterate as doubles (exact for Float32 values)
  cb = @cfunction(_ba_log_row, Cvoid, (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cint))
  @info log_header([:iter, :f, :Δf, :dFeas, :λ, :δ, :ρ, :status], [Int, T, T, T, T, T, T, String],
                   hdr_override = Dict(:f => "f(x)", :dFeas => "‖Jᵀr‖", :δ => "‖δ‖"))
  GC.@preserve xd st begin
    bacheck(ccall((:ba_lm_solve, libba), Cint, (Ptr{Cvoid}, Ref{BaLmOpts}, Ptr{Float64}, Ref{BaLmStats}, Ptr{Cvoid}, Ptr{Cvoid}),
                  nlp.handle, o, xd, st, cb, C_NULL))
  end
  x .= T.(xd)
  # the evaluations happened inside the library: keep the model's counters truthful (src/BALNLPModels.jl:116,126,162)
  nlp.counters.neval_cons += st.n_residual
  nlp.counters.neval_jac += st.n_jacobian + 1
  status = BA_STATUS[st.status + 1]
  if variant == 1   # src/lm.jl:409-415
    return GenericExecutionStats(status, model, solution=x, objective=st.objective, iter=Int(st.iter),
                                 elapsed_time=st.elapsed_s, dual_feas=st.dual_feas)
  else              # src/LevenbergMarquardt.jl:384: |Jᵀr| is reported as primal_feas there
    return GenericExecutionStats(status, model, solution=x, objective=st.objective, iter=Int(st.iter),
                                 elapsed_time=st.elapsed_s, primal_feas=st.dual_feas)
  end
end

"src/lm.jl:15-26 -- `Levenberg_Marquardt(model, facto, perm, normalize, linesearch; kwargs...)`"
function Levenberg_Marquardt(model :: AbstractNLSModel, facto :: Symbol, perm :: Symbol, normalize :: Symbol,
                             linesearch :: Bool;
                             x :: AbstractVector = copy(model.meta.x0), facto_type :: DataType = eltype(x),
                             restol = nothing, satol = nothing, srtol = nothing, oatol = nothing, ortol = nothing,
                             atol = nothing, rtol = nothing, νd = nothing, νm = nothing, λ = nothing, δd = nothing,
                             ite_max :: Int = 200, max_time :: Int = 3600, pcg_tol :: Real = -1.0, pcg_max_iter :: Int = -1,
                             loss :: Symbol = :linear, f_scale = 1.0, fixed_cameras = nothing, fixed_points = nothing,
                             fixed_camera_params = nothing, point_priors = nothing, camera_priors = nothing,
                             centre_priors = nothing, obs_info = nothing)
  return _ba_lm(model, 1, facto, perm, normalize, linesearch, x, facto_type, restol, satol, srtol, oatol, ortol, atol, rtol,
                νd, νm, λ, δd, ite_max, max_time, pcg_tol, pcg_max_iter, loss, f_scale, fixed_cameras, fixed_points,
                fixed_camera_params, point_priors, camera_priors, centre_priors, obs_info)
end

"src/LevenbergMarquardt.jl:16-26 -- the 4-argument method src/solve_ba.jl:26 calls (no linesearch, no facto_type)"
function Levenberg_Marquardt(model :: AbstractNLSModel, facto :: Symbol, perm :: Symbol, normalize :: Symbol;
                             x :: AbstractVector = copy(model.meta.x0),
                             restol = nothing, satol = nothing, srtol = nothing, oatol = nothing, ortol = nothing,
                             atol = nothing, rtol = nothing, νd = nothing, νm = nothing, λ = nothing, δd = nothing,
                             ite_max :: Int = 100, loss :: Symbol = :linear, f_scale = 1.0, fixed_cameras = nothing,
                             fixed_points = nothing, fixed_camera_params = nothing, point_priors = nothing,
                             camera_priors = nothing, centre_priors = nothing, obs_info = nothing)
  return _ba_lm(model, 0, facto, perm, normalize, false, x, eltype(x), restol, satol, srtol, oatol, ortol, atol, rtol,
                νd, νm, λ, δd, ite_max, 3600, -1.0, -1, loss, f_scale, fixed_cameras, fixed_points, fixed_camera_params,
                point_priors, camera_priors, centre_priors, obs_info)
end

"""
    covariance(nlp, x; λ = 0.0, loss = :linear, f_scale = 1.0, fixed_cameras = nothing, fixed_points = nothing,
               fixed_camera_params = nothing, rank_tol = nothing, point_priors = nothing, camera_priors = nothing,
               centre_priors = nothing, obs_info = nothing)

Covariance at `x` (an extension; include/ba_hip.h, ba_covariance): the diagonal blocks of (J̃_F'J̃_F + Σ H_k'Λ_k H_k + λI)⁻¹ under
the loss, the fixed parameters, the priors and the observations' information given (keywords as Levenberg_Marquardt's).  Returns `(cam_cov, pnt_cov, min_rel_pivot)`:
cam_cov[:, :, c] the 9 × 9 block of camera c (block order r1 r2 r3 t1 t2 t3 k1 k2 f), pnt_cov[:, :, i] the 3 × 3 block of
point i; fixed rows and columns are 0.  Not scaled by a residual variance.  With the gauge free and λ = 0 the reduced
camera system is singular: SQDException (rank_tol = nothing: the library's default, 0: no check).
"""
function covariance(nlp, x :: AbstractVector; λ :: Real = 0.0, loss :: Symbol = :linear, f_scale = 1.0,
                    fixed_cameras = nothing, fixed_points = nothing, fixed_camera_params = nothing, rank_tol = nothing,
                    point_priors = nothing, camera_priors = nothing, centre_priors = nothing, obs_info = nothing)
  (isfinite(λ) && λ >= 0) || error("λ must be finite and >= 0")
  _ba_set_loss(nlp, loss, f_scale)
  _ba_set_fixed(nlp, fixed_cameras, fixed_points, fixed_camera_params, 0)
  _ba_set_priors(nlp, point_priors, camera_priors, centre_priors, false, 0, Float64)
  _ba_set_obs_info(nlp, obs_info, false, 0, Float64)
  xv = Vector{Float64}(x)
  cam = zeros(Float64, 81 * nlp.ncams)
  pnt = zeros(Float64, 9 * nlp.npnts)
  piv = Ref{Cdouble}(0.0)
  bacheck(ccall((:ba_covariance, libba), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                                                Ref{Cdouble}),
                nlp.handle, xv, Float64(λ), rank_tol === nothing ? -1.0 : Float64(rank_tol), cam, pnt, piv))
  # the library's blocks are row-major; Julia is column-major: transpose each (they are symmetric up to rounding)
  cc = permutedims(reshape(cam, 9, 9, nlp.ncams), (2, 1, 3))
  pc = permutedims(reshape(pnt, 3, 3, nlp.npnts), (2, 1, 3))
  return cc, pc, piv[]
end
