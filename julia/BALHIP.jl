# BALHIP.jl -- shared part of the Julia shim over libba_hip.so (include/ba_hip.h): library handle, error mapping and the
# C structs.  Included by BALNLPModelsHIP.jl and LevenbergMarquardtHIP.jl, which replace src/BALNLPModels.jl and
# src/LevenbergMarquardt.jl / src/lm.jl of CelestineAngla/BundleAdjustment.jl in the `include` lines of
# src/solve_ba.jl:1-2, src/main.jl, src/benchmark.jl, src/diffprecsions.jl and src/benchmark_diffprec.jl.
#
# NOT EXECUTED in the build image (no Julia runtime there): the struct layouts below are kept equal to the C header by
# tests/test_host.py::test_julia_shim_matches_header, which reads THIS file's field lists and compares them with the
# sizeof/offsetof the C compiler reports (tests/c_abi/abi_check.c).

const libba = get(ENV, "BA_HIP_LIB", joinpath(@__DIR__, "..", "bundleadjustment.jl_amd", "libba_hip.so"))

# error codes of include/ba_hip.h
const BA_OK = 0
const BA_ERR_ZERO_PIVOT = 4

"Zero pivot in the LDLᵀ factorisation: src/ldl_aux.jl:45-47,199"
struct SQDException <: Exception
  msg :: String
end

struct BAError <: Exception
  code :: Int
  msg :: String
end

function bacheck(rc :: Integer)
  rc == BA_OK && return nothing
  msg = unsafe_string(ccall((:ba_last_error, libba), Cstring, ()))
  rc == BA_ERR_ZERO_PIVOT && throw(SQDException(msg))
  throw(BAError(rc, msg))
end

# struct ba_lm_opts (include/ba_hip.h) -- field order and types ARE the ABI
struct BaLmOpts
  variant :: Cint
  facto :: Cint
  normalize :: Cint
  linesearch :: Cint
  facto_type :: Cint
  ite_max :: Cint
  verbose :: Cint
  x_f32 :: Cint
  restol :: Cdouble
  satol :: Cdouble
  srtol :: Cdouble
  oatol :: Cdouble
  ortol :: Cdouble
  atol :: Cdouble
  rtol :: Cdouble
  nu_d :: Cdouble
  nu_m :: Cdouble
  lambda :: Cdouble
  delta_d :: Cdouble
  max_time :: Cdouble
  pcg_tol :: Cdouble
  pcg_max_iter :: Cint
  perm :: Cint
end

# struct ba_lm_stats (include/ba_hip.h)
mutable struct BaLmStats
  status :: Cint
  iter :: Cint
  n_accepted :: Cint
  n_rejected :: Cint
  n_residual :: Cint
  n_jacobian :: Cint
  n_factor :: Cint
  n_cg :: Cint
  objective :: Cdouble
  dual_feas :: Cdouble
  lambda_final :: Cdouble
  elapsed_s :: Cdouble
  loop_s :: Cdouble
  BaLmStats() = new(-1, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
end

# BA_ST_* -> the status symbols of src/lm.jl:391-405 (index = code + 1)
const BA_STATUS = (:small_step, :first_order, :small_residual, :acceptable, :neg_pred, :exception, :max_iter)

# shared camera intrinsics (an extension): include/ba_hip.h, ba_lm_set_shared_intrinsics.  `group`: nothing (clears the grouping)
# or ncams labels, 0 = the camera keeps its own (k1, k2, f), g in 1..8 = member of calibration group g.  The members of a group
# must hold identical (k1, k2, f) in the x of the next solve.  Stays on the handle until it is set again.
function set_shared_intrinsics(nlp, group)
  if group === nothing
    bacheck(ccall((:ba_lm_set_shared_intrinsics, libba), Cint, (Ptr{Cvoid}, Ptr{Int32}), nlp.handle, Ptr{Int32}(C_NULL)))
    return nothing
  end
  length(group) == nlp.ncams || error("shared intrinsics: one label per camera ($(nlp.ncams)), got $(length(group))")
  lab = collect(Int32, group)
  GC.@preserve lab begin
    bacheck(ccall((:ba_lm_set_shared_intrinsics, libba), Cint, (Ptr{Cvoid}, Ptr{Int32}), nlp.handle, pointer(lab)))
  end
  return nothing
end

"(groups, members) of the grouping the handle holds (ba_lm_get_shared_intrinsics)"
function shared_intrinsics_counts(nlp)
  g, m = Ref{Cint}(0), Ref{Int64}(0)
  bacheck(ccall((:ba_lm_get_shared_intrinsics, libba), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}), nlp.handle, g, m))
  return Int(g[]), m[]
end

# per-observation information matrices (an extension): include/ba_hip.h, ba_lm_set_obs_info.  `info3`: nothing (clears the array)
# or a 3 x nobs Float64 matrix, column i = (xx, xy, yy) of the symmetric positive semi-definite Lambda_i of observation i, in the
# model's observation order.  Stays on the handle until it is set again; Levenberg_Marquardt and covariance set it from their
# `obs_info` keyword at every call (julia/LevenbergMarquardtHIP.jl).
function set_obs_info(nlp, info3)
  if info3 === nothing
    bacheck(ccall((:ba_lm_set_obs_info, libba), Cint, (Ptr{Cvoid}, Ptr{Float64}), nlp.handle, Ptr{Float64}(C_NULL)))
    return nothing
  end
  size(info3) == (3, nlp.nobs) || error("obs_info: a 3 x nobs ($(nlp.nobs)) matrix of (xx, xy, yy) columns, got $(size(info3))")
  a = Matrix{Float64}(info3)
  GC.@preserve a begin
    bacheck(ccall((:ba_lm_set_obs_info, libba), Cint, (Ptr{Cvoid}, Ptr{Float64}), nlp.handle, pointer(a)))
  end
  return nothing
end

# points with the cameras held (an extension): include/ba_hip.h, ba_refine_points.  Refines the points of `x` in place under the
# loss, information, point priors and fixed points the handle holds (set them with the setters above, or by an earlier
# Levenberg_Marquardt call); `triangulate = true` starts every point from the linear triangulation of its rays.  Returns
# (status :: Vector{UInt8} (BA_PT_* | 0x80 when behind a camera), cost :: 2 x npnts (before, after), counts :: Vector{Int64}
# (the six states, then the points flagged behind), iters_max).
function refine_points!(nlp, x :: Vector{Float64}; triangulate :: Bool = false, max_iter :: Integer = -1, xtol :: Real = -1.0,
                        lam0 :: Real = -1.0)
  status = zeros(UInt8, nlp.npnts)
  cost = zeros(Float64, 2, nlp.npnts)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  GC.@preserve x status cost counts begin
    bacheck(ccall((:ba_refine_points, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint}),
                  nlp.handle, pointer(x), Cint(triangulate), Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status),
                  pointer(cost), pointer(counts), iters))
  end
  return status, cost, counts, Int(iters[])
end

# cameras with the points held (an extension): include/ba_hip.h, ba_refine_cameras.  Refines the cameras of `x` in place under the
# loss, information, camera and centre priors, camera masks and grouping the handle holds (the members of a group keep their
# k1, k2, f).  Returns (status :: Vector{UInt8} (BA_PT_* | 0x80 when a point lies behind the camera), cost :: 2 x ncams (before,
# after), counts :: Vector{Int64} (the six states, then the cameras flagged behind), iters_max).
function refine_cameras!(nlp, x :: Vector{Float64}; max_iter :: Integer = -1, xtol :: Real = -1.0, lam0 :: Real = -1.0)
  status = zeros(UInt8, nlp.ncams)
  cost = zeros(Float64, 2, nlp.ncams)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  GC.@preserve x status cost counts begin
    bacheck(ccall((:ba_refine_cameras, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint}),
                  nlp.handle, pointer(x), Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters))
  end
  return status, cost, counts, Int(iters[])
end

# linear camera resection as the start of refine_cameras! (an extension): include/ba_hip.h, ba_resect_cameras.  Every camera
# whose pose is free starts from the closed-form pose of its 2D-3D correspondences (the pose entries of `x` are not read, NaN
# included; fewer than 6 observations or a degenerate configuration: BA_PT_DEGENERATE, untouched); a camera with a held pose
# component starts from `x` as in refine_cameras!.  `max_iter = 0` returns the resected poses.  Same return values.
function resect_cameras!(nlp, x :: Vector{Float64}; max_iter :: Integer = -1, xtol :: Real = -1.0, lam0 :: Real = -1.0)
  status = zeros(UInt8, nlp.ncams)
  cost = zeros(Float64, 2, nlp.ncams)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  GC.@preserve x status cost counts begin
    bacheck(ccall((:ba_resect_cameras, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint}),
                  nlp.handle, pointer(x), Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters))
  end
  return status, cost, counts, Int(iters[])
end

# the device-resident form: d_x, d_status (or C_NULL) and d_cost (or C_NULL) are device pointers (ba_dev_malloc); enqueued on
# `stream` (C_NULL: the handle's) and not synchronised -- counts and iters_max are not fetched
function resect_cameras_dev!(nlp, d_x :: Ptr{Cvoid}; max_iter :: Integer = -1, xtol :: Real = -1.0, lam0 :: Real = -1.0,
                             d_status :: Ptr{Cvoid} = C_NULL, d_cost :: Ptr{Cvoid} = C_NULL, stream :: Ptr{Cvoid} = C_NULL)
  bacheck(ccall((:ba_resect_cameras_dev, libba), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}, Ptr{Cvoid}),
                nlp.handle, d_x, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), d_status, d_cost, Ptr{Int64}(C_NULL),
                Ptr{Cint}(C_NULL), stream))
  return nothing
end

# outlier-robust camera resection (an extension): include/ba_hip.h, ba_ransac_cameras.  resect_cameras! with a consensus stage in
# front: `hypotheses` minimal samples of `sample` correspondences per camera are resected and scored by their inliers
# (reprojection within `threshold` pixels, in front of the camera); the best one defines the inlier set, up to `refits` linear
# refits re-score it, and the resection and the refinement run on that set only.  A value below its range means the default
# (128, 6, 2, max(sample, 6)).  Returns what resect_cameras! returns, then the inlier mask (nobs, caller's observation order),
# the size of every camera's set and its winning hypothesis (-1: not attempted or none valid).
struct BaRansacOpts
  threshold :: Cdouble
  hypotheses :: Cint
  sample :: Cint
  refits :: Cint
  min_inliers :: Cint
  seed :: UInt64
end

function ransac_cameras!(nlp, x :: Vector{Float64}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                         refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                         xtol :: Real = -1.0, lam0 :: Real = -1.0)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  status = zeros(UInt8, nlp.ncams)
  cost = zeros(Float64, 2, nlp.ncams)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  inlier = zeros(UInt8, nlp.nobs)
  n_inliers = zeros(Int32, nlp.ncams)
  best_hyp = zeros(Int32, nlp.ncams)
  GC.@preserve x status cost counts inlier n_inliers best_hyp begin
    bacheck(ccall((:ba_ransac_cameras, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}),
                  nlp.handle, pointer(x), opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters, pointer(inlier), pointer(n_inliers), pointer(best_hyp)))
  end
  return status, cost, counts, Int(iters[]), inlier .!= 0, n_inliers, best_hyp
end

# the device-resident form: d_x and the outputs (each may be C_NULL) are device pointers (ba_dev_malloc); enqueued on `stream`
# (C_NULL: the handle's) and not synchronised -- counts and iters_max are not fetched
function ransac_cameras_dev!(nlp, d_x :: Ptr{Cvoid}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                             refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                             xtol :: Real = -1.0, lam0 :: Real = -1.0, d_status :: Ptr{Cvoid} = C_NULL, d_cost :: Ptr{Cvoid} = C_NULL,
                             d_inlier :: Ptr{Cvoid} = C_NULL, d_n_inliers :: Ptr{Cvoid} = C_NULL, d_best_hyp :: Ptr{Cvoid} = C_NULL,
                             stream :: Ptr{Cvoid} = C_NULL)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  bacheck(ccall((:ba_ransac_cameras_dev, libba), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                nlp.handle, d_x, opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), d_status, d_cost, Ptr{Int64}(C_NULL),
                Ptr{Cint}(C_NULL), d_inlier, d_n_inliers, d_best_hyp, stream))
  return nothing
end

# camera resection with unknown focal length (an extension): include/ba_hip.h, ba_resect_cameras_focal / ba_ransac_cameras_focal.
# resect_cameras! and ransac_cameras! for images without calibration: every camera whose pose and f are both free gets f from
# the linear stage (and from every hypothesis) along with its pose -- its (r, t, f) and free k1, k2 in `x` are not read, NaN
# included; f is written into `x`, a free k1 / k2 as 0 before the refinement.  A camera with f held or in a group is resected with
# the intrinsics of `x`.  Arguments and return values are those of the siblings.
function resect_cameras_focal!(nlp, x :: Vector{Float64}; max_iter :: Integer = -1, xtol :: Real = -1.0, lam0 :: Real = -1.0)
  status = zeros(UInt8, nlp.ncams)
  cost = zeros(Float64, 2, nlp.ncams)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  GC.@preserve x status cost counts begin
    bacheck(ccall((:ba_resect_cameras_focal, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint}),
                  nlp.handle, pointer(x), Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters))
  end
  return status, cost, counts, Int(iters[])
end

function resect_cameras_focal_dev!(nlp, d_x :: Ptr{Cvoid}; max_iter :: Integer = -1, xtol :: Real = -1.0, lam0 :: Real = -1.0,
                                   d_status :: Ptr{Cvoid} = C_NULL, d_cost :: Ptr{Cvoid} = C_NULL, stream :: Ptr{Cvoid} = C_NULL)
  bacheck(ccall((:ba_resect_cameras_focal_dev, libba), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}, Ptr{Cvoid}),
                nlp.handle, d_x, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), d_status, d_cost, Ptr{Int64}(C_NULL),
                Ptr{Cint}(C_NULL), stream))
  return nothing
end

function ransac_cameras_focal!(nlp, x :: Vector{Float64}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                               refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                               xtol :: Real = -1.0, lam0 :: Real = -1.0)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  status = zeros(UInt8, nlp.ncams)
  cost = zeros(Float64, 2, nlp.ncams)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  inlier = zeros(UInt8, nlp.nobs)
  n_inliers = zeros(Int32, nlp.ncams)
  best_hyp = zeros(Int32, nlp.ncams)
  GC.@preserve x status cost counts inlier n_inliers best_hyp begin
    bacheck(ccall((:ba_ransac_cameras_focal, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}),
                  nlp.handle, pointer(x), opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters, pointer(inlier), pointer(n_inliers), pointer(best_hyp)))
  end
  return status, cost, counts, Int(iters[]), inlier .!= 0, n_inliers, best_hyp
end

function ransac_cameras_focal_dev!(nlp, d_x :: Ptr{Cvoid}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                                   refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                                   xtol :: Real = -1.0, lam0 :: Real = -1.0, d_status :: Ptr{Cvoid} = C_NULL,
                                   d_cost :: Ptr{Cvoid} = C_NULL, d_inlier :: Ptr{Cvoid} = C_NULL, d_n_inliers :: Ptr{Cvoid} = C_NULL,
                                   d_best_hyp :: Ptr{Cvoid} = C_NULL, stream :: Ptr{Cvoid} = C_NULL)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  bacheck(ccall((:ba_ransac_cameras_focal_dev, libba), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                nlp.handle, d_x, opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), d_status, d_cost, Ptr{Int64}(C_NULL),
                Ptr{Cint}(C_NULL), d_inlier, d_n_inliers, d_best_hyp, stream))
  return nothing
end

# relative pose of camera pairs (an extension): include/ba_hip.h, ba_pair_matches / ba_relative_pose.  pair_matches lists the
# points two cameras both observe (host only): pairs_a, pairs_b are 1-based cameras; returns match_ptr (npairs + 1 offsets) and the
# 1-based observations of every match in camera a and in camera b.  relative_pose gives P_b = R(r) P_a + t, |t| = 1, per pair by
# the eight-point algorithm; with a threshold (pixels) a consensus stage stands in front (a value below its range means the
# default: 128 hypotheses, samples of 8, 2 refits, min_inliers = max(sample, 8)).  Of `x` only (k1, k2, f) of the pairs' cameras
# are read.  Returns pose (6 x npairs: r, then t; NaN where the state is not 0), status (BA_RP_*), match_ptr, the inlier mask per
# match, the size of every pair's set, its winning hypothesis (-1: none) and the pairs per state.
function pair_matches(nlp, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64})
  npairs = length(pairs_a)
  cam = Vector{Int64}(nlp.cams_indices)
  pnt = Vector{Int64}(nlp.pnts_indices)
  match_ptr = zeros(Int64, npairs + 1)
  sig = (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64})
  GC.@preserve cam pnt pairs_a pairs_b match_ptr begin
    bacheck(ccall((:ba_pair_matches, libba), Cint, sig, nlp.ncams, nlp.npnts, nlp.nobs, pointer(cam), pointer(pnt), npairs,
                  pointer(pairs_a), pointer(pairs_b), pointer(match_ptr), Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL)))
  end
  obs_a = zeros(Int64, match_ptr[end])
  obs_b = zeros(Int64, match_ptr[end])
  GC.@preserve cam pnt pairs_a pairs_b match_ptr obs_a obs_b begin
    bacheck(ccall((:ba_pair_matches, libba), Cint, sig, nlp.ncams, nlp.npnts, nlp.nobs, pointer(cam), pointer(pnt), npairs,
                  pointer(pairs_a), pointer(pairs_b), pointer(match_ptr), pointer(obs_a), pointer(obs_b)))
  end
  return match_ptr, obs_a, obs_b
end

function relative_pose(nlp, x :: Vector{Float64}, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64};
                       threshold :: Union{Real, Nothing} = nothing, hypotheses :: Integer = 0, sample :: Integer = 0,
                       refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0)
  npairs = length(pairs_a)
  match_ptr, _, _ = pair_matches(nlp, pairs_a, pairs_b)
  pose = fill(NaN, 6, npairs)
  status = zeros(UInt8, npairs)
  inlier = zeros(UInt8, match_ptr[end])
  n_inliers = zeros(Int32, npairs)
  best_hyp = zeros(Int32, npairs)
  counts = zeros(Int64, 4)
  opts = Ref(BaRansacOpts(Cdouble(threshold === nothing ? 1.0 : threshold), Cint(hypotheses), Cint(sample), Cint(refits),
                          Cint(min_inliers), UInt64(seed)))
  GC.@preserve x pairs_a pairs_b opts pose status match_ptr inlier n_inliers best_hyp counts begin
    optr = threshold === nothing ? Ptr{BaRansacOpts}(C_NULL) : Base.unsafe_convert(Ptr{BaRansacOpts}, opts)
    bacheck(ccall((:ba_relative_pose, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{BaRansacOpts}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int64},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                  nlp.handle, pointer(x), npairs, pointer(pairs_a), pointer(pairs_b), optr, pointer(pose), pointer(status),
                  pointer(match_ptr), pointer(inlier), pointer(n_inliers), pointer(best_hyp), pointer(counts)))
  end
  return pose, status, match_ptr, inlier .!= 0, n_inliers, best_hyp, counts
end

# The same with the five-point minimal solver as the hypothesis generator (ba_relative_pose_five_point): every real essential
# matrix through five sampled matches is a candidate; the winner, the refits and the final eight-point fit on the consensus set
# are those of relative_pose, and so is what is returned.  The threshold is required; the sample is 5, min_inliers at least 8.
function relative_pose_five_point(nlp, x :: Vector{Float64}, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64};
                                  threshold :: Real, hypotheses :: Integer = 0, refits :: Integer = -1,
                                  min_inliers :: Integer = 0, seed :: Integer = 0)
  npairs = length(pairs_a)
  match_ptr, _, _ = pair_matches(nlp, pairs_a, pairs_b)
  pose = fill(NaN, 6, npairs)
  status = zeros(UInt8, npairs)
  inlier = zeros(UInt8, match_ptr[end])
  n_inliers = zeros(Int32, npairs)
  best_hyp = zeros(Int32, npairs)
  counts = zeros(Int64, 4)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(5), Cint(refits), Cint(min_inliers), UInt64(seed)))
  GC.@preserve x pairs_a pairs_b opts pose status match_ptr inlier n_inliers best_hyp counts begin
    bacheck(ccall((:ba_relative_pose_five_point, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{BaRansacOpts}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int64},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                  nlp.handle, pointer(x), npairs, pointer(pairs_a), pointer(pairs_b), Base.unsafe_convert(Ptr{BaRansacOpts}, opts),
                  pointer(pose), pointer(status), pointer(match_ptr), pointer(inlier), pointer(n_inliers), pointer(best_hyp),
                  pointer(counts)))
  end
  return pose, status, match_ptr, inlier .!= 0, n_inliers, best_hyp, counts
end

# The solver alone (ba_five_point): qa, qb are 2 x 5 x n, undistorted image points already divided by f (the ray is (q, -1)).
# Returns E (3 x 3 x 10 x n in C's row-major order: E[j, i, s, k] is entry (i, j) of solution s of problem k; |E|_F = 1, NaN in
# the unused slots) and the number of real solutions of every problem.
function five_point(nlp, qa :: Array{Float64, 3}, qb :: Array{Float64, 3})
  size(qa) == size(qb) && size(qa, 1) == 2 && size(qa, 2) == 5 || error("five_point: qa and qb must both be 2 x 5 x n")
  n = size(qa, 3)
  E = fill(NaN, 3, 3, 10, n)
  n_sol = zeros(Int32, n)
  GC.@preserve qa qb E n_sol begin
    bacheck(ccall((:ba_five_point, libba), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                  nlp.handle, n, pointer(qa), pointer(qb), pointer(E), pointer(n_sol)))
  end
  return E, n_sol
end

# Homography of camera pairs (an extension): include/ba_hip.h, ba_homography / ba_decompose_homography / ba_homography_pose.
# homography is relative_pose with the second two-view model, d_b ~ H d_a, for matches on one plane and pairs without a
# baseline: with a threshold (pixels) the consensus stage stands in front (samples of 4..16, default 4; min_inliers at least 4,
# default 8).  Returns H (3 x 3 x npairs in C's row-major order: H[j, i, k] is entry (i, j) of pair k; sigma_2 = 1; NaN where the
# state is not 0), status (BA_HG_*), match_ptr, the inlier mask per match, the size of every pair's set, its winning hypothesis
# and the pairs per state.
function homography(nlp, x :: Vector{Float64}, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64};
                    threshold :: Union{Real, Nothing} = nothing, hypotheses :: Integer = 0, sample :: Integer = 0,
                    refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0)
  npairs = length(pairs_a)
  match_ptr, _, _ = pair_matches(nlp, pairs_a, pairs_b)
  H = fill(NaN, 3, 3, npairs)
  status = zeros(UInt8, npairs)
  inlier = zeros(UInt8, match_ptr[end])
  n_inliers = zeros(Int32, npairs)
  best_hyp = zeros(Int32, npairs)
  counts = zeros(Int64, 4)
  opts = Ref(BaRansacOpts(Cdouble(threshold === nothing ? 1.0 : threshold), Cint(hypotheses), Cint(sample), Cint(refits),
                          Cint(min_inliers), UInt64(seed)))
  GC.@preserve x pairs_a pairs_b opts H status match_ptr inlier n_inliers best_hyp counts begin
    optr = threshold === nothing ? Ptr{BaRansacOpts}(C_NULL) : Base.unsafe_convert(Ptr{BaRansacOpts}, opts)
    bacheck(ccall((:ba_homography, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{BaRansacOpts}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int64},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                  nlp.handle, pointer(x), npairs, pointer(pairs_a), pointer(pairs_b), optr, pointer(H), pointer(status),
                  pointer(match_ptr), pointer(inlier), pointer(n_inliers), pointer(best_hyp), pointer(counts)))
  end
  return H, status, match_ptr, inlier .!= 0, n_inliers, best_hyp, counts
end

# The decomposition alone (ba_decompose_homography): H is 3 x 3 x n in C's row-major order, its sign as given.  Returns R
# (3 x 3 x 4 x n, row-major like H), t (3 x 4 x n, in units of the plane distance), the normals (3 x 4 x n), NaN in the unused
# slots, the number of solutions of every problem (0, 1: a rotation, or 4) and the parallax |t| / d.
function decompose_homography(nlp, H :: Array{Float64, 3})
  size(H, 1) == 3 && size(H, 2) == 3 || error("decompose_homography: H must be 3 x 3 x n")
  n = size(H, 3)
  R = fill(NaN, 3, 3, 4, n)
  t = fill(NaN, 3, 4, n)
  normal = fill(NaN, 3, 4, n)
  n_sol = zeros(Int32, n)
  parallax = fill(NaN, n)
  GC.@preserve H R t normal n_sol parallax begin
    bacheck(ccall((:ba_decompose_homography, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                  nlp.handle, n, pointer(H), pointer(R), pointer(t), pointer(normal), pointer(n_sol), pointer(parallax)))
  end
  return R, t, normal, n_sol, parallax
end

# The pose of planar pairs (ba_homography_pose) from what homography returned (H, status, the inlier mask): per pair the
# parallax, the number of candidates (0..2), their poses (6 x 2 x npairs: r, then the unit t), their normals (3 x 2 x npairs) and
# their supports (2 x npairs: the inliers of relative_pose's test over the pair's whole list; -1 in the unused slots).  A pair
# without a baseline has one candidate with its r and NaN for t.
function homography_pose(nlp, x :: Vector{Float64}, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64}, H :: Array{Float64, 3},
                         status :: Vector{UInt8}, inlier :: AbstractVector{Bool}; threshold :: Real)
  npairs = length(pairs_a)
  size(H) == (3, 3, npairs) && length(status) == npairs || error("homography_pose: H must be 3 x 3 x npairs and status npairs")
  bytes = Vector{UInt8}(inlier)
  parallax = fill(NaN, npairs)
  n_pose = zeros(Int32, npairs)
  pose = fill(NaN, 6, 2, npairs)
  normal = fill(NaN, 3, 2, npairs)
  support = fill(Int32(-1), 2, npairs)
  GC.@preserve x pairs_a pairs_b H status bytes parallax n_pose pose normal support begin
    bacheck(ccall((:ba_homography_pose, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}, Ptr{UInt8}, Cdouble, Ptr{Float64},
                   Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                  nlp.handle, pointer(x), npairs, pointer(pairs_a), pointer(pairs_b), pointer(H), pointer(status), pointer(bytes),
                  Cdouble(threshold), pointer(parallax), pointer(n_pose), pointer(pose), pointer(normal), pointer(support)))
  end
  return parallax, n_pose, pose, normal, support
end

# P3P minimal samples for the consensus stage of the camera resection (an extension): include/ba_hip.h, ba_ransac_cameras_p3p.
# ransac_cameras! with three correspondences per hypothesis instead of six, solved exactly: every real P3P pose (up to four) is
# scored and the best is the hypothesis.  `sample` must be 3 (or below its range: the default 3), min_inliers is still at least
# 6; the intrinsics of `x` are read.  Arguments and return values are those of ransac_cameras!.
function ransac_cameras_p3p!(nlp, x :: Vector{Float64}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                             refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                             xtol :: Real = -1.0, lam0 :: Real = -1.0)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  status = zeros(UInt8, nlp.ncams)
  cost = zeros(Float64, 2, nlp.ncams)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  inlier = zeros(UInt8, nlp.nobs)
  n_inliers = zeros(Int32, nlp.ncams)
  best_hyp = zeros(Int32, nlp.ncams)
  GC.@preserve x status cost counts inlier n_inliers best_hyp begin
    bacheck(ccall((:ba_ransac_cameras_p3p, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}),
                  nlp.handle, pointer(x), opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters, pointer(inlier), pointer(n_inliers), pointer(best_hyp)))
  end
  return status, cost, counts, Int(iters[]), inlier .!= 0, n_inliers, best_hyp
end

function ransac_cameras_p3p_dev!(nlp, d_x :: Ptr{Cvoid}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                                 refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                                 xtol :: Real = -1.0, lam0 :: Real = -1.0, d_status :: Ptr{Cvoid} = C_NULL,
                                 d_cost :: Ptr{Cvoid} = C_NULL, d_inlier :: Ptr{Cvoid} = C_NULL, d_n_inliers :: Ptr{Cvoid} = C_NULL,
                                 d_best_hyp :: Ptr{Cvoid} = C_NULL, stream :: Ptr{Cvoid} = C_NULL)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  bacheck(ccall((:ba_ransac_cameras_p3p_dev, libba), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                nlp.handle, d_x, opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), d_status, d_cost, Ptr{Int64}(C_NULL),
                Ptr{Cint}(C_NULL), d_inlier, d_n_inliers, d_best_hyp, stream))
  return nothing
end

# Outlier-robust triangulation (an extension): include/ba_hip.h, ba_ransac_points.  refine_points with init = 1 and a consensus
# stage in front: every pair of a point's observations (`hypotheses` random pairs where it has more) is triangulated and scored
# by its inliers, the best pair defines the point's set, and the triangulation and the refinement run on the set only.  `sample`
# must be 2 (or below its range: the default 2), min_inliers at least 2 (the default).  The points of `x` are not read; they are
# replaced.  Returns the status, cost, counts and trials of refine_points, then the inlier mask (nobs), the size of every point's
# set and its winning hypothesis (-1: not attempted or none valid).
function ransac_points!(nlp, x :: Vector{Float64}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                        refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                        xtol :: Real = -1.0, lam0 :: Real = -1.0)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  status = zeros(UInt8, nlp.npnts)
  cost = zeros(Float64, 2, nlp.npnts)
  counts = zeros(Int64, 7)
  iters = Ref{Cint}(0)
  inlier = zeros(UInt8, nlp.nobs)
  n_inliers = zeros(Int32, nlp.npnts)
  best_hyp = zeros(Int32, nlp.npnts)
  GC.@preserve x status cost counts inlier n_inliers best_hyp begin
    bacheck(ccall((:ba_ransac_points, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ref{Cint},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}),
                  nlp.handle, pointer(x), opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), pointer(status), pointer(cost),
                  pointer(counts), iters, pointer(inlier), pointer(n_inliers), pointer(best_hyp)))
  end
  return status, cost, counts, Int(iters[]), inlier .!= 0, n_inliers, best_hyp
end

function ransac_points_dev!(nlp, d_x :: Ptr{Cvoid}; threshold :: Real, hypotheses :: Integer = 0, sample :: Integer = 0,
                            refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, max_iter :: Integer = -1,
                            xtol :: Real = -1.0, lam0 :: Real = -1.0, d_status :: Ptr{Cvoid} = C_NULL,
                            d_cost :: Ptr{Cvoid} = C_NULL, d_inlier :: Ptr{Cvoid} = C_NULL, d_n_inliers :: Ptr{Cvoid} = C_NULL,
                            d_best_hyp :: Ptr{Cvoid} = C_NULL, stream :: Ptr{Cvoid} = C_NULL)
  opts = Ref(BaRansacOpts(Cdouble(threshold), Cint(hypotheses), Cint(sample), Cint(refits), Cint(min_inliers), UInt64(seed)))
  bacheck(ccall((:ba_ransac_points_dev, libba), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ref{BaRansacOpts}, Cint, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                nlp.handle, d_x, opts, Cint(max_iter), Cdouble(xtol), Cdouble(lam0), d_status, d_cost, Ptr{Int64}(C_NULL),
                Ptr{Cint}(C_NULL), d_inlier, d_n_inliers, d_best_hyp, stream))
  return nothing
end

# The solver alone (ba_p3p): q is 2 x 3 x n, undistorted image points already divided by f (the ray is (q, -1)); X is 3 x 3 x n,
# X[:, i, k] the world point of correspondence i of problem k.  Returns pose (6 x 4 x n: pose[:, s, k] is (r, t) of solution s of
# problem k, in ascending order of the quartic's root, NaN in the unused slots) and the number of solutions of every problem.
function p3p(nlp, q :: Array{Float64, 3}, X :: Array{Float64, 3})
  size(q, 1) == 2 && size(q, 2) == 3 && size(X) == (3, 3, size(q, 3)) || error("p3p: q must be 2 x 3 x n and X 3 x 3 x n")
  n = size(q, 3)
  pose = fill(NaN, 6, 4, n)
  n_sol = zeros(Int32, n)
  GC.@preserve q X pose n_sol begin
    bacheck(ccall((:ba_p3p, libba), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                  nlp.handle, n, pointer(q), pointer(X), pointer(pose), pointer(n_sol)))
  end
  return pose, n_sol
end

# struct ba_pair_refine_opts (include/ba_hip.h)
struct BaPairRefineOpts
  max_iter :: Cint
  xtol :: Cdouble
  lambda0 :: Cdouble
  loss :: Cint
  f_scale :: Cdouble
  threshold :: Cdouble
  rounds :: Cint
end

# The non-linear refinement of the relative pose on its consensus set (ba_refine_relative_pose): per pair a Marquardt iteration
# on the robustified Sampson error over the five degrees of freedom of (R, unit t), then the pair's list re-scored under the
# result; `rounds` further rounds adopt the re-scored set by the rule of the refits.  pose (6 x npairs), status and inlier are
# what relative_pose / relative_pose_five_point returned for the same pairs; loss is a BA_LOSS_* value.  A value below its
# range means the default (50, 1e-10, 1e-4, 2).  Returns the refined pose, the state of every pair (BA_RR_*), the set the last
# refinement ran on, the cost before and after (2 x npairs), the sizes of the sets, the matches consistent with the returned
# pose, the trials and the pairs per state.
function refine_relative_pose(nlp, x :: Vector{Float64}, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64},
                              pose :: Matrix{Float64}, status :: Vector{UInt8}, inlier :: AbstractVector{Bool};
                              threshold :: Real, max_iter :: Integer = -1, xtol :: Real = -1.0, lam0 :: Real = -1.0,
                              loss :: Integer = 0, f_scale :: Real = 1.0, rounds :: Integer = -1)
  npairs = length(pairs_a)
  size(pose) == (6, npairs) && length(status) == npairs || error("refine_relative_pose: pose must be 6 x npairs, status npairs")
  pose = copy(pose)
  bytes = Vector{UInt8}(inlier)
  state = zeros(UInt8, npairs)
  cost = zeros(Float64, 2, npairs)
  n_inliers = zeros(Int32, npairs)
  n_consistent = zeros(Int32, npairs)
  iters = zeros(Int32, npairs)
  counts = zeros(Int64, 5)
  opts = Ref(BaPairRefineOpts(Cint(max_iter), Cdouble(xtol), Cdouble(lam0), Cint(loss), Cdouble(f_scale), Cdouble(threshold), Cint(rounds)))
  GC.@preserve x pairs_a pairs_b opts pose status bytes state cost n_inliers n_consistent iters counts begin
    bacheck(ccall((:ba_refine_relative_pose, libba), Cint,
                  (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{BaPairRefineOpts}, Ptr{Float64}, Ptr{UInt8}, Ptr{UInt8},
                   Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                  nlp.handle, pointer(x), npairs, pointer(pairs_a), pointer(pairs_b), Base.unsafe_convert(Ptr{BaPairRefineOpts}, opts),
                  pointer(pose), pointer(status), pointer(bytes), pointer(state), pointer(cost), pointer(n_inliers),
                  pointer(n_consistent), pointer(iters), pointer(counts)))
  end
  return pose, state, bytes .!= 0, cost, n_inliers, n_consistent, iters, counts
end

# ---- rotation averaging over the view graph (an extension): include/ba_hip.h, "rotation averaging" ----------------------------
# Pair k is (pairs_a[k], pairs_b[k]), 1-based cameras; r (3 x npairs) is the rotation vector of R_k with R_b = R_k R_a, the r of
# relative_pose.  All angles are radians.  A pair of cameras listed twice, in either orientation, is refused.

# struct ba_rotavg_opts (include/ba_hip.h)
struct BaRotavgOpts
  loss :: Cint
  max_sweeps :: Cint
  loops :: Cint
  min_support :: Cint
  f_scale :: Cdouble
  damping :: Cdouble
  xtol :: Cdouble
  loop_threshold :: Cdouble
end

_used_bytes(used, npairs) = used === nothing ? UInt8[] : (length(used) == npairs ? Vector{UInt8}(used) : error("used must hold one entry per pair"))
_or_null(v, T) = isempty(v) ? Ptr{T}(C_NULL) : pointer(v)

# The loop consistency of the pairs (ba_rotation_loops): per pair the triangles through it among the used pairs and those
# whose rotation around the triangle is within `threshold` of the identity.  used: nothing ("r is finite") or one Bool per pair.
function rotation_loops(nlp, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64}, r :: Matrix{Float64}; threshold :: Real, used = nothing)
  npairs = length(pairs_a)
  length(pairs_b) == npairs && size(r) == (3, npairs) || error("rotation_loops: pairs_a, pairs_b of one length and r 3 x npairs")
  bytes = _used_bytes(used, npairs)
  n_loops = zeros(Int32, npairs)
  support = zeros(Int32, npairs)
  GC.@preserve pairs_a pairs_b r bytes n_loops support begin
    bacheck(ccall((:ba_rotation_loops, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}, Cdouble, Ptr{Int32}, Ptr{Int32}),
                  nlp.handle, npairs, pointer(pairs_a), pointer(pairs_b), pointer(r), _or_null(bytes, UInt8), Cdouble(threshold),
                  pointer(n_loops), pointer(support)))
  end
  return n_loops, support
end

# The maximum spanning forest of the used pairs (ba_view_graph_forest; host only) under the order support descending, weight
# descending, pair index ascending.  Returns component (0-based ids in the order of the lowest camera, -1: no used pair),
# parent_pair (0-based pair, -1: root or outside the graph), order (1-based cameras, breadth first from the roots) and roots
# (1-based).  fixed: nothing or one Bool per camera (the lowest fixed camera of a component is its root).
function view_graph_forest(ncams :: Integer, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64}; used = nothing,
                           support :: Vector{Int32} = Int32[], weights :: Vector{Float64} = Float64[], fixed = nothing)
  npairs = length(pairs_a)
  length(pairs_b) == npairs || error("view_graph_forest: pairs_a and pairs_b of one length")
  (isempty(support) || length(support) == npairs) && (isempty(weights) || length(weights) == npairs) ||
    error("view_graph_forest: support and weights hold one entry per pair")
  bytes = _used_bytes(used, npairs)
  held = fixed === nothing ? UInt8[] : (length(fixed) == ncams ? Vector{UInt8}(fixed) : error("fixed must hold one entry per camera"))
  component = zeros(Int32, ncams)
  parent_pair = zeros(Int64, ncams)
  order = zeros(Int64, ncams)
  roots = zeros(Int64, ncams)
  n_order = Ref{Int64}(0)
  n_components = Ref{Int64}(0)
  GC.@preserve pairs_a pairs_b bytes support weights held component parent_pair order roots begin
    bacheck(ccall((:ba_view_graph_forest, libba), Cint,
                  (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int64},
                   Ptr{Int64}, Ref{Int64}, Ref{Int64}, Ptr{Int64}),
                  Int64(ncams), npairs, pointer(pairs_a), pointer(pairs_b), _or_null(bytes, UInt8), _or_null(support, Int32),
                  _or_null(weights, Float64), _or_null(held, UInt8), pointer(component), pointer(parent_pair), pointer(order),
                  n_order, n_components, pointer(roots)))
  end
  return component, parent_pair, order[1:n_order[]], roots[1:n_components[]]
end

# Robust rotation averaging (ba_average_rotations): the absolute rotation of every camera from all pairs at once.  loss is a
# BA_LOSS_* value with f_scale = c in radians; loop_threshold > 0 runs the loop filter first (a pair with triangles of which
# fewer than min_support close is dropped); r0 (3 x ncams) is a start of the caller's, required with fixed (one Bool per camera,
# held at r0).  Returns r (3 x ncams, NaN for a camera without a kept pair), the state of every camera (BA_RA_*), its
# component, the kept pairs, the loop counts, the residual and the weight of every pair, the sweeps, the largest step of every
# sweep, the cost before and after, and the cameras per state.  The rotations of different components are unrelated.
function average_rotations(nlp, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64}, r :: Matrix{Float64};
                           weights :: Vector{Float64} = Float64[], used = nothing, loop_threshold :: Real = 0.0,
                           min_support :: Integer = 1, r0 :: Matrix{Float64} = zeros(3, 0), fixed = nothing, loss :: Integer = 0,
                           f_scale :: Real = 0.0, damping :: Real = 0.8, max_sweeps :: Integer = 1000, xtol :: Real = 1e-6)
  npairs = length(pairs_a)
  ncams = nlp.ncams
  length(pairs_b) == npairs && size(r) == (3, npairs) || error("average_rotations: pairs_a, pairs_b of one length and r 3 x npairs")
  isempty(weights) || length(weights) == npairs || error("average_rotations: weights hold one entry per pair")
  isempty(r0) || size(r0) == (3, ncams) || error("average_rotations: r0 must be 3 x ncams")
  1 <= max_sweeps <= 100000 || error("average_rotations: max_sweeps in 1..100000")
  bytes = _used_bytes(used, npairs)
  held = fixed === nothing ? UInt8[] : (length(fixed) == ncams ? Vector{UInt8}(fixed) : error("fixed must hold one entry per camera"))
  opts = Ref(BaRotavgOpts(Cint(loss), Cint(max_sweeps), Cint(loop_threshold > 0), Cint(min_support), Cdouble(f_scale), Cdouble(damping),
                          Cdouble(xtol), Cdouble(loop_threshold)))
  out = fill(NaN, 3, ncams)
  status = zeros(UInt8, ncams)
  component = zeros(Int32, ncams)
  kept = zeros(UInt8, npairs)
  n_loops = zeros(Int32, npairs)
  support = zeros(Int32, npairs)
  residual = fill(NaN, npairs)
  edge_weight = zeros(Float64, npairs)
  sweeps = Ref{Int32}(0)
  delta = zeros(Float64, max_sweeps)
  cost = zeros(Float64, 2)
  counts = zeros(Int64, 4)
  GC.@preserve pairs_a pairs_b r weights bytes r0 held opts out status component kept n_loops support residual edge_weight delta cost counts begin
    bacheck(ccall((:ba_average_rotations, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{UInt8},
                   Ptr{BaRotavgOpts}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                   Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                  nlp.handle, npairs, pointer(pairs_a), pointer(pairs_b), pointer(r), _or_null(weights, Float64), _or_null(bytes, UInt8),
                  _or_null(r0, Float64), _or_null(held, UInt8), Base.unsafe_convert(Ptr{BaRotavgOpts}, opts), pointer(out),
                  pointer(status), pointer(component), pointer(kept), pointer(n_loops), pointer(support), pointer(residual),
                  pointer(edge_weight), sweeps, pointer(delta), pointer(cost), pointer(counts)))
  end
  return out, status, component, kept .!= 0, n_loops, support, residual, edge_weight, Int(sweeps[]), delta[1:sweeps[]], cost, counts
end

# ---- translation averaging over the view graph (an extension): include/ba_hip.h, "translation averaging" ------------------------
# Pair k is (pairs_a[k], pairs_b[k]), 1-based cameras; dir (3 x npairs) is the direction of the baseline in the world frame, from
# the centre of a to the centre of b: -R_b' t with the unit t of relative_pose and the R_b of average_rotations.  It need not be
# normalised.  Angles are radians.  A pair of cameras listed twice, in either orientation, is refused.

# struct ba_transavg_opts (include/ba_hip.h)
struct BaTransavgOpts
  loss :: Cint
  loops :: Cint
  min_support :: Cint
  max_iterations :: Cint
  max_cg :: Cint
  f_scale :: Cdouble
  loop_threshold :: Cdouble
  min_ratio :: Cdouble
  ftol :: Cdouble
  cg_tol :: Cdouble
  lambda0 :: Cdouble
end

# The loop consistency of the directions (ba_translation_loops): per pair (a, b) the triangles (a, c, b) among the used pairs
# that can be checked and those in which the direction a -> b lies within `threshold` of the shorter arc between the directions
# a -> c and c -> b.  used: nothing ("dir is finite with a norm >= 1e-12") or one Bool per pair.
function translation_loops(nlp, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64}, dir :: Matrix{Float64}; threshold :: Real, used = nothing)
  npairs = length(pairs_a)
  length(pairs_b) == npairs && size(dir) == (3, npairs) || error("translation_loops: pairs_a, pairs_b of one length and dir 3 x npairs")
  bytes = _used_bytes(used, npairs)
  n_loops = zeros(Int32, npairs)
  support = zeros(Int32, npairs)
  GC.@preserve pairs_a pairs_b dir bytes n_loops support begin
    bacheck(ccall((:ba_translation_loops, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}, Cdouble, Ptr{Int32}, Ptr{Int32}),
                  nlp.handle, npairs, pointer(pairs_a), pointer(pairs_b), pointer(dir), _or_null(bytes, UInt8), Cdouble(threshold),
                  pointer(n_loops), pointer(support)))
  end
  return n_loops, support
end

# Robust translation averaging (ba_average_translations): the centre of every camera from the directions of all pairs at once, up
# to a shift and a scale per component.  loss is a BA_LOSS_* value with f_scale = c in units of the chord; loop_threshold > 0 runs
# the loop filter first (a pair with checked triangles of which fewer than min_support, or fewer than min_ratio of them, close is
# dropped); c0 (3 x ncams) is a start of the caller's, required with fixed (one Bool per camera, held at c0).  Returns c (3 x
# ncams, NaN for a camera without a kept pair), the state of every camera (BA_TA_*), its component, the kept pairs, the loop
# counts, the residual and the weight of every pair, the iterations, the conjugate-gradient iterations, the trace (4 x
# iterations: cost of the trial, lambda, conjugate-gradient iterations, accepted), the cost before and after, and the cameras
# per state.  The centres of different components are unrelated.
function average_translations(nlp, pairs_a :: Vector{Int64}, pairs_b :: Vector{Int64}, dir :: Matrix{Float64};
                              weights :: Vector{Float64} = Float64[], used = nothing, loop_threshold :: Real = 0.0,
                              min_support :: Integer = 1, min_ratio :: Real = 0.34, c0 :: Matrix{Float64} = zeros(3, 0), fixed = nothing,
                              loss :: Integer = 0, f_scale :: Real = 0.0, max_iterations :: Integer = 50, ftol :: Real = 1e-10,
                              cg_tol :: Real = 1e-6, max_cg :: Integer = 500, lambda0 :: Real = 1e-3)
  npairs = length(pairs_a)
  ncams = nlp.ncams
  length(pairs_b) == npairs && size(dir) == (3, npairs) || error("average_translations: pairs_a, pairs_b of one length and dir 3 x npairs")
  isempty(weights) || length(weights) == npairs || error("average_translations: weights hold one entry per pair")
  isempty(c0) || size(c0) == (3, ncams) || error("average_translations: c0 must be 3 x ncams")
  1 <= max_iterations <= 100000 && 1 <= max_cg <= 100000 || error("average_translations: max_iterations and max_cg in 1..100000")
  bytes = _used_bytes(used, npairs)
  held = fixed === nothing ? UInt8[] : (length(fixed) == ncams ? Vector{UInt8}(fixed) : error("fixed must hold one entry per camera"))
  opts = Ref(BaTransavgOpts(Cint(loss), Cint(loop_threshold > 0), Cint(min_support), Cint(max_iterations), Cint(max_cg), Cdouble(f_scale),
                            Cdouble(loop_threshold), Cdouble(min_ratio), Cdouble(ftol), Cdouble(cg_tol), Cdouble(lambda0)))
  out = fill(NaN, 3, ncams)
  status = zeros(UInt8, ncams)
  component = zeros(Int32, ncams)
  kept = zeros(UInt8, npairs)
  n_loops = zeros(Int32, npairs)
  support = zeros(Int32, npairs)
  residual = fill(NaN, npairs)
  edge_weight = zeros(Float64, npairs)
  iterations = Ref{Int32}(0)
  cg_iterations = Ref{Int32}(0)
  trace = zeros(Float64, 4, max_iterations)
  cost = zeros(Float64, 2)
  counts = zeros(Int64, 4)
  GC.@preserve pairs_a pairs_b dir weights bytes c0 held opts out status component kept n_loops support residual edge_weight trace cost counts begin
    bacheck(ccall((:ba_average_translations, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{UInt8},
                   Ptr{BaTransavgOpts}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                   Ref{Int32}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                  nlp.handle, npairs, pointer(pairs_a), pointer(pairs_b), pointer(dir), _or_null(weights, Float64), _or_null(bytes, UInt8),
                  _or_null(c0, Float64), _or_null(held, UInt8), Base.unsafe_convert(Ptr{BaTransavgOpts}, opts), pointer(out),
                  pointer(status), pointer(component), pointer(kept), pointer(n_loops), pointer(support), pointer(residual),
                  pointer(edge_weight), iterations, cg_iterations, pointer(trace), pointer(cost), pointer(counts)))
  end
  return out, status, component, kept .!= 0, n_loops, support, residual, edge_weight, Int(iterations[]), Int(cg_iterations[]),
         trace[:, 1:iterations[]], cost, counts
end

# Similarity alignment of reconstructions (an extension): include/ba_hip.h, ba_similarity.  (s, R, t) with dst ~ s R src + t from
# 3D-3D correspondences: src, dst are 3 x n, offsets (0-based, nprob + 1 entries from 0 to n) split them into independent
# problems (empty: one problem of all rows), used holds one Bool per row (nothing: all; a row with a number that is not finite
# is never used).  With a threshold (the units of dst) the consensus stage stands in front (samples of 3..16, default 3;
# min_inliers at least 3); with_scale = false fixes s = 1.  Returns sim (7 x nprob: s, the rotation vector, t; NaN where the
# state is not 0), status (BA_SM_*), the inlier mask per row, the size of every problem's set, its winning hypothesis, the rms
# of the residual over the set and the problems per state.
function similarity(nlp, src :: Matrix{Float64}, dst :: Matrix{Float64}; offsets :: Vector{Int64} = Int64[], used = nothing,
                    threshold :: Union{Real, Nothing} = nothing, hypotheses :: Integer = 0, sample :: Integer = 0,
                    refits :: Integer = -1, min_inliers :: Integer = 0, seed :: Integer = 0, with_scale :: Bool = true)
  n = size(src, 2)
  size(src, 1) == 3 && size(dst) == size(src) || error("similarity: src and dst must be 3 x n")
  row_ptr = isempty(offsets) ? Int64[0, n] : offsets
  row_ptr[1] == 0 && row_ptr[end] == n && issorted(row_ptr) || error("similarity: offsets run from 0 to n and do not decrease")
  nprob = length(row_ptr) - 1
  bytes = _used_bytes(used, n)
  sim = fill(NaN, 7, nprob)
  status = zeros(UInt8, nprob)
  inlier = zeros(UInt8, n)
  n_inliers = zeros(Int32, nprob)
  best_hyp = zeros(Int32, nprob)
  rms = fill(NaN, nprob)
  counts = zeros(Int64, 4)
  opts = Ref(BaRansacOpts(Cdouble(threshold === nothing ? 1.0 : threshold), Cint(hypotheses), Cint(sample), Cint(refits),
                          Cint(min_inliers), UInt64(seed)))
  GC.@preserve row_ptr src dst bytes opts sim status inlier n_inliers best_hyp rms counts begin
    optr = threshold === nothing ? Ptr{BaRansacOpts}(C_NULL) : Base.unsafe_convert(Ptr{BaRansacOpts}, opts)
    bacheck(ccall((:ba_similarity, libba), Cint,
                  (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{BaRansacOpts}, Cint, Ptr{Float64}, Ptr{UInt8},
                   Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}),
                  nlp.handle, nprob, pointer(row_ptr), pointer(src), pointer(dst), _or_null(bytes, UInt8), optr, Cint(with_scale),
                  pointer(sim), pointer(status), pointer(inlier), pointer(n_inliers), pointer(best_hyp), pointer(rms), pointer(counts)))
  end
  return sim, status, inlier .!= 0, n_inliers, best_hyp, rms, counts
end
