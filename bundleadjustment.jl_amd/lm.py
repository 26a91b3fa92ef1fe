"""Levenberg_Marquardt(model, facto, perm, normalize[, linesearch]; kwargs...) -- host mirror of the two solver
entry points of the reference over ba_lm_solve (include/ba_hip.h):

  * 4 positional arguments  -> src/LevenbergMarquardt.jl:16-26 (old API; what src/solve_ba.jl:26 calls)
  * 5 positional arguments  -> src/lm.jl:15-26 (new API with `linesearch`; src/main.jl:30, src/diffprecsions.jl:41)

Keyword names follow the reference with ASCII spellings (νd -> nu_d, νm -> nu_m, λ -> lam, δd -> delta_d).
Returns a GenericExecutionStats with the fields the reference fills (src/lm.jl:409-415,
src/LevenbergMarquardt.jl:384).
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .model import BALNLPModel, FeasibilityResidual

_FACTO = {"LDL": 0, "QR": 1, "PCG": 2}
_NORM = {"None": 0, "J": 1, "A": 2}
_PERM = ("AMD", "Metis", "natural")


@dataclass
class GenericExecutionStats:
    status: str
    solution: np.ndarray
    objective: float
    iter: int
    elapsed_time: float
    dual_feas: float = float("inf")
    primal_feas: float = float("inf")
    # extras (not in the reference struct)
    loop_time: float = 0.0
    n_accepted: int = 0
    n_rejected: int = 0
    n_residual: int = 0
    n_jacobian: int = 0
    n_factor: int = 0
    lambda_final: float = 0.0
    log: list = field(default_factory=list)
    n_cg: int = 0  # facto = :PCG: conjugate-gradient iterations over the whole solve

    def __str__(self):
        return (f"Generic Execution stats\n  status: {self.status}\n  objective value: {self.objective!r}\n"
                f"  primal feasibility: {self.primal_feas!r}\n  dual feasibility: {self.dual_feas!r}\n"
                f"  solution: [{'  '.join(repr(float(v)) for v in self.solution[:4])} ⋯ {float(self.solution[-1])!r}]\n"
                f"  iterations: {self.iter}\n  elapsed time: {self.elapsed_time!r}")


def _sym(s):
    return s[1:] if isinstance(s, str) and s.startswith(":") else s


def Levenberg_Marquardt(model, facto, perm, normalize, linesearch=None, *, x=None, facto_type=None,
                        restol=None, satol=None, srtol=None, oatol=None, ortol=None, atol=None, rtol=None,
                        nu_d=None, nu_m=None, lam=None, delta_d=None, ite_max=None, max_time=None, verbose=False,
                        log=True, pcg_tol=None, pcg_max_iter=None, x_device_ptr=None, loss="linear", f_scale=1.0,
                        fixed_cameras=None, fixed_points=None, fixed_camera_params=None, point_priors=None,
                        camera_priors=None, centre_priors=None, shared_intrinsics=None, obs_info=None):
    """x_device_ptr (an extension for device-resident callers, e.g. bench.py): the address of nvar doubles of DEVICE memory
    holding x0; the loop then runs through ba_lm_solve_dev -- no host copy of the iterate on either side -- the solution
    stays there and `solution` of the result is None.

    loss / f_scale (an extension, scipy's least_squares names): minimise f = 1/2 sum_i c^2 rho(|r_i|^2 / c^2) over the
    observations i, c = f_scale in pixels, rho one of "linear" (the default: 1/2 |r|^2, the reference's objective), "huber",
    "soft_l1", "cauchy", "arctan" (":huber" symbols are accepted).  The step is the reweighted (IRLS) one, see ba_lm_set_loss
    in include/ba_hip.h; `objective`, the log's f and |J'r| are then the robust f and its gradient norm.  Not with linesearch
    = True, a Float32 model or facto_type = Float16 (ValueError).

    fixed_cameras / fixed_points / fixed_camera_params (an extension): parameters held at their values in x0, the solve
    runs over the free entries only (see _lib.fixed_masks for the forms and ba_lm_set_fixed in include/ba_hip.h for the
    semantics).  Set on the handle at every call: a call without them runs the unmasked path.  Not with facto_type =
    Float16 (ValueError).

    point_priors / camera_priors / centre_priors (an extension): Gaussian priors (index, mu, info) on points, camera blocks
    (r, t, k1, k2, f) and camera centres c = -R(r)' t, added to the objective as 1/2 (h(x) - mu)' info (h(x) - mu) -- ground
    control points, calibration priors or an earlier solve's posterior, GPS positions (see _lib._prior_lists for the forms and
    ba_lm_set_priors in include/ba_hip.h for the semantics).  `objective`, the log's f and |J'r| include them; they are not
    passed through the robust loss.  Set on the handle at every call: a call without them runs the path without priors.  Not
    with linesearch = True, a Float32 model or facto_type = Float16 (ValueError).

    shared_intrinsics (an extension): calibration groups -- cameras that share one (k1, k2, f), estimated from all their
    images: an array of ncams labels (0: own intrinsics, g in 1..8: member of group g) or a list of lists of 1-based camera
    indices (see _lib.shared_labels for the forms and ba_lm_set_shared_intrinsics in include/ba_hip.h for the semantics).  The
    members of a group must hold identical (k1, k2, f) in x0 (tie_intrinsics makes such an x) and come back identical;
    dual_feas and the log's |J'r| are the gradient over the tied parameters.  Set on the handle at every call: a call without
    it runs the untied path.  Not with facto_type = Float32 / Float16, a Float32 model, normalize :J / :A or linesearch = True
    (ValueError).

    obs_info (an extension): the uncertainty of every observation -- standard deviations in pixels, (nobs,) isotropic or
    (nobs, 2) sigma_x, sigma_y (inf: dropped), or 2 x 2 information matrices (nobs, 2, 2), symmetric positive semi-definite
    (see _lib.obs_info_pack for the forms and ba_lm_set_obs_info in include/ba_hip.h for the semantics).  The objective becomes
    1/2 sum_i r_i' Lambda_i r_i; a robust loss then acts on the Mahalanobis distance and f_scale is in units of sigma;
    `objective`, the log's f and |J'r| are those of the whitened problem.  Set on the handle at every call: a call without
    it runs the unweighted path.  Not with linesearch = True, a Float32 model or facto_type = Float16 (ValueError)."""
    terms = _lib.ProblemTerms(loss, f_scale, fixed_cameras, fixed_points, fixed_camera_params, point_priors, camera_priors,
                              centre_priors, shared_intrinsics, obs_info)
    terms.refuse(linesearch=linesearch, facto_type=facto_type, normalize=normalize)
    facto, perm, normalize = _sym(facto), _sym(perm), _sym(normalize)
    if facto not in _FACTO:
        raise ValueError(f"facto must be :QR, :LDL or :PCG (extension: matrix-free CG on the reduced camera system), got {facto!r}")
    if perm not in _PERM:
        raise ValueError(f"perm must be :AMD or :Metis (or :natural, an extension: the caller's camera numbering), got {perm!r}")
    if normalize not in _NORM:
        raise ValueError(f"normalize must be :None, :J or :A, got {normalize!r}")
    nlp = model.nlp if isinstance(model, FeasibilityResidual) else model
    if not isinstance(nlp, BALNLPModel):
        raise TypeError("model must be a FeasibilityResidual(BALNLPModel) or a BALNLPModel")
    xf32 = nlp.T is np.float32  # eltype(x) = Float32: facto_type defaults to it (lm.jl:20), eps(T) tolerances
    terms.refuse(xf32=xf32)
    variant = 0 if linesearch is None else 1
    if variant == 0 and (facto_type is not None or max_time is not None):
        raise TypeError("LevenbergMarquardt.jl's Levenberg_Marquardt has no facto_type / max_time keyword")
    if x_device_ptr is not None and x is not None:
        raise TypeError("x and x_device_ptr are exclusive")
    x0 = None if x_device_ptr is not None else np.array(nlp.meta.x0 if x is None else x, dtype=np.float64, copy=True)
    if x0 is not None and x0.shape != (nlp.meta.nvar,):
        raise ValueError("x has the wrong length")
    if facto_type is not None and np.dtype(facto_type) not in (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError("facto_type must be Float64, Float32 or Float16")
    # ba_lm_opts.facto_type: 0 = eltype(x), 1 = Float32, 2 = Float16 (src/lm.jl:165-173)
    if facto_type is None:
        ft = 1 if (xf32 and variant == 1) else 0  # facto_type defaults to eltype(x) (lm.jl:20)
    else:
        ft = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.float16): 2}[np.dtype(facto_type)]
    if ft == 2 and _FACTO[facto] != 0:
        raise ValueError("facto_type = Float16 exists in the :LDL branch only (src/lm.jl:92-95)")
    if facto == "PCG" and normalize != "None":
        raise ValueError("facto = :PCG has its own scaling (block-Jacobi preconditioner): normalize must be :None")
    if facto == "PCG" and facto_type is not None and ft == 1 and not xf32:
        raise ValueError("facto = :PCG runs in Float64: facto_type = Float32 belongs to the direct branches")

    def d(v):
        return -1.0 if v is None else float(v)

    o = _lib.LMOpts(variant=variant, facto=_FACTO[facto], normalize=_NORM[normalize], linesearch=int(bool(linesearch)),
                    facto_type=ft, ite_max=-1 if ite_max is None else int(ite_max), verbose=int(verbose), x_f32=int(xf32),
                    restol=d(restol), satol=d(satol), srtol=d(srtol), oatol=d(oatol), ortol=d(ortol), atol=d(atol),
                    rtol=d(rtol), nu_d=d(nu_d), nu_m=d(nu_m), lam=d(lam), delta_d=d(delta_d), max_time=d(max_time),
                    pcg_tol=d(pcg_tol), pcg_max_iter=-1 if pcg_max_iter is None else int(pcg_max_iter),
                    perm=_lib.ORDERINGS[perm])  # src/lm.jl:84-88: orders the cameras of the reduced system (ba_order.cpp)
    st = _lib.LMStats()
    rows = []

    def _cb(ctx, it, f, df, njtr, lmb, nd, rho, acc):
        rows.append((it, f, df, njtr, lmb, nd, rho, bool(acc)))

    cb = _lib.LOG_CB(_cb) if log else C.cast(None, _lib.LOG_CB)
    terms.apply(nlp, x0)  # every call: one without a term's keyword runs without that term
    if x_device_ptr is not None:
        _lib.check(_lib.lib().ba_lm_solve_dev(nlp.handle, C.byref(o), C.c_void_p(int(x_device_ptr)), C.byref(st), cb, None))
    else:
        _lib.check(_lib.lib().ba_lm_solve(nlp.handle, C.byref(o), _lib.ptr(x0), C.byref(st), cb, None))
    nlp.counters.neval_cons += st.n_residual
    nlp.counters.neval_residual += st.n_residual
    nlp.counters.neval_jac += st.n_jacobian + 1  # + jac_structure! (src/BALNLPModels.jl:126)
    nlp.counters.neval_jac_residual += st.n_jacobian
    out = GenericExecutionStats(status=_lib.STATUS[st.status], solution=None if x0 is None else (x0.astype(nlp.T) if xf32 else x0), objective=st.objective, iter=st.iter,
                                elapsed_time=st.elapsed_s, loop_time=st.loop_s, n_accepted=st.n_accepted,
                                n_rejected=st.n_rejected, n_residual=st.n_residual, n_jacobian=st.n_jacobian,
                                n_factor=st.n_factor, lambda_final=st.lambda_final, log=rows, n_cg=st.n_cg)
    if variant == 1:
        out.dual_feas = st.dual_feas    # lm.jl:415
    else:
        out.primal_feas = st.dual_feas  # LevenbergMarquardt.jl:384 passes |J'r| as primal_feas
    return out


def lm_step(nlp, x, lam, want_jtr=True, facto_type=None, pcg=None, loss=None, f_scale=1.0, fixed_cameras=None,
            fixed_points=None, fixed_camera_params=None, point_priors=None, camera_priors=None, centre_priors=None,
            shared_intrinsics=None, obs_info=None):
    """One linear LM step from (x, lambda): delta, 1/2|J delta + r|^2, J'r  (ba_lm_step; facto_type=np.float32:
    ba_lm_step_f32, the reduced camera system factored in Float32 as src/lm.jl:170-173 does; pcg=(tol, max_iter):
    ba_lm_step_pcg, the step by preconditioned CG -- the CG iteration count is then appended to the result).
    loss / f_scale (see Levenberg_Marquardt; None = "linear"): the reweighted step, 1/2|J~ delta + r~|^2 and J~'r~.
    fixed_* (see Levenberg_Marquardt): the step over the free entries; the fixed entries of delta and J'r are exactly 0.
    *_priors (see Levenberg_Marquardt): the step of the objective with the prior terms; they are in all three outputs.
    shared_intrinsics (see Levenberg_Marquardt): the step over the tied parameters, expanded to the layout of x (the members of
    a group receive identical steps); J'r holds a group's summed gradient at its first member and exact zeros at the other
    members' (k1, k2, f).  Not with facto_type = Float32 (ValueError).
    obs_info (see Levenberg_Marquardt): the step of the whitened problem; all three outputs are quantities of r^ and J^."""
    terms = _lib.ProblemTerms("linear" if loss is None else loss, f_scale, fixed_cameras, fixed_points, fixed_camera_params,
                              point_priors, camera_priors, centre_priors, shared_intrinsics, obs_info)
    f64 = facto_type is None or np.dtype(facto_type) == np.float64
    terms.refuse(facto_type=None if f64 else np.float32)  # (the step has one other factorisation)
    x = np.ascontiguousarray(x, dtype=np.float64)
    terms.apply(nlp, x)
    delta = np.empty(nlp.meta.nvar)
    jtr = np.empty(nlp.meta.nvar) if want_jtr else None
    half = C.c_double(0)
    if pcg is not None:
        its = C.c_int(0)
        _lib.check(_lib.lib().ba_lm_step_pcg(nlp.handle, _lib.ptr(x), float(lam), float(pcg[0]), int(pcg[1]), _lib.ptr(delta),
                                             C.byref(half), _lib.ptr(jtr) if want_jtr else None, C.byref(its)))
        return delta, half.value, jtr, its.value
    f32 = facto_type is not None and np.dtype(facto_type) == np.float32
    fn = _lib.lib().ba_lm_step_f32 if f32 else _lib.lib().ba_lm_step
    _lib.check(fn(nlp.handle, _lib.ptr(x), float(lam), _lib.ptr(delta), C.byref(half), _lib.ptr(jtr) if want_jtr else None))
    return delta, half.value, jtr


def covariance(nlp, x, lam=0.0, *, loss=None, f_scale=1.0, fixed_cameras=None, fixed_points=None, fixed_camera_params=None,
               rank_tol=None, cameras=True, points=True, point_priors=None, camera_priors=None, centre_priors=None,
               obs_info=None):
    """Covariance at x (ba_covariance): the diagonal blocks of (J~_F'J~_F + sum_k H_k' info_k H_k + lam I)^-1, J~ the Jacobian
    as lm_step sees it under `loss` / `f_scale` and the fixed_* options, the sum over the *_priors (see Levenberg_Marquardt),
    F the free entries; obs_info (see Levenberg_Marquardt): J~ is whitened by the observations' information first, so the
    result is in the units the sigmas were given in.  Priors that fix the gauge softly make it well defined at lam = 0.  Returns (cam_cov (ncams,
    9, 9) or None, pnt_cov (npnts, 3, 3) or None, min_rel_pivot): camera blocks in block order r1 r2 r3 t1 t2 t3 k1 k2 f,
    rows and columns of fixed entries exactly 0, not scaled by a residual variance (multiply by 2 f / (nequ - n_free) for
    that).  min_rel_pivot = min D_i / S_ii of the factored reduced camera system; at or below rank_tol (None: 1e-10, 0: no
    check) it is numerically singular -- the gauge left free at lam = 0 -- and SQDException is raised (with the value as its
    min_rel_pivot attribute).  Bad arguments raise ValueError before any device call."""
    terms = _lib.ProblemTerms("linear" if loss is None else loss, f_scale, fixed_cameras, fixed_points, fixed_camera_params,
                              point_priors, camera_priors, centre_priors, obs_info=obs_info)
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        raise ValueError(f"lam must be a finite number >= 0, got {lam!r}") from None
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError(f"lam must be a finite number >= 0, got {lam!r}")
    if rank_tol is None:
        tol = -1.0
    else:
        try:
            tol = float(rank_tol)
        except (TypeError, ValueError):
            raise ValueError(f"rank_tol must be a finite number >= 0 (or None), got {rank_tol!r}") from None
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError(f"rank_tol must be a finite number >= 0 (or None), got {rank_tol!r}")
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (nlp.meta.nvar,):
        raise ValueError(f"x must have shape ({nlp.meta.nvar},), got {x.shape}")
    terms.apply(nlp, shared=False)  # (a grouping left on the handle stays: ba_covariance refuses it)
    cam = np.empty((nlp.ncams, 9, 9)) if cameras else None
    pnt = np.empty((nlp.npnts, 3, 3)) if points else None
    piv = C.c_double(0)
    try:
        _lib.check(_lib.lib().ba_covariance(nlp.handle, _lib.ptr(x), lam, tol, _lib.ptr(cam) if cameras else None,
                                            _lib.ptr(pnt) if points else None, C.byref(piv)))
    except _lib.SQDException as e:
        e.min_rel_pivot = piv.value
        raise
    return cam, pnt, piv.value


def _opt_float(v, what):
    """None, or a finite float (ValueError otherwise)"""
    if v is None:
        return None
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a finite number (or None), got {v!r}") from None
    if not np.isfinite(f):
        raise ValueError(f"{what} must be a finite number (or None), got {v!r}")
    return f


def _block_args(nlp, x, max_iter, xtol, lam0):
    """The arguments refine_points and refine_cameras share, checked (ValueError) -> (a Float64 copy of x, (max_iter, xtol, lam0)
    as the C entries take them: a negative value for None, the entry's default).  nlp is read last, for the length of x."""
    if max_iter is not None and (not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool) or max_iter < 0):
        raise ValueError(f"max_iter must be an integer >= 0 (or None), got {max_iter!r}")
    tol, l0 = _opt_float(xtol, "xtol"), _opt_float(lam0, "lam0")
    if (tol is not None and tol <= 0) or (l0 is not None and l0 <= 0):
        raise ValueError(f"xtol and lam0 must be > 0 (or None), got {xtol!r} and {lam0!r}")
    x = np.array(x, dtype=np.float64, copy=True)
    if x.shape != (nlp.meta.nvar,):
        raise ValueError(f"x must have shape ({nlp.meta.nvar},), got {x.shape}")
    return x, (-1 if max_iter is None else int(max_iter), -1.0 if tol is None else tol, -1.0 if l0 is None else l0)


def _block_info(status, cost, counts, its):
    """the info dict of refine_points and refine_cameras from what the C entry filled"""
    names = np.array(_lib.POINT_STATES)
    return dict(status=names[status & 0x7F], behind=(status & _lib.POINT_BEHIND) != 0, cost_before=cost[:, 0].copy(),
                cost_after=cost[:, 1].copy(), iters_max=its.value,
                counts={**{n: int(c) for n, c in zip(_lib.POINT_STATES, counts)}, "behind": int(counts[-1])})


def refine_points(nlp, x, *, triangulate=False, max_iter=None, xtol=None, lam0=None, loss=None, f_scale=1.0, obs_info=None,
                  fixed_points=None, point_priors=None, ransac=None):
    """The points of x with its cameras held (ba_refine_points): every point is an independent problem in 3 unknowns -- the
    objective of Levenberg_Marquardt under `loss` / `f_scale`, `obs_info` and `point_priors`, restricted to that point -- solved
    by a Marquardt iteration of its own (accept test, damping and stopping test per point).  triangulate=True starts every
    point from the linear triangulation of its rays instead of from x (the points of x are then not read): how an x0 is built
    when only cameras are known.  max_iter (None: 50; 0: evaluate only -- with triangulate=True the triangulated points are
    returned), xtol (None: 1e-10; |delta| <= xtol (|X| + xtol)), lam0 (None: 1e-4).  fixed_points are skipped.
    ransac=dict(threshold=, hypotheses=, refits=, min_inliers=, seed=) with triangulate=True puts a consensus stage in front
    (ba_ransac_points; _lib.ransac_opts for the ranges, `sample` 2 or unset): every pair of a point's observations -- `hypotheses`
    random pairs where the point has more pairs than that -- is triangulated and scored by its inliers (reprojection within
    `threshold` pixels, in front of the camera), the best pair defines the point's inlier set, up to `refits` triangulations on
    the set re-score it, and the triangulation and the refinement run on that set only -- the result has the bits of
    triangulate=True with an obs_info that drops the outliers.  A point whose best pair has fewer than `min_inliers` (None: 2)
    inliers is `degenerate`.  info then also holds `inliers` (bool, nobs), `n_inliers` and `best_hypothesis` (per point; -1: not
    attempted or no valid pair).
    Returns (x_new, info): x_new a copy of x with the points replaced (cameras and skipped points bit-identical); info a dict
    with `status` (npnts names among _lib.POINT_STATES), `behind` (bool: at the returned point an observation sees it from
    behind, P1.z >= 0), `cost_before`, `cost_after` (per point, cost_after <= cost_before), `counts` (points per status name,
    plus "behind") and `iters_max`.  Bad arguments raise ValueError before any device call."""
    terms = _lib.ProblemTerms("linear" if loss is None else loss, f_scale, fixed_points=fixed_points, point_priors=point_priors,
                              obs_info=obs_info)
    if not isinstance(triangulate, (bool, np.bool_)):
        raise ValueError(f"triangulate must be True or False, got {triangulate!r}")
    opts = None
    if ransac is not None:
        if not triangulate:
            raise ValueError("ransac needs triangulate=True (the consensus stage stands in front of the linear triangulation)")
        opts = _lib.ransac_opts(ransac, least=2, most=2, least_set=2)
    x, args = _block_args(nlp, x, max_iter, xtol, lam0)
    terms.apply(nlp, shared=False)  # (a grouping concerns the cameras: what the handle holds stays)
    status, cost = np.zeros(nlp.npnts, dtype=np.uint8), np.zeros((nlp.npnts, 2))
    counts, its = np.zeros(len(_lib.POINT_STATES) + 1, dtype=np.int64), C.c_int(0)
    if opts is not None:
        inlier, n_in, best = np.zeros(nlp.nobs, dtype=np.uint8), np.zeros(nlp.npnts, dtype=np.int32), np.zeros(nlp.npnts, dtype=np.int32)
        _lib.check(_lib.lib().ba_ransac_points(nlp.handle, _lib.ptr(x), C.byref(opts), *args, _lib.ptr(status), _lib.ptr(cost),
                                               _lib.ptr(counts), C.byref(its), _lib.ptr(inlier), _lib.ptr(n_in), _lib.ptr(best)))
        return x, dict(_block_info(status, cost, counts, its), inliers=inlier != 0, n_inliers=n_in, best_hypothesis=best)
    _lib.check(_lib.lib().ba_refine_points(nlp.handle, _lib.ptr(x), int(bool(triangulate)), *args, _lib.ptr(status), _lib.ptr(cost),
                                           _lib.ptr(counts), C.byref(its)))
    return x, _block_info(status, cost, counts, its)


def refine_cameras(nlp, x, *, resect=False, estimate_focal=False, ransac=None, minimal=None, max_iter=None, xtol=None, lam0=None, loss=None, f_scale=1.0, obs_info=None, fixed_cameras=None,
                   fixed_camera_params=None, camera_priors=None, centre_priors=None, shared_intrinsics=None):
    """The cameras of x with its points held (ba_refine_cameras), the other half of refine_points: every camera is an independent
    problem in at most 9 unknowns -- the objective of Levenberg_Marquardt under `loss` / `f_scale`, `obs_info`, `camera_priors`
    and `centre_priors`, restricted to that camera -- solved by a Marquardt iteration of its own (accept test, damping and
    stopping test per camera).  resect=True starts every camera whose pose is free from the linear resection of its 2D-3D
    correspondences instead of from x (ba_resect_cameras: the pose of x is then not read, NaN included; a camera with a held
    pose component starts from x as before; fewer than 6 observations or a degenerate configuration: `degenerate`, untouched):
    how new images are registered against a structure, and with refine_points(triangulate=True) how an x0 is built.
    ransac=dict(threshold=, hypotheses=, sample=, refits=, min_inliers=, seed=) with resect=True puts a consensus stage in front
    (ba_ransac_cameras; _lib.ransac_opts for the ranges): `hypotheses` minimal samples of `sample` correspondences per camera are
    resected and scored by their inliers (reprojection within `threshold` pixels, in front of the camera), the best one defines
    the inlier set, up to `refits` linear refits on the set re-score it, and the resection and the refinement run on that set
    only -- the result has the bits of resect=True with an obs_info that drops the outliers.  A camera whose best hypothesis has
    fewer than `min_inliers` inliers is `degenerate`.  info then also holds `inliers` (bool, nobs), `n_inliers` and
    `best_hypothesis` (per camera; -1: not attempted or no valid hypothesis).
    estimate_focal=True with resect=True (ba_resect_cameras_focal, with ransac ba_ransac_cameras_focal) registers images without
    calibration: every camera whose pose and f are both free (f not in fixed_camera_params, the camera in no group of
    shared_intrinsics) gets f from the linear stage along with its pose -- its (r, t, f) and free k1, k2 in x are not read, NaN
    included; f is written into x_new, a free k1 / k2 starts the refinement at 0, a held one keeps its value and is ignored by
    the linear stage.  Every hypothesis of the consensus stage then carries its own f.  A camera with f held or in a group is
    resected with the intrinsics of x as without the flag.  On noisy data the linear f is only a start for the refinement.
    minimal="p3p" with resect=True and ransac= (ba_ransac_cameras_p3p) draws three correspondences per hypothesis instead of six and
    solves them exactly: every real P3P pose (up to four) is scored and the best is the hypothesis.  A sample is clean with
    probability w^3 instead of w^6 at inlier share w, which is what registers a camera at 60-70 % wrong matches.  `sample` must be
    3 (or unset); min_inliers is still at least 6, the winner, the refits and the finish are those of the ransac= call, and so
    is the returned dict.  It needs the intrinsics of x (a camera whose f is not finite or 0 is `degenerate`) and excludes
    estimate_focal=True.  None: the six-point linear hypotheses.
    max_iter (None: 100; 0: evaluate only -- with resect=True the resected poses are returned), xtol (None: 1e-10; |D delta| <= xtol (|D C| + xtol) with
    D_j = sqrt(H_jj): the predicted motion in pixels), lam0 (None: 1e-4).  fixed_camera_params hold components (("k1", "k2",
    "f"): a pose-only refit); fixed_cameras are skipped; the members of the groups of shared_intrinsics keep their (k1, k2, f).
    Returns (x_new, info): x_new a copy of x with the cameras replaced (points, held components and skipped cameras
    bit-identical); info a dict with `status` (ncams names among _lib.POINT_STATES), `behind` (bool: at the returned camera an
    observation sees its point from behind, P1.z >= 0), `cost_before`, `cost_after` (per camera, cost_after <= cost_before),
    `counts` (cameras per status name, plus "behind") and `iters_max`.  Bad arguments raise ValueError before any device call."""
    terms = _lib.ProblemTerms("linear" if loss is None else loss, f_scale, fixed_cameras=fixed_cameras,
                              fixed_camera_params=fixed_camera_params, camera_priors=camera_priors, centre_priors=centre_priors,
                              shared_intrinsics=shared_intrinsics, obs_info=obs_info)
    if not isinstance(resect, (bool, np.bool_)):
        raise ValueError(f"resect must be True or False, got {resect!r}")
    if not isinstance(estimate_focal, (bool, np.bool_)):
        raise ValueError(f"estimate_focal must be True or False, got {estimate_focal!r}")
    if estimate_focal and not resect:
        raise ValueError("estimate_focal needs resect=True (the focal length comes out of the linear resection)")
    if minimal is not None and not (isinstance(minimal, str) and minimal == "p3p"):
        raise ValueError(f'minimal must be "p3p" or None, got {minimal!r}')
    if minimal is not None and (not resect or ransac is None):
        raise ValueError('minimal="p3p" needs resect=True and ransac= (P3P is the hypothesis generator of the consensus stage)')
    if minimal is not None and estimate_focal:
        raise ValueError('minimal="p3p" excludes estimate_focal=True (P3P needs the focal length; P4Pf is not provided)')
    focal = "_p3p" if minimal is not None else ("_focal" if estimate_focal else "")
    opts = None
    if ransac is not None:
        if not resect:
            raise ValueError("ransac needs resect=True (the consensus stage stands in front of the linear resection)")
        opts = _lib.ransac_opts(ransac, least=3, most=3, least_set=6) if minimal is not None else _lib.ransac_opts(ransac)
    x, args = _block_args(nlp, x, max_iter, xtol, lam0)
    terms.apply(nlp)  # (x is not checked against the grouping: the members' intrinsics are held, whatever they are)
    status, cost = np.zeros(nlp.ncams, dtype=np.uint8), np.zeros((nlp.ncams, 2))
    counts, its = np.zeros(len(_lib.POINT_STATES) + 1, dtype=np.int64), C.c_int(0)
    if opts is not None:
        inlier, n_in, best = np.zeros(nlp.nobs, dtype=np.uint8), np.zeros(nlp.ncams, dtype=np.int32), np.zeros(nlp.ncams, dtype=np.int32)
        _lib.check(getattr(_lib.lib(), "ba_ransac_cameras" + focal)(nlp.handle, _lib.ptr(x), C.byref(opts), *args, _lib.ptr(status), _lib.ptr(cost),
                                                _lib.ptr(counts), C.byref(its), _lib.ptr(inlier), _lib.ptr(n_in), _lib.ptr(best)))
        return x, dict(_block_info(status, cost, counts, its), inliers=inlier != 0, n_inliers=n_in, best_hypothesis=best)
    entry = getattr(_lib.lib(), "ba_resect_cameras" + focal) if resect else _lib.lib().ba_refine_cameras
    _lib.check(entry(nlp.handle, _lib.ptr(x), *args, _lib.ptr(status), _lib.ptr(cost), _lib.ptr(counts), C.byref(its)))
    return x, _block_info(status, cost, counts, its)


def pair_matches(problem, pairs):
    """The match lists of camera pairs (ba_pair_matches; host only, no device): problem is a BALNLPModel or a dict with cam_idx1,
    pnt_idx1, ncams and npnts (what synthetic.make_problem returns); pairs is (npairs, 2), 1-based cameras.
    Returns (match_ptr, obs_a, obs_b), 0-based: the matches of pair k are obs_a[match_ptr[k]:match_ptr[k + 1]] (camera a's
    observations, in the order of a's list) and obs_b (camera b's first observation of the same point)."""
    if isinstance(problem, dict):
        cam, pnt, ncams, npnts = problem["cam_idx1"], problem["pnt_idx1"], problem["ncams"], problem["npnts"]
    else:
        cam, pnt, ncams, npnts = problem.cams_indices, problem.pnts_indices, problem.ncams, problem.npnts
    return _lib.pair_matches(cam, pnt, ncams, npnts, pairs)


def relative_pose(nlp, x, pairs, *, ransac=None, obs_info=None, **chain):
    """The relative pose of camera pairs from their 2D-2D matches (ba_relative_pose): the eight-point essential matrix, with
    ransac=dict(threshold=, hypotheses=, sample=, refits=, min_inliers=, seed=) behind a consensus stage (_lib.ransac_opts with
    sample in 8..16, default 8, and min_inliers >= 8).  pairs: (npairs, 2), 1-based cameras (a, b).  Of x only (k1, k2, f) of the
    pairs' cameras are read: the poses and the points may be NaN.  obs_info: as in Levenberg_Marquardt, here only "information 0
    drops the observation" -- a match is used iff both its observations are.
    Returns a dict: `r`, `t` (npairs, 3): P_b = R(r) P_a + t with |t| = 1, NaN where the pair has no pose; `status` (names among
    _lib.PAIR_STATES); `match_ptr` and, per match in the order of pair_matches, `inliers` (bool); `n_inliers`; `best_hypothesis`
    (-1: none); `counts` (pairs per state).  compose_relative turns (r, t) into camera b's pose.  On noisy data the eight-point
    fit is only a start for the refinement that follows: refine=dict(...) (the one further keyword; None: no refinement) chains
    refine_relative_pose behind the call, the dict holding its options (_lib.PAIR_REFINE_KEYS), threshold defaulting to the
    ransac threshold.  Bad arguments raise ValueError before any device call."""
    refine = _refine_option("relative_pose", chain, ransac)
    return _relative_pose("ba_relative_pose", None if ransac is None else _lib.ransac_opts(ransac, least=8), nlp, x, pairs, obs_info, refine)


def _refine_option(who, chain, ransac):
    """the keyword arguments of refine_relative_pose from the `refine=` of relative_pose* (None: no refinement).  `refine` arrives
    in **chain: the keyword-only defaults of relative_pose* are pinned by their tests, and None is today's call, bit for bit."""
    unknown = [k for k in chain if k != "refine"]
    if unknown:
        raise TypeError(f"{who}() got an unexpected keyword argument {unknown[0]!r}")
    refine = chain.get("refine")
    if refine is None:
        return None
    if not isinstance(refine, dict):
        raise ValueError(f"refine must be a dict with the keys {', '.join(_lib.PAIR_REFINE_KEYS)} (or None), got {refine!r}")
    unknown = [k for k in refine if k not in _lib.PAIR_REFINE_KEYS]
    if unknown:
        raise ValueError(f"refine: unknown key {unknown[0]!r} (keys: {', '.join(_lib.PAIR_REFINE_KEYS)})")
    refine = dict(refine)
    if "threshold" not in refine:
        if not isinstance(ransac, dict) or "threshold" not in ransac:
            raise ValueError("refine: threshold (pixels) is required where there is no ransac threshold")
        refine["threshold"] = ransac["threshold"]
    _lib.pair_refine_opts(**refine)
    return refine


def _relative_pose(entry, opts, nlp, x, pairs, obs_info, refine=None):
    """the call of ba_relative_pose and of ba_relative_pose_five_point behind the check of their options; refine: the keyword
    arguments of the refine_relative_pose that follows, or None"""
    info3 = _lib.obs_info_pack(obs_info)
    a1, b1 = _lib._pairs(pairs, nlp.ncams)
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (nlp.meta.nvar,):
        raise ValueError(f"x must have shape ({nlp.meta.nvar},), got {x.shape}")
    if info3 is not None and info3.shape[0] != nlp.nobs:
        raise ValueError(f"obs_info: one entry per observation ({nlp.nobs}), got {info3.shape[0]}")
    n = len(a1)
    mp = np.zeros(n + 1, dtype=np.int64)  # (the counting form: the size of the inlier array)
    _lib.check(_lib.lib().ba_pair_matches(nlp.ncams, nlp.npnts, nlp.nobs, _lib.ptr(nlp.cams_indices), _lib.ptr(nlp.pnts_indices), n, _lib.ptr(a1),
                                          _lib.ptr(b1), _lib.ptr(mp), None, None))
    _lib.set_obs_info(nlp.handle, info3)
    pose, status = np.full((n, 6), np.nan), np.zeros(n, dtype=np.uint8)
    inlier, n_in, best = np.zeros(int(mp[-1]), dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    counts, mp2 = np.zeros(len(_lib.PAIR_STATES), dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    _lib.check(getattr(_lib.lib(), entry)(nlp.handle, _lib.ptr(x), n, _lib.ptr(a1), _lib.ptr(b1), None if opts is None else C.byref(opts),
                                          _lib.ptr(pose), _lib.ptr(status), _lib.ptr(mp2), _lib.ptr(inlier), _lib.ptr(n_in), _lib.ptr(best),
                                          _lib.ptr(counts)))
    info = dict(r=pose[:, :3].copy(), t=pose[:, 3:].copy(), status=np.array(_lib.PAIR_STATES)[status], match_ptr=mp2, inliers=inlier != 0,
                n_inliers=n_in, best_hypothesis=best, counts={s: int(c) for s, c in zip(_lib.PAIR_STATES, counts)})
    return info if refine is None else refine_relative_pose(nlp, x, pairs, info, obs_info=obs_info, **refine)


def relative_pose_five_point(nlp, x, pairs, *, ransac, obs_info=None, **chain):
    """relative_pose with the five-point minimal solver as the hypothesis generator of the consensus stage
    (ba_relative_pose_five_point): every real essential matrix through five sampled matches is a candidate; the winner, the
    refits and the final eight-point fit on the consensus set are those of relative_pose, and so is the returned dict.  ransac
    is required: dict(threshold=, hypotheses=, sample=, refits=, min_inliers=, seed=) with sample 5 (the default; nothing else
    is taken) and min_inliers >= 8 (default 8).  This is the entry for noisy detections: eight noisy matches give a poor
    hypothesis, five give a good one.  refine=dict(...) as in relative_pose.  Bad arguments raise ValueError before any device
    call."""
    if ransac is None:
        raise ValueError("relative_pose_five_point: ransac is required (the five-point solver is the hypothesis generator of the consensus stage)")
    opts = _lib.ransac_opts(ransac, least=5, most=5, least_set=8)
    refine = _refine_option("relative_pose_five_point", chain, ransac)
    return _relative_pose("ba_relative_pose_five_point", opts, nlp, x, pairs, obs_info, refine)


def refine_relative_pose(nlp, x, pairs, info, *, max_iter=None, xtol=None, lam0=None, loss=None, f_scale=1.0, threshold, rounds=None,
                         obs_info=None):
    """The non-linear refinement of the relative pose of camera pairs on their inlier sets (ba_refine_relative_pose): per pair a
    Marquardt iteration on the robustified Sampson error over the five degrees of freedom of (R, unit t), then the pair's list
    re-scored under the result; `rounds` further rounds adopt the re-scored set by the rule of the refits and refine on it.
    info: the dict relative_pose* returned for the same nlp, x, pairs and obs_info; its `r`, `t`, `status` and `inliers` are
    read.  max_iter (None: 50; 0 evaluates only), xtol (None: 1e-10, on |delta| in radians), lam0 (None: 1e-4), loss (None:
    "linear") with f_scale in pixels, threshold (pixels, required: the tau of the inlier test), rounds (None: 2; at most 8).
    Returns a dict with the keys of info -- `r`, `t`, `inliers` (the set the last refinement ran on) and `n_inliers` replaced for
    every pair that is not skipped -- plus `refine_status` (names among _lib.PAIR_REFINE_STATES), `cost_before`, `cost_after`,
    `n_consistent` (the matches that pass the inlier test under the returned pose), `iters` and `refine_counts` (pairs per
    state).  Bad arguments raise ValueError before any device call."""
    opts = _lib.pair_refine_opts(max_iter, xtol, lam0, loss, f_scale, threshold, rounds)
    info3 = _lib.obs_info_pack(obs_info)
    a1, b1 = _lib._pairs(pairs, nlp.ncams)
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (nlp.meta.nvar,):
        raise ValueError(f"x must have shape ({nlp.meta.nvar},), got {x.shape}")
    if info3 is not None and info3.shape[0] != nlp.nobs:
        raise ValueError(f"obs_info: one entry per observation ({nlp.nobs}), got {info3.shape[0]}")
    if not isinstance(info, dict) or any(k not in info for k in ("r", "t", "status", "inliers")):
        raise ValueError("info must be the dict of relative_pose or relative_pose_five_point (r, t, status, inliers are read)")
    n = len(a1)
    mp = np.zeros(n + 1, dtype=np.int64)
    _lib.check(_lib.lib().ba_pair_matches(nlp.ncams, nlp.npnts, nlp.nobs, _lib.ptr(nlp.cams_indices), _lib.ptr(nlp.pnts_indices), n, _lib.ptr(a1),
                                          _lib.ptr(b1), _lib.ptr(mp), None, None))
    r, t = np.asarray(info["r"], dtype=np.float64), np.asarray(info["t"], dtype=np.float64)
    names = np.asarray(info["status"])
    inlier = np.ascontiguousarray(np.asarray(info["inliers"]) != 0, dtype=np.uint8)
    if r.shape != (n, 3) or t.shape != (n, 3) or names.shape != (n,):
        raise ValueError(f"info: r and t must have shape ({n}, 3) and status ({n},), got {r.shape}, {t.shape}, {names.shape}")
    if inlier.shape != (int(mp[-1]),):
        raise ValueError(f"info: inliers must hold one entry per match ({int(mp[-1])}), got {inlier.shape}")
    if not np.isin(names, _lib.PAIR_STATES).all():
        raise ValueError(f"info: status must hold names among {', '.join(_lib.PAIR_STATES)}")
    status = np.array([_lib.PAIR_STATES.index(s) for s in names], dtype=np.uint8)
    pose = np.ascontiguousarray(np.concatenate([r, t], axis=1))
    _lib.set_obs_info(nlp.handle, info3)
    state, cost = np.zeros(n, dtype=np.uint8), np.zeros((n, 2))
    n_in = np.array(info["n_inliers"], dtype=np.int32) if "n_inliers" in info else np.zeros(n, dtype=np.int32)
    n_con, its = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    counts = np.zeros(len(_lib.PAIR_REFINE_STATES), dtype=np.int64)
    _lib.check(_lib.lib().ba_refine_relative_pose(nlp.handle, _lib.ptr(x), n, _lib.ptr(a1), _lib.ptr(b1), C.byref(opts), _lib.ptr(pose),
                                                  _lib.ptr(status), _lib.ptr(inlier), _lib.ptr(state), _lib.ptr(cost), _lib.ptr(n_in),
                                                  _lib.ptr(n_con), _lib.ptr(its), _lib.ptr(counts)))
    return dict(info, r=pose[:, :3].copy(), t=pose[:, 3:].copy(), inliers=inlier != 0, n_inliers=n_in,
                refine_status=np.array(_lib.PAIR_REFINE_STATES)[state], cost_before=cost[:, 0].copy(), cost_after=cost[:, 1].copy(),
                n_consistent=n_con, iters=its, refine_counts={s: int(c) for s, c in zip(_lib.PAIR_REFINE_STATES, counts)})


def five_point(nlp, qa, qb):
    """The essential matrices through five matches (ba_five_point), n independent problems: qa, qb (n, 5, 2) are undistorted
    image points already divided by f, the ray of a point is (q, -1).  Returns (E, n_sol): E (n, 10, 3, 3) holds the real
    solutions of a problem first, each with Frobenius norm 1 (d_b' E d_a = 0), NaN in the unused slots; n_sol (n,) their number.
    Neither the sign of a solution nor the order of the solutions is specified.  nlp supplies the device and the stream.
    Bad arguments raise ValueError before any device call."""
    qa, qb = np.ascontiguousarray(qa, dtype=np.float64), np.ascontiguousarray(qb, dtype=np.float64)
    if qa.ndim != 3 or qa.shape[1:] != (5, 2) or qb.shape != qa.shape:
        raise ValueError(f"five_point: qa and qb must both have shape (n, 5, 2), got {qa.shape} and {qb.shape}")
    n = qa.shape[0]
    E, n_sol = np.full((n, 10, 3, 3), np.nan), np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib().ba_five_point(nlp.handle, n, _lib.ptr(qa), _lib.ptr(qb), _lib.ptr(E), _lib.ptr(n_sol)))
    return E, n_sol


def p3p(nlp, q, X):
    """The poses of a calibrated camera through three 2D-3D correspondences (ba_p3p), n independent problems: q (n, 3, 2) are
    undistorted image points already divided by f (the ray of a point is (q, -1)), X (n, 3, 3) their world points.  Returns
    (poses, n_sol): poses (n, 4, 6) holds the solutions (r, t) of a problem first, in ascending order of the root of the
    quartic they come from, NaN in the unused slots; n_sol (n,) their number, 0..4 (0: two points coincide, the three lie on a
    line, or an entry is not finite).  nlp supplies the device and the stream.  Bad arguments raise ValueError before any device
    call."""
    q, X = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64)
    if q.ndim != 3 or q.shape[1:] != (3, 2) or X.shape != (q.shape[0], 3, 3):
        raise ValueError(f"p3p: q must have shape (n, 3, 2) and X (n, 3, 3), got {q.shape} and {X.shape}")
    n = q.shape[0]
    poses, n_sol = np.full((n, 4, 6), np.nan), np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib().ba_p3p(nlp.handle, n, _lib.ptr(q), _lib.ptr(X), _lib.ptr(poses), _lib.ptr(n_sol)))
    return poses, n_sol


def _pair_call_args(who, nlp, x, pairs, obs_info):
    """what the pair-level entries check and count before they call the library: (x, a1, b1, info3, match_ptr)"""
    info3 = _lib.obs_info_pack(obs_info)
    a1, b1 = _lib._pairs(pairs, nlp.ncams)
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (nlp.meta.nvar,):
        raise ValueError(f"x must have shape ({nlp.meta.nvar},), got {x.shape}")
    if info3 is not None and info3.shape[0] != nlp.nobs:
        raise ValueError(f"obs_info: one entry per observation ({nlp.nobs}), got {info3.shape[0]}")
    mp = np.zeros(len(a1) + 1, dtype=np.int64)
    _lib.check(_lib.lib().ba_pair_matches(nlp.ncams, nlp.npnts, nlp.nobs, _lib.ptr(nlp.cams_indices), _lib.ptr(nlp.pnts_indices), len(a1),
                                          _lib.ptr(a1), _lib.ptr(b1), _lib.ptr(mp), None, None))
    return x, a1, b1, info3, mp


def homography(nlp, x, pairs, *, ransac=None, obs_info=None):
    """The homography of camera pairs from their 2D-2D matches (ba_homography): the second two-view model, for matches on one
    plane and for pairs without a baseline, where the eight-point fit of relative_pose* is degenerate or arbitrary.  d_b ~ H d_a
    for the rays d = (q, -1).  ransac=dict(threshold=, hypotheses=, sample=, refits=, min_inliers=, seed=) puts the consensus
    stage of relative_pose in front (sample in 4..16, default 4; min_inliers at least 4, default 8); None: the linear fit on all
    used matches.  pairs, x and obs_info as in relative_pose.
    Returns the dict of relative_pose with `H` (npairs, 3, 3; sigma_2 = 1, the sign under which the points are in front; NaN
    where the pair has none) in place of `r`, `t`: `status` (names among _lib.HOMOGRAPHY_STATES; few_matches: fewer than 4 used
    matches), `match_ptr`, `inliers`, `n_inliers`, `best_hypothesis`, `counts`.  Bad arguments raise ValueError before any device
    call."""
    opts = None if ransac is None else _lib.ransac_opts(ransac, least=4, most=16, least_set=4)
    x, a1, b1, info3, mp = _pair_call_args("homography", nlp, x, pairs, obs_info)
    n = len(a1)
    _lib.set_obs_info(nlp.handle, info3)
    H, status = np.full((n, 3, 3), np.nan), np.zeros(n, dtype=np.uint8)
    inlier, n_in, best = np.zeros(int(mp[-1]), dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    counts, mp2 = np.zeros(len(_lib.HOMOGRAPHY_STATES), dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    _lib.check(_lib.lib().ba_homography(nlp.handle, _lib.ptr(x), n, _lib.ptr(a1), _lib.ptr(b1), None if opts is None else C.byref(opts),
                                        _lib.ptr(H), _lib.ptr(status), _lib.ptr(mp2), _lib.ptr(inlier), _lib.ptr(n_in), _lib.ptr(best),
                                        _lib.ptr(counts)))
    return dict(H=H, status=np.array(_lib.HOMOGRAPHY_STATES)[status], match_ptr=mp2, inliers=inlier != 0, n_inliers=n_in,
                best_hypothesis=best, counts={s: int(c) for s, c in zip(_lib.HOMOGRAPHY_STATES, counts)})


def decompose_homography(nlp, H):
    """The decomposition of homographies H = R + t n' / d (ba_decompose_homography), n independent problems: H (n, 3, 3), its sign
    as given (homography returns the sign under which the points are in front).  Returns (R, t, normal, n_sol, parallax): R
    (n, 4, 3, 3), t (n, 4, 3) in units of the plane distance d, normal (n, 4, 3) in camera a's frame, NaN in the unused slots;
    n_sol (n,) 0 (H not finite), 1 (a rotation: t = 0, normal = 0) or 4, in the order (+), -(+), (-), -(-) of the header;
    parallax (n,) = sigma_1 - sigma_3 at sigma_2 = 1, which is |t| / d.  nlp supplies the device and the stream.  Bad arguments
    raise ValueError before any device call."""
    H = np.ascontiguousarray(H, dtype=np.float64)
    if H.ndim != 3 or H.shape[1:] != (3, 3):
        raise ValueError(f"decompose_homography: H must have shape (n, 3, 3), got {H.shape}")
    n = H.shape[0]
    R, t, normal = np.full((n, 4, 3, 3), np.nan), np.full((n, 4, 3), np.nan), np.full((n, 4, 3), np.nan)
    n_sol, parallax = np.zeros(n, dtype=np.int32), np.full(n, np.nan)
    _lib.check(_lib.lib().ba_decompose_homography(nlp.handle, n, _lib.ptr(H), _lib.ptr(R), _lib.ptr(t), _lib.ptr(normal), _lib.ptr(n_sol),
                                                  _lib.ptr(parallax)))
    return R, t, normal, n_sol, parallax


def homography_pose(nlp, x, pairs, info, *, threshold, obs_info=None):
    """The pose of planar pairs from their homographies (ba_homography_pose).  info: the dict homography returned for the same
    nlp, x, pairs and obs_info (`H`, `status` and `inliers` are read); threshold (pixels, required): the tau of the support count.
    Per pair that is "ok": H is decomposed, and the candidates whose plane lies in front of camera a for more than half of the
    set are kept in solver order, at most two.  Returns a dict: `parallax` (npairs,) = |t| / d; `n_pose` (0..2); `r`, `t`
    (npairs, 2, 3: the rotation vector and the unit translation of each candidate), `normal` (npairs, 2, 3), NaN in the unused
    slots; `support` (npairs, 2): the matches of the pair's whole list that pass the inlier test of relative_pose under the
    candidate, -1 in the unused slots -- off-plane matches tell the two apart, and on a pure plane the counts tie.  A pair
    without a baseline has n_pose = 1 with its r, t NaN and support -1.  Bad arguments raise ValueError before any device call."""
    try:
        tau = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"homography_pose: threshold must be a finite number > 0, got {threshold!r}") from None
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError(f"homography_pose: threshold must be a finite number > 0, got {threshold!r}")
    x, a1, b1, info3, mp = _pair_call_args("homography_pose", nlp, x, pairs, obs_info)
    if not isinstance(info, dict) or any(k not in info for k in ("H", "status", "inliers")):
        raise ValueError("info must be the dict of homography (H, status, inliers are read)")
    n = len(a1)
    H, names = np.ascontiguousarray(info["H"], dtype=np.float64), np.asarray(info["status"])
    inlier = np.ascontiguousarray(np.asarray(info["inliers"]) != 0, dtype=np.uint8)
    if H.shape != (n, 3, 3) or names.shape != (n,):
        raise ValueError(f"info: H must have shape ({n}, 3, 3) and status ({n},), got {H.shape}, {names.shape}")
    if inlier.shape != (int(mp[-1]),):
        raise ValueError(f"info: inliers must hold one entry per match ({int(mp[-1])}), got {inlier.shape}")
    if not np.isin(names, _lib.HOMOGRAPHY_STATES).all():
        raise ValueError(f"info: status must hold names among {', '.join(_lib.HOMOGRAPHY_STATES)}")
    status = np.array([_lib.HOMOGRAPHY_STATES.index(s) for s in names], dtype=np.uint8)
    _lib.set_obs_info(nlp.handle, info3)
    parallax, n_pose = np.full(n, np.nan), np.zeros(n, dtype=np.int32)
    pose, normal, support = np.full((n, 2, 6), np.nan), np.full((n, 2, 3), np.nan), np.full((n, 2), -1, dtype=np.int32)
    _lib.check(_lib.lib().ba_homography_pose(nlp.handle, _lib.ptr(x), n, _lib.ptr(a1), _lib.ptr(b1), _lib.ptr(H), _lib.ptr(status),
                                             _lib.ptr(inlier), tau, _lib.ptr(parallax), _lib.ptr(n_pose), _lib.ptr(pose), _lib.ptr(normal),
                                             _lib.ptr(support)))
    return dict(parallax=parallax, n_pose=n_pose, r=pose[:, :, :3].copy(), t=pose[:, :, 3:].copy(), normal=normal, support=support)


TWO_VIEW_MODELS = ("general", "planar", "rotation", "none")


def two_view(nlp, x, pairs, *, ransac, ratio=0.8, min_parallax=0.05, refine=None, obs_info=None):
    """Which two-view model explains each pair, its pose, and the order in which the pairs can seed a reconstruction.  Runs
    relative_pose_five_point and homography under the same ransac options (sample forced to 5 and 4), then homography_pose with
    the ransac threshold.  With n_E and n_H the sizes of the two consensus sets, `model` is per pair
      "general"   n_H < ratio n_E: the pose of the essential stage (refine=dict(...) as in relative_pose_five_point);
      "planar"    n_H >= ratio n_E and parallax >= min_parallax: r, t of the homography candidate with the larger support, ties
                  to the first with `ambiguous` True; both candidates are in `candidates`;
      "rotation"  n_H >= ratio n_E and parallax < min_parallax: r is valid, t is NaN -- the pair has no baseline and must not
                  seed a reconstruction;
      "none"      neither stage found a consensus.
    ratio and min_parallax are the caller's choices; the defaults are conventions (0.8 is COLMAP's H/E inlier ratio for a
    planar pair), not thresholds measured here.
    Returns a dict: `model`, `r`, `t` (npairs, 3; NaN where there is none), `ambiguous`, `candidates` (the dict of
    homography_pose), `n_general`, `n_planar` (the two set sizes, 0 without a consensus), `parallax`, `normal` (npairs, 3: of the
    chosen planar candidate), `off_plane` (the matches in the essential set that are not in the homography's), `general` and
    `planar` (the dicts of the two stages) and `seed_order`: the indices of the pairs with a translation, general before planar,
    by off_plane and then n_inliers descending, ties by pair index.  Bad arguments raise ValueError before any device call."""
    if ransac is None:
        raise ValueError("two_view: ransac is required (both models are fitted by the consensus stage)")
    _lib.ransac_opts(ransac, least=4, most=16, least_set=4)  # (the keys and the shared ranges, before either stage runs)
    for name, v in (("ratio", ratio), ("min_parallax", min_parallax)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError(f"two_view: {name} must be a finite number >= 0, got {v!r}")
    gen = relative_pose_five_point(nlp, x, pairs, ransac=dict(ransac, sample=5, min_inliers=max(int(ransac.get("min_inliers") or 0), 8)),
                                   obs_info=obs_info, refine=refine)
    pla = homography(nlp, x, pairs, ransac=dict(ransac, sample=4), obs_info=obs_info)
    cand = homography_pose(nlp, x, pairs, pla, threshold=ransac["threshold"], obs_info=obs_info)
    n = len(gen["status"])
    ok_e, ok_h = gen["status"] == "ok", pla["status"] == "ok"
    n_e, n_h = np.where(ok_e, gen["n_inliers"], 0).astype(np.int64), np.where(ok_h, pla["n_inliers"], 0).astype(np.int64)
    mp = gen["match_ptr"]
    off = np.array([int((gen["inliers"][mp[k]:mp[k + 1]] & ~pla["inliers"][mp[k]:mp[k + 1]]).sum()) if ok_e[k] else 0 for k in range(n)],
                   dtype=np.int64)
    model = np.full(n, "none", dtype=object)
    r, t, normal = np.full((n, 3), np.nan), np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    ambiguous = np.zeros(n, dtype=bool)
    for k in range(n):
        explains = ok_h[k] and n_h[k] >= ratio * n_e[k]
        if explains and cand["parallax"][k] < min_parallax:
            model[k] = "rotation"
            r[k] = cand["r"][k, 0]  # (of the first candidate: at no parallax they share the rotation)
        elif explains and cand["n_pose"][k] > 0:
            model[k] = "planar"
            pick = 0
            if cand["n_pose"][k] == 2:
                s0, s1 = cand["support"][k]
                pick, ambiguous[k] = (1 if s1 > s0 else 0), bool(s0 == s1)
            r[k], t[k], normal[k] = cand["r"][k, pick], cand["t"][k, pick], cand["normal"][k, pick]
        elif ok_e[k]:
            model[k] = "general"
            r[k], t[k] = gen["r"][k], gen["t"][k]
    rank = {"general": 0, "planar": 1}
    n_in = np.where(model == "general", n_e, n_h)
    seeds = [k for k in range(n) if model[k] in rank]
    seed_order = np.array(sorted(seeds, key=lambda k: (rank[model[k]], -off[k], -n_in[k], k)), dtype=np.int64)
    return dict(model=model.astype(str), r=r, t=t, ambiguous=ambiguous, candidates=cand, n_general=n_e, n_planar=n_h,
                parallax=cand["parallax"], normal=normal, off_plane=off, general=gen, planar=pla, seed_order=seed_order)


def _view_graph_args(who, pairs, used=None, weights=None, r=None):
    """The arguments of the view-graph entries that need no model, checked (ValueError): (a1, b1, used as bytes or None,
    weights or None, r or None).  A pair of cameras listed twice, in either orientation, is refused."""
    a1, b1 = _lib._pairs(pairs)
    n = len(a1)
    key = np.sort(np.minimum(a1, b1) * (max(int(a1.max()), int(b1.max())) + 1) + np.maximum(a1, b1)) if n else a1
    if n and (key[1:] == key[:-1]).any():
        raise ValueError(f"{who}: a pair of cameras is listed twice")
    if used is not None:
        used = np.asarray(used)
        if used.dtype != np.bool_ or used.shape != (n,):
            raise ValueError(f"{who}: used must be a boolean array of shape ({n},), got dtype {used.dtype}, shape {used.shape}")
        used = np.ascontiguousarray(used, dtype=np.uint8)
    if weights is not None:
        try:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: weights must be numbers") from None
        if weights.shape != (n,) or not np.isfinite(weights).all() or (weights < 0).any():
            raise ValueError(f"{who}: weights must have shape ({n},) and be finite and >= 0")
    if r is not None:
        try:
            r = np.ascontiguousarray(r, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: r must be numbers") from None
        if r.shape != (n, 3):
            raise ValueError(f"{who}: r must have shape ({n}, 3), one rotation vector per pair, got {r.shape}")
    return a1, b1, used, weights, r


def _in_range(who, a1, b1, ncams):
    if a1.size and max(int(a1.max()), int(b1.max())) > int(ncams):
        raise ValueError(f"{who}: pairs: 1-based cameras must lie in 1..{int(ncams)}, got {max(int(a1.max()), int(b1.max()))}")


def _angle(who, key, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {key} (radians) must be a finite number > 0, got {v!r}") from None
    if not (np.isfinite(f) and f > 0):
        raise ValueError(f"{who}: {key} (radians) must be a finite number > 0, got {v!r}")
    return f


def rotation_loops(nlp, pairs, r, *, threshold, used=None):
    """The loop consistency of a view graph (ba_rotation_loops).  pairs (npairs, 2), 1-based cameras; r (npairs, 3): the rotation
    vector of pair (a, b) with R_b = R R_a, the `r` of relative_pose* and two_view.  For every used pair (a, b) and every camera
    c for which (a, c) and (b, c) are both used pairs, the rotation around the triangle should be the identity: returns
    (n_loops, support), the number of triangles of a pair and of those whose angle is <= threshold (radians).  used (npairs,)
    boolean, default "r is finite" (a pair whose r is not finite is never used); an unused pair gets 0, 0.  nlp supplies the
    device, the stream and ncams.  Bad arguments, a pair listed twice among them, raise ValueError before any device call."""
    tau = _angle("rotation_loops", "threshold", threshold)
    a1, b1, used, _, r = _view_graph_args("rotation_loops", pairs, used=used, r=r)
    _in_range("rotation_loops", a1, b1, nlp.ncams)
    n = len(a1)
    n_loops, support = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib().ba_rotation_loops(nlp.handle, n, _lib.ptr(a1), _lib.ptr(b1), _lib.ptr(r), None if used is None else _lib.ptr(used),
                                            tau, _lib.ptr(n_loops), _lib.ptr(support)))
    return n_loops, support


def view_graph_forest(ncams, pairs, *, used=None, support=None, weights=None, fixed_cameras=None):
    """The maximum spanning forest of a view graph (ba_view_graph_forest; host only, no device): the used pairs under the total
    order `support` descending, `weights` descending, pair index ascending, under which the forest is unique.  The root of a
    component is its lowest fixed camera where it has one, else the camera with the largest sum of the weights of its used
    pairs, ties to the lowest index.  Returns a dict: `component` (ncams,: the components numbered in the order of their lowest
    camera, -1 for a camera without a used pair), `parent_pair` (ncams,: the 0-based pair to the parent, -1 for roots and cameras
    outside the graph), `order` (the 1-based cameras breadth first from the roots, component after component, neighbours
    ascending), `roots` (1-based, one per component), `n_components`.  Bad arguments raise ValueError."""
    who = "view_graph_forest"
    if not isinstance(ncams, (int, np.integer)) or isinstance(ncams, (bool, np.bool_)) or ncams < 0:
        raise ValueError(f"{who}: ncams must be an integer >= 0, got {ncams!r}")
    ncams = int(ncams)
    a1, b1, used, weights, _ = _view_graph_args(who, pairs, used=used, weights=weights)
    _in_range(who, a1, b1, ncams)
    n = len(a1)
    if support is not None:
        support = np.asarray(support)
        if support.shape != (n,) or not np.issubdtype(support.dtype, np.integer):
            raise ValueError(f"{who}: support must be an integer array of shape ({n},), got dtype {support.dtype}, shape {support.shape}")
        support = np.ascontiguousarray(support, dtype=np.int32)
    fixed = None if fixed_cameras is None else np.ascontiguousarray(_lib._fixed_set(fixed_cameras, ncams, "fixed_cameras"), dtype=np.uint8)
    component, parent, order, roots = (np.zeros(ncams, dtype=np.int32), np.zeros(ncams, dtype=np.int64), np.zeros(ncams, dtype=np.int64),
                                       np.zeros(ncams, dtype=np.int64))
    n_order, n_comp = C.c_int64(0), C.c_int64(0)
    opt = lambda a: None if a is None else _lib.ptr(a)  # noqa: E731
    _lib.check(_lib.lib().ba_view_graph_forest(ncams, n, _lib.ptr(a1), _lib.ptr(b1), opt(used), opt(support), opt(weights), opt(fixed),
                                               _lib.ptr(component), _lib.ptr(parent), _lib.ptr(order), C.byref(n_order), C.byref(n_comp),
                                               _lib.ptr(roots)))
    return dict(component=component, parent_pair=parent, order=order[:n_order.value].copy(), roots=roots[:n_comp.value].copy(),
                n_components=n_comp.value)


LOOPS_KEYS = ("threshold", "min_support")


def _rotavg_opts(loops, loss, f_scale, damping, max_sweeps, xtol):
    """RotavgOpts of the options of average_rotations, or ValueError"""
    who = "average_rotations"
    o = _lib.RotavgOpts()
    loss = "linear" if loss is None else loss
    if not isinstance(loss, str) or loss not in _lib.LOSSES:
        raise ValueError(f"{who}: loss must be one of {', '.join(_lib.LOSSES)}, got {loss!r}")
    o.loss = _lib.LOSSES[loss]
    if o.loss != 0 and f_scale is None:
        raise ValueError(f"{who}: f_scale (radians) is required under the loss {loss!r}")
    o.f_scale = 1.0 if f_scale is None else _angle(who, "f_scale", f_scale)
    d = 0.8 if damping is None else _opt_float(damping, f"{who}: damping")
    if not 0 < d <= 1:
        raise ValueError(f"{who}: damping must lie in (0, 1], got {damping!r}")
    o.damping = d
    if max_sweeps is None:
        max_sweeps = 1000
    if not isinstance(max_sweeps, (int, np.integer)) or isinstance(max_sweeps, (bool, np.bool_)) or not 1 <= max_sweeps <= 100000:
        raise ValueError(f"{who}: max_sweeps must be an integer in 1..100000 (or None), got {max_sweeps!r}")
    o.max_sweeps = int(max_sweeps)
    o.xtol = 1e-6 if xtol is None else _opt_float(xtol, f"{who}: xtol")
    o.loops = 0
    if loops is not None:
        if not isinstance(loops, dict) or any(k not in LOOPS_KEYS for k in loops) or "threshold" not in loops:
            raise ValueError(f"{who}: loops must be a dict with the keys {', '.join(LOOPS_KEYS)} (threshold is required), got {loops!r}")
        o.loops, o.loop_threshold = 1, _angle(who, "loops: threshold", loops["threshold"])
        ms = loops.get("min_support", 1)
        if not isinstance(ms, (int, np.integer)) or isinstance(ms, (bool, np.bool_)) or ms < 1:
            raise ValueError(f"{who}: loops: min_support must be an integer >= 1, got {ms!r}")
        o.min_support = int(ms)
    return o


def average_rotations(nlp, pairs, r, *, weights=None, used=None, loops=None, r0=None, fixed_cameras=None, loss=None, f_scale=None,
                      damping=None, max_sweeps=None, xtol=None):
    """Robust rotation averaging over a view graph (ba_average_rotations): the absolute rotation of every camera from all pairs
    at once.  pairs (npairs, 2), 1-based cameras; r (npairs, 3): the rotation vector of pair (a, b) with R_b = R R_a, the `r` of
    relative_pose* and two_view.  All angles are radians.
    weights (npairs,) >= 0, default 1 (n_inliers is the natural choice).  used (npairs,) boolean, default "r is finite".
    loops=dict(threshold=, min_support=1): rotation_loops first; a used pair with triangles of which fewer than min_support
    close is dropped (a pair without a triangle cannot be checked and is kept), and the support becomes the first key of the
    spanning forest.  loss: a name of LOSSES (default linear) with f_scale = c in radians, required unless the loss is linear.
    damping in (0, 1], default 0.8; max_sweeps default 1000, at most 100000; xtol default 1e-6, <= 0 runs exactly max_sweeps.
    r0 (ncams, 3): the start, finite for every camera with a used pair -- a warm start, or with fixed_cameras (1-based or
    boolean; held at r0, which is then required) a registration against an earlier solve.  Without r0 the start is composed
    along the maximum spanning forest of the kept pairs from R = I at each root.
    The sweeps update all cameras at once: each moves by `damping` times the weighted mean of the rotation vectors that its
    kept pairs ask for, the weights w rho'(theta^2 / c^2).  The host reads the largest step after every 8 sweeps and stops
    after the first batch that holds a sweep with a step <= xtol.  The gauge is free during the sweeps; afterwards every
    component without a fixed camera is turned so that its root is back at its start.  The rotations of different components
    are unrelated to each other.
    Returns a dict: `r` (ncams, 3; NaN for a camera without a kept pair), `status` (names among _lib.ROTAVG_STATES: "fixed" for
    a held camera, "root" for the root of a component without one), `component`, `kept` (npairs,), `n_loops` and `support`
    (with loops), `residual` (npairs,: the angle of R_k R_a R_b' for every pair with a finite r inside one component, else NaN:
    a dropped pair can be re-admitted by it), `edge_weight` (rho' on kept pairs, else 0), `sweeps`, `delta` (sweeps,),
    `cost_before`, `cost_after` (half the sum of w c^2 rho over the kept pairs), `counts`.  nlp supplies the device, the stream
    and ncams.  Bad arguments raise ValueError before any device call."""
    who = "average_rotations"
    o = _rotavg_opts(loops, loss, f_scale, damping, max_sweeps, xtol)
    a1, b1, used, weights, r = _view_graph_args(who, pairs, used=used, weights=weights, r=r)
    if fixed_cameras is not None:
        _lib._fixed_set(fixed_cameras, None, "fixed_cameras")
        if r0 is None and np.asarray(fixed_cameras).size and np.asarray(fixed_cameras).any():
            raise ValueError(f"{who}: fixed_cameras are held at r0, which is required with them")
    if r0 is not None:
        try:
            r0 = np.ascontiguousarray(r0, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: r0 must be numbers") from None
        if r0.ndim != 2 or r0.shape[1] != 3:
            raise ValueError(f"{who}: r0 must have shape (ncams, 3), got {r0.shape}")
        in_use = np.isfinite(r).all(axis=1) if used is None else (used != 0) & np.isfinite(r).all(axis=1)
        touched = np.unique(np.concatenate([a1[in_use], b1[in_use]])) - 1
        if touched.size and (touched.max() >= len(r0) or not np.isfinite(r0[touched]).all()):
            raise ValueError(f"{who}: r0 must be finite for every camera that has a used pair")
    ncams, n = nlp.ncams, len(a1)
    _in_range(who, a1, b1, ncams)
    if r0 is not None and r0.shape != (ncams, 3):
        raise ValueError(f"{who}: r0 must have shape ({ncams}, 3), got {r0.shape}")
    fixed = None if fixed_cameras is None else np.ascontiguousarray(_lib._fixed_set(fixed_cameras, ncams, "fixed_cameras"), dtype=np.uint8)
    out_r, status, component = np.full((ncams, 3), np.nan), np.zeros(ncams, dtype=np.uint8), np.zeros(ncams, dtype=np.int32)
    kept, n_loops, support = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    residual, edge_weight = np.full(n, np.nan), np.zeros(n)
    sweeps, delta, cost = C.c_int32(0), np.zeros(o.max_sweeps), np.zeros(2)
    counts = np.zeros(len(_lib.ROTAVG_STATES), dtype=np.int64)
    opt = lambda a: None if a is None else _lib.ptr(a)  # noqa: E731
    _lib.check(_lib.lib().ba_average_rotations(nlp.handle, n, _lib.ptr(a1), _lib.ptr(b1), _lib.ptr(r), opt(weights), opt(used), opt(r0),
                                               opt(fixed), C.byref(o), _lib.ptr(out_r), _lib.ptr(status), _lib.ptr(component),
                                               _lib.ptr(kept), _lib.ptr(n_loops), _lib.ptr(support), _lib.ptr(residual),
                                               _lib.ptr(edge_weight), C.byref(sweeps), _lib.ptr(delta), _lib.ptr(cost), _lib.ptr(counts)))
    info = dict(r=out_r, status=np.array(_lib.ROTAVG_STATES)[status], component=component, kept=kept != 0, residual=residual,
                edge_weight=edge_weight, sweeps=sweeps.value, delta=delta[:sweeps.value].copy(), cost_before=float(cost[0]),
                cost_after=float(cost[1]), counts={s: int(c) for s, c in zip(_lib.ROTAVG_STATES, counts)})
    if loops is not None:
        info.update(n_loops=n_loops, support=support)
    return info


def _directions(who, directions, n):
    try:
        d = np.ascontiguousarray(directions, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: directions must be numbers") from None
    if d.shape != (n, 3):
        raise ValueError(f"{who}: directions must have shape ({n}, 3), one baseline direction per pair, got {d.shape}")
    return d


def translation_directions(pairs, t, r_abs):
    """The baseline directions of a view graph in the world frame, on the host: d_k = -R_b' t_k for pair k = (a, b), with the unit
    t of relative_pose* and two_view (P_b = R P_a + t) and r_abs (ncams, 3) the rotation vectors of average_rotations.  d_k points
    from the centre of a to the centre of b.  A pair whose t, or whose camera b's rotation, is not finite gets NaN (such a pair is
    never used by average_translations).  Returns (npairs, 3)."""
    who = "translation_directions"
    a1, b1 = _lib._pairs(pairs)
    try:
        t, r_abs = np.asarray(t, dtype=np.float64), np.asarray(r_abs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: t and r_abs must be numbers") from None
    if t.shape != (len(a1), 3) or r_abs.ndim != 2 or r_abs.shape[1] != 3:
        raise ValueError(f"{who}: t must have shape ({len(a1)}, 3) and r_abs (ncams, 3), got {t.shape}, {r_abs.shape}")
    _in_range(who, a1, b1, len(r_abs))
    from .synthetic import rotation_matrices
    rb = r_abs[b1 - 1]
    ok = np.isfinite(rb).all(axis=1)
    R = rotation_matrices(np.where(ok[:, None], rb, 0.0))
    d = -np.einsum("kji,kj->ki", R, t)
    d[~ok] = np.nan
    return d


def camera_translations(r_abs, centres):
    """T = -R C per camera, the translation of the BAL camera model (P = R X + T), from the rotation vectors r_abs (ncams, 3) and
    the centres (ncams, 3) of average_translations; on the host.  Returns (ncams, 3)."""
    who = "camera_translations"
    try:
        r_abs, centres = np.asarray(r_abs, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: r_abs and centres must be numbers") from None
    if r_abs.ndim != 2 or r_abs.shape[1] != 3 or centres.shape != r_abs.shape:
        raise ValueError(f"{who}: r_abs and centres must both have shape (ncams, 3), got {r_abs.shape}, {centres.shape}")
    from .synthetic import rotation_matrices
    ok = np.isfinite(r_abs).all(axis=1)
    T = -np.einsum("kij,kj->ki", rotation_matrices(np.where(ok[:, None], r_abs, 0.0)), centres)
    T[~ok] = np.nan
    return T


def translation_loops(nlp, pairs, directions, *, used=None, threshold):
    """The loop consistency of the baseline directions of a view graph (ba_translation_loops).  pairs (npairs, 2), 1-based
    cameras; directions (npairs, 3): the direction from the centre of a to the centre of b in the world frame
    (translation_directions), normalised on the device.  For every used pair (a, b) and every camera c for which (a, c) and
    (c, b) are both used pairs, the direction a -> b lies on the shorter great-circle arc between the directions a -> c and
    c -> b: returns (n_loops, support), the number of triangles of a pair that can be checked (a triangle whose other two
    directions are opposite cannot) and of those whose distance to the arc is <= threshold (radians).  used (npairs,) boolean,
    default "the direction is finite with a norm >= 1e-12" (another pair is never used); an unused pair gets 0, 0.  nlp supplies
    the device, the stream and ncams.  Bad arguments, a pair listed twice among them, raise ValueError before any device call."""
    who = "translation_loops"
    tau = _angle(who, "threshold", threshold)
    a1, b1, used, _, _ = _view_graph_args(who, pairs, used=used)
    d = _directions(who, directions, len(a1))
    _in_range(who, a1, b1, nlp.ncams)
    n = len(a1)
    n_loops, support = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib().ba_translation_loops(nlp.handle, n, _lib.ptr(a1), _lib.ptr(b1), _lib.ptr(d), None if used is None else _lib.ptr(used),
                                               tau, _lib.ptr(n_loops), _lib.ptr(support)))
    return n_loops, support


TRANSLATION_LOOPS_KEYS = ("threshold", "min_support", "min_ratio")


def _count(who, key, v, lo, hi):
    if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or not lo <= v <= hi:
        raise ValueError(f"{who}: {key} must be an integer in {lo}..{hi} (or None), got {v!r}")
    return int(v)


def _transavg_opts(loops, loss, f_scale, max_iterations, ftol, cg_tol, max_cg):
    """TransavgOpts of the options of average_translations, or ValueError"""
    who = "average_translations"
    o = _lib.TransavgOpts()
    loss = "linear" if loss is None else loss
    if not isinstance(loss, str) or loss not in _lib.LOSSES:
        raise ValueError(f"{who}: loss must be one of {', '.join(_lib.LOSSES)}, got {loss!r}")
    o.loss = _lib.LOSSES[loss]
    if o.loss != 0 and f_scale is None:
        raise ValueError(f"{who}: f_scale (chordal units) is required under the loss {loss!r}")
    o.f_scale = 1.0 if f_scale is None else _angle(who, "f_scale", f_scale)
    o.max_iterations = 50 if max_iterations is None else _count(who, "max_iterations", max_iterations, 1, 100000)
    o.max_cg = 500 if max_cg is None else _count(who, "max_cg", max_cg, 1, 100000)
    for key, v, default in (("ftol", ftol, 1e-10), ("cg_tol", cg_tol, 1e-6)):
        f = default if v is None else _opt_float(v, f"{who}: {key}")
        if not f > 0:
            raise ValueError(f"{who}: {key} must be a finite number > 0 (or None), got {v!r}")
        setattr(o, key, f)
    o.lambda0 = 1e-3
    o.loops = 0
    if loops is not None:
        if not isinstance(loops, dict) or any(k not in TRANSLATION_LOOPS_KEYS for k in loops) or "threshold" not in loops:
            raise ValueError(f"{who}: loops must be a dict with the keys {', '.join(TRANSLATION_LOOPS_KEYS)} (threshold is required), "
                             f"got {loops!r}")
        o.loops, o.loop_threshold = 1, _angle(who, "loops: threshold", loops["threshold"])
        o.min_support = _count(who, "loops: min_support", loops.get("min_support", 1), 1, 2 ** 31 - 1)
        ratio = _opt_float(loops.get("min_ratio", 0.34), f"{who}: loops: min_ratio")
        if ratio is None or not 0 <= ratio <= 1:
            raise ValueError(f"{who}: loops: min_ratio must lie in [0, 1] (0: off), got {loops.get('min_ratio')!r}")
        o.min_ratio = ratio
    return o


def average_translations(nlp, pairs, directions, *, weights=None, used=None, loops=None, c0=None, fixed_cameras=None, loss=None,
                         f_scale=None, max_iterations=None, ftol=None, cg_tol=None, max_cg=None):
    """Robust translation averaging over a view graph (ba_average_translations): the centre of every camera from the baseline
    directions of all pairs at once, up to a shift and a scale per component.  pairs (npairs, 2), 1-based cameras; directions
    (npairs, 3): the direction from the centre of a to the centre of b in the world frame (translation_directions), normalised
    on the device.
    weights (npairs,) >= 0, default 1.  used (npairs,) boolean, default "the direction is finite with a norm >= 1e-12".
    loops=dict(threshold=, min_support=1, min_ratio=0.34): translation_loops first; a used pair with checked triangles is
    dropped if fewer than min_support, or fewer than min_ratio of them, close (a pair without a checked triangle is kept), and
    the support becomes the first key of the spanning forest.  loss: a name of LOSSES (default linear) on the chord
    |u^ - d|, with f_scale = c in its units (about radians for small angles), required unless the loss is linear.
    c0 (ncams, 3): the start, finite for every camera with a used pair -- a warm start, or with fixed_cameras (1-based or
    boolean; held at c0, which is then required) a registration against an earlier solve.  Without c0 the root of every
    component is at 0 and the other cameras follow along the maximum spanning forest of the kept pairs with baselines of length 1.
    The solve is Levenberg-Marquardt on F = sum w c^2 rho(|u^_k - d_k|^2 / c^2) / 2, u_k = C_b - C_a: every iteration solves
    (H + lambda diag H) delta = -g on the device by conjugate gradients under the cameras' 3 x 3 diagonal blocks, to
    |r|_M <= cg_tol |r0|_M (default 1e-6) or max_cg iterations (default 500); a trial is accepted iff F decreases
    (lambda / 3, else 4 lambda); it stops when F changes by at most ftol F (default 1e-10), after max_iterations (default 50) or
    when lambda passes 1e8.  Afterwards every component without a fixed camera is moved so that its root is back at its start
    and scaled about it so that the mean length of its kept baselines is that of the start.  The centres of different
    components are unrelated to each other.
    Returns a dict: `c` (ncams, 3; NaN for a camera without a kept pair), `status` (names among _lib.TRANSAVG_STATES),
    `component`, `kept` (npairs,), `n_loops` and `support` (with loops), `residual` (npairs,: the angle between C_b - C_a and the
    direction for every pair with a usable direction inside one component, else NaN: a dropped pair can be re-admitted by it),
    `edge_weight` (rho' on kept pairs, else 0), `iterations`, `cg_iterations` (their total), `trace` (iterations, 4: the cost of
    the trial, lambda, the conjugate-gradient iterations, accepted), `cost_before`, `cost_after`, `counts`.  nlp supplies the
    device, the stream and ncams.  Bad arguments raise ValueError before any device call."""
    who = "average_translations"
    o = _transavg_opts(loops, loss, f_scale, max_iterations, ftol, cg_tol, max_cg)
    a1, b1, used, weights, _ = _view_graph_args(who, pairs, used=used, weights=weights)
    d = _directions(who, directions, len(a1))
    if fixed_cameras is not None:
        _lib._fixed_set(fixed_cameras, None, "fixed_cameras")
        if c0 is None and np.asarray(fixed_cameras).size and np.asarray(fixed_cameras).any():
            raise ValueError(f"{who}: fixed_cameras are held at c0, which is required with them")
    if c0 is not None:
        try:
            c0 = np.ascontiguousarray(c0, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: c0 must be numbers") from None
        if c0.ndim != 2 or c0.shape[1] != 3:
            raise ValueError(f"{who}: c0 must have shape (ncams, 3), got {c0.shape}")
        with np.errstate(invalid="ignore", over="ignore"):
            usable = np.isfinite(d).all(axis=1) & (np.sqrt((d * d).sum(axis=1)) >= 1e-12)
        in_use = usable if used is None else (used != 0) & usable
        touched = np.unique(np.concatenate([a1[in_use], b1[in_use]])) - 1
        if touched.size and (touched.max() >= len(c0) or not np.isfinite(c0[touched]).all()):
            raise ValueError(f"{who}: c0 must be finite for every camera that has a used pair")
    ncams, n = nlp.ncams, len(a1)
    _in_range(who, a1, b1, ncams)
    if c0 is not None and c0.shape != (ncams, 3):
        raise ValueError(f"{who}: c0 must have shape ({ncams}, 3), got {c0.shape}")
    fixed = None if fixed_cameras is None else np.ascontiguousarray(_lib._fixed_set(fixed_cameras, ncams, "fixed_cameras"), dtype=np.uint8)
    out_c, status, component = np.full((ncams, 3), np.nan), np.zeros(ncams, dtype=np.uint8), np.zeros(ncams, dtype=np.int32)
    kept, n_loops, support = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    residual, edge_weight = np.full(n, np.nan), np.zeros(n)
    its, cg, trace, cost = C.c_int32(0), C.c_int32(0), np.zeros((o.max_iterations, 4)), np.zeros(2)
    counts = np.zeros(len(_lib.TRANSAVG_STATES), dtype=np.int64)
    opt = lambda a: None if a is None else _lib.ptr(a)  # noqa: E731
    _lib.check(_lib.lib().ba_average_translations(nlp.handle, n, _lib.ptr(a1), _lib.ptr(b1), _lib.ptr(d), opt(weights), opt(used), opt(c0),
                                                  opt(fixed), C.byref(o), _lib.ptr(out_c), _lib.ptr(status), _lib.ptr(component),
                                                  _lib.ptr(kept), _lib.ptr(n_loops), _lib.ptr(support), _lib.ptr(residual),
                                                  _lib.ptr(edge_weight), C.byref(its), C.byref(cg), _lib.ptr(trace), _lib.ptr(cost),
                                                  _lib.ptr(counts)))
    info = dict(c=out_c, status=np.array(_lib.TRANSAVG_STATES)[status], component=component, kept=kept != 0, residual=residual,
                edge_weight=edge_weight, iterations=its.value, cg_iterations=cg.value, trace=trace[:its.value].copy(),
                cost_before=float(cost[0]), cost_after=float(cost[1]), counts={s: int(c) for s, c in zip(_lib.TRANSAVG_STATES, counts)})
    if loops is not None:
        info.update(n_loops=n_loops, support=support)
    return info


def similarity(nlp, src, dst, *, offsets=None, used=None, ransac=None, scale=True):
    """Robust similarity alignment of 3D-3D correspondences (ba_similarity): (s, R, t) with dst ~ s R src + t, which brings a
    reconstruction into the frame of its ground control, of GPS centres or of another model.  src, dst (n, 3); offsets
    (nprob + 1,), 0-based, starting at 0 and not decreasing with offsets[-1] = n: problem k owns the rows offsets[k] ..
    offsets[k + 1] (None: one problem of all rows) -- many problems in one call merge sub-models or the components of a view
    graph.  used (n,) boolean, default all; a row with a number that is not finite is never used (the NaN centres of
    average_translations drop out this way).
    ransac=dict(threshold=, hypotheses=, sample=, refits=, min_inliers=, seed=) puts the consensus stage of refine_cameras in front
    (threshold in the units of dst; sample in 3..16, default 3; min_inliers at least 3, default max(sample, 3)): minimal samples,
    the winner by its inlier count |s R src + t - dst| <= threshold, refits on the set; None: the fit on all used rows.
    scale=False fixes s = 1 (a rigid alignment).
    Returns a dict: `s` (nprob,), `r` (nprob, 3: the rotation vector of R), `t` (nprob, 3), all NaN where the problem is not ok;
    `status` (names among _lib.SIMILARITY_STATES; few_rows: fewer than 3 used rows; degenerate: collinear rows), `inliers` (n,)
    bool, `n_inliers`, `best_hypothesis` (-1: none), `rms` (of the residual over the final set; NaN where not ok), `counts`
    (problems per state).  _lib.apply_similarity moves x by (s, r, t).  nlp supplies the device, the stream and the buffers: no
    model data is read.  Bad arguments raise ValueError before any device call."""
    who = "similarity"
    opts = None if ransac is None else _lib.ransac_opts(ransac, least=3, most=16, least_set=3)
    if not isinstance(scale, (bool, np.bool_)):
        raise ValueError(f"{who}: scale must be True or False, got {scale!r}")
    try:
        src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: src and dst must be numbers") from None
    if src.ndim != 2 or src.shape[1] != 3 or dst.shape != src.shape:
        raise ValueError(f"{who}: src and dst must have one shape (n, 3), got {src.shape} and {dst.shape}")
    n = src.shape[0]
    if offsets is None:
        ptr = np.array([0, n], dtype=np.int64)
    else:
        ptr = np.asarray(offsets)
        if ptr.ndim != 1 or ptr.size < 1 or not np.issubdtype(ptr.dtype, np.integer):
            raise ValueError(f"{who}: offsets must be an integer array of shape (nprob + 1,), got dtype {ptr.dtype}, shape {ptr.shape}")
        ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        if ptr[0] != 0 or ptr[-1] != n or (np.diff(ptr) < 0).any():
            raise ValueError(f"{who}: offsets are 0-based, start at 0, do not decrease and end at n = {n}, got {ptr[0]} .. {ptr[-1]}")
    if used is not None:
        used = np.asarray(used)
        if used.shape != (n,) or used.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"{who}: used must be a boolean array of shape ({n},), got dtype {used.dtype}, shape {used.shape}")
        used = np.ascontiguousarray(used != 0, dtype=np.uint8)
    nprob = len(ptr) - 1
    sim, status = np.full((nprob, 7), np.nan), np.zeros(nprob, dtype=np.uint8)
    inlier, n_in, best = np.zeros(n, dtype=np.uint8), np.zeros(nprob, dtype=np.int32), np.zeros(nprob, dtype=np.int32)
    rms, counts = np.full(nprob, np.nan), np.zeros(len(_lib.SIMILARITY_STATES), dtype=np.int64)
    _lib.check(_lib.lib().ba_similarity(nlp.handle, nprob, _lib.ptr(ptr), _lib.ptr(src), _lib.ptr(dst), None if used is None else _lib.ptr(used),
                                        None if opts is None else C.byref(opts), 1 if scale else 0, _lib.ptr(sim), _lib.ptr(status),
                                        _lib.ptr(inlier), _lib.ptr(n_in), _lib.ptr(best), _lib.ptr(rms), _lib.ptr(counts)))
    return dict(s=sim[:, 0].copy(), r=sim[:, 1:4].copy(), t=sim[:, 4:7].copy(), status=np.array(_lib.SIMILARITY_STATES)[status],
                inliers=inlier != 0, n_inliers=n_in, best_hypothesis=best, rms=rms,
                counts={s: int(c) for s, c in zip(_lib.SIMILARITY_STATES, counts)})


def schur_pattern(nlp):
    """(tile_fill, flop_fill, sparse_schedule) of the reduced camera system of a handle that has run a direct solve
    (ba_lm_schur_pattern): the fraction of the lower 128 x 128 tiles in the factor's pattern, the fraction of the dense
    factorisation's trailing-update tiles that pattern needs, and whether the block-sparse list schedule is in use."""
    tf, ff, sp = C.c_double(0), C.c_double(0), C.c_int(0)
    _lib.check(_lib.lib().ba_lm_schur_pattern(nlp.handle, C.byref(tf), C.byref(ff), C.byref(sp)))
    return tf.value, ff.value, bool(sp.value)


def set_ordering(nlp, perm):
    """Camera ordering of the handle's next direct solves outside Levenberg_Marquardt (lm_step): "AMD", "Metis", "natural"."""
    _lib.check(_lib.lib().ba_lm_set_ordering(nlp.handle, _lib.ORDERINGS[_sym(perm)]))


def schur_ordering_used(nlp):
    """(perm1, name): the camera sequence of the reduced camera system of a handle that has run a direct solve (perm1[k] =
    1-based camera at block row k of S) and the name of the candidate sequence that won (ba_lm_schur_ordering)."""
    perm = np.zeros(nlp.ncams, dtype=np.int64)
    name = C.c_char_p()
    _lib.check(_lib.lib().ba_lm_schur_ordering(nlp.handle, _lib.ptr(perm), C.byref(name)))
    return perm, name.value.decode()


def schur_memory(nlp):
    """(tiles_full, tiles_held, tiles_staging) of a handle that has run a direct solve (ba_lm_schur_memory): the 128 x 128
    tiles of the whole reduced camera matrix, what this handle holds of it, and its staging buffer (distributed runs)."""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().ba_lm_schur_memory(nlp.handle, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value
