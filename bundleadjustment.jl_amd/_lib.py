"""ctypes binding of libba_hip.so (include/ba_hip.h).  There is no CPU fallback: if the HIP library is
missing or no MI355X is visible, every compute entry raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libba_hip.so")

BA_OK = 0
ERR_NAMES = {1: "BA_ERR_ARG", 2: "BA_ERR_HIP", 3: "BA_ERR_IO", 4: "BA_ERR_ZERO_PIVOT", 5: "BA_ERR_NAN_STEP",
             6: "BA_ERR_COMM"}
STATUS = {-1: "unknown", 0: "small_step", 1: "first_order", 2: "small_residual", 3: "acceptable", 4: "neg_pred",
          5: "exception", 6: "max_iter"}


class BAError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class BAArgError(BAError, ValueError):
    """BA_ERR_ARG: an argument the library refuses (also a ValueError)."""


class SQDException(BAError):
    """Zero pivot in the LDL' factorisation (reference: src/ldl_aux.jl:45-47,199)."""


class LMOpts(C.Structure):
    _fields_ = [("variant", C.c_int), ("facto", C.c_int), ("normalize", C.c_int), ("linesearch", C.c_int),
                ("facto_type", C.c_int), ("ite_max", C.c_int), ("verbose", C.c_int), ("x_f32", C.c_int),
                ("restol", C.c_double), ("satol", C.c_double), ("srtol", C.c_double), ("oatol", C.c_double),
                ("ortol", C.c_double), ("atol", C.c_double), ("rtol", C.c_double),
                ("nu_d", C.c_double), ("nu_m", C.c_double), ("lam", C.c_double), ("delta_d", C.c_double),
                ("max_time", C.c_double), ("pcg_tol", C.c_double), ("pcg_max_iter", C.c_int), ("perm", C.c_int)]


class LMStats(C.Structure):
    _fields_ = [("status", C.c_int), ("iter", C.c_int), ("n_accepted", C.c_int), ("n_rejected", C.c_int),
                ("n_residual", C.c_int), ("n_jacobian", C.c_int), ("n_factor", C.c_int), ("n_cg", C.c_int),
                ("objective", C.c_double), ("dual_feas", C.c_double), ("lambda_final", C.c_double),
                ("elapsed_s", C.c_double), ("loop_s", C.c_double)]


class RansacOpts(C.Structure):
    """ba_ransac_opts"""
    _fields_ = [("threshold", C.c_double), ("hypotheses", C.c_int), ("sample", C.c_int), ("refits", C.c_int),
                ("min_inliers", C.c_int), ("seed", C.c_uint64)]


class PairRefineOpts(C.Structure):
    """ba_pair_refine_opts"""
    _fields_ = [("max_iter", C.c_int), ("xtol", C.c_double), ("lambda0", C.c_double), ("loss", C.c_int), ("f_scale", C.c_double),
                ("threshold", C.c_double), ("rounds", C.c_int)]


class RotavgOpts(C.Structure):
    """ba_rotavg_opts"""
    _fields_ = [("loss", C.c_int), ("max_sweeps", C.c_int), ("loops", C.c_int), ("min_support", C.c_int), ("f_scale", C.c_double),
                ("damping", C.c_double), ("xtol", C.c_double), ("loop_threshold", C.c_double)]


class TransavgOpts(C.Structure):
    """ba_transavg_opts"""
    _fields_ = [("loss", C.c_int), ("loops", C.c_int), ("min_support", C.c_int), ("max_iterations", C.c_int), ("max_cg", C.c_int),
                ("f_scale", C.c_double), ("loop_threshold", C.c_double), ("min_ratio", C.c_double), ("ftol", C.c_double),
                ("cg_tol", C.c_double), ("lambda0", C.c_double)]


LOG_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                     C.c_double, C.c_int)
COMM_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
COMM_ALLREDUCE_F64, COMM_REDUCE_F64, COMM_BCAST_BYTES, COMM_REDUCE_F32, COMM_REDUCE_SCATTER_F64, COMM_REDUCE_SCATTER_F32 = 0, 1, 2, 3, 4, 5
COMM_OPS = 6
COMM_OP_NAMES = ("allreduce_f64", "reduce_f64", "bcast_bytes", "reduce_f32", "reduce_scatter_f64", "reduce_scatter_f32")
COMM_ID_BYTES = 128

# every symbol include/ba_hip.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "ba_last_error", "ba_device_count", "ba_device_info", "ba_read_bal_header", "ba_read_bal", "ba_read_bal_f32",
    "ba_problem_create", "ba_problem_destroy", "ba_problem_dims", "ba_residual", "ba_residual_f32",
    "ba_jac_structure", "ba_jac_coord", "ba_jac_coord_f32", "ba_jtr", "ba_residual_dev", "ba_residual_f32_dev",
    "ba_jac_structure_dev", "ba_jac_coord_dev", "ba_jac_coord_f32_dev", "ba_jtr_dev", "ba_dev_malloc", "ba_dev_free",
    "ba_memcpy_h2d", "ba_memcpy_d2h", "ba_memcpy_h2d_on", "ba_memcpy_d2h_on", "ba_synchronize", "ba_lm_solve", "ba_lm_solve_dev", "ba_comm_get_unique_id", "ba_lm_set_comm_rccl",
    "ba_lm_set_comm_hook", "ba_comm_stats", "ba_comm_stats_ops", "ba_dist_layout",
    "ba_lm_step", "ba_lm_step_f32", "ba_lm_step_pcg", "ba_lm_schur_pattern", "ba_lm_schur_memory", "ba_schur_ordering", "ba_lm_set_ordering", "ba_lm_schur_ordering", "ba_lm_set_loss", "ba_lm_get_loss", "ba_robust_eval", "ba_lm_set_fixed", "ba_lm_get_fixed", "ba_lm_set_priors", "ba_lm_get_priors", "ba_prior_eval", "ba_covariance", "ba_profile_enable", "ba_profile_reset", "ba_profile_get", "ba_dense_ldl_solve", "ba_dense_ldl_solve_f32",
    "ba_lm_set_shared_intrinsics", "ba_lm_get_shared_intrinsics", "ba_dense_ldl_solve_multi",
    "ba_lm_set_obs_info", "ba_lm_get_obs_info",
    "ba_refine_points", "ba_refine_points_dev",
    "ba_refine_cameras", "ba_refine_cameras_dev", "ba_resect_cameras", "ba_resect_cameras_dev",
    "ba_ransac_cameras", "ba_ransac_cameras_dev", "ba_ransac_sample",
    "ba_resect_cameras_focal", "ba_resect_cameras_focal_dev", "ba_ransac_cameras_focal", "ba_ransac_cameras_focal_dev",
    "ba_pair_matches", "ba_relative_pose", "ba_relative_pose_five_point", "ba_five_point",
    "ba_ransac_cameras_p3p", "ba_ransac_cameras_p3p_dev", "ba_p3p",
    "ba_refine_relative_pose",
    "ba_ransac_points", "ba_ransac_points_dev",
    "ba_homography", "ba_decompose_homography", "ba_homography_pose",
    "ba_rotation_loops", "ba_view_graph_forest", "ba_average_rotations",
    "ba_translation_loops", "ba_average_translations", "ba_transavg_lm_decide",
    "ba_similarity",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.ba_last_error.restype = C.c_char_p
    vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
    L.ba_device_count.argtypes = [C.POINTER(C.c_int)]
    L.ba_device_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.ba_read_bal_header.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.ba_read_bal.argtypes = [C.c_char_p, i64, i64, i64, vp, vp, vp, vp]
    L.ba_read_bal_f32.argtypes = [C.c_char_p, i64, i64, i64, vp, vp, vp, vp]
    L.ba_problem_create.argtypes = [C.c_int, i64, i64, i64, vp, vp, vp, C.POINTER(vp)]
    L.ba_problem_destroy.argtypes = [vp]
    L.ba_problem_destroy.restype = None
    L.ba_problem_dims.argtypes = [vp] + [C.POINTER(i64)] * 6
    for name in ("ba_residual", "ba_residual_f32", "ba_jac_structure", "ba_jac_coord", "ba_jac_coord_f32"):
        getattr(L, name).argtypes = [vp, vp, vp]
    L.ba_jtr.argtypes = [vp, vp, vp, vp]
    for name in ("ba_residual_dev", "ba_residual_f32_dev", "ba_jac_structure_dev", "ba_jac_coord_dev",
                 "ba_jac_coord_f32_dev"):
        getattr(L, name).argtypes = [vp, vp, vp, vp]
    L.ba_jtr_dev.argtypes = [vp, vp, vp, vp, vp]
    L.ba_dev_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.ba_dev_free.argtypes = [vp, vp]
    L.ba_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.ba_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.ba_memcpy_h2d_on.argtypes = [vp, vp, vp, vp, C.c_size_t]
    L.ba_memcpy_d2h_on.argtypes = [vp, vp, vp, vp, C.c_size_t]
    L.ba_synchronize.argtypes = [vp]
    L.ba_lm_solve.argtypes = [vp, C.POINTER(LMOpts), vp, C.POINTER(LMStats), LOG_CB, vp]
    L.ba_lm_solve_dev.argtypes = [vp, C.POINTER(LMOpts), vp, C.POINTER(LMStats), LOG_CB, vp]
    L.ba_comm_get_unique_id.argtypes = [vp]
    L.ba_lm_set_comm_rccl.argtypes = [vp, C.c_int, C.c_int, vp]
    L.ba_lm_set_comm_hook.argtypes = [vp, C.c_int, C.c_int, COMM_CB, vp]
    L.ba_comm_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.ba_comm_stats_ops.argtypes = [vp, vp, vp]
    L.ba_dist_layout.argtypes = [i64, C.c_int, vp, vp]
    L.ba_lm_step.argtypes = [vp, vp, f64, vp, C.POINTER(f64), vp]
    L.ba_lm_step_f32.argtypes = [vp, vp, f64, vp, C.POINTER(f64), vp]
    L.ba_lm_step_pcg.argtypes = [vp, vp, f64, f64, C.c_int, vp, C.POINTER(f64), vp, C.POINTER(C.c_int)]
    L.ba_lm_schur_pattern.argtypes = [vp, C.POINTER(f64), C.POINTER(f64), C.POINTER(C.c_int)]
    L.ba_lm_schur_memory.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.ba_schur_ordering.argtypes = [i64, i64, i64, vp, vp, C.c_int, vp, C.POINTER(f64), C.POINTER(f64), C.POINTER(f64)]
    L.ba_lm_set_ordering.argtypes = [vp, C.c_int]
    L.ba_lm_schur_ordering.argtypes = [vp, vp, C.POINTER(C.c_char_p)]
    L.ba_lm_set_loss.argtypes = [vp, C.c_int, f64]
    L.ba_lm_get_loss.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(f64)]
    L.ba_robust_eval.argtypes = [vp, vp, vp, C.POINTER(f64)]
    L.ba_lm_set_fixed.argtypes = [vp, vp, vp]
    L.ba_lm_get_fixed.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.ba_lm_set_priors.argtypes = [vp] + [i64, vp, vp, vp] * 3
    L.ba_lm_get_priors.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.ba_prior_eval.argtypes = [vp, vp, C.POINTER(f64), vp, vp, vp]
    L.ba_covariance.argtypes = [vp, vp, f64, f64, vp, vp, C.POINTER(f64)]
    L.ba_profile_enable.argtypes = [vp, C.c_int]
    L.ba_profile_reset.argtypes = [vp]
    L.ba_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(f64), C.POINTER(i64), C.POINTER(C.c_int)]
    L.ba_dense_ldl_solve.argtypes = [C.c_int, i64, vp, vp, vp, C.POINTER(f64)]
    L.ba_dense_ldl_solve_f32.argtypes = [C.c_int, i64, vp, vp, vp, C.POINTER(f64)]
    L.ba_lm_set_shared_intrinsics.argtypes = [vp, vp]
    L.ba_lm_get_shared_intrinsics.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(i64)]
    L.ba_dense_ldl_solve_multi.argtypes = [C.c_int, i64, vp, C.c_int, vp, vp, C.POINTER(f64)]
    L.ba_lm_set_obs_info.argtypes = [vp, vp]
    L.ba_lm_get_obs_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.ba_refine_points.argtypes = [vp, vp, C.c_int, C.c_int, f64, f64, vp, vp, vp, C.POINTER(C.c_int)]
    L.ba_refine_points_dev.argtypes = [vp, vp, C.c_int, C.c_int, f64, f64, vp, vp, vp, C.POINTER(C.c_int), vp]
    L.ba_refine_cameras.argtypes = [vp, vp, C.c_int, f64, f64, vp, vp, vp, C.POINTER(C.c_int)]
    L.ba_refine_cameras_dev.argtypes = [vp, vp, C.c_int, f64, f64, vp, vp, vp, C.POINTER(C.c_int), vp]
    L.ba_resect_cameras.argtypes = L.ba_refine_cameras.argtypes
    L.ba_resect_cameras_dev.argtypes = L.ba_refine_cameras_dev.argtypes
    L.ba_ransac_cameras.argtypes = [vp, vp, C.POINTER(RansacOpts), C.c_int, f64, f64, vp, vp, vp, C.POINTER(C.c_int), vp, vp, vp]
    L.ba_ransac_cameras_dev.argtypes = L.ba_ransac_cameras.argtypes + [vp]
    L.ba_resect_cameras_focal.argtypes = L.ba_resect_cameras.argtypes
    L.ba_resect_cameras_focal_dev.argtypes = L.ba_resect_cameras_dev.argtypes
    L.ba_ransac_cameras_focal.argtypes = L.ba_ransac_cameras.argtypes
    L.ba_ransac_cameras_focal_dev.argtypes = L.ba_ransac_cameras_dev.argtypes
    L.ba_ransac_sample.argtypes = [C.c_uint64, C.c_int, i64, vp, C.c_int, vp, C.POINTER(C.c_int)]
    L.ba_pair_matches.argtypes = [i64, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp]
    L.ba_relative_pose.argtypes = [vp, vp, i64, vp, vp, C.POINTER(RansacOpts), vp, vp, vp, vp, vp, vp, vp]
    L.ba_relative_pose_five_point.argtypes = [vp, vp, i64, vp, vp, C.POINTER(RansacOpts), vp, vp, vp, vp, vp, vp, vp]
    L.ba_five_point.argtypes = [vp, i64, vp, vp, vp, vp]
    L.ba_ransac_cameras_p3p.argtypes = L.ba_ransac_cameras.argtypes
    L.ba_ransac_cameras_p3p_dev.argtypes = L.ba_ransac_cameras_dev.argtypes
    L.ba_ransac_points.argtypes = L.ba_ransac_cameras.argtypes
    L.ba_ransac_points_dev.argtypes = L.ba_ransac_cameras_dev.argtypes
    L.ba_p3p.argtypes = [vp, i64, vp, vp, vp, vp]
    L.ba_refine_relative_pose.argtypes = [vp, vp, i64, vp, vp, C.POINTER(PairRefineOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ba_homography.argtypes = L.ba_relative_pose.argtypes
    L.ba_decompose_homography.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
    L.ba_homography_pose.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp]
    L.ba_similarity.argtypes = [vp, i64, vp, vp, vp, vp, C.POINTER(RansacOpts), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.ba_rotation_loops.argtypes = [vp, i64, vp, vp, vp, vp, C.c_double, vp, vp]
    L.ba_view_graph_forest.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ba_average_rotations.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RotavgOpts)] + [vp] * 12
    L.ba_translation_loops.argtypes = L.ba_rotation_loops.argtypes
    L.ba_average_translations.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(TransavgOpts)] + [vp] * 13
    L.ba_transavg_lm_decide.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != BA_OK:
        msg = lib().ba_last_error().decode("utf-8", "replace")
        if rc == 4:
            raise SQDException(rc, msg)
        if rc == 1:
            raise BAArgError(rc, msg)
        raise BAError(rc, msg)


def ptr(a):
    """host pointer of a C-contiguous numpy array"""
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    try:
        rc = lib().ba_device_count(C.byref(n))
    except OSError:
        return 0
    return n.value if rc == BA_OK else 0


ORDERINGS = {"AMD": 0, "Metis": 1, "natural": 2}

# robust losses of the LM entries (ba_lm_set_loss): scipy's names
LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}


def loss_code(loss, f_scale):
    """(BA_LOSS_* code, scale) of a loss name ("huber" or the symbol-style ":huber") and f_scale; ValueError for an unknown
    name or a scale that is not finite and > 0 -- before any device call."""
    name = loss[1:] if isinstance(loss, str) and loss.startswith(":") else loss
    if name not in LOSSES:
        raise ValueError(f"loss must be one of {', '.join(LOSSES)} (or :name), got {loss!r}")
    try:
        c = float(f_scale)
    except (TypeError, ValueError):
        raise ValueError(f"f_scale must be a finite number > 0, got {f_scale!r}") from None
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"f_scale must be a finite number > 0, got {f_scale!r}")
    return LOSSES[name], c


def set_loss(handle, loss, f_scale):
    """the handle's loss for its next LM calls (ba_lm_set_loss)"""
    kind, c = loss_code(loss, f_scale)
    check(lib().ba_lm_set_loss(handle, kind, c))


# fixed parameters of the LM entries (ba_lm_set_fixed): bit b of a camera's mask is component b of its block, in the
# storage order r1 r2 r3 t1 t2 t3 k1 k2 f
CAMERA_PARAMS = {"r": 0x007, "t": 0x038, "k1": 0x040, "k2": 0x080, "f": 0x100}
CAMERA_ALL = 0x1FF


def _fixed_set(v, n, what):
    """boolean array of length n from 1-based indices or a boolean array of length n (n None: the checks that need no n)"""
    a = np.asarray(v)
    if a.dtype == np.bool_:
        if a.ndim != 1 or (n is not None and a.shape[0] != n):
            raise ValueError(f"{what}: a boolean array must have shape ({'n' if n is None else n},), got {a.shape}")
        return a if n is not None else None
    if a.size == 0:
        return np.zeros(n, dtype=bool) if n is not None else None
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: 1-based integer indices or a boolean array, got dtype {a.dtype}, shape {a.shape}")
    if a.min() < 1 or (n is not None and a.max() > n):
        raise ValueError(f"{what}: 1-based indices must lie in 1..{'n' if n is None else n}, got {a.min()}..{a.max()}")
    if n is None:
        return None
    out = np.zeros(n, dtype=bool)
    out[a - 1] = True
    return out


def _camera_params(v, ncams):
    """(ncams,) uint16 masks of fixed_camera_params: names applied to every camera, or a boolean (ncams, 9) array"""
    if isinstance(v, str):
        v = (v,)
    a = np.asarray(v)
    if a.dtype == np.bool_:
        if a.ndim != 2 or a.shape[1] != 9 or (ncams is not None and a.shape[0] != ncams):
            raise ValueError(f"fixed_camera_params: a boolean array must have shape ({'ncams' if ncams is None else ncams}, 9), "
                             f"got {a.shape}")
        return None if ncams is None else (a.astype(np.uint16) << np.arange(9, dtype=np.uint16)).sum(axis=1).astype(np.uint16)
    m = 0
    for name in v:
        if not isinstance(name, str) or name not in CAMERA_PARAMS:
            raise ValueError(f"fixed_camera_params: names among {', '.join(CAMERA_PARAMS)}, got {name!r}")
        m |= CAMERA_PARAMS[name]
    return None if ncams is None else np.full(ncams, m, dtype=np.uint16)


def check_fixed(fixed_cameras=None, fixed_points=None, fixed_camera_params=None):
    """the checks of fixed_masks that need no problem size (ValueError); True when the options select something"""
    some = False
    for v, what in ((fixed_cameras, "fixed_cameras"), (fixed_points, "fixed_points"), (fixed_camera_params, None)):
        if v is None:
            continue
        if what is None:
            _camera_params(v, None)
        else:
            _fixed_set(v, None, what)
        a = np.asarray((v,) if isinstance(v, str) else v)
        some = some or (bool(a.any()) if a.dtype == np.bool_ else a.size > 0)
    return some


def fixed_masks(ncams, npnts, fixed_cameras=None, fixed_points=None, fixed_camera_params=None):
    """(cam_mask uint16[ncams], pnt_fixed uint8[npnts]) of ba_lm_set_fixed, host only.  fixed_cameras / fixed_points:
    1-based indices (the Julia convention) or a boolean array of length ncams / npnts; a listed camera is fixed as a whole.
    fixed_camera_params: names among "r", "t", "k1", "k2", "f", applied to every camera (("k1", "k2", "f"): calibrated
    intrinsics), or a boolean (ncams, 9) array in block order (r1 r2 r3 t1 t2 t3 k1 k2 f).  The options are OR-ed.
    ValueError for an index 0 or above n, a wrong shape or an unknown name."""
    cam = np.zeros(ncams, dtype=np.uint16)
    pnt = np.zeros(npnts, dtype=np.uint8)
    if fixed_cameras is not None:
        cam[_fixed_set(fixed_cameras, ncams, "fixed_cameras")] = CAMERA_ALL
    if fixed_camera_params is not None:
        cam |= _camera_params(fixed_camera_params, ncams)
    if fixed_points is not None:
        pnt[_fixed_set(fixed_points, npnts, "fixed_points")] = 1
    return cam, pnt


def set_fixed(handle, cam_mask, pnt_fixed):
    """the handle's mask for its next LM calls (ba_lm_set_fixed); all-zero masks clear it"""
    cam = np.ascontiguousarray(cam_mask, dtype=np.uint16)
    pnt = np.ascontiguousarray(pnt_fixed, dtype=np.uint8)
    check(lib().ba_lm_set_fixed(handle, ptr(cam) if cam.any() else None, ptr(pnt) if pnt.any() else None))


def get_fixed(handle):
    """(fixed camera components, fixed points) the handle holds (ba_lm_get_fixed)"""
    nc, npt = C.c_int64(0), C.c_int64(0)
    check(lib().ba_lm_get_fixed(handle, C.byref(nc), C.byref(npt)))
    return nc.value, npt.value


# Gaussian priors of the LM entries (ba_lm_set_priors): (index, mu, info) per kind
_PRIOR_KINDS = (("point_priors", 3), ("camera_priors", 9), ("centre_priors", 3))


def _prior_lists(v, dim, n, what):
    """(idx1 int64 (m,), mu float64 (m, dim), packed info float64 (m, dim (dim + 1) / 2)) of one (index, mu, info) option, or
    None when it selects nothing.  index: 1-based indices or a boolean array of length n (n None: only the checks that need
    no problem size); mu: (m, dim); info: full symmetric blocks (m, dim, dim), or standard deviations (m, dim) meaning
    diag(1 / sigma^2), inf = unconstrained.  ValueError for anything else."""
    if v is None:
        return None
    try:
        index, mu, info = v
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a tuple (index, mu, info)") from None
    a = np.asarray(index)
    if a.dtype == np.bool_:
        if a.ndim != 1 or (n is not None and a.shape[0] != n):
            raise ValueError(f"{what}: a boolean index array must have shape ({'n' if n is None else n},), got {a.shape}")
        idx = np.flatnonzero(a).astype(np.int64) + 1
    elif a.size == 0:
        idx = np.zeros(0, dtype=np.int64)
    else:
        if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what}: 1-based integer indices or a boolean array, got dtype {a.dtype}, shape {a.shape}")
        idx = a.astype(np.int64)
        if idx.min() < 1 or (n is not None and idx.max() > n):
            raise ValueError(f"{what}: 1-based indices must lie in 1..{'n' if n is None else n}, got {idx.min()}..{idx.max()}")
        if np.unique(idx).size != idx.size:
            raise ValueError(f"{what}: an index may appear once")
    m = idx.size
    try:
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        info = np.asarray(info, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: mu and info must be numeric arrays") from None
    if mu.shape != (m, dim):
        raise ValueError(f"{what}: mu must have shape ({m}, {dim}), got {mu.shape}")
    if not np.isfinite(mu).all():
        raise ValueError(f"{what}: mu must be finite")
    if info.shape == (m, dim, dim):
        if not np.isfinite(info).all():
            raise ValueError(f"{what}: info must be finite")
        if not np.array_equal(info, info.transpose(0, 2, 1)):
            raise ValueError(f"{what}: the information blocks must be symmetric")
        full = info
    elif info.shape == (m, dim):
        if np.isnan(info).any() or (info <= 0).any():
            raise ValueError(f"{what}: standard deviations must be > 0 (inf: unconstrained)")
        full = np.zeros((m, dim, dim))
        full[:, np.arange(dim), np.arange(dim)] = 1.0 / info ** 2
    else:
        raise ValueError(f"{what}: info must be symmetric blocks ({m}, {dim}, {dim}) or standard deviations ({m}, {dim}), "
                         f"got {info.shape}")
    d = np.einsum("kii->ki", full)
    if (d < 0).any() or (full ** 2 > d[:, :, None] * d[:, None, :]).any():
        raise ValueError(f"{what}: the information blocks must be positive semi-definite")
    if m == 0:
        return None
    il, jl = np.tril_indices(dim)
    return idx, mu, np.ascontiguousarray(full[:, il, jl])


def check_priors(point_priors=None, camera_priors=None, centre_priors=None):
    """the checks of set_priors that need no problem size (ValueError); True when the options select something"""
    some = False
    for (what, dim), v in zip(_PRIOR_KINDS, (point_priors, camera_priors, centre_priors)):
        some = (_prior_lists(v, dim, None, what) is not None) or some
    return some


def set_priors(handle, ncams, npnts, point_priors=None, camera_priors=None, centre_priors=None):
    """the handle's priors for its next LM calls (ba_lm_set_priors), host only; nothing given clears them"""
    args = []
    keep = []
    for (what, dim), v, n in zip(_PRIOR_KINDS, (point_priors, camera_priors, centre_priors), (npnts, ncams, ncams)):
        lists = _prior_lists(v, dim, n, what)
        if lists is None:
            args += [0, None, None, None]
        else:
            keep.append(lists)
            args += [lists[0].size, ptr(lists[0]), ptr(lists[1]), ptr(lists[2])]
    check(lib().ba_lm_set_priors(handle, *args))


def get_priors(handle):
    """(point, camera, centre) prior counts the handle holds (ba_lm_get_priors)"""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib().ba_lm_get_priors(handle, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


# shared intrinsics of the LM entries (ba_lm_set_shared_intrinsics): calibration groups
MAX_GROUPS = 8


def _shared_groups(v, ncams=None):
    """the members of every group of a grouping, as a list of 0-based camera index arrays (group g at g - 1), from either form:
    an integer array of labels (0: own intrinsics, g in 1..8: member of group g) or a list of lists of 1-based camera indices.
    ncams None: only the checks that need no problem size.  ValueError for a negative label, a label above 8, a gap in the
    labels, an index outside 1..ncams, a camera in two groups or a wrong shape."""
    if isinstance(v, (list, tuple)) and (len(v) == 0 or all(isinstance(g, (list, tuple, np.ndarray)) for g in v)):
        if len(v) > MAX_GROUPS:
            raise ValueError(f"shared_intrinsics: at most {MAX_GROUPS} groups, got {len(v)}")
        groups = []
        for g, members in enumerate(v, 1):
            a = np.asarray(members)
            if a.size == 0:
                raise ValueError(f"shared_intrinsics: group {g} is empty (the labels may have no gap)")
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"shared_intrinsics: group {g}: 1-based integer camera indices, got dtype {a.dtype}, shape {a.shape}")
            if a.min() < 1 or (ncams is not None and a.max() > ncams):
                raise ValueError(f"shared_intrinsics: group {g}: 1-based indices must lie in 1..{'ncams' if ncams is None else ncams}, "
                                 f"got {a.min()}..{a.max()}")
            groups.append(a.astype(np.int64) - 1)
        every = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
        if np.unique(every).size != every.size:
            raise ValueError("shared_intrinsics: a camera may belong to one group only")
        return groups
    a = np.asarray(v)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer) or (ncams is not None and a.shape[0] != ncams):
        raise ValueError(f"shared_intrinsics: integer labels of shape ({'ncams' if ncams is None else ncams},) or a list of "
                         f"lists of 1-based camera indices, got dtype {a.dtype}, shape {a.shape}")
    if a.size and (a.min() < 0 or a.max() > MAX_GROUPS):
        raise ValueError(f"shared_intrinsics: labels must lie in 0..{MAX_GROUPS} (0: own intrinsics), got {a.min()}..{a.max()}")
    groups = [np.flatnonzero(a == g) for g in range(1, (int(a.max()) if a.size else 0) + 1)]
    for g, mem in enumerate(groups, 1):
        if mem.size == 0:
            raise ValueError(f"shared_intrinsics: the labels have a gap: no camera in group {g}, but one in group {len(groups)}")
    return groups


def check_shared(shared_intrinsics):
    """the checks of shared_labels that need no problem size (ValueError); True when the option ties something (a group of two
    cameras or more)"""
    return shared_intrinsics is not None and any(g.size >= 2 for g in _shared_groups(shared_intrinsics))


def shared_labels(shared_intrinsics, ncams):
    """int32 labels (ncams,) of a grouping in either form of _shared_groups -- 0: the camera keeps its own (k1, k2, f); g in
    1..G <= 8: it shares them with the other members of group g -- or None when nothing is shared (None, all labels 0, only
    groups of one camera).  ValueError as _shared_groups, before any device call."""
    if shared_intrinsics is None:
        return None
    groups = _shared_groups(shared_intrinsics, int(ncams))
    if not any(g.size >= 2 for g in groups):
        return None
    lab = np.zeros(int(ncams), dtype=np.int32)
    for g, mem in enumerate(groups, 1):
        lab[mem] = g
    return lab


def set_shared(handle, labels):
    """the handle's grouping for its next LM calls (ba_lm_set_shared_intrinsics); None clears it"""
    check(lib().ba_lm_set_shared_intrinsics(handle, None if labels is None else ptr(labels)))


def get_shared(handle):
    """(groups, members) the handle holds (ba_lm_get_shared_intrinsics)"""
    g, m = C.c_int(0), C.c_int64(0)
    check(lib().ba_lm_get_shared_intrinsics(handle, C.byref(g), C.byref(m)))
    return g.value, m.value


def tie_intrinsics(x, npnts, shared_intrinsics):
    """A copy of x (layout [points; cameras]) in which the members of every group hold the (k1, k2, f) of the group's first
    member (lowest camera index): what a step or solve with shared_intrinsics asks of its x."""
    x = np.array(x, dtype=np.float64, copy=True)
    npnts = int(npnts)
    if x.ndim != 1 or (x.size - 3 * npnts) % 9 != 0 or x.size < 3 * npnts:
        raise ValueError(f"tie_intrinsics: x must have 3 npnts + 9 ncams entries, got {x.shape} with npnts = {npnts}")
    ncams = (x.size - 3 * npnts) // 9
    lab = shared_labels(shared_intrinsics, ncams)
    if lab is None:
        return x
    cams = x[3 * npnts:].reshape(ncams, 9)
    for g in range(1, int(lab.max()) + 1):
        mem = np.flatnonzero(lab == g)
        if mem.size >= 2:
            cams[mem[1:], 6:9] = cams[mem[0], 6:9]
    return x


def _check_tied(x, npnts, labels):
    """ValueError when the members of a group do not hold identical (k1, k2, f) in x (labels: shared_labels)"""
    tied = tie_intrinsics(x, npnts, labels)
    bad = np.flatnonzero((tied.view(np.int64) != np.ascontiguousarray(x, dtype=np.float64).view(np.int64))[3 * npnts:])
    if bad.size:
        c = int(bad[0]) // 9
        raise ValueError(f"shared_intrinsics: camera {c + 1} holds other (k1, k2, f) than the first member of its group "
                         f"{int(labels[c])}: the members of a group must be identical in x (see tie_intrinsics)")


# per-observation information of the LM entries (ba_lm_set_obs_info)
def obs_info_pack(obs_info, nobs=None):
    """(nobs, 3) float64 array xx xy yy of ba_lm_set_obs_info, host only, or None for None.  obs_info: standard deviations in
    pixels, (nobs,) isotropic or (nobs, 2) sigma_x, sigma_y -- meaning diag(1 / sigma^2), inf = information 0 (the convention of
    the priors' info) -- or the information matrices themselves, (nobs, 2, 2) symmetric positive semi-definite.  nobs None: only
    the checks that need no problem size.  ValueError for another shape, sigma <= 0 or NaN, a block that is not finite, not
    symmetric or not positive semi-definite."""
    if obs_info is None:
        return None
    try:
        a = np.asarray(obs_info, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("obs_info: a numeric array of standard deviations or information matrices") from None
    n = "nobs" if nobs is None else int(nobs)
    if not (a.ndim == 1 or (a.ndim == 2 and a.shape[1] == 2) or (a.ndim == 3 and a.shape[1:] == (2, 2))) or \
            (nobs is not None and a.shape[0] != int(nobs)):
        raise ValueError(f"obs_info: standard deviations ({n},) or ({n}, 2), or information matrices ({n}, 2, 2), got {a.shape}")
    out = np.zeros((a.shape[0], 3))
    if a.ndim == 3:
        if not np.isfinite(a).all():
            raise ValueError("obs_info: the information matrices must be finite")
        if not np.array_equal(a[:, 0, 1], a[:, 1, 0]):
            raise ValueError("obs_info: the information matrices must be symmetric")
        out[:, 0], out[:, 1], out[:, 2] = a[:, 0, 0], a[:, 0, 1], a[:, 1, 1]
        if (out[:, 0] < 0).any() or (out[:, 2] < 0).any() or (out[:, 1] ** 2 > out[:, 0] * out[:, 2]).any():
            raise ValueError("obs_info: the information matrices must be positive semi-definite")
        return out
    if np.isnan(a).any() or (a <= 0).any():
        raise ValueError("obs_info: standard deviations must be > 0 (inf: the observation, or that direction, is dropped)")
    s = a if a.ndim == 2 else np.stack([a, a], axis=1)
    out[:, 0], out[:, 2] = 1.0 / s[:, 0] ** 2, 1.0 / s[:, 1] ** 2
    return out


def set_obs_info(handle, info3):
    """the handle's information array for its next LM calls (ba_lm_set_obs_info); info3: obs_info_pack's array, None clears"""
    a = None if info3 is None else np.ascontiguousarray(info3, dtype=np.float64)
    check(lib().ba_lm_set_obs_info(handle, None if a is None else ptr(a)))


def get_obs_info(handle):
    """(observations with an information matrix: 0 or nobs, those with Lambda = 0) the handle holds (ba_lm_get_obs_info)"""
    n, z = C.c_int64(0), C.c_int64(0)
    check(lib().ba_lm_get_obs_info(handle, C.byref(n), C.byref(z)))
    return n.value, z.value


# states of ba_refine_points and ba_refine_cameras (BA_PT_*): the low bits of a point's or camera's status; BA_PT_BEHIND is OR-ed
# into it
POINT_STATES = ("converged", "stalled", "max_iter", "fixed", "degenerate", "nonfinite")
POINT_BEHIND = 0x80


# the consensus stage of refine_cameras(resect=True, ransac=...) (ba_ransac_cameras): the options and their ranges
RANSAC_KEYS = ("threshold", "hypotheses", "sample", "refits", "min_inliers", "seed")


def ransac_opts(ransac, least=6, most=16, least_set=None):
    """RansacOpts of the dict `ransac` -- threshold (pixels, required), hypotheses (None or <= 0: 128; at most 4096), sample
    (None or <= 0: 6; 6..16), refits (None or < 0: 2; at most 8), min_inliers (None or <= 0: max(sample, 6); at least 6), seed
    (0 .. 2^64 - 1, default 0) -- or ValueError, before any device call.  least: the smallest sample and min_inliers of the
    entry (6: the resection; 8: relative_pose, where it is also the default sample).  most: the largest sample; least_set: the
    smallest min_inliers where it is not `least` (relative_pose_five_point: least = most = 5, a sample of exactly 5, and
    least_set = 8, the sets of the eight-point fits behind it; refine_cameras(minimal="p3p"): least = most = 3 and least_set = 6,
    the sets of the linear resection behind it; refine_points(triangulate=True, ransac=): least = most = least_set = 2, two
    rays are a hypothesis and the smallest set the triangulation takes)."""
    least_set = least if least_set is None else least_set
    if not isinstance(ransac, dict):
        raise ValueError(f"ransac must be a dict with the keys {', '.join(RANSAC_KEYS)} (or None), got {ransac!r}")
    unknown = [k for k in ransac if k not in RANSAC_KEYS]
    if unknown:
        raise ValueError(f"ransac: unknown key {unknown[0]!r} (keys: {', '.join(RANSAC_KEYS)})")
    if "threshold" not in ransac:
        raise ValueError("ransac: threshold (pixels) is required")
    try:
        tau = float(ransac["threshold"])
    except (TypeError, ValueError):
        raise ValueError(f"ransac: threshold must be a finite number > 0, got {ransac['threshold']!r}") from None
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError(f"ransac: threshold must be a finite number > 0, got {ransac['threshold']!r}")
    ints = {}
    for key, unset in (("hypotheses", 0), ("sample", 0), ("refits", -1), ("min_inliers", 0), ("seed", 0)):
        v = ransac.get(key)
        if v is None:
            v = unset
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
            raise ValueError(f"ransac: {key} must be an integer (or None), got {v!r}")
        ints[key] = int(v)
    if ints["hypotheses"] > 4096:
        raise ValueError(f"ransac: hypotheses must be <= 4096, got {ints['hypotheses']}")
    if ints["sample"] > 0 and not least <= ints["sample"] <= most:
        want = f"be {least}" if least == most else f"lie in {least}..{most}"
        raise ValueError(f"ransac: sample must {want}, got {ints['sample']}")
    if ints["refits"] > 8:
        raise ValueError(f"ransac: refits must be <= 8, got {ints['refits']}")
    if 0 < ints["min_inliers"] < least_set:
        raise ValueError(f"ransac: min_inliers must be >= {least_set}, got {ints['min_inliers']}")
    if not 0 <= ints["seed"] < 1 << 64:
        raise ValueError(f"ransac: seed must lie in 0 .. 2^64 - 1, got {ints['seed']}")
    for key in ("hypotheses", "sample", "refits", "min_inliers"):
        ints[key] = max(ints[key], -1)  # (any value below the range means "the default")
    return RansacOpts(tau, ints["hypotheses"], ints["sample"], ints["refits"], ints["min_inliers"], ints["seed"])


def ransac_sample(seed, hypothesis, degree, sample=6, used=None):
    """The positions hypothesis `hypothesis` samples in an observation list of `degree` entries (ba_ransac_sample, host only):
    an int64 array of `sample` positions in the order of their draws, or None when the hypothesis is void.  used: a boolean
    array of length degree, or None (all used)."""
    pos, n = np.zeros(16, dtype=np.int64), C.c_int(0)
    u = None if used is None else np.ascontiguousarray(used, dtype=np.uint8)
    if u is not None and u.shape != (int(degree),):
        raise ValueError(f"used must have shape ({int(degree)},), got {u.shape}")
    check(lib().ba_ransac_sample(int(seed), int(hypothesis), int(degree), None if u is None else ptr(u), int(sample), ptr(pos), C.byref(n)))
    m = 6 if sample <= 0 else int(sample)
    return pos[:m].copy() if n.value == m else None


# states of ba_relative_pose (BA_RP_*)
PAIR_STATES = ("ok", "few_matches", "degenerate", "no_consensus")

# states of ba_homography (BA_HG_*): the names of PAIR_STATES; few_matches is "fewer than 4 used matches" here
HOMOGRAPHY_STATES = PAIR_STATES

# states of ba_similarity (BA_SM_*), per problem; few_rows is "fewer than 3 used rows"
SIMILARITY_STATES = ("ok", "few_rows", "degenerate", "no_consensus")

# states of ba_refine_relative_pose (BA_RR_*) and the keys of the `refine=` dict of relative_pose*
PAIR_REFINE_STATES = ("converged", "stalled", "max_iter", "nonfinite", "skipped")
PAIR_REFINE_KEYS = ("max_iter", "xtol", "lam0", "loss", "f_scale", "threshold", "rounds")


def pair_refine_opts(max_iter=None, xtol=None, lam0=None, loss=None, f_scale=1.0, threshold=None, rounds=None):
    """PairRefineOpts of the options of refine_relative_pose -- max_iter (None or < 0: 50), xtol (None or <= 0: 1e-10), lam0 (None
    or <= 0: 1e-4), loss (None: "linear"; a name of LOSSES) with f_scale (pixels, finite and > 0), threshold (pixels, required,
    finite and > 0), rounds (None or < 0: 2; at most 8) -- or ValueError, before any device call"""
    ints = {}
    for key, v in (("max_iter", max_iter), ("rounds", rounds)):
        v = -1 if v is None else v
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
            raise ValueError(f"refine_relative_pose: {key} must be an integer (or None), got {v!r}")
        ints[key] = max(int(v), -1)
    if ints["rounds"] > 8:
        raise ValueError(f"refine_relative_pose: rounds must be <= 8, got {ints['rounds']}")
    reals = {}
    for key, v, positive in (("xtol", xtol, False), ("lam0", lam0, False), ("f_scale", f_scale, True), ("threshold", threshold, True)):
        if v is None and not positive:
            v = 0.0
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"refine_relative_pose: {key} must be a finite number, got {v!r}") from None
        if not np.isfinite(v) or (positive and not v > 0):
            raise ValueError(f"refine_relative_pose: {key} must be a finite number{' > 0' if positive else ''}, got {v!r}")
        reals[key] = v
    loss = "linear" if loss is None else loss
    if not isinstance(loss, str) or loss not in LOSSES:
        raise ValueError(f"refine_relative_pose: loss must be one of {', '.join(LOSSES)}, got {loss!r}")
    return PairRefineOpts(ints["max_iter"], reals["xtol"], reals["lam0"], LOSSES[loss], reals["f_scale"], reals["threshold"],
                          ints["rounds"])


# states of ba_average_rotations (BA_RA_*), per camera
ROTAVG_STATES = ("ok", "root", "fixed", "isolated")
# states of ba_average_translations (BA_TA_*), per camera: the same four
TRANSAVG_STATES = ROTAVG_STATES


def _pairs(pairs, ncams=None):
    """(a1, b1) int64 arrays of `pairs` (npairs, 2), 1-based cameras; ValueError for another shape, a dtype that is not integer, an
    index below 1 (above ncams when given) or a pair of one camera"""
    a = np.asarray(pairs)
    if a.size == 0:
        a = a.reshape(0, 2).astype(np.int64)
    if a.ndim != 2 or a.shape[1] != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"pairs must be an integer array of shape (npairs, 2) of 1-based cameras, got dtype {a.dtype}, shape {a.shape}")
    a = a.astype(np.int64)
    if a.size and (a.min() < 1 or (ncams is not None and a.max() > int(ncams))):
        raise ValueError(f"pairs: 1-based cameras must lie in 1..{'ncams' if ncams is None else int(ncams)}, got {a.min()}..{a.max()}")
    if (a[:, 0] == a[:, 1]).any():
        raise ValueError("pairs: a pair holds two different cameras")
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])


def pair_matches(cam_idx1, pnt_idx1, ncams, npnts, pairs):
    """The match lists of camera pairs (ba_pair_matches, host only): (match_ptr (npairs + 1), obs_a, obs_b), the observations
    0-based.  The matches of pair (a, b) -- pairs[k], 1-based cameras -- are the points both cameras observe, ordered by a's list
    (the caller's order), each with a's and b's first observation of the point."""
    a1, b1 = _pairs(pairs, ncams)
    cam = np.ascontiguousarray(cam_idx1, dtype=np.int64)
    pnt = np.ascontiguousarray(pnt_idx1, dtype=np.int64)
    if cam.ndim != 1 or cam.shape != pnt.shape:
        raise ValueError(f"cam_idx1 and pnt_idx1 must be one-dimensional and of one length, got {cam.shape} and {pnt.shape}")
    mp = np.zeros(len(a1) + 1, dtype=np.int64)
    args = (int(ncams), int(npnts), len(cam), ptr(cam), ptr(pnt), len(a1), ptr(a1), ptr(b1), ptr(mp))
    check(lib().ba_pair_matches(*args, None, None))
    oa, ob = np.zeros(int(mp[-1]), dtype=np.int64), np.zeros(int(mp[-1]), dtype=np.int64)
    check(lib().ba_pair_matches(*args, ptr(oa), ptr(ob)))
    return mp, oa - 1, ob - 1


def compose_relative(x, npnts, a, b, r, t, baseline=1.0):
    """A copy of x (layout [points; cameras]) in which camera b (1-based) has the pose (R R_a, R t_a + baseline t) from camera a's
    pose in x and the relative pose (r, t) of relative_pose: P_b = R P_a + baseline t.  The rotation vector is written by the rule
    of the library's resection (theta < 1e-12: (1e-12, 0, 0)).  numpy, host only.  With camera a at the canonical pose
    (r = (1e-12, 0, 0), t = 0) this seeds a reconstruction: camera b becomes (R, baseline t)."""
    x = np.array(x, dtype=np.float64, copy=True)
    npnts = int(npnts)
    if x.ndim != 1 or (x.size - 3 * npnts) % 9 != 0 or x.size < 3 * npnts:
        raise ValueError(f"compose_relative: x must have 3 npnts + 9 ncams entries, got {x.shape} with npnts = {npnts}")
    ncams = (x.size - 3 * npnts) // 9
    for c in (a, b):
        if not isinstance(c, (int, np.integer)) or isinstance(c, (bool, np.bool_)) or not 1 <= c <= ncams:
            raise ValueError(f"compose_relative: cameras are 1-based integers in 1..{ncams}, got {c!r}")
    if a == b:
        raise ValueError("compose_relative: a and b are two different cameras")
    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if r.shape != (3,) or t.shape != (3,):
        raise ValueError(f"compose_relative: r and t must have shape (3,), got {r.shape} and {t.shape}")
    cams = x[3 * npnts:].reshape(ncams, 9)

    def rodrigues(v):
        th = np.sqrt(v @ v)
        k = v / th
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return np.cos(th) * np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * np.outer(k, k)

    R = rodrigues(r)
    Rb = R @ rodrigues(cams[a - 1, :3])
    cams[b - 1, :3] = rotation_vector(Rb)
    cams[b - 1, 3:6] = R @ cams[a - 1, 3:6] + float(baseline) * t
    return x


def _rodrigues(v):
    """the rotation matrix of the rotation vector v (the model's formula: no theta -> 0 branch)"""
    th = np.sqrt(v @ v)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * np.outer(k, k)


def _x_parts(who, x, npnts):
    """(a copy of x, its points (npnts, 3), its cameras (ncams, 9)) -- views into the copy -- or ValueError"""
    x = np.array(x, dtype=np.float64, copy=True)
    npnts = int(npnts)
    if x.ndim != 1 or npnts < 0 or x.size < 3 * npnts or (x.size - 3 * npnts) % 9 != 0:
        raise ValueError(f"{who}: x must have 3 npnts + 9 ncams entries, got {x.shape} with npnts = {npnts}")
    return x, x[:3 * npnts].reshape(npnts, 3), x[3 * npnts:].reshape(-1, 9)


def _subset(who, name, idx1, n):
    """0-based indices of the 1-based integer array idx1 (None: all n), or ValueError"""
    if idx1 is None:
        return np.arange(n)
    a = np.asarray(idx1)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer) or a.min() < 1 or a.max() > n:
        raise ValueError(f"{who}: {name} must be a one-dimensional array of 1-based integers in 1..{n}, got dtype {a.dtype}, shape {a.shape}")
    return np.unique(a.astype(np.int64)) - 1


def camera_centres(x, npnts):
    """The centres -R' t of the cameras of x (layout [points; cameras]), shape (ncams, 3).  numpy, host only."""
    _, _, cams = _x_parts("camera_centres", x, npnts)
    return np.array([-_rodrigues(c[:3]).T @ c[3:6] for c in cams]).reshape(-1, 3)


def apply_similarity(x, npnts, s, r, t, *, cameras=None, points=None):
    """A copy of x (layout [points; cameras]) moved by the similarity (s, r, t) of `similarity`: a point X becomes s Q X + t with
    Q the rotation of r; a camera (R, t_c) becomes (R Q', s t_c - R Q' t), so that its centre C becomes s Q C + t and R X + t_c
    of every point is multiplied by s: the intrinsics are untouched and every reprojection is unchanged.  The rotation vector
    is written by the rule of compose_relative.  cameras, points: 1-based index arrays that move only one component or one
    sub-model (None: all).  numpy, host only."""
    who = "apply_similarity"
    x, pts, cams = _x_parts(who, x, npnts)
    try:
        s, r, t = float(s), np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: s must be a number, r and t arrays of numbers") from None
    if r.shape != (3,) or t.shape != (3,):
        raise ValueError(f"{who}: r and t must have shape (3,), got {r.shape} and {t.shape}")
    if not (np.isfinite(s) and s > 0 and np.isfinite(r).all() and np.isfinite(t).all() and r @ r > 0):
        raise ValueError(f"{who}: s must be finite and > 0, r finite and not 0, t finite, got {s!r}, {r!r}, {t!r}")
    ci, pi = _subset(who, "cameras", cameras, len(cams)), _subset(who, "points", points, len(pts))
    Q = _rodrigues(r)
    pts[pi] = s * (pts[pi] @ Q.T) + t
    for c in ci:
        Rn = _rodrigues(cams[c, :3]) @ Q.T
        cams[c, :3] = rotation_vector(Rn)
        cams[c, 3:6] = s * cams[c, 3:6] - Rn @ t
    return x


def rotation_vector(R):
    """the rotation vector of a 3 x 3 rotation by the rule of the library's resection: theta = atan2(|w| / 2, (tr R - 1) / 2), w
    the skew part, axis w / |w|; for cos theta < 0 the axis comes from the diagonal of R + I with the sign of w; theta < 1e-12:
    (1e-12, 0, 0)"""
    R = np.asarray(R, dtype=np.float64)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    wn = np.sqrt(w @ w)
    co = 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(0.5 * wn, co)
    if th < 1e-12:
        return np.array([1e-12, 0.0, 0.0])
    if co >= 0:
        return th * w / wn
    i = int(np.argmax(np.diag(R)))
    ki = np.sqrt((R[i, i] - co) / (1.0 - co))
    k = np.array([ki if j == i else 0.5 * (R[i, j] + R[j, i]) / ((1.0 - co) * ki) for j in range(3)])
    k = k / np.sqrt(k @ k)
    return th * (-k if k @ w < 0 else k)


# the matrix of DESIGN §5h as Python sees it (the communicator and ba_covariance columns are the library's): per term the
# attribute of ProblemTerms that says it is on, its name in a message, the uses it is not supported with in reporting order
_REFUSED = (("tied", "shared_intrinsics is", ("linesearch", "facto_f32", "facto_f16", "normalize", "xf32")),
            ("robust", "a robust loss is", ("linesearch", "xf32", "facto_f16")),
            ("with_priors", "priors are", ("linesearch", "facto_f16", "xf32")),
            ("masked", "fixed parameters are", ("facto_f16",)),
            ("weighted", "obs_info is", ("linesearch", "xf32", "facto_f16")))


class ProblemTerms:
    """The optional terms of one LM call from its keywords: at construction the checks that need no problem size (ValueError
    before anything touches a model or the device); refuse(): the options a term is not supported with; apply(): onto a handle."""

    def __init__(self, loss="linear", f_scale=1.0, fixed_cameras=None, fixed_points=None, fixed_camera_params=None,
                 point_priors=None, camera_priors=None, centre_priors=None, shared_intrinsics=None, obs_info=None):
        self.fixed = (fixed_cameras, fixed_points, fixed_camera_params)
        self.priors = (point_priors, camera_priors, centre_priors)
        self.shared, self.tied = shared_intrinsics, check_shared(shared_intrinsics)
        self.kind, self.c = loss_code(loss, f_scale)
        self.robust = self.kind != 0
        self.with_priors = check_priors(*self.priors)
        self.masked = check_fixed(*self.fixed)
        self.info3 = obs_info_pack(obs_info)  # (packed once; its length is held to the problem's when it meets one)
        self.weighted = self.info3 is not None

    def refuse(self, linesearch=False, facto_type=None, normalize="None", xf32=False):
        """ValueError when a term that is on is not supported with one of these options"""
        ft = facto_type if facto_type is None else np.dtype(facto_type)
        uses = {"linesearch": (linesearch, "with linesearch = true"), "facto_f32": (ft == np.float32, "with facto_type = Float32"),
                "facto_f16": (ft == np.float16, "with facto_type = Float16"), "xf32": (xf32, "for a Float32 model (x_f32)"),
                "normalize": (normalize in ("J", "A", ":J", ":A"), "with normalize = :J or :A")}
        for on, subject, refused in _REFUSED:
            for use in refused:
                if getattr(self, on) and uses[use][0]:
                    raise ValueError(f"{subject} not supported {uses[use][1]}")

    def set_loss(self, nlp):  # (alone: BALNLPModel.robust_weights, the rest of the handle stays)
        check(lib().ba_lm_set_loss(nlp.handle, self.kind, self.c))

    def set_priors(self, nlp):  # (alone: BALNLPModel.prior_eval)
        set_priors(nlp.handle, nlp.ncams, nlp.npnts, *self.priors)

    def sized_info(self, nobs):
        if self.info3 is not None and self.info3.shape[0] != int(nobs):
            raise ValueError(f"obs_info: one entry per observation ({int(nobs)}), got {self.info3.shape[0]}")
        return self.info3

    def set_obs_info(self, nlp):  # (with set_loss: BALNLPModel.robust_weights)
        set_obs_info(nlp.handle, self.sized_info(nlp.nobs))

    def apply(self, nlp, x=None, shared=True):
        """Pack the terms for nlp's sizes (ValueError before the handle changes), check that x (if given) is tied as the grouping
        asks, and set them on the handle: a term without its keyword is cleared.  shared=False leaves the handle's grouping."""
        cam_mask, pnt_fixed = fixed_masks(nlp.ncams, nlp.npnts, *self.fixed)
        labels = shared_labels(self.shared, nlp.ncams) if shared else None
        info3 = self.sized_info(nlp.nobs)
        if x is not None and labels is not None:
            _check_tied(x, nlp.npnts, labels)
        self.set_loss(nlp)
        set_fixed(nlp.handle, cam_mask, pnt_fixed)
        self.set_priors(nlp)
        if shared:
            set_shared(nlp.handle, labels)
        set_obs_info(nlp.handle, info3)


def dense_ldl_solve_multi(A, B, device=0):
    """Solve A X = B for the columns of B (n, nrhs) with ONE device LDL' and the multi-right-hand-side sweeps
    (ba_dense_ldl_solve_multi); only the lower triangle of A is read.  -> (X (n, nrhs), factor_ms)"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    Bc = np.ascontiguousarray(np.asarray(B, dtype=np.float64).T)  # column-major n x nrhs
    nrhs, n = Bc.shape
    X = np.zeros_like(Bc)
    ms = C.c_double(0)
    check(lib().ba_dense_ldl_solve_multi(device, n, ptr(A), nrhs, ptr(Bc), ptr(X), C.byref(ms)))
    return np.ascontiguousarray(X.T), ms.value


def schur_ordering(cam_idx1, pnt_idx1, ncams, npnts, method="AMD"):
    """Fill-reducing camera ordering of a problem (`perm` of src/lm.jl:84-88 applied to the reduced camera system) and the
    tile fill it leaves: (perm1, tile_fill, flop_fill, block_fill); perm1[k] = 1-based camera at block row k of S.  Host
    only: needs no device."""
    cam = np.ascontiguousarray(cam_idx1, dtype=np.int64)
    pnt = np.ascontiguousarray(pnt_idx1, dtype=np.int64)
    perm = np.zeros(int(ncams), dtype=np.int64)
    tf, ff, bf = C.c_double(0), C.c_double(0), C.c_double(0)
    check(lib().ba_schur_ordering(int(ncams), int(npnts), len(cam), ptr(cam), ptr(pnt), ORDERINGS[method], ptr(perm),
                                  C.byref(tf), C.byref(ff), C.byref(bf)))
    return perm, tf.value, ff.value, bf.value


def dense_ldl_solve(A, b, device=0, f32=False):
    """Solve A x = b with the device blocked LDL' (A symmetric, only its lower triangle is read); f32: in Float32."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = A.shape[0]
    x = np.zeros(n)
    ms = C.c_double(0)
    fn = lib().ba_dense_ldl_solve_f32 if f32 else lib().ba_dense_ldl_solve
    check(fn(device, n, ptr(A), ptr(b), ptr(x), C.byref(ms)))
    return x, ms.value
