"""What test_refine_points.py, test_refine_cameras.py and test_resect_cameras.py share: the model of a scene, the status codes of
an info dict, bit views, the scenes of isolated cameras, camera priors and the two measures the camera bounds are stated in."""
import numpy as np

from _lm_run import arrays
from block_ref import BEHIND
from cameras_ref import cameras
from scenes import _scene_from_lists

# standard deviations of a camera prior, block order r t k1 k2 f: the scales of the generator's cameras
PRIOR_SIGMA = np.array([1e-3] * 3 + [1e-2] * 3 + [1e-8, 1e-13, 1.0])
_SMALL = []


def small_scene(ba):
    """small_prob (conftest.py), for the helpers of a module that cannot take fixtures"""
    if not _SMALL:
        _SMALL.append(ba.synthetic.make_problem(12, 400, 1800, seed=11))
    return _SMALL[0]


def _model(ba, p):
    return ba.BALNLPModel(arrays=arrays(p))


def codes(ba, info):
    """uint8 status as the C entries return it, from the info of refine_points / refine_cameras"""
    names = list(ba._lib.POINT_STATES)
    return (np.array([names.index(s) for s in info["status"]]) | np.where(info["behind"], BEHIND, 0)).astype(np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _isolated(ba, degrees, seed):
    """isolated cameras with the given degrees, every point seen once"""
    degrees = np.asarray(degrees, dtype=np.int64)
    npnts = int(degrees.sum())
    return _scene_from_lists(ba, len(degrees), npnts, np.arange(npnts, dtype=np.int64), np.repeat(np.arange(len(degrees)), degrees), seed)


def only_camera(p, c):
    """the scene that holds camera c (0-based) of p alone, with its points in their order"""
    n = p["npnts"]
    keep = (np.asarray(p["cam_idx1"]) - 1) == c
    pnts, new = np.unique(np.asarray(p["pnt_idx1"])[keep] - 1, return_inverse=True)
    out = dict(cam_idx1=np.ones(int(keep.sum()), dtype=np.int64), pnt_idx1=new.astype(np.int64) + 1,
               pt2d=np.ascontiguousarray(np.asarray(p["pt2d"]).reshape(-1, 2)[keep].ravel()), ncams=1, npnts=len(pnts), nobs=int(keep.sum()))
    for key in ("x0", "x_true"):
        x = np.asarray(p[key])
        out[key] = np.concatenate([x[:3 * n].reshape(n, 3)[pnts].ravel(), x[3 * n + 9 * c:3 * n + 9 * c + 9]])
    return out


def cam_prior_on(p, idx, seed):
    """full-rank camera priors on the cameras idx (0-based): mu = the true camera moved by 0.3 sigma, Lambda = S^-1 M S^-1 with
    S = diag(PRIOR_SIGMA) and M a well-conditioned full symmetric matrix"""
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx, dtype=np.int64)
    true = cameras(p, p["x_true"])[idx]
    mu = true + 0.3 * PRIOR_SIGMA * rng.standard_normal((len(idx), 9))
    B = rng.standard_normal((len(idx), 9, 9))
    M = np.eye(9) + 0.05 * np.einsum("kij,klj->kil", B, B)
    Lam = M / (PRIOR_SIGMA[:, None] * PRIOR_SIGMA[None, :])
    return idx, mu, 0.5 * (Lam + Lam.transpose(0, 2, 1))


def scaled(D, C, C_ref):
    return np.linalg.norm(D * (C - C_ref), axis=1) / (1.0 + np.linalg.norm(D * C_ref, axis=1))


def rel_cost(after, cost_ref):
    """relative difference of cost_after per camera; where the reference's minimum is numerically zero against its start (a
    camera held by a prior alone: the minimum of a quadratic is exactly 0) the difference is taken against 1e-12 of the start"""
    den = np.maximum(cost_ref[:, 1], 1e-12 * cost_ref[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, np.abs(after - cost_ref[:, 1]) / den, 0.0)
