"""numpy restatement of ba_resect_cameras (include/ba_hip.h, "linear camera resection"): per camera the undistorted
measurements, the Hartley normalisation of its points, the 12 x 12 normal matrix of the two homogeneous equations per observation,
the eigenvector of its smallest eigenvalue, the degeneracy decisions, the pose recovered from it and the rotation vector; then
cameras_ref.refine carries on from that pose.  Written from the text of the header, not from the kernel: the eigen-decomposition
is np.linalg.eigh on the assembled matrix and the nearest rotation comes from np.linalg.svd, where the kernel runs Jacobi
sweeps of its own."""
import numpy as np

import cameras_ref as cr
from block_ref import undistort

DONE, SKIPPED, DEGENERATE = 0, 1, 2
MIN_OBS = 6
POSE = np.array([True] * 6 + [False] * 3)


def rotation_vector(R):
    """theta = atan2(|w| / 2, (tr R - 1) / 2), w the skew part of R, axis w / |w|; near pi (cos theta < 0) the axis comes from the
    diagonal of R + I with the sign of w; theta < 1e-12: (1e-12, 0, 0)"""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    wn = np.linalg.norm(w)
    co = 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(0.5 * wn, co)
    if th < 1e-12:
        return np.array([1e-12, 0.0, 0.0])
    if co >= 0:
        return th * w / wn
    B = 0.5 * (R + R.T) - co * np.eye(3)  # (1 - cos) k k'
    i = int(np.argmax(np.diag(R)))
    k = B[i] / np.sqrt(B[i, i] * (1.0 - co))
    k /= np.linalg.norm(k)
    return th * (-k if k @ w < 0 else k)


def moments(Xn, q):
    """M = [[S0, 0, Sx], [0, S0, Sy], [Sx, Sy, Sq]] of the normalised points Xn (n, 3) and the image points q (n, 2)"""
    h = np.concatenate([Xn, np.ones((len(Xn), 1))], axis=1)
    hh = h[:, :, None] * h[:, None, :]
    S0, Sx, Sy = hh.sum(0), (q[:, 0, None, None] * hh).sum(0), (q[:, 1, None, None] * hh).sum(0)
    Sq = ((q * q).sum(1)[:, None, None] * hh).sum(0)
    Z = np.zeros((4, 4))
    return np.block([[S0, Z, Sx], [Z, S0, Sy], [Sx, Sy, Sq]])


def resect_one(X, m, k1, k2, f, normalise=True):
    """the pose (r, t) of one camera from its used points X (n, 3) and measurements m (n, 2), or None: degenerate.
    -> (r, t, lambda_2 / lambda_12)"""
    if len(X) < MIN_OBS or not np.isfinite(f) or f == 0:
        return None, None, np.nan
    with np.errstate(all="ignore"):
        q = undistort(m, k1, k2, f)
        if normalise:
            d = X - X[0]
            mean = X[0] + d.mean(0)
            rms = np.sqrt((((X - mean) ** 2).sum(1)).mean())
            if not (rms > 0) or not np.isfinite(rms):
                return None, None, np.nan
            s = 1.0 / rms
        else:
            mean, s = np.zeros(3), 1.0
        Xn = s * (X - mean)
        M = moments(Xn, q)
    if not np.isfinite(M).all():
        return None, None, np.nan
    lam, V = np.linalg.eigh(M)
    ratio = lam[1] / lam[11]
    if not lam[1] > 1e-10 * lam[11]:
        return None, None, ratio
    P = V[:, 0].reshape(3, 4)
    A, b = P[:, :3], P[:, 3]
    front = (Xn @ A[2] + b[2] < 0).sum()
    if 2 * front < len(X):
        A, b = -A, -b
    U, sg, Vt = np.linalg.svd(A)
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    gamma = s * sg.mean()
    t = b / gamma - R @ mean
    r = rotation_vector(R)
    if not (np.isfinite(r).all() and np.isfinite(t).all()):
        return None, None, ratio
    return r, t, ratio


def resect(p, x, info=None, held=None, groups=None, normalise=True):
    """-> (x with the resected poses written, flag (ncams,): DONE / SKIPPED (a pose component held) / DEGENERATE, lambda_2 /
    lambda_12 per camera (NaN where it was not reached)).  The pose entries of x are not read."""
    x = np.array(x, dtype=np.float64, copy=True)
    sc = cr.Scene(p, x, info)
    C = cr.cameras(p, x)  # a view: written below
    mask = cr.held_mask(p, held, groups)
    flag = np.full(sc.ncams, DEGENERATE, dtype=np.uint8)
    ratio = np.full(sc.ncams, np.nan)
    for c in range(sc.ncams):
        if mask[c, :6].any():
            flag[c] = SKIPPED
            continue
        o = np.flatnonzero((sc.cam0 == c) & sc.used)  # the camera's list, in the caller's order
        r, t, ratio[c] = resect_one(sc.X[o], sc.m[o], C[c, 6], C[c, 7], C[c, 8], normalise)
        if r is not None:
            C[c, :3], C[c, 3:6] = r, t
            flag[c] = DONE
    return x, flag, ratio


def refine(p, x, max_iter=100, xtol=1e-10, lam0=1e-4, loss="linear", c=1.0, info=None, held=None, groups=None, cam_prior=None,
           ctr_prior=None):
    """ba_resect_cameras: the resection, then cameras_ref.refine from its poses; a camera the resection found degenerate comes
    back with the bits of x, DEGENERATE, cost entries 0, no flag, no trial.  Returns what cameras_ref.refine returns."""
    xs, flag, _ = resect(p, x, info, held, groups)
    out, st, cost, trials, D = cr.refine(p, xs, max_iter, xtol, lam0, loss, c, info, held, groups, cam_prior, ctr_prior)
    deg = flag == DEGENERATE
    cr.cameras(p, out)[deg] = cr.cameras(p, np.asarray(x, dtype=np.float64))[deg]
    st = st.copy()
    st[deg] = cr.DEGENERATE
    cost[deg] = 0.0
    trials[deg] = 0
    return out, st, cost, trials, D
