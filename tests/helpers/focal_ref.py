"""numpy restatement of ba_resect_cameras_focal and ba_ransac_cameras_focal (include/ba_hip.h, "camera resection with unknown
focal length") on top of resect_ref, ransac_ref and cameras_ref: which cameras run in focal mode, the image scale, the
normal matrix on raw measurements, phi from the row norms of the eigenvector, the pose through the steps of resect_ref, the
write-back, and the consensus stage whose hypotheses carry their own f.  Written from the text of the header, not from the
kernels: np.linalg.eigh and np.linalg.svd where the kernels run Jacobi sweeps."""
import numpy as np

import cameras_ref as cr
import ransac_ref as nr
import resect_ref as rr

DONE, SKIPPED, DEGENERATE = rr.DONE, rr.SKIPPED, rr.DEGENERATE
K1, K2, F = 6, 7, 8


def focal_mode(mask):
    """boolean (ncams,): the pose is free and f is free (mask: cameras_ref.held_mask, the groups' intrinsics included)"""
    return ~mask[:, :6].any(axis=1) & ~mask[:, F]


def resect_one(X, m):
    """(r, t, f, lambda_2 / lambda_12) of one focal-mode camera from its used points X (n, 3) and raw measurements m (n, 2);
    r is None: degenerate"""
    none = (None, None, None)
    if len(X) < rr.MIN_OBS:
        return none + (np.nan,)
    with np.errstate(all="ignore"):
        a = np.sqrt((m * m).sum() / len(m))
        if not np.isfinite(a) or a == 0:
            return none + (np.nan,)
        u = m / a
        mean = X[0] + (X - X[0]).mean(0)
        rms = np.sqrt((((X - mean) ** 2).sum(1)).mean())
        if not (rms > 0) or not np.isfinite(rms):
            return none + (np.nan,)
        s = 1.0 / rms
        Xn = s * (X - mean)
        M = rr.moments(Xn, u)
    if not np.isfinite(M).all():
        return none + (np.nan,)
    lam, V = np.linalg.eigh(M)
    ratio = lam[1] / lam[11]
    if not lam[1] > 1e-10 * lam[11]:
        return none + (ratio,)
    P = V[:, 0].reshape(3, 4).copy()
    with np.errstate(all="ignore"):
        phi = np.sqrt(((P[0, :3] ** 2).sum() + (P[1, :3] ** 2).sum()) / (2.0 * (P[2, :3] ** 2).sum()))
    if not np.isfinite(phi) or not phi > 0:
        return none + (ratio,)
    P[:2] /= phi
    A, b = P[:, :3], P[:, 3]
    if 2 * (Xn @ A[2] + b[2] < 0).sum() < len(X):
        A, b = -A, -b
    U, sg, Vt = np.linalg.svd(A)
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    t = b / (s * sg.mean()) - R @ mean
    r = rr.rotation_vector(R)
    if not (np.isfinite(r).all() and np.isfinite(t).all()):
        return none + (ratio,)
    return r, t, a * phi, ratio


def solve_camera(X, m, C9, mask9):
    """The camera a resection on (X, m) writes for a camera with the entries C9 of x and the mask mask9 (its pose free), or None:
    focal mode -- pose and f from resect_one, a free k1 / k2 as 0, a held one kept -- or the calibrated resection with the
    intrinsics of C9.  -> (camera (9,) or None, lambda_2 / lambda_12)"""
    out = np.array(C9, dtype=np.float64, copy=True)
    if mask9[F]:
        r, t, ratio = rr.resect_one(X, m, C9[K1], C9[K2], C9[F])
    else:
        r, t, f, ratio = resect_one(X, m)
        if r is not None:
            out[K1], out[K2] = (C9[K1] if mask9[K1] else 0.0), (C9[K2] if mask9[K2] else 0.0)
            out[F] = f
    if r is None:
        return None, ratio
    out[:3], out[3:6] = r, t
    return out, ratio


def resect(p, x, info=None, held=None, groups=None):
    """-> (x with the resected cameras written, flag (ncams,): DONE / SKIPPED / DEGENERATE, lambda_2 / lambda_12 per camera)"""
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
        cam, ratio[c] = solve_camera(sc.X[o], sc.m[o], C[c], mask[c])
        if cam is not None:
            C[c] = cam
            flag[c] = DONE
    return x, flag, ratio


def refine(p, x, max_iter=100, xtol=1e-10, lam0=1e-4, loss="linear", c=1.0, info=None, held=None, groups=None, cam_prior=None,
           ctr_prior=None):
    """ba_resect_cameras_focal: the resection, then cameras_ref.refine from its cameras; a camera the resection found degenerate
    comes back with the bits of x, DEGENERATE, cost entries 0, no flag, no trial.  Returns what cameras_ref.refine returns."""
    xs, flag, _ = resect(p, x, info, held, groups)
    deg = flag == DEGENERATE
    out, st, cost, trials, D = cr.refine(p, xs, max_iter, xtol, lam0, loss, c, info, held, groups, cam_prior, ctr_prior)
    cr.cameras(p, out)[deg] = cr.cameras(p, np.asarray(x, dtype=np.float64))[deg]
    st = st.copy()
    st[deg] = cr.DEGENERATE
    cost[deg] = 0.0
    trials[deg] = 0
    return out, st, cost, trials, D


def consensus(p, x, threshold, hypotheses=0, sample_size=0, refits=-1, min_inliers=0, seed=0, info=None, held=None, groups=None):
    """The consensus stage of ba_ransac_cameras_focal -> the dict of ransac_ref.consensus, and `f_best` (ncams: the f^ of the
    winning hypothesis, NaN where there is none)."""
    H, m, refits, min_inliers = nr.defaults(hypotheses, sample_size, refits, min_inliers)
    sc = cr.Scene(p, x, info)
    C = cr.cameras(p, x)
    mask = cr.held_mask(p, held, groups)
    nc = sc.ncams
    out = dict(inlier=np.zeros(sc.nobs, dtype=bool), n_inliers=np.zeros(nc, dtype=np.int32), best_hyp=np.full(nc, -1, dtype=np.int32),
               attempted=np.zeros(nc, dtype=bool), failed=np.zeros(nc, dtype=bool), counts=np.full((nc, H), -1, dtype=np.int64),
               ratio=np.full((nc, H), np.nan), samples=[[None] * H for _ in range(nc)], adopted=np.zeros(nc, dtype=np.int64),
               margin=np.full(nc, np.inf), f_best=np.full(nc, np.nan))
    for c in range(nc):
        o = np.flatnonzero(sc.cam0 == c)  # the camera's list, in the caller's order
        used = sc.used[o]
        if mask[c, :6].any():
            out["inlier"][o] = used
            out["n_inliers"][c] = used.sum()
            continue
        out["attempted"][c] = True
        X, m2d = sc.X[o], sc.m[o]
        cams = {}
        for h in range(H):
            s = nr.sample(seed, h, len(o), used, m)
            if s is None:
                continue
            out["samples"][c][h] = o[s]
            cam, out["ratio"][c, h] = solve_camera(X[s], m2d[s], C[c], mask[c])
            if cam is None:
                continue
            cams[h] = cam
            out["counts"][c, h] = nr.inliers(X, m2d, used, cam, threshold).sum()
        best = int(np.argmax(out["counts"][c]))  # (the first of the largest: ties go to the lowest h)
        count = int(out["counts"][c, best])
        if count < 0 or count < min_inliers:
            out["failed"][c] = True
            out["n_inliers"][c] = max(count, 0)
            out["best_hyp"][c] = best if count >= 0 else -1
            continue
        M = nr.inliers(X, m2d, used, cams[best], threshold)
        out["best_hyp"][c], out["f_best"][c] = best, cams[best][F]
        for _ in range(refits):
            cam, _ratio = solve_camera(X[M], m2d[M], C[c], mask[c])
            if cam is None:
                break
            M2 = nr.inliers(X, m2d, used, cam, threshold)
            if M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"][c] += 1
        out["inlier"][o] = M
        out["n_inliers"][c] = M.sum()
        cam, _ratio = solve_camera(X[M], m2d[M], C[c], mask[c])
        if cam is not None and used.any():
            e = nr.residual_norms(X, m2d, cam)[1][used]
            out["margin"][c] = np.abs(e / threshold - 1.0).min()
    return out


def refine_ransac(p, x, threshold, hypotheses=0, sample_size=0, refits=-1, min_inliers=0, seed=0, info=None, **kw):
    """ba_ransac_cameras_focal -> (what refine returns on the final set, the consensus dict)"""
    con = consensus(p, x, threshold, hypotheses, sample_size, refits, min_inliers, seed, info, kw.get("held"), kw.get("groups"))
    return refine(p, x, info=nr.masked_info(p, con["inlier"], info), **kw), con
