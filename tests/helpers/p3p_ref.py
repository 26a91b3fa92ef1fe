"""numpy restatement of ba_p3p and ba_ransac_cameras_p3p (include/ba_hip.h, "P3P minimal samples"): the quartic of
the header with np.roots where the kernel runs the Aberth-Ehrlich iteration, the same polishing steps, the frames, and the
consensus stage on top of ransac_ref (its sampling, inlier test, selection and refits).  Written from the text of the header,
not from the kernels."""
import numpy as np

import cameras_ref as cr
import ransac_ref as nr
import resect_ref as rr
from block_ref import undistort

MAX_SOL = 4


def rays(q):
    """unit rays (q, -1) / |(q, -1)| of the undistorted image points q (3, 2)"""
    d = np.concatenate([q, -np.ones((len(q), 1))], axis=1)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def quartic(q, X):
    """-> (coefficients ascending in v, the dict of what the later steps need), or (None, None): 0 solutions by the geometry"""
    j = rays(q)
    a, b, c = np.linalg.norm(X[1] - X[2]), np.linalg.norm(X[0] - X[2]), np.linalg.norm(X[0] - X[1])
    if not (np.isfinite([a, b, c]).all() and a > 0 and b > 0 and c > 0):
        return None, None
    if not np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0])) > 1e-12 * c * b:
        return None, None
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    A, B = c * c / (b * b), a * a / (b * b)
    P = np.polynomial.polynomial
    w = np.array([1.0, -2.0 * cb, 1.0])
    c1 = np.array([1.0, 0.0, 0.0]) - A * w
    c2 = np.array([0.0, 0.0, 1.0]) - B * w
    b1, b2 = np.array([-2.0 * cg]), np.array([0.0, -2.0 * ca])
    D = c2 - c1
    Q = P.polysub(P.polymul(D, D), P.polymul(P.polysub(b2, b1), P.polysub(P.polymul(b1, c2), P.polymul(b2, c1))))
    Q = np.concatenate([Q, np.zeros(5 - len(Q))])
    return Q, dict(j=j, a=a, b=b, c=c, ca=ca, cb=cb, cg=cg, A=A, B=B)


def real_roots(Q):
    """the real roots of the quartic (|Im| <= 1e-7 |z|), two Newton steps each, ascending"""
    if not np.isfinite(Q).all() or Q[4] == 0:
        return np.zeros(0)
    z = np.roots(Q[::-1])
    z = z[np.isfinite(z)]
    out = []
    for v in z[np.abs(z.imag) <= 1e-7 * np.abs(z)].real:
        for _ in range(2):
            p = np.polynomial.polynomial.polyval(v, Q)
            d = np.polynomial.polynomial.polyval(v, np.polynomial.polynomial.polyder(Q))
            with np.errstate(all="ignore"):
                step = p / d
            if np.isfinite(step):
                v = v - step
        out.append(v)
    return np.sort(np.array(out))


def frame(p1, p2, p3):
    """the orthonormal frame of (p2 - p1, p3 - p1), as columns"""
    e1 = (p2 - p1) / np.linalg.norm(p2 - p1)
    e3 = np.cross(e1, p3 - p1)
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def depth_ratio(g, v):
    """u = s2 / s1 at the root v"""
    w = v * v - 2.0 * g["cb"] * v + 1.0
    c1, c2 = 1.0 - g["A"] * w, v * v - g["B"] * w
    den = -2.0 * g["cg"] + 2.0 * g["ca"] * v
    with np.errstate(all="ignore"):
        u = (c2 - c1) / den
    if den == 0 or not np.isfinite(u):
        sq = np.sqrt(max(g["cg"] ** 2 - c1, 0.0))
        ua, ub = g["cg"] + sq, g["cg"] - sq
        second = lambda t: abs(t * t - 2.0 * g["ca"] * v * t + c2)  # noqa: E731
        u = ub if second(ub) < second(ua) else ua
    return u, w


def solve(q, X, details=False):
    """ba_p3p on one problem: q (3, 2) undistorted image points divided by f, X (3, 3) -> poses (n_sol, 6) in ascending order
    of the quartic's root (details: also the real roots and the depth ratios u of every real root)"""
    q, X = np.asarray(q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    none = (np.zeros((0, 6)), np.zeros(0), np.zeros(0)) if details else np.zeros((0, 6))
    with np.errstate(all="ignore"):
        Q, g = quartic(q, X)
        if Q is None:
            return none
        vs = real_roots(Q)
        poses, us = [], []
        Fw = frame(X[0], X[1], X[2])
        for v in vs:
            u, w = depth_ratio(g, v)
            us.append(u)
            if not (v > 0 and u > 0):
                continue
            s = np.array([1.0, u, v]) * (g["b"] / np.sqrt(w))
            for _ in range(2):
                f = np.array([s[1] ** 2 + s[2] ** 2 - 2 * g["ca"] * s[1] * s[2] - g["a"] ** 2,
                              s[0] ** 2 + s[2] ** 2 - 2 * g["cb"] * s[0] * s[2] - g["b"] ** 2,
                              s[0] ** 2 + s[1] ** 2 - 2 * g["cg"] * s[0] * s[1] - g["c"] ** 2])
                J = 2.0 * np.array([[0.0, s[1] - g["ca"] * s[2], s[2] - g["ca"] * s[1]],
                                    [s[0] - g["cb"] * s[2], 0.0, s[2] - g["cb"] * s[0]],
                                    [s[0] - g["cg"] * s[1], s[1] - g["cg"] * s[0], 0.0]])
                try:
                    step = np.linalg.solve(J, f)
                except np.linalg.LinAlgError:
                    continue
                if np.isfinite(step).all():
                    s = s - step
            Y = s[:, None] * g["j"]
            R = frame(Y[0], Y[1], Y[2]) @ Fw.T
            pose = np.concatenate([rr.rotation_vector(R), Y[0] - R @ X[0]])
            if np.isfinite(pose).all():
                poses.append(pose)
    poses = np.array(poses).reshape(-1, 6)
    return (poses, vs, np.array(us)) if details else poses


def comparable_triple(q, X):
    """the rule of the header's test: the real roots pairwise apart by more than 1e-3 (relative) and no depth ratio (u, v) of a
    real root within 1e-6 of 0"""
    _, vs, us = solve(q, X, details=True)
    for i in range(len(vs)):
        for k in range(i):
            if abs(vs[i] - vs[k]) <= 1e-3 * max(abs(vs[i]), abs(vs[k])):
                return False
    return not (np.abs(vs) <= 1e-6).any() and not (np.abs(us) <= 1e-6).any()


def project_q(pose, X):
    """the undistorted image points -P.xy / P.z of the points X under (r, t), and P.z"""
    R = cr.rotations(pose[None, :3])[0]
    P = X @ R.T + pose[3:6]
    return -P[:, :2] / P[:, 2:3], P[:, 2]


def consensus(p, x, threshold, hypotheses=0, refits=-1, min_inliers=0, seed=0, info=None, held=None, groups=None):
    """The consensus stage of ba_ransac_cameras_p3p -> the dict of ransac_ref.consensus (no ratio; margin as there); counts is the
    best candidate's count of a hypothesis, n_cand (ncams, H) the number of candidates"""
    H, _, refits, min_inliers = nr.defaults(hypotheses, 6, refits, min_inliers)
    sc = cr.Scene(p, x, info)
    C = cr.cameras(p, x)
    mask = cr.held_mask(p, held, groups)
    nc = sc.ncams
    out = dict(inlier=np.zeros(sc.nobs, dtype=bool), n_inliers=np.zeros(nc, dtype=np.int32), best_hyp=np.full(nc, -1, dtype=np.int32),
               attempted=np.zeros(nc, dtype=bool), failed=np.zeros(nc, dtype=bool), counts=np.full((nc, H), -1, dtype=np.int64),
               n_cand=np.zeros((nc, H), dtype=np.int64), samples=[[None] * H for _ in range(nc)], adopted=np.zeros(nc, dtype=np.int64),
               margin=np.full(nc, np.inf))
    for c in range(nc):
        o = np.flatnonzero(sc.cam0 == c)
        used = sc.used[o]
        if mask[c, :6].any():
            out["inlier"][o] = used
            out["n_inliers"][c] = used.sum()
            continue
        out["attempted"][c] = True
        X, m2d, (k1, k2, f) = sc.X[o], sc.m[o], C[c, 6:]
        poses = {}
        for h in range(H):
            if not np.isfinite(f) or f == 0:
                break
            s = nr.sample(seed, h, len(o), used, 3)
            if s is None:
                continue
            out["samples"][c][h] = o[s]
            with np.errstate(all="ignore"):
                cands = solve(undistort(m2d[s], k1, k2, f), X[s])
            out["n_cand"][c, h] = len(cands)
            for cand in cands:
                C9 = np.concatenate([cand, [k1, k2, f]])
                n = nr.inliers(X, m2d, used, C9, threshold).sum()
                if n > out["counts"][c, h]:
                    out["counts"][c, h], poses[h] = n, C9
        best = int(np.argmax(out["counts"][c]))
        count = int(out["counts"][c, best])
        if count < 0 or count < min_inliers:
            out["failed"][c] = True
            out["n_inliers"][c] = max(count, 0)
            out["best_hyp"][c] = best if count >= 0 else -1
            continue
        M = nr.inliers(X, m2d, used, poses[best], threshold)
        out["best_hyp"][c] = best
        for _ in range(refits):
            r, t, _ratio = rr.resect_one(X[M], m2d[M], k1, k2, f)
            if r is None:
                break
            M2 = nr.inliers(X, m2d, used, np.concatenate([r, t, [k1, k2, f]]), threshold)
            if M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"][c] += 1
        out["inlier"][o] = M
        out["n_inliers"][c] = M.sum()
        r, t, _ratio = rr.resect_one(X[M], m2d[M], k1, k2, f)
        if r is not None and used.any():
            e = nr.residual_norms(X, m2d, np.concatenate([r, t, [k1, k2, f]]))[1][used]
            out["margin"][c] = np.abs(e / threshold - 1.0).min()
    return out


def refine(p, x, threshold, hypotheses=0, refits=-1, min_inliers=0, seed=0, info=None, **kw):
    """ba_ransac_cameras_p3p -> (what resect_ref.refine returns on the final set, the consensus dict)"""
    con = consensus(p, x, threshold, hypotheses, refits, min_inliers, seed, info, kw.get("held"), kw.get("groups"))
    return rr.refine(p, x, info=nr.masked_info(p, con["inlier"], info), **kw), con
