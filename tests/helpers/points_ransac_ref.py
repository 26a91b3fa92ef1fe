"""numpy restatement of ba_ransac_points (include/ba_hip.h, "outlier-robust triangulation") on top of points_ref
(the rays of the linear triangulation, its 3 x 3 solve, the refinement) and ransac_ref (mix, sample, masked_info): the pairs of a
point in rank order or sampled, their two-ray triangulation, the inlier test, the selection, the refits, and the finish as
points_ref.refine(init=1) with the outliers' information set to 0.  Written from the text of the header, not from the kernel."""
import numpy as np

import block_ref as br
import points_ref as pr
import ransac_ref as nr


def defaults(hypotheses=0, refits=-1, min_inliers=0):
    return (128 if hypotheses <= 0 else hypotheses), (2 if refits < 0 else refits), (2 if min_inliers <= 0 else min_inliers)


def ray_sums(sc):
    """per observation: the six packed entries of I - dd' and the three of (I - dd') c of the linear triangulation"""
    q = br.undistort(sc.m, sc.k1, sc.k2, sc.f[:, None])
    v = np.concatenate([q, -np.ones((sc.nobs, 1))], axis=1)
    with np.errstate(all="ignore"):
        d = np.einsum("oji,oj->oi", sc.R, v)
        d /= np.sqrt((d * d).sum(1))[:, None]
        c = -np.einsum("oji,oj->oi", sc.R, sc.t)
        M = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
        return np.stack([M[:, i, j] for i, j in pr._PACK], axis=1), np.einsum("oij,oj->oi", M, c)


def solve_sums(A, b):
    """the 3 x 3 solve of the triangulation on summed rays (n, 6), (n, 3) -> X, ok"""
    return pr.chol3_solve(A, b, 1e-12 * (A[:, 0] + A[:, 2] + A[:, 5]))


def pairs_of(d):
    """the pairs (a, b), a < b, of a list of d entries in rank order: (0,1), (0,2), ..., (0,d-1), (1,2), ..."""
    a, b = np.triu_indices(d, 1)
    return np.stack([a, b], axis=1)


def residual_norms(sc, o, X):
    """(P1.z (n, d), |project - pt2d| (n, d)) of the n points X under the cameras of the d observations o"""
    n, d = len(X), len(o)
    rep = lambda v: np.repeat(v[None], n, axis=0).reshape((n * d,) + v.shape[1:])  # noqa: E731
    with np.errstate(all="ignore"):
        P1, _, _, _, e, _, _ = br.project(rep(sc.R[o]), np.repeat(X, d, axis=0), rep(sc.t[o]), rep(sc.k1[o]), rep(sc.k2[o]), rep(sc.f[o]),
                                          rep(sc.m[o]))
        return P1[:, 2].reshape(n, d), np.sqrt((e * e).sum(1)).reshape(n, d)


def inliers(sc, o, X, tau):
    """the inlier test of the header (a comparison with NaN fails): (n, d) boolean"""
    z, e = residual_norms(sc, o, X)
    with np.errstate(invalid="ignore"):
        return sc.used[o][None, :] & (z < 0) & (e * e <= tau * tau)


def consensus(p, x, threshold, hypotheses=0, refits=-1, min_inliers=0, seed=0, info=None, fixed=None):
    """The consensus stage -> dict: inlier (nobs, bool), n_inliers, best_hyp (npnts), attempted, failed (npnts, bool), counts
    (npnts, H; -1: void), samples (per point a list of H observation-index pairs or None), adopted (npnts: refits adopted),
    margin (npnts: the smallest | |e| / tau - 1 | over the used observations under the linear point on the final set; inf where
    there is none)."""
    H, refits, min_inliers = defaults(hypotheses, refits, min_inliers)
    x = np.array(x, dtype=np.float64, copy=True)
    npnts = p["npnts"]
    x[:3 * npnts] = 0.0  # (the points of x are never read)
    sc = pr.Scene(p, x, info)
    fixed = np.zeros(npnts, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    A_o, b_o = ray_sums(sc)
    out = dict(inlier=np.zeros(sc.nobs, dtype=bool), n_inliers=np.zeros(npnts, dtype=np.int32), best_hyp=np.full(npnts, -1, dtype=np.int32),
               attempted=~fixed, failed=np.zeros(npnts, dtype=bool), counts=np.full((npnts, H), -1, dtype=np.int64),
               samples=[[None] * H for _ in range(npnts)], adopted=np.zeros(npnts, dtype=np.int64), margin=np.full(npnts, np.inf))
    lists = np.split(np.argsort(sc.pnt0, kind="stable"), np.cumsum(sc.deg)[:-1])  # every point's list, in the caller's order
    for i in range(npnts):
        o = lists[i]
        used, d = sc.used[o], len(o)
        if fixed[i]:
            out["inlier"][o] = used
            out["n_inliers"][i] = used.sum()
            continue
        n = d * (d - 1) // 2
        if n <= H:
            pos = [tuple(ab) if used[ab[0]] and used[ab[1]] else None for ab in pairs_of(d)] + [None] * (H - n)
        else:
            pos = [nr.sample(seed, h, d, used, 2) for h in range(H)]
        hs = [h for h in range(H) if pos[h] is not None]
        if hs:
            ab = np.array([pos[h] for h in hs], dtype=np.int64).reshape(-1, 2)
            for h, s in zip(hs, ab):
                out["samples"][i][h] = o[s]
            X, ok = solve_sums(A_o[o[ab[:, 0]]] + A_o[o[ab[:, 1]]], b_o[o[ab[:, 0]]] + b_o[o[ab[:, 1]]])
            cnt = inliers(sc, o, X, threshold).sum(1)
            out["counts"][i, np.array(hs)[ok]] = cnt[ok]
        best = int(np.argmax(out["counts"][i]))  # (the first of the largest: ties go to the lowest h)
        count = int(out["counts"][i, best])
        if count < 0 or count < min_inliers:
            out["failed"][i] = True
            out["n_inliers"][i] = max(count, 0)
            out["best_hyp"][i] = best if count >= 0 else -1
            continue
        M = inliers(sc, o, X[hs.index(best)][None], threshold)[0]
        out["best_hyp"][i] = best
        for _ in range(refits):
            Xr, ok = solve_sums(A_o[o[M]].sum(0)[None], b_o[o[M]].sum(0)[None])
            if not ok[0] or M.sum() < 2:
                break
            M2 = inliers(sc, o, Xr, threshold)[0]
            if M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"][i] += 1
        out["inlier"][o] = M
        out["n_inliers"][i] = M.sum()
        Xr, ok = solve_sums(A_o[o[M]].sum(0)[None], b_o[o[M]].sum(0)[None])
        if ok[0] and used.any():
            e = residual_norms(sc, o, Xr)[1][0][used]
            out["margin"][i] = np.abs(e / threshold - 1.0).min()
    return out


def refine(p, x, threshold, hypotheses=0, refits=-1, min_inliers=0, seed=0, info=None, fixed=None, **kw):
    """ba_ransac_points -> (what points_ref.refine(init=1) returns on the final set, the consensus dict)"""
    con = consensus(p, x, threshold, hypotheses, refits, min_inliers, seed, info, fixed)
    return pr.refine(p, x, init=1, info=nr.masked_info(p, con["inlier"], info), fixed=fixed, **kw), con
