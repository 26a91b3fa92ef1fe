"""numpy restatement of ba_ransac_cameras (include/ba_hip.h, "outlier-robust camera resection") on top of
resect_ref.resect_one and cameras_ref.refine: the sampling in Python integers, the hypothesis poses through np.linalg.eigh, the
inlier test, the selection, the refits, and the finish as resect_ref.refine with the outliers' information set to 0.  Written
from the text of the header, not from the kernels."""
import numpy as np

import block_ref as br
import cameras_ref as cr
import resect_ref as rr

M64 = (1 << 64) - 1
DRAWS = 64


def mix(z):
    """splitmix64"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, h, degree, used, m):
    """the list positions hypothesis h samples in a list of `degree` entries (used: boolean per position, or None), in the
    order of their draws, or None: void"""
    key = mix(mix(seed) ^ h)
    out = []
    for j in range(DRAWS):
        if degree <= 0:
            break
        pos = ((mix(key ^ j) >> 32) * degree) >> 32
        if (used is not None and not used[pos]) or pos in out:
            continue
        out.append(pos)
        if len(out) == m:
            return out
    return None


def residual_norms(X, m2d, C9):
    """(P1.z, |project - pt2d| in pixels) of the points X (n, 3) and measurements m2d (n, 2) under the camera C9"""
    n = len(X)
    with np.errstate(all="ignore"):
        R = np.repeat(cr.rotations(C9[None, :3]), n, axis=0)
        P1, _, _, _, e, _, _ = br.project(R, X, np.repeat(C9[None, 3:6], n, axis=0), np.full(n, C9[6]), np.full(n, C9[7]), np.full(n, C9[8]), m2d)
        return P1[:, 2], np.sqrt((e * e).sum(1))


def inliers(X, m2d, used, C9, tau):
    """the inlier test of the header (a comparison with NaN fails)"""
    z, e = residual_norms(X, m2d, C9)
    with np.errstate(invalid="ignore"):
        return used & (z < 0) & (e * e <= tau * tau)


def defaults(hypotheses=0, sample_size=0, refits=-1, min_inliers=0):
    H = 128 if hypotheses <= 0 else hypotheses
    m = 6 if sample_size <= 0 else sample_size
    return H, m, (2 if refits < 0 else refits), (max(m, 6) if min_inliers <= 0 else min_inliers)


def consensus(p, x, threshold, hypotheses=0, sample_size=0, refits=-1, min_inliers=0, seed=0, info=None, held=None, groups=None):
    """The consensus stage -> dict: inlier (nobs, bool), n_inliers, best_hyp (ncams), attempted, failed (ncams, bool), counts
    (ncams, H; -1: void), ratio (ncams, H: lambda_2 / lambda_12 of a hypothesis, NaN where it was not reached), samples (per
    camera a list of H observation-index arrays or None), adopted (ncams: refits adopted), margin (ncams: the smallest
    | |e| / tau - 1 | over the used observations under the linear pose on the final set; inf where there is none)."""
    H, m, refits, min_inliers = defaults(hypotheses, sample_size, refits, min_inliers)
    sc = cr.Scene(p, x, info)
    C = cr.cameras(p, x)
    mask = cr.held_mask(p, held, groups)
    nc = sc.ncams
    out = dict(inlier=np.zeros(sc.nobs, dtype=bool), n_inliers=np.zeros(nc, dtype=np.int32), best_hyp=np.full(nc, -1, dtype=np.int32),
               attempted=np.zeros(nc, dtype=bool), failed=np.zeros(nc, dtype=bool), counts=np.full((nc, H), -1, dtype=np.int64),
               ratio=np.full((nc, H), np.nan), samples=[[None] * H for _ in range(nc)], adopted=np.zeros(nc, dtype=np.int64),
               margin=np.full(nc, np.inf))
    for c in range(nc):
        o = np.flatnonzero(sc.cam0 == c)  # the camera's list, in the caller's order
        used = sc.used[o]
        if mask[c, :6].any():
            out["inlier"][o] = used
            out["n_inliers"][c] = used.sum()
            continue
        out["attempted"][c] = True
        X, m2d, (k1, k2, f) = sc.X[o], sc.m[o], C[c, 6:]
        poses = {}
        for h in range(H):
            s = sample(seed, h, len(o), used, m)
            if s is None:
                continue
            out["samples"][c][h] = o[s]
            r, t, out["ratio"][c, h] = rr.resect_one(X[s], m2d[s], k1, k2, f)
            if r is None:
                continue
            poses[h] = np.concatenate([r, t, [k1, k2, f]])
            out["counts"][c, h] = inliers(X, m2d, used, poses[h], threshold).sum()
        best = int(np.argmax(out["counts"][c]))  # (the first of the largest: ties go to the lowest h)
        count = int(out["counts"][c, best])
        if count < 0 or count < min_inliers:
            out["failed"][c] = True
            out["n_inliers"][c] = max(count, 0)
            out["best_hyp"][c] = best if count >= 0 else -1
            continue
        M = inliers(X, m2d, used, poses[best], threshold)
        out["best_hyp"][c] = best
        for _ in range(refits):
            r, t, _ratio = rr.resect_one(X[M], m2d[M], k1, k2, f)
            if r is None:
                break
            M2 = inliers(X, m2d, used, np.concatenate([r, t, [k1, k2, f]]), threshold)
            if M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"][c] += 1
        out["inlier"][o] = M
        out["n_inliers"][c] = M.sum()
        r, t, _ratio = rr.resect_one(X[M], m2d[M], k1, k2, f)
        if r is not None and used.any():
            e = residual_norms(X, m2d, np.concatenate([r, t, [k1, k2, f]]))[1][used]
            out["margin"][c] = np.abs(e / threshold - 1.0).min()
    return out


def masked_info(p, inlier, info=None):
    """(nobs, 2, 2) information matrices: the caller's (the identity when None) on the inliers, 0 elsewhere"""
    full = np.tile(np.eye(2), (p["nobs"], 1, 1)) if info is None else np.array(info, dtype=np.float64, copy=True)
    full[~np.asarray(inlier, dtype=bool)] = 0.0
    return full


def refine(p, x, threshold, hypotheses=0, sample_size=0, refits=-1, min_inliers=0, seed=0, info=None, **kw):
    """ba_ransac_cameras -> (what resect_ref.refine returns on the final set, the consensus dict)"""
    con = consensus(p, x, threshold, hypotheses, sample_size, refits, min_inliers, seed, info, kw.get("held"), kw.get("groups"))
    return rr.refine(p, x, info=masked_info(p, con["inlier"], info), **kw), con
