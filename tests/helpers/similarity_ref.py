"""numpy restatement of ba_similarity (include/ba_hip.h, "similarity alignment of reconstructions"): the used rows, the
fit of a set from its 16 sums about the first row (np.linalg.svd where the kernels run the one-sided Jacobi), the inlier test, the
sampling of ransac_ref.sample, the selection and the refits.  Written from the text of the header, not from the kernels."""
import numpy as np

from ransac_ref import sample

STATES = ("ok", "few_rows", "degenerate", "no_consensus")


def rotation_of(v):
    """the rotation matrix of a rotation vector (the model's formula)"""
    v = np.asarray(v, dtype=np.float64)
    th = np.sqrt(v @ v)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * np.outer(k, k)


def rotation_vector(R):
    """the rule of ba_resect_cameras"""
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


def used_rows(src, dst, used=None):
    """a row is used iff its byte says so (None: all) and its six numbers are finite"""
    fin = np.isfinite(src).all(axis=1) & np.isfinite(dst).all(axis=1)
    return fin if used is None else fin & (np.asarray(used) != 0)


def fit(src, dst, scale=True):
    """The fit of the rows src, dst (m, 3) in their order (the first is the origin of the sums) -> (s, R, t), or None:
    degenerate"""
    m = len(src)
    with np.errstate(all="ignore"):
        a, b = src - src[0], dst - dst[0]
        Sa, Sb, Saa, Sba = a.sum(0), b.sum(0), (a * a).sum(), b.T @ a
        if not (np.isfinite(Sa).all() and np.isfinite(Sb).all() and np.isfinite(Saa) and np.isfinite(Sba).all()):
            return None
        ma, mb = Sa / m, Sb / m
        va = Saa - m * (ma @ ma)
        if not va > 0:
            return None
        K = Sba - m * np.outer(mb, ma)
        try:
            U, sg, Vt = np.linalg.svd(K)
        except np.linalg.LinAlgError:
            return None
        if not np.isfinite(sg).all() or not sg[1] > 1e-10 * sg[0]:
            return None
        d = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
        R = U @ np.diag([1.0, 1.0, d]) @ Vt
        s = (sg[0] + sg[1] + d * sg[2]) / va if scale else 1.0
        if not np.isfinite(s) or not s > 0:
            return None
        t = (dst[0] + mb) - s * (R @ (src[0] + ma))
    return s, R, t


def residuals(src, dst, f):
    """|s R src + t - dst| per row"""
    s, R, t = f
    with np.errstate(all="ignore"):
        e = s * (src @ R.T) + t - dst
        return np.sqrt((e * e).sum(axis=1))


def inliers(src, dst, used, f, tau):
    """the inlier test of the header (a comparison with NaN fails)"""
    with np.errstate(invalid="ignore"):
        return used & (residuals(src, dst, f) ** 2 <= tau * tau)


def defaults(hypotheses=0, sample_size=0, refits=-1, min_inliers=0):
    H = 128 if hypotheses <= 0 else hypotheses
    m = 3 if sample_size <= 0 else sample_size
    return H, m, (2 if refits < 0 else refits), (max(m, 3) if min_inliers <= 0 else min_inliers)


def margin_of(src, dst, used, f, tau):
    """the smallest | |e| / tau - 1 | over the used rows under a fit (inf where there is none)"""
    if f is None or not used.any():
        return np.inf
    return float(np.abs(residuals(src[used], dst[used], f) / tau - 1.0).min())


def one(src, dst, used=None, ransac=None, scale=True):
    """ba_similarity on one problem -> dict: status (a name), s, R, r, t (NaN where not ok), inlier (n, bool), n_inliers, best_hyp,
    rms, adopted (refits adopted), margin (the smallest | |e| / tau - 1 | over the used rows under every valid hypothesis, every
    refit and the final fit; inf without ransac), margin_main (the same without the hypotheses that did not win)"""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    n = len(src)
    u = used_rows(src, dst, used)
    out = dict(status="ok", s=np.nan, R=np.full((3, 3), np.nan), r=np.full(3, np.nan), t=np.full(3, np.nan), inlier=np.zeros(n, dtype=bool),
               n_inliers=0, best_hyp=-1, rms=np.nan, adopted=0, margin=np.inf, margin_main=np.inf)
    if u.sum() < 3:
        return dict(out, status="few_rows")
    if ransac is None:
        M = u.copy()
    else:
        tau, seed = float(ransac["threshold"]), int(ransac.get("seed", 0) or 0)
        H, m, refits, min_inliers = defaults(ransac.get("hypotheses", 0) or 0, ransac.get("sample", 0) or 0,
                                             -1 if ransac.get("refits") is None else ransac["refits"], ransac.get("min_inliers", 0) or 0)
        counts, fits = np.full(H, -1, dtype=np.int64), {}
        for h in range(H):
            pos = sample(seed, h, n, u, m)
            if pos is None:
                continue
            f = fit(src[pos], dst[pos], scale)
            if f is None:
                continue
            fits[h] = f
            counts[h] = inliers(src, dst, u, f, tau).sum()
            out["margin"] = min(out["margin"], margin_of(src, dst, u, f, tau))
        best = int(np.argmax(counts))  # (the first of the largest: ties go to the lowest h)
        count = int(counts[best])
        if count < 0 or count < min_inliers:
            return dict(out, status="no_consensus", n_inliers=max(count, 0), best_hyp=best if count >= 0 else -1)
        out["best_hyp"] = best
        out["margin_main"] = margin_of(src, dst, u, fits[best], tau)
        M = inliers(src, dst, u, fits[best], tau)
        for _ in range(refits):
            f = fit(src[M], dst[M], scale)
            if f is None:
                break
            out["margin_main"] = min(out["margin_main"], margin_of(src, dst, u, f, tau))
            M2 = inliers(src, dst, u, f, tau)
            if M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"] += 1
    out["inlier"], out["n_inliers"] = M, int(M.sum())
    f = fit(src[M], dst[M], scale)
    if f is None:
        return dict(out, status="degenerate")
    if ransac is not None:
        out["margin_main"] = min(out["margin_main"], margin_of(src, dst, u, f, float(ransac["threshold"])))
        out["margin"] = min(out["margin"], out["margin_main"])
    e = residuals(src[M], dst[M], f)
    return dict(out, s=f[0], R=f[1], r=rotation_vector(f[1]), t=f[2], rms=float(np.sqrt((e * e).sum() / M.sum())))


def many(src, dst, offsets=None, used=None, ransac=None, scale=True):
    """ba_similarity -> the list of `one` per problem"""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    offsets = np.array([0, len(src)]) if offsets is None else np.asarray(offsets)
    return [one(src[a:b], dst[a:b], None if used is None else np.asarray(used)[a:b], ransac, scale) for a, b in zip(offsets[:-1], offsets[1:])]
