"""numpy restatement of ba_pair_matches and ba_relative_pose (include/ba_hip.h, "relative pose of camera pairs") on
top of ransac_ref.sample / mix, block_ref.undistort and resect_ref.rotation_vector: the match lists from dictionaries, the
undistorted rays, the eight-point fit through np.linalg.eigh and np.linalg.svd (where the kernels run Jacobi sweeps), the
cheirality vote, the inlier test, the selection, the refits and the finish.  Written from the text of the header, not from the
kernels."""
import numpy as np

import block_ref as br
import ransac_ref as nr
import resect_ref as rr

OK, FEW_MATCHES, DEGENERATE, NO_CONSENSUS = range(4)
MIN_MATCHES = 8


def matches(p, pairs):
    """(match_ptr, obs_a, obs_b), 0-based observations, of the pairs (npairs, 2; 1-based cameras): walk a's list in the caller's
    order; an observation is a match iff it is a's first of its point and b observes the point; its partner is b's first"""
    cam0, pnt0 = np.asarray(p["cam_idx1"]) - 1, np.asarray(p["pnt_idx1"]) - 1
    lists = {}
    for o, c in enumerate(cam0):
        lists.setdefault(int(c), []).append(o)
    ptr, oa, ob = [0], [], []
    for a, b in np.asarray(pairs).reshape(-1, 2) - 1:
        first_b = {}
        for o in lists.get(int(b), []):
            first_b.setdefault(int(pnt0[o]), o)
        seen = set()
        for o in lists.get(int(a), []):
            P = int(pnt0[o])
            if P in seen:
                continue
            seen.add(P)
            if P in first_b:
                oa.append(o)
                ob.append(first_b[P])
        ptr.append(len(oa))
    return np.array(ptr, dtype=np.int64), np.array(oa, dtype=np.int64), np.array(ob, dtype=np.int64)


def cameras(p, x):
    return np.asarray(x, dtype=np.float64)[3 * p["npnts"]:].reshape(p["ncams"], 9)


def true_relative(p, x, a, b):
    """(R, unit t, baseline) of cameras a, b (0-based) of x: P_b = R P_a + baseline t"""
    Cm = cameras(p, x)
    Ra, Rb = br.rotations(Cm[[a]])[0], br.rotations(Cm[[b]])[0]
    R = Rb @ Ra.T
    t = Cm[b, 3:6] - R @ Cm[a, 3:6]
    n = np.linalg.norm(t)
    return R, t / n, n


def depths(R, t, qa, qb):
    """(alpha, beta) per match of alpha R d_a + t = beta d_b from its 2 x 2 normal equations, d = (q, -1)"""
    da = np.concatenate([qa, -np.ones((len(qa), 1))], axis=1)
    db = np.concatenate([qb, -np.ones((len(qb), 1))], axis=1)
    u = da @ R.T
    with np.errstate(all="ignore"):
        uu, vv, uv, ut, vt = (u * u).sum(1), (db * db).sum(1), (u * db).sum(1), u @ t, db @ t
        det = uu * vv - uv * uv
        return (uv * vt - ut * vv) / det, (uu * vt - uv * ut) / det


def in_front(R, t, qa, qb):
    al, be = depths(R, t, qa, qb)
    with np.errstate(invalid="ignore"):
        return (al > 0) & (be > 0)


def essential(R, t):
    return br.skew(t[None])[0] @ R


def sampson(R, t, qa, qb, fa, fb):
    """the Sampson distance in pixels^2 per match under E = [t]x R"""
    E = essential(R, t)
    da = np.concatenate([qa, -np.ones((len(qa), 1))], axis=1)
    db = np.concatenate([qb, -np.ones((len(qb), 1))], axis=1)
    with np.errstate(all="ignore"):
        l, m = da @ E.T, db @ E
        num = (db * l).sum(1)
        return num * num / ((l[:, 0] ** 2 + l[:, 1] ** 2) / fb ** 2 + (m[:, 0] ** 2 + m[:, 1] ** 2) / fa ** 2)


def inliers(r, t, qa, qb, used, fa, fb, tau):
    """the inlier test of the header under (r, t): everything from the R and E rebuilt from them (a comparison with NaN fails)"""
    R = br.rotations(np.asarray(r, dtype=np.float64)[None])[0]
    with np.errstate(invalid="ignore"):
        return used & in_front(R, t, qa, qb) & (sampson(R, t, qa, qb, fa, fb) <= tau * tau)


def hartley(q):
    """(c, s) of the image points q about the first of them, or None"""
    with np.errstate(all="ignore"):
        d = q - q[0]
        c = q[0] + d.mean(0)
        rms = np.sqrt(((q - c) ** 2).sum(1).mean())
    if not (rms > 0) or not np.isfinite(rms):
        return None
    return c, np.sqrt(2.0) / rms


def linear_fit(qa, qb):
    """the eight-point fit of the header on the matches (qa, qb), in their order -> (r, t, stats) with r None where it is
    degenerate; stats: ratio = lambda_2 / lambda_9 (NaN if not reached), lead = the winner's cheirality count minus the runner-up's"""
    stats = dict(ratio=np.nan, lead=0)
    if len(qa) == 0:
        return None, None, stats
    ha, hb = hartley(qa), hartley(qb)
    if ha is None or hb is None:
        return None, None, stats
    (ca, sa), (cb, sb) = ha, hb
    n = len(qa)
    da = np.concatenate([sa * (qa - ca), -np.ones((n, 1))], axis=1)
    db = np.concatenate([sb * (qb - cb), -np.ones((n, 1))], axis=1)
    A = (db[:, :, None] * da[:, None, :]).reshape(n, 9)
    M = A.T @ A
    if not np.isfinite(M).all():
        return None, None, stats
    lam, V = np.linalg.eigh(M)
    stats["ratio"] = lam[1] / lam[8]
    if not lam[1] > 1e-10 * lam[8]:
        return None, None, stats
    Ta = np.array([[sa, 0, sa * ca[0]], [0, sa, sa * ca[1]], [0, 0, 1.0]])  # d~ = T d: the third entry of d is -1
    Tb = np.array([[sb, 0, sb * cb[0]], [0, sb, sb * cb[1]], [0, 0, 1.0]])
    E = Tb.T @ V[:, 0].reshape(3, 3) @ Ta
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U[:, 2] *= -1
    if np.linalg.det(Vt) < 0:
        Vt[2] *= -1
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tn = U[:, 2] / np.linalg.norm(U[:, 2])
    cands = [(U @ W @ Vt, tn), (U @ W @ Vt, -tn), (U @ W.T @ Vt, tn), (U @ W.T @ Vt, -tn)]
    cnt = np.array([in_front(R, t, qa, qb).sum() for R, t in cands])
    best = int(np.argmax(cnt))
    stats["lead"] = int(cnt[best] - np.sort(cnt)[-2])
    stats["candidates"] = cands
    if cnt[best] <= 0:
        return None, None, stats
    R, t = cands[best]
    r = rr.rotation_vector(R)
    if not (np.isfinite(r).all() and np.isfinite(t).all()):
        return None, None, stats
    return r, t, stats


def defaults(hypotheses=0, sample_size=0, refits=-1, min_inliers=0):
    H = 128 if hypotheses <= 0 else hypotheses
    m = MIN_MATCHES if sample_size <= 0 else sample_size
    return H, m, (2 if refits < 0 else refits), (max(m, MIN_MATCHES) if min_inliers <= 0 else min_inliers)


def rays(p, x, pairs, info=None):
    """per pair: (q_a, q_b, used, f_a, f_b) of its match list"""
    ptr, oa, ob = matches(p, pairs)
    sc = br.Scene(p, info)
    Cm = cameras(p, x)
    out = []
    for k, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2) - 1):
        ia, ib = oa[ptr[k]:ptr[k + 1]], ob[ptr[k]:ptr[k + 1]]
        qa = br.undistort(sc.m[ia], Cm[a, 6], Cm[a, 7], Cm[a, 8])
        qb = br.undistort(sc.m[ib], Cm[b, 6], Cm[b, 7], Cm[b, 8])
        out.append((qa, qb, sc.used[ia] & sc.used[ib], Cm[a, 8], Cm[b, 8]))
    return ptr, oa, ob, out


def relative_pose(p, x, pairs, threshold=None, hypotheses=0, sample_size=0, refits=-1, min_inliers=0, seed=0, info=None):
    """ba_relative_pose -> dict: status, r, t (NaN where the pair has no pose), match_ptr, inlier (per match), n_inliers, best_hyp;
    and what the conditions of the tests are stated in: counts (npairs, H; -1: void), ratio (npairs, H), samples (per pair a list
    of H position arrays or None), hyp_lead (npairs, H: the cheirality lead of a hypothesis' vote), counts_hi (npairs, H: counts,
    or where that lead is below 3 the largest count any of the four candidates reaches -- what the hypothesis could score if
    rounding turned its vote), runner_lead (per pair the winner's count minus the largest counts_hi of any other hypothesis),
    chain_margin (per pair the smallest | sqrt(sampson) / tau - 1 | over the used matches under the winner's pose and under the
    pose of every refit), lead (per pair the smallest cheirality lead over the refits and the final fit), margin (per pair the smallest | sqrt(sampson) / tau - 1 | over the used matches under the final
    pose; inf where there is none), adopted (refits adopted).  threshold None: no consensus stage."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    H, m, refits, min_inliers = defaults(hypotheses, sample_size, refits, min_inliers)
    if threshold is None:
        H, refits = 0, 0
    n = len(pairs)
    ptr, oa, ob, data = rays(p, x, pairs, info)
    out = dict(status=np.zeros(n, dtype=np.uint8), r=np.full((n, 3), np.nan), t=np.full((n, 3), np.nan), match_ptr=ptr, obs_a=oa, obs_b=ob,
               inlier=np.zeros(ptr[-1], dtype=bool), n_inliers=np.zeros(n, dtype=np.int32), best_hyp=np.full(n, -1, dtype=np.int32),
               counts=np.full((n, H), -1, dtype=np.int64), counts_hi=np.full((n, H), -1, dtype=np.int64),
               hyp_lead=np.full((n, H), 10 ** 9, dtype=np.int64), ratio=np.full((n, H), np.nan), samples=[[None] * H for _ in range(n)],
               runner_lead=np.full(n, 10 ** 9, dtype=np.int64), chain_margin=np.full(n, np.inf),
               lead=np.full(n, 10 ** 9, dtype=np.int64), margin=np.full(n, np.inf), adopted=np.zeros(n, dtype=np.int64))
    def closeness(r, t, qa, qb, used, fa, fb):
        with np.errstate(all="ignore"):
            e = np.sqrt(sampson(br.rotations(r[None])[0], t, qa, qb, fa, fb)[used])
        return np.abs(e / threshold - 1.0).min() if used.any() else np.inf

    for k, (qa, qb, used, fa, fb) in enumerate(data):
        sl = slice(ptr[k], ptr[k + 1])
        if used.sum() < MIN_MATCHES:
            out["status"][k] = FEW_MATCHES
            continue
        if not (np.isfinite(fa) and fa != 0 and np.isfinite(fb) and fb != 0):
            out["status"][k] = DEGENERATE
            continue
        if threshold is None:
            M = used.copy()
        else:
            poses = {}
            for h in range(H):
                s = nr.sample(seed, h, len(qa), used, m)
                if s is None:
                    continue
                out["samples"][k][h] = np.array(s)
                r, t, st = linear_fit(qa[s], qb[s])
                out["ratio"][k, h] = st["ratio"]
                if r is None:
                    continue
                out["hyp_lead"][k, h] = st["lead"]
                poses[h] = (r, t)
                out["counts"][k, h] = out["counts_hi"][k, h] = inliers(r, t, qa, qb, used, fa, fb, threshold).sum()
                if st["lead"] < 3:
                    alt = [inliers(rr.rotation_vector(Rc), tc, qa, qb, used, fa, fb, threshold).sum() for Rc, tc in st["candidates"]]
                    out["counts_hi"][k, h] = max(out["counts_hi"][k, h], max(alt))
            best = int(np.argmax(out["counts"][k]))
            count = int(out["counts"][k, best])
            if count < 0 or count < min_inliers:
                out["status"][k] = NO_CONSENSUS
                out["n_inliers"][k] = max(count, 0)
                out["best_hyp"][k] = best if count >= 0 else -1
                continue
            out["best_hyp"][k] = best
            others = np.delete(out["counts_hi"][k], best)
            if others.size and others.max() >= 0:
                out["runner_lead"][k] = count - others.max()
            out["chain_margin"][k] = closeness(*poses[best], qa, qb, used, fa, fb)
            M = inliers(*poses[best], qa, qb, used, fa, fb, threshold)
            for _ in range(refits):
                r, t, st = linear_fit(qa[M], qb[M])
                if r is None:
                    break
                out["lead"][k] = min(out["lead"][k], st["lead"])
                out["chain_margin"][k] = min(out["chain_margin"][k], closeness(r, t, qa, qb, used, fa, fb))
                M2 = inliers(r, t, qa, qb, used, fa, fb, threshold)
                if M2.sum() < M.sum() or np.array_equal(M2, M):
                    break
                M = M2
                out["adopted"][k] += 1
        out["inlier"][sl] = M
        out["n_inliers"][k] = M.sum()
        r, t, st = linear_fit(qa[M], qb[M])
        if r is None:
            out["status"][k] = DEGENERATE
            continue
        out["lead"][k] = min(out["lead"][k], st["lead"])
        out["r"][k], out["t"][k] = r, t
        if threshold is not None:
            out["margin"][k] = closeness(r, t, qa, qb, used, fa, fb)
    return out


def pose_error(r, t, r_ref, t_ref):
    """|R - R_ref|_F + |t - t_ref| per pair"""
    R, Rr = br.rotations(np.atleast_2d(r)), br.rotations(np.atleast_2d(r_ref))
    return np.sqrt(((R - Rr) ** 2).sum(axis=(1, 2))) + np.linalg.norm(np.atleast_2d(t) - np.atleast_2d(t_ref), axis=1)
