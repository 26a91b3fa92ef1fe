"""numpy restatement of ba_homography, ba_decompose_homography, ba_homography_pose and of two_view (include/ba_hip.h, "homography
of camera pairs"): the linear fit through np.linalg.eigh and np.linalg.svd (where the kernels run Jacobi sweeps),
the transfer-error test, the selection, the refits and the finish, the four solutions of the decomposition, the plane vote and
the supports, the model of a pair and the seed order.  The sampler is ransac_ref.sample; the rays, the matches and the Sampson
test are pair_ref's.  Written from the text of the header, not from the kernels."""
import numpy as np

import block_ref as br
import pair_ref as pf
import ransac_ref as nr
import resect_ref as rr

OK, FEW_MATCHES, DEGENERATE, NO_CONSENSUS = range(4)
MIN_MATCHES = 4


def rays3(q):
    return np.concatenate([q, -np.ones((len(q), 1))], axis=1)


def cross_matrix(d):
    return np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def linear_fit(qa, qb, force=False):
    """the fit of the header on the matches (qa, qb), in their order -> (H or None, stats); stats: ratio = lambda_2 / lambda_9 and
    sigma = sigma_3 / sigma_1 (NaN where not reached), vote = |2 pos - n| of the sign vote.  force: the two limits on those
    ratios are not applied (what a fit next to a limit would give on the other side of it)"""
    stats = dict(ratio=np.nan, sigma=np.nan, vote=0)
    if len(qa) == 0:
        return None, stats
    ha, hb = pf.hartley(qa), pf.hartley(qb)
    if ha is None or hb is None:
        return None, stats
    (ca, sa), (cb, sb) = ha, hb
    n = len(qa)
    da = np.concatenate([sa * (qa - ca), -np.ones((n, 1))], axis=1)
    db = np.concatenate([sb * (qb - cb), -np.ones((n, 1))], axis=1)
    A = np.concatenate([np.kron(cross_matrix(db[i]), da[i][None, :]) for i in range(n)], axis=0)
    M = A.T @ A
    if not np.isfinite(M).all():
        return None, stats
    lam, V = np.linalg.eigh(M)
    stats["ratio"] = lam[1] / lam[8]
    if not lam[1] > 1e-10 * lam[8] and not force:
        return None, stats
    Ta = np.array([[sa, 0, sa * ca[0]], [0, sa, sa * ca[1]], [0, 0, 1.0]])
    Tb = np.array([[sb, 0, sb * cb[0]], [0, sb, sb * cb[1]], [0, 0, 1.0]])
    H = np.linalg.inv(Tb) @ V[:, 0].reshape(3, 3) @ Ta
    if not np.isfinite(H).all():
        return None, stats
    sg = np.linalg.svd(H, compute_uv=False)
    stats["sigma"] = sg[2] / sg[0]
    if not np.isfinite(sg).all() or not (sg[2] > 1e-6 * sg[0] or force) or not sg[1] > 0:
        return None, stats
    H = H / sg[1]
    with np.errstate(invalid="ignore"):
        pos = int((np.einsum("ni,ij,nj->n", rays3(qb), H, rays3(qa)) > 0).sum())
    stats["vote"] = abs(2 * pos - n)
    if 2 * pos < n or (2 * pos == n and np.linalg.det(H) < 0):
        H = -H
    return H, stats


def adjugate(H):
    return np.array([[H[1, 1] * H[2, 2] - H[1, 2] * H[2, 1], H[0, 2] * H[2, 1] - H[0, 1] * H[2, 2], H[0, 1] * H[1, 2] - H[0, 2] * H[1, 1]],
                     [H[1, 2] * H[2, 0] - H[1, 0] * H[2, 2], H[0, 0] * H[2, 2] - H[0, 2] * H[2, 0], H[0, 2] * H[1, 0] - H[0, 0] * H[1, 2]],
                     [H[1, 0] * H[2, 1] - H[1, 1] * H[2, 0], H[0, 1] * H[2, 0] - H[0, 0] * H[2, 1], H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0]]])


def transfer(H, qa, qb, fa, fb):
    """(front, e_b, e_a): both third entries negative, and the two transfer errors in pixels^2, per match"""
    with np.errstate(all="ignore"):
        m, mp = rays3(qa) @ H.T, rays3(qb) @ adjugate(H).T
        eb = fb * fb * ((qb + m[:, :2] / m[:, 2:]) ** 2).sum(1)
        ea = fa * fa * ((qa + mp[:, :2] / mp[:, 2:]) ** 2).sum(1)
        return (m[:, 2] < 0) & (mp[:, 2] < 0), eb, ea


def inliers(H, qa, qb, used, fa, fb, tau):
    front, eb, ea = transfer(H, qa, qb, fa, fb)
    with np.errstate(invalid="ignore"):
        return used & front & (eb <= tau * tau) & (ea <= tau * tau)


def closeness(H, qa, qb, used, fa, fb, tau):
    """the smallest | sqrt(e) / tau - 1 | over both transfer errors of the used matches; inf where there is none"""
    _, eb, ea = transfer(H, qa, qb, fa, fb)
    with np.errstate(all="ignore"):
        e = np.sqrt(np.concatenate([eb[used], ea[used]]))
        e = e[np.isfinite(e)]
    return np.abs(e / tau - 1.0).min() if e.size else np.inf


def defaults(hypotheses=0, sample_size=0, refits=-1, min_inliers=0):
    return (128 if hypotheses <= 0 else hypotheses, MIN_MATCHES if sample_size <= 0 else sample_size, 2 if refits < 0 else refits,
            8 if min_inliers <= 0 else min_inliers)


def homography(p, x, pairs, threshold=None, hypotheses=0, sample_size=0, refits=-1, min_inliers=0, seed=0, info=None):
    """ba_homography -> dict: status, H (NaN where the pair has none), match_ptr, inlier, n_inliers, best_hyp; and what the
    conditions of the tests are stated in: counts (npairs, H; -1: void), counts_hi (counts, or for a hypothesis whose lambda or
    sigma ratio lies within a factor 100 of its limit the larger of its count and the count it reaches with the limits lifted:
    what it could score if rounding moved it across), hyp_margin (npairs, H: the closeness, below, under a hypothesis' own H), ratio and sigma (npairs, H), samples, chain_margin (per
    pair the smallest closeness under the winner's H and under the H of every refit), margin (under the final H), near (a
    lambda or sigma ratio of the winner, a refit or the final fit within a factor 100 of its limit), vote (the smallest sign
    vote |2 pos - n| of the winner, the refits and the final fit), adopted.  threshold None: no consensus stage."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Hn, m, refits, min_inliers = defaults(hypotheses, sample_size, refits, min_inliers)
    if threshold is None:
        Hn, refits = 0, 0
    n = len(pairs)
    ptr, oa, ob, data = pf.rays(p, x, pairs, info)
    out = dict(status=np.zeros(n, dtype=np.uint8), H=np.full((n, 3, 3), np.nan), match_ptr=ptr, obs_a=oa, obs_b=ob,
               inlier=np.zeros(ptr[-1], dtype=bool), n_inliers=np.zeros(n, dtype=np.int32), best_hyp=np.full(n, -1, dtype=np.int32),
               counts=np.full((n, Hn), -1, dtype=np.int64), counts_hi=np.full((n, Hn), -1, dtype=np.int64),
               hyp_margin=np.full((n, Hn), np.inf), ratio=np.full((n, Hn), np.nan), sigma=np.full((n, Hn), np.nan),
               samples=[[None] * Hn for _ in range(n)], chain_margin=np.full(n, np.inf), margin=np.full(n, np.inf),
               near=np.zeros(n, dtype=bool), vote=np.full(n, 10 ** 9, dtype=np.int64), adopted=np.zeros(n, dtype=np.int64))

    def is_near(st):
        return bool(1e-12 < st["ratio"] < 1e-8) or bool(1e-8 < st["sigma"] < 1e-4)

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
            fits = {}
            for h in range(Hn):
                s = nr.sample(seed, h, len(qa), used, m)
                if s is None:
                    continue
                out["samples"][k][h] = np.array(s)
                Hh, st = linear_fit(qa[s], qb[s])
                out["ratio"][k, h], out["sigma"][k, h] = st["ratio"], st["sigma"]
                if is_near(st):
                    Hf, _ = linear_fit(qa[s], qb[s], force=True)
                    if Hf is not None:
                        out["counts_hi"][k, h] = inliers(Hf, qa, qb, used, fa, fb, threshold).sum()
                if Hh is None:
                    continue
                fits[h] = (Hh, st)
                out["counts"][k, h] = inliers(Hh, qa, qb, used, fa, fb, threshold).sum()
                out["counts_hi"][k, h] = max(out["counts_hi"][k, h], out["counts"][k, h])
                out["hyp_margin"][k, h] = closeness(Hh, qa, qb, used, fa, fb, threshold)
            best = int(np.argmax(out["counts"][k]))
            count = int(out["counts"][k, best])
            if count < 0 or count < min_inliers:
                out["status"][k] = NO_CONSENSUS
                out["n_inliers"][k] = max(count, 0)
                out["best_hyp"][k] = best if count >= 0 else -1
                continue
            out["best_hyp"][k] = best
            out["near"][k] |= is_near(fits[best][1])
            out["vote"][k] = fits[best][1]["vote"]
            out["chain_margin"][k] = closeness(fits[best][0], qa, qb, used, fa, fb, threshold)
            M = inliers(fits[best][0], qa, qb, used, fa, fb, threshold)
            for _ in range(refits):
                Hh, st = linear_fit(qa[M], qb[M])
                out["near"][k] |= is_near(st)
                if Hh is None:
                    break
                out["vote"][k] = min(out["vote"][k], st["vote"])
                out["chain_margin"][k] = min(out["chain_margin"][k], closeness(Hh, qa, qb, used, fa, fb, threshold))
                M2 = inliers(Hh, qa, qb, used, fa, fb, threshold)
                if M2.sum() < M.sum() or np.array_equal(M2, M):
                    break
                M = M2
                out["adopted"][k] += 1
        out["inlier"][sl] = M
        out["n_inliers"][k] = M.sum()
        Hh, st = linear_fit(qa[M], qb[M])
        out["near"][k] |= is_near(st)
        if Hh is None:
            out["status"][k] = DEGENERATE
            continue
        out["vote"][k] = min(out["vote"][k], st["vote"])
        out["H"][k] = Hh
        if threshold is not None:
            out["margin"][k] = closeness(Hh, qa, qb, used, fa, fb, threshold)
    return out


def signed(v):
    """v with its entry of the largest magnitude positive (ties to the lowest index)"""
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def sign_gap(H):
    """how far the two sign decisions of decompose are from a tie: the smallest difference of the two largest |entries| of v_1, v_3"""
    _, _, Vt = np.linalg.svd(H)
    return min(np.diff(np.sort(np.abs(v))[-2:])[0] for v in (Vt[0], Vt[2]))


def decompose(H):
    """ba_decompose_homography on one matrix -> (R (4, 3, 3), t (4, 3), n (4, 3), n_sol, parallax), the unused slots NaN"""
    R, t, nv = np.full((4, 3, 3), np.nan), np.full((4, 3), np.nan), np.full((4, 3), np.nan)
    H = np.asarray(H, dtype=np.float64)
    if not np.isfinite(H).all():
        return R, t, nv, 0, np.nan
    _, sg, Vt = np.linalg.svd(H)
    if not (np.isfinite(sg).all() and sg[1] > 0):
        return R, t, nv, 0, np.nan
    v1, v3 = signed(Vt[0]), signed(Vt[2])
    v2 = np.cross(v3, v1)
    Hs = H / sg[1]
    g1, g3 = sg[0] / sg[1], sg[2] / sg[1]
    parallax = g1 - g3
    dd = g1 * g1 - g3 * g3
    if not dd > 1e-12:
        u1, u2 = Hs @ v1 / g1, Hs @ v2
        R[0] = np.stack([u1, u2, np.cross(u1, u2)], axis=1) @ np.stack([v1, v2, v3], axis=0)
        t[0], nv[0] = 0.0, 0.0
        return R, t, nv, 1, parallax
    ca, cb = np.sqrt(max(1.0 - g3 * g3, 0.0)), np.sqrt(max(g1 * g1 - 1.0, 0.0))
    for s, sgn in enumerate((1.0, -1.0)):
        u = (ca * v1 + sgn * cb * v3) / np.sqrt(dd)
        U = np.stack([v2, u, np.cross(v2, u)], axis=1)
        W = np.stack([Hs @ v2, Hs @ u, np.cross(Hs @ v2, Hs @ u)], axis=1)
        Rm = W @ U.T
        n = np.cross(v2, u)
        tv = (Hs - Rm) @ n
        R[2 * s], t[2 * s], nv[2 * s] = Rm, tv, n
        R[2 * s + 1], t[2 * s + 1], nv[2 * s + 1] = Rm, -tv, -n
    return R, t, nv, 4, parallax


def homography_pose(p, x, pairs, con, threshold, info=None):
    """ba_homography_pose on the dict `con` of homography -> dict: parallax, n_pose, r, t, normal (npairs, 2, 3), support
    (npairs, 2), and plane_vote (per pair the smallest |2 count - |set|| over the four solutions: how far the vote is from a tie)"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = len(pairs)
    ptr, _, _, data = pf.rays(p, x, pairs, info)
    out = dict(parallax=np.full(n, np.nan), n_pose=np.zeros(n, dtype=np.int32), r=np.full((n, 2, 3), np.nan), t=np.full((n, 2, 3), np.nan),
               normal=np.full((n, 2, 3), np.nan), support=np.full((n, 2), -1, dtype=np.int32), plane_vote=np.full(n, 10 ** 9, dtype=np.int64))
    for k, (qa, qb, used, fa, fb) in enumerate(data):
        if con["status"][k] != OK or not (np.isfinite(fa) and fa != 0 and np.isfinite(fb) and fb != 0):
            continue
        R, t, nv, ns, par = decompose(con["H"][k])
        if ns == 0:
            continue
        out["parallax"][k] = par
        if ns == 1:
            out["n_pose"][k], out["r"][k, 0] = 1, rr.rotation_vector(R[0])
            continue
        M = con["inlier"][ptr[k]:ptr[k + 1]]
        da = rays3(qa[M])
        j = 0
        for c in range(4):
            cnt = int((da @ nv[c] > 0).sum())
            out["plane_vote"][k] = min(out["plane_vote"][k], abs(2 * cnt - len(da)))
            if 2 * cnt > len(da) and j < 2:
                r, tn = rr.rotation_vector(R[c]), t[c] / np.linalg.norm(t[c])
                out["r"][k, j], out["t"][k, j], out["normal"][k, j] = r, tn, nv[c]
                out["support"][k, j] = pf.inliers(r, tn, qa, qb, used, fa, fb, threshold).sum()
                j += 1
        out["n_pose"][k] = j
    return out


def two_view(gen, pla, cand, ratio=0.8, min_parallax=0.05):
    """two_view of the package from the reference dicts of the essential stage (pair_ref / five_point_ref: status, r, t, inlier,
    n_inliers, match_ptr), of homography and of homography_pose -> model, r, t, ambiguous, pick, n_general, n_planar, off_plane,
    seed_order"""
    n = len(gen["status"])
    ok_e, ok_h = gen["status"] == OK, pla["status"] == OK
    n_e, n_h = np.where(ok_e, gen["n_inliers"], 0).astype(np.int64), np.where(ok_h, pla["n_inliers"], 0).astype(np.int64)
    mp = gen["match_ptr"]
    off = np.array([int((gen["inlier"][mp[k]:mp[k + 1]] & ~pla["inlier"][mp[k]:mp[k + 1]]).sum()) if ok_e[k] else 0 for k in range(n)])
    model, pick, amb = ["none"] * n, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    r, t = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    for k in range(n):
        explains = ok_h[k] and n_h[k] >= ratio * n_e[k]
        if explains and cand["parallax"][k] < min_parallax:
            model[k], r[k] = "rotation", cand["r"][k, 0]
        elif explains and cand["n_pose"][k] > 0:
            model[k] = "planar"
            if cand["n_pose"][k] == 2:
                s0, s1 = cand["support"][k]
                pick[k], amb[k] = (1 if s1 > s0 else 0), s0 == s1
            r[k], t[k] = cand["r"][k, pick[k]], cand["t"][k, pick[k]]
        elif ok_e[k]:
            model[k], r[k], t[k] = "general", gen["r"][k], gen["t"][k]
    rank = {"general": 0, "planar": 1}
    n_in = np.where(np.array(model) == "general", n_e, n_h)
    order = sorted((k for k in range(n) if model[k] in rank), key=lambda k: (rank[model[k]], -off[k], -n_in[k], k))
    return dict(model=np.array(model), r=r, t=t, ambiguous=amb, pick=pick, n_general=n_e, n_planar=n_h, off_plane=off,
                seed_order=np.array(order, dtype=np.int64))


def unit_H(H):
    """H at sigma_2 = 1 (its sign kept)"""
    return H / np.linalg.svd(H, compute_uv=False)[1]
