"""numpy restatement of ba_refine_relative_pose (include/ba_hip.h, "non-linear refinement of the relative pose") on top
of pair_ref (rays, essential, sampson, inliers): the signed Sampson residual, its analytic Jacobian in the five local parameters,
the basis B across t, the Marquardt rules and the re-scoring rounds.  Written from the text of the header, not from the kernel."""
import numpy as np

import block_ref as br
import pair_ref as pf
import resect_ref as rr

CONVERGED, STALLED, MAX_ITER, NONFINITE, SKIPPED = range(5)
STATES = ("converged", "stalled", "max_iter", "nonfinite", "skipped")
MIN_SET = 5


def defaults(max_iter=-1, xtol=0.0, lam0=0.0, rounds=-1):
    return (50 if max_iter < 0 else max_iter), (1e-10 if xtol <= 0 else xtol), (1e-4 if lam0 <= 0 else lam0), (2 if rounds < 0 else rounds)


def rays3(q):
    return np.concatenate([q, -np.ones((len(q), 1))], axis=1)


def parts(E, qa, qb, fa, fb):
    """(n, D, l, m) per match: n = d_b' E d_a, l = E d_a, m = E' d_b, D the Sampson denominator in pixels"""
    da, db = rays3(qa), rays3(qb)
    l, m = da @ E.T, db @ E
    n = (db * l).sum(1)
    D = (l[:, 0] ** 2 + l[:, 1] ** 2) / fb ** 2 + (m[:, 0] ** 2 + m[:, 1] ** 2) / fa ** 2
    return n, D, l, m


def residual(R, t, qa, qb, fa, fb):
    """e = n / sqrt(D) per match: e^2 is pair_ref.sampson"""
    with np.errstate(all="ignore"):
        n, D, _, _ = parts(pf.essential(R, t), qa, qb, fa, fb)
        return n / np.sqrt(D)


def basis(t):
    """B (3, 2): b1 = (e_i x t) / |e_i x t| for i the index of the smallest |t_i| (ties to the lowest), b2 = t x b1"""
    i = int(np.argmin(np.abs(t)))  # (argmin returns the first of equal entries)
    with np.errstate(all="ignore"):
        b1 = np.cross(np.eye(3)[i], t)
        b1 = b1 / np.linalg.norm(b1)
    return np.stack([b1, np.cross(t, b1)], axis=1)


def tangent(R, t):
    """the five dE of a unit step in each local parameter: [t]x [e_j]x R and [b_j]x R"""
    sk = lambda v: br.skew(np.asarray(v, dtype=np.float64)[None])[0]  # noqa: E731
    B = basis(t)
    return [sk(t) @ sk(np.eye(3)[j]) @ R for j in range(3)] + [sk(B[:, j]) @ R for j in range(2)]


def jacobian(R, t, qa, qb, fa, fb):
    """(e (n,), J (n, 5)), analytic: de = dn / sqrt(D) - n dD / (2 D^(3/2))"""
    da, db = rays3(qa), rays3(qb)
    with np.errstate(all="ignore"):
        n, D, l, m = parts(pf.essential(R, t), qa, qb, fa, fb)
        J = np.zeros((len(qa), 5))
        for j, G in enumerate(tangent(R, t)):
            dl, dm = da @ G.T, db @ G
            dn = (db * dl).sum(1)
            dD = 2 * (l[:, 0] * dl[:, 0] + l[:, 1] * dl[:, 1]) / fb ** 2 + 2 * (m[:, 0] * dm[:, 0] + m[:, 1] * dm[:, 1]) / fa ** 2
            J[:, j] = dn / np.sqrt(D) - n * dD / (2 * D ** 1.5)
        return n / np.sqrt(D), J


def retract(R, t, delta):
    """R+ = exp([d_omega]x) R, t+ = (t + B d_tau) / |t + B d_tau|"""
    w = np.asarray(delta[:3], dtype=np.float64)
    th = np.linalg.norm(w)
    K = br.skew(w[None])[0]
    a, b = (1.0, 0.5) if th == 0 else (np.sin(th) / th, 0.5 * (np.sin(0.5 * th) / (0.5 * th)) ** 2)
    with np.errstate(all="ignore"):
        u = t + basis(t) @ np.asarray(delta[3:], dtype=np.float64)
        Rn = R + a * (K @ R) + b * (K @ (K @ R))
        return Rn, (t if np.array_equal(u, t) else u / np.linalg.norm(u))  # (a step that does not move t leaves its bits)


def rho(loss, s, c):
    """(c^2 rho(s / c^2), rho'(s / c^2)) per entry: scipy's losses"""
    z = s / (c * c)
    with np.errstate(all="ignore"):
        if loss == "huber":
            sz = np.sqrt(np.maximum(z, 1.0))
            return c * c * np.where(z <= 1, z, 2 * sz - 1), np.where(z <= 1, 1.0, 1 / sz)
        if loss == "soft_l1":
            tt = np.sqrt(1 + z)
            return c * c * 2 * z / (tt + 1), 1 / tt
        if loss == "cauchy":
            return c * c * np.log1p(z), 1 / (1 + z)
        if loss == "arctan":
            return c * c * np.arctan(z), 1 / (1 + z * z)
    assert loss == "linear", loss
    return s, np.ones_like(s)


def cost(R, t, qa, qb, fa, fb, loss="linear", c=1.0):
    e = residual(R, t, qa, qb, fa, fb)
    return 0.5 * rho(loss, e * e, c)[0].sum()


def normal_sums(R, t, qa, qb, fa, fb, loss="linear", c=1.0):
    """(F, g, H) of the set at (R, t)"""
    e, J = jacobian(R, t, qa, qb, fa, fb)
    r, w = rho(loss, e * e, c)
    with np.errstate(all="ignore"):
        return 0.5 * r.sum(), J.T @ (w * e), J.T @ (w[:, None] * J)


def marquardt(R, t, qa, qb, fa, fb, max_iter=50, xtol=1e-10, lam0=1e-4, loss="linear", c=1.0):
    """the iteration of the header on one set -> dict(R, t, state, F0, F, trials, moved)"""
    F, g, H = normal_sums(R, t, qa, qb, fa, fb, loss, c)
    out = dict(R=R, t=t, state=MAX_ITER, F0=F, F=F, trials=0, moved=False)
    if not np.isfinite(F):
        return dict(out, state=NONFINITE)
    lam = lam0
    for it in range(max_iter):
        out["trials"] = it + 1
        accept, delta = False, None
        with np.errstate(all="ignore"):
            A = H + lam * np.diag(np.diag(H))
            try:
                L = np.linalg.cholesky(A)
                delta = np.linalg.solve(L.T, np.linalg.solve(L, -g))
            except np.linalg.LinAlgError:
                delta = None
        if delta is not None and np.isfinite(delta).all():
            Rn, tn = retract(out["R"], out["t"], delta)
            Fn = cost(Rn, tn, qa, qb, fa, fb, loss, c)
            accept = bool(np.isfinite(Fn) and Fn <= out["F"])
        if accept:
            out.update(R=Rn, t=tn, F=Fn, moved=True)
            _, g, H = normal_sums(Rn, tn, qa, qb, fa, fb, loss, c)
            lam = max(lam / 10.0, 1e-12)
            if np.linalg.norm(delta) <= xtol:
                out["state"] = CONVERGED
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                out["state"] = STALLED
                break
    return out


def gradient_ratio(R, t, qa, qb, fa, fb, loss="linear", c=1.0):
    """|g|_2 / |H|_F at (R, t): how far from stationary the reference's own result is, as a step length"""
    _, g, H = normal_sums(R, t, qa, qb, fa, fb, loss, c)
    return float(np.linalg.norm(g) / np.linalg.norm(H))


def refine(p, x, pairs, r, t, status=None, inlier=None, info=None, max_iter=-1, xtol=0.0, lam0=0.0, loss="linear", f_scale=1.0,
           threshold=None, rounds=-1, order=None):
    """ba_refine_relative_pose -> dict: state, r, t, inlier (per match), n_inliers, n_consistent, cost (npairs, 2), iters; and what
    the tests' conditions are stated in: margin (per pair the smallest | sqrt(sampson) / tau - 1 | over the used matches under the
    pose of every round; inf for a pair that is not refined), grad (|g| / |H| at the returned pose on the returned set), adopted
    (rounds whose set was adopted).  inlier None: every used match.  order: per pair a permutation of its match list in which
    the sums are taken (the reference's spread under its own summation order), or None."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    max_iter, xtol, lam0, rounds = defaults(max_iter, xtol, lam0, rounds)
    n = len(pairs)
    ptr, oa, ob, data = pf.rays(p, x, pairs, info)
    r, t = np.array(r, dtype=np.float64, copy=True).reshape(n, 3), np.array(t, dtype=np.float64, copy=True).reshape(n, 3)
    out = dict(state=np.full(n, SKIPPED, dtype=np.uint8), r=r, t=t, match_ptr=ptr, obs_a=oa, obs_b=ob,
               inlier=np.ones(ptr[-1], dtype=bool) if inlier is None else np.array(inlier, dtype=bool, copy=True),
               n_inliers=np.zeros(n, dtype=np.int32), n_consistent=np.zeros(n, dtype=np.int32), cost=np.zeros((n, 2)),
               iters=np.zeros(n, dtype=np.int32), margin=np.full(n, np.inf), grad=np.zeros(n), adopted=np.zeros(n, dtype=np.int64))
    for k, (qa, qb, used, fa, fb) in enumerate(data):
        sl = slice(ptr[k], ptr[k + 1])
        M = out["inlier"][sl] & used
        if (status is not None and status[k] != pf.OK) or not (np.isfinite(fa) and fa != 0 and np.isfinite(fb) and fb != 0) or M.sum() < MIN_SET:
            continue
        perm = np.arange(len(qa)) if order is None else np.asarray(order[k])
        R, tk = br.rotations(r[k][None])[0], t[k].copy()
        for j in range(rounds + 1):
            idx = perm[M[perm]]
            res = marquardt(R, tk, qa[idx], qb[idx], fa, fb, max_iter, xtol, lam0, loss, f_scale)
            out["state"][k] = res["state"]
            out["iters"][k] += res["trials"]
            if j == 0:
                out["cost"][k, 0] = res["F0"]
            out["cost"][k, 1] = res["F"]
            out["inlier"][sl], out["n_inliers"][k] = M, M.sum()
            if res["state"] == NONFINITE:
                break
            if res["moved"]:
                R, tk = res["R"], res["t"]
                r[k], t[k] = rr.rotation_vector(R), tk
            out["grad"][k] = gradient_ratio(R, tk, qa[idx], qb[idx], fa, fb, loss, f_scale)
            M2 = pf.inliers(r[k], t[k], qa, qb, used, fa, fb, threshold)
            out["n_consistent"][k] = M2.sum()
            with np.errstate(all="ignore"):
                e = np.sqrt(pf.sampson(br.rotations(r[k][None])[0], t[k], qa, qb, fa, fb)[used])
            out["margin"][k] = min(out["margin"][k], np.abs(e / threshold - 1.0).min())
            if j == rounds or M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"][k] += 1
            R = br.rotations(r[k][None])[0]  # (a round starts from the pose as it is returned)
    return out


def numeric_jacobian(R, t, qa, qb, fa, fb, h=1e-6):
    """central differences of the residual through the retraction, column by column"""
    J = np.zeros((len(qa), 5))
    for j in range(5):
        d = np.zeros(5)
        d[j] = h
        J[:, j] = (residual(*retract(R, t, d), qa, qb, fa, fb) - residual(*retract(R, t, -d), qa, qb, fa, fb)) / (2 * h)
    return J


def angles(p, x_true, k, r, t):
    """(rotation error, translation-direction error) in degrees of pair k's (r, t) against the generator"""
    Rt, tt, _ = pf.true_relative(p, x_true, 2 * k, 2 * k + 1)
    R = br.rotations(np.asarray(r, dtype=np.float64)[None])[0]
    cr = np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1)
    ct = np.clip(t @ tt / np.linalg.norm(t), -1, 1)
    return float(np.degrees(np.arccos(cr))), float(np.degrees(np.arccos(ct)))
