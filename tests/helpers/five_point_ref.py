"""numpy restatement of ba_five_point and ba_relative_pose_five_point (include/ba_hip.h, "the five-point essential matrix";
DESIGN §5p) on top of pair_ref (rays, the inlier test, linear_fit, pose_error), ransac_ref.sample and resect_ref.rotation_vector:
the null space through np.linalg.eigh (or svd), the ten cubics through tensors of the four basis matrices, the elimination
through np.linalg.solve, the roots of the degree-10 determinant through np.roots (where the kernel runs a simultaneous complex
iteration), (x, y) through the svd of the 3 x 3 at a root, the two Gauss-Newton steps on the cubics through np.linalg.solve.  Written from the text of the header, not from the kernels."""
import itertools

import numpy as np

import pair_ref as pf
import ransac_ref as nr
import resect_ref as rr

SAMPLE = 5
NULL_RATIO = 1e-12   # lambda_5 <= NULL_RATIO lambda_9: the null space is not four-dimensional
REAL_ROOT = 1e-7     # |Im z| <= REAL_ROOT |z|: a real root
# the 20 monomials in (x, y, z, 1) = variables (0, 1, 2, 3), the column order of the header:
# x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
MONOMIALS = ((0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
             (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3))


def rays3(q):
    return np.concatenate([q, -np.ones((len(q), 1))], axis=1)


def system(qa, qb):
    """the 5 x 9 matrix of a_k = d_b (x) d_a"""
    da, db = rays3(np.asarray(qa, dtype=np.float64)), rays3(np.asarray(qb, dtype=np.float64))
    return (db[:, :, None] * da[:, None, :]).reshape(len(da), 9)


def null_space(qa, qb, how="eigh"):
    """(basis (4, 3, 3) = X, Y, Z, W or None, lambda_5 / lambda_9)"""
    A = system(qa, qb)
    if not np.isfinite(A).all():
        return None, np.nan
    if how == "eigh":
        lam, V = np.linalg.eigh(A.T @ A)
        ratio = lam[4] / lam[8]
        basis = V[:, :4].T
    else:
        _, s, Vt = np.linalg.svd(A)
        ratio = (s[4] / s[0]) ** 2
        basis = Vt[5:][::-1]
    if not ratio > NULL_RATIO:
        return None, ratio
    return basis.reshape(4, 3, 3), ratio


def cubics(N):
    """the 10 x 20 matrix of det E = 0 (row 0) and 2 E E' E - tr(E E') E = 0 (rows 1..9, row-major) for E = sum_k v_k N[k]"""
    EEt = np.einsum("pil,qjl->ijpq", N, N)
    T = 2.0 * np.einsum("ilpq,rlj->ijpqr", EEt, N) - np.einsum("llpq,rij->ijpqr", EEt, N)
    D = np.zeros((4, 4, 4))
    for (a, b, c), sign in ((( 0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((2, 1, 0), -1), ((1, 0, 2), -1)):
        D += sign * np.einsum("p,q,r->pqr", N[:, 0, a], N[:, 1, b], N[:, 2, c])
    full = np.concatenate([D[None], T.reshape(9, 4, 4, 4)])
    C = np.zeros((10, 20))
    for m, mono in enumerate(MONOMIALS):
        for p, q, r in set(itertools.permutations(mono)):
            C[:, m] += full[:, p, q, r]
    return C


def poly_matrix(C):
    """(B (3, 3) of np.poly1d in z from the eliminated system: B(z) (x, y, 1)' = 0, the eliminated 10 x 20 system [I | G]); (None,
    None): a singular elimination"""
    with np.errstate(all="ignore"):
        try:
            G = np.linalg.solve(C[:, :10], C[:, 10:])
        except np.linalg.LinAlgError:
            return None, None
    if not np.isfinite(G).all():
        return None, None
    B = []
    for e in (4, 6, 8):
        a, b = G[e], G[e + 1]  # the rows of (x^2z, x^2), (y^2z, y^2), (xyz, xy); columns 10..19 of the header's order
        B.append([np.poly1d([-b[0], a[0] - b[1], a[1] - b[2], a[2]]), np.poly1d([-b[3], a[3] - b[4], a[4] - b[5], a[5]]),
                  np.poly1d([-b[6], a[6] - b[7], a[7] - b[8], a[8] - b[9], a[9]])])
    return B, np.concatenate([np.eye(10), G], axis=1)


def monomials(v):
    """(the 20 monomials at v = (x, y, z), their gradients (20, 3))"""
    h = np.array([v[0], v[1], v[2], 1.0])
    m, g = np.zeros(20), np.zeros((20, 3))
    for k, mono in enumerate(MONOMIALS):
        m[k] = h[mono[0]] * h[mono[1]] * h[mono[2]]
        for i in range(3):
            for pos in range(3):
                if mono[pos] == i:
                    g[k, i] += np.prod([h[mono[q]] for q in range(3) if q != pos])
    return m, g


def polish(C, v, steps=2):
    """Gauss-Newton steps on the ten eliminated cubics C m(x, y, z) = 0; a step that is not finite is not taken"""
    v = np.array(v, dtype=np.float64)
    for _ in range(steps):
        m, g = monomials(v)
        f, J = C @ m, C @ g
        with np.errstate(all="ignore"):
            try:
                step = np.linalg.solve(J.T @ J, J.T @ f)
            except np.linalg.LinAlgError:
                break
        if np.isfinite(step).all():
            v = v - step
    return v


def solve(qa, qb, how="eigh", roots=np.roots):
    """the real solutions of one tuple -> (E (n_sol, 3, 3) with |E|_F = 1, stats): ratio = lambda_5 / lambda_9, imag = the smallest
    |Im z| / |z| over the complex roots (inf: none)"""
    stats = dict(ratio=np.nan, imag=np.inf)
    none = np.zeros((0, 3, 3))
    N, stats["ratio"] = null_space(qa, qb, how)
    if N is None:
        return none, stats
    B, C = poly_matrix(cubics(N))
    if B is None:
        return none, stats
    det = (B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0])
           + B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0]))
    coef = np.zeros(11)
    coef[11 - len(det.coeffs):] = det.coeffs
    if not np.isfinite(coef).all() or coef[0] == 0.0:
        return none, stats
    out = []
    for z in roots(coef):
        rel = abs(z.imag) / abs(z) if abs(z) > 0 else 0.0
        if rel > REAL_ROOT:
            stats["imag"] = min(stats["imag"], rel)
            continue
        z = float(z.real)
        with np.errstate(all="ignore"):
            for _ in range(2):  # Newton on the real axis
                step = det(z) / det.deriv()(z)
                if np.isfinite(step):
                    z -= step
        Bz = np.array([[B[i][j](z) for j in range(3)] for i in range(3)])
        v = np.linalg.svd(Bz)[2][-1]
        with np.errstate(all="ignore"):
            x, y, z = polish(C, (v[0] / v[2], v[1] / v[2], z))
            E = x * N[0] + y * N[1] + z * N[2] + N[3]
            E = E / np.linalg.norm(E)
        if np.isfinite(E).all():
            out.append(E)
    return (np.array(out) if out else none), stats


def residuals(E, qa, qb):
    """(epipolar, determinant, trace): the largest |d_b' E d_a| over the five, |det E|, the largest entry of |2 E E' E - tr(E E') E|"""
    da, db = rays3(np.asarray(qa, dtype=np.float64)), rays3(np.asarray(qb, dtype=np.float64))
    return (np.abs(np.einsum("ki,ij,kj->k", db, E, da)).max(), abs(np.linalg.det(E)),
            np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


def distance(E, F):
    """|E - F|_F up to sign, both of norm 1"""
    return min(np.linalg.norm(E - F), np.linalg.norm(E + F))


def nearest(E, many):
    return min((distance(E, F) for F in many), default=np.inf)


def candidates(E):
    """the four (R, t) of an essential matrix, the order of the header's step 6"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U[:, 2] *= -1
    if np.linalg.det(Vt) < 0:
        Vt[2] *= -1
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tn = U[:, 2] / np.linalg.norm(U[:, 2])
    return [(U @ W @ Vt, tn), (U @ W @ Vt, -tn), (U @ W.T @ Vt, tn), (U @ W.T @ Vt, -tn)]


def hypothesis(qa, qb, s, used, fa, fb, tau):
    """hypothesis with the sample s over the list (qa, qb): (r, t, count) of its best candidate or (None, None, -1), and stats:
    ratio, n_sol, cand_lead (the best candidate's count minus the second's; 10^9 with one candidate), lead (the cheirality lead of
    the best candidate's vote), hi (the largest count any of the four (R, t) of any solution reaches)"""
    st = dict(ratio=np.nan, n_sol=0, cand_lead=10 ** 9, lead=10 ** 9, hi=-1)
    Es, sol = solve(qa[s], qb[s])
    st["ratio"], st["n_sol"] = sol["ratio"], len(Es)
    scored = []
    for E in Es:
        cands = candidates(E)
        cnt = np.array([pf.in_front(R, t, qa[s], qb[s]).sum() for R, t in cands])
        b = int(np.argmax(cnt))
        every = [int(pf.inliers(rr.rotation_vector(R), t, qa, qb, used, fa, fb, tau).sum()) for R, t in cands]
        st["hi"] = max(st["hi"], max(every))
        if cnt[b] <= 0:
            continue
        r, t = rr.rotation_vector(cands[b][0]), cands[b][1]
        if not (np.isfinite(r).all() and np.isfinite(t).all()):
            continue
        scored.append((every[b], int(cnt[b] - np.sort(cnt)[-2]), r, t))
    if not scored:
        return None, None, -1, st
    order = sorted(range(len(scored)), key=lambda i: -scored[i][0])
    count, st["lead"], r, t = scored[order[0]]
    if len(order) > 1:
        st["cand_lead"] = count - scored[order[1]][0]
    return r, t, count, st


def relative_pose(p, x, pairs, threshold, hypotheses=0, refits=-1, min_inliers=0, seed=0, info=None):
    """ba_relative_pose_five_point -> the dict of pair_ref.relative_pose (same keys, same meaning: ratio is lambda_5 / lambda_9
    here, hyp_lead the cheirality lead of a hypothesis' best candidate, counts_hi the largest count any (R, t) of any solution
    of the hypothesis reaches) and cand_lead (npairs, H): the lead of a hypothesis' best candidate over its second."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    H = 128 if hypotheses <= 0 else hypotheses
    refits = 2 if refits < 0 else refits
    min_inliers = pf.MIN_MATCHES if min_inliers <= 0 else min_inliers
    n = len(pairs)
    ptr, oa, ob, data = pf.rays(p, x, pairs, info)
    out = dict(status=np.zeros(n, dtype=np.uint8), r=np.full((n, 3), np.nan), t=np.full((n, 3), np.nan), match_ptr=ptr, obs_a=oa, obs_b=ob,
               inlier=np.zeros(ptr[-1], dtype=bool), n_inliers=np.zeros(n, dtype=np.int32), best_hyp=np.full(n, -1, dtype=np.int32),
               counts=np.full((n, H), -1, dtype=np.int64), counts_hi=np.full((n, H), -1, dtype=np.int64),
               hyp_lead=np.full((n, H), 10 ** 9, dtype=np.int64), cand_lead=np.full((n, H), 10 ** 9, dtype=np.int64),
               ratio=np.full((n, H), np.nan), samples=[[None] * H for _ in range(n)],
               runner_lead=np.full(n, 10 ** 9, dtype=np.int64), chain_margin=np.full(n, np.inf),
               lead=np.full(n, 10 ** 9, dtype=np.int64), margin=np.full(n, np.inf), adopted=np.zeros(n, dtype=np.int64))

    def closeness(r, t, qa, qb, used, fa, fb):
        with np.errstate(all="ignore"):
            e = np.sqrt(pf.sampson(pf.br.rotations(r[None])[0], t, qa, qb, fa, fb)[used])
        return np.abs(e / threshold - 1.0).min() if used.any() else np.inf

    for k, (qa, qb, used, fa, fb) in enumerate(data):
        sl = slice(ptr[k], ptr[k + 1])
        if used.sum() < pf.MIN_MATCHES:
            out["status"][k] = pf.FEW_MATCHES
            continue
        if not (np.isfinite(fa) and fa != 0 and np.isfinite(fb) and fb != 0):
            out["status"][k] = pf.DEGENERATE
            continue
        poses = {}
        for h in range(H):
            s = nr.sample(seed, h, len(qa), used, SAMPLE)
            if s is None:
                continue
            s = np.array(s)
            out["samples"][k][h] = s
            r, t, count, st = hypothesis(qa, qb, s, used, fa, fb, threshold)
            out["ratio"][k, h], out["counts_hi"][k, h] = st["ratio"], st["hi"]
            if r is None:
                continue
            poses[h] = (r, t)
            out["counts"][k, h], out["hyp_lead"][k, h], out["cand_lead"][k, h] = count, st["lead"], st["cand_lead"]
        best = int(np.argmax(out["counts"][k]))
        count = int(out["counts"][k, best])
        if count < 0 or count < min_inliers:
            out["status"][k] = pf.NO_CONSENSUS
            out["n_inliers"][k] = max(count, 0)
            out["best_hyp"][k] = best if count >= 0 else -1
            continue
        out["best_hyp"][k] = best
        others = np.delete(out["counts_hi"][k], best)
        if others.size and others.max() >= 0:
            out["runner_lead"][k] = count - others.max()
        out["chain_margin"][k] = closeness(*poses[best], qa, qb, used, fa, fb)
        M = pf.inliers(*poses[best], qa, qb, used, fa, fb, threshold)
        for _ in range(refits):
            r, t, st = pf.linear_fit(qa[M], qb[M])
            if r is None:
                break
            out["lead"][k] = min(out["lead"][k], st["lead"])
            out["chain_margin"][k] = min(out["chain_margin"][k], closeness(r, t, qa, qb, used, fa, fb))
            M2 = pf.inliers(r, t, qa, qb, used, fa, fb, threshold)
            if M2.sum() < M.sum() or np.array_equal(M2, M):
                break
            M = M2
            out["adopted"][k] += 1
        out["inlier"][sl] = M
        out["n_inliers"][k] = M.sum()
        r, t, st = pf.linear_fit(qa[M], qb[M])
        if r is None:
            out["status"][k] = pf.DEGENERATE
            continue
        out["lead"][k] = min(out["lead"][k], st["lead"])
        out["r"][k], out["t"][k] = r, t
        out["margin"][k] = closeness(r, t, qa, qb, used, fa, fb)
    return out
