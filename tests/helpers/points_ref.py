"""numpy restatement of ba_refine_points (include/ba_hip.h, "points with the cameras held"), vectorised over the
points: the linear triangulation, the whitening by the observations' information, the losses, the point prior, the per-point
Marquardt loop and the states.  Written from the text of the header, not from the kernel: the BAL projection and its 2 x 3 point
Jacobian are derived here (P1 = R X + t, P2 = -P1.xy / P1.z, out = f (1 + k1 n + k2 n^2) P2, n = |P2|^2)."""
import numpy as np

from _lm_ref import factor, rho  # the two definitions this text shares with the LM reference: scipy's loss table, the header's factor

CONVERGED, STALLED, MAX_ITER, FIXED, DEGENERATE, NONFINITE = range(6)
BEHIND = 0x80
UNDIST_ITERS = 8
_PACK = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))  # packed lower 3 x 3, row-major


def rotations(cams):
    """(ncams, 3, 3) Rodrigues matrices of the rotation vectors"""
    r = cams[:, :3]
    th = np.sqrt((r * r).sum(1))
    k = r / th[:, None]
    c, s = np.cos(th), np.sin(th)
    K = np.zeros((len(cams), 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -k[:, 2], k[:, 1]
    K[:, 1, 0], K[:, 1, 2] = k[:, 2], -k[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -k[:, 1], k[:, 0]
    return c[:, None, None] * np.eye(3) + s[:, None, None] * K + (1 - c)[:, None, None] * k[:, :, None] * k[:, None, :]


class Scene:
    def __init__(self, p, x, info=None):
        self.npnts, self.ncams, self.nobs = p["npnts"], p["ncams"], p["nobs"]
        self.cam0 = np.asarray(p["cam_idx1"]) - 1
        self.pnt0 = np.asarray(p["pnt_idx1"]) - 1
        self.m = np.asarray(p["pt2d"], dtype=np.float64).reshape(-1, 2)
        cams = np.asarray(x[3 * self.npnts:], dtype=np.float64).reshape(self.ncams, 9)
        self.R = rotations(cams)[self.cam0]        # per observation
        self.t = cams[self.cam0, 3:6]
        self.k1, self.k2, self.f = cams[self.cam0, 6], cams[self.cam0, 7], cams[self.cam0, 8]
        self.L = np.tile([1.0, 0.0, 1.0], (self.nobs, 1)) if info is None else np.stack(factor(np.asarray(info, dtype=np.float64)), axis=1)
        self.used = ~np.all(self.L == 0.0, axis=1)
        self.deg = np.bincount(self.pnt0, minlength=self.npnts)

    def psum(self, v):
        """per-point sums of a per-observation array (nobs,) or (nobs, k)"""
        if v.ndim == 1:
            return np.bincount(self.pnt0, weights=v, minlength=self.npnts)
        return np.stack([np.bincount(self.pnt0, weights=v[:, j], minlength=self.npnts) for j in range(v.shape[1])], axis=1)


def chol3_solve(A, b, piv_min):
    """x of A x = b for packed lower 3 x 3 blocks A (n, 6), and ok (n,): every pivot above piv_min, x finite"""
    with np.errstate(all="ignore"):
        d0 = A[:, 0]
        l00 = np.sqrt(d0)
        l10, l20 = A[:, 1] / l00, A[:, 3] / l00
        d1 = A[:, 2] - l10 * l10
        l11 = np.sqrt(d1)
        l21 = (A[:, 4] - l20 * l10) / l11
        d2 = A[:, 5] - l20 * l20 - l21 * l21
        l22 = np.sqrt(d2)
        y0 = b[:, 0] / l00
        y1 = (b[:, 1] - l10 * y0) / l11
        y2 = (b[:, 2] - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = (y0 - l10 * x1 - l20 * x2) / l00
        x = np.stack([x0, x1, x2], axis=1)
        ok = (d0 > piv_min) & (d1 > piv_min) & (d2 > piv_min) & np.isfinite(x).all(axis=1)
    return x, ok


def triangulate(sc):
    """(X (npnts, 3), ok (npnts,)) of the linear triangulation"""
    u = sc.m / sc.f[:, None]
    q = u.copy()
    for _ in range(UNDIST_ITERS):
        n2 = (q * q).sum(1)
        q = u / (1.0 + sc.k1 * n2 + sc.k2 * n2 * n2)[:, None]
    v = np.concatenate([q, -np.ones((sc.nobs, 1))], axis=1)
    d = np.einsum("oji,oj->oi", sc.R, v)  # R'v
    d /= np.sqrt((d * d).sum(1))[:, None]
    c = -np.einsum("oji,oj->oi", sc.R, sc.t)
    use = sc.used.astype(float)
    M = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    A = sc.psum(np.stack([M[:, i, j] for i, j in _PACK], axis=1) * use[:, None])
    b = sc.psum(np.einsum("oij,oj->oi", M, c) * use[:, None])
    n = sc.psum(use)
    X, ok = chol3_solve(A, b, 1e-12 * (A[:, 0] + A[:, 2] + A[:, 5]))
    return X, ok & (n >= 2)


def evaluate(sc, X, loss="linear", c=1.0, prior=None):
    """per point at X (npnts, 3): f, H (packed lower, (npnts, 6)), g (npnts, 3), behind (bool), and per observation the
    whitened residual (nobs, 2), the whitened 2 x 3 block (nobs, 2, 3) and the weight"""
    with np.errstate(all="ignore"):
        P1 = np.einsum("oij,oj->oi", sc.R, X[sc.pnt0]) + sc.t
        P2 = -P1[:, :2] / P1[:, 2:3]
        n = (P2 * P2).sum(1)
        rr = 1.0 + sc.k1 * n + sc.k2 * n * n
        e = (sc.f * rr)[:, None] * P2 - sc.m
        # d out / d P2 = f (rr I + (2 k1 + 4 k2 n) P2 P2');  d P2 / d P1 = [-1/z 0 x/z^2; 0 -1/z y/z^2]
        D3 = sc.f[:, None, None] * (rr[:, None, None] * np.eye(2) + (2 * sc.k1 + 4 * sc.k2 * n)[:, None, None] * P2[:, :, None] * P2[:, None, :])
        iz = 1.0 / P1[:, 2]
        D2 = np.zeros((sc.nobs, 2, 3))
        D2[:, 0, 0] = D2[:, 1, 1] = -iz
        D2[:, 0, 2], D2[:, 1, 2] = P1[:, 0] * iz * iz, P1[:, 1] * iz * iz
        J = np.einsum("oab,obc,ocd->oad", D3, D2, sc.R)
        J[~np.isfinite(J).all(axis=(1, 2)) | (P1[:, 2] == 0)] = 0.0  # (the model's Jacobian: NaN -> 0)
        l00, l10, l11 = sc.L[:, 0], sc.L[:, 1], sc.L[:, 2]
        rh = np.stack([l00 * e[:, 0] + l10 * e[:, 1], l11 * e[:, 1]], axis=1)
        Jh = np.stack([l00[:, None] * J[:, 0] + l10[:, None] * J[:, 1], l11[:, None] * J[:, 1]], axis=1)
        s = (rh * rh).sum(1)
        r_, w = rho(loss, s / c ** 2)
        f = 0.5 * sc.psum(c ** 2 * r_)
        JJ = np.einsum("oai,oaj->oij", Jh, Jh)
        H = sc.psum(np.stack([JJ[:, i, j] for i, j in _PACK], axis=1) * w[:, None])
        g = sc.psum(np.einsum("oai,oa->oi", Jh, rh) * w[:, None])
        behind = sc.psum((sc.used & (P1[:, 2] >= 0)).astype(float)) > 0
        if prior is not None:
            idx, mu, Lam = prior
            d = X[idx] - mu
            Ld = np.einsum("kij,kj->ki", Lam, d)
            f[idx] += 0.5 * (d * Ld).sum(1)
            H[idx] += np.stack([Lam[:, i, j] for i, j in _PACK], axis=1)
            g[idx] += Ld
    return f, H, g, behind, rh, Jh, w


def refine(p, x, init=0, max_iter=50, xtol=1e-10, lam0=1e-4, loss="linear", c=1.0, info=None, fixed=None, prior=None):
    """-> (x_new, status (uint8, BEHIND OR-ed in), cost (npnts, 2), trials (npnts,)).  fixed: boolean (npnts,) or None; prior:
    (0-based indices, mu (m, 3), Lambda (m, 3, 3)) or None; info: (nobs, 2, 2) or None."""
    x = np.array(x, dtype=np.float64, copy=True)
    sc = Scene(p, x, info)
    npnts = sc.npnts
    fixed = np.zeros(npnts, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    X0 = x[:3 * npnts].reshape(npnts, 3).copy()
    status = np.full(npnts, MAX_ITER, dtype=np.int64)
    status[fixed] = FIXED
    degenerate = ~fixed & (sc.deg == 0)
    X = X0.copy()
    if init == 1:
        Xt, ok = triangulate(sc)
        degenerate |= ~fixed & ~ok
        take = ~fixed & ~degenerate
        X[take] = Xt[take]
    status[degenerate] = DEGENERATE
    X[degenerate] = 0.0  # (evaluated along with the others, never used)
    f, H, g, behind, _, _, _ = evaluate(sc, X, loss, c, prior)
    cost = np.stack([f, f], axis=1)
    nonfinite = ~fixed & ~degenerate & ~np.isfinite(f)
    status[nonfinite] = NONFINITE
    active = ~fixed & ~degenerate & ~nonfinite
    lam = np.full(npnts, float(lam0))
    trials = np.zeros(npnts, dtype=np.int64)
    for _ in range(max_iter):
        if not active.any():
            break
        trials[active] += 1
        A = H.copy()
        A[:, [0, 2, 5]] += lam[:, None] * H[:, [0, 2, 5]]
        d, ok = chol3_solve(A, -g, 0.0)
        Xn = np.where((ok & active)[:, None], X + d, X)
        fn, Hn, gn, bn, _, _, _ = evaluate(sc, Xn, loss, c, prior)
        with np.errstate(invalid="ignore"):
            acc = active & ok & (fn <= f)
        rej = active & ~acc
        X[acc], f[acc], H[acc], g[acc], behind[acc] = Xn[acc], fn[acc], Hn[acc], gn[acc], bn[acc]
        lam[acc] = np.maximum(lam[acc] / 10.0, 1e-12)
        nd, nx = np.sqrt((d * d).sum(1)), np.sqrt((X * X).sum(1))
        with np.errstate(invalid="ignore"):
            conv = acc & (nd <= xtol * (nx + xtol))
        status[conv] = CONVERGED
        lam[rej] *= 10.0
        stall = rej & (lam > 1e12)
        status[stall] = STALLED
        active &= ~(conv | stall)
    cost[:, 1] = f
    cost[degenerate] = 0.0
    behind = behind & ~degenerate & ~nonfinite
    keep = degenerate | nonfinite | fixed
    X[keep] = X0[keep]
    x[:3 * npnts] = X.ravel()
    return x, (status | np.where(behind, BEHIND, 0)).astype(np.uint8), cost, trials

