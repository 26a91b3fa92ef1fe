"""numpy restatement of ba_refine_points (include/ba_hip.h, "points with the cameras held"), vectorised over the
points: the linear triangulation, the whitening by the observations' information, the losses, the point prior, the per-point
Marquardt loop and the states.  Written from the text of the header, not from the kernel: the BAL projection and its 2 x 3 point
Jacobian are derived here (P1 = R X + t, P2 = -P1.xy / P1.z, out = f (1 + k1 n + k2 n^2) P2, n = |P2|^2)."""
import numpy as np

from _lm_ref import rho  # scipy's loss table, shared with the LM reference
import block_ref as br
from block_ref import BEHIND, CONVERGED, DEGENERATE, FIXED, MAX_ITER, NONFINITE, STALLED, rotations  # noqa: F401

_PACK = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))  # packed lower 3 x 3, row-major


class Scene(br.Scene):
    """... and the held cameras of x, per observation"""

    def __init__(self, p, x, info=None):
        super().__init__(p, info)
        cams = np.asarray(x[3 * self.npnts:], dtype=np.float64).reshape(self.ncams, 9)
        self.R = rotations(cams)[self.cam0]
        self.t = cams[self.cam0, 3:6]
        self.k1, self.k2, self.f = cams[self.cam0, 6], cams[self.cam0, 7], cams[self.cam0, 8]
        self.deg = np.bincount(self.pnt0, minlength=self.npnts)

    def psum(self, v):
        """per-point sums of a per-observation array (nobs, ...)"""
        return self.gsum(self.pnt0, self.npnts, v)


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
    q = br.undistort(sc.m, sc.k1, sc.k2, sc.f[:, None])
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
        P1, _, _, _, e, D3, D2 = br.project(sc.R, X[sc.pnt0], sc.t, sc.k1, sc.k2, sc.f, sc.m)
        J = np.einsum("oab,obc,ocd->oad", D3, D2, sc.R)
        J[~np.isfinite(J).all(axis=(1, 2)) | (P1[:, 2] == 0)] = 0.0  # (the model's Jacobian: NaN -> 0)
        rh, Jh = br.whiten(sc.L, e, J)
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
    degenerate = ~fixed & (sc.deg == 0)
    X = X0.copy()
    if init == 1:
        Xt, ok = triangulate(sc)
        degenerate |= ~fixed & ~ok
        take = ~fixed & ~degenerate
        X[take] = Xt[take]
    X[degenerate] = 0.0  # (evaluated along with the others, never used)

    def solve(H, g, lam):
        A = H.copy()
        A[:, [0, 2, 5]] += lam[:, None] * H[:, [0, 2, 5]]
        return chol3_solve(A, -g, 0.0)

    X, status, cost, trials, _ = br.marquardt(X, X0, lambda Xk: evaluate(sc, Xk, loss, c, prior)[:4], solve, lambda H: 1.0, fixed,
                                              degenerate, None, max_iter, xtol, lam0)
    x[:3 * npnts] = X.ravel()
    return x, status, cost, trials
