"""numpy restatement of ba_refine_cameras (include/ba_hip.h, "cameras with the points held"), vectorised over the
cameras: the whitening by the observations' information, the losses, the camera and centre priors, the held components, the
per-camera Marquardt loop with its scaled stopping test, and the states.  Written from the text of the header, not from the
kernel: the BAL projection and its 2 x 9 camera Jacobian are derived here (P1 = R(r) X + t, P2 = -P1.xy / P1.z,
out = f (1 + k1 n + k2 n^2) P2, n = |P2|^2; d(R(r) X)/dr = -R [X]x (r r' + (R' - I) [r]x) / |r|^2, Gallego & Yezzi 2015)."""
import numpy as np

from _lm_ref import centre, centre_jac, rho  # noqa: F401 -- scipy's loss table, the centre and its Jacobian
import block_ref as br
from block_ref import BEHIND, CONVERGED, DEGENERATE, FIXED, MAX_ITER, NONFINITE, STALLED, rotations, skew  # noqa: F401

INTRINSICS = np.array([False] * 6 + [True] * 3)


class Scene(br.Scene):
    """... and the held points of x, per observation"""

    def __init__(self, p, x, info=None):
        super().__init__(p, info)
        self.X = np.asarray(x[:3 * self.npnts], dtype=np.float64).reshape(self.npnts, 3)[self.pnt0]
        self.nused = np.bincount(self.cam0, weights=self.used.astype(float), minlength=self.ncams)

    def csum(self, v):
        """per-camera sums of a per-observation array (nobs, ...)"""
        return self.gsum(self.cam0, self.ncams, v)


def cameras(p, x):
    return np.asarray(x[3 * p["npnts"]:], dtype=np.float64).reshape(p["ncams"], 9)


def evaluate(sc, C, loss="linear", c=1.0, cam_prior=None, ctr_prior=None):
    """per camera at C (ncams, 9): f, H (ncams, 9, 9), g (ncams, 9), behind (bool); priors: (0-based indices, mu, Lambda) or
    None -- camera priors mu (m, 9), Lambda (m, 9, 9); centre priors mu (m, 3), Lambda (m, 3, 3)"""
    with np.errstate(all="ignore"):
        Co = C[sc.cam0]
        r, t, k1, k2, fo = Co[:, :3], Co[:, 3:6], Co[:, 6], Co[:, 7], Co[:, 8]
        R = rotations(r)
        P1, P2, n, rr, e, D3, D2 = br.project(R, sc.X, t, k1, k2, fo, sc.m)
        D32 = np.einsum("oab,obc->oac", D3, D2)
        th2 = (r * r).sum(1)
        inner = r[:, :, None] * r[:, None, :] + np.einsum("oij,ojk->oik", np.swapaxes(R, 1, 2) - np.eye(3), skew(r))
        G = -np.einsum("oij,ojk,okl->oil", R, skew(sc.X), inner) / th2[:, None, None]
        J = np.zeros((sc.nobs, 2, 9))
        J[:, :, 0:3] = np.einsum("oab,obc->oac", D32, G)
        J[:, :, 3:6] = D32
        J[:, :, 6] = (fo * n)[:, None] * P2
        J[:, :, 7] = (fo * n * n)[:, None] * P2
        J[:, :, 8] = rr[:, None] * P2
        J[~np.isfinite(J).all(axis=(1, 2)) | (P1[:, 2] == 0)] = 0.0  # (the model's Jacobian: NaN -> 0)
        rh, Jh = br.whiten(sc.L, e, J)
        rh[~sc.used] = 0.0  # Lambda = 0: dropped, whatever the projection gives
        Jh[~sc.used] = 0.0
        r_, w = rho(loss, (rh * rh).sum(1) / c ** 2)
        f = 0.5 * sc.csum(c ** 2 * r_)
        H = sc.csum(np.einsum("oai,oaj->oij", Jh, Jh) * w[:, None, None])
        g = sc.csum(np.einsum("oai,oa->oi", Jh, rh) * w[:, None])
        behind = sc.csum((sc.used & (P1[:, 2] >= 0)).astype(float)) > 0
        if cam_prior is not None:
            idx, mu, Lam = cam_prior
            d = C[idx] - mu
            Ld = np.einsum("kij,kj->ki", Lam, d)
            f[idx] += 0.5 * (d * Ld).sum(1)
            H[idx] += Lam
            g[idx] += Ld
        if ctr_prior is not None:
            idx, mu, Lam = ctr_prior
            for q, i in enumerate(idx):
                d = centre(C[i]) - mu[q]
                Hc = centre_jac(C[i])
                f[i] += 0.5 * d @ Lam[q] @ d
                H[i, :6, :6] += Hc.T @ Lam[q] @ Hc
                g[i, :6] += Hc.T @ (Lam[q] @ d)
    return f, H, g, behind


def chol_solve(A, b):
    """x of A x = b for (n, 9, 9) blocks by Cholesky, and ok (n,): every pivot positive and finite, x finite"""
    n, m = A.shape[0], A.shape[1]
    L = np.zeros_like(A)
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(m):
            s = A[:, j, j] - (L[:, j, :j] ** 2).sum(1)
            ok &= (s > 0) & np.isfinite(s)
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, m):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / L[:, j, j]
        y = np.zeros_like(b)
        for i in range(m):
            y[:, i] = (b[:, i] - (L[:, i, :i] * y[:, :i]).sum(1)) / L[:, i, i]
        x = np.zeros_like(b)
        for i in range(m - 1, -1, -1):
            x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(1)) / L[:, i, i]
        ok &= np.isfinite(x).all(axis=1)
    return x, ok


def scales(H, held):
    """D (ncams, 9): sqrt(H_jj), 0 on held components"""
    with np.errstate(invalid="ignore"):
        return np.where(held, 0.0, np.sqrt(np.einsum("cii->ci", H)))


def held_mask(p, held=None, groups=None):
    """boolean (ncams, 9): the mask of held components, with (k1, k2, f) of every member of a group (labels (ncams,), 0 = own)"""
    out = np.zeros((p["ncams"], 9), dtype=bool) if held is None else np.array(held, dtype=bool, copy=True)
    if groups is not None:
        out[np.asarray(groups) > 0] |= INTRINSICS
    return out


def refine(p, x, max_iter=100, xtol=1e-10, lam0=1e-4, loss="linear", c=1.0, info=None, held=None, groups=None, cam_prior=None,
           ctr_prior=None):
    """-> (x_new, status (uint8, BEHIND OR-ed in), cost (ncams, 2), trials (ncams,), D (ncams, 9) at the returned cameras)"""
    x = np.array(x, dtype=np.float64, copy=True)
    sc = Scene(p, x, info)
    nc = sc.ncams
    held = held_mask(p, held, groups)
    C0 = cameras(p, x).copy()
    has_prior = np.zeros(nc, dtype=bool)
    for pr in (cam_prior, ctr_prior):
        if pr is not None:
            has_prior[np.asarray(pr[0])] = True
    fixed = held.all(axis=1)
    degenerate = ~fixed & (sc.nused == 0) & ~has_prior
    eye = np.eye(9, dtype=bool)

    def solve(H, g, lam):
        hh = held[:, :, None] | held[:, None, :]
        A = np.where(hh, np.eye(9)[None], H)
        A = A + lam[:, None, None] * np.where(eye[None], A, 0.0)
        d, ok = chol_solve(A, np.where(held, 0.0, -g))
        return np.where(held, 0.0, d), ok

    C, status, cost, trials, H = br.marquardt(C0.copy(), C0, lambda Ck: evaluate(sc, Ck, loss, c, cam_prior, ctr_prior), solve,
                                              lambda H: scales(H, held), fixed, degenerate, held, max_iter, xtol, lam0)
    x[3 * sc.npnts:] = C.ravel()
    return x, status, cost, trials, scales(H, held)
