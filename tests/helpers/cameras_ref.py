"""numpy restatement of ba_refine_cameras (include/ba_hip.h, "cameras with the points held"), vectorised over the
cameras: the whitening by the observations' information, the losses, the camera and centre priors, the held components, the
per-camera Marquardt loop with its scaled stopping test, and the states.  Written from the text of the header, not from the
kernel: the BAL projection and its 2 x 9 camera Jacobian are derived here (P1 = R(r) X + t, P2 = -P1.xy / P1.z,
out = f (1 + k1 n + k2 n^2) P2, n = |P2|^2; d(R(r) X)/dr = -R [X]x (r r' + (R' - I) [r]x) / |r|^2, Gallego & Yezzi 2015)."""
import numpy as np

from _lm_ref import centre, centre_jac, factor, rho  # scipy's loss table, the header's factor, the centre and its Jacobian

CONVERGED, STALLED, MAX_ITER, FIXED, DEGENERATE, NONFINITE = range(6)
BEHIND = 0x80
INTRINSICS = np.array([False] * 6 + [True] * 3)


def skew(v):
    """(n, 3, 3) cross-product matrices of (n, 3) vectors"""
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -v[:, 2], v[:, 1]
    K[:, 1, 0], K[:, 1, 2] = v[:, 2], -v[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -v[:, 1], v[:, 0]
    return K


def rotations(r):
    """(n, 3, 3) Rodrigues matrices of (n, 3) rotation vectors (theta = |r|, axis r / theta, no small-angle branch)"""
    th = np.sqrt((r * r).sum(1))
    k = r / th[:, None]
    c, s = np.cos(th), np.sin(th)
    return c[:, None, None] * np.eye(3) + s[:, None, None] * skew(k) + (1 - c)[:, None, None] * k[:, :, None] * k[:, None, :]


class Scene:
    """The held part of a problem: the observation lists, the measurements, the points of x and the information factors."""

    def __init__(self, p, x, info=None):
        self.npnts, self.ncams, self.nobs = p["npnts"], p["ncams"], p["nobs"]
        self.cam0 = np.asarray(p["cam_idx1"]) - 1
        self.pnt0 = np.asarray(p["pnt_idx1"]) - 1
        self.m = np.asarray(p["pt2d"], dtype=np.float64).reshape(-1, 2)
        self.X = np.asarray(x[:3 * self.npnts], dtype=np.float64).reshape(self.npnts, 3)[self.pnt0]  # per observation
        self.L = np.tile([1.0, 0.0, 1.0], (self.nobs, 1)) if info is None else np.stack(factor(np.asarray(info, dtype=np.float64)), axis=1)
        self.used = ~np.all(self.L == 0.0, axis=1)
        self.nused = np.bincount(self.cam0, weights=self.used.astype(float), minlength=self.ncams)

    def csum(self, v):
        """per-camera sums of a per-observation array (nobs, ...)"""
        flat = v.reshape(self.nobs, -1)
        out = np.stack([np.bincount(self.cam0, weights=flat[:, j], minlength=self.ncams) for j in range(flat.shape[1])], axis=1)
        return out.reshape((self.ncams,) + v.shape[1:])


def cameras(p, x):
    return np.asarray(x[3 * p["npnts"]:], dtype=np.float64).reshape(p["ncams"], 9)


def evaluate(sc, C, loss="linear", c=1.0, cam_prior=None, ctr_prior=None):
    """per camera at C (ncams, 9): f, H (ncams, 9, 9), g (ncams, 9), behind (bool); priors: (0-based indices, mu, Lambda) or
    None -- camera priors mu (m, 9), Lambda (m, 9, 9); centre priors mu (m, 3), Lambda (m, 3, 3)"""
    with np.errstate(all="ignore"):
        Co = C[sc.cam0]
        r, t, k1, k2, fo = Co[:, :3], Co[:, 3:6], Co[:, 6], Co[:, 7], Co[:, 8]
        R = rotations(r)
        P1 = np.einsum("oij,oj->oi", R, sc.X) + t
        P2 = -P1[:, :2] / P1[:, 2:3]
        n = (P2 * P2).sum(1)
        rr = 1.0 + k1 * n + k2 * n * n
        e = (fo * rr)[:, None] * P2 - sc.m
        D3 = fo[:, None, None] * (rr[:, None, None] * np.eye(2) + (2 * k1 + 4 * k2 * n)[:, None, None] * P2[:, :, None] * P2[:, None, :])
        iz = 1.0 / P1[:, 2]
        D2 = np.zeros((sc.nobs, 2, 3))
        D2[:, 0, 0] = D2[:, 1, 1] = -iz
        D2[:, 0, 2], D2[:, 1, 2] = P1[:, 0] * iz * iz, P1[:, 1] * iz * iz
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
        l00, l10, l11 = sc.L[:, 0], sc.L[:, 1], sc.L[:, 2]
        rh = np.stack([l00 * e[:, 0] + l10 * e[:, 1], l11 * e[:, 1]], axis=1)
        Jh = np.stack([l00[:, None] * J[:, 0] + l10[:, None] * J[:, 1], l11[:, None] * J[:, 1]], axis=1)
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
    C = C0.copy()
    has_prior = np.zeros(nc, dtype=bool)
    for pr in (cam_prior, ctr_prior):
        if pr is not None:
            has_prior[np.asarray(pr[0])] = True
    fixed = held.all(axis=1)
    degenerate = ~fixed & (sc.nused == 0) & ~has_prior
    f, H, g, behind = evaluate(sc, C, loss, c, cam_prior, ctr_prior)
    cost = np.stack([f, f], axis=1)
    nonfinite = ~fixed & ~degenerate & ~np.isfinite(f)
    status = np.full(nc, MAX_ITER, dtype=np.int64)
    status[fixed], status[degenerate], status[nonfinite] = FIXED, DEGENERATE, NONFINITE
    active = ~fixed & ~degenerate & ~nonfinite
    lam = np.full(nc, float(lam0))
    trials = np.zeros(nc, dtype=np.int64)
    eye = np.eye(9, dtype=bool)
    for _ in range(max_iter):
        if not active.any():
            break
        trials[active] += 1
        hh = held[:, :, None] | held[:, None, :]
        A = np.where(hh, np.eye(9)[None], H)
        A = A + lam[:, None, None] * np.where(eye[None], A, 0.0)
        b = np.where(held, 0.0, -g)
        d, ok = chol_solve(A, b)
        d = np.where(held, 0.0, d)
        D = scales(H, held)
        Cn = np.where((ok & active)[:, None] & ~held, C + d, C)
        fn, Hn, gn, bn = evaluate(sc, Cn, loss, c, cam_prior, ctr_prior)
        with np.errstate(invalid="ignore"):
            acc = active & ok & (fn <= f)
        rej = active & ~acc
        C[acc], f[acc], H[acc], g[acc], behind[acc] = Cn[acc], fn[acc], Hn[acc], gn[acc], bn[acc]
        lam[acc] = np.maximum(lam[acc] / 10.0, 1e-12)
        with np.errstate(invalid="ignore"):
            nd, nx = np.sqrt(((D * d) ** 2).sum(1)), np.sqrt(((D * C) ** 2).sum(1))
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
    C[keep] = C0[keep]
    x[3 * sc.npnts:] = C.ravel()
    return x, (status | np.where(behind, BEHIND, 0)).astype(np.uint8), cost, trials, scales(H, held)
