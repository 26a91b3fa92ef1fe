"""What the numpy restatements of the block refinements share (points_ref.py: ba_refine_points, cameras_ref.py: ba_refine_cameras,
resect_ref.py: ba_resect_cameras; include/ba_hip.h): the states, the Rodrigues rotation, the held part of a
problem, the BAL projection with its two inner Jacobians, the whitening, the undistortion and the per-block Marquardt loop.
Written from the text of the header, not from the kernels: P1 = R X + t, P2 = -P1.xy / P1.z, out = f (1 + k1 n + k2 n^2) P2,
n = |P2|^2."""
import numpy as np

from _lm_ref import factor  # the header's factor L of Lambda = L L'

CONVERGED, STALLED, MAX_ITER, FIXED, DEGENERATE, NONFINITE = range(6)
BEHIND = 0x80
UNDIST_ITERS = 8


def skew(v):
    """(n, 3, 3) cross-product matrices of (n, 3) vectors"""
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -v[:, 2], v[:, 1]
    K[:, 1, 0], K[:, 1, 2] = v[:, 2], -v[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -v[:, 1], v[:, 0]
    return K


def rotations(r):
    """(n, 3, 3) Rodrigues matrices of (n, 3) rotation vectors, or of the cameras (n, 9) that start with them (theta = |r|, axis
    r / theta, no small-angle branch)"""
    r = r[:, :3]
    th = np.sqrt((r * r).sum(1))
    k = r / th[:, None]
    c, s = np.cos(th), np.sin(th)
    return c[:, None, None] * np.eye(3) + s[:, None, None] * skew(k) + (1 - c)[:, None, None] * k[:, :, None] * k[:, None, :]


class Scene:
    """What both sides hold of a problem: the observation lists, the measurements and the information factors."""

    def __init__(self, p, info=None):
        self.npnts, self.ncams, self.nobs = p["npnts"], p["ncams"], p["nobs"]
        self.cam0 = np.asarray(p["cam_idx1"]) - 1
        self.pnt0 = np.asarray(p["pnt_idx1"]) - 1
        self.m = np.asarray(p["pt2d"], dtype=np.float64).reshape(-1, 2)
        self.L = np.tile([1.0, 0.0, 1.0], (self.nobs, 1)) if info is None else np.stack(factor(np.asarray(info, dtype=np.float64)), axis=1)
        self.used = ~np.all(self.L == 0.0, axis=1)

    def gsum(self, idx, n, v):
        """sums of a per-observation array (nobs, ...) over the n groups of the index idx (nobs,)"""
        flat = v.reshape(self.nobs, -1)
        out = np.stack([np.bincount(idx, weights=flat[:, j], minlength=n) for j in range(flat.shape[1])], axis=1)
        return out.reshape((n,) + v.shape[1:])


def project(R, X, t, k1, k2, f, m):
    """per observation: P1, P2, n, rr = 1 + k1 n + k2 n^2, the residual e = f rr P2 - m, D3 = d out / d P2 (2 x 2) and
    D2 = d P2 / d P1 (2 x 3).  (Called under np.errstate(all="ignore").)"""
    P1 = np.einsum("oij,oj->oi", R, X) + t
    P2 = -P1[:, :2] / P1[:, 2:3]
    n = (P2 * P2).sum(1)
    rr = 1.0 + k1 * n + k2 * n * n
    e = (f * rr)[:, None] * P2 - m
    # d out / d P2 = f (rr I + (2 k1 + 4 k2 n) P2 P2');  d P2 / d P1 = [-1/z 0 x/z^2; 0 -1/z y/z^2]
    D3 = f[:, None, None] * (rr[:, None, None] * np.eye(2) + (2 * k1 + 4 * k2 * n)[:, None, None] * P2[:, :, None] * P2[:, None, :])
    iz = 1.0 / P1[:, 2]
    D2 = np.zeros((len(P1), 2, 3))
    D2[:, 0, 0] = D2[:, 1, 1] = -iz
    D2[:, 0, 2], D2[:, 1, 2] = P1[:, 0] * iz * iz, P1[:, 1] * iz * iz
    return P1, P2, n, rr, e, D3, D2


def whiten(L, e, J):
    """r^ = L'e (nobs, 2) and J^ = L'J (nobs, 2, k) of the factors L (nobs, 3: l00 l10 l11)"""
    l00, l10, l11 = L[:, 0], L[:, 1], L[:, 2]
    rh = np.stack([l00 * e[:, 0] + l10 * e[:, 1], l11 * e[:, 1]], axis=1)
    Jh = np.stack([l00[:, None] * J[:, 0] + l10[:, None] * J[:, 1], l11[:, None] * J[:, 1]], axis=1)
    return rh, Jh


def undistort(m, k1, k2, f):
    """(n, 2) measurements -> normalised image points: u = m / f, 8 iterations of q <- u / (1 + k1 |q|^2 + k2 |q|^4)"""
    with np.errstate(all="ignore"):
        u = m / f
        q = u.copy()
        for _ in range(UNDIST_ITERS):
            n2 = (q * q).sum(1)
            q = u / (1.0 + k1 * n2 + k2 * n2 * n2)[:, None]
    return q


def marquardt(Z, Z0, evaluate, solve, scale, fixed, degenerate, held=None, max_iter=50, xtol=1e-10, lam0=1e-4):
    """The per-block Marquardt loop, vectorised over the blocks, from the start Z (nblocks, k); Z0: what a block that is not
    refined comes back with.  evaluate(Z) -> f, H, g, behind; solve(H, g, lam) -> delta, ok (the damped step); scale(H) -> D of
    the stopping test |D delta| <= xtol (|D Z| + xtol); held: boolean (nblocks, k) of components that do not move, or None.
    -> (Z, status (uint8, BEHIND OR-ed in), cost (nblocks, 2), trials (nblocks,), H at the returned blocks)"""
    nb = len(Z)
    f, H, g, behind = evaluate(Z)
    cost = np.stack([f, f], axis=1)
    nonfinite = ~fixed & ~degenerate & ~np.isfinite(f)
    status = np.full(nb, MAX_ITER, dtype=np.int64)
    status[fixed], status[degenerate], status[nonfinite] = FIXED, DEGENERATE, NONFINITE
    active = ~fixed & ~degenerate & ~nonfinite
    lam = np.full(nb, float(lam0))
    trials = np.zeros(nb, dtype=np.int64)
    for _ in range(max_iter):
        if not active.any():
            break
        trials[active] += 1
        d, ok = solve(H, g, lam)
        D = scale(H)
        move = (ok & active)[:, None] if held is None else (ok & active)[:, None] & ~held
        Zn = np.where(move, Z + d, Z)
        fn, Hn, gn, bn = evaluate(Zn)
        with np.errstate(invalid="ignore"):
            acc = active & ok & (fn <= f)
        rej = active & ~acc
        Z[acc], f[acc], H[acc], g[acc], behind[acc] = Zn[acc], fn[acc], Hn[acc], gn[acc], bn[acc]
        lam[acc] = np.maximum(lam[acc] / 10.0, 1e-12)
        with np.errstate(invalid="ignore"):
            nd, nx = np.sqrt(((D * d) ** 2).sum(1)), np.sqrt(((D * Z) ** 2).sum(1))
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
    Z[keep] = Z0[keep]
    return Z, (status | np.where(behind, BEHIND, 0)).astype(np.uint8), cost, trials, H
