"""Translation averaging over the view graph (include/ba_hip.h, "translation averaging") restated in numpy: the arc
distance and the loop counts, the filter, the forest start, the linearisation, the preconditioned conjugate gradient with the
device's stop rule, the Levenberg-Marquardt control and the gauge.  Cameras are 0-based in here except in `pairs` (1-based, as
the package takes them).  Sums over a camera's pairs are taken with np.add.at in the order of the directed edge list, which
`edge_seed` permutes: the spread between two such runs is the reference's own rounding."""
import numpy as np

import rotavg_ref as ra
from rotavg_ref import STATES, rho  # noqa: F401

NAN = float("nan")
MIN_LENGTH = 1e-12


def normalise(dirs):
    """(usable, d): finite with a norm >= 1e-12; d = dirs / norm (NaN where not usable)"""
    v = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        usable = np.isfinite(v).all(axis=1) & (nn >= MIN_LENGTH)
        d = np.where(usable[:, None], v / np.where(usable, nn, 1.0)[:, None], NAN)
    return usable, d


def angle(x, y):
    return float(np.arctan2(np.linalg.norm(np.cross(x, y)), x @ y))


def arc_distance(d, d1, d2):
    """the distance of d to the shorter arc from d1 to d2, or None where d1 and d2 are opposite"""
    n = np.cross(d1, d2)
    nn = np.linalg.norm(n)
    if nn < 1e-6:
        return angle(d, d1) if d1 @ d2 > 0 else None
    n = n / nn
    h = d @ n
    q = d - h * n
    if np.cross(d1, q) @ n >= 0 and np.cross(q, d2) @ n >= 0:
        return float(np.arcsin(min(1.0, abs(h))))
    return min(angle(d, d1), angle(d, d2))


def _pairs0(pairs):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return p[:, 0] - 1, p[:, 1] - 1


def loops(ncams, pairs, dirs, threshold, used=None):
    """(n_loops, support, distances, unchecked): per pair the checked triangles and those with a distance <= threshold; every
    distance evaluated; the number of triangles that could not be checked"""
    a, b = _pairs0(pairs)
    usable, d = normalise(dirs)
    use = usable if used is None else usable & np.asarray(used, dtype=bool)
    to, nb = {}, [set() for _ in range(ncams)]
    for k in np.flatnonzero(use):
        to[(a[k], b[k])], to[(b[k], a[k])] = d[k], -d[k]
        nb[a[k]].add(b[k]), nb[b[k]].add(a[k])
    n_loops, support, dist, unchecked = np.zeros(len(a), dtype=np.int32), np.zeros(len(a), dtype=np.int32), [], 0
    for k in np.flatnonzero(use):
        for c in sorted(nb[a[k]] & nb[b[k]]):
            e = arc_distance(d[k], to[(a[k], c)], to[(c, b[k])])
            if e is None:
                unchecked += 1
                continue
            n_loops[k] += 1
            support[k] += e <= threshold
            dist.append(e)
    return n_loops, support, np.array(dist), unchecked


def lm_decide(F, F_trial, lam, iteration, max_iterations, ftol):
    """(accepted, stop, the next lambda): ba_transavg_lm_decide"""
    accepted = bool(F_trial < F)
    lam = max(lam / 3.0, 1e-9) if accepted else 4.0 * lam
    stop = 1 if abs(F - F_trial) <= ftol * F else 2 if lam > 1e8 else 3 if iteration >= max_iterations else 0
    return accepted, stop, lam


def linearise(c, a, b, d, wt, kept, loss, c2):
    """(A (n, 3, 3), g (n, 3), F, rho' (n,)): zeros on pairs that are not kept"""
    n = len(a)
    A, g, rw, val = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    kk = np.flatnonzero(kept)
    u = c[b[kk]] - c[a[kk]]
    nu = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
    ok = nu >= MIN_LENGTH
    uh = u / np.where(ok, nu, 1.0)[:, None]
    r = uh - d[kk]
    s = np.where(ok, (r * r).sum(axis=1), 4.0)
    v, der = rho(loss, s / c2)
    om = np.where(ok, wt[kk] * der, 0.0)
    h = (uh * r).sum(axis=1)
    safe = np.where(ok, nu, 1.0)
    g[kk] = (om / safe)[:, None] * (r - h[:, None] * uh)
    A[kk] = (om / (safe * safe))[:, None, None] * (np.eye(3) - uh[:, :, None] * uh[:, None, :])
    rw[kk], val[kk] = der, wt[kk] * c2 * v
    return A, g, 0.5 * float(val.sum()), rw


class System:
    """(H + lambda diag H) delta = -g over the directed edges of the kept pairs"""

    def __init__(self, ncams, a, b, kept, fixed, edge_seed=None):
        kk = np.flatnonzero(kept)
        self.n = ncams
        self.ei, self.ej = np.concatenate([a[kk], b[kk]]), np.concatenate([b[kk], a[kk]])
        self.ek, self.sign = np.concatenate([kk, kk]), np.concatenate([-np.ones(len(kk)), np.ones(len(kk))])
        if edge_seed is not None:
            perm = np.random.default_rng(edge_seed).permutation(len(self.ei))
            self.ei, self.ej, self.ek, self.sign = self.ei[perm], self.ej[perm], self.ek[perm], self.sign[perm]
        self.fixed = fixed

    def assemble(self, A, g, lam):
        self.A = A
        self.gc, D = np.zeros((self.n, 3)), np.zeros((self.n, 3, 3))
        np.add.at(self.gc, self.ei, self.sign[:, None] * g[self.ek])
        np.add.at(D, self.ei, A[self.ek])
        self.dg = lam * np.diagonal(D, axis1=1, axis2=2)
        S = D + self.dg[:, :, None] * np.eye(3)
        c00 = S[:, 1, 1] * S[:, 2, 2] - S[:, 1, 2] * S[:, 1, 2]
        c01 = S[:, 0, 2] * S[:, 1, 2] - S[:, 0, 1] * S[:, 2, 2]
        c02 = S[:, 0, 1] * S[:, 1, 2] - S[:, 0, 2] * S[:, 1, 1]
        det = (S[:, 0, 0] * c00 + S[:, 0, 1] * c01) + S[:, 0, 2] * c02
        tr = (S[:, 0, 0] + S[:, 1, 1]) + S[:, 2, 2]
        self.active = (det > 1e-12 * ((tr * tr) * tr)) & ~self.fixed
        self.Minv = np.zeros((self.n, 3, 3))
        self.Minv[self.active] = np.linalg.inv(S[self.active])

    def matvec(self, p):
        y = np.zeros((self.n, 3))
        np.add.at(y, self.ei, np.einsum("kij,kj->ki", self.A[self.ek], p[self.ei] - p[self.ej]))
        return np.where(self.active[:, None], y + self.dg * p, 0.0)

    def dense(self):
        """(the matrix and the right-hand side over the active cameras, their indices)"""
        idx = np.flatnonzero(self.active)
        pos = -np.ones(self.n, dtype=np.int64)
        pos[idx] = np.arange(len(idx))
        H = np.zeros((3 * len(idx), 3 * len(idx)))
        for i, j, k in zip(self.ei, self.ej, self.ek):
            if pos[i] < 0:
                continue
            H[3 * pos[i]:3 * pos[i] + 3, 3 * pos[i]:3 * pos[i] + 3] += self.A[k]
            if pos[j] >= 0:
                H[3 * pos[i]:3 * pos[i] + 3, 3 * pos[j]:3 * pos[j] + 3] -= self.A[k]
        H[np.arange(len(H)), np.arange(len(H))] += self.dg[idx].ravel()
        return H, -self.gc[idx].ravel(), idx

    def pcg(self, cg_tol, max_cg):
        """(delta, iterations, |r|_M per iteration, |r0|_M)"""
        x = np.zeros((self.n, 3))
        r = np.where(self.active[:, None], -self.gc, 0.0)
        z = np.einsum("kij,kj->ki", self.Minv, r)
        p = z.copy()
        rz = float((r * z).sum(axis=1).sum())
        r0 = np.sqrt(rz)
        norms = []
        if not r0 > 0:
            return x, 0, norms, r0
        for _ in range(max_cg):
            q = self.matvec(p)
            pq = float((p * q).sum(axis=1).sum())
            if not pq > 0:
                break
            al = rz / pq
            x, r = x + al * p, r - al * q
            z = np.einsum("kij,kj->ki", self.Minv, r)
            rzn = float((r * z).sum(axis=1).sum())
            norms.append(np.sqrt(rzn))
            if not norms[-1] > cg_tol * r0:
                break
            p, rz = z + (rzn / rz) * p, rzn
        return x, len(norms), norms, r0


def average(ncams, pairs, dirs, weights=None, used=None, loops_opt=None, c0=None, fixed=None, loss="linear", f_scale=None,
            max_iterations=50, ftol=1e-10, cg_tol=1e-6, max_cg=500, lambda0=1e-3, edge_seed=None):
    """average_translations of the package; beside its dict: `c_start`, `forest`, `solves` (per iteration: |r|_M per
    conjugate-gradient iteration and |r0|_M), `F` (per iteration: the cost of the iterate before the trial) and `first` (the
    System of the first iteration with its delta).  fixed: boolean (ncams,)"""
    a, b = _pairs0(pairs)
    n = len(a)
    usable, d = normalise(dirs)
    use = usable if used is None else usable & np.asarray(used, dtype=bool)
    wt = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    fx = np.zeros(ncams, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    c2 = 1.0 if loss == "linear" else float(f_scale) ** 2
    out = {}
    kept, sup = use.copy(), None
    if loops_opt is not None:
        nl, sup, _, _ = loops(ncams, pairs, dirs, loops_opt["threshold"], used=use)
        ratio = loops_opt.get("min_ratio", 0.34)
        kept &= ~((nl > 0) & ((sup < loops_opt.get("min_support", 1)) | (sup.astype(np.float64) < ratio * nl.astype(np.float64))))
        out.update(n_loops=nl, support=sup)
    f = ra.forest(ncams, pairs, used=kept, support=sup, weights=wt, fixed=fx)
    comp = f["component"]
    fx = fx & (comp >= 0)
    if c0 is not None:
        c = np.where(comp[:, None] >= 0, np.asarray(c0, dtype=np.float64), 0.0)
    else:
        c = np.zeros((ncams, 3))
        for i in f["order"] - 1:
            k = f["parent_pair"][i]
            if k >= 0:
                c[i] = c[a[k]] + d[k] if b[k] == i else c[b[k]] - d[k]
    c_start = c.copy()
    sys_ = System(ncams, a, b, kept, fx, edge_seed=edge_seed)
    A, g, F, _ = linearise(c, a, b, d, wt, kept, loss, c2)
    cost_before, lam, it, trace, solves, Fs, first, cg_total = F, lambda0, 0, [], [], [], None, 0
    while kept.any():
        it += 1
        sys_.assemble(A, g, lam)
        delta, cg, norms, r0 = sys_.pcg(cg_tol, max_cg)
        if first is None:
            first = dict(H=sys_.dense(), delta=delta.copy(), active=sys_.active.copy())
        trial = c + delta
        At, gt, Ft, _ = linearise(trial, a, b, d, wt, kept, loss, c2)
        accepted, stop, lam_next = lm_decide(F, Ft, lam, it, max_iterations, ftol)
        trace.append((Ft, lam, cg, float(accepted)))
        solves.append((norms, r0))
        Fs.append(F)
        cg_total += cg
        lam = lam_next
        if accepted:
            c, A, g, F = trial, At, gt, Ft
        if stop:
            break
    # the gauge
    length = lambda v: np.sqrt(((v[b] - v[a]) ** 2).sum(axis=1))  # noqa: E731
    l0, l1 = length(c_start), length(c)
    for gi, root in enumerate(f["roots"] - 1):
        mem = comp == gi
        if fx[mem].any():
            continue
        kk = kept & (comp[a] == gi)
        s = l0[kk].sum() / l1[kk].sum()
        c[mem] = c_start[root] + (s if np.isfinite(s) and s > 0 else 1.0) * (c[mem] - c[root])
    _, _, cost_after, rw = linearise(c, a, b, d, wt, kept, loss, c2)
    residual = np.full(n, NAN)
    inside = usable & (comp[a] >= 0) & (comp[a] == comp[b])
    u = c[b] - c[a]
    nu = np.linalg.norm(u, axis=1)
    for k in np.flatnonzero(inside & (nu >= MIN_LENGTH)):
        residual[k] = angle(u[k] / nu[k], d[k])
    c_out = np.where(comp[:, None] >= 0, c, NAN)
    is_root = np.zeros(ncams, dtype=bool)
    is_root[f["roots"] - 1] = True
    status = np.where(comp < 0, "isolated", np.where(fx, "fixed", np.where(is_root, "root", "ok")))
    out.update(c=c_out, c_start=c_start, status=status, component=comp, kept=kept, residual=residual, edge_weight=rw, iterations=it,
               cg_iterations=cg_total, trace=np.array(trace).reshape(-1, 4), cost_before=cost_before, cost_after=cost_after, forest=f,
               solves=solves, F=np.array(Fs), first=first, counts={s: int((status == s).sum()) for s in STATES})
    return out


def align(c, c_true):
    """c under the similarity (scale, rotation, shift) that brings it closest to c_true (Umeyama), over the finite rows"""
    ok = np.isfinite(c).all(axis=1)
    x, y = c[ok], c_true[ok]
    mx, my = x.mean(axis=0), y.mean(axis=0)
    U, S, Vt = np.linalg.svd((y - my).T @ (x - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = (S * np.diag(D)).sum() / ((x - mx) ** 2).sum()
    out = np.full_like(c, NAN)
    out[ok] = s * (x - mx) @ R.T + my
    return out
