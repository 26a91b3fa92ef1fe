"""Rotation averaging over the view graph (include/ba_hip.h, "rotation averaging") restated in numpy: the loop
counts, the maximum spanning forest and the averaging itself.  Cameras are 0-based in here except in `pairs` (1-based, as the
package takes them) and in the forest's `order` and `roots` (1-based, as it returns them).  Sums over a camera's pairs are
taken with np.add.at in the order of the directed edge list, which `edge_seed` permutes: the spread between two such runs is
the reference's own rounding."""
import numpy as np

NAN = float("nan")


def exp_many(v):
    """(n, 3, 3): Rodrigues, the identity at |v| = 0"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    th = np.sqrt((v * v).sum(axis=1))
    k = v / np.where(th > 0, th, 1.0)[:, None]
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    return c * np.eye(3) + s * K + (1.0 - c) * k[:, :, None] * k[:, None, :]


def angle_many(M):
    """atan2(|w| / 2, (tr M - 1) / 2), w the skew part"""
    w = np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], axis=1)
    return np.arctan2(0.5 * np.sqrt((w * w).sum(axis=1)), 0.5 * (np.trace(M, axis1=1, axis2=2) - 1.0))


def rotation_vector(R, identity=(1e-12, 0.0, 0.0)):
    """the library's rule for one matrix: theta w / |w|; for cos theta < 0 the axis from the row of the largest diagonal entry
    of the symmetric part with the sign of w; theta < 1e-12: `identity`"""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    wn = np.sqrt(w @ w)
    co = 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(0.5 * wn, co)
    if not th >= 1e-12:
        return np.array(identity) if th < 1e-12 else np.full(3, NAN)
    if co >= 0:
        return th * w / wn
    i = int(np.argmax(np.diag(R)))
    ki = np.sqrt((R[i, i] - co) / (1.0 - co))
    k = np.array([ki if j == i else 0.5 * (R[i, j] + R[j, i]) / ((1.0 - co) * ki) for j in range(3)])
    k = k / np.sqrt(k @ k)
    return th * (-k if k @ w < 0 else k)


def log_many(M):
    """Log: the rotation vector with 0 for theta < 1e-12"""
    w = np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], axis=1)
    wn = np.sqrt((w * w).sum(axis=1))
    co = 0.5 * (np.trace(M, axis1=1, axis2=2) - 1.0)
    th = np.arctan2(0.5 * wn, co)
    v = np.zeros((len(M), 3))
    near = (th >= 1e-12) & (co >= 0)
    v[near] = (th[near] / wn[near])[:, None] * w[near]
    for i in np.flatnonzero(~near & ~(th < 1e-12)):
        v[i] = rotation_vector(M[i], identity=(0.0, 0.0, 0.0))
    return v


def rho(loss, z):
    """(rho(z), rho'(z)) of scipy's losses"""
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return z.copy(), np.ones_like(z)
    if loss == "huber":
        big = z > 1.0
        sz = np.sqrt(np.where(big, z, 1.0))
        return np.where(big, 2.0 * sz - 1.0, z), np.where(big, 1.0 / sz, 1.0)
    if loss == "soft_l1":
        t = np.sqrt(1.0 + z)
        return 2.0 * (t - 1.0), 1.0 / t
    if loss == "cauchy":
        return np.log1p(z), 1.0 / (1.0 + z)
    if loss == "arctan":
        return np.arctan(z), 1.0 / (1.0 + z * z)
    raise ValueError(loss)


def _pairs0(pairs):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return p[:, 0] - 1, p[:, 1] - 1


def _used(r, used):
    fin = np.isfinite(np.asarray(r, dtype=np.float64).reshape(-1, 3)).all(axis=1)
    return fin, fin if used is None else fin & np.asarray(used, dtype=bool)


def loops(ncams, pairs, r, threshold, used=None):
    """(n_loops, support, angles): per pair the triangles through it and those with angle <= threshold; every angle evaluated"""
    a, b = _pairs0(pairs)
    _, use = _used(r, used)
    Rk = exp_many(np.where(np.isfinite(r), r, 0.0))
    to = {}  # (i, j) -> R_{i -> j}
    nb = [set() for _ in range(ncams)]
    for k in np.flatnonzero(use):
        to[(a[k], b[k])], to[(b[k], a[k])] = Rk[k], Rk[k].T
        nb[a[k]].add(b[k]), nb[b[k]].add(a[k])
    n_loops, support, angles = np.zeros(len(a), dtype=np.int32), np.zeros(len(a), dtype=np.int32), []
    for k in np.flatnonzero(use):
        common = sorted(nb[a[k]] & nb[b[k]])
        if not common:
            continue
        L = np.array([to[(c, a[k])] @ to[(b[k], c)] @ to[(a[k], b[k])] for c in common])
        ang = angle_many(L)
        n_loops[k], support[k] = len(common), int((ang <= threshold).sum())
        angles.append(ang)
    return n_loops, support, np.concatenate(angles) if angles else np.zeros(0)


def forest(ncams, pairs, used=None, support=None, weights=None, fixed=None):
    """the maximum spanning forest: dict(component, parent_pair, order (1-based), roots (1-based), n_components)"""
    a, b = _pairs0(pairs)
    n = len(a)
    use = np.ones(n, dtype=bool) if used is None else np.asarray(used, dtype=bool)
    sup = np.zeros(n, dtype=np.int64) if support is None else np.asarray(support, dtype=np.int64)
    wt = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    fx = np.zeros(ncams, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    label = np.arange(ncams)
    tree = []
    for k in sorted(np.flatnonzero(use), key=lambda k: (-sup[k], -wt[k], k)):
        if label[a[k]] != label[b[k]]:
            label[label == label[b[k]]] = label[a[k]]
            tree.append(k)
    touched = np.zeros(ncams, dtype=bool)
    wsum = np.zeros(ncams)
    for k in np.flatnonzero(use):
        touched[a[k]] = touched[b[k]] = True
        wsum[a[k]] += wt[k]
        wsum[b[k]] += wt[k]
    component, ids = np.full(ncams, -1, dtype=np.int32), {}
    for c in np.flatnonzero(touched):
        component[c] = ids.setdefault(label[c], len(ids))
    roots = []
    for g in range(len(ids)):
        mem = np.flatnonzero(component == g)
        held = mem[fx[mem]]
        roots.append(int(held[0]) if held.size else int(mem[np.argmax(wsum[mem])]))  # (argmax: the first of the largest)
    nbr = [[] for _ in range(ncams)]
    for k in tree:
        nbr[a[k]].append((b[k], k)), nbr[b[k]].append((a[k], k))
    parent, order, seen = np.full(ncams, -1, dtype=np.int64), [], np.zeros(ncams, dtype=bool)
    for root in roots:
        queue = [root]
        seen[root] = True
        while queue:
            c = queue.pop(0)
            order.append(c)
            for j, k in sorted(nbr[c]):
                if not seen[j]:
                    seen[j], parent[j] = True, k
                    queue.append(j)
    return dict(component=component, parent_pair=parent, order=np.array(order, dtype=np.int64) + 1,
                roots=np.array(roots, dtype=np.int64) + 1, n_components=len(ids))


STATES = ("ok", "root", "fixed", "isolated")


def average(ncams, pairs, r, weights=None, used=None, loops_opt=None, r0=None, fixed=None, loss="linear", f_scale=None, damping=0.8,
            max_sweeps=1000, xtol=1e-6, edge_seed=None):
    """average_rotations of the package; `R` (ncams, 3, 3) and `R_start` are returned beside its dict.  fixed: boolean (ncams,)"""
    a, b = _pairs0(pairs)
    n = len(a)
    r = np.asarray(r, dtype=np.float64).reshape(n, 3)
    fin, use = _used(r, used)
    wt = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    fx = np.zeros(ncams, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    c2 = 1.0 if loss == "linear" else float(f_scale) ** 2
    Rk = exp_many(np.where(np.isfinite(r), r, 0.0))
    out = {}
    kept = use.copy()
    sup = None
    if loops_opt is not None:
        nl, sup, _ = loops(ncams, pairs, r, loops_opt["threshold"], used=use)
        kept &= ~((nl > 0) & (sup < loops_opt.get("min_support", 1)))
        out.update(n_loops=nl, support=sup)
    f = forest(ncams, pairs, used=kept, support=sup, weights=wt, fixed=fx)
    comp = f["component"]
    fx = fx & (comp >= 0)
    # the start
    if r0 is not None:
        R = exp_many(np.where(comp[:, None] >= 0, np.asarray(r0, dtype=np.float64), 0.0))
    else:
        R = np.tile(np.eye(3), (ncams, 1, 1))
        for c in f["order"] - 1:
            k = f["parent_pair"][c]
            if k >= 0:
                R[c] = Rk[k] @ R[a[k]] if b[k] == c else Rk[k].T @ R[b[k]]
    R_start = R.copy()
    # the directed edges of the kept pairs: camera i, neighbour j, R_{j -> i}
    kk = np.flatnonzero(kept)
    ei, ej = np.concatenate([a[kk], b[kk]]), np.concatenate([b[kk], a[kk]])
    eR = np.concatenate([np.transpose(Rk[kk], (0, 2, 1)), Rk[kk]])
    ew = np.concatenate([wt[kk], wt[kk]])
    if edge_seed is not None:
        perm = np.random.default_rng(edge_seed).permutation(len(ei))
        ei, ej, eR, ew = ei[perm], ej[perm], eR[perm], ew[perm]

    def edges(R):
        ok = fin & (comp[a] >= 0) & (comp[a] == comp[b])
        th = np.full(n, NAN)
        th[ok] = angle_many(Rk[ok] @ R[a[ok]] @ np.transpose(R[b[ok]], (0, 2, 1)))
        val, der = rho(loss, np.where(kept, th, 0.0) ** 2 / c2)
        return th, np.where(kept, der, 0.0), 0.5 * float(np.sum(np.where(kept, wt * c2 * val, 0.0)))

    _, _, cost_before = edges(R)
    delta, done = [], 0
    while done < max_sweeps:
        batch = min(8, max_sweeps - done)
        for _ in range(batch):
            M = eR @ R[ej] @ np.transpose(R[ei], (0, 2, 1))
            v = log_many(M)
            om = ew * rho(loss, (v * v).sum(axis=1) / c2)[1]
            S, sw = np.zeros((ncams, 3)), np.zeros(ncams)
            np.add.at(S, ei, om[:, None] * v)
            np.add.at(sw, ei, om)
            move = ~fx & (sw > 0)
            step = np.zeros((ncams, 3))
            step[move] = damping * (S[move] / sw[move, None])
            R = np.where(move[:, None, None], exp_many(step) @ R, R)
            delta.append(float(np.sqrt((step * step).sum(axis=1)).max()) if ncams else 0.0)
        done += batch
        if xtol > 0 and min(delta[-batch:]) <= xtol:
            break
    # the gauge: the root of a component without a held camera returns to its start
    for g, root in enumerate(f["roots"] - 1):
        mem = comp == g
        if not fx[mem].any():
            R[mem] = R[mem] @ (R[root].T @ R_start[root])
    residual, edge_weight, cost_after = edges(R)
    rv = np.full((ncams, 3), NAN)
    for c in np.flatnonzero(comp >= 0):
        rv[c] = rotation_vector(R[c])
    is_root = np.zeros(ncams, dtype=bool)
    is_root[f["roots"] - 1] = True
    status = np.where(comp < 0, "isolated", np.where(fx, "fixed", np.where(is_root, "root", "ok")))
    out.update(r=rv, R=R, R_start=R_start, status=status, component=comp, kept=kept, residual=residual, edge_weight=edge_weight,
               sweeps=done, delta=np.array(delta), cost_before=cost_before, cost_after=cost_after, forest=f,
               counts={s: int((status == s).sum()) for s in STATES})
    return out


def camera_errors(R, R_true, root):
    """the angle of every camera's rotation against the truth, gauge aligned at camera `root` (0-based)"""
    G = R[root].T @ R_true[root]
    return angle_many((R @ G) @ np.transpose(R_true, (0, 2, 1)))
