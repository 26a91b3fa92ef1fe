"""numpy reference of the per-observation information matrices of the LM solve (ba_lm_set_obs_info): seeded arrays of 2 x 2
information matrices, their factor Lambda = L L' as include/ba_hip.h defines it, the whitened residual r^ = L' r and Jacobian
J^ = L' J of the oracle's r and J, the reweighting of a robust loss on top (on r^' r^ = r' Lambda r), and the dense step.  The
residual is interleaved (x, y per observation) and so are the rows of J, as everywhere."""
import numpy as np
import scipy.sparse as sp

from _lm_ref import jac, residual, rho


def blocks(sig1, sig2, angle):
    """(n, 2, 2): rotations by `angle` of diag(1 / sig1^2, 1 / sig2^2), exactly symmetric"""
    c, s = np.cos(angle), np.sin(angle)
    a, b = 1.0 / np.asarray(sig1) ** 2, 1.0 / np.asarray(sig2) ** 2
    out = np.empty((len(angle), 2, 2))
    out[:, 0, 0] = c * c * a + s * s * b
    out[:, 1, 1] = s * s * a + c * c * b
    out[:, 0, 1] = out[:, 1, 0] = c * s * (a - b)
    return out


def random_info(p, seed, frac_zero=0.05, frac_rank1=0.05):
    """Anisotropic information of every observation of p: random rotations of diag(1 / s1^2, 1 / s2^2), s in [0.5, 4]; about
    frac_zero of them exactly 0 and about frac_rank1 rank one (u u' / s^2), drawn only among the observations a point can
    spare: every point keeps at least two full-rank observations (full_rank_per_point checks it)."""
    rng = np.random.default_rng(seed)
    n = p["nobs"]
    info = blocks(rng.uniform(0.5, 4.0, n), rng.uniform(0.5, 4.0, n), rng.uniform(0.0, np.pi, n))
    pnt = np.asarray(p["pnt_idx1"]) - 1
    spare = np.bincount(pnt, minlength=p["npnts"]) - 2  # observations a point can lose
    kind = rng.random(n)
    for o in rng.permutation(n):
        if kind[o] < frac_zero + frac_rank1 and spare[pnt[o]] > 0:
            spare[pnt[o]] -= 1
            if kind[o] < frac_zero:
                info[o] = 0.0
            else:
                th, s = rng.uniform(0.0, np.pi), rng.uniform(0.5, 4.0)
                u = np.array([np.cos(th), np.sin(th)])
                info[o] = np.outer(u, u) / s ** 2
    return clip_psd(info)


def clip_psd(info):
    """the blocks with xy moved towards 0 by as many ulps as it takes for xy^2 <= xx yy to hold in floating point (a rank-one
    block formed in floating point may miss it by one)"""
    bad = info[:, 0, 1] ** 2 > info[:, 0, 0] * info[:, 1, 1]
    while bad.any():
        info[bad, 0, 1] = info[bad, 1, 0] = np.nextafter(info[bad, 0, 1], 0.0)
        bad = info[:, 0, 1] ** 2 > info[:, 0, 0] * info[:, 1, 1]
    return info


def full_rank_per_point(p, info):
    """the smallest number of full-rank (det > 1e-8 trace^2) observations any point has"""
    det = info[:, 0, 0] * info[:, 1, 1] - info[:, 0, 1] ** 2
    tr = info[:, 0, 0] + info[:, 1, 1]
    full = det > 1e-8 * tr ** 2
    return int(np.bincount(np.asarray(p["pnt_idx1"]) - 1, weights=full.astype(float), minlength=p["npnts"]).min())


def factor(info):
    """(l00, l10, l11) of Lambda = L L', L lower triangular: l00 = sqrt(xx), l10 = xy / l00 (0 when xx = 0),
    l11 = sqrt(max(yy - l10^2, 0))"""
    xx, xy, yy = info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]
    l00 = np.sqrt(xx)
    l10 = np.divide(xy, l00, out=np.zeros_like(xy), where=xx > 0)
    l11 = np.sqrt(np.maximum(yy - l10 * l10, 0.0))
    return l00, l10, l11


def whiten_residual(r, info):
    """r^ = L' r, interleaved: (l00 r_x + l10 r_y, l11 r_y)"""
    l00, l10, l11 = factor(info)
    out = np.empty_like(r)
    out[0::2] = l00 * r[0::2] + l10 * r[1::2]
    out[1::2] = l11 * r[1::2]
    return out


def whitener(info):
    """the sparse block-diagonal W with W r = r^ (and W J = J^)"""
    l00, l10, l11 = factor(info)
    n = len(l00)
    even, odd = 2 * np.arange(n), 2 * np.arange(n) + 1
    return sp.csr_matrix((np.concatenate([l00, l10, l11]), (np.concatenate([even, even, odd]), np.concatenate([even, odd, odd]))),
                         shape=(2 * n, 2 * n))


def weights_cost(r, info, loss, c):
    """(w, f) of a residual r (not whitened): w_i = rho'(r_i' Lambda_i r_i / c^2), f = 1/2 sum c^2 rho(.)"""
    rh = whiten_residual(r, info)
    s = rh[0::2] ** 2 + rh[1::2] ** 2
    if loss == "linear":
        return np.ones_like(s), 0.5 * np.sum(s)
    val, w = rho(loss, s / c ** 2)
    return w, 0.5 * np.sum(c ** 2 * val)


def reweighted(orc, p, x, info, loss="linear", c=1.0):
    """(r~, J~, w, f): the oracle's r and J at x, whitened, then reweighted under the loss"""
    r = residual(orc, p, x)
    W = whitener(info)
    w, f = weights_cost(r, info, loss, c)
    sw = np.repeat(np.sqrt(w), 2)
    return sw * (W @ r), sp.diags(sw) @ (W @ jac(orc, p, x)), w, f
