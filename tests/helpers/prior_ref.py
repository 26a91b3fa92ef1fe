"""numpy reference of the Gaussian priors of the LM solve (ba_lm_set_priors): the camera centre and its Jacobian, the prior
terms of the objective, gradient and Gauss-Newton matrix, the dense step of the augmented normal equations and a dense LM loop
with the controller of src/lm.jl.  x = [points; cameras], camera block (r, t, k1, k2, f), indices 1-based, as everywhere."""
import numpy as np

KINDS = ("point", "camera", "centre")


def rotation(r):
    """Rodrigues rotation of the rotation vector r, evaluated as the model does (theta = |r|, axis r / theta, no small-angle
    branch); works for complex r (complex-step differentiation)"""
    th = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    k = r / th
    K = np.array([[0 * th, -k[2], k[1]], [k[2], 0 * th, -k[0]], [-k[1], k[0], 0 * th]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * np.outer(k, k)


def centre(cam):
    """camera centre c = -R(r)' t of a camera block: the point with P1(r, t, c) = R c + t = 0"""
    return -rotation(cam[:3]).T @ cam[3:6]


def centre_jac(cam):
    """dc/d(r, t), 3 x 6, by complex-step differentiation of centre() (exact to rounding: no difference is formed)"""
    H = np.empty((3, 6))
    for j in range(6):
        z = np.array(cam[:6], dtype=complex)
        z[j] += 1e-30j
        H[:, j] = centre(z).imag / 1e-30
    return H


def centre_jac_fd(cam, h=1e-6):
    """the same by central differences (the cross-check of centre_jac)"""
    H = np.empty((3, 6))
    for j in range(6):
        a, b = np.array(cam[:6], dtype=float), np.array(cam[:6], dtype=float)
        a[j] += h
        b[j] -= h
        H[:, j] = (centre(a) - centre(b)) / (2 * h)
    return H


def _lists(v):
    if v is None:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 0)), np.zeros((0, 0, 0))
    idx, mu, info = v
    idx, mu, info = np.asarray(idx, dtype=np.int64), np.asarray(mu, dtype=float), np.asarray(info, dtype=float)
    if info.ndim == 2:  # standard deviations
        info = np.stack([np.diag(1.0 / s ** 2) for s in info])
    return idx, mu, info


def rows(x, ncams, npnts, point_priors=None, camera_priors=None, centre_priors=None, fixed=None):
    """[(kind, cols, H, d, Lambda)] of every prior at x: cols the entries of x the prior acts on, H = dh/dx[cols] with the
    columns of fixed entries zeroed, d = h(x) - mu"""
    out = []
    np3 = 3 * npnts
    for kind, v in zip(KINDS, (point_priors, camera_priors, centre_priors)):
        idx, mu, info = _lists(v)
        for q, i in enumerate(idx):
            if kind == "point":
                cols = np.arange(3 * (i - 1), 3 * i)
                H, d = np.eye(3), x[cols] - mu[q]
            elif kind == "camera":
                cols = np.arange(np3 + 9 * (i - 1), np3 + 9 * i)
                H, d = np.eye(9), x[cols] - mu[q]
            else:
                cols = np.arange(np3 + 9 * (i - 1), np3 + 9 * (i - 1) + 6)
                cam = x[np3 + 9 * (i - 1):np3 + 9 * i]
                H, d = centre_jac(cam), centre(cam) - mu[q]
            if fixed is not None:
                H = H * (~fixed[cols]).astype(float)[None, :]
            out.append((kind, cols, H, d, info[q]))
    return out


def chi2(prior_rows):
    """d' Lambda d per kind, in the order given"""
    return {k: np.array([d @ L @ d for kind, _, _, d, L in prior_rows if kind == k]) for k in KINDS}


def cost(prior_rows):
    return 0.5 * sum(d @ L @ d for _, _, _, d, L in prior_rows)


def normal_terms(prior_rows, nvar):
    """(sum H' Lambda H dense nvar x nvar, sum H' Lambda d)"""
    A, g = np.zeros((nvar, nvar)), np.zeros(nvar)
    for _, cols, H, d, L in prior_rows:
        A[np.ix_(cols, cols)] += H.T @ L @ H
        g[cols] += H.T @ (L @ d)
    return A, g


def model(prior_rows, delta):
    """1/2 sum (H delta + d)' Lambda (H delta + d)"""
    return 0.5 * sum((H @ delta[cols] + d) @ L @ (H @ delta[cols] + d) for _, cols, H, d, L in prior_rows)


def step(Jt, rt, lam, prior_rows, fixed=None):
    """(delta, model value, gradient, A) of (Jt'Jt + sum H'Lambda H + lam I) delta = -(Jt'rt + sum H'Lambda d): Jt, rt the
    (reweighted) Jacobian (scipy sparse) and residual; columns of fixed entries zeroed"""
    import scipy.sparse as sp
    nvar = Jt.shape[1]
    if fixed is not None:
        Jt = Jt @ sp.diags((~fixed).astype(float))
    Ap, gp = normal_terms(prior_rows, nvar)
    A = (Jt.T @ Jt).toarray() + Ap
    A[np.diag_indices_from(A)] += lam
    g = Jt.T @ rt + gp
    d = np.linalg.solve(A, -g)
    m = Jt @ d + rt
    return d, 0.5 * (m @ m) + model(prior_rows, d), g, A


def kappa_jacobi_S(A, npnts):
    """condition number of the Jacobi-scaled reduced camera system of A = [[U W], [W' V]] (points first)"""
    np3 = 3 * npnts
    S = A[np3:, np3:] - A[np3:, :np3] @ np.linalg.solve(A[:np3, :np3], A[:np3, np3:])
    s = 1.0 / np.sqrt(np.diag(S))
    e = np.linalg.eigvalsh(S * s[:, None] * s[None, :])
    return float(e[-1] / e[0]), S


def lm_dense(fun, x0, lam=30.0, ite_max=200, atol=None, rtol=None, satol=None, srtol=None):
    """Dense LM with the controller of src/lm.jl (variant 1, no line search, oatol = ortol = 0, restol = 0): fun(x) ->
    (f, gradient, Gauss-Newton matrix, model(delta) -> value).  Returns (x, status, iterations)."""
    eps = np.finfo(float).eps
    atol = np.sqrt(eps) if atol is None else atol
    rtol = eps ** (1 / 3) if rtol is None else rtol
    satol = np.sqrt(eps) if satol is None else satol
    srtol = np.sqrt(eps) if srtol is None else srtol
    x = np.array(x0, dtype=float)
    f, g, A, mod = fun(x)
    lam = max(lam, 1e10 / np.linalg.norm(g))
    eps_first = atol + rtol * np.linalg.norm(g)
    for it in range(1, ite_max + 2):
        d = np.linalg.solve(A + lam * np.eye(len(x)), -g)
        f_new = fun(x + d)[0]
        pred, ared = f - mod(d), f - f_new
        if ared >= 1e-4 * pred:
            lam = lam / 3.0
            if ared >= 0.9 * pred:
                lam = lam / 3.0
            lam = max(1e-8, lam)
            x = x + d
            f, g, A, mod = fun(x)
            if np.linalg.norm(d) < satol + srtol * np.linalg.norm(x):
                return x, "small_step", it
            if np.linalg.norm(g) < eps_first:
                return x, "first_order", it
        else:
            lam = max(lam, 1.0 / np.linalg.norm(d)) * 3.0
    return x, "max_iter", ite_max
