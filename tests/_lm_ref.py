"""The numpy reference of the LM term tests, and nothing else (the run plumbing is tests/_lm_run.py): the oracle's residual and
Jacobian, whitened by the observations' information and reweighted under a robust loss; the rows of the Gaussian priors; the
expansion E of calibration groups (x = E z); the normal equations formed once; ONE step that takes every term as an argument --
absent terms are skipped, so an argument's neutral element gives the bits of the argument left out; ONE dense LM loop with the
controllers of src/lm.jl and src/LevenbergMarquardt.jl; the covariance references; the tolerances and their rule.
x = [points; cameras], camera block (r, t, k1, k2, f), indices 1-based, residual and rows of J interleaved (x, y per observation)."""
import numpy as np
import scipy.sparse as sp

from _util import parity_record

EPS = np.finfo(np.float64).eps
C_BOUND = 100.0
STEP_TOL = {1e3: 1e-12, 30.0: 1e-11, 1.0: 1e-11, 1e-2: 1e-9}  # test_lm_step_vs_oracle's limits at these lambda
F32_TOL = 5e-3  # the Float32-factor limit of tests/test_fixed_params.py and tests/test_robust_loss.py
PCG_TOL = 1e-8  # their limit of the pcg=(1e-12, 5000) step
KINDS = ("point", "camera", "centre")


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def limit(tol, kappa):
    """the project's limit of a step at this lambda, or 100 kappa eps where the conditioning of the damped reduced camera
    system (priors included) is worse: the rule of check_cov"""
    return max(tol, C_BOUND * kappa * EPS)


# ---- the two definitions: scipy's loss table, the header's factor of an information matrix ------------------------------------
def rho(loss, z):
    """(rho(z), rho'(z)) of scipy's losses"""
    if loss == "linear":
        return z, np.ones_like(z)
    if loss == "huber":
        sz = np.sqrt(np.maximum(z, 1.0))
        return np.where(z <= 1.0, z, 2.0 * sz - 1.0), np.where(z <= 1.0, 1.0, 1.0 / sz)
    if loss == "soft_l1":
        t = np.sqrt(1.0 + z)
        return 2.0 * z / (t + 1.0), 1.0 / t
    if loss == "cauchy":
        return np.log1p(z), 1.0 / (1.0 + z)
    if loss == "arctan":
        return np.arctan(z), 1.0 / (1.0 + z * z)
    raise ValueError(loss)


def factor(info):
    """(l00, l10, l11) of Lambda = L L', L lower triangular, from (n, 2, 2) blocks, as include/ba_hip.h defines it:
    l00 = sqrt(xx), l10 = xy / l00 (0 when xx = 0), l11 = sqrt(max(yy - l10^2, 0))"""
    xx, xy, yy = info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]
    l00 = np.sqrt(xx)
    l10 = np.divide(xy, l00, out=np.zeros_like(xy), where=xx > 0)
    l11 = np.sqrt(np.maximum(yy - l10 * l10, 0.0))
    return l00, l10, l11


# ---- residual, Jacobian, whitening, reweighting ---------------------------------------------------------------------------------
def residual(orc, p, x):
    return orc.residuals(p["cam_idx1"], p["pnt_idx1"], x, p["pt2d"], p["npnts"])


def jac(orc, p, x):
    rows, cols = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    vals = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], x, p["npnts"])
    nvar = 9 * p["ncams"] + 3 * p["npnts"]
    return sp.csr_matrix((vals, (rows - 1, cols - 1)), shape=(2 * p["nobs"], nvar))


def whiten_residual(r, info):
    """r^ = L' r: (l00 r_x + l10 r_y, l11 r_y)"""
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


def weights_cost(r, loss="linear", c=1.0, info=None):
    """(w, f) of a residual r (not whitened): w_i = rho'(r_i' Lambda_i r_i / c^2), f = 1/2 sum c^2 rho(.); Lambda = I without
    info"""
    if info is not None:
        r = whiten_residual(r, info)
    s = r[0::2] ** 2 + r[1::2] ** 2
    if loss == "linear":
        return np.ones_like(s), 0.5 * np.sum(s)
    val, w = rho(loss, s / c ** 2)
    return w, 0.5 * np.sum(c ** 2 * val)


def linearise(orc, p, x, info=None, loss="linear", c=1.0):
    """(r~, J~, w, f): the oracle's r and J at x, whitened where info is given (r^ = L' r, J^ = L' J), then reweighted under the
    loss: r~ = sqrt(w) r^, J~ = sqrt(w) J^, w = rho'(|r^_i|^2 / c^2) per observation.  An absent term is no operation."""
    r, J = residual(orc, p, x), jac(orc, p, x)
    if info is not None:
        W = whitener(info)
        r, J = W @ r, W @ J
    w, f = weights_cost(r, loss, c)
    if loss != "linear":
        sw = np.repeat(np.sqrt(w), 2)
        r, J = sw * r, sp.diags(sw) @ J
    J.sort_indices()  # (scipy's product leaves a row's entries in another order than jac(): J~ delta sums in the order of the row)
    return r, J, w, f


# ---- Gaussian priors (ba_lm_set_priors): the camera centre, the prior rows and their terms -------------------------------------
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


def rows(x, ncams, npnts, point_priors=None, camera_priors=None, centre_priors=None):
    """[(kind, cols, H, d, Lambda)] of every prior at x: cols the entries of x the prior acts on, H = dh/dx[cols],
    d = h(x) - mu"""
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


# ---- shared intrinsics (ba_lm_set_shared_intrinsics): x = E z -------------------------------------------------------
def labels(groups, ncams):
    """int labels (ncams,) of a list of lists of 1-based camera indices (or of an array of labels); groups of one camera -> 0"""
    if len(groups) and np.ndim(groups[0]) == 0:
        lab = np.array(groups, dtype=int)
    else:
        lab = np.zeros(ncams, dtype=int)
        for g, mem in enumerate(groups, 1):
            lab[np.asarray(mem) - 1] = g
    for g in range(1, lab.max() + 1 if lab.size else 1):
        if np.count_nonzero(lab == g) < 2:
            lab[lab == g] = 0
    return lab


def expansion(groups, ncams, npnts):
    """(E, keep): E (nvar x nz, scipy csr) copies a group's (k1, k2, f) -- held at its first member, the lowest camera index --
    to every member; keep: the entries of x that are entries of z, ascending (z = x[keep])"""
    lab = labels(groups, ncams)
    nvar, np3 = 3 * npnts + 9 * ncams, 3 * npnts
    owner = np.arange(nvar)
    for g in np.unique(lab[lab > 0]):
        mem = np.flatnonzero(lab == g)
        for c in mem[1:]:
            owner[np3 + 9 * c + 6:np3 + 9 * c + 9] = np3 + 9 * mem[0] + 6 + np.arange(3)
    keep = np.flatnonzero(owner == np.arange(nvar))
    col_of = -np.ones(nvar, dtype=int)
    col_of[keep] = np.arange(keep.size)
    E = sp.csr_matrix((np.ones(nvar), (np.arange(nvar), col_of[owner])), shape=(nvar, keep.size))
    return E, keep


def _tied(groups, ncams, npnts):
    """expansion(), or (None, None) where nothing is tied (no groups, or groups of one camera only)"""
    if groups is None or not labels(groups, ncams).any():
        return None, None
    return expansion(groups, ncams, npnts)


def reduced(A, g, npnts):
    """(S, rhs) of the point-eliminated system of A d = -g (points first)"""
    np3 = 3 * npnts
    U, W, V = A[:np3, :np3], A[:np3, np3:], A[np3:, np3:]
    UiW, Uig = np.linalg.solve(U, W), np.linalg.solve(U, g[:np3])
    return V - W.T @ UiW, -(g[np3:] - W.T @ Uig)


def bordered(H, g, lam, groups, ncams, npnts):
    """The camera part of the step by the bordered solve of DESIGN §5g, from the reduced camera system of the UNtied problem:
    S_full = the point-eliminated H + lam I over all 9 ncams rows, M = the intrinsic rows of all members, E_g the 9 ncams x 3G
    indicator of (group, component):  B = S_full E_g with its rows in M zeroed, C = E_g'(S_full - lam I)E_g + lam I, A = S_full
    with rows and columns M replaced by the identity; A [Y | a0] = [B | rhs_a], T = C - B'Y, y = T^-1 (rhs_y - B'a0), a = a0 -
    Y y, step = a + E_g y."""
    lab = labels(groups, ncams)
    n = 9 * ncams
    A_full = H + lam * np.eye(H.shape[0])
    S, rhs = reduced(A_full, g, npnts)
    G = int(lab.max())
    Eg = np.zeros((n, 3 * G))
    for c in np.flatnonzero(lab > 0):
        for q in range(3):
            Eg[9 * c + 6 + q, 3 * (lab[c] - 1) + q] = 1.0
    M = np.flatnonzero(Eg.sum(axis=1) > 0)
    SB = S @ Eg
    B = SB.copy()
    B[M] = 0.0
    C = Eg.T @ (S - lam * np.eye(n)) @ Eg + lam * np.eye(3 * G)
    rhs_y = Eg.T @ rhs
    A = S.copy()
    A[M, :] = 0.0
    A[:, M] = 0.0
    A[M, M] = 1.0
    rhs_a = rhs.copy()
    rhs_a[M] = 0.0
    sol = np.linalg.solve(A, np.column_stack([B, rhs_a]))
    Y, a0 = sol[:, :-1], sol[:, -1]
    T = C - B.T @ Y
    y = np.linalg.solve(T, rhs_y - B.T @ a0)
    return a0 - Y @ y + Eg @ y


# ---- the normal equations and the step ------------------------------------------------------------------------------------------
def normal_equations(orc, p, x, *, info=None, loss="linear", c=1.0, priors=None, dense=True):
    """(H, g, J~, r~, prior rows) over x: H = J~'J~ + sum H_k' Lambda_k H_k without damping (a dense array, or scipy csr where
    dense is False: the prior terms are dense, so that form takes no priors), g = J~'r~ + sum H_k' Lambda_k d_k"""
    rt, Jt, _, _ = linearise(orc, p, x, info, loss, c)
    prior_rows = rows(x, p["ncams"], p["npnts"], **priors) if priors else []
    H, g = Jt.T @ Jt, Jt.T @ rt
    if dense:
        H = H.toarray()
    if prior_rows:
        assert dense, "prior rows are formed densely"
        Hp, gp = normal_terms(prior_rows, len(x))
        H, g = H + Hp, g + gp
    return H, g, Jt, rt, prior_rows


def step(orc, p, x, lam, *, info=None, loss="linear", c=1.0, fixed=None, priors=None, groups=None, solve="dense", zeroed=False):
    """One LM step with every term as an argument: (E_F'(H + ...)E_F + lam I) dz_F = -E_F'g over the free entries of z (x = E z;
    z = x without groups), zeros scattered to the fixed ones.  fixed: boolean over x (the members of a group agree).  zeroed:
    the other form of the same step -- the fixed rows and columns zeroed, lam on their diagonal, the full system solved -- for
    the one test whose reference would move by more than a tenth of its limit between the forms.
    solve = "dense": the dense solve of that system; "schur": the point blocks eliminated through schur(), H kept sparse (the
    scenes too large for a dense H; it takes info and loss only).  The two differ by about kappa eps.
    -> dict: delta (x layout), model = 1/2 |J~ delta + r~|^2 + the priors' model term, grad = E'g in the x layout (a group's sum
    at its first member, zeros at the others and at fixed entries), kappa of the Jacobi-scaled damped reduced camera system the
    solve runs on; with groups also H, g (over x, no mask), E, keep and dz."""
    npnts, ncams = p["npnts"], p["ncams"]
    H, g, Jt, rt, prior_rows = normal_equations(orc, p, x, info=info, loss=loss, c=c, priors=priors, dense=solve == "dense")
    E, keep = _tied(groups, ncams, npnts)
    A, b, fz = H, g, fixed
    assert solve == "dense" or (fixed is None and E is None)
    if E is not None:
        A = E.T @ (E.T @ H).T
        A, b, fz = 0.5 * (A + A.T), E.T @ g, None if fixed is None else fixed[keep]
    np3, free, bs = 3 * npnts, None, b
    if fz is not None and zeroed:
        A, bs = A * np.outer(~fz, ~fz), np.where(fz, 0.0, b)
    elif fz is not None:  # the solve runs over the free columns only (points are fixed as a whole: the point blocks stay 3 x 3)
        free = np.flatnonzero(~fz)
        A, bs, np3 = A[np.ix_(free, free)], b[free], int(np.count_nonzero(~fz[:np3]))
    if solve == "dense":
        A = A.copy()
        A[np.diag_indices_from(A)] += lam
        ds = np.linalg.solve(A, -bs)
        kappa = kappa_jacobi(reduced(A, bs, np3 // 3)[0])
    else:
        S, G, Ubi = schur((A + sp.diags(np.full(len(bs), float(lam)))).tocsr(), p)
        u = np.einsum("pij,pj->pi", Ubi, bs[:np3].reshape(-1, 3)).ravel()
        dc = np.linalg.solve(S, -(bs[np3:] - G.T @ bs[:np3]))
        ds, kappa = np.concatenate([-u - G @ dc, dc]), kappa_jacobi(S)
    dz, gz = ds, bs
    if free is not None:
        dz, gz = np.zeros(len(b)), np.zeros(len(b))
        dz[free], gz[free] = ds, bs
    delta, grad = dz, gz
    if E is not None:
        delta, grad = E @ dz, np.zeros(len(g))
        grad[keep] = gz
    m = Jt @ delta + rt
    out = dict(delta=delta, model=0.5 * float(m @ m) + model(prior_rows, delta), grad=grad, kappa=kappa)
    if E is not None:
        out.update(H=H, g=g, E=E, keep=keep, dz=dz)
    return out


_steps = {}


def step_once(key, *args, **kw):
    """step(*args, **kw) computed once per key (a scene's name, lambda, ...), its arrays read-only: the tests of one file share
    the steps of a scene"""
    if key not in _steps:
        _steps[key] = step(*args, **kw)
        for v in _steps[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _steps[key]


# ---- ONE dense LM loop -------------------------------------------------------------------------------------------------------
def lm_dense(fun, x0, *, groups=None, ncams=None, npnts=None, variant=1, lam=None, ite_max=None, atol=None, rtol=None, satol=None,
             srtol=None):
    """Dense LM over z (x = E z; z = x without groups).  variant 1: the controller of src/lm.jl without line search; variant 0:
    that of src/LevenbergMarquardt.jl; oatol = ortol = 0, and restol is never met on the scenes of the tests (noisy
    observations).  fun(x) -> (f, gradient, Gauss-Newton matrix, model(delta) -> value), all over x; the loop reduces them with
    E and damps with lam I over z.  |delta| and |x| of the small-step test are norms of E dz and E z, the first-order test reads
    |E'g|.  -> (x, status, iterations, f, |E'g|)"""
    V = variant
    E, keep = _tied(groups, ncams, npnts)
    if atol is None:
        atol = np.sqrt(EPS) if V else 100 * np.sqrt(EPS)
    if rtol is None:
        rtol = EPS ** (1 / 3) if V else 1000 * np.sqrt(EPS)
    satol = np.sqrt(EPS) if satol is None else satol
    srtol = np.sqrt(EPS) if srtol is None else srtol
    ite_max = (200 if V else 100) if ite_max is None else ite_max

    def expand(z):
        return z if E is None else E @ z

    def at(z):
        f, g, A, mod = fun(expand(z))
        if E is None:
            return f, g, A, mod
        Az = E.T @ (E.T @ A).T
        return f, E.T @ g, 0.5 * (Az + Az.T), mod

    z = np.array(x0, dtype=float)
    if E is not None:
        z = z[keep]
    f, g, A, mod = at(z)
    if lam is None:
        lam = 30.0 if V else 0.1
    if V:
        lam = max(lam, 1e10 / np.linalg.norm(g))
    eps_first = atol + rtol * np.linalg.norm(g)
    it, status = 0, "max_iter"
    if np.linalg.norm(g) < eps_first:
        return expand(z), "first_order", 0, f, float(np.linalg.norm(g))
    while it <= ite_max:
        it += 1
        dz = np.linalg.solve(A + lam * np.eye(len(z)), -g)
        d = expand(dz)
        f_new = fun(expand(z + dz))[0]
        pred, ared = f - mod(d), f - f_new
        if (ared >= 1e-4 * pred) if V else (ared > 1e-4 * pred):  # lm.jl:259 / LevenbergMarquardt.jl:243
            lam = lam / 3.0
            if V:
                if ared >= 0.9 * pred:
                    lam = lam / 3.0
                lam = max(1e-8, lam)
            z = z + dz
            f, g, A, mod = at(z)
            if np.linalg.norm(d) < satol + srtol * np.linalg.norm(expand(z)):
                status = "small_step"
                break
            if np.linalg.norm(g) < eps_first:
                status = "first_order"
                break
        else:
            lam = (max(lam, 1.0 / np.linalg.norm(d)) * 3.0) if V else lam * 3.0
    return expand(z), status, it, f, float(np.linalg.norm(g))


# ---- covariance references -----------------------------------------------------------------------------------------------------
def hessian(orc, p, x, lam, fixed, loss=None, c=1.0, info=None):
    """J~_F'J~_F + diag(lam on the free entries, 1 on the fixed ones) (sparse; the fixed rows / columns hold only the 1)"""
    J = linearise(orc, p, x, info, loss or "linear", c)[1] @ sp.diags((~fixed).astype(float))
    return (J.T @ J + sp.diags(np.where(fixed, 1.0, lam))).tocsr()


def ref_dense(H, p, fixed):
    """camera and point blocks of the inverse of the full dense H, fixed rows / columns zeroed"""
    Hi = np.linalg.inv(H.toarray())
    Hi[fixed, :] = 0.0
    Hi[:, fixed] = 0.0
    np3 = 3 * p["npnts"]
    pts = np.stack([Hi[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(p["npnts"])])
    cams = np.stack([Hi[np3 + 9 * c:np3 + 9 * c + 9, np3 + 9 * c:np3 + 9 * c + 9] for c in range(p["ncams"])])
    return cams, pts


def schur(H, p):
    """(S dense, U^-1 W sparse, the blocks of U^-1) of H = [[U W], [W' V]] (points first)"""
    np3 = 3 * p["npnts"]
    U = H[:np3, :np3].tocoo()
    Ub = np.zeros((p["npnts"], 3, 3))
    np.add.at(Ub, (U.row // 3, U.row % 3, U.col % 3), np.where(U.row // 3 == U.col // 3, U.data, 0.0))
    Ubi = np.linalg.inv(Ub)
    W = H[:np3, np3:]
    G = (sp.block_diag(list(Ubi), format="csr") @ W).tocsr()
    S = H[np3:, np3:].toarray() - (W.T @ G).toarray()
    return S, G, Ubi


def ref_schur(H, p, fixed):
    """camera and point blocks from the explicit Schur complement: Z = S^-1, Sigma_pp = U^-1 + (U^-1 W) Z (U^-1 W)'"""
    S, G, Ubi = schur(H, p)
    Z = np.linalg.inv(S)
    cams = np.stack([Z[9 * c:9 * c + 9, 9 * c:9 * c + 9] for c in range(p["ncams"])])
    npnts = p["npnts"]
    pts = np.empty((npnts, 3, 3))
    for a in range(0, npnts, 500):
        b = min(npnts, a + 500)
        Gc = G[3 * a:3 * b]
        P = np.asarray(Gc @ Z).reshape(b - a, 3, -1)
        Q = Gc.toarray().reshape(b - a, 3, -1)
        pts[a:b] = Ubi[a:b] + np.einsum("irk,imk->irm", P, Q)
    fp = fixed[:3 * npnts].reshape(npnts, 3)
    fc = fixed[3 * npnts:].reshape(p["ncams"], 9)
    cams[fc[:, :, None] | fc[:, None, :]] = 0.0
    pts[fp[:, :, None] | fp[:, None, :]] = 0.0
    return cams, pts, S, Z


def _lmax(A, its=200):
    """largest eigenvalue of a symmetric positive semi-definite A (power iteration; eigvalsh for small A)"""
    if A.shape[0] <= 3000:
        return float(np.linalg.eigvalsh(A)[-1])
    v = np.random.default_rng(0).standard_normal(A.shape[0])
    lam = 0.0
    for _ in range(its):
        w = A @ v
        lam = float(np.linalg.norm(w))
        v = w / lam
    return lam


def kappa_jacobi(S, Z=None):
    """condition number of the Jacobi-scaled S"""
    d = 1.0 / np.sqrt(np.diag(S))
    Ss = S * d[:, None] * d[None, :]
    Zs = (np.linalg.inv(S) if Z is None else Z) / (d[:, None] * d[None, :])
    return _lmax(Ss) * _lmax(Zs)


def block_errs(got, ref):
    """largest relative Frobenius error over the blocks that are not all zero"""
    num = np.linalg.norm((got - ref).reshape(len(ref), -1), axis=1)
    den = np.linalg.norm(ref.reshape(len(ref), -1), axis=1)
    m = den > 0
    return float(np.max(num[m] / den[m])) if m.any() else 0.0


def check_cov(test, cams, pts, ref_c, ref_p, kappa, fixed, p, **extra):
    ec, ep = block_errs(cams, ref_c), block_errs(pts, ref_p)
    bound = C_BOUND * kappa * EPS
    parity_record(test, cam_block_rel_err=ec, pnt_block_rel_err=ep, kappa_jacobi_scaled_S=kappa, bound=bound,
                  c_cam=ec / (kappa * EPS), c_pnt=ep / (kappa * EPS), **extra)
    npnts = p["npnts"]
    fp = fixed[:3 * npnts].reshape(npnts, 3)
    fc = fixed[3 * npnts:].reshape(p["ncams"], 9)
    assert np.all(cams[fc[:, :, None] | fc[:, None, :]] == 0.0), "a fixed camera component's row / column is not exactly 0"
    assert np.all(pts[fp[:, :, None] | fp[:, None, :]] == 0.0), "a fixed point's block is not exactly 0"
    assert np.all(np.isfinite(cams)) and np.all(np.isfinite(pts))
    assert ec <= bound, f"{test}: camera blocks {ec:.3e} > {C_BOUND:g} kappa eps = {bound:.3e} (kappa {kappa:.3e})"
    assert ep <= bound, f"{test}: point blocks {ep:.3e} > {C_BOUND:g} kappa eps = {bound:.3e} (kappa {kappa:.3e})"
