"""numpy reference of shared camera intrinsics (ba_lm_set_shared_intrinsics): calibration groups tie (k1, k2, f) of
their members, x = E z.  E as a scipy sparse matrix, the dense step of (E'HE + lam I) dz = -E'g with H and g formed as
prior_ref.step forms them (reweighted J and r, columns of fixed entries zeroed, prior terms added), the same reduced camera
system solved as the bordered system the device solves, and a dense LM loop over z with the controllers of src/lm.jl and
src/LevenbergMarquardt.jl.  x = [points; cameras], camera block (r, t, k1, k2, f), cameras 1-based in the groups."""
import numpy as np
import scipy.sparse as sp

import prior_ref as pr


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


def normal_equations(Jt, rt, prior_rows, fixed=None):
    """(H, g, Jt): the Gauss-Newton matrix without damping and the gradient over x, as prior_ref.step forms them"""
    nvar = Jt.shape[1]
    if fixed is not None:
        Jt = Jt @ sp.diags((~fixed).astype(float))
    Ap, gp = pr.normal_terms(prior_rows, nvar)
    return (Jt.T @ Jt).toarray() + Ap, Jt.T @ rt + gp, Jt


def reduced(A, g, npnts):
    """(S, rhs) of the point-eliminated system of A d = -g (points first)"""
    np3 = 3 * npnts
    U, W, V = A[:np3, :np3], A[:np3, np3:], A[np3:, np3:]
    UiW, Uig = np.linalg.solve(U, W), np.linalg.solve(U, g[:np3])
    return V - W.T @ UiW, -(g[np3:] - W.T @ Uig)


def kappa_jacobi(S):
    s = 1.0 / np.sqrt(np.diag(S))
    e = np.linalg.eigvalsh(S * s[:, None] * s[None, :])
    return float(e[-1] / e[0])


def step(Jt, rt, lam, prior_rows, groups, ncams, npnts, fixed=None):
    """The dense solve over z.  -> dict: delta = E dz (x layout), model = 1/2 |Jt delta + rt|^2 + the priors' model term,
    grad = E'g in the x layout (a group's sum at its first member, zeros at the others), kappa of the Jacobi-scaled reduced
    camera system over z, and what bordered() needs (H, g, E, keep)"""
    H, g, Jt = normal_equations(Jt, rt, prior_rows, fixed)
    E, keep = expansion(groups, ncams, npnts)
    Az = E.T @ (E.T @ H).T
    Az = 0.5 * (Az + Az.T)
    gz = E.T @ g
    Az[np.diag_indices_from(Az)] += lam
    dz = np.linalg.solve(Az, -gz)
    d = E @ dz
    m = Jt @ d + rt
    grad = np.zeros(len(g))
    grad[keep] = gz
    Sz, _ = reduced(Az, gz, npnts)
    return dict(delta=d, model=0.5 * (m @ m) + pr.model(prior_rows, d), grad=grad, kappa=kappa_jacobi(Sz), H=H, g=g, E=E, keep=keep,
                dz=dz)


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


def lm_dense_z(fun, x0, groups, ncams, npnts, variant=1, ite_max=None):
    """The dense LM loop over z.  It restates the controller of prior_ref.lm_dense instead of calling it, for two reasons:
    lm_dense takes |delta| and |x| of its small-step test on the vector it iterates on, here z, while the solve takes them on
    E dz and E z (no rescaling of z gives both those norms and the damping lambda I over z); and lm_dense has the controller of
    src/lm.jl only, while the solves under test run both variants.  The variant 1 branch below is lm_dense's loop line by line
    with those two norms replaced -- a change to prior_ref.lm_dense must be made here too.
    Variant 1: the controller of src/lm.jl without line search; variant 0: that of src/LevenbergMarquardt.jl; oatol = ortol = 0: fun(x) -> (f, gradient, Gauss-Newton matrix, model(delta) -> value), all over
    x; the loop reduces them with E.  |delta| and |x| of the small-step test are norms of E dz and E z, the first-order test
    reads |E'g|.  restol is never met on these scenes (noisy observations).  -> (x, status, iterations, f, |E'g|)"""
    eps = np.finfo(float).eps
    E, keep = expansion(groups, ncams, npnts)
    V = variant
    atol, rtol = (np.sqrt(eps), eps ** (1 / 3)) if V else (100 * np.sqrt(eps), 1000 * np.sqrt(eps))
    satol = srtol = np.sqrt(eps)
    ite_max = (200 if V else 100) if ite_max is None else ite_max

    def at(z):
        f, g, A, mod = fun(E @ z)
        Az = E.T @ (E.T @ A).T
        return f, E.T @ g, 0.5 * (Az + Az.T), mod

    z = np.array(x0, dtype=float)[keep]
    f, g, A, mod = at(z)
    lam = max(30.0, 1e10 / np.linalg.norm(g)) if V else 0.1
    eps_first = atol + rtol * np.linalg.norm(g)
    it = 0
    status = "max_iter"
    if np.linalg.norm(g) < eps_first:
        return E @ z, "first_order", 0, f, float(np.linalg.norm(g))
    while it <= ite_max:
        it += 1
        dz = np.linalg.solve(A + lam * np.eye(len(z)), -g)
        d = E @ dz
        f_new = fun(E @ (z + dz))[0]
        pred, ared = f - mod(d), f - f_new
        if (ared >= 1e-4 * pred) if V else (ared > 1e-4 * pred):  # lm.jl:259 / LevenbergMarquardt.jl:243
            if V:
                lam = lam / 3.0
                if ared >= 0.9 * pred:
                    lam = lam / 3.0
                lam = max(1e-8, lam)
            else:
                lam = lam / 3.0
            z = z + dz
            f, g, A, mod = at(z)
            if np.linalg.norm(d) < satol + srtol * np.linalg.norm(E @ z):
                status = "small_step"
                break
            if np.linalg.norm(g) < eps_first:
                status = "first_order"
                break
        else:
            lam = (max(lam, 1.0 / np.linalg.norm(d)) * 3.0) if V else lam * 3.0
    return E @ z, status, it, f, float(np.linalg.norm(g))
