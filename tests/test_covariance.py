"""Covariance at a solution (ba_covariance, include/ba_hip.h): the cameras' 9 x 9 and the points' 3 x 3 diagonal
blocks of (J~_F'J~_F + lambda I)^-1 from the selected inversion of the factored reduced camera matrix.  References: numpy --
the inverse of the full dense J_F'J_F (small scene), the inverse of the explicit Schur complement (scenes of many tile rows).
Bound of a block's relative error: c kappa eps with kappa the condition number of the Jacobi-scaled S and c <= 100.  The first
tests need no device (the Python layer refuses bad arguments before any device call); the rest run on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from _util import bits_report, parity_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPBACK = os.path.join(ROOT, "tests", "helpers", "libba_loopback.so")
EPS = np.finfo(np.float64).eps
C_BOUND = 100.0
INTRINSICS = ("k1", "k2", "f")


# ---- numpy reference -------------------------------------------------------------------------------------------------------
def _arrays(p):
    return (p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], p["ncams"], p["npnts"], p["nobs"])


def _fixed_vector(ba, p, kw):
    """boolean over x = [points; cameras]: True where the options of kw fix the entry"""
    cam, pnt = ba._lib.fixed_masks(p["ncams"], p["npnts"], kw.get("fixed_cameras"), kw.get("fixed_points"),
                                   kw.get("fixed_camera_params"))
    return np.concatenate([np.repeat(pnt.astype(bool), 3), ((cam[:, None] >> np.arange(9)) & 1).astype(bool).ravel()])


def _gauge_kw(p):
    """camera 1's pose (r, t) and the first translation component of camera 2: the 7 DoF of a similarity transform"""
    comp = np.zeros((p["ncams"], 9), dtype=bool)
    comp[0, :6] = True
    comp[1, 3] = True
    return dict(fixed_camera_params=comp)


def _huber_w(r, c):
    s = r[0::2] ** 2 + r[1::2] ** 2
    return np.where(s <= c * c, 1.0, c / np.sqrt(np.maximum(s, c * c)))


def _hessian(orc, p, x, lam, fixed, loss=None, c=1.0):
    """J~_F'J~_F + diag(lam on the free entries, 1 on the fixed ones) (sparse; the fixed rows / columns hold only the 1)"""
    r = orc.residuals(p["cam_idx1"], p["pnt_idx1"], x, p["pt2d"], p["npnts"])
    rows, cols = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    vals = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], x, p["npnts"])
    nvar = 9 * p["ncams"] + 3 * p["npnts"]
    J = sp.csr_matrix((vals, (rows - 1, cols - 1)), shape=(2 * p["nobs"], nvar))
    if loss == "huber":
        J = sp.diags(np.repeat(np.sqrt(_huber_w(r, c)), 2)) @ J
    J = J @ sp.diags((~fixed).astype(float))
    return (J.T @ J + sp.diags(np.where(fixed, 1.0, lam))).tocsr()


def _ref_dense(H, p, fixed):
    """camera and point blocks of the inverse of the full dense H, fixed rows / columns zeroed"""
    Hi = np.linalg.inv(H.toarray())
    Hi[fixed, :] = 0.0
    Hi[:, fixed] = 0.0
    np3 = 3 * p["npnts"]
    pts = np.stack([Hi[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(p["npnts"])])
    cams = np.stack([Hi[np3 + 9 * c:np3 + 9 * c + 9, np3 + 9 * c:np3 + 9 * c + 9] for c in range(p["ncams"])])
    return cams, pts


def _schur(H, p):
    """(S dense, U^-1 W sparse) of H = [[U W], [W' V]] (points first)"""
    np3 = 3 * p["npnts"]
    U = H[:np3, :np3].tocoo()
    Ub = np.zeros((p["npnts"], 3, 3))
    np.add.at(Ub, (U.row // 3, U.row % 3, U.col % 3), np.where(U.row // 3 == U.col // 3, U.data, 0.0))
    Ubi = np.linalg.inv(Ub)
    W = H[:np3, np3:]
    G = (sp.block_diag(list(Ubi), format="csr") @ W).tocsr()
    S = H[np3:, np3:].toarray() - (W.T @ G).toarray()
    return S, G, Ubi


def _ref_schur(H, p, fixed):
    """camera and point blocks from the explicit Schur complement: Z = S^-1, Sigma_pp = U^-1 + (U^-1 W) Z (U^-1 W)'"""
    S, G, Ubi = _schur(H, p)
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


def _kappa(S, Z=None):
    """condition number of the Jacobi-scaled S"""
    d = 1.0 / np.sqrt(np.diag(S))
    Ss = S * d[:, None] * d[None, :]
    Zs = (np.linalg.inv(S) if Z is None else Z) / (d[:, None] * d[None, :])
    return _lmax(Ss) * _lmax(Zs)


def _block_errs(got, ref):
    """largest relative Frobenius error over the blocks that are not all zero"""
    num = np.linalg.norm((got - ref).reshape(len(ref), -1), axis=1)
    den = np.linalg.norm(ref.reshape(len(ref), -1), axis=1)
    m = den > 0
    return float(np.max(num[m] / den[m])) if m.any() else 0.0


def _check(test, cams, pts, ref_c, ref_p, kappa, fixed, p, **extra):
    ec, ep = _block_errs(cams, ref_c), _block_errs(pts, ref_p)
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


def _env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# ---- CPU: refusals before any device call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam="x"),
                                dict(rank_tol=-1e-3), dict(rank_tol=float("nan")), dict(loss="l2"), dict(f_scale=0.0),
                                dict(fixed_points=[0]), dict(fixed_camera_params=("q",))])
def test_covariance_refuses_bad_arguments_before_any_device_call(ba, kw):
    with pytest.raises(ValueError):
        ba.covariance(None, np.zeros(3), **kw)


def test_covariance_is_exported(ba):
    assert "covariance" in ba.__all__ and callable(ba.covariance)
    assert "ba_covariance" in ba._lib.SYMBOLS


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_covariance_gauge_fixed_matches_dense_inverse(ba, orc, small_prob, gpu_ok):
    p = small_prob
    kw = _gauge_kw(p)
    fixed = _fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=_arrays(p))
    try:
        cams, pts, piv = ba.covariance(m, p["x0"], 0.0, **kw)
    finally:
        m.close()
    H = _hessian(orc, p, p["x0"], 0.0, fixed)
    ref_c, ref_p = _ref_dense(H, p, fixed)
    S, _, _ = _schur(H, p)
    assert cams.shape == (p["ncams"], 9, 9) and pts.shape == (p["npnts"], 3, 3)
    _check("covariance_gauge_fixed", cams, pts, ref_c, ref_p, _kappa(S), fixed, p, min_rel_pivot=piv)
    assert piv > 1e-10


@pytest.mark.gpu
def test_covariance_damped_gauge_free(ba, orc, small_prob, gpu_ok):
    p = small_prob
    lam = 10.0
    fixed = np.zeros(9 * p["ncams"] + 3 * p["npnts"], dtype=bool)
    m = ba.BALNLPModel(arrays=_arrays(p))
    try:
        cams, pts, piv = ba.covariance(m, p["x0"], lam)
    finally:
        m.close()
    H = _hessian(orc, p, p["x0"], lam, fixed)
    ref_c, ref_p = _ref_dense(H, p, fixed)
    S, _, _ = _schur(H, p)
    _check("covariance_damped", cams, pts, ref_c, ref_p, _kappa(S), fixed, p, lam=lam, min_rel_pivot=piv)


@pytest.mark.gpu
def test_covariance_gauge_free_is_refused(ba, small_prob, gpu_ok):
    """lambda = 0 with the similarity gauge free: S is singular, the rank check refuses (SQDException); min D_i / S_ii sits
    far below its value with the gauge fixed"""
    p = small_prob
    m = ba.BALNLPModel(arrays=_arrays(p))
    try:
        with pytest.raises(ba.SQDException) as ei:
            ba.covariance(m, p["x0"], 0.0)
        free_piv = getattr(ei.value, "min_rel_pivot", None)
        _, _, fixed_piv = ba.covariance(m, p["x0"], 0.0, cameras=False, points=False, **_gauge_kw(p))
    finally:
        m.close()
    parity_record("covariance_gauge_free_refused", min_rel_pivot_free=free_piv if free_piv is not None else float("nan"),
                  min_rel_pivot_gauge_fixed=fixed_piv)
    assert "gauge" in str(ei.value)
    assert fixed_piv > 1e-10
    if free_piv is not None:  # (an exactly zero pivot is refused before the ratio exists)
        assert free_piv <= 1e-10 and free_piv < 1e-4 * fixed_piv, (free_piv, fixed_piv)


@pytest.mark.gpu
def test_covariance_huber(ba, orc, small_prob, gpu_ok):
    p = small_prob
    kw = _gauge_kw(p)
    fixed = _fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=_arrays(p))
    try:
        cams, pts, _ = ba.covariance(m, p["x0"], 0.0, loss="huber", f_scale=1.0, **kw)
    finally:
        m.close()
    H = _hessian(orc, p, p["x0"], 0.0, fixed, loss="huber", c=1.0)
    ref_c, ref_p = _ref_dense(H, p, fixed)
    S, _, _ = _schur(H, p)
    _check("covariance_huber", cams, pts, ref_c, ref_p, _kappa(S), fixed, p)


@pytest.mark.gpu
def test_covariance_intrinsics_and_points_fixed(ba, orc, small_prob, gpu_ok):
    p = small_prob
    rng = np.random.default_rng(3)
    kw = dict(fixed_camera_params=INTRINSICS, fixed_points=np.sort(rng.choice(p["npnts"], p["npnts"] // 5, replace=False)) + 1)
    fixed = _fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=_arrays(p))
    try:
        cams, pts, _ = ba.covariance(m, p["x0"], 0.0, **kw)
    finally:
        m.close()
    H = _hessian(orc, p, p["x0"], 0.0, fixed)
    ref_c, ref_p = _ref_dense(H, p, fixed)
    S, _, _ = _schur(H, p)
    _check("covariance_intrinsics_points_fixed", cams, pts, ref_c, ref_p, _kappa(S), fixed, p)


def _scene(ba, name):
    if name == "band AMD":
        return ba.synthetic.shuffle_cameras(ba.synthetic.make_problem(300, 900, 4500, seed=5, locality=0.08), seed=2)[0], "AMD"
    if name == "band Metis":
        return ba.synthetic.shuffle_cameras(ba.synthetic.make_problem(300, 900, 4500, seed=5, locality=0.08), seed=2)[0], "Metis"
    if name == "plane":
        return ba.synthetic.make_problem(300, 900, 4500, seed=14, plane_radius=0.15), "AMD"
    return ba.synthetic.make_problem(1100, 6000, 30000, seed=35, locality=0.1), "AMD"  # two-ended (test_block_sparse_two_chains)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["band AMD", "band Metis", "plane", "two-ended"])
def test_covariance_block_sparse_equals_dense_and_schur(ba, orc, gpu_ok, name):
    """scenes of many tile rows: the list schedule (BA_SPARSE_S=1, Z on the factor's pattern only) against the dense one
    (BA_SPARSE_S=0) and the inverse of the explicit Schur complement"""
    p, perm = _scene(ba, name)
    kw = _gauge_kw(p)
    lam = 1.0
    fixed = _fixed_vector(ba, p, kw)

    def run():
        m = ba.BALNLPModel(arrays=_arrays(p))
        try:
            ba.set_ordering(m, perm)
            out = ba.covariance(m, p["x0"], lam, **kw)
            return out, ba.schur_pattern(m), ba.schur_ordering_used(m)[1]
        finally:
            m.close()

    (cs, ps, _), pat_s, order = _env("BA_SPARSE_S", "1", run)
    (cd, pd, _), pat_d, _ = _env("BA_SPARSE_S", "0", run)
    assert pat_s[2] and not pat_d[2], (pat_s, pat_d)
    if name == "two-ended":
        assert order == "two-ended", order
    H = _hessian(orc, p, p["x0"], lam, fixed)
    ref_c, ref_p, S, Z = _ref_schur(H, p, fixed)
    kappa = _kappa(S, Z)
    _check(f"covariance_sparse[{name}]", cs, ps, ref_c, ref_p, kappa, fixed, p, tile_fill=pat_s[0], order=order,
           sparse_vs_dense_cam=_block_errs(cs, cd), sparse_vs_dense_pnt=_block_errs(ps, pd))
    _check(f"covariance_dense[{name}]", cd, pd, ref_c, ref_p, kappa, fixed, p)
    assert _block_errs(cs, cd) <= C_BOUND * kappa * EPS and _block_errs(ps, pd) <= C_BOUND * kappa * EPS


@pytest.mark.gpu
def test_covariance_same_bits_and_handle_untouched(ba, small_prob, gpu_ok):
    """two calls give the same bits; an lm_step after a covariance call gives the bits of an lm_step alone"""
    p = small_prob
    kw = _gauge_kw(p)
    a = ba.BALNLPModel(arrays=_arrays(p))
    b = ba.BALNLPModel(arrays=_arrays(p))
    try:
        ref = ba.lm_step(a, p["x0"], 10.0)
        c1 = ba.covariance(b, p["x0"], 0.0, loss="huber", **kw)
        c2 = ba.covariance(b, p["x0"], 0.0, loss="huber", **kw)
        got = ba.lm_step(b, p["x0"], 10.0)
        again = ba.lm_step(a, p["x0"], 10.0)
    finally:
        a.close()
        b.close()
    for x, y, what in ((c1[0], c2[0], "cam_cov"), (c1[1], c2[1], "pnt_cov")):
        assert not bits_report(x, y, what), bits_report(x, y, what)
    assert c1[2] == c2[2]
    for i, what in ((0, "delta"), (2, "jtr")):
        assert not bits_report(got[i], ref[i], what), bits_report(got[i], ref[i], what)
        assert not bits_report(again[i], ref[i], what), bits_report(again[i], ref[i], what)
    assert got[1] == ref[1]


@pytest.mark.gpu
def test_covariance_refuses_a_communicator_and_bad_c_arguments(ba, small_prob, gpu_ok):
    assert os.path.exists(LOOPBACK), f"{LOOPBACK} is missing: __graft_entry__.build() compiles it"
    L = C.CDLL(LOOPBACK)
    L.ba_loopback_create.restype = C.c_void_p
    L.ba_loopback_create.argtypes = [C.c_int, C.c_size_t]
    L.ba_loopback_destroy.argtypes = [C.c_void_p]
    L.ba_loopback_rank.restype = C.c_void_p
    L.ba_loopback_rank.argtypes = [C.c_void_p, C.c_int]
    p = small_prob
    lib = ba._lib.lib()
    m = ba.BALNLPModel(arrays=_arrays(p))
    x = np.ascontiguousarray(p["x0"])
    piv = C.c_double(0)
    try:
        for lam in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ba.BAArgError, match="lambda"):
                ba._lib.check(lib.ba_covariance(m.handle, ba._lib.ptr(x), lam, -1.0, None, None, C.byref(piv)))
        loop = L.ba_loopback_create(1, 16 << 20)
        assert loop
        try:
            hook = C.cast(L.ba_loopback_hook, ba._lib.COMM_CB)
            ba._lib.check(lib.ba_lm_set_comm_hook(m.handle, 0, 1, hook, L.ba_loopback_rank(loop, 0)))
            with pytest.raises(ba.BAArgError, match="communicator"):
                ba.covariance(m, x, 1.0)
        finally:
            m.close()
            L.ba_loopback_destroy(loop)
    finally:
        m.close()
