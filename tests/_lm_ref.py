"""What the tests of the LM terms (robust loss, fixed parameters, covariance, priors, shared intrinsics) share: the numpy
reference of the oracle's residual and Jacobian with the reweighting of a robust loss, the dense covariance references, the
handle's options as vectors, the solve and option builders, and the in-process loopback communicator."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from _util import parity_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPBACK = os.path.join(ROOT, "tests", "helpers", "libba_loopback.so")
EPS = np.finfo(np.float64).eps
C_BOUND = 100.0
STEP_TOL = {1e3: 1e-12, 30.0: 1e-11, 1.0: 1e-11, 1e-2: 1e-9}  # test_lm_step_vs_oracle's limits at these lambda
F32_TOL = 5e-3  # the Float32-factor limit of tests/test_fixed_params.py and tests/test_robust_loss.py
PCG_TOL = 1e-8  # their limit of the pcg=(1e-12, 5000) step


def arrays(p):
    return (p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], p["ncams"], p["npnts"], p["nobs"])


def env(name, value, fn):
    """fn() with the environment variable set to value (None: unset), the variable restored afterwards"""
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def limit(tol, kappa):
    """the project's limit of a step at this lambda, or 100 kappa eps where the conditioning of the damped reduced camera
    system (priors included) is worse: the rule of check_cov"""
    return max(tol, C_BOUND * kappa * EPS)


# ---- numpy reference: residual, Jacobian, reweighting ---------------------------------------------------------------------
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


def weights_cost(r, loss, c):
    s = r[0::2] ** 2 + r[1::2] ** 2
    if loss == "linear":
        return np.ones_like(s), 0.5 * np.sum(s)
    rh, w = rho(loss, s / c ** 2)
    return w, 0.5 * np.sum(c ** 2 * rh)


def residual(orc, p, x):
    return orc.residuals(p["cam_idx1"], p["pnt_idx1"], x, p["pt2d"], p["npnts"])


def jac(orc, p, x):
    rows, cols = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    vals = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], x, p["npnts"])
    nvar = 9 * p["ncams"] + 3 * p["npnts"]
    return sp.csr_matrix((vals, (rows - 1, cols - 1)), shape=(2 * p["nobs"], nvar))


def reweighted(orc, p, x, loss, c):
    """(r~, J~, w, f) under a loss: r~ = sqrt(w) r, J~ = sqrt(w) J, w = rho'(|r_i|^2 / c^2) per observation"""
    r = residual(orc, p, x)
    w, f = weights_cost(r, loss, c)
    sw = np.repeat(np.sqrt(w), 2)
    return sw * r, sp.diags(sw) @ jac(orc, p, x), w, f


# ---- the handle's options as vectors and keywords -------------------------------------------------------------------------
def fixed_vector(ba, p, kw):
    """boolean over x = [points; cameras]: True where the options of kw fix the entry"""
    cam, pnt = ba._lib.fixed_masks(p["ncams"], p["npnts"], kw.get("fixed_cameras"), kw.get("fixed_points"),
                                   kw.get("fixed_camera_params"))
    fixed_p = np.repeat(pnt.astype(bool), 3)
    fixed_c = ((cam[:, None] >> np.arange(9)) & 1).astype(bool).ravel()
    return np.concatenate([fixed_p, fixed_c])


def gauge_kw(p):
    """camera 1's pose (r, t) and the first translation component of camera 2: the 7 DoF of a similarity transform"""
    comp = np.zeros((p["ncams"], 9), dtype=bool)
    comp[0, :6] = True
    comp[1, 3] = True
    return dict(fixed_camera_params=comp)


def solve(ba, m, variant=1, facto="LDL", normalize="None", **kw):
    args = (facto, "AMD", normalize) + ((False,) if variant == 1 else ())
    return ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), *args, **kw)


def lm_opts(ba, **kw):
    """ba_lm_opts with every field at its default (lm.jl's variant, :LDL, :AMD), then the fields of kw"""
    o = ba._lib.LMOpts(variant=1, facto=0, normalize=0, linesearch=0, facto_type=0, ite_max=-1, verbose=0, x_f32=0, restol=-1,
                       satol=-1, srtol=-1, oatol=-1, ortol=-1, atol=-1, rtol=-1, nu_d=-1, nu_m=-1, lam=-1, delta_d=-1, max_time=-1,
                       pcg_tol=-1, pcg_max_iter=-1, perm=0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---- covariance references (tests/test_covariance.py, the covariance test of tests/test_priors.py) ---------------------------
def hessian(orc, p, x, lam, fixed, loss=None, c=1.0):
    """J~_F'J~_F + diag(lam on the free entries, 1 on the fixed ones) (sparse; the fixed rows / columns hold only the 1)"""
    J = reweighted(orc, p, x, loss, c)[1] if loss else jac(orc, p, x)
    J = J @ sp.diags((~fixed).astype(float))
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


# ---- several ranks in one process over the stream-ordered loopback transport (tests/helpers/ba_loopback.hip) -----------------
_loopback_lib = None


def loopback_lib():
    """the loopback transport's library, its ctypes signatures declared"""
    global _loopback_lib
    if _loopback_lib is None:
        assert os.path.exists(LOOPBACK), f"{LOOPBACK} is missing: __graft_entry__.build() compiles it"
        L = C.CDLL(LOOPBACK)
        L.ba_loopback_create.restype = C.c_void_p
        L.ba_loopback_create.argtypes = [C.c_int, C.c_size_t]
        L.ba_loopback_destroy.argtypes = [C.c_void_p]
        L.ba_loopback_rank.restype = C.c_void_p
        L.ba_loopback_rank.argtypes = [C.c_void_p, C.c_int]
        L.ba_loopback_ops.restype = C.c_long
        L.ba_loopback_ops.argtypes = [C.c_void_p]
        _loopback_lib = L
    return _loopback_lib


@contextlib.contextmanager
def loopback_world(world, stage_bytes):
    """(library, communicator) of `world` ranks with stage_bytes of staging each; destroyed on exit"""
    L = loopback_lib()
    loop = L.ba_loopback_create(world, stage_bytes)
    assert loop, "loopback communicator could not be created"
    try:
        yield L, loop
    finally:
        L.ba_loopback_destroy(loop)


def attach_loopback(ba, m, L, loop, rank, world):
    """rank `rank` of the communicator as the handle's transport (before the handle's first solve)"""
    hook = C.cast(L.ba_loopback_hook, ba._lib.COMM_CB)
    ba._lib.check(ba._lib.lib().ba_lm_set_comm_hook(m.handle, rank, world, hook, L.ba_loopback_rank(loop, rank)))


@pytest.fixture(scope="module")
def loopback(gpu_ok):
    return loopback_lib()


class Ranks:
    """`world` shards of one problem as handles in this process, attached to one loopback communicator."""

    def __init__(self, ba, L, prob, world, stage_mb=64):
        self.ba, self.L, self.world, self.prob = ba, L, world, prob
        whole = ba.synthetic.as_arrays(prob)
        self.loop = L.ba_loopback_create(world, stage_mb << 20)
        assert self.loop, "loopback communicator could not be created"
        self.shards, self.models = [], []
        for r in range(world):
            local, info = ba.parallel.shard_problem(whole, r, world)
            m = ba.BALNLPModel(arrays=local, device=0)
            attach_loopback(ba, m, L, self.loop, r, world)
            self.shards.append((local, info))
            self.models.append(m)

    def step(self, lam, **kw):
        """one sharded LM step, every rank on its own host thread -> (global delta from rank 0's cameras, per-rank camera
        parts, model value)"""
        out, err = [None] * self.world, [None] * self.world

        def run(r):
            try:
                out[r] = self.ba.lm_step(self.models[r], self.shards[r][0][3], lam, **kw)
            except Exception as e:  # noqa: BLE001 -- reported below with the rank
                err[r] = e

        ts = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        bad = [(r, e) for r, e in enumerate(err) if e is not None]
        assert not bad, f"rank(s) failed: {bad}"
        ncams, npnts = self.prob["ncams"], self.prob["npnts"]
        delta = np.zeros(3 * npnts + 9 * ncams)
        cams = []
        for r in range(self.world):
            pb, pe = self.shards[r][1]["point_range"]
            d = out[r][0]
            delta[3 * pb:3 * pe] = d[:3 * (pe - pb)]
            cams.append(d[3 * (pe - pb):].copy())
        delta[3 * npnts:] = cams[0]
        return delta, cams, out[0][1]

    def close(self):
        for m in self.models:
            m.close()
        self.L.ba_loopback_destroy(self.loop)
