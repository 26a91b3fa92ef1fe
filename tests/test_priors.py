"""Gaussian priors of the LM solve (ba_lm_set_priors, include/ba_hip.h): priors on points, camera blocks and
camera centres c(r, t) = -R(r)' t, added to the objective as 1/2 sum_k d_k' Lambda_k d_k, d_k = h_k(x) - mu_k.  The references
are numpy (tests/_lm_ref.py): the oracle's residual and Jacobian plus the prior rows restated in numpy, the dense
solve of the augmented normal equations, a dense LM loop.  The numpy centre is checked against the oracle's P1 (R c + t = 0) and
its complex-step Jacobian against central differences.  The first tests need no device; the rest run on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial.transform import Rotation

import _lm_ref as pr
from _lm_ref import (F32_TOL, PCG_TOL, STEP_TOL, check_cov, hessian, jac, kappa_jacobi, limit, linearise, lm_dense, ref_dense,
                     residual, schur, step, sym)
from _lm_run import arrays, attach_loopback, env, fixed_vector, lm_opts, loopback_world, solve
from _util import bits_report, parity_record, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prior_set(p, offset=0.01, seed=5):
    """All three kinds on a scene: 40 control points with full 3 x 3 information blocks; 3 cameras with a correlated prior on
    (r, t, f) and k1, k2 left free (zero rows and columns); 4 centres, three at sigma = 0.01 and one "height only" (standard
    deviations with inf).  The means sit `offset` sigma-scaled units away from x_true."""
    rng = np.random.default_rng(seed)
    np3 = 3 * p["npnts"]
    X = p["x_true"][:np3].reshape(-1, 3)
    cams = p["x_true"][np3:].reshape(-1, 9)
    pidx = np.arange(3, p["npnts"] + 1, max(1, p["npnts"] // 40))[:40]
    B = rng.standard_normal((len(pidx), 3, 3))
    pinfo = sym(1e4 * B @ np.swapaxes(B, 1, 2) + 1e3 * np.eye(3))
    pmu = X[pidx - 1] + offset * rng.standard_normal((len(pidx), 3))
    cidx = np.array([2, 5, 9])
    sig = np.array([0.01, 0.01, 0.01, 0.05, 0.05, 0.05, 1.0, 1.0, 5.0])
    keep = np.array([1, 1, 1, 1, 1, 1, 0, 0, 1.0])
    cinfo = np.empty((len(cidx), 9, 9))
    for q in range(len(cidx)):
        Q = np.linalg.qr(rng.standard_normal((9, 9)))[0]
        M = Q @ np.diag(rng.uniform(0.5, 2.0, 9)) @ Q.T
        D = keep / sig
        cinfo[q] = sym(D[:, None] * M * D[None, :])
    cmu = cams[cidx - 1] + (offset / 0.01) * sig * keep * rng.standard_normal((len(cidx), 9))
    tidx = np.array([1, 6, 12, 7])
    tsig = np.full((4, 3), 0.01)
    tsig[3] = (np.inf, np.inf, 0.02)
    tmu = np.stack([pr.centre(cams[i - 1]) for i in tidx]) + offset * rng.standard_normal((4, 3))
    return dict(point_priors=(pidx, pmu, pinfo), camera_priors=(cidx, cmu, cinfo), centre_priors=(tidx, tmu, tsig))


def _subsets(kw):
    return {"point": {"point_priors": kw["point_priors"]}, "camera": {"camera_priors": kw["camera_priors"]},
            "centre": {"centre_priors": kw["centre_priors"]}, "all": kw}


def _unpack(ref):
    """(delta, model, gradient, kappa of the Jacobi-scaled damped S with the priors) of _lm_ref.step's record"""
    return ref["delta"], ref["model"], ref["grad"], ref["kappa"]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_numpy_centre_and_its_jacobian(ba, orc, small_prob):
    """The reference's own checks: R c + t = 0 through the oracle's P1 (a few ulps of |t| ~ 7), the complex-step Jacobian
    against central differences (h = 1e-6: truncation h^2, rounding eps / h)."""
    p = small_prob
    cams = p["x0"][3 * p["npnts"]:].reshape(-1, 9)
    worst = max(np.max(np.abs(orc.P1(c[:3], c[3:6], pr.centre(c)))) for c in cams)
    assert worst <= 1e-14, worst
    for c in cams:
        H = pr.centre_jac(c)
        assert np.max(np.abs(H - pr.centre_jac_fd(c))) <= 1e-8 * np.max(np.abs(H))
        assert np.max(np.abs(H[:, 3:] + pr.rotation(c[:3]).T)) <= 1e-15  # dc/dt = -R'


_GOOD = (np.array([1, 2]), np.zeros((2, 3)), np.ones((2, 3)))
_BAD = [
    {"point_priors": (np.array([1, 2]), np.zeros((2, 3)))},                                  # not a triple
    {"point_priors": (np.array([0, 2]), np.zeros((2, 3)), np.ones((2, 3)))},                 # index 0
    {"point_priors": (np.array([2, 2]), np.zeros((2, 3)), np.ones((2, 3)))},                 # repeated
    {"point_priors": (np.array([1.5, 2]), np.zeros((2, 3)), np.ones((2, 3)))},               # not integers
    {"point_priors": (np.array([1, 2]), np.zeros((2, 4)), np.ones((2, 3)))},                 # mu shape
    {"point_priors": (np.array([1, 2]), np.zeros((2, 3)), np.ones((2, 2)))},                 # info shape
    {"point_priors": (np.array([1, 2]), np.full((2, 3), np.nan), np.ones((2, 3)))},          # mu not finite
    {"point_priors": (np.array([1, 2]), np.zeros((2, 3)), np.zeros((2, 3)))},                # sigma 0
    {"point_priors": (np.array([1, 2]), np.zeros((2, 3)), -np.ones((2, 3)))},                # sigma < 0
    {"camera_priors": (np.array([1]), np.zeros((1, 9)), np.ones((1, 3, 3)))},                # block size
    {"camera_priors": (np.array([1]), np.zeros((1, 9)), np.triu(np.ones((9, 9)))[None])},    # asymmetric
    {"centre_priors": (np.array([1]), np.zeros((1, 3)), np.array([[[1.0, 2, 0], [2, 1, 0], [0, 0, 1]]]))},  # not PSD
    {"centre_priors": (np.array([1]), np.zeros((1, 3)), -np.eye(3)[None])},                  # negative diagonal
    {"centre_priors": (np.array([1]), np.zeros((1, 3)), np.full((1, 3, 3), np.inf))},        # block not finite
]


@pytest.mark.parametrize("bad", _BAD)
def test_bad_priors_refused_before_the_device(ba, bad):
    """No model exists here (None): the ValueError comes before anything looks at the model or the device."""
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, **bad)
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", **bad)
    with pytest.raises(ValueError):
        ba.lm_step(None, np.zeros(3), 1.0, **bad)
    with pytest.raises(ValueError):
        ba.covariance(None, np.zeros(3), **bad)


def test_refused_combinations_before_the_device(ba):
    with pytest.raises(ValueError, match="linesearch"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", True, point_priors=_GOOD)
    with pytest.raises(ValueError, match="Float16"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, facto_type=np.float16, centre_priors=_GOOD)
    assert ba._lib.check_priors(point_priors=_GOOD) and not ba._lib.check_priors()
    assert not ba._lib.check_priors(point_priors=(np.zeros(0, dtype=int), np.zeros((0, 3)), np.zeros((0, 3))))


def test_prior_forms_pack_to_the_c_layout(ba):
    """standard deviations -> diag(1 / sigma^2) with inf -> 0; full blocks -> packed lower row-major; boolean index arrays"""
    idx, mu, info = ba._lib._prior_lists((np.array([3, 1]), np.zeros((2, 3)), np.array([[0.1, np.inf, 2.0], [1.0, 1.0, 1.0]])), 3, 5, "x")
    assert idx.tolist() == [3, 1] and info.shape == (2, 6)
    assert np.allclose(info[0], [100.0, 0, 0, 0, 0, 0.25]) and info[0, 2] == 0.0
    M = np.arange(81.0).reshape(9, 9)
    M = M + M.T + 200 * np.eye(9)
    _, _, packed = ba._lib._prior_lists((np.array([True, False]), np.zeros((1, 9)), M[None]), 9, 2, "x")
    il, jl = np.tril_indices(9)
    assert packed.shape == (1, 45) and np.array_equal(packed[0], M[il, jl])
    assert packed[0, 1] == M[1, 0] and packed[0, 2] == M[1, 1] and packed[0, 3] == M[2, 0]


def test_symbols_and_c_abi_argument_checks(ba):
    """the three entries are declared and exported; what ba_lm_set_priors can refuse without a handle"""
    L = ba._lib.lib()
    for name in ("ba_lm_set_priors", "ba_lm_get_priors", "ba_prior_eval"):
        assert name in ba._lib.SYMBOLS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_lm_set_priors", "ba_lm_get_priors", "ba_prior_eval"):
        assert f"int {name}(" in header
    assert L.ba_lm_set_priors(None, *([0, None, None, None] * 3)) == 1
    assert L.ba_lm_get_priors(None, None, None, None) == 1
    assert L.ba_prior_eval(None, None, None, None, None, None) == 1
    with pytest.raises(ba.BAArgError, match="null handle"):
        ba._lib.check(L.ba_lm_set_priors(None, *([0, None, None, None] * 3)))
    for kw in ("point_priors", "camera_priors", "centre_priors"):
        assert kw in ba.Levenberg_Marquardt.__kwdefaults__ and kw in ba.covariance.__kwdefaults__
        assert kw in ba.lm_step.__code__.co_varnames
    assert callable(ba.BALNLPModel.prior_eval)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c_abi_refuses_bad_lists_and_keeps_the_handle(ba, small_prob, gpu_ok):
    """ba_lm_set_priors through ctypes: index out of range / repeated, a value that is not finite, a negative diagonal entry,
    Lambda_ij^2 > Lambda_ii Lambda_jj -> BA_ERR_ARG, and the handle keeps what it had."""
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p))
    L = ba._lib.lib()
    try:
        ba._lib.set_priors(m.handle, p["ncams"], p["npnts"], point_priors=_GOOD)
        assert ba._lib.get_priors(m.handle) == (2, 0, 0)

        def call(idx, mu, info, kind=0):
            idx, mu, info = np.array(idx, dtype=np.int64), np.array(mu, dtype=float), np.array(info, dtype=float)
            args = [0, None, None, None] * 3
            args[4 * kind:4 * kind + 4] = [len(idx), ba._lib.ptr(idx), ba._lib.ptr(mu), ba._lib.ptr(info)]
            return L.ba_lm_set_priors(m.handle, *args)

        ok6 = [1.0, 0, 1, 0, 0, 1]
        assert call([p["npnts"] + 1], [0.0] * 3, ok6) == 1 and "outside" in L.ba_last_error().decode()
        assert call([0], [0.0] * 3, ok6) == 1
        assert call([4, 4], [0.0] * 6, ok6 * 2) == 1 and "twice" in L.ba_last_error().decode()
        assert call([1], [np.nan, 0, 0], ok6) == 1 and "finite" in L.ba_last_error().decode()
        assert call([1], [0.0] * 3, [1.0, 0, np.inf, 0, 0, 1]) == 1
        assert call([1], [0.0] * 3, [1.0, 0, -1.0, 0, 0, 1]) == 1 and "negative" in L.ba_last_error().decode()
        assert call([1], [0.0] * 3, [1.0, 2.0, 1.0, 0, 0, 1]) == 1 and "semi-definite" in L.ba_last_error().decode()
        assert call([p["ncams"] + 1], [0.0] * 3, ok6, kind=2) == 1
        assert call([p["ncams"] + 1], [0.0] * 9, [0.0] * 45, kind=1) == 1
        assert ba._lib.get_priors(m.handle) == (2, 0, 0)
        assert call([1], [0.0] * 3, [1.0, 1.0, 1.0, 0, 0, 0]) == 0  # rank one, a zero row: valid
        assert ba._lib.get_priors(m.handle) == (1, 0, 0)
        ba._lib.set_priors(m.handle, p["ncams"], p["npnts"])
        assert ba._lib.get_priors(m.handle) == (0, 0, 0)
    finally:
        m.close()


@pytest.mark.gpu
def test_prior_eval_against_numpy(ba, orc, small_prob, gpu_ok):
    """Cost and per-prior chi^2 to 1e-13 relative, all three kinds.  The means sit 0.5 units from the truth, so d is not a
    small difference of large numbers: a centre carries a few ulps of |c| ~ 7 (1e-15), which is 1e-14 of such a d."""
    p = small_prob
    kw = _prior_set(p, offset=0.5)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cost, cp, cc, ct = m.prior_eval(p["x0"], **kw)
        assert ba._lib.get_priors(m.handle) == (40, 3, 4)
        rows = pr.rows(p["x0"], p["ncams"], p["npnts"], **kw)
        ref = pr.chi2(rows)
        worst = 0.0
        for got, kind in ((cp, "point"), (cc, "camera"), (ct, "centre")):
            e = float(np.max(np.abs(got - ref[kind]) / ref[kind]))
            print(f"prior_eval: {kind} chi2, max relative error {e:.3e}")
            worst = max(worst, e)
        ecost = abs(cost - pr.cost(rows)) / pr.cost(rows)
        print(f"prior_eval: cost {cost!r} vs numpy {pr.cost(rows)!r} ({ecost:.3e})")
        parity_record("prior_eval", chi2_rel_err=worst, cost_rel_err=ecost)
        assert worst <= 1e-13 and ecost <= 1e-13
        none = m.prior_eval(p["x0"])  # nothing given clears the handle's priors
        assert none[0] == 0.0 and all(v.size == 0 for v in none[1:]) and ba._lib.get_priors(m.handle) == (0, 0, 0)
    finally:
        m.close()


@pytest.mark.gpu
def test_cleared_priors_leave_the_plain_bits(ba, small_prob, gpu_ok):
    """after calls with priors, calls without them give the bits of a handle that never had any: lm_step and robust_eval"""
    p = small_prob
    kw = _prior_set(p)
    m = ba.BALNLPModel(arrays=arrays(p))
    fresh = ba.BALNLPModel(arrays=arrays(p))
    try:
        with_p = ba.lm_step(m, p["x0"], 1.0, **kw)
        m.prior_eval(p["x0"], **kw)
        a = ba.lm_step(m, p["x0"], 1.0)
        assert ba._lib.get_priors(m.handle) == (0, 0, 0)
        b = ba.lm_step(fresh, p["x0"], 1.0)
        for got, want, name in zip(a, b, ("delta", "half_sq_model", "jtr")):
            rep = bits_report(np.atleast_1d(got), np.atleast_1d(want), f"{name} after priors were cleared vs a fresh handle")
            assert not rep, rep
        assert rel_err(with_p[0], b[0]) > 1e-6
        wb, fb = fresh.robust_weights(p["x0"], "huber", 1.0)
        ba._lib.set_priors(m.handle, p["ncams"], p["npnts"], **kw)
        wa, fa = m.robust_weights(p["x0"], "huber", 1.0)  # (the model entries ignore the priors)
        assert not bits_report(wa, wb, "robust weights with priors set") and fa == fb
        ba.lm_step(m, p["x0"], 1.0, loss="huber", **kw)  # priors uploaded and used under the loss, then cleared
        ba._lib.set_priors(m.handle, p["ncams"], p["npnts"])
        assert ba._lib.get_priors(m.handle) == (0, 0, 0)
        wa, fa = m.robust_weights(p["x0"], "huber", 1.0)
        assert not bits_report(wa, wb, "robust weights after priors were cleared vs a fresh handle") and fa == fb
    finally:
        m.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", ["point", "camera", "centre", "all"])
def test_prior_step_vs_dense_numpy(ba, orc, small_prob, gpu_ok, kinds):
    """The step of the augmented normal equations at the four lambda of STEP_TOL: :LDL, facto_type = Float32 and
    pcg = (1e-12, 5000).  Limits: STEP_TOL / 5e-3 / 1e-8, or 100 kappa eps (Float64's eps, as tests/_lm_ref.py::check_cov)
    where that is larger -- for the Float32 factor it never is here: 5e-3 on every case."""
    p = small_prob
    pri = _subsets(_prior_set(p))[kinds]
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            d_ref, mod_ref, g_ref, kappa = _unpack(step(orc, p, p["x0"], lam, priors=pri))
            d, half, jtr = ba.lm_step(m, p["x0"], lam, **pri)
            d32 = ba.lm_step(m, p["x0"], lam, facto_type=np.float32, **pri)[0]
            dp, halfp, _, its = ba.lm_step(m, p["x0"], lam, pcg=(1e-12, 5000), **pri)
            e, e32, ep = rel_err(d, d_ref), rel_err(d32, d_ref), rel_err(dp, d_ref)
            em = abs(half - mod_ref) / mod_ref
            eg = float(np.linalg.norm(jtr - g_ref) / np.linalg.norm(g_ref))
            lim, lim32, limp = limit(tol, kappa), limit(F32_TOL, kappa), limit(PCG_TOL, kappa)
            print(f"prior_step[{kinds}] lambda {lam:g}: kappa {kappa:.3e}  LDL {e:.3e} (limit {lim:.1e})  f32 {e32:.3e} "
                  f"({lim32:.1e})  pcg {ep:.3e} ({limp:.1e}, {its} its)  model {em:.3e}  jtr {eg:.3e}")
            parity_record(f"prior_step[{kinds}-{lam:g}]", kappa=kappa, ldl=e, ldl_limit=lim, f32=e32, f32_limit=lim32, pcg=ep,
                          pcg_limit=limp, model=em, jtr=eg, cg_iters=its)
            assert e <= lim, f"{kinds}, lambda {lam}: :LDL step {e:.3e} > {lim:.3e}"
            assert e32 <= lim32, f"{kinds}, lambda {lam}: Float32-factor step {e32:.3e} > {lim32:.3e}"
            assert ep <= limp, f"{kinds}, lambda {lam}: PCG step {ep:.3e} > {limp:.3e}"
            assert em <= 1e-10, f"{kinds}, lambda {lam}: model value {half!r} vs {mod_ref!r}"
            assert abs(halfp - mod_ref) <= 1e-7 * mod_ref  # (the PCG step's own model value: its step is 1e-8 off)
            assert eg <= 1e-12, f"{kinds}, lambda {lam}: gradient {eg:.3e}"
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["linear", "huber"])
def test_prior_step_with_loss_and_fixed_mask(ba, orc, small_prob, gpu_ok, loss):
    """Camera 6 is fixed as a whole and carries a centre prior; point 3 is fixed and carries a point prior; the intrinsics
    of camera 2 (which has a camera prior) are fixed too.  Fixed entries of delta and jtr are exactly 0, the free part is
    numpy's.  Priors are not passed through the loss.  Under huber the reference keeps the form with the fixed columns zeroed
    (step(zeroed=True)): at lambda = 1 it differs from the solve over the free columns by 1.04e-12, a tenth of the limit."""
    p = small_prob
    pri = _prior_set(p)
    comp = np.zeros((p["ncams"], 9), dtype=bool)
    comp[1, 6:] = True
    mask = dict(fixed_cameras=[6], fixed_points=[3, 50], fixed_camera_params=comp)
    fixed = fixed_vector(ba, p, mask)
    assert 3 in pri["point_priors"][0] and 6 in pri["centre_priors"][0] and 2 in pri["camera_priors"][0]
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            ref = step(orc, p, p["x0"], lam, priors=pri, fixed=fixed, loss=loss, c=1.0, zeroed=loss == "huber")
            d_ref, mod_ref, g_ref, kappa = _unpack(ref)
            d, half, jtr = ba.lm_step(m, p["x0"], lam, loss=loss, f_scale=1.0, **mask, **pri)
            assert np.all(d[fixed] == 0.0), f"lambda {lam}: {np.count_nonzero(d[fixed])} fixed entries of delta are not 0"
            assert np.all(jtr[fixed] == 0.0), f"lambda {lam}: fixed entries of the gradient are not 0"
            e, lim = rel_err(d, d_ref), limit(tol, kappa)
            em = abs(half - mod_ref) / mod_ref
            eg = float(np.linalg.norm(jtr - g_ref) / np.linalg.norm(g_ref))
            print(f"prior_step_masked[{loss}] lambda {lam:g}: kappa {kappa:.3e}  step {e:.3e} (limit {lim:.1e})  model {em:.3e}  "
                  f"jtr {eg:.3e}")
            parity_record(f"prior_step_masked[{loss}-{lam:g}]", kappa=kappa, ldl=e, ldl_limit=lim, model=em, jtr=eg)
            assert e <= lim and em <= 1e-10 and eg <= 1e-12
        if loss == "huber":  # the loss acts on the observations only: the step differs from the linear one, the prior cost does not
            assert rel_err(d, step(orc, p, p["x0"], 1e-2, priors=pri, fixed=fixed)["delta"]) > 1e-6
    finally:
        m.close()


@pytest.mark.gpu
def test_prior_step_block_sparse_schedule(ba, orc, gpu_ok):
    """The scene of test_robust_step_block_sparse_schedule: with BA_SPARSE_S=1 and =0 the step is numpy's to that test's
    limit (1e-10, or 100 kappa eps)."""
    p = ba.synthetic.make_problem(300, 700, 3500, seed=5, locality=0.08)
    rng = np.random.default_rng(3)
    np3 = 3 * p["npnts"]
    cams = p["x_true"][np3:].reshape(-1, 9)
    tidx = np.arange(1, 301, 10)
    pidx = np.arange(2, 701, 20)
    pri = dict(centre_priors=(tidx, np.stack([pr.centre(cams[i - 1]) for i in tidx]) + 0.01 * rng.standard_normal((30, 3)),
                              np.full((30, 3), 0.01)),
               point_priors=(pidx, p["x_true"][:np3].reshape(-1, 3)[pidx - 1], np.full((len(pidx), 3), 0.005)))
    lam = 1.0
    d_ref, mod_ref, g_ref, kappa = _unpack(step(orc, p, p["x0"], lam, priors=pri))
    lim = limit(1e-10, kappa)
    for flag in ("1", "0"):
        def run():
            m = ba.BALNLPModel(arrays=arrays(p))
            try:
                return ba.lm_step(m, p["x0"], lam, **pri), ba.schur_pattern(m)
            finally:
                m.close()

        (d, half, jtr), pat = env("BA_SPARSE_S", flag, run)
        assert pat[2] == (flag == "1"), "the schedule asked for was not used"
        e = rel_err(d, d_ref)
        print(f"prior_step_sparse[BA_SPARSE_S={flag}]: kappa {kappa:.3e}  step {e:.3e} (limit {lim:.1e})")
        parity_record(f"prior_step_sparse[{flag}]", kappa=kappa, step=e, limit=lim)
        assert e <= lim
        assert abs(half - mod_ref) <= 1e-10 * mod_ref
        assert np.linalg.norm(jtr - g_ref) <= 1e-12 * np.linalg.norm(g_ref)


def _objective_and_gradient(orc, p, x, pri):
    r = residual(orc, p, x)
    rows = pr.rows(x, p["ncams"], p["npnts"], **pri)
    g = jac(orc, p, x).T @ r + pr.normal_terms(rows, len(x))[1]
    return 0.5 * (r @ r) + pr.cost(rows), float(np.linalg.norm(g))


def _solve(ba, m, variant, facto, normalize, **kw):
    return solve(ba, m, variant, facto, normalize, oatol=0.0, ortol=0.0, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,facto,normalize", [(1, "LDL", "None"), (1, "LDL", "J"), (0, "LDL", "None"), (0, "LDL", "J"),
                                                     (1, "PCG", "None"), (0, "PCG", "None")])
def test_prior_solve(ba, orc, small_prob, gpu_ok, variant, facto, normalize):
    p = small_prob
    pri = _prior_set(p)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = _solve(ba, m, variant, facto, normalize, **pri)
        st2 = _solve(ba, m, variant, facto, normalize, **pri)
    finally:
        m.close()
    f_acc = [row[1] for row in st.log if row[7]]
    assert len(f_acc) >= 2 and all(b < a for a, b in zip(f_acc, f_acc[1:])), f"accepted rows: f not strictly decreasing {f_acc}"
    f_ref, g_ref = _objective_and_gradient(orc, p, st.solution, pri)
    feas = st.dual_feas if variant == 1 else st.primal_feas
    ef, eg = abs(st.objective - f_ref) / f_ref, abs(feas - g_ref) / g_ref
    print(f"prior_solve[{variant}-{facto}-{normalize}]: status {st.status}, {st.iter} iterations, objective {ef:.3e}, "
          f"gradient norm {eg:.3e}")
    parity_record(f"prior_solve[{variant}-{facto}-{normalize}]", objective=ef, dual_feas=eg, iter=st.iter, status=st.status)
    assert ef <= 1e-12, f"objective {st.objective!r} vs numpy {f_ref!r}"
    assert eg <= 1e-10, f"gradient norm {feas!r} vs numpy {g_ref!r}"
    assert st.status in ("first_order", "small_step"), st.status
    rep = bits_report(st.solution, st2.solution, "two runs")
    assert not rep, rep
    assert st.log == st2.log


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 0])
def test_prior_solve_with_huber(ba, orc, small_prob, gpu_ok, variant):
    """A complete solve with priors under a robust loss: the checks of test_prior_solve against the robust objective plus the
    priors, and -- variant 1 -- the gain ratio of the first log row against numpy.  Under a loss the controller predicts
    m(0) - m(delta) with m(0) = 1/2 |r~|^2 + f_prior (not f, which holds rho): the one place that reads the priors' share of
    the zero-step model value.  Limit of the ratio: the step is numpy's to 1e-11 (STEP_TOL) and both differences are of the
    order of f itself at x0, so 1e-9 leaves two digits."""
    p = small_prob
    pri = _prior_set(p)
    loss, c = "huber", 1.0
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = _solve(ba, m, variant, "LDL", "None", loss=loss, f_scale=c, **pri)
        st2 = _solve(ba, m, variant, "LDL", "None", loss=loss, f_scale=c, **pri)
    finally:
        m.close()

    def terms(x):
        rt, Jt, _, f_obs = linearise(orc, p, x, loss=loss, c=c)
        rows = pr.rows(x, p["ncams"], p["npnts"], **pri)
        return rt, Jt, rows, f_obs + pr.cost(rows)

    f_acc = [row[1] for row in st.log if row[7]]
    assert len(f_acc) >= 2 and all(b < a for a, b in zip(f_acc, f_acc[1:])), f"accepted rows: f not strictly decreasing {f_acc}"
    rt, Jt, rows, f_ref = terms(st.solution)
    g_ref = float(np.linalg.norm(Jt.T @ rt + pr.normal_terms(rows, len(st.solution))[1]))
    feas = st.dual_feas if variant == 1 else st.primal_feas
    ef, eg = abs(st.objective - f_ref) / f_ref, abs(feas - g_ref) / g_ref
    print(f"prior_solve_huber[{variant}]: status {st.status}, {st.iter} iterations, objective {ef:.3e}, gradient norm {eg:.3e}")
    assert ef <= 1e-12, f"objective {st.objective!r} vs numpy {f_ref!r}"
    assert eg <= 1e-10, f"gradient norm {feas!r} vs numpy {g_ref!r}"
    assert st.status in ("first_order", "small_step"), st.status
    rep = bits_report(st.solution, st2.solution, "two runs")
    assert not rep, rep
    assert st.log == st2.log
    rec = dict(objective=ef, dual_feas=eg, iter=st.iter, status=st.status)
    if variant == 1:
        row = st.log[0]
        x0, lam = p["x0"], row[4]
        rt, Jt, rows, f0 = terms(x0)
        ref = step(orc, p, x0, lam, priors=pri, loss=loss, c=c)
        d, mod = ref["delta"], ref["model"]
        pred = 0.5 * (rt @ rt) + pr.cost(rows) - mod
        ared = f0 - terms(x0 + d)[3]
        erho = abs(row[6] - ared / pred) / abs(ared / pred)
        print(f"prior_solve_huber[1]: first row lambda {lam:g}, rho {row[6]!r} vs numpy {ared / pred!r} ({erho:.3e}); "
              f"f_prior / pred = {pr.cost(rows) / pred:.3e}")
        assert abs(row[1] - f0) <= 1e-12 * f0
        assert erho <= 1e-9, f"gain ratio {row[6]!r} vs numpy {ared / pred!r}"
        rec["rho_first_row"] = erho
    parity_record(f"prior_solve_huber[{variant}]", **rec)


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [None, "0"])
def test_no_stale_recorded_sequence_with_priors(ba, small_prob, gpu_ok, prefetch):
    """ONE handle solves with priors, without, with other priors, with fewer kinds, without: each solve gives the bits and the
    log of the same solve on a fresh handle -- a sequence recorded for one set of priors is never replayed for another."""
    p = small_prob
    a, b = _prior_set(p), _prior_set(p, seed=6)
    seq = [a, {}, b, {"centre_priors": a["centre_priors"]}, {"point_priors": b["point_priors"]}, {}]

    def run():
        shared = ba.BALNLPModel(arrays=arrays(p))
        try:
            for k, pri in enumerate(seq):
                s1 = _solve(ba, shared, 1, "LDL", "None", **pri)
                fresh = ba.BALNLPModel(arrays=arrays(p))
                s2 = _solve(ba, fresh, 1, "LDL", "None", **pri)
                fresh.close()
                rep = bits_report(s1.solution, s2.solution, f"solve {k} ({sorted(pri)}): reused handle vs fresh handle")
                assert not rep, rep
                assert s1.log == s2.log, f"solve {k}: log rows differ between the reused and a fresh handle"
        finally:
            shared.close()

    env("BA_LM_PREFETCH", prefetch, run)


@pytest.mark.gpu
def test_no_prior_kernel_without_priors(ba, small_prob, gpu_ok):
    """With no prior set a solve launches no prior kernel, and its kernel classes and call counts are those of a handle that
    had priors and lost them; with priors the class appears."""
    p = small_prob
    pri = _prior_set(p)

    def profile(m, **kw):
        m.profile(True)
        st = _solve(ba, m, 1, "LDL", "None", **kw)
        prof = {k: v[1] for k, v in m.profile_get().items() if v[1] > 0}
        m.profile(False)
        return st, prof

    m = ba.BALNLPModel(arrays=arrays(p))
    fresh = ba.BALNLPModel(arrays=arrays(p))
    try:
        _, plain = profile(fresh)
        st_p, with_p = profile(m, **pri)
        _, after = profile(m)
    finally:
        m.close()
        fresh.close()
    print("kernel classes of a solve without priors:", plain)
    assert "k_prior" not in plain and "k_prior" not in after
    assert after == plain
    # the classes of a plain :LDL solve on one GPU: the model and normal-equation passes, the factorisation of the one-tile S
    # and its triangular solves, the reductions; nothing of the loss, the mask, the covariance, the priors or a transport
    required = {"k_residual", "k_jac_coord", "k_point_blocks", "k_cam_blocks", "k_schur_prep", "k_schur_blocks", "k_schur_rhs",
                "k_ldl_diag", "k_tri_solve", "k_backsub", "k_reduce"}
    optional = {"k_model_sq", "k_ldl_trsm", "k_ldl_col", "k_ldl_update", "k_ldl_update_rs"}
    assert required <= set(plain) <= required | optional, sorted(plain)
    # one k_prior scope per linearisation (first + accepted steps), and per linear step one for the camera right-hand side
    # and one for the trial point
    assert with_p["k_prior"] == st_p.n_jacobian + 2 * st_p.n_factor, (with_p["k_prior"], st_p.n_jacobian, st_p.n_factor)


@pytest.mark.gpu
def test_centre_priors_make_the_covariance_well_defined(ba, orc, small_prob, gpu_ok):
    """Gauge free, lambda = 0: centre priors (sigma = 0.01) on cameras 1, 6, 12 fix the similarity softly -- the covariance is
    the dense inverse (numpy's S has min D_i / S_ii = 3.1e-4); on cameras 1 and 6 only, the rotation about their axis stays
    free (numpy's S: smallest eigenvalue ~1e-10 against 8e6) and the call is refused like the prior-free one."""
    p = small_prob
    x = p["x0"]
    np3 = 3 * p["npnts"]
    cams = x[np3:].reshape(-1, 9)
    fixed = np.zeros(len(x), dtype=bool)

    def pri(sel):
        return dict(centre_priors=(np.array(sel), np.stack([pr.centre(cams[i - 1]) for i in sel]), np.full((len(sel), 3), 0.01)))

    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        with pytest.raises(ba.SQDException):
            ba.covariance(m, x, 0.0)
        cov_c, cov_p, piv = ba.covariance(m, x, 0.0, **pri([1, 6, 12]))
        with pytest.raises(ba.SQDException) as ei:
            ba.covariance(m, x, 0.0, **pri([1, 6]))
        assert "gauge" in str(ei.value)
        cams_cov2, _, piv2 = ba.covariance(m, x, 0.0, points=False, **pri([1, 6, 12]))  # ... and the handle is as before
        assert not bits_report(cams_cov2, cov_c, "camera blocks, second call") and piv2 == piv
    finally:
        m.close()
    rows = pr.rows(x, p["ncams"], p["npnts"], **pri([1, 6, 12]))
    H = (hessian(orc, p, x, 0.0, fixed) + sp.csr_matrix(pr.normal_terms(rows, len(x))[0])).tocsr()
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    check_cov("covariance_centre_priors", cov_c, cov_p, ref_c, ref_p, kappa_jacobi(S), fixed, p, min_rel_pivot=piv)
    assert piv > 1e-10, piv


def _similarity(x, npnts, s, Q, T):
    """the scene under X -> s Q X + T: every reprojection is unchanged (R -> R Q', t -> s t - R Q' T)"""
    y = x.copy()
    np3 = 3 * npnts
    y[:np3] = (s * x[:np3].reshape(-1, 3) @ Q.T + T).ravel()
    for c in y[np3:].reshape(-1, 9):
        R2 = pr.rotation(c[:3]) @ Q.T
        c[:3] = Rotation.from_matrix(R2).as_rotvec()
        c[3:6] = s * c[3:6] - R2 @ T
    return y


@pytest.mark.gpu
def test_control_points_bring_the_scene_back(ba, orc, small_prob, gpu_ok):
    """small_prob with exact observations of x_true, started from x0 moved by a similarity (3 % scale, ~2 degrees, 0.06
    units).  Point priors at the true positions of 4 points in general position (sigma = 1e-3) bring the solve back to the true
    frame: the RMS of ALL points against x_true is within 3 sigma; without priors the solve stays in the moved frame.  The
    numpy LM loop of the same controller is held to the same two statements first."""
    p = dict(small_prob)
    npnts, np3, sigma = p["npnts"], 3 * p["npnts"], 1e-3
    xt = p["x_true"]
    p["pt2d"] = p["pt2d"] + residual(orc, p, xt)  # r = projection - pt2d: the observations of x_true, exactly
    assert np.max(np.abs(residual(orc, p, xt))) < 1e-9
    Q = Rotation.from_rotvec([0.02, -0.03, 0.01]).as_matrix()
    x_start = _similarity(p["x0"], npnts, 1.03, Q, np.array([0.05, -0.02, 0.03]))
    r0, r1 = residual(orc, p, p["x0"]), residual(orc, p, x_start)
    assert abs(r0 @ r0 - r1 @ r1) <= 1e-9 * (r0 @ r0)  # the similarity changes no reprojection
    idx = np.array([1, 101, 201, 301])
    Xc = xt[:np3].reshape(-1, 3)[idx - 1]
    assert np.linalg.matrix_rank(Xc[1:] - Xc[0], tol=1e-2) == 3  # not collinear, not even coplanar
    pri = dict(point_priors=(idx, Xc, np.full((len(idx), 3), sigma)))

    def rms(x):
        return float(np.sqrt(np.mean(np.sum((x[:np3] - xt[:np3]).reshape(-1, 3) ** 2, axis=1))))

    def fun(pri_):
        def f(x):
            r, J = residual(orc, p, x), jac(orc, p, x).toarray()
            rows = pr.rows(x, p["ncams"], npnts, **pri_)
            Ap, gp = pr.normal_terms(rows, len(x))
            return (0.5 * (r @ r) + pr.cost(rows), J.T @ r + gp, J.T @ J + Ap,
                    lambda d: 0.5 * np.sum((J @ d + r) ** 2) + pr.model(rows, d))
        return f

    ref_with, ref_without = rms(lm_dense(fun(pri), x_start)[0]), rms(lm_dense(fun({}), x_start)[0])
    print(f"control points, numpy LM: rms with priors {ref_with:.3e}, without {ref_without:.3e}")
    assert ref_with <= 3 * sigma < 10 * sigma < ref_without
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, x=x_start, **pri)
        st0 = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, x=x_start)
    finally:
        m.close()
    got_with, got_without = rms(st.solution), rms(st0.solution)
    print(f"control points, device: rms with priors {got_with:.3e} ({st.status}, {st.iter}), without {got_without:.3e}")
    parity_record("prior_control_points", rms_with=got_with, rms_without=got_without, numpy_with=ref_with,
                  numpy_without=ref_without, iter=st.iter, status=st.status)
    assert got_with <= 3 * sigma, got_with
    assert got_without > 10 * sigma, got_without


@pytest.mark.gpu
def test_refused_combinations_on_the_device(ba, small_prob, gpu_ok):
    """Line search, Float32 model, Float16 and a communicator: ValueError / BA_ERR_ARG with the documented text, from the
    Python layer and from ba_lm_solve / ba_lm_step themselves; the handle is usable afterwards."""
    p = small_prob
    pri = _prior_set(p)
    lib = ba._lib.lib()
    m = ba.BALNLPModel(arrays=arrays(p))
    m32 = ba.BALNLPModel(arrays=arrays(p), T=np.float32)
    try:
        before = ba.lm_step(m, p["x0"], 1.0, **pri)
        nls = ba.FeasibilityResidual(m)
        with pytest.raises(ValueError, match="linesearch"):
            ba.Levenberg_Marquardt(nls, "LDL", "AMD", "None", True, **pri)
        with pytest.raises(ValueError, match="Float16"):
            ba.Levenberg_Marquardt(nls, "LDL", "AMD", "None", False, facto_type=np.float16, **pri)
        with pytest.raises(ValueError, match="Float32 model"):
            ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), "LDL", "AMD", "None", False, **pri)
        # the library itself (the priors are on the handle from the step above)
        assert ba._lib.get_priors(m.handle) == (40, 3, 4)
        x = np.array(p["x0"])
        for field, text in (("linesearch", "linesearch = true"), ("x_f32", "Float32 model"), ("facto_type", "Float16")):
            o = lm_opts(ba, **{field: 2 if field == "facto_type" else 1})
            st = ba._lib.LMStats()
            rc = lib.ba_lm_solve(m.handle, C.byref(o), ba._lib.ptr(x), C.byref(st), C.cast(None, ba._lib.LOG_CB), None)
            msg = lib.ba_last_error().decode()
            assert rc == 1 and "priors" in msg and text in msg, (field, rc, msg)
        assert np.array_equal(x, p["x0"])
        after = ba.lm_step(m, p["x0"], 1.0, **pri)
        assert not bits_report(after[0], before[0], "step after the refusals")
        assert _solve(ba, m, 1, "LDL", "None", **pri).status in ("first_order", "small_step")
        # a communicator (attached before the handle's first solve, as documented)
        mc = ba.BALNLPModel(arrays=arrays(p))
        with loopback_world(1, 16 << 20) as (L, loop):
            try:
                attach_loopback(ba, mc, L, loop, 0, 1)
                with pytest.raises(ba.BAArgError, match="priors.*communicator"):
                    ba.lm_step(mc, p["x0"], 1.0, **pri)
                with pytest.raises(ba.BAArgError, match="priors.*communicator"):
                    ba.lm_step(mc, p["x0"], 1.0, pcg=(1e-8, 100), **pri)
                with pytest.raises(ba.BAArgError, match="priors.*communicator"):
                    _solve(ba, mc, 1, "LDL", "None", **pri)
                plain = ba.lm_step(mc, p["x0"], 1.0)  # without priors the handle still steps
                assert np.all(np.isfinite(plain[0])) and rel_err(plain[0], before[0]) > 1e-6
            finally:
                mc.close()
    finally:
        m.close()
        m32.close()
