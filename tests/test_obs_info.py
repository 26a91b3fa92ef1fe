"""Per-observation 2 x 2 information matrices of the LM solve (ba_lm_set_obs_info, include/ba_hip.h): observation i
counts with Lambda_i = L_i L_i', the LM entries run on r^_i = L_i' r_i and J^_i = L_i' J_i.  The references are numpy
(tests/_lm_ref.py): the oracle's residual and Jacobian whitened there, the dense solve of the normal equations.  Every
limit is one the other term tests use (tests/_lm_ref.py: STEP_TOL, F32_TOL, PCG_TOL through limit(), check_cov; the figures of
test_prior_step_vs_dense_numpy, test_robust_eval_weights_and_cost and test_robust_solve).  The first tests need no device; the
rest run on the GPU.  small_prob has 1800 observations = 7 tiles of 256 and a tail of 8."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_ref import (F32_TOL, PCG_TOL, STEP_TOL, check_cov, factor, hessian, kappa_jacobi, limit, linearise, ref_dense, residual,
                     schur, step, weights_cost, whiten_residual, whitener)
from _lm_run import arrays, attach_loopback, env, fixed_vector, gauge_kw, lm_opts, loopback_world, solve
from _util import bits_report, parity_record, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from scenes import blocks, clip_psd, full_rank_per_point, random_info  # noqa: E402

NAMES = ("ba_lm_set_obs_info", "ba_lm_get_obs_info")
NOBS = 7


def _unpack(ref):
    """(delta, model, gradient, kappa of the Jacobi-scaled damped S) of _lm_ref.step's record"""
    return ref["delta"], ref["model"], ref["grad"], ref["kappa"]


def _identity(p):
    return np.broadcast_to(np.eye(2), (p["nobs"], 2, 2)).copy()


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_keywords(ba):
    L = ba._lib.lib()
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in NAMES:
        assert name in ba._lib.SYMBOLS and hasattr(L, name)
        assert f"int {name}(" in header
    assert L.ba_lm_set_obs_info(None, None) == 1
    assert L.ba_lm_get_obs_info(None, None, None) == 1
    with pytest.raises(ba.BAArgError, match="null handle"):
        ba._lib.check(L.ba_lm_set_obs_info(None, None))
    assert "obs_info" in ba.Levenberg_Marquardt.__kwdefaults__ and "obs_info" in ba.covariance.__kwdefaults__
    assert "obs_info" in ba.lm_step.__code__.co_varnames and "obs_info" in ba.BALNLPModel.robust_weights.__code__.co_varnames


_ASYM = np.broadcast_to(np.array([[1.0, 0.5], [0.25, 1.0]]), (NOBS, 2, 2))
_NOT_PSD = np.broadcast_to(np.array([[1.0, 2.0], [2.0, 1.0]]), (NOBS, 2, 2))
_BAD = [np.ones((NOBS, 3)), np.ones((NOBS, 2, 3)), np.ones((NOBS, 2, 2, 1)), np.float64(1.0), np.zeros(NOBS), -np.ones(NOBS),
        np.full(NOBS, np.nan), np.array([[1.0, 0.0]] * NOBS), np.array([[1.0, -2.0]] * NOBS), _ASYM, _NOT_PSD,
        -_identity({"nobs": NOBS}), np.full((NOBS, 2, 2), np.inf), "sigma"]


@pytest.mark.parametrize("bad", _BAD, ids=[str(k) for k in range(len(_BAD))])
def test_bad_obs_info_refused_before_the_model(ba, bad):
    """No model exists here (None): the ValueError comes before anything looks at the model or the device."""
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, obs_info=bad)
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", obs_info=bad)
    with pytest.raises(ValueError):
        ba.lm_step(None, np.zeros(3), 1.0, obs_info=bad)
    with pytest.raises(ValueError):
        ba.covariance(None, np.zeros(3), obs_info=bad)
    with pytest.raises(ValueError):
        ba.BALNLPModel.robust_weights(None, np.zeros(3), "huber", 1.0, obs_info=bad)


def test_refused_and_accepted_combinations_before_the_model(ba):
    sig = np.ones(NOBS)
    with pytest.raises(ValueError, match="obs_info.*linesearch"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", True, obs_info=sig)
    with pytest.raises(ValueError, match="obs_info.*Float16"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, facto_type=np.float16, obs_info=sig)
    with pytest.raises(ValueError, match="obs_info.*Float32 model"):
        ba._lib.ProblemTerms(obs_info=sig).refuse(xf32=True)
    for kw in (dict(normalize="J"), dict(normalize=":A"), dict(facto_type=np.float32), dict(loss="huber")):
        args = ("LDL", "AMD", kw.pop("normalize", "None"), False)
        with pytest.raises(TypeError, match="model must be"):
            ba.Levenberg_Marquardt(None, *args, obs_info=sig, **kw)
    with pytest.raises((AttributeError, TypeError)):  # accepted with the step's Float32 factor: fails on the first look at the model
        ba.lm_step(None, np.zeros(3), 1.0, facto_type=np.float32, obs_info=sig)
    assert ba._lib.ProblemTerms(obs_info=sig).weighted and not ba._lib.ProblemTerms().weighted


def test_obs_info_forms_pack_to_the_c_layout(ba):
    pack = ba._lib.obs_info_pack
    sig = np.array([0.5, 1.0, 2.0, 4.0, np.inf, 1.0, 3.0])
    want = np.stack([1.0 / sig ** 2, np.zeros(NOBS), 1.0 / sig ** 2], axis=1)
    full = np.zeros((NOBS, 2, 2))
    full[:, 0, 0] = full[:, 1, 1] = 1.0 / sig ** 2
    for form in (sig, np.stack([sig, sig], axis=1), full):
        got = pack(form, NOBS)
        assert got.shape == (NOBS, 3) and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, want)
    assert np.all(pack(sig)[4] == 0.0)  # sigma = inf: information 0
    assert np.array_equal(pack(np.array([[2.0, np.inf]] * NOBS))[0], [0.25, 0.0, 0.0])
    blk = np.array([[[4.0, -1.5], [-1.5, 1.0]]] * NOBS)
    assert np.array_equal(pack(blk, NOBS), np.array([[4.0, -1.5, 1.0]] * NOBS))  # a full block round-trips
    assert pack(None) is None and pack(None, NOBS) is None
    with pytest.raises(ValueError, match="obs_info"):
        pack(sig, NOBS + 1)
    assert np.array_equal(pack(_identity({"nobs": NOBS})), np.array([[1.0, 0.0, 1.0]] * NOBS))


def test_seeded_array_packs_and_the_reference_factors_it(ba, small_prob):
    """The seeded array of the device tests (zero and rank-one blocks included) passes the package's checks and packs to its
    xx xy yy, and the reference's factor of it holds: L L' = Lambda to rounding, r^' r^ = r' Lambda r, every point keeps two
    full-rank observations."""
    p = small_prob
    info = random_info(p, 3)
    packed = ba._lib.obs_info_pack(info, p["nobs"])
    assert np.array_equal(packed, np.stack([info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]], axis=1))
    assert ba._lib.ProblemTerms(obs_info=info).weighted
    l00, l10, l11 = factor(info)
    back = np.stack([l00 * l00, l00 * l10, l10 * l10 + l11 * l11], axis=1)
    want = np.stack([info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]], axis=1)
    assert np.max(np.abs(back - want)) <= 4 * np.finfo(float).eps * np.max(want)
    zero = np.all(info.reshape(-1, 4) == 0.0, axis=1)
    assert 0.02 * p["nobs"] < zero.sum() < 0.08 * p["nobs"]
    assert full_rank_per_point(p, info) >= 2
    r = np.random.default_rng(0).standard_normal(2 * p["nobs"])
    rh = whiten_residual(r, info)
    quad = np.einsum("ni,nij,nj->n", r.reshape(-1, 2), info, r.reshape(-1, 2))
    assert np.max(np.abs(rh[0::2] ** 2 + rh[1::2] ** 2 - quad)) <= 1e-13 * np.max(quad)
    assert np.array_equal(whitener(info) @ r, rh)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c_abi_refuses_bad_arrays_and_keeps_the_handle(ba, small_prob, gpu_ok):
    p = small_prob
    L = ba._lib.lib()
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        assert ba._lib.get_obs_info(m.handle) == (0, 0)
        good = np.tile([1.0, 0.0, 1.0], (p["nobs"], 1))
        good[5] = 0.0
        ba._lib.set_obs_info(m.handle, good)
        assert ba._lib.get_obs_info(m.handle) == (p["nobs"], 1)
        for row, text in (([np.nan, 0, 1], "finite"), ([1, np.inf, 1], "finite"), ([-1.0, 0, 1], "negative"), ([1, 0, -1.0], "negative"),
                          ([1.0, 1.5, 1.0], "semi-definite")):
            bad = good.copy()
            bad[p["nobs"] - 1] = row
            assert L.ba_lm_set_obs_info(m.handle, ba._lib.ptr(bad)) == 1 and text in L.ba_last_error().decode(), row
            assert ba._lib.get_obs_info(m.handle) == (p["nobs"], 1)
        rank1 = good.copy()
        rank1[7] = [1.0, 1.0, 1.0]
        assert L.ba_lm_set_obs_info(m.handle, ba._lib.ptr(rank1)) == 0  # rank one: valid
        ba._lib.set_obs_info(m.handle, np.tile([1.0, 0.0, 1.0], (p["nobs"], 1)))
        assert ba._lib.get_obs_info(m.handle) == (p["nobs"], 0)  # identities are kept as given, not collapsed to "cleared"
        ba._lib.set_obs_info(m.handle, None)
        assert ba._lib.get_obs_info(m.handle) == (0, 0)
    finally:
        m.close()


@pytest.mark.gpu
def test_identity_gives_the_plain_bits(ba, orc, small_prob, gpu_ok):
    """Lambda = I everywhere.  lm_step and a 5-iteration solve give the bits of the run without the keyword (multiplying by
    1.0 is exact, a zero l10 adds nothing), and so do lm_step and robust_weights under every robust loss: one pass (k_obs_scale)
    applies the loss with and without information, in the same arithmetic.  The huber step is also held to numpy at the
    project's limit of the step."""
    p = small_prob
    eye = _identity(p)
    m, plain = ba.BALNLPModel(arrays=arrays(p)), ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam in (30.0, 1e-2):
            a, b = ba.lm_step(m, p["x0"], lam, obs_info=eye), ba.lm_step(plain, p["x0"], lam)
            for got, want, name in zip(a, b, ("delta", "half_sq_model", "jtr")):
                rep = bits_report(np.atleast_1d(got), np.atleast_1d(want), f"{name} at lambda {lam:g}: Lambda = I vs no obs_info")
                assert not rep, rep
        assert ba._lib.get_obs_info(m.handle) == (p["nobs"], 0) and ba._lib.get_obs_info(plain.handle) == (0, 0)
        for variant in (1, 0):
            s1 = solve(ba, m, variant, ite_max=5, obs_info=np.ones(p["nobs"]))
            s2 = solve(ba, plain, variant, ite_max=5)
            rep = bits_report(s1.solution, s2.solution, f"variant {variant}: 5 iterations with sigma = 1 vs no obs_info")
            assert not rep, rep
            assert s1.log == s2.log and s1.objective == s2.objective
        for loss in ("huber", "soft_l1", "cauchy", "arctan"):
            for lam in (30.0, 1e-2):
                a = ba.lm_step(m, p["x0"], lam, loss=loss, f_scale=1.0, obs_info=eye)
                b = ba.lm_step(plain, p["x0"], lam, loss=loss, f_scale=1.0)
                for got, want, name in zip(a, b, ("delta", "half_sq_model", "jtr")):
                    rep = bits_report(np.atleast_1d(got), np.atleast_1d(want), f"{loss}, {name} at lambda {lam:g}: Lambda = I vs no obs_info")
                    assert not rep, rep
                if loss == "huber":
                    d_ref, _, _, kappa = _unpack(step(orc, p, p["x0"], lam, info=eye, loss="huber", c=1.0))
                    e, lim = rel_err(a[0], d_ref), limit(STEP_TOL[lam], kappa)
                    print(f"obs_info identity, huber, lambda {lam:g}: step vs numpy {e:.3e} (limit {lim:.1e})")
                    assert e <= lim
            (wa, fa), (wb, fb) = m.robust_weights(p["x0"], loss, 1.0, obs_info=eye), plain.robust_weights(p["x0"], loss, 1.0)
            rep = bits_report(wa, wb, f"{loss}: robust weights, Lambda = I vs no obs_info")
            assert not rep and fa == fb, (rep, fa, fb)
    finally:
        m.close()
        plain.close()


@pytest.mark.gpu
def test_scaling_by_four_is_a_quarter_of_the_damping(ba, orc, small_prob, gpu_ok):
    """Lambda = 4 I: (4 J'J + lambda I) d = -4 J'r is the plain system at lambda / 4; the model value and the gradient are 4
    times the plain ones."""
    p = small_prob
    four = 4.0 * _identity(p)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam in (30.0, 1.0, 1e-2):
            d, half, jtr = ba.lm_step(m, p["x0"], lam, obs_info=four)
            d0, half0, jtr0 = ba.lm_step(m, p["x0"], lam / 4)
            kappa = step(orc, p, p["x0"], lam / 4, info=_identity(p))["kappa"]
            e, lim = rel_err(d, d0), limit(STEP_TOL[lam], kappa)
            em, eg = abs(half - 4 * half0) / (4 * half0), rel_err(jtr, 4 * jtr0)
            print(f"obs_info 4 I, lambda {lam:g}: step {e:.3e} (limit {lim:.1e})  model {em:.3e}  jtr {eg:.3e}")
            assert e <= lim and em <= 1e-10 and eg <= 1e-12
        d_sig = ba.lm_step(m, p["x0"], 1.0, obs_info=np.full(p["nobs"], 0.5))[0]  # sigma = 1/2 is the same array
        assert not bits_report(d_sig, ba.lm_step(m, p["x0"], 1.0, obs_info=four)[0], "sigma = 0.5 vs Lambda = 4 I")
    finally:
        m.close()


@pytest.mark.gpu
def test_zero_information_drops_the_observation(ba, orc, small_prob, gpu_ok):
    """Lambda_i = 0 on a random 10 % of the observations (every point keeps two): the step of a model built from the others."""
    p = small_prob
    rng = np.random.default_rng(17)
    pnt = p["pnt_idx1"] - 1
    spare = np.bincount(pnt, minlength=p["npnts"]) - 2
    drop = np.zeros(p["nobs"], dtype=bool)
    for o in rng.permutation(p["nobs"]):
        if drop.sum() < p["nobs"] // 10 and spare[pnt[o]] > 0:
            drop[o] = True
            spare[pnt[o]] -= 1
    assert drop.sum() == p["nobs"] // 10 and np.bincount(pnt[~drop], minlength=p["npnts"]).min() >= 2
    sig = np.where(drop, np.inf, 1.0)
    q = dict(p, cam_idx1=p["cam_idx1"][~drop], pnt_idx1=p["pnt_idx1"][~drop], pt2d=p["pt2d"][np.repeat(~drop, 2)],
             nobs=int((~drop).sum()))
    m, mq = ba.BALNLPModel(arrays=arrays(p)), ba.BALNLPModel(arrays=arrays(q))
    try:
        for lam in (30.0, 1.0, 1e-2):
            tol = STEP_TOL[lam]
            d, half, jtr = ba.lm_step(m, p["x0"], lam, obs_info=sig)
            dq, halfq, jtrq = ba.lm_step(mq, p["x0"], lam)
            kappa = step(orc, q, p["x0"], lam, info=_identity(q))["kappa"]
            e, lim = rel_err(d, dq), limit(tol, kappa)
            print(f"obs_info dropping, lambda {lam:g}: step {e:.3e} (limit {lim:.1e})")
            assert e <= lim and abs(half - halfq) <= 1e-10 * halfq and rel_err(jtr, jtrq) <= 1e-12
        assert ba._lib.get_obs_info(m.handle) == (p["nobs"], int(drop.sum()))
        w, f = m.robust_weights(p["x0"], "linear", 1.0, obs_info=sig)
        wq, fq = mq.robust_weights(p["x0"], "linear", 1.0)
        assert np.all(w == 1.0) and abs(f - fq) <= 1e-13 * fq
    finally:
        m.close()
        mq.close()


@pytest.mark.gpu
def test_step_vs_dense_numpy(ba, orc, small_prob, gpu_ok):
    """Anisotropic Lambda with zero and rank-one blocks, lambda in {30, 1, 1e-2}: :LDL, facto_type = Float32 and
    pcg = (1e-12, 5000) against the dense numpy solve, with the limits of test_prior_step_vs_dense_numpy."""
    p = small_prob
    info = random_info(p, 3)
    assert full_rank_per_point(p, info) >= 2
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam in (30.0, 1.0, 1e-2):
            tol = STEP_TOL[lam]
            d_ref, mod_ref, g_ref, kappa = _unpack(step(orc, p, p["x0"], lam, info=info))
            d, half, jtr = ba.lm_step(m, p["x0"], lam, obs_info=info)
            d32 = ba.lm_step(m, p["x0"], lam, facto_type=np.float32, obs_info=info)[0]
            dp, halfp, _, its = ba.lm_step(m, p["x0"], lam, pcg=(1e-12, 5000), obs_info=info)
            e, e32, ep = rel_err(d, d_ref), rel_err(d32, d_ref), rel_err(dp, d_ref)
            em = abs(half - mod_ref) / mod_ref
            eg = float(np.linalg.norm(jtr - g_ref) / np.linalg.norm(g_ref))
            lim, lim32, limp = limit(tol, kappa), limit(F32_TOL, kappa), limit(PCG_TOL, kappa)
            print(f"obs_info_step lambda {lam:g}: kappa {kappa:.3e}  LDL {e:.3e} (limit {lim:.1e})  f32 {e32:.3e} ({lim32:.1e})  "
                  f"pcg {ep:.3e} ({limp:.1e}, {its} its)  model {em:.3e}  jtr {eg:.3e}")
            parity_record(f"obs_info_step[{lam:g}]", kappa=kappa, ldl=e, ldl_limit=lim, f32=e32, f32_limit=lim32, pcg=ep,
                          pcg_limit=limp, model=em, jtr=eg, cg_iters=its)
            assert e <= lim, f"lambda {lam}: :LDL step {e:.3e} > {lim:.3e}"
            assert e32 <= lim32, f"lambda {lam}: Float32-factor step {e32:.3e} > {lim32:.3e}"
            assert ep <= limp, f"lambda {lam}: PCG step {ep:.3e} > {limp:.3e}"
            assert em <= 1e-10, f"lambda {lam}: model value {half!r} vs {mod_ref!r}"
            assert abs(halfp - mod_ref) <= 1e-7 * mod_ref
            assert eg <= 1e-12, f"lambda {lam}: gradient {eg:.3e}"
        assert rel_err(d, ba.lm_step(m, p["x0"], 1e-2)[0]) > 1e-6  # (the information changes the step)
    finally:
        m.close()


@pytest.mark.gpu
def test_step_with_mask_huber_and_point_prior(ba, orc, small_prob, gpu_ok):
    """Every term in one call: fixed parameters, a huber loss (on the Mahalanobis distance), a point prior and the information.
    Fixed entries of delta and jtr are exactly 0, the free part is numpy's."""
    p = small_prob
    info = random_info(p, 4)
    assert full_rank_per_point(p, info) >= 2
    comp = np.zeros((p["ncams"], 9), dtype=bool)
    comp[1, 6:] = True
    mask = dict(fixed_cameras=[6], fixed_points=[3, 50], fixed_camera_params=comp)
    fixed = fixed_vector(ba, p, mask)
    pidx = np.array([3, 40, 200])
    X = p["x_true"][:3 * p["npnts"]].reshape(-1, 3)
    pri = dict(point_priors=(pidx, X[pidx - 1] + 0.01, np.full((3, 3), 0.05)))
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam in (30.0, 1.0, 1e-2):
            d_ref, mod_ref, g_ref, kappa = _unpack(step(orc, p, p["x0"], lam, info=info, loss="huber", c=1.5, fixed=fixed, priors=pri))
            d, half, jtr = ba.lm_step(m, p["x0"], lam, loss="huber", f_scale=1.5, obs_info=info, **mask, **pri)
            assert np.all(d[fixed] == 0.0) and np.all(jtr[fixed] == 0.0)
            e, lim = rel_err(d, d_ref), limit(STEP_TOL[lam], kappa)
            em = abs(half - mod_ref) / mod_ref
            eg = float(np.linalg.norm(jtr - g_ref) / np.linalg.norm(g_ref))
            print(f"obs_info_step_all_terms lambda {lam:g}: kappa {kappa:.3e}  step {e:.3e} (limit {lim:.1e})  model {em:.3e}  jtr {eg:.3e}")
            parity_record(f"obs_info_step_all_terms[{lam:g}]", kappa=kappa, ldl=e, ldl_limit=lim, model=em, jtr=eg)
            assert e <= lim and em <= 1e-10 and eg <= 1e-12
        assert rel_err(d, step(orc, p, p["x0"], 1e-2, info=info, fixed=fixed, priors=pri)["delta"]) > 1e-6  # (the loss acts)
    finally:
        m.close()


@pytest.mark.gpu
def test_step_block_sparse_schedule(ba, orc, gpu_ok):
    """The scene and the switch of test_robust_step_block_sparse_schedule: the step on the block-sparse list schedule."""
    p = ba.synthetic.make_problem(300, 700, 3500, seed=5, locality=0.08)
    info = random_info(p, 5)
    assert full_rank_per_point(p, info) >= 2
    lam = 1.0

    def run():
        m = ba.BALNLPModel(arrays=arrays(p))
        try:
            return ba.lm_step(m, p["x0"], lam, obs_info=info), ba.schur_pattern(m)
        finally:
            m.close()

    (d, half, jtr), pat = env("BA_SPARSE_S", "1", run)
    assert pat[2], "the block-sparse list schedule was not used"
    d_ref, mod_ref, g_ref, kappa = _unpack(step(orc, p, p["x0"], lam, info=info))
    e, lim = rel_err(d, d_ref), limit(STEP_TOL[lam], kappa)
    print(f"obs_info_step_sparse: kappa {kappa:.3e}  step {e:.3e} (limit {lim:.1e})")
    parity_record("obs_info_step_sparse", kappa=kappa, step=e, limit=lim)
    assert e <= lim
    assert abs(half - mod_ref) <= 1e-10 * mod_ref
    assert np.linalg.norm(jtr - g_ref) <= 1e-12 * np.linalg.norm(g_ref)


def _check_eval(ba, m, x, info, losses, c, what):
    """ba_robust_eval with obs_info against numpy on the device's own residual, at the limits of
    test_robust_eval_weights_and_cost (1e-14 per weight, 1e-13 on the cost)"""
    r = m.cons(x)
    for loss in losses:
        w, f = m.robust_weights(x, loss, c, obs_info=info)
        w_ref, f_ref = weights_cost(r, loss, c, info)
        e, ef = float(np.max(np.abs(w - w_ref) / w_ref)), abs(f - f_ref) / f_ref
        print(f"{what}: {loss}, c = {c}: weights {e:.3e}, cost {ef:.3e}")
        parity_record(f"{what}[{loss}]", weights=e, cost=ef)
        assert e <= 1e-14, f"{what}, {loss}: weights, max relative error {e:.3e}"
        assert ef <= 1e-13, f"{what}, {loss}: cost {f!r} vs {f_ref!r}"
        if loss == "linear":
            assert np.all(w == 1.0)


@pytest.mark.gpu
def test_robust_eval_weights_and_cost_with_information(ba, small_prob, gpu_ok):
    """weights = rho'(r' Lambda r / c^2) and the cost, cauchy and the other losses; a call without the keyword is plain again"""
    p = small_prob
    info = random_info(p, 6)
    m, fresh = ba.BALNLPModel(arrays=arrays(p)), ba.BALNLPModel(arrays=arrays(p))
    try:
        _check_eval(ba, m, p["x0"], info, ("cauchy", "linear", "huber", "soft_l1", "arctan"), 2.0, "obs_info_eval")
        zero = np.all(info.reshape(-1, 4) == 0.0, axis=1)
        assert np.all(m.robust_weights(p["x0"], "cauchy", 2.0, obs_info=info)[0][zero] == 1.0)
        wa, fa = m.robust_weights(p["x0"], "cauchy", 2.0)
        wb, fb = fresh.robust_weights(p["x0"], "cauchy", 2.0)
        assert not bits_report(wa, wb, "robust weights after the information was cleared vs a fresh handle") and fa == fb
    finally:
        m.close()
        fresh.close()


@pytest.mark.gpu
def test_robust_eval_many_tiles(ba, small_prob, gpu_ok):
    """nobs = 1024 * 256 + 300: more tiles than workgroups, so the loop over tiles runs more than once per workgroup, with a
    tail.  145 copies of small_prob (their own cameras and points) and a 1444-observation scene behind them.  With information,
    and huber without it (the instantiation without information reuses its LDS factors across the trips of the loop too) at the
    limits of test_robust_eval_weights_and_cost; Lambda = I gives the bits of the run without information."""
    p, copies = small_prob, 145
    last = ba.synthetic.make_problem(12, 400, 1024 * 256 + 300 - copies * small_prob["nobs"], seed=12)
    parts = [p] * copies + [last]
    np3 = 3 * p["npnts"]
    q = dict(cam_idx1=np.concatenate([s["cam_idx1"] + 12 * k for k, s in enumerate(parts)]),
             pnt_idx1=np.concatenate([s["pnt_idx1"] + 400 * k for k, s in enumerate(parts)]),
             pt2d=np.concatenate([s["pt2d"] for s in parts]),
             x0=np.concatenate([s["x0"][:np3] for s in parts] + [s["x0"][np3:] for s in parts]),
             ncams=12 * len(parts), npnts=400 * len(parts), nobs=1024 * 256 + 300)
    assert len(q["cam_idx1"]) == q["nobs"] == 262444
    info = random_info(q, 7)
    m = ba.BALNLPModel(arrays=arrays(q))
    try:
        _check_eval(ba, m, q["x0"], info, ("linear", "huber"), 1.0, "obs_info_eval_many_tiles")
        w, f = m.robust_weights(q["x0"], "huber", 1.0)
        w_ref, f_ref = weights_cost(m.cons(q["x0"]), "huber", 1.0)
        e, ef = float(np.max(np.abs(w - w_ref) / w_ref)), abs(f - f_ref) / f_ref
        print(f"many tiles, huber without information: weights {e:.3e}, cost {ef:.3e}")
        assert e <= 1e-14 and ef <= 1e-13, (e, ef)
        wi, fi = m.robust_weights(q["x0"], "huber", 1.0, obs_info=_identity(q))
        rep = bits_report(wi, w, "many tiles, huber: robust weights, Lambda = I vs no obs_info")
        assert not rep and fi == f, (rep, fi, f)
    finally:
        m.close()


def _noisy(ba, orc, p, seed):
    """small_prob with exact observations of x_true plus heteroscedastic noise: sigma_i in {0.5, 1, 2, 4} px per observation"""
    rng = np.random.default_rng(seed)
    sig = rng.choice([0.5, 1.0, 2.0, 4.0], p["nobs"])
    q = dict(p)
    q["pt2d"] = p["pt2d"] + residual(orc, p, p["x_true"]) + np.repeat(sig, 2) * rng.standard_normal(2 * p["nobs"])
    return q, sig


@pytest.mark.gpu
@pytest.mark.parametrize("variant,facto,normalize", [(1, "LDL", "None"), (0, "LDL", "None"), (1, "PCG", "None"), (0, "PCG", "None"),
                                                     (1, "LDL", "J")])
def test_solve_with_heteroscedastic_noise(ba, orc, small_prob, gpu_ok, variant, facto, normalize):
    """A complete solve with obs_info = sigma: objective and gradient norm at the solution against numpy, the checks and limits
    of test_robust_solve (oatol = ortol = 0 as there).  Once with normalize = :J (the step entries have no such option), and
    there with anisotropic full blocks: sigma_i along a random direction, sigma_i / 2 across it."""
    p, sig = _noisy(ba, orc, small_prob, 21)
    info = blocks(sig, sig, np.zeros(p["nobs"]))
    if normalize == "J":
        sig = info = clip_psd(blocks(sig, 0.5 * sig, np.random.default_rng(22).uniform(0.0, np.pi, p["nobs"])))
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = solve(ba, m, variant, facto, normalize, obs_info=sig, oatol=0.0, ortol=0.0)
        st2 = solve(ba, m, variant, facto, normalize, obs_info=sig, oatol=0.0, ortol=0.0)
        plain = solve(ba, m, variant, facto, normalize, oatol=0.0, ortol=0.0)
    finally:
        m.close()
    f_acc = [row[1] for row in st.log if row[7]]
    assert len(f_acc) >= 2 and all(b < a for a, b in zip(f_acc, f_acc[1:])), f"accepted rows: f not strictly decreasing {f_acc}"
    rt, Jt, _, f_ref = linearise(orc, p, st.solution, info)
    g = np.linalg.norm(Jt.T @ rt)
    feas = st.dual_feas if variant == 1 else st.primal_feas
    ef, eg = abs(st.objective - f_ref) / f_ref, abs(feas - g) / g
    print(f"obs_info_solve[{variant}-{facto}-{normalize}]: status {st.status}, {st.iter} iterations, objective {ef:.3e}, gradient {eg:.3e}")
    parity_record(f"obs_info_solve[{variant}-{facto}-{normalize}]", objective=ef, dual_feas=eg, iter=st.iter, status=st.status)
    assert ef <= 1e-12, f"objective {st.objective!r} vs numpy {f_ref!r}"
    assert eg <= 1e-10, f"|J^'r^| {feas!r} vs numpy {g!r}"
    assert st.status in ("first_order", "small_step"), st.status
    rep = bits_report(st.solution, st2.solution, "two runs")
    assert not rep, rep
    assert st.log == st2.log
    # the weighted solution has the lower weighted objective, the plain one the lower plain objective
    assert f_ref < linearise(orc, p, plain.solution, info)[3]


@pytest.mark.gpu
def test_covariance_with_information(ba, orc, small_prob, gpu_ok):
    """The blocks of (J^_F' J^_F)^-1 against the dense inverse (check_cov); for Lambda = I / sigma^2 with one sigma they are
    sigma^2 times the blocks without information."""
    p = small_prob
    kw = gauge_kw(p)
    fixed = fixed_vector(ba, p, kw)
    info = random_info(p, 8)
    assert full_rank_per_point(p, info) >= 2
    sigma = 2.0
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cams, pts, piv = ba.covariance(m, p["x0"], 0.0, obs_info=info, **kw)
        cams_s, pts_s, _ = ba.covariance(m, p["x0"], 0.0, obs_info=np.full(p["nobs"], sigma), **kw)
        cams_0, pts_0, _ = ba.covariance(m, p["x0"], 0.0, **kw)
    finally:
        m.close()
    H = hessian(orc, p, p["x0"], 0.0, fixed, info=info)
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    check_cov("covariance_obs_info", cams, pts, ref_c, ref_p, kappa_jacobi(S), fixed, p, min_rel_pivot=piv)
    assert piv > 1e-10
    S0, _, _ = schur(hessian(orc, p, p["x0"], 0.0, fixed), p)  # (kappa of the plain system, for the scaling statement)
    check_cov("covariance_obs_info_one_sigma", cams_s, pts_s, sigma ** 2 * cams_0, sigma ** 2 * pts_0, kappa_jacobi(S0), fixed, p)


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [None, "0"])
def test_no_stale_recorded_sequence_with_information(ba, small_prob, gpu_ok, prefetch):
    """ONE handle solves without information, with array A, with array B, without: each solve gives the bits and the log of the
    same solve on a fresh handle -- a sequence recorded with or without information, or under one array, is never replayed
    under another setting."""
    p = small_prob
    seq = [None, random_info(p, 9), random_info(p, 10), None]

    def run():
        shared = ba.BALNLPModel(arrays=arrays(p))
        try:
            for k, info in enumerate(seq):
                s1 = solve(ba, shared, obs_info=info)
                fresh = ba.BALNLPModel(arrays=arrays(p))
                s2 = solve(ba, fresh, obs_info=info)
                fresh.close()
                rep = bits_report(s1.solution, s2.solution, f"solve {k}: reused handle vs fresh handle")
                assert not rep, rep
                assert s1.log == s2.log, f"solve {k}: log rows differ between the reused and a fresh handle"
                assert s1.n_accepted >= 2
        finally:
            shared.close()

    env("BA_LM_PREFETCH", prefetch, run)


@pytest.mark.gpu
def test_refused_combinations_at_the_c_entries(ba, small_prob, gpu_ok):
    """With information on the handle ba_lm_solve returns BA_ERR_ARG under linesearch, x_f32, facto_type = Float16 and on a
    handle with a communicator, the step entries on that handle; the message names the term and the condition, x stays
    untouched, and after clearing a plain step gives the bits from before."""
    p = small_prob
    lib = ba._lib.lib()
    info3 = ba._lib.obs_info_pack(random_info(p, 11), p["nobs"])
    no_cb = C.cast(None, ba._lib.LOG_CB)
    m, mc = ba.BALNLPModel(arrays=arrays(p)), ba.BALNLPModel(arrays=arrays(p))
    m32 = ba.BALNLPModel(arrays=arrays(p), T=np.float32)

    def c_solve(h, **kw):
        x, o, st = np.array(p["x0"]), lm_opts(ba, ite_max=1, **kw), ba._lib.LMStats()
        rc = lib.ba_lm_solve(h.handle, C.byref(o), ba._lib.ptr(x), C.byref(st), no_cb, None)
        return rc, lib.ba_last_error().decode(), x

    try:
        before = ba.lm_step(m, p["x0"], 1.0)
        ba._lib.set_obs_info(m.handle, info3)
        for kw, text in ((dict(linesearch=1), "linesearch = true"), (dict(x_f32=1), "Float32 model"), (dict(facto_type=2), "Float16")):
            rc, msg, x = c_solve(m, **kw)
            assert rc == 1 and "per-observation information" in msg and "ba_lm_set_obs_info" in msg and text in msg, (kw, rc, msg)
            assert np.array_equal(x, p["x0"]), "a refused solve changed x"
        for kw in (dict(facto_type=1), dict(normalize=1), dict(facto=2)):  # accepted
            rc, msg, _ = c_solve(m, **kw)
            assert rc == 0, (kw, msg)
        with pytest.raises(ValueError, match="obs_info.*Float32 model"):
            ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), "LDL", "AMD", "None", False, obs_info=np.ones(p["nobs"]))
        with loopback_world(1, 16 << 20) as (L, loop):
            try:
                attach_loopback(ba, mc, L, loop, 0, 1)  # before the handle's first solve, as documented
                ba._lib.set_obs_info(mc.handle, info3)
                rc, msg, x = c_solve(mc)
                assert rc == 1 and "per-observation information" in msg and "communicator" in msg, (rc, msg)
                assert np.array_equal(x, p["x0"])
                d, half, its = np.empty_like(p["x0"]), C.c_double(0), C.c_int(0)
                x0 = np.ascontiguousarray(p["x0"])
                for entry in ("ba_lm_step", "ba_lm_step_f32"):
                    assert getattr(lib, entry)(mc.handle, ba._lib.ptr(x0), 1.0, ba._lib.ptr(d), C.byref(half), None) == 1
                    msg = lib.ba_last_error().decode()
                    assert entry in msg and "per-observation information" in msg and "communicator" in msg, msg
                assert lib.ba_lm_step_pcg(mc.handle, ba._lib.ptr(x0), 1.0, 1e-8, 100, ba._lib.ptr(d), C.byref(half), None, C.byref(its)) == 1
                msg = lib.ba_last_error().decode()
                assert "ba_lm_step_pcg" in msg and "per-observation information" in msg and "communicator" in msg, msg
                ba._lib.set_obs_info(mc.handle, None)
                assert np.all(np.isfinite(ba.lm_step(mc, p["x0"], 1.0)[0]))  # without the array the handle steps
            finally:
                mc.close()
        ba._lib.set_obs_info(m.handle, None)
        after = ba.lm_step(m, p["x0"], 1.0)
        for a, b, name in zip(after, before, ("delta", "half_sq_model", "jtr")):
            rep = bits_report(np.atleast_1d(a), np.atleast_1d(b), f"{name} of a plain step after the refusals vs before them")
            assert not rep, rep
    finally:
        m.close()
        m32.close()


@pytest.mark.gpu
def test_profile_shows_the_pass_and_nothing_without_it(ba, small_prob, gpu_ok):
    """With information the class k_info_whiten appears (once per linearisation, once per trial step) and k_robust_scale does
    not, also under a loss; without it the classes and counts are those of a handle that never had any."""
    p = small_prob
    info = random_info(p, 12)

    def profile(m, **kw):
        m.profile(True)
        st = solve(ba, m, **kw)
        prof = {k: v[1] for k, v in m.profile_get().items() if v[1] > 0}
        m.profile(False)
        return st, prof

    m, fresh = ba.BALNLPModel(arrays=arrays(p)), ba.BALNLPModel(arrays=arrays(p))
    try:
        _, plain = profile(fresh)
        st, with_info = profile(m, obs_info=info)
        st_h, with_both = profile(m, obs_info=info, loss="huber")
        _, after = profile(m)
    finally:
        m.close()
        fresh.close()
    assert "k_info_whiten" not in plain and after == plain
    assert with_info["k_info_whiten"] == st.n_jacobian + st.n_factor, (with_info, st.n_jacobian, st.n_factor)
    assert with_both["k_info_whiten"] == st_h.n_jacobian + st_h.n_factor and "k_robust_scale" not in with_both
