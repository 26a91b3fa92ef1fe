"""Robust losses of the LM solve (ba_lm_set_loss, include/ba_hip.h): f(x) = 1/2 sum_i c^2 rho(|r_i|^2 / c^2) per observation,
rho one of scipy's linear / huber / soft_l1 / cauchy / arctan, the step in the first-order (IRLS) form r~ = sqrt(w) r,
J~ = sqrt(w) J, w = rho'(z).  The references are numpy: the oracle's residuals / jac_structure / jac_coord, a dense solve of
(J~'J~ + lambda I) delta = -J~'r~.  The first tests need no device (the Python layer refuses bad arguments before it makes a
device call); the rest run on the GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from _lm_ref import STEP_TOL, linearise, residual, step, weights_cost
from _lm_run import Ranks, arrays, env, loopback, solve  # noqa: F401 (loopback: a fixture)
from _util import bits_report, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import scenes  # noqa: E402

LOSSES = ("linear", "huber", "soft_l1", "cauchy", "arctan")


# ---- CPU: the Python layer refuses before any device call --------------------------------------------------------------------
@pytest.mark.parametrize("bad", [{"loss": "tukey"}, {"loss": ":welsch"}, {"loss": None}, {"loss": "huber", "f_scale": 0.0},
                                 {"loss": "huber", "f_scale": -1.0}, {"loss": "cauchy", "f_scale": float("nan")},
                                 {"loss": "cauchy", "f_scale": float("inf")}, {"loss": "linear", "f_scale": 0.0}])
def test_bad_loss_refused_before_the_device(ba, bad):
    """No model exists here (model=None / nlp=None): the ValueError comes before anything looks at the model or the device."""
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, **bad)
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", **bad)
    if bad["loss"] is not None:
        with pytest.raises(ValueError):
            ba.lm_step(None, np.zeros(3), 1.0, **bad)
        with pytest.raises(ValueError):
            ba.BALNLPModel.robust_weights(None, np.zeros(3), bad["loss"], bad.get("f_scale", 1.0))


@pytest.mark.parametrize("loss", ["huber", ":soft_l1", "cauchy", "arctan"])
def test_robust_loss_with_line_search_refused(ba, loss):
    with pytest.raises(ValueError, match="linesearch"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", True, loss=loss, f_scale=2.0)


def test_loss_names_and_c_abi_codes(ba):
    """scipy's names map to the BA_LOSS_* codes; the C entry refuses a null handle, an unknown kind and a bad scale with
    BA_ERR_ARG (host-side checks, no device), and the Python layer maps that code to ValueError."""
    assert ba.LOSSES == {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}
    assert ba._lib.loss_code(":huber", 2) == (1, 2.0)
    L = ba._lib.lib()
    for name in ("ba_lm_set_loss", "ba_lm_get_loss", "ba_robust_eval"):
        assert name in ba._lib.SYMBOLS and hasattr(L, name)
    assert L.ba_lm_set_loss(None, 1, 1.0) == 1
    assert L.ba_robust_eval(None, None, None, None) == 1
    with pytest.raises(ValueError, match="null handle"):
        ba._lib.check(L.ba_lm_set_loss(None, 1, 1.0))
    assert issubclass(ba.BAArgError, ba.BAError)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _small_forced(p, orc):
    """small_prob with observations 0..9 exactly on their projection (s = 0) and 10..14 moved ~1e6 px away"""
    q = dict(p)
    r = residual(orc, p, p["x0"])
    pt = p["pt2d"].copy()
    pt[:20] += r[:20]  # r = projection - pt2d
    pt[20:30] += np.array([1e6, -7e5, 3e5, 9e5, -1e6, 1e6, 2e5, -8e5, 6e5, 4e5])
    q["pt2d"] = pt
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("c", [0.5, 3.0])
def test_robust_eval_weights_and_cost(ba, orc, small_prob, gpu_ok, c):
    """ba_robust_eval against numpy for every loss.  The reference takes the device's own residual (which
    test_gpu_parity.py holds to the oracle's at its own limit): the comparison is of the loss pass, at 1e-14 per weight."""
    p = _small_forced(small_prob, orc)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        r = m.cons(p["x0"])
        r_orc = residual(orc, p, p["x0"])
        assert np.max(np.abs(r - r_orc) / (np.abs(p["pt2d"]) + np.abs(r_orc) + 1.0)) < 64 * 2.3e-16
        s = r[0::2] ** 2 + r[1::2] ** 2
        assert np.all(s[:10] < 1e-20) and np.all(s[10:15] > 1e10)
        for loss in LOSSES:
            w, f = m.robust_weights(p["x0"], loss, c)
            w_ref, f_ref = weights_cost(r, loss, c)
            e = np.max(np.abs(w - w_ref) / w_ref)
            assert e <= 1e-14, f"{loss}, c = {c}: weights, max relative error {e:.3e}"
            assert abs(f - f_ref) <= 1e-13 * f_ref, f"{loss}, c = {c}: cost {f!r} vs {f_ref!r}"
            if loss != "linear":
                assert np.all(w[10:15] < 1.0) and np.all(w[:10] == 1.0)
            # the oracle's residual: the same to its agreement with the device
            w2, f2 = weights_cost(r_orc, loss, c)
            assert abs(f - f2) <= 1e-12 * f2
        kind, scale = C.c_int(-1), C.c_double(0)
        ba._lib.check(ba._lib.lib().ba_lm_get_loss(m.handle, C.byref(kind), C.byref(scale)))
        assert (kind.value, scale.value) == (4, c)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 30, 100), (4, 70, 256), (6, 100, 512)], ids=["partial_tile", "one_tile", "two_tiles"])
def test_robust_eval_tile_shapes(ba, gpu_ok, shape):
    """The tile of 256 observations of k_obs_scale at its edges: one partial tile, exactly one full tile, two full tiles without
    a tail.  Every loss, against numpy on the device's own residual at the limits of test_robust_eval_weights_and_cost: without
    information, with a seeded array of information matrices, and with Lambda = I, which gives the bits of the run without
    information.  The partial tile also through lm_step under huber (the J side of the tile), Lambda = I against none by bits."""
    p = ba.synthetic.make_problem(*shape, seed=5)
    info, eye = scenes.random_info(p, 5), np.broadcast_to(np.eye(2), (p["nobs"], 2, 2)).copy()
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        r = m.cons(p["x0"])
        for loss in LOSSES:
            w, f = m.robust_weights(p["x0"], loss, 1.0)
            for what, (got_w, got_f), (w_ref, f_ref) in (
                    ("plain", (w, f), weights_cost(r, loss, 1.0)),
                    ("information", m.robust_weights(p["x0"], loss, 1.0, obs_info=info), weights_cost(r, loss, 1.0, info))):
                e, ef = float(np.max(np.abs(got_w - w_ref) / w_ref)), abs(got_f - f_ref) / f_ref
                print(f"nobs {p['nobs']}, {loss}, {what}: weights {e:.3e}, cost {ef:.3e}")
                assert e <= 1e-14, f"{loss}, {what}: weights, max relative error {e:.3e}"
                assert ef <= 1e-13, f"{loss}, {what}: cost {got_f!r} vs {f_ref!r}"
            wi, fi = m.robust_weights(p["x0"], loss, 1.0, obs_info=eye)
            rep = bits_report(wi, w, f"{loss}: robust weights, Lambda = I vs no obs_info")
            assert not rep and fi == f, (rep, fi, f)
        if p["nobs"] == 100:
            a = ba.lm_step(m, p["x0"], 30.0, loss="huber", f_scale=1.0, obs_info=eye)
            b = ba.lm_step(m, p["x0"], 30.0, loss="huber", f_scale=1.0)
            for got, want, name in zip(a, b, ("delta", "half_sq_model", "jtr")):
                rep = bits_report(np.atleast_1d(got), np.atleast_1d(want), f"huber, {name}: Lambda = I vs no obs_info")
                assert not rep, rep
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("loss,c", [("huber", 1.0), ("soft_l1", 2.0), ("cauchy", 1.5)])
def test_robust_step_vs_dense_numpy(ba, orc, small_prob, gpu_ok, loss, c):
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            d, half, jtr = ba.lm_step(m, p["x0"], lam, loss=loss, f_scale=c)
            ref = step(orc, p, p["x0"], lam, loss=loss, c=c)
            d_ref, half_ref, g_ref = ref["delta"], ref["model"], ref["grad"]
            e = rel_err(d, d_ref)
            assert e <= tol, f"{loss}, lambda {lam}: |d - d_ref| / |d_ref| = {e:.3e} (limit {tol:.0e})"
            assert abs(half - half_ref) <= 1e-9 * half_ref, f"{loss}, lambda {lam}: model {half!r} vs {half_ref!r}"
            assert np.max(np.abs(jtr - g_ref)) <= 1e-12 * np.max(np.abs(g_ref)), f"{loss}, lambda {lam}: J~'r~"
        lam = 1.0
        d_ref = step(orc, p, p["x0"], lam, loss=loss, c=c)["delta"]
        dp = ba.lm_step(m, p["x0"], lam, pcg=(1e-12, 5000), loss=loss, f_scale=c)[0]
        assert rel_err(dp, d_ref) <= 1e-8, f"{loss}: PCG step {rel_err(dp, d_ref):.3e}"
        d32 = ba.lm_step(m, p["x0"], lam, facto_type=np.float32, loss=loss, f_scale=c)[0]
        assert rel_err(d32, d_ref) <= 5e-3, f"{loss}: Float32-factor step {rel_err(d32, d_ref):.3e}"
        # a call without loss= is the plain step again: the bits of a handle that never saw a loss
        d_lin = ba.lm_step(m, p["x0"], lam)[0]
        fresh = ba.BALNLPModel(arrays=arrays(p))
        d_fresh = ba.lm_step(fresh, p["x0"], lam)[0]
        fresh.close()
        rep = bits_report(d_lin, d_fresh, "linear step after robust ones vs a fresh handle")
        assert not rep, rep
        assert rel_err(d_lin, d_ref) > 1e-6
    finally:
        m.close()


@pytest.mark.gpu
def test_robust_step_block_sparse_schedule(ba, orc, gpu_ok):
    """The block-sparse list schedule (BA_SPARSE_S=1) on a banded problem: the huber step of the dense numpy solve."""
    p = ba.synthetic.make_problem(300, 700, 3500, seed=5, locality=0.08)
    lam, c = 1.0, 1.0

    def run():
        m = ba.BALNLPModel(arrays=arrays(p))
        try:
            out = ba.lm_step(m, p["x0"], lam, loss="huber", f_scale=c)
            return out, ba.schur_pattern(m)
        finally:
            m.close()

    (d, half, jtr), pat = env("BA_SPARSE_S", "1", run)
    assert pat[2], "the block-sparse list schedule was not used"
    ref = step(orc, p, p["x0"], lam, loss="huber", c=c)
    d_ref, half_ref, g_ref = ref["delta"], ref["model"], ref["grad"]
    e = rel_err(d, d_ref)
    assert e <= 1e-10, f"block-sparse huber step: {e:.3e}"
    assert abs(half - half_ref) <= 1e-9 * half_ref
    assert np.max(np.abs(jtr - g_ref)) <= 1e-12 * np.max(np.abs(g_ref))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 0])
def test_linear_loss_changes_nothing(ba, small_prob, gpu_ok, variant):
    p = small_prob
    out = []
    for kw in ({}, {"loss": "linear"}, {"loss": ":linear", "f_scale": 3.0}):
        m = ba.BALNLPModel(arrays=arrays(p))
        out.append(solve(ba, m, variant, **kw))
        m.close()
    for st in out[1:]:
        rep = bits_report(out[0].solution, st.solution, f"variant {variant}: solution with loss = linear vs without loss=")
        assert not rep, rep
        assert st.log == out[0].log and st.iter == out[0].iter and st.objective == out[0].objective


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [None, "0"])
def test_no_stale_recorded_sequence(ba, small_prob, gpu_ok, prefetch):
    """ONE handle solves linear, huber (c = 1), huber (c = 3), cauchy, linear: each solve gives the bits of the same solve on
    a fresh handle -- a sequence recorded under one loss (recorded graphs, the prefetched trial step) is never replayed under
    another."""
    p = small_prob
    seq = [("linear", 1.0), ("huber", 1.0), ("huber", 3.0), ("cauchy", 2.0), ("linear", 1.0)]

    def run():
        shared = ba.BALNLPModel(arrays=arrays(p))
        try:
            for loss, c in seq:
                a = solve(ba, shared, loss=loss, f_scale=c)
                fresh = ba.BALNLPModel(arrays=arrays(p))
                b = solve(ba, fresh, loss=loss, f_scale=c)
                fresh.close()
                rep = bits_report(a.solution, b.solution, f"{loss} c = {c}: reused handle vs fresh handle")
                assert not rep, rep
                assert a.log == b.log, f"{loss} c = {c}: log rows differ between the reused and a fresh handle"
        finally:
            shared.close()

    env("BA_LM_PREFETCH", prefetch, run)


@pytest.mark.gpu
@pytest.mark.parametrize("loss,c,variant", [("huber", 1.0, 1), ("soft_l1", 1.0, 1), ("cauchy", 2.0, 1), ("arctan", 2.0, 1),
                                            ("huber", 1.0, 0), ("cauchy", 2.0, 0)])
def test_robust_solve(ba, orc, small_prob, gpu_ok, loss, c, variant):
    """Complete solves.  The reweighted (IRLS) step converges linearly, not quadratically: with the default ortol (cbrt(eps))
    the relative-objective-change test ends these runs first (status :acceptable -- a numpy run of the same controller stops
    there too), so it is switched off (oatol = ortol = 0) and the run must end on the first-order or the small-step test."""
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = solve(ba, m, variant, loss=loss, f_scale=c, oatol=0.0, ortol=0.0)
        st2 = solve(ba, m, variant, loss=loss, f_scale=c, oatol=0.0, ortol=0.0)
    finally:
        m.close()
    f_acc = [row[1] for row in st.log if row[7]]
    assert len(f_acc) >= 2 and all(b < a for a, b in zip(f_acc, f_acc[1:])), f"accepted rows: f not strictly decreasing {f_acc}"
    rt, Jt, _, f_ref = linearise(orc, p, st.solution, loss=loss, c=c)
    assert abs(st.objective - f_ref) <= 1e-12 * f_ref, f"objective {st.objective!r} vs numpy {f_ref!r}"
    g = np.linalg.norm(Jt.T @ rt)
    feas = st.dual_feas if variant == 1 else st.primal_feas
    assert abs(feas - g) <= 1e-10 * g, f"|J~'r~| {feas!r} vs numpy {g!r}"
    assert st.status in ("first_order", "small_step"), st.status
    rep = bits_report(st.solution, st2.solution, f"{loss}: two runs")
    assert not rep, rep
    assert st.log == st2.log


# ---- what the feature is for: outliers ----------------------------------------------------------------------------------
# shape of the problem and of its outliers (fixed seed): 5 % of the observations displaced by 30-100 px in random directions
OUTLIER_SHAPE = dict(ncams=30, npnts=2000, nobs=8000, seed=2024)


def _outlier_problem(ba):
    s = OUTLIER_SHAPE
    p = ba.synthetic.make_problem(s["ncams"], s["npnts"], s["nobs"], seed=s["seed"])  # image noise 0.5 px
    rng = np.random.default_rng(s["seed"] + 1)
    nout = int(round(0.05 * p["nobs"]))
    out = np.sort(rng.choice(p["nobs"], nout, replace=False))
    mag, ang = rng.uniform(30.0, 100.0, nout), rng.uniform(0.0, 2 * np.pi, nout)
    pt = p["pt2d"].copy()
    pt[2 * out] += mag * np.cos(ang)
    pt[2 * out + 1] += mag * np.sin(ang)
    q = dict(p, pt2d=pt)
    inl = np.ones(p["nobs"], dtype=bool)
    inl[out] = False
    clean = dict(p, cam_idx1=p["cam_idx1"][inl], pnt_idx1=p["pnt_idx1"][inl], pt2d=p["pt2d"].reshape(-1, 2)[inl].ravel(),
                 nobs=int(inl.sum()))
    return q, clean, inl


def _inlier_rms(orc, p, x, inl):
    r = residual(orc, p, x).reshape(-1, 2)[inl]
    return float(np.sqrt(np.mean(np.sum(r * r, axis=1))))


@pytest.mark.gpu
def test_robust_loss_resists_outliers(ba, orc, gpu_ok):
    """RMS reprojection error of the inlier observations (independent of the gauge) at the solution: cauchy at c = 2 px
    reaches the outlier-free linear solve's within 5 %; the linear loss is pulled 1.5 x or more away from it.  huber (and
    soft_l1: both keep a force of c per outlier, whatever its size) cannot reach 5 % on this scene -- its own minimum lies at
    5.3 x (a numpy IRLS run to the first-order test; the default stop here gives 4.8 x, the numpy run of the same controller
    4.8046 x as well): it is held to halving the linear loss's error."""
    q, clean, inl = _outlier_problem(ba)
    m = ba.BALNLPModel(arrays=arrays(clean))
    st = solve(ba, m)
    m.close()
    rms_clean = _inlier_rms(orc, q, st.solution, inl)
    got = {}
    for loss in ("linear", "huber", "cauchy"):
        m = ba.BALNLPModel(arrays=arrays(q))
        st = solve(ba, m, loss=loss, f_scale=2.0)
        m.close()
        got[loss] = _inlier_rms(orc, q, st.solution, inl)
    print(f"inlier RMS: clean {rms_clean:.4f} px; " + ", ".join(f"{k} {v:.4f} ({v / rms_clean:.3f} x)" for k, v in got.items()))
    assert got["cauchy"] <= 1.05 * rms_clean
    assert got["linear"] >= 1.5 * rms_clean
    assert got["huber"] <= 0.5 * got["linear"]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_loopback_huber_step_equals_one_rank(ba, loopback, world):
    """Observations sharded by point: every rank reweights its own observations, the robust partial sums ride the existing
    all-reduce of the scalars.  The huber step of the unsharded problem to 1e-9, the model value to 1e-10, the cost (the sum
    of the ranks' parts) to 1e-12; the camera step bit-identical on every rank."""
    prob = ba.synthetic.make_problem(200, 1500, 9000, seed=11)
    lam, c = 10.0, 1.0
    ref = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(prob))
    d_ref, half_ref, _ = ba.lm_step(ref, prob["x0"], lam, loss="huber", f_scale=c)
    _, f_ref = ref.robust_weights(prob["x0"], "huber", c)
    ref.close()
    R = Ranks(ba, loopback, prob, world)
    try:
        d, cams, half = R.step(lam, loss="huber", f_scale=c)
        e = rel_err(d, d_ref)
        assert e <= 1e-9, f"{world} ranks: |delta - delta_one_rank| / |delta_one_rank| = {e:.3e}"
        assert abs(half - half_ref) <= 1e-10 * half_ref, f"{world} ranks: model value {half!r} vs {half_ref!r}"
        for r in range(1, world):
            rep = bits_report(cams[0], cams[r], f"huber camera step of rank 0 vs rank {r}")
            assert not rep, rep
        f = math.fsum(m.robust_weights(R.shards[r][0][3], "huber", c)[1] for r, m in enumerate(R.models))
        assert abs(f - f_ref) <= 1e-12 * f_ref, f"{world} ranks: cost {f!r} vs {f_ref!r}"
    finally:
        R.close()
