"""Fixed parameters of the LM solve (ba_lm_set_fixed, include/ba_hip.h): points fixed as a whole, camera components by a
9-bit mask (r1 r2 r3 t1 t2 t3 k1 k2 f).  The solve runs over the free entries only: the columns of the fixed parameters are
zeroed in J after every evaluation.  The references are numpy (the oracle's residuals / jac_structure / jac_coord, a dense
solve of (J_F'J_F + lambda I) delta_F = -J_F'r over the free columns) and scipy's least_squares on the free variables.  The
first tests need no device (the Python layer refuses bad arguments before it makes a device call); the rest run on the GPU."""
import ctypes as C
import threading

import numpy as np
import pytest

from _lm_ref import STEP_TOL, jac, residual, step
from _lm_run import arrays, attach_loopback, env, fixed_vector, gauge_kw, lm_opts, loopback_world, solve
from _util import bits_report, parity_record, rel_err

INTRINSICS = ("k1", "k2", "f")


def _step_masks(p):
    """the three masks of the step tests: intrinsics of every camera; camera 1 whole plus 20 % of the points; random
    per-camera components"""
    rng = np.random.default_rng(3)
    pts = np.sort(rng.choice(p["npnts"], p["npnts"] // 5, replace=False)) + 1
    comp = rng.random((p["ncams"], 9)) < 0.3
    return {"intrinsics": dict(fixed_camera_params=INTRINSICS),
            "cam1+20%pts": dict(fixed_cameras=[1], fixed_points=pts),
            "random components": dict(fixed_camera_params=comp)}


# ---- CPU: host masks and the refusals before any device call ----------------------------------------------------------------
def test_fixed_masks_bit_patterns(ba):
    fm = ba._lib.fixed_masks
    cam, pnt = fm(3, 5)
    assert cam.dtype == np.uint16 and pnt.dtype == np.uint8 and not cam.any() and not pnt.any()
    cam, pnt = fm(3, 5, fixed_cameras=[2], fixed_points=[1, 5])
    assert cam.tolist() == [0, 0x1FF, 0] and pnt.tolist() == [1, 0, 0, 0, 1]
    cam, pnt = fm(3, 5, fixed_cameras=np.array([True, False, True]), fixed_points=np.array([False, True, False, False, False]))
    assert cam.tolist() == [0x1FF, 0, 0x1FF] and pnt.tolist() == [0, 1, 0, 0, 0]
    for names, bits in ((("r",), 0x007), (("t",), 0x038), (("k1",), 0x040), (("k2",), 0x080), (("f",), 0x100),
                        (INTRINSICS, 0x1C0), (("r", "t"), 0x03F), ("f", 0x100), ((), 0)):
        assert fm(2, 1, fixed_camera_params=names)[0].tolist() == [bits, bits], names
    comp = np.zeros((3, 9), dtype=bool)
    comp[0, 0] = comp[1, 8] = comp[2, 3] = comp[2, 4] = True
    assert fm(3, 1, fixed_camera_params=comp)[0].tolist() == [0x001, 0x100, 0x018]
    # the options are OR-ed
    cam, _ = fm(3, 1, fixed_cameras=[3], fixed_camera_params=comp)
    assert cam.tolist() == [0x001, 0x100, 0x1FF]
    cam, _ = fm(3, 1, fixed_camera_params=("k1",), fixed_cameras=np.array([False, True, False]))
    assert cam.tolist() == [0x040, 0x1FF, 0x040]
    # empty index lists fix nothing
    cam, pnt = fm(3, 5, fixed_cameras=[], fixed_points=np.array([], dtype=np.int64), fixed_camera_params=())
    assert not cam.any() and not pnt.any()
    assert ba._lib.CAMERA_PARAMS == {"r": 0x007, "t": 0x038, "k1": 0x040, "k2": 0x080, "f": 0x100}


def test_shard_point_mask(ba):
    info = {"point_range": (3, 7), "npnts_global": 10}
    assert ba.parallel.shard_fixed_points([1, 4, 7, 8, 10], info).tolist() == [True, False, False, True]
    glob = np.zeros(10, dtype=bool)
    glob[[3, 6]] = True
    assert ba.parallel.shard_fixed_points(glob, info).tolist() == [True, False, False, True]


_BAD_SIZED = [dict(fixed_cameras=[0]), dict(fixed_cameras=[4]), dict(fixed_points=[0]), dict(fixed_points=[6]),
              dict(fixed_points=[-1]), dict(fixed_cameras=np.ones(2, dtype=bool)), dict(fixed_points=np.ones(6, dtype=bool)),
              dict(fixed_camera_params=np.ones((3, 8), dtype=bool)), dict(fixed_camera_params=np.ones((2, 9), dtype=bool)),
              dict(fixed_camera_params=("k3",)), dict(fixed_camera_params=("R",)), dict(fixed_points=[1.0]),
              dict(fixed_points=[[1, 2]])]


@pytest.mark.parametrize("bad", _BAD_SIZED)
def test_bad_fixed_masks_refused(ba, bad):
    with pytest.raises(ValueError):
        ba._lib.fixed_masks(3, 5, bad.get("fixed_cameras"), bad.get("fixed_points"), bad.get("fixed_camera_params"))


@pytest.mark.parametrize("bad", [dict(fixed_cameras=[0]), dict(fixed_points=[0, 3]), dict(fixed_points=[-2]),
                                 dict(fixed_camera_params=("k3",)), dict(fixed_camera_params=("k1", "focal")),
                                 dict(fixed_camera_params=np.ones((3, 8), dtype=bool)),
                                 dict(fixed_cameras=np.ones((2, 2), dtype=bool)), dict(fixed_points=[0.5]),
                                 dict(fixed_cameras=[1], facto_type=np.float16),
                                 dict(fixed_camera_params=INTRINSICS, facto_type=np.float16)])
def test_bad_fixed_refused_before_the_device(ba, bad):
    """No model exists here (model=None / nlp=None): the ValueError comes before anything looks at the model or the device."""
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, **bad)
    if "facto_type" not in bad:
        with pytest.raises(ValueError):
            ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", **bad)
        with pytest.raises(ValueError):
            ba.lm_step(None, np.zeros(3), 1.0, **bad)


def test_fixed_c_abi_host_checks(ba):
    L = ba._lib.lib()
    for name in ("ba_lm_set_fixed", "ba_lm_get_fixed"):
        assert name in ba._lib.SYMBOLS and hasattr(L, name)
    assert L.ba_lm_set_fixed(None, None, None) == 1
    assert L.ba_lm_get_fixed(None, None, None) == 1
    with pytest.raises(ba.BAArgError, match="null handle"):
        ba._lib.check(L.ba_lm_set_fixed(None, None, None))


# ---- GPU: the step ---------------------------------------------------------------------------------------------------------
def _check_step(ba, orc, m, p, lam, kw, tol, fixed, what, loss=None, c=1.0):
    """against _lm_ref.step: delta and J_F'r with zeros on the fixed entries, 1/2 |J_F delta_F + r|^2, of the dense solve over
    the free columns"""
    d, half, jtr = ba.lm_step(m, p["x0"], lam, **kw, **({"loss": loss, "f_scale": c} if loss else {}))
    ref = step(orc, p, p["x0"], lam, fixed=fixed, loss=loss or "linear", c=c)
    d_ref, half_ref, g_ref = ref["delta"], ref["model"], ref["grad"]
    assert np.all(d[fixed] == 0.0), f"{what}, lambda {lam}: {np.count_nonzero(d[fixed])} fixed entries of delta are not 0"
    assert np.all(jtr[fixed] == 0.0), f"{what}, lambda {lam}: fixed entries of J'r are not 0"
    e = rel_err(d, d_ref)
    assert e <= tol, f"{what}, lambda {lam}: |d - d_ref| / |d_ref| = {e:.3e} (limit {tol:.0e})"
    assert abs(half - half_ref) <= 1e-9 * half_ref, f"{what}, lambda {lam}: model {half!r} vs {half_ref!r}"
    eg = np.max(np.abs(jtr - g_ref)) / np.max(np.abs(g_ref))
    assert eg <= 1e-12, f"{what}, lambda {lam}: J_F'r {eg:.3e}"
    return e, d_ref


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ["intrinsics", "cam1+20%pts", "random components"])
def test_fixed_step_vs_dense_numpy(ba, orc, small_prob, gpu_ok, mask):
    p = small_prob
    kw = _step_masks(p)[mask]
    fixed = fixed_vector(ba, p, kw)
    assert 0 < fixed.sum() < len(fixed)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        worst = 0.0
        for lam, tol in STEP_TOL.items():
            e, _ = _check_step(ba, orc, m, p, lam, kw, tol, fixed, mask)
            worst = max(worst, e / tol)
        assert ba._lib.get_fixed(m.handle) == (int(fixed[3 * p["npnts"]:].sum()), int(fixed[:3 * p["npnts"]].sum()) // 3)
        lam = 1.0
        d_ref = step(orc, p, p["x0"], lam, fixed=fixed)["delta"]
        dp = ba.lm_step(m, p["x0"], lam, pcg=(1e-12, 5000), **kw)[0]
        assert np.all(dp[fixed] == 0.0), f"{mask}: PCG step, fixed entries"
        ep = rel_err(dp, d_ref)
        assert ep <= 1e-8, f"{mask}: PCG step {ep:.3e}"
        d32 = ba.lm_step(m, p["x0"], lam, facto_type=np.float32, **kw)[0]
        assert np.all(d32[fixed] == 0.0), f"{mask}: Float32-factor step, fixed entries"
        e32 = rel_err(d32, d_ref)
        assert e32 <= 5e-3, f"{mask}: Float32-factor step {e32:.3e}"
        parity_record(f"fixed_step[{mask}]", worst_over_limit=worst, pcg=ep, f32=e32)
        # a call without fixed_* is the plain step again: the bits of a handle that never saw a mask
        d_plain = ba.lm_step(m, p["x0"], lam)[0]
        fresh = ba.BALNLPModel(arrays=arrays(p))
        d_fresh = ba.lm_step(fresh, p["x0"], lam)[0]
        fresh.close()
        rep = bits_report(d_plain, d_fresh, "unmasked step after masked ones vs a fresh handle")
        assert not rep, rep
        assert ba._lib.get_fixed(m.handle) == (0, 0)
    finally:
        m.close()


@pytest.mark.gpu
def test_fixed_step_under_huber(ba, orc, small_prob, gpu_ok):
    p = small_prob
    kw = _step_masks(p)["cam1+20%pts"]
    fixed = fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            _check_step(ba, orc, m, p, lam, kw, tol, fixed, "huber", loss="huber", c=1.0)
    finally:
        m.close()


@pytest.mark.gpu
def test_fixed_step_block_sparse_schedule(ba, orc, gpu_ok):
    """BA_SPARSE_S=1 on a banded problem, whole cameras fixed inside the band (their rows of S hold only the damping)."""
    p = ba.synthetic.make_problem(300, 700, 3500, seed=5, locality=0.08)
    kw = dict(fixed_cameras=np.arange(100, 111), fixed_points=np.arange(1, 701, 7))
    fixed = fixed_vector(ba, p, kw)
    lam = 1.0

    def run():
        m = ba.BALNLPModel(arrays=arrays(p))
        try:
            return ba.lm_step(m, p["x0"], lam, **kw), ba.schur_pattern(m)
        finally:
            m.close()

    (d, half, jtr), pat = env("BA_SPARSE_S", "1", run)
    assert pat[2], "the block-sparse list schedule was not used"
    ref = step(orc, p, p["x0"], lam, fixed=fixed)
    d_ref, half_ref, g_ref = ref["delta"], ref["model"], ref["grad"]
    assert np.all(d[fixed] == 0.0) and np.all(jtr[fixed] == 0.0)
    e = rel_err(d, d_ref)
    assert e <= 1e-10, f"block-sparse masked step: {e:.3e}"
    assert abs(half - half_ref) <= 1e-9 * half_ref
    assert np.max(np.abs(jtr - g_ref)) <= 1e-12 * np.max(np.abs(g_ref))


@pytest.mark.gpu
def test_c_abi_refuses_bad_masks(ba, small_prob, gpu_ok):
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        L = ba._lib.lib()
        cam = np.zeros(p["ncams"], dtype=np.uint16)
        cam[3] = 1 << 9
        with pytest.raises(ba.BAArgError, match="bit above 8"):
            ba._lib.check(L.ba_lm_set_fixed(m.handle, ba._lib.ptr(cam), None))
        pnt = np.zeros(p["npnts"], dtype=np.uint8)
        pnt[7] = 2
        with pytest.raises(ba.BAArgError, match="0 or 1"):
            ba._lib.check(L.ba_lm_set_fixed(m.handle, None, ba._lib.ptr(pnt)))
        assert ba._lib.get_fixed(m.handle) == (0, 0)  # a refused mask leaves the handle as it was
        # an out-of-range index from Python: ValueError, the handle's mask untouched
        ba.lm_step(m, p["x0"], 1.0, fixed_camera_params=INTRINSICS)
        with pytest.raises(ValueError):
            ba.lm_step(m, p["x0"], 1.0, fixed_points=[p["npnts"] + 1])
        assert ba._lib.get_fixed(m.handle) == (3 * p["ncams"], 0)
        # the C entry refuses a mask with facto_type = Float16 (the Python layer does so before it: see the CPU tests)
        ba._lib.set_fixed(m.handle, *ba._lib.fixed_masks(p["ncams"], p["npnts"], [1]))
        o = lm_opts(ba, facto_type=2)
        x = p["x0"].copy()
        with pytest.raises(ba.BAArgError, match="Float16"):
            ba._lib.check(L.ba_lm_solve(m.handle, C.byref(o), ba._lib.ptr(x), C.byref(ba._lib.LMStats()),
                                        C.cast(None, ba._lib.LOG_CB), None))
        assert not bits_report(x, p["x0"])
    finally:
        m.close()


# ---- GPU: complete solves ----------------------------------------------------------------------------------------------------
_SOLVE_SCENE = dict(ncams=8, npnts=200, nobs=900, seed=3)
_scipy_cache = {}


def _solve_scene(ba):
    s = _SOLVE_SCENE
    return ba.synthetic.make_problem(s["ncams"], s["npnts"], s["nobs"], seed=s["seed"])


def _scipy_free(orc, p, fixed):
    """scipy.optimize.least_squares over the free variables only, from x0, to its tightest tolerances"""
    key = fixed.tobytes()
    if key in _scipy_cache:
        return _scipy_cache[key]
    from scipy.optimize import least_squares
    free = np.flatnonzero(~fixed)
    x_base = p["x0"].copy()

    def full(xf):
        x = x_base.copy()
        x[free] = xf
        return x

    res = least_squares(lambda xf: residual(orc, p, full(xf)), x_base[free],
                        jac=lambda xf: jac(orc, p, full(xf))[:, free].toarray(), method="trf", x_scale="jac",
                        ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=500)
    out = (full(res.x), 0.5 * float(res.fun @ res.fun))
    _scipy_cache[key] = out
    return out


_SOLVE_CASES = [(1, "LDL", "None"), (1, "LDL", "J"), (1, "LDL", "A"), (0, "LDL", "None"), (0, "LDL", "J"), (1, "PCG", "None"),
                (0, "PCG", "None")]
OBJ_TOL, X_TOL = 1e-13, 1e-8  # achieved on an MI355X: <= 2.2e-16 and <= 2.6e-9 over the seven cases
TIGHT = dict(oatol=0.0, ortol=0.0, atol=0.0, rtol=1e-12)


def _assert_decreasing(st):
    """the objective of the accepted steps strictly decreases -- down to the rounding floor of the final objective, where
    the model decrease pred itself is rounding and the accept test no longer orders anything"""
    f_acc = [row[1] for row in st.log if row[7]]
    floor = st.objective * (1 + 1e-13)
    above = [f for f in f_acc if f > floor]
    assert len(above) >= 2 and all(b < a for a, b in zip(above, above[1:])), f"accepted rows: f not strictly decreasing {f_acc}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant,facto,normalize", _SOLVE_CASES)
def test_fixed_solve_vs_scipy(ba, orc, gpu_ok, variant, facto, normalize):
    """Gauge-fixed scene (camera 1's pose, t1 of camera 2) plus the intrinsics of camera 3 and every 10th point.  The
    default stopping tests end a run at |J'r| <= cbrt(eps) |J'r_0|, which leaves x_F about 1e-5 from the minimum: the
    objective-change and first-order tests are tightened (TIGHT), as scipy's run is (1e-15)."""
    p = _solve_scene(ba)
    kw = gauge_kw(p)
    kw["fixed_camera_params"][2, 6:] = True
    kw["fixed_points"] = np.arange(1, p["npnts"] + 1, 10)
    fixed = fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = solve(ba, m, variant, facto, normalize, **TIGHT, **kw)
    finally:
        m.close()
    x = st.solution
    rep = bits_report(x[fixed], p["x0"][fixed], "fixed entries of the solution vs x0")
    assert not rep, rep
    _assert_decreasing(st)
    x_ref, f_ref = _scipy_free(orc, p, fixed)
    eo = abs(st.objective - f_ref) / f_ref
    ex = rel_err(x[~fixed], x_ref[~fixed])
    parity_record(f"fixed_solve[{variant}-{facto}-{normalize}]", objective=eo, x_free=ex, iter=st.iter, status=st.status)
    assert eo <= OBJ_TOL, f"objective {st.objective!r} vs scipy {f_ref!r}: {eo:.3e}"
    assert ex <= X_TOL, f"x_F vs scipy: {ex:.3e}"
    r = residual(orc, p, x)
    assert abs(st.objective - 0.5 * (r @ r)) <= 1e-12 * st.objective


@pytest.mark.gpu
def test_gauge_fixed_reaches_the_free_minimum(ba, gpu_ok):
    """BA is invariant to a similarity transform: holding its 7 DoF changes the parameters of the minimum, not its value
    (4.8e-15 relative on an MI355X)."""
    p = _solve_scene(ba)
    out = {}
    for name, kw in (("free", {}), ("gauge", gauge_kw(p))):
        m = ba.BALNLPModel(arrays=arrays(p))
        out[name] = solve(ba, m, **TIGHT, **kw)
        m.close()
    f0, f1 = out["free"].objective, out["gauge"].objective
    e = abs(f0 - f1) / f0
    parity_record("fixed_gauge", objective=e, free=f0, gauge=f1)
    assert e <= 1e-12, f"free minimum {f0!r} vs gauge-fixed {f1!r}: {e:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 0])
def test_motion_only(ba, orc, gpu_ok, variant):
    """Noise-free observations of x_true; every point held at its true position, the cameras start from x0."""
    p = dict(ba.synthetic.make_problem(12, 400, 1800, seed=11))
    p["pt2d"] = orc.residuals(p["cam_idx1"], p["pnt_idx1"], p["x_true"], np.zeros(2 * p["nobs"]), p["npnts"])
    nP = 3 * p["npnts"]
    x0 = np.concatenate([p["x_true"][:nP], p["x0"][nP:]])
    m = ba.BALNLPModel(arrays=arrays(dict(p, x0=x0)))
    try:
        st = solve(ba, m, variant, x=x0, fixed_points=np.arange(1, p["npnts"] + 1), restol=0.0, **TIGHT)
    finally:
        m.close()
    x = st.solution
    assert not bits_report(x[:nP], x0[:nP])
    r = residual(orc, p, x)
    rms = float(np.sqrt(np.mean(r[0::2] ** 2 + r[1::2] ** 2)))
    ec = rel_err(x[nP:], p["x_true"][nP:])
    parity_record(f"fixed_motion_only[{variant}]", rms_px=rms, cameras=ec, iter=st.iter, status=st.status)
    assert rms < 1e-6, f"RMS reprojection error {rms:.3e} px"
    assert ec < 1e-6, f"cameras vs x_true: {ec:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 0])
def test_everything_fixed(ba, orc, small_prob, gpu_ok, variant):
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        st = solve(ba, m, variant, fixed_cameras=np.arange(1, p["ncams"] + 1), fixed_points=np.ones(p["npnts"], dtype=bool))
        st2 = solve(ba, m, variant, fixed_camera_params=("r", "t", "k1", "k2", "f"), fixed_points=np.arange(1, p["npnts"] + 1))
    finally:
        m.close()
    r = residual(orc, p, p["x0"])
    for s in (st, st2):
        assert s.status == "first_order" and s.iter == 0, (s.status, s.iter)
        rep = bits_report(s.solution, p["x0"], "solution with everything fixed vs x0")
        assert not rep, rep
        assert abs(s.objective - 0.5 * (r @ r)) <= 1e-12 * s.objective
        assert (s.dual_feas if variant == 1 else s.primal_feas) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 0])
def test_no_mask_changes_nothing(ba, small_prob, gpu_ok, variant):
    p = small_prob
    fresh = ba.BALNLPModel(arrays=arrays(p))
    ref = solve(ba, fresh, variant)
    fresh.close()
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        solve(ba, m, variant, fixed_camera_params=INTRINSICS, fixed_points=[1, 2, 3])  # the handle has seen a mask
        for kw in ({}, dict(fixed_cameras=None, fixed_points=None, fixed_camera_params=None),
                   dict(fixed_cameras=[], fixed_points=[], fixed_camera_params=())):
            st = solve(ba, m, variant, **kw)
            rep = bits_report(ref.solution, st.solution, f"variant {variant}, {kw}: solution vs a fresh handle")
            assert not rep, rep
            assert st.log == ref.log and st.iter == ref.iter and st.objective == ref.objective
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [None, "0"])
def test_no_stale_recorded_sequence(ba, small_prob, gpu_ok, prefetch):
    """ONE handle solves without a mask, under mask A, mask B, huber + mask B, without a mask: each solve gives the bits and
    log rows of the same solve on a fresh handle -- a sequence recorded under one mask is never replayed under another."""
    p = small_prob
    masks = _step_masks(p)
    seq = [("none", {}), ("A", masks["intrinsics"]), ("B", masks["cam1+20%pts"]),
           ("huber+B", dict(masks["cam1+20%pts"], loss="huber", f_scale=1.0)), ("none", {})]

    def run():
        shared = ba.BALNLPModel(arrays=arrays(p))
        try:
            for name, kw in seq:
                a = solve(ba, shared, **kw)
                fresh = ba.BALNLPModel(arrays=arrays(p))
                b = solve(ba, fresh, **kw)
                fresh.close()
                rep = bits_report(a.solution, b.solution, f"{name}: reused handle vs fresh handle")
                assert not rep, rep
                assert a.log == b.log, f"{name}: log rows differ between the reused and a fresh handle"
        finally:
            shared.close()

    env("BA_LM_PREFETCH", prefetch, run)


@pytest.mark.gpu
def test_float32_model_keeps_fixed_entries(ba, small_prob, gpu_ok):
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p), T=np.float32)
    kw = dict(fixed_cameras=[2, 5], fixed_camera_params=INTRINSICS, fixed_points=np.arange(1, p["npnts"] + 1, 3))
    try:
        st = solve(ba, m, **kw)
    finally:
        m.close()
    fixed = fixed_vector(ba, p, kw)
    x = np.asarray(st.solution)
    assert x.dtype == np.float32
    rep = bits_report(x[fixed], p["x0"].astype(np.float32)[fixed], "Float32 model: fixed entries vs float32(x0)")
    assert not rep, rep
    assert st.iter > 0 and np.any(x[~fixed] != p["x0"].astype(np.float32)[~fixed])


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_loopback_fixed_step_equals_one_rank(ba, gpu_ok, world):
    """Observations sharded by point: every rank masks its own observations (its slice of the point mask, the global camera
    mask).  The step of the unsharded problem to 1e-9, the camera step bit-identical on every rank, fixed entries 0.  The
    mask is set on every shard BEFORE its communicator is attached."""
    prob = ba.synthetic.make_problem(200, 1500, 9000, seed=11)
    lam = 10.0
    g_pts = np.arange(1, prob["npnts"] + 1, 4)
    cam_kw = dict(fixed_cameras=[1, 50], fixed_camera_params=INTRINSICS)
    ref = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(prob))
    d_ref, half_ref, _ = ba.lm_step(ref, prob["x0"], lam, fixed_points=g_pts, **cam_kw)
    ref.close()
    fixed = fixed_vector(ba, prob, dict(cam_kw, fixed_points=g_pts))
    assert np.all(d_ref[fixed] == 0.0)
    whole = ba.synthetic.as_arrays(prob)
    models, shards = [], []
    with loopback_world(world, 64 << 20) as (L, loop):
        try:
            for r in range(world):
                local, info = ba.parallel.shard_problem(whole, r, world)
                m = ba.BALNLPModel(arrays=local, device=0)
                models.append(m)
                loc_pts = ba.parallel.shard_fixed_points(g_pts, info)
                ba._lib.set_fixed(m.handle, *ba._lib.fixed_masks(local[4], local[5], cam_kw["fixed_cameras"], loc_pts,
                                                                 cam_kw["fixed_camera_params"]))
                attach_loopback(ba, m, L, loop, r, world)
                shards.append((local, info, loc_pts))
            out, err = [None] * world, [None] * world

            def run(r):
                try:
                    out[r] = ba.lm_step(models[r], shards[r][0][3], lam, fixed_points=shards[r][2], **cam_kw)
                except Exception as e:  # noqa: BLE001 -- reported below with the rank
                    err[r] = e

            ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            bad = [(r, e) for r, e in enumerate(err) if e is not None]
            assert not bad, f"rank(s) failed: {bad}"
            npnts, ncams = prob["npnts"], prob["ncams"]
            delta = np.zeros(3 * npnts + 9 * ncams)
            cams = []
            for r in range(world):
                pb, pe = shards[r][1]["point_range"]
                d = out[r][0]
                delta[3 * pb:3 * pe] = d[:3 * (pe - pb)]
                cams.append(d[3 * (pe - pb):].copy())
            delta[3 * npnts:] = cams[0]
            assert np.all(delta[fixed] == 0.0), f"{world} ranks: fixed entries of delta are not 0"
            e = rel_err(delta, d_ref)
            assert e <= 1e-9, f"{world} ranks: |delta - delta_one_rank| / |delta_one_rank| = {e:.3e}"
            assert abs(out[0][1] - half_ref) <= 1e-10 * half_ref
            for r in range(1, world):
                rep = bits_report(cams[0], cams[r], f"masked camera step of rank 0 vs rank {r}")
                assert not rep, rep
        finally:
            for m in models:
                m.close()
