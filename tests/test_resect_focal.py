"""Camera resection with unknown focal length (ba_resect_cameras_focal, ba_ransac_cameras_focal, include/ba_hip.h; DESIGN §5n;
refine_cameras(resect=True, estimate_focal=True)).  The reference is tests/helpers/focal_ref.py (np.linalg.eigh and np.linalg.svd
where the kernels run Jacobi sweeps), carried on by cameras_ref and ransac_ref.  The first tests need no device; the rest run on
the GPU.

Scene: the `resect_boundary` scene of test_resect_cameras (isolated cameras of degree 0, 1, 5, 6, 7, 8, 12, 63, 64, 65, 255, 256,
257, 600; seed 69), shared with that module, in the forms
  pinhole    the true cameras with k1 = k2 = 0, pt2d re-projected, the true points held;
  far        pinhole under the similarity X' = 1e3 X + (1e4, -2e4, 3e4);
  distorted  the `exact` form of test_resect_cameras: the true k1, k2, re-projected (reference only);
  noisy      the `noisy` form of test_resect_cameras: 0.5 px on pt2d, the points of x0 held.
In every start vector all nine entries (r, t, k1, k2, f) of the focal-mode cameras are NaN.
RANSAC: the outlier layout of test_ransac_cameras on its cameras of degree >= 12 (true points held, add_outliers at 100..500 px),
exact at tau = 1 px and noisy (0.5 px) at tau = 4 px, sample = 8, 128 hypotheses.  On the noisy form the sampling seed is 1: under
seed 0 the winners of two cameras count fewer inliers than the truth (292 of 420) before the refit repairs the set, so that their
winner is not protected against rounding by the conditions below; the choice was made on the reference alone.

Bounds (from the reference alone, never from the device):
  linear stage (max_iter = 0): 100 x the reference against itself with the observations permuted, floor 1e-12, on
      |dC_pose| / (1 + |C_pose|) and on |df| / f per camera;
  refined result: the recipe of test_resect_cameras.bounds -- cost 100 x spread (1) with the floor 1e-13, parameters 10 x spread
      (2) with the floor 100 xtol -- where the two paths are the reference from the focal start and the reference from a 1e-3
      perturbation of that start (pose and f), per optional term, on the cameras where both end CONVERGED in the same minimum
      (cost_after equal to 1e-6 relative); which cameras those are is asserted on the reference (test_reference_paths).
Measured spreads and the device's achieved maxima: DESIGN §5n."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_run import attach_loopback, loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cameras_ref as cr  # noqa: E402
import focal_ref as fr  # noqa: E402
import ransac_ref as nr  # noqa: E402
import test_ransac_cameras as trn  # noqa: E402 -- clean_hypotheses, comparable, SCENE_SEED, OUTLIER_SEED
import test_resect_cameras as trc  # noqa: E402 -- the scene, its forms and the helpers around them
from refine_util import _isolated, _model, bits, codes, only_camera, rel_cost, scaled, small_scene  # noqa: E402

XTOL, XTOL_REF, MAX_ITER = trc.XTOL, trc.XTOL_REF, trc.MAX_ITER
DEG = trc.DEG
K1, K2, F = 6, 7, 8
cached = trc.cached


def nan_cameras(p, x, which=None):
    """x with all nine entries of the cameras `which` (boolean, None: all) overwritten with NaN"""
    x = np.array(x, dtype=np.float64, copy=True)
    sel = np.ones(p["ncams"], dtype=bool) if which is None else np.asarray(which)
    cr.cameras(p, x)[sel] = np.nan
    return x


def form(ba, kind):
    """(problem, the base vector: the held points and the true / generated cameras) of a form"""
    def build():
        if kind == "noisy":
            return trc.form(ba, "noisy")
        if kind == "distorted":
            return trc.form(ba, "exact")
        p = trc.form(ba, "noisy")[0]
        xt = np.array(p["x_true"], dtype=np.float64, copy=True)
        cr.cameras(p, xt)[:, K1:F] = 0.0
        if kind == "far":
            xt = trc.similarity(p, xt, trc.FAR_SCALE, trc.FAR_SHIFT)
        return dict(p, pt2d=trc.reproject(ba, p, xt), x_true=xt), xt
    return cached(("focal form", kind), build)


def truth(ba, kind):
    p, base = form(ba, kind)
    return cr.cameras(p, base if kind != "noisy" else p["x_true"])


def f_err(Cm, C_ref):
    with np.errstate(invalid="ignore"):
        return np.abs(Cm[:, F] - C_ref[:, F]) / np.abs(C_ref[:, F])


def linear_ref(p, x, info=None, **kw):
    """(x, flag, lambda_2 / lambda_12, spread of the pose, spread of f under a permutation of the observations) of the reference"""
    xs, flag, ratio = fr.resect(p, x, info, **kw)
    q, qi = trc.permuted(p, 3, info)
    x2, flag2, _ = fr.resect(q, x, qi, **kw)
    assert np.array_equal(flag, flag2)
    done = flag == fr.DONE
    sp = sf = 0.0
    if done.any():
        sp = float(trc.pose_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max())
        sf = float(f_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max())
    return xs, flag, ratio, sp, sf


def linear(ba, kind, what="plain"):
    p, base = form(ba, kind)
    info = trc.terms(ba, what)[1].get("info") if kind == "noisy" else None
    return cached(("focal linear", kind, what), lambda: linear_ref(p, nan_cameras(p, base), info))


def linear_bound(spread):
    return max(100 * spread, 1e-12)


def rms_px(p, xs, info=None):
    """RMS reprojection error per camera at the cameras of xs (NaN cameras evaluated at 1)"""
    Cm = cr.cameras(p, xs)
    f = cr.evaluate(cr.Scene(p, xs, info), np.where(np.isnan(Cm), 1.0, Cm))[0]
    with np.errstate(all="ignore"):
        return np.sqrt(2 * f / DEG)


def perturbed(p, xs, seed=1):
    """xs with pose and f of every camera perturbed by 1e-3 relative (NaN -> 1: those cameras are not compared)"""
    x = np.array(xs, dtype=np.float64, copy=True)
    Cm = cr.cameras(p, x)
    rng = np.random.default_rng(seed)
    Cm[:, :6] *= 1.0 + rng.normal(0.0, 1e-3, (p["ncams"], 6))
    Cm[:, F] *= 1.0 + rng.normal(0.0, 1e-3, p["ncams"])
    return np.where(np.isnan(x), 1.0, x)


def paths(ba, kind, what="plain"):
    """The reference's two paths of a (form, term), both to xtol = 1e-13: from the focal start, and cameras_ref.refine from the 1e-3
    perturbation of that start.  -> dict: x, st, cost, trials, D of the first; same (ncams, bool): both CONVERGED in one minimum;
    s1, s2: the cost and parameter spreads over `same`; cost_bound, par_bound"""
    def run():
        p, base = form(ba, kind)
        kw = trc.terms(ba, what)[1] if kind == "noisy" else {}
        x1, st1, cost1, tr1, D = fr.refine(p, nan_cameras(p, base), max_iter=MAX_ITER, xtol=XTOL_REF, **kw)
        x2, st2, cost2, _, _ = cr.refine(p, perturbed(p, linear(ba, kind, what)[0]), max_iter=MAX_ITER, xtol=XTOL_REF, **kw)
        conv = ((st1 & 0x7F) == cr.CONVERGED) & ((st2 & 0x7F) == cr.CONVERGED) & (linear(ba, kind, what)[1] == fr.DONE)
        if kind == "noisy":
            same = conv & (np.abs(cost2[:, 1] - cost1[:, 1]) <= 1e-6 * cost1[:, 1])
        else:  # noise-free: the minimum is 0, both costs are rounding; the same minimum = both below the cost of 1e-9 px RMS
            same = conv & (cost1[:, 1] <= 0.5 * DEG * 1e-18) & (cost2[:, 1] <= 0.5 * DEG * 1e-18)
        s1 = float(rel_cost(cost2[:, 1], cost1)[same].max()) if kind == "noisy" else 0.0
        s2 = float(scaled(D, cr.cameras(p, x2), cr.cameras(p, x1))[same].max())
        out = dict(x=x1, st=st1, cost=cost1, trials=tr1, D=D, same=same, s1=s1, s2=s2, st2=st2, x2=x2,
                   cost_bound=max(100 * s1, 1e-13), par_bound=max(10 * s2, 100 * XTOL))
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out
    return cached(("focal paths", kind, what), run)


# ---- RANSAC scenes ------------------------------------------------------------------------------------------------------------
R_KEEP = {"exact": [3, 4, 5, 6, 7, 8, 9, 10, 11], "noisy": trn.KEEP_NOISY}  # the cameras of degree >= 12 of test_ransac_cameras
R_OPTS = {"exact": dict(threshold=1.0, hypotheses=128, sample=8, refits=0, seed=0),
          "noisy": dict(threshold=4.0, hypotheses=128, sample=8, refits=2, seed=1)}


def rform(ba, kind):
    """(problem with the outliers in pt2d, x_true, the boolean outlier mask) of a RANSAC form"""
    def build():
        keep = R_KEEP[kind]
        p = _isolated(ba, tuple(trn.DEGREES[i] for i in keep), trn.SCENE_SEED)
        xt = p["x_true"]
        if kind == "exact":
            p = dict(p, pt2d=trc.reproject(ba, p, xt))
        pt2d, out = ba.synthetic.add_outliers(p, n_per_camera=np.array([trn.OUTLIERS[i] for i in keep]), seed=trn.OUTLIER_SEED)
        return dict(p, pt2d=np.ascontiguousarray(pt2d.ravel())), xt, out
    return cached(("focal rform", kind), build)


def rconsensus(ba, kind):
    p, xt, _ = rform(ba, kind)
    return cached(("focal consensus", kind), lambda: fr.consensus(p, nan_cameras(p, xt), **trn.ref_kw(R_OPTS[kind])))


def rcomparable(ba, kind):
    """the cameras the device is held to the reference's consensus on: comparable (test_ransac_cameras; min_inliers = 8), the final
    mask equal to the truth (or the camera failed), and no used observation within 10 % of tau under the final linear camera"""
    p, xt, outlier = rform(ba, kind)
    con = rconsensus(ba, kind)
    cam0 = p["cam_idx1"] - 1
    same = np.array([np.array_equal(con["inlier"][cam0 == c], ~outlier[cam0 == c]) for c in range(p["ncams"])])
    return trn.comparable(p, con, outlier, 8) & (con["failed"] | (same & (con["margin"] >= 0.1)))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_keyword(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_resect_cameras_focal", "ba_resect_cameras_focal_dev", "ba_ransac_cameras_focal", "ba_ransac_cameras_focal_dev"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header
    flat = " ".join(header.split())
    for line in ("camera resection with unknown focal length", "phi = sqrt((|A_1|^2 + |A_2|^2) / (2 |A_3|^2))",
                 "a = sqrt(sum |m|^2 / n)", "an unknown f: ba_resect_cameras_focal", "an unknown f: ba_ransac_cameras_focal"):
        assert line in flat, line
    assert L.ba_resect_cameras_focal(None, None, -1, -1.0, -1.0, None, None, None, None) == 1 and b"null argument" in L.ba_last_error()
    assert L.ba_resect_cameras_focal_dev(None, None, -1, -1.0, -1.0, None, None, None, None, None) == 1
    good, tail = lib.RansacOpts(1.0, 0, 0, -1, 0, 0), (None,) * 7
    assert L.ba_ransac_cameras_focal(None, None, C.byref(good), -1, -1.0, -1.0, *tail) == 1 and b"null argument" in L.ba_last_error()
    assert L.ba_ransac_cameras_focal_dev(None, None, C.byref(good), -1, -1.0, -1.0, *tail, None) == 1
    assert L.ba_ransac_cameras_focal(None, None, None, -1, -1.0, -1.0, *tail) == 1 and b"options" in L.ba_last_error()
    bad = lib.RansacOpts(1.0, 0, 5, -1, 0, 0)
    for fn, extra in ((L.ba_ransac_cameras_focal, ()), (L.ba_ransac_cameras_focal_dev, (None,))):
        assert fn(None, None, C.byref(bad), -1, -1.0, -1.0, *tail, *extra) == 1
        assert b"sample" in L.ba_last_error() and b"ba_ransac_cameras_focal" in L.ba_last_error()
    kwd = ba.refine_cameras.__kwdefaults__
    assert kwd["estimate_focal"] is False and kwd["resect"] is False and kwd["ransac"] is None
    x = np.zeros(3)
    for bad_flag in (1, "yes", None):
        with pytest.raises(ValueError, match="estimate_focal"):
            ba.refine_cameras(None, x, resect=True, estimate_focal=bad_flag)
    with pytest.raises(ValueError, match="resect=True"):
        ba.refine_cameras(None, x, estimate_focal=True)
    with pytest.raises(ValueError, match="resect=True"):
        ba.refine_cameras(None, x, estimate_focal=True, ransac=dict(threshold=1.0))
    with pytest.raises(ValueError, match="threshold"):
        ba.refine_cameras(None, x, resect=True, estimate_focal=True, ransac=dict())


@pytest.mark.parametrize("kind", ["pinhole", "far"])
def test_reference_on_exact_data(ba, kind):
    """Every camera of degree >= 6 is resected, the rest are DEGENERATE and bit-unchanged; at max_iter = 0 the reprojection is below
    1e-9 px RMS and |f^ - f| / f <= 1e-10.  Measured at seed 69: pinhole 2.7e-12 px and 1.1e-13, far 1.3e-11 px and 2.0e-13.  The
    refinement from there (all nine components free) ends at the true camera to the noise-free bound 3e-9 (scaled)."""
    p, base = form(ba, kind)
    xs, flag, ratio, sp, sf = linear(ba, kind)
    ok = DEG >= 6
    assert np.array_equal(flag == fr.DONE, ok) and (flag[~ok] == fr.DEGENERATE).all()
    assert np.array_equal(bits(cr.cameras(p, xs)[~ok]), bits(cr.cameras(p, nan_cameras(p, base))[~ok]))
    rms, fe = rms_px(p, xs)[ok].max(), f_err(cr.cameras(p, xs), truth(ba, kind))[ok].max()
    print(f"{kind}: reprojection {rms:.3e} px RMS, |f^ - f| / f {fe:.3e}, lambda_2 / lambda_12 {np.nanmin(ratio):.1e} .. {np.nanmax(ratio):.1e}, "
          f"spread under a permutation: pose {sp:.3e}, f {sf:.3e}")
    assert rms < 1e-9 and fe <= 1e-10
    assert (cr.cameras(p, xs)[ok, K1:F] == 0).all()
    pa = paths(ba, kind)
    err = scaled(pa["D"], cr.cameras(p, pa["x"]), truth(ba, kind))[ok].max()
    print(f"{kind}: refined against the truth {err:.3e}, {pa['trials'].max()} trials")
    assert ((pa["st"] & 0x7F)[ok] == cr.CONVERGED).all() and ((pa["st"] & 0x7F)[~ok] == cr.DEGENERATE).all() and err <= 3e-9


def test_reference_on_distorted_exact_data(ba):
    """The true k1, k2: the linear stage ignores them (its f^ is off by what the distortion moves the detections), and the
    refinement with all nine components free returns the true camera, k1 and k2 included -- on every camera of degree >= 6: both
    paths (the focal start, its 1e-3 perturbation) end CONVERGED below the cost of 1e-9 px RMS."""
    p, base = form(ba, "distorted")
    xs, flag, ratio, sp, sf = linear(ba, "distorted")
    ok = DEG >= 6
    pa = paths(ba, "distorted")
    Ct = truth(ba, "distorted")
    err = scaled(pa["D"], cr.cameras(p, pa["x"]), Ct)[ok].max()
    err2 = scaled(pa["D"], cr.cameras(p, pa["x2"]), Ct)[ok].max()
    print(f"distorted: linear f^ off by {f_err(cr.cameras(p, xs), Ct)[ok].max():.3e}, {rms_px(p, xs)[ok].max():.3e} px RMS; refined against the "
          f"truth {err:.3e} (from the perturbed start {err2:.3e}), {pa['trials'].max()} trials")
    assert np.array_equal(flag == fr.DONE, ok) and np.array_equal(pa["same"], ok)
    assert err <= 3e-9 and err2 <= 3e-9
    assert (np.abs(cr.cameras(p, pa["x"])[ok, K1] - Ct[ok, K1]) <= 1e-6 * np.abs(Ct[ok, K1])).all()


@pytest.mark.parametrize("what", ["plain", "huber", "info", "cam_prior"])
def test_reference_paths(ba, what):
    """What the GPU comparison on the noisy form rests on: the linear stage under a second permutation stays inside the linear
    bound; the two paths end in the same minimum on every camera with 6 used observations or more (info: degree 12 keeps 5 and
    degree 64 none); the spreads are printed."""
    p, base = form(ba, "noisy")
    kw = trc.terms(ba, what)[1]
    xs, flag, ratio, sp, sf = linear(ba, "noisy", what)
    q, qi = trc.permuted(p, 4, kw.get("info"))
    x2, flag2, _ = fr.resect(q, nan_cameras(p, base), qi)
    done = flag == fr.DONE
    nused = cr.Scene(p, base, kw.get("info")).nused
    e_pose = trc.pose_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max()
    e_f = f_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max()
    pa = paths(ba, "noisy", what)
    print(f"noisy {what}: linear spread pose {sp:.3e}, f {sf:.3e}; second permutation {e_pose:.3e}, {e_f:.3e}; |f^ - f| / f "
          f"{f_err(cr.cameras(p, xs), truth(ba, 'noisy'))[done].min():.1e} .. {f_err(cr.cameras(p, xs), truth(ba, 'noisy'))[done].max():.1e}; "
          f"paths: (1) {pa['s1']:.3e} (bound {pa['cost_bound']:.1e}), (2) {pa['s2']:.3e} (bound {pa['par_bound']:.1e}), trials {pa['trials'].max()}")
    assert np.array_equal(flag, flag2) and np.array_equal(done, nused >= 6)
    assert e_pose <= linear_bound(sp) and e_f <= linear_bound(sf)
    assert np.array_equal(pa["same"], done)
    assert ((pa["st"] & 0x7F)[~done] == cr.DEGENERATE).all() and (pa["cost"][~done] == 0).all() and (pa["cost"][:, 1] <= pa["cost"][:, 0]).all()
    if what == "info":
        assert nused[DEG == 12] == 5 and nused[DEG == 63] == 6 and nused[DEG == 64] == 0


@pytest.mark.parametrize("kind", ["exact", "noisy"])
def test_reference_ransac_conditions(ba, kind):
    """The reference's final mask is the true inlier mask on every camera that does not fail; the camera that keeps 4 inliers of 12
    fails (exact); every camera meets the conditions under which the device is held to the winner and the counts (rcomparable);
    no hypothesis has lambda_2 / lambda_12 within a factor 100 of the degeneracy threshold."""
    p, xt, outlier = rform(ba, kind)
    con = rconsensus(ba, kind)
    cam0 = p["cam_idx1"] - 1
    true_n = np.bincount(cam0, weights=(~outlier).astype(float), minlength=p["ncams"]).astype(int)
    fails = true_n < 8
    good = ~fails
    with np.errstate(invalid="ignore"):
        near = (con["ratio"] > 1e-12) & (con["ratio"] < 1e-8)
    print(f"{kind}: winners {con['best_hyp']}, clean hypotheses {trn.clean_hypotheses(p, con, outlier).sum(1)}, adopted {con['adopted']}, "
          f"margin {con['margin'][good].min():.3f}, f^ of the winners off by {np.nanmax(np.abs(con['f_best'] / cr.cameras(p, xt)[:, F] - 1)):.2e}")
    assert con["attempted"].all() and np.array_equal(con["failed"], fails) and fails.sum() == (1 if kind == "exact" else 0)
    assert np.array_equal(con["inlier"][good[cam0]], ~outlier[good[cam0]]) and not con["inlier"][fails[cam0]].any()
    assert np.array_equal(con["n_inliers"][good], true_n[good]) and not near.any()
    assert rcomparable(ba, kind).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _run(ba, p, x, **kw):
    m = _model(ba, p)
    try:
        return ba.refine_cameras(m, x, resect=True, estimate_focal=True, **kw)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pinhole", "noisy"])
def test_linear_stage(ba, gpu_ok, kind):
    """max_iter = 0: the pose and f^ of the linear stage are written, a free k1 / k2 as 0; both cost entries are f_c there (noisy:
    within 1e-13 relative of the reference's f_c at the device's camera; pinhole: below the cost of 1e-9 px RMS)."""
    p, base = form(ba, kind)
    n = p["npnts"]
    xs, flag, _, sp, sf = linear(ba, kind)
    x0 = nan_cameras(p, base)
    x, info = _run(ba, p, x0, max_iter=0)
    done = flag == fr.DONE
    st_ref = cr.refine(p, np.where(np.isnan(xs), 1.0, xs), max_iter=0)[1]
    st = codes(ba, info)
    assert np.array_equal(done, DEG >= 6)
    assert np.array_equal(st[done], st_ref[done]) and (st[~done] == cr.DEGENERATE).all() and ((st & 0x7F)[done] == cr.MAX_ITER).all()
    Cd, C0, Cr = cr.cameras(p, x), cr.cameras(p, x0), cr.cameras(p, xs)
    assert np.array_equal(bits(Cd[~done]), bits(C0[~done])) and (info["cost_before"][~done] == 0).all() and (info["cost_after"][~done] == 0).all()
    e_pose, e_f = trc.pose_err(Cd, Cr)[done].max(), f_err(Cd, Cr)[done].max()
    cost_ref = cr.refine(p, np.where(np.isnan(x), 1.0, x), max_iter=0)[2][:, 0]
    nz = done & (cost_ref > 0)
    e_cost = (np.abs(info["cost_before"] - cost_ref)[nz] / cost_ref[nz]).max()
    print(f"{kind}: linear pose {e_pose:.3e} (bound {linear_bound(sp):.1e}), f^ {e_f:.3e} (bound {linear_bound(sf):.1e}), cost {e_cost:.3e}, "
          f"worst cost {info['cost_before'].max():.3e}")
    assert e_pose <= linear_bound(sp) and e_f <= linear_bound(sf)
    assert (Cd[done, K1:F] == 0).all() and np.isfinite(Cd[done]).all()
    assert np.array_equal(bits(info["cost_before"]), bits(info["cost_after"])) and info["iters_max"] == 0
    if kind == "noisy":
        assert e_cost <= 1e-13
    else:
        assert (info["cost_before"][done] <= 0.5 * DEG[done] * 1e-18).all() and (cost_ref[done] <= 0.5 * DEG[done] * 1e-18).all()
    assert np.array_equal(bits(x[:3 * n]), bits(x0[:3 * n]))
    assert info["counts"]["degenerate"] == 3 and info["counts"]["max_iter"] == 11


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pinhole", "far"])
def test_end_to_end_exact(ba, gpu_ok, kind):
    """Noise-free: the refinement from the focal start, all nine components free, ends at the true camera (3e-9 scaled, the
    noise-free bound of test_refine_cameras) with a cost below that of 1e-9 px RMS; the linear stage within its bounds."""
    p, base = form(ba, kind)
    x0 = nan_cameras(p, base)
    xs, flag, _, sp, sf = linear(ba, kind)
    m = _model(ba, p)
    try:
        xl, il = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, max_iter=0)
        x, info = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, xtol=XTOL, max_iter=MAX_ITER)
    finally:
        m.close()
    ok = DEG >= 6
    D = paths(ba, kind)["D"]
    e_pose, e_f = trc.pose_err(cr.cameras(p, xl), cr.cameras(p, xs))[ok].max(), f_err(cr.cameras(p, xl), cr.cameras(p, xs))[ok].max()
    err = scaled(D, cr.cameras(p, x), truth(ba, kind))[ok].max()
    print(f"{kind}: linear pose {e_pose:.3e} (bound {linear_bound(sp):.1e}), f^ {e_f:.3e} (bound {linear_bound(sf):.1e}); refined against the "
          f"truth {err:.3e}, f {f_err(cr.cameras(p, x), truth(ba, kind))[ok].max():.3e}; cost_after {info['cost_after'].max():.3e}; trials {info['iters_max']}")
    assert e_pose <= linear_bound(sp) and e_f <= linear_bound(sf)
    assert (info["status"][ok] == "converged").all() and (info["status"][~ok] == "degenerate").all() and not info["behind"].any()
    assert err <= 3e-9 and (info["cost_after"][ok] <= 0.5 * DEG[ok] * 1e-18).all()
    assert np.array_equal(bits(cr.cameras(p, x)[~ok]), bits(cr.cameras(p, x0)[~ok]))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["plain", "huber", "info", "cam_prior"])
def test_end_to_end_noisy(ba, gpu_ok, what):
    """The noisy form under the optional terms against the reference, on the cameras where the reference's two paths end in the
    same minimum (test_reference_paths: every camera the linear stage places)."""
    p, base = form(ba, "noisy")
    dev_kw = trc.terms(ba, what)[0]
    x0 = nan_cameras(p, base)
    x, info = _run(ba, p, x0, xtol=XTOL, max_iter=MAX_ITER, **dev_kw)
    pa = paths(ba, "noisy", what)
    same = pa["same"]
    st = codes(ba, info)
    Cd, Cr, C0 = cr.cameras(p, x), cr.cameras(p, pa["x"]), cr.cameras(p, x0)
    e_after = rel_cost(info["cost_after"], pa["cost"])[same].max()
    e_par = scaled(pa["D"], Cd, Cr)[same].max()
    print(f"noisy {what}: cost_after {e_after:.3e} (bound {pa['cost_bound']:.1e}), parameters {e_par:.3e} (bound {pa['par_bound']:.1e}), "
          f"trials {info['iters_max']} (reference {pa['trials'].max()})")
    assert np.array_equal(st, pa["st"]), (st, pa["st"])
    assert e_after <= pa["cost_bound"] and e_par <= pa["par_bound"]
    assert np.array_equal(bits(Cd[~same]), bits(C0[~same])) and (info["cost_before"][~same] == 0).all() and (info["cost_after"][~same] == 0).all()
    assert np.array_equal(info["status"] == "degenerate", ~same) and (info["cost_after"] <= info["cost_before"]).all()
    assert np.array_equal(bits(x[:3 * p["npnts"]]), bits(x0[:3 * p["npnts"]]))
    assert sum(info["counts"][s] for s in ba._lib.POINT_STATES) == p["ncams"] and info["counts"]["behind"] == int(info["behind"].sum())


@pytest.mark.gpu
def test_cameras_not_in_focal_mode(ba, gpu_ok):
    """One call: f held on one camera and a group of two -- both get the calibrated resection with the bits of resect=True
    without estimate_focal on the same handle; a camera with a pose component held starts from x (the bits of resect=False); a
    fully fixed camera is FIXED; a held non-zero k1 keeps its bits while f^ is written."""
    p, base = form(ba, "noisy")
    nc = p["ncams"]
    held = np.zeros((nc, 9), dtype=bool)
    held[7, F] = True                  # degree 63: f held
    members = np.array([6, 10])        # degrees 12 and 255: a group
    held[11, 4] = True                 # degree 256: a pose component held
    held[9] = True                     # degree 65: fixed
    held[12, K1] = True                # degree 257: k1 held, f free
    labels = np.zeros(nc, dtype=np.int64)
    labels[members] = 1
    calibrated = np.zeros(nc, dtype=bool)
    calibrated[[7, 6, 10]] = True
    from_x = held[:, :6].any(axis=1)
    focal = ~calibrated & ~from_x
    x0 = nan_cameras(p, base, focal)
    C0 = cr.cameras(p, x0)
    C0[calibrated, :6] = np.nan
    C0[12, K1] = cr.cameras(p, base)[12, K1]
    assert C0[12, K1] != 0
    kw = dict(fixed_camera_params=held, shared_intrinsics=[list(members + 1)], xtol=XTOL, max_iter=MAX_ITER)
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, **kw)
        xc, ic = ba.refine_cameras(m, x0, resect=True, **kw)
        xp, ip = ba.refine_cameras(m, x0, resect=False, **kw)
    finally:
        m.close()
    Cd = cr.cameras(p, x)
    for sel, (xo, io) in ((calibrated, (xc, ic)), (from_x, (xp, ip))):
        assert np.array_equal(bits(Cd[sel]), bits(cr.cameras(p, xo)[sel])) and np.array_equal(codes(ba, info)[sel], codes(ba, io)[sel])
        for key in ("cost_before", "cost_after"):
            assert np.array_equal(bits(info[key][sel]), bits(io[key][sel]))
    assert (info["status"][calibrated] == "converged").all() and info["status"][9] == "fixed" and info["status"][11] == "converged"
    assert (ic["status"][focal] == "degenerate").all()  # (without the flag a camera whose f is NaN cannot be resected)
    assert np.array_equal(bits(Cd[held]), bits(C0[held])) and np.array_equal(bits(Cd[members][:, K1:]), bits(C0[members][:, K1:]))
    assert info["status"][12] == "converged" and np.isfinite(Cd[12]).all() and Cd[12, K1] == C0[12, K1]
    x_ref, st_ref, cost_ref, _, D = fr.refine(p, x0, max_iter=MAX_ITER, xtol=XTOL_REF, held=held, groups=labels)
    moved = (st_ref & 0x7F) <= cr.MAX_ITER
    pa = paths(ba, "noisy")
    e_after, e_par = rel_cost(info["cost_after"], cost_ref)[moved].max(), scaled(D, Cd, cr.cameras(p, x_ref))[moved].max()
    print(f"mixed modes: cost_after {e_after:.3e} (bound {pa['cost_bound']:.1e}), parameters {e_par:.3e} (bound {pa['par_bound']:.1e})")
    assert np.array_equal(codes(ba, info), st_ref) and e_after <= pa["cost_bound"] and e_par <= pa["par_bound"]


@pytest.mark.gpu
def test_inputs_never_read(ba, gpu_ok):
    """(r, t, k1, k2, f) of a focal-mode camera are not read: NaN, zeros, sevens and the generator's cameras give identical bits."""
    p, base = form(ba, "noisy")
    x0 = nan_cameras(p, base)
    m = _model(ba, p)
    try:
        runs = [ba.refine_cameras(m, np.where(np.isnan(x0), fill, x0), resect=True, estimate_focal=True, xtol=XTOL, max_iter=MAX_ITER)
                for fill in (np.nan, 0.0, 7.0, base)]
    finally:
        m.close()
    (x, info), done = runs[0], DEG >= 6
    assert (info["status"][done] == "converged").all()
    for xo, io in runs[1:]:
        assert np.array_equal(bits(cr.cameras(p, xo)[done]), bits(cr.cameras(p, x)[done])) and np.array_equal(codes(ba, io), codes(ba, info))
        for key in ("cost_before", "cost_after"):
            assert np.array_equal(bits(io[key]), bits(info[key]))
        assert io["iters_max"] == info["iters_max"] and io["counts"] == info["counts"]


@pytest.mark.gpu
def test_degenerate_inputs(ba, gpu_ok):
    """Degree 5, points in a plane (the _flattened construction of test_resect_cameras) and every detection of a camera at 0
    (a = 0): DEGENERATE, bit-unchanged, cost entries 0, no flag -- on the reference and on the device."""
    p5 = only_camera(form(ba, "pinhole")[0], int(np.flatnonzero(DEG == 5)[0]))
    flat = trc._flattened(ba, 0.0)[0]
    one = trc._one(ba)
    zero = dict(one, pt2d=np.zeros_like(one["pt2d"]))
    for name, p in (("degree 5", p5), ("coplanar", flat), ("a = 0", zero)):
        x0 = nan_cameras(p, p["x_true"])
        assert fr.resect(p, x0)[1][0] == fr.DEGENERATE, name
        for it in (0, 5):
            x, info = _run(ba, p, x0, max_iter=it)
            assert info["status"][0] == "degenerate" and np.array_equal(bits(x), bits(x0)), name
            assert info["cost_before"][0] == 0 and info["cost_after"][0] == 0 and not info["behind"][0] and info["counts"]["degenerate"] == 1
    x, info = _run(ba, one, nan_cameras(one, one["x_true"]), max_iter=0)  # (the scene of the last two is regular as it stands)
    assert info["status"][0] == "max_iter" and np.isfinite(x).all()


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """Two calls, and the host and the device-resident entry, give the same bits; cameras of degree 12, 255 and 600 give the same
    bits alone as inside the scene; the next lm_step has the bits it has without the call; a communicator is refused."""
    p, base = form(ba, "noisy")
    nc, nvar = p["ncams"], len(base)
    x0 = nan_cameras(p, base)
    L = ba._lib.lib()
    q = small_scene(ba)
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    try:
        x1, i1 = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, xtol=XTOL, max_iter=MAX_ITER)
        x2, i2 = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, xtol=XTOL, max_iter=MAX_ITER)
        d = [C.c_void_p() for _ in range(3)]
        for ptr_, size in zip(d, (8 * nvar, nc, 16 * nc)):
            ba._lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        x3, st3, cost3 = x0.copy(), np.zeros(nc, dtype=np.uint8), np.zeros((nc, 2))
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        ba._lib.check(L.ba_memcpy_h2d(m.handle, d[0], ba._lib.ptr(x3), 8 * nvar))
        ba._lib.check(L.ba_resect_cameras_focal_dev(m.handle, d[0], MAX_ITER, XTOL, -1.0, d[1], d[2], ba._lib.ptr(counts), C.byref(its), None))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(x3), d[0], 8 * nvar))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(st3), d[1], nc))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(cost3), d[2], 16 * nc))
        for ptr_ in d:
            ba._lib.check(L.ba_dev_free(m.handle, ptr_))
        alone = {}
        for c in (6, 10, nc - 1):  # degrees 12, 255 and 600
            pc = only_camera(p, c)
            alone[c] = _run(ba, pc, nan_cameras(pc, pc["x0"]), xtol=XTOL, max_iter=MAX_ITER)
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.refine_cameras(ms, nan_cameras(q, q["x0"]), resect=True, estimate_focal=True, xtol=XTOL)
        ba.refine_cameras(ms, nan_cameras(q, q["x0"]), resect=True, estimate_focal=True, ransac=dict(threshold=4.0, sample=8), xtol=XTOL)
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.refine_cameras(mc, x0, resect=True, estimate_focal=True)
                with pytest.raises(ba.BAArgError) as er:
                    ba.refine_cameras(mc, x0, resect=True, estimate_focal=True, ransac=dict(threshold=4.0))
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_resect_cameras_focal" in str(e.value) and "communicator" in str(e.value)
    assert "ba_ransac_cameras_focal" in str(er.value) and "communicator" in str(er.value)
    assert np.array_equal(bits(x1), bits(x2)) and np.array_equal(bits(x1), bits(x3))
    assert np.array_equal(bits(i1["cost_after"]), bits(i2["cost_after"])) and np.array_equal(bits(i1["cost_after"]), bits(cost3[:, 1]))
    assert np.array_equal(bits(i1["cost_before"]), bits(cost3[:, 0]))
    assert np.array_equal(codes(ba, i1), st3) and its.value == i1["iters_max"] and counts[0] == i1["counts"]["converged"]
    for c, (xa, ia) in alone.items():
        assert np.array_equal(bits(xa[-9:]), bits(cr.cameras(p, x1)[c])), c
        assert ia["cost_after"][0] == i1["cost_after"][c] and ia["cost_before"][0] == i1["cost_before"][c]
    for a, b, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c_))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "noisy"])
def test_ransac(ba, gpu_ok, kind):
    """The consensus stage in focal mode: the inlier bytes, n_inliers and best_hypothesis of the reference on the cameras for which
    the reference conditions hold (test_reference_ransac_conditions: all); x, status and cost equal, bit for bit, the focal
    resection on the same handle with that mask as obs_info; the camera whose best count is below min_inliers (exact: 4 inliers of
    12) is DEGENERATE and untouched; the device-resident entry gives the same bits.  exact: max_iter = 0, the linear camera within
    the linear bound of the reference on the set; noisy: the refined cameras end CONVERGED."""
    p, xt, outlier = rform(ba, kind)
    nc, nvar, nobs = p["ncams"], len(xt), p["nobs"]
    cam0 = p["cam_idx1"] - 1
    x0 = nan_cameras(p, xt)
    con, sel = rconsensus(ba, kind), rcomparable(ba, kind)
    o = R_OPTS[kind]
    kw = dict(max_iter=0) if kind == "exact" else dict(xtol=XTOL, max_iter=MAX_ITER)
    L, lib = ba._lib.lib(), ba._lib
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, ransac=o, **kw)
        sig = np.ones((nobs, 2))
        sig[~info["inliers"]] = np.inf
        y, iy = ba.refine_cameras(m, x0, resect=True, estimate_focal=True, obs_info=sig, **kw)
        lib.check(L.ba_lm_set_obs_info(m.handle, None))
        d = [C.c_void_p() for _ in range(6)]
        sizes = (8 * nvar, nc, 16 * nc, nobs, 4 * nc, 4 * nc)
        for ptr_, size in zip(d, sizes):
            lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        host = [x0.copy(), np.zeros(nc, dtype=np.uint8), np.zeros((nc, 2)), np.zeros(nobs, dtype=np.uint8), np.zeros(nc, dtype=np.int32),
                np.zeros(nc, dtype=np.int32)]
        lib.check(L.ba_memcpy_h2d(m.handle, d[0], lib.ptr(host[0]), 8 * nvar))
        lib.check(L.ba_ransac_cameras_focal_dev(m.handle, d[0], C.byref(lib.ransac_opts(o)), kw["max_iter"], XTOL, -1.0, d[1], d[2], None, None,
                                                d[3], d[4], d[5], None))
        lib.check(L.ba_synchronize(m.handle))
        for a, ptr_, size in zip(host, d, sizes):
            lib.check(L.ba_memcpy_d2h(m.handle, lib.ptr(a), ptr_, size))
            lib.check(L.ba_dev_free(m.handle, ptr_))
    finally:
        m.close()
    assert sel.all()
    assert np.array_equal(info["inliers"][sel[cam0]], con["inlier"][sel[cam0]])
    assert np.array_equal(info["n_inliers"][sel], con["n_inliers"][sel]) and np.array_equal(info["best_hypothesis"][sel], con["best_hyp"][sel])
    assert np.array_equal((info["status"] == "degenerate")[sel], con["failed"][sel])
    good = ~con["failed"]
    assert np.array_equal(info["inliers"][good[cam0]], ~outlier[good[cam0]])
    # bit for bit the focal resection on the set
    assert np.array_equal(bits(x), bits(y)) and np.array_equal(codes(ba, info), codes(ba, iy))
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key]), bits(iy[key]))
    assert info["iters_max"] == iy["iters_max"] and info["counts"] == iy["counts"]
    # the device-resident entry
    assert np.array_equal(bits(x), bits(host[0])) and np.array_equal(codes(ba, info), host[1])
    assert np.array_equal(bits(info["cost_before"]), bits(host[2][:, 0])) and np.array_equal(bits(info["cost_after"]), bits(host[2][:, 1]))
    assert np.array_equal(info["inliers"], host[3] != 0) and np.array_equal(info["n_inliers"], host[4]) and np.array_equal(info["best_hypothesis"], host[5])
    Cd, C0 = cr.cameras(p, x), cr.cameras(p, x0)
    fails = np.flatnonzero(con["failed"])
    assert np.array_equal(bits(Cd[fails]), bits(C0[fails])) and (info["cost_before"][fails] == 0).all() and (info["cost_after"][fails] == 0).all()
    assert not info["inliers"][np.isin(cam0, fails)].any() and not info["behind"][fails].any()
    assert np.isfinite(Cd[good]).all() and (info["status"][good] == ("max_iter" if kind == "exact" else "converged")).all()
    if kind == "exact":
        assert len(fails) == 1 and info["n_inliers"][fails[0]] < 8
        xs, flag, _, sp, sf = linear_ref(p, x0, nr.masked_info(p, con["inlier"]))
        e_pose, e_f = trc.pose_err(Cd, cr.cameras(p, xs))[good].max(), f_err(Cd, cr.cameras(p, xs))[good].max()
        print(f"exact: linear pose {e_pose:.3e} (bound {linear_bound(sp):.1e}), f^ {e_f:.3e} (bound {linear_bound(sf):.1e}); f^ against the "
              f"truth {f_err(Cd, cr.cameras(p, xt))[good].max():.3e}")
        assert np.array_equal(flag == fr.DONE, good) and e_pose <= linear_bound(sp) and e_f <= linear_bound(sf)
    else:
        print(f"noisy: f against the truth {f_err(Cd, cr.cameras(p, xt)).max():.3e}, trials {info['iters_max']}")
        assert (info["cost_after"] <= info["cost_before"]).all()
