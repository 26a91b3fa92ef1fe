"""Outlier-robust camera resection (ba_ransac_cameras, include/ba_hip.h; refine_cameras(resect=True, ransac=...)).
The reference is tests/helpers/ransac_ref.py: the header restated in numpy on top of resect_ref.resect_one (np.linalg.eigh where
the kernel runs Jacobi sweeps inside a wave) and cameras_ref.refine.  The first tests need no device; the rest run on the GPU.

Scenes: isolated cameras (refine_util._isolated, seed 69), the true points held, the pose entries NaN, the intrinsics true.
  exact  degrees 5, 6, 7, 12, 12, 63, 64, 65, 255, 256, 257, 600 with 0, 0, 1, 3, 8, 19, 19, 20, 76, 77, 77, 180 outliers
         (synthetic.add_outliers: 100..500 px), the other detections re-projected; tau = 1 px.  Degree 5 and the camera that
         keeps 4 inliers of 12 fail.
  noisy  the eight cameras of degree >= 12 that keep 6 inliers or more, the other detections re-projected + 0.5 px Gaussian;
         tau = 4 px.  (A 6-point linear pose from noisy data fits nothing at degree 6 and 7: a property of the method.)
The gap between 0.5 px of noise and 100 px outliers is what makes the final mask insensitive to rounding; the conditions under
which the device can be held to the reference's masks are asserted on the reference first (test_reference_conditions).  The
seeds were chosen on the reference, never on the device.

Bounds (from the reference alone): the linear pose -- 100 x the reference against itself with the observations permuted, floor
1e-12 (the recipe of test_resect_cameras); the refined result -- cost 100 x spread (1) with the floor 1e-13, parameters 10 x
spread (2) with the floor 100 xtol, the two paths being the reference from its resected start and the reference from a 1e-3
perturbation of the true pose, both on the true inliers (the recipe of test_refine_cameras.bounds)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_run import attach_loopback, loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cameras_ref as cr  # noqa: E402
import ransac_ref as nr  # noqa: E402
import resect_ref as rr  # noqa: E402
from refine_util import _isolated, _model, bits, cam_prior_on, codes, only_camera, rel_cost, scaled, small_scene  # noqa: E402

XTOL, XTOL_REF, MAX_ITER = 1e-10, 1e-13, 400
SCENE_SEED, OUTLIER_SEED = 69, 5
DEGREES = (5, 6, 7, 12, 12, 63, 64, 65, 255, 256, 257, 600)
OUTLIERS = (0, 0, 1, 3, 8, 19, 19, 20, 76, 77, 77, 180)
KEEP_NOISY = [3, 5, 6, 7, 8, 9, 10, 11]
FORMS = {"exact": dict(degrees=DEGREES, outliers=OUTLIERS, tau=1.0, refits=0, seed=0),
         "noisy": dict(degrees=tuple(DEGREES[i] for i in KEEP_NOISY), outliers=tuple(OUTLIERS[i] for i in KEEP_NOISY), tau=4.0,
                       refits=2, seed=0)}
POSE = np.array([True] * 6 + [False] * 3)
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def nan_poses(p, x, which=None):
    x = np.array(x, dtype=np.float64, copy=True)
    sel = np.ones(p["ncams"], dtype=bool) if which is None else np.asarray(which)
    cr.cameras(p, x)[np.ix_(sel, POSE)] = np.nan
    return x


def form(ba, kind):
    """(problem with the outliers in pt2d, the base vector x_true, the boolean outlier mask) of a form"""
    def build():
        f = FORMS[kind]
        p = _isolated(ba, f["degrees"], SCENE_SEED)
        xt = p["x_true"]
        if kind == "exact":
            n = p["npnts"]
            X, Cm = np.asarray(xt[:3 * n]).reshape(n, 3), cr.cameras(p, xt)
            p = dict(p, pt2d=np.ascontiguousarray(ba.synthetic.project(X[p["pnt_idx1"] - 1], Cm[p["cam_idx1"] - 1]).ravel()))
        pt2d, out = ba.synthetic.add_outliers(p, n_per_camera=np.array(f["outliers"]), seed=OUTLIER_SEED)
        return dict(p, pt2d=np.ascontiguousarray(pt2d.ravel())), xt, out
    return cached(("form", kind), build)


def opts(kind, **over):
    f = FORMS[kind]
    return dict(dict(threshold=f["tau"], hypotheses=128, sample=6, refits=f["refits"], seed=f["seed"]), **over)


def ref_kw(o):
    return dict(threshold=o["threshold"], hypotheses=o.get("hypotheses", 0), sample_size=o.get("sample", 0), refits=o.get("refits", -1),
                min_inliers=o.get("min_inliers", 0), seed=o.get("seed", 0))


def consensus(ba, kind, info=None, key=None, **over):
    p, base, _ = form(ba, kind)
    return cached(("consensus", kind, key, tuple(sorted(over.items()))),
                  lambda: nr.consensus(p, nan_poses(p, base), info=info, **ref_kw(opts(kind, **over))))


def clean_hypotheses(p, con, outlier):
    """(ncams, H) boolean: the hypothesis has a sample, and no outlier in it"""
    H = con["counts"].shape[1]
    return np.array([[s is not None and not outlier[s].any() for s in con["samples"][c]] for c in range(p["ncams"])]).reshape(p["ncams"], H)


def comparable(p, con, outlier, min_inliers=6):
    """the cameras whose outcome rounding cannot change: the winner is clean, counts every true inlier and leads every contaminated
    hypothesis by 3 or more -- or the camera failed with every count <= min_inliers - 3"""
    clean = clean_hypotheses(p, con, outlier)
    cam0 = p["cam_idx1"] - 1
    truth = np.bincount(cam0, weights=(~outlier).astype(float), minlength=p["ncams"]).astype(int)
    ok = np.zeros(p["ncams"], dtype=bool)
    for c in np.flatnonzero(con["attempted"]):
        cnt = con["counts"][c]
        if con["failed"][c]:
            ok[c] = cnt.max() <= min_inliers - 3
        else:
            b = con["best_hyp"][c]
            dirty = cnt[~clean[c]]
            ok[c] = clean[c, b] and cnt[b] == truth[c] and (dirty.size == 0 or dirty.max() <= cnt[b] - 3)
    return ok


def pose_err(Cm, C_ref):
    return np.linalg.norm((Cm - C_ref)[:, :6], axis=1) / (1.0 + np.linalg.norm(C_ref[:, :6], axis=1))


def linear_ref(p, x, info):
    """(x, flag, spread under a permutation of the observations) of the reference's resection on the set `info` keeps"""
    xs, flag, _ = rr.resect(p, x, info)
    perm = np.random.default_rng(3).permutation(p["nobs"])
    q = dict(p, cam_idx1=p["cam_idx1"][perm], pnt_idx1=p["pnt_idx1"][perm], pt2d=np.ascontiguousarray(p["pt2d"].reshape(-1, 2)[perm].ravel()))
    x2, flag2, _ = rr.resect(q, x, info[perm])
    assert np.array_equal(flag, flag2)
    done = flag == rr.DONE
    return xs, flag, float(pose_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max())


def run(ba, p, x, ransac, **kw):
    m = _model(ba, p)
    try:
        return ba.refine_cameras(m, x, resect=True, ransac=ransac, **kw)
    finally:
        m.close()


def sigma_of(inlier):
    return np.where(inlier, 1.0, np.inf)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_keyword_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_ransac_cameras", "ba_ransac_cameras_dev", "ba_ransac_sample"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header
    assert "typedef struct ba_ransac_opts { double threshold; int hypotheses, sample, refits, min_inliers; uint64_t seed; }" in " ".join(header.split())
    good = lib.RansacOpts(1.0, 0, 0, -1, 0, 0)
    tail = (None,) * 7
    assert L.ba_ransac_cameras(None, None, C.byref(good), -1, -1.0, -1.0, *tail) == 1 and b"null argument" in L.ba_last_error()
    assert L.ba_ransac_cameras_dev(None, None, C.byref(good), -1, -1.0, -1.0, *tail, None) == 1
    assert L.ba_ransac_cameras(None, None, None, -1, -1.0, -1.0, *tail) == 1 and b"options" in L.ba_last_error()
    # the options are checked first: every refusal of the header through the C entry, by its message
    for bad, word in ((dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=np.nan), b"threshold"),
                      (dict(threshold=np.inf), b"threshold"), (dict(hypotheses=4097), b"hypotheses"), (dict(sample=5), b"sample"),
                      (dict(sample=17), b"sample"), (dict(refits=9), b"refits"), (dict(min_inliers=5), b"min_inliers")):
        o = lib.RansacOpts(**dict(dict(threshold=1.0, hypotheses=0, sample=0, refits=-1, min_inliers=0, seed=0), **bad))
        for fn, extra in ((L.ba_ransac_cameras, ()), (L.ba_ransac_cameras_dev, (None,))):
            assert fn(None, None, C.byref(o), -1, -1.0, -1.0, *tail, *extra) == 1
            msg = L.ba_last_error()
            assert word in msg and b"ba_ransac_cameras" in msg, (bad, msg)
    pos, n = np.zeros(16, dtype=np.int64), C.c_int(0)
    for args in ((0, -1, 10, None, 6), (0, 0, -1, None, 6), (0, 0, 1 << 31, None, 6), (0, 0, 10, None, 5), (0, 0, 10, None, 17)):
        assert L.ba_ransac_sample(*args, lib.ptr(pos), C.byref(n)) == 1
    assert L.ba_ransac_sample(0, 0, 10, None, 6, None, C.byref(n)) == 1
    # the keyword
    kwd = ba.refine_cameras.__kwdefaults__
    assert kwd["ransac"] is None and kwd["resect"] is False
    x = np.zeros(3)
    with pytest.raises(ValueError, match="resect=True"):
        ba.refine_cameras(None, x, ransac=dict(threshold=1.0))
    for bad in (dict(), dict(threshold=0.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold="a"),
                dict(threshold=1.0, hypotheses=4097), dict(threshold=1.0, hypotheses=1.5), dict(threshold=1.0, sample=5),
                dict(threshold=1.0, sample=17), dict(threshold=1.0, refits=9), dict(threshold=1.0, min_inliers=5),
                dict(threshold=1.0, seed=-1), dict(threshold=1.0, seed=1 << 64), dict(threshold=1.0, sample=True),
                dict(threshold=1.0, tau=2.0), 4.0, [("threshold", 1.0)]):
        with pytest.raises(ValueError):
            ba.refine_cameras(None, x, resect=True, ransac=bad)
    o = lib.ransac_opts(dict(threshold=2.5, hypotheses=None, refits=None, seed=(1 << 64) - 1))
    assert (o.threshold, o.hypotheses, o.sample, o.refits, o.min_inliers, o.seed) == (2.5, 0, 0, -1, 0, (1 << 64) - 1)


def test_mix_vectors():
    assert nr.mix(0) == 0xE220A8397B1DCDAF
    assert nr.mix(nr.mix(0) ^ 1) == 0x08B4FDA8C892B50E


@pytest.mark.parametrize("degree", [6, 7, 64, 600])
def test_sampling_against_the_reference(ba, degree):
    """ba_ransac_sample (host only) against the Python integers of ransac_ref.sample: every degree with and without a `used` mask,
    over the hypotheses 0..199 of three seeds; degree 6 with two entries unused is void."""
    rng = np.random.default_rng(degree)
    masks = [None, rng.random(degree) < 0.7]
    if degree == 6:
        masks[1] = np.array([True, False, True, True, False, True])
    void = 0
    for seed in (0, 1, 0xFEDCBA9876543210):
        for used in masks:
            for h in range(200):
                for m in (6, 8) if degree > 7 else (6,):
                    want = nr.sample(seed, h, degree, used, m)
                    got = ba._lib.ransac_sample(seed, h, degree, m, used)
                    void += want is None
                    assert (got is None) == (want is None) and (want is None or list(got) == want), (seed, h, m)
                    if want is not None:
                        assert len(set(want)) == m and max(want) < degree and (used is None or used[want].all())
    if degree == 6:
        assert void == 3 * 200 and ba._lib.ransac_sample(0, 0, 6, 0, None) is not None
    # the first draw of hypothesis 0 under seed 0, from the two vectors of the header
    key = nr.mix(nr.mix(0) ^ 0)
    assert ba._lib.ransac_sample(0, 0, degree)[0] == ((nr.mix(key ^ 0) >> 32) * degree) >> 32


@pytest.mark.parametrize("kind", ["exact", "noisy"])
def test_reference_conditions(ba, kind):
    """What the device comparison rests on, asserted on the reference: the winner of every camera that does not fail is an
    all-inlier sample; every contaminated hypothesis scores at least 3 below it; no hypothesis has lambda_2 / lambda_12 within a
    factor 100 of the degeneracy threshold 1e-10; no used observation's residual under the final linear pose lies within 10 % of
    tau; the final mask is the truth (exact: already the winner's, which counts every true inlier; noisy: after at most one
    adopted refit).  exact: the same under the seeds 1 and 2; degree 5 and the 4-inlier camera fail as the header says."""
    p, base, outlier = form(ba, kind)
    cam0 = p["cam_idx1"] - 1
    truth = np.bincount(cam0, weights=(~outlier).astype(float), minlength=p["ncams"]).astype(int)
    for seed in ((0, 1, 2) if kind == "exact" else (FORMS[kind]["seed"], 1)):
        con = consensus(ba, kind, seed=seed)
        clean = clean_hypotheses(p, con, outlier)
        fails = truth < 6
        assert con["attempted"].all() and np.array_equal(con["failed"], fails)
        b = con["best_hyp"]
        good = np.flatnonzero(~fails)
        lead = [int(con["counts"][c, b[c]] - con["counts"][c][~clean[c]].max()) if (~clean[c]).any() else 999 for c in good]
        with np.errstate(invalid="ignore"):
            near = (con["ratio"] > 1e-12) & (con["ratio"] < 1e-8)
        print(f"{kind}, seed {seed}: winners {b}, clean hypotheses {clean.sum(1)}, lead over contaminated {lead}, contaminated max "
              f"{[int(con['counts'][c][~clean[c]].max()) if (~clean[c]).any() else -1 for c in range(p['ncams'])]}, adopted {con['adopted']}, "
              f"margin {con['margin'][good].min():.3f}, lambda_2 / lambda_12 {np.nanmin(con['ratio']):.1e} .. {np.nanmax(con['ratio']):.1e}")
        assert all(clean[c, b[c]] for c in good) and min(lead) >= 3 and not near.any()
        assert con["margin"][good].min() >= 0.1
        assert np.array_equal(con["inlier"][~fails[cam0]], ~outlier[~fails[cam0]]) and not con["inlier"][fails[cam0]].any()
        assert np.array_equal(con["n_inliers"][good], truth[good])
        if kind == "exact":
            assert all(con["counts"][c, b[c]] == truth[c] for c in good) and comparable(p, con, outlier)[good].all()
            assert (con["counts"][fails].max(axis=1) <= 3).all() and (con["counts"][0] == -1).all() and con["best_hyp"][0] == -1
            assert np.array_equal(con["n_inliers"][fails], np.maximum(con["counts"][fails].max(axis=1), 0))
        else:
            assert con["adopted"].max() <= 1


def test_add_outliers(ba):
    """exactly the flagged detections move, each by r_min..r_max; the counts per camera are as asked; the fraction form rounds down"""
    p = small_scene(ba)
    cam0 = p["cam_idx1"] - 1
    deg = np.bincount(cam0, minlength=p["ncams"])
    want = np.arange(p["ncams"]) % 5
    pt2d, out = ba.synthetic.add_outliers(p, n_per_camera=want, seed=3, r_min=100.0, r_max=500.0)
    d = np.linalg.norm(pt2d - p["pt2d"].reshape(-1, 2), axis=1)
    assert pt2d.shape == (p["nobs"], 2) and out.dtype == np.bool_ and np.array_equal(np.bincount(cam0[out], minlength=p["ncams"]), want)
    assert (d[~out] == 0).all() and (d[out] >= 100.0 * (1 - 1e-12)).all() and (d[out] <= 500.0 * (1 + 1e-12)).all()
    pt2, out2 = ba.synthetic.add_outliers(p, fraction=0.3, seed=3)
    assert np.array_equal(np.bincount(cam0[out2], minlength=p["ncams"]), np.floor(0.3 * deg).astype(int))
    again = ba.synthetic.add_outliers(p, fraction=0.3, seed=3)
    assert np.array_equal(pt2, again[0]) and np.array_equal(out2, again[1]) and not np.shares_memory(pt2, p["pt2d"])
    for bad in (dict(), dict(n_per_camera=1, fraction=0.1), dict(fraction=1.5), dict(n_per_camera=10 ** 6), dict(n_per_camera=1, r_min=5.0, r_max=1.0)):
        with pytest.raises(ValueError):
            ba.synthetic.add_outliers(p, **bad)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _compare_consensus(ba, p, info, con, sel):
    cam0 = p["cam_idx1"] - 1
    assert np.array_equal(info["inliers"][sel[cam0]], con["inlier"][sel[cam0]])
    assert np.array_equal(info["n_inliers"][sel], con["n_inliers"][sel]) and np.array_equal(info["best_hypothesis"][sel], con["best_hyp"][sel])
    assert np.array_equal((info["status"] == "degenerate")[sel], con["failed"][sel])


@pytest.mark.gpu
def test_exact_masks_and_linear_pose(ba, gpu_ok):
    """exact, max_iter = 0, refits = 0: the masks, counts, winners and states of the reference; the linear pose within the bound."""
    p, base, outlier = form(ba, "exact")
    x0 = nan_poses(p, base)
    con = consensus(ba, "exact")
    x, info = run(ba, p, x0, opts("exact"), max_iter=0)
    _compare_consensus(ba, p, info, con, np.ones(p["ncams"], dtype=bool))
    xs, flag, spread = linear_ref(p, x0, nr.masked_info(p, con["inlier"]))
    done = flag == rr.DONE
    assert np.array_equal(done, ~con["failed"]) and info["inliers"].dtype == np.bool_
    st_ref = cr.refine(p, np.where(np.isnan(xs), 1.0, xs), max_iter=0, info=nr.masked_info(p, con["inlier"]))[1]
    st = codes(ba, info)
    assert np.array_equal(st[done], st_ref[done]) and (st[~done] == cr.DEGENERATE).all()
    err = pose_err(cr.cameras(p, x), cr.cameras(p, xs))[done].max()
    bound = max(100 * spread, 1e-12)
    print(f"exact: linear pose {err:.3e} (bound {bound:.1e}), worst cost {info['cost_before'].max():.3e}")
    assert err <= bound
    Cd, C0 = cr.cameras(p, x), cr.cameras(p, x0)
    assert np.array_equal(bits(Cd[~done]), bits(C0[~done])) and (info["cost_before"][~done] == 0).all() and (info["cost_after"][~done] == 0).all()
    assert np.array_equal(bits(Cd[:, 6:]), bits(C0[:, 6:])) and np.array_equal(bits(x[:3 * p["npnts"]]), bits(x0[:3 * p["npnts"]]))
    assert info["counts"]["degenerate"] == 2 and info["counts"]["max_iter"] == 10 and info["iters_max"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 4, 5, 129])
def test_hypothesis_counts_around_a_workgroup(ba, gpu_ok, H):
    """H around the four waves of a workgroup: the cameras whose reference outcome rounding cannot change (comparable) are at least
    half of those attempted, and on them the device gives the reference's masks, counts, winners and states."""
    p, base, outlier = form(ba, "exact")
    con = consensus(ba, "exact", hypotheses=H)
    sel = comparable(p, con, outlier)
    print(f"H = {H}: {int(sel.sum())} of {int(con['attempted'].sum())} cameras compared, failed {np.flatnonzero(con['failed'])}")
    assert 2 * sel.sum() >= con["attempted"].sum()
    x, info = run(ba, p, nan_poses(p, base), opts("exact", hypotheses=H), max_iter=0)
    _compare_consensus(ba, p, info, con, sel)


@pytest.mark.gpu
def test_noisy_end_to_end(ba, gpu_ok):
    """noisy, refits = 2: the final mask is the truth; cost and parameters against the reference on the true inliers."""
    p, base, outlier = form(ba, "noisy")
    x0 = nan_poses(p, base)
    con = consensus(ba, "noisy")
    truth_info = nr.masked_info(p, ~outlier)
    x1, st1, cost1, tr1, D = rr.refine(p, x0, max_iter=MAX_ITER, xtol=XTOL_REF, info=truth_info)
    xp = np.array(base, copy=True)
    cr.cameras(p, xp)[:, :6] *= 1.0 + np.random.default_rng(1).normal(0.0, 1e-3, (p["ncams"], 6))
    x2, st2, cost2, _, _ = cr.refine(p, xp, max_iter=MAX_ITER, xtol=XTOL_REF, info=truth_info)
    assert ((st1 & 0x7F) == cr.CONVERGED).all() and np.array_equal(st1, st2)
    s1, s2 = float(rel_cost(cost2[:, 1], cost1).max()), float(scaled(D, cr.cameras(p, x2), cr.cameras(p, x1)).max())
    cost_bound, par_bound = max(100 * s1, 1e-13), max(10 * s2, 100 * XTOL)
    x, info = run(ba, p, x0, opts("noisy"), xtol=XTOL, max_iter=MAX_ITER)
    assert np.array_equal(info["inliers"], ~outlier) and np.array_equal(info["inliers"], con["inlier"])
    assert np.array_equal(info["n_inliers"], con["n_inliers"]) and np.array_equal(info["best_hypothesis"], con["best_hyp"])
    e_after, e_par = rel_cost(info["cost_after"], cost1).max(), scaled(D, cr.cameras(p, x), cr.cameras(p, x1)).max()
    print(f"noisy: spreads {s1:.3e}, {s2:.3e}; cost_after {e_after:.3e} (bound {cost_bound:.1e}), parameters {e_par:.3e} (bound {par_bound:.1e}), "
          f"trials {info['iters_max']} (reference {tr1.max()})")
    assert np.array_equal(codes(ba, info), st1) and e_after <= cost_bound and e_par <= par_bound
    assert (info["cost_after"] <= info["cost_before"]).all() and not info["behind"].any()


def _terms(ba, p, outlier, what):
    """keywords of refine_cameras for the bit-for-bit property"""
    if what == "huber":
        return dict(loss="huber", f_scale=2.0)
    if what == "cam_prior":
        pri = cam_prior_on(p, [1, p["ncams"] - 1], 7)
        return dict(camera_priors=(pri[0] + 1, pri[1], pri[2]))
    if what == "intrinsics":
        return dict(fixed_camera_params=("k1", "k2", "f"))
    if what == "obs_info":  # anisotropic sigma; ten true inliers of the largest camera dropped
        rng = np.random.default_rng(23)
        s = rng.uniform(0.5, 3.0, (p["nobs"], 2))
        last = np.flatnonzero((p["cam_idx1"] - 1 == p["ncams"] - 1) & ~outlier)
        s[last[::len(last) // 10][:10]] = np.inf
        return dict(obs_info=s)
    return {}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,what", [("exact", "plain"), ("noisy", "plain"), ("noisy", "huber"), ("noisy", "cam_prior"),
                                       ("noisy", "intrinsics"), ("noisy", "obs_info")])
def test_bits_of_the_resection_on_the_inliers(ba, gpu_ok, kind, what):
    """x, status and cost equal bit for bit those of refine_cameras(resect=True) with an obs_info that is the caller's on the returned
    inliers and inf elsewhere.  obs_info: the ten dropped inliers are neither sampled nor flagged, and the mask is still the truth."""
    p, base, outlier = form(ba, kind)
    x0 = nan_poses(p, base)
    kw = _terms(ba, p, outlier, what)
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, ransac=opts(kind), xtol=XTOL, max_iter=MAX_ITER, **kw)
        sig = np.array(kw["obs_info"], copy=True) if what == "obs_info" else np.ones((p["nobs"], 2))
        sig[~info["inliers"]] = np.inf
        y, iy = ba.refine_cameras(m, x0, resect=True, xtol=XTOL, max_iter=MAX_ITER, **dict(kw, obs_info=sig))
    finally:
        m.close()
    assert np.array_equal(bits(x), bits(y)) and np.array_equal(codes(ba, info), codes(ba, iy))
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key]), bits(iy[key]))
    assert info["iters_max"] == iy["iters_max"] and info["counts"] == iy["counts"]
    moved = np.isin(info["status"], ("converged", "max_iter", "stalled"))
    assert moved.sum() == (10 if kind == "exact" else 8) and np.isfinite(cr.cameras(p, x)[moved]).all()
    if what == "obs_info":
        dropped = np.isinf(kw["obs_info"]).all(axis=1)
        assert dropped.sum() == 10 and not info["inliers"][dropped].any() and np.array_equal(info["inliers"], ~outlier & ~dropped)
        con = nr.consensus(p, x0, info=ba._lib.obs_info_pack(kw["obs_info"])[:, [0, 1, 1, 2]].reshape(-1, 2, 2), **ref_kw(opts(kind)))
        assert np.array_equal(info["best_hypothesis"], con["best_hyp"]) and np.array_equal(info["inliers"], con["inlier"])
    else:
        assert np.array_equal(info["inliers"][moved[p["cam_idx1"] - 1]], ~outlier[moved[p["cam_idx1"] - 1]])


@pytest.mark.gpu
def test_cameras_that_are_not_attempted(ba, gpu_ok):
    """A camera with one pose component held starts from x with the bits of ba_refine_cameras, a fixed camera is FIXED: for both
    inlier = the used observations, best_hypothesis = -1.  Degree 5 and the 4-inlier camera: degenerate, bit-unchanged, NaN."""
    p, base, outlier = form(ba, "exact")
    nc = p["ncams"]
    cam0 = p["cam_idx1"] - 1
    held = np.zeros((nc, 9), dtype=bool)
    held[6, 1] = True  # degree 64
    held[8] = True     # degree 255
    from_x = held[:, :6].any(axis=1)
    x0 = nan_poses(p, base, ~from_x)
    kw = dict(fixed_camera_params=held, xtol=XTOL, max_iter=MAX_ITER)
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, ransac=opts("exact"), **kw)
        xp, ip = ba.refine_cameras(m, x0, resect=False, **kw)
    finally:
        m.close()
    Cd, Cp, C0 = cr.cameras(p, x), cr.cameras(p, xp), cr.cameras(p, x0)
    assert np.array_equal(bits(Cd[from_x]), bits(Cp[from_x])) and np.array_equal(codes(ba, info)[from_x], codes(ba, ip)[from_x])
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key][from_x]), bits(ip[key][from_x]))
    assert info["status"][8] == "fixed" and info["status"][6] != "degenerate" and (info["best_hypothesis"][from_x] == -1).all()
    assert info["inliers"][from_x[cam0]].all() and np.array_equal(info["n_inliers"][from_x], np.array(DEGREES)[from_x])
    fails = np.array([0, 4])
    assert (info["status"][fails] == "degenerate").all() and np.array_equal(bits(Cd[fails]), bits(C0[fails])) and np.isnan(Cd[fails, :6]).all()
    assert (info["cost_before"][fails] == 0).all() and (info["cost_after"][fails] == 0).all() and not info["behind"][fails].any()
    assert not info["inliers"][np.isin(cam0, fails)].any() and info["best_hypothesis"][0] == -1 and info["n_inliers"][0] == 0
    rest = ~from_x & ~np.isin(np.arange(nc), fails)
    assert (info["status"][rest] == "converged").all() and np.array_equal(info["inliers"][rest[cam0]], ~outlier[rest[cam0]])


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """Two calls, and the host and the device-resident entry, give the same bits; cameras of degree 12, 255 and 600 give the same
    bits alone as inside the scene; another seed gives the same masks on exact data; the next lm_step has the bits it has without
    the call; a communicator is refused with the entry's name."""
    p, base, outlier = form(ba, "noisy")
    nc, nvar, nobs = p["ncams"], len(base), p["nobs"]
    x0 = nan_poses(p, base)
    L, lib = ba._lib.lib(), ba._lib
    q = small_scene(ba)
    o = opts("noisy")
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    try:
        x1, i1 = ba.refine_cameras(m, x0, resect=True, ransac=o, xtol=XTOL, max_iter=MAX_ITER)
        x2, i2 = ba.refine_cameras(m, x0, resect=True, ransac=o, xtol=XTOL, max_iter=MAX_ITER)
        d = [C.c_void_p() for _ in range(6)]
        sizes = (8 * nvar, nc, 16 * nc, nobs, 4 * nc, 4 * nc)
        for ptr_, size in zip(d, sizes):
            lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        host = [x0.copy(), np.zeros(nc, dtype=np.uint8), np.zeros((nc, 2)), np.zeros(nobs, dtype=np.uint8), np.zeros(nc, dtype=np.int32),
                np.zeros(nc, dtype=np.int32)]
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        lib.check(L.ba_memcpy_h2d(m.handle, d[0], lib.ptr(host[0]), 8 * nvar))
        lib.check(L.ba_ransac_cameras_dev(m.handle, d[0], C.byref(lib.ransac_opts(o)), MAX_ITER, XTOL, -1.0, d[1], d[2], lib.ptr(counts),
                                          C.byref(its), d[3], d[4], d[5], None))
        for a, ptr_, size in zip(host, d, sizes):
            lib.check(L.ba_memcpy_d2h(m.handle, lib.ptr(a), ptr_, size))
            lib.check(L.ba_dev_free(m.handle, ptr_))
        alone = {}
        for c in (0, 4, nc - 1):  # degrees 12, 255 and 600
            pc = only_camera(p, c)
            alone[c] = run(ba, pc, nan_poses(pc, pc["x_true"]), o, xtol=XTOL, max_iter=MAX_ITER)
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.refine_cameras(ms, nan_poses(q, q["x0"]), resect=True, ransac=dict(threshold=4.0), xtol=XTOL)
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.refine_cameras(mc, x0, resect=True, ransac=o)
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_ransac_cameras" in str(e.value) and "communicator" in str(e.value)
    assert np.array_equal(bits(x1), bits(x2)) and np.array_equal(bits(x1), bits(host[0]))
    for key in ("cost_before", "cost_after", "inliers", "n_inliers", "best_hypothesis"):
        assert np.array_equal(i1[key], i2[key])
    assert np.array_equal(bits(i1["cost_before"]), bits(host[2][:, 0])) and np.array_equal(bits(i1["cost_after"]), bits(host[2][:, 1]))
    assert np.array_equal(codes(ba, i1), host[1]) and its.value == i1["iters_max"] and counts[0] == i1["counts"]["converged"]
    assert np.array_equal(i1["inliers"], host[3] != 0) and np.array_equal(i1["n_inliers"], host[4]) and np.array_equal(i1["best_hypothesis"], host[5])
    cam0 = p["cam_idx1"] - 1
    for c, (xa, ia) in alone.items():
        assert np.array_equal(bits(xa[-9:]), bits(cr.cameras(p, x1)[c])), c
        assert ia["cost_after"][0] == i1["cost_after"][c] and ia["cost_before"][0] == i1["cost_before"][c]
        assert np.array_equal(ia["inliers"], i1["inliers"][cam0 == c]) and ia["best_hypothesis"][0] == i1["best_hypothesis"][c]
    for a, b, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c_))
    pe, be, _ = form(ba, "exact")
    xe0 = nan_poses(pe, be)
    (_, ia), (_, ib) = (run(ba, pe, xe0, opts("exact", seed=s), max_iter=0) for s in (0, 1))
    assert np.array_equal(ia["inliers"], ib["inliers"]) and np.array_equal(ia["n_inliers"][[1, 2, 3] + list(range(5, 12))], ib["n_inliers"][[1, 2, 3] + list(range(5, 12))])
