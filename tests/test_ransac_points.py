"""Outlier-robust triangulation (ba_ransac_points, include/ba_hip.h; refine_points(triangulate=True, ransac=...)).
The reference is tests/helpers/points_ransac_ref.py: the header restated in numpy on top of points_ref (the rays, the 3 x 3 solve,
the refinement) and ransac_ref (mix, sample, masked_info).  The first tests need no device; the rest run on the GPU.

Scenes, the true cameras held and the point entries of x NaN (they are never read):
  tracks    make_problem(12, 80, 480, seed=7): degrees 2 to about 12, every point exhaustive at H = 128
  high      make_problem(100, 60, 2700, seed=11): degrees 14 to 100, both tiers of the kernel, exhaustive and sampled
  boundary  scene_from_degrees: 2, 3, 16, 17, 32, 33, 64, 65, 129 -- at H = 128 the exhaustive / sampled switch falls between 16
            and 17 (C(16,2) = 120, C(17,2) = 136), the tier switch between 32 and 33
Forms of tracks and high, 34 % of every track displaced by 100..500 px (synthetic.add_point_outliers, seed 1):
  noisy  the detections as generated (0.5 px Gaussian); tau = 4 px, refits 2
  exact  the detections re-projected from x_true; tau = 1 px, refits 0
The gap between 0.5 px of noise and 100 px outliers is what makes the masks insensitive to rounding; the conditions under which
the device can be held to the reference's masks are asserted on the reference first (test_reference_conditions).  The seeds were
chosen on the reference, never on the device."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import points_ransac_ref as qr  # noqa: E402
import points_ref as pr  # noqa: E402
import ransac_ref as nr  # noqa: E402
from refine_util import _model, bits, codes, small_scene  # noqa: E402
from scenes import random_info, scene_from_degrees  # noqa: E402

XTOL, XTOL_REF = 1e-10, 1e-13
FRACTION, OUTLIER_SEED = 0.34, 1
KINDS = {"noisy": dict(threshold=4.0, refits=2), "exact": dict(threshold=1.0, refits=0)}
BOUNDARY_DEGREES = (2, 3, 16, 17, 32, 33, 64, 65, 129)
BOUNDARY_H = (1, 3, 63, 64, 65, 128, 129)
TIER = 32  # PT_TIER of csrc/ba_point_kernels.hip
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def pts(p, x):
    return np.asarray(x)[:3 * p["npnts"]].reshape(-1, 3)


def scene(ba, name):
    def build():
        if name == "tracks":
            return ba.synthetic.make_problem(12, 80, 480, seed=7)
        if name == "high":
            return ba.synthetic.make_problem(100, 60, 2700, seed=11)
        if name == "boundary":
            return scene_from_degrees(ba, 140, BOUNDARY_DEGREES, 51)
        raise ValueError(name)
    return cached(("scene", name), build)


def reprojected(ba, p):
    xt = p["x_true"]
    cams = xt[3 * p["npnts"]:].reshape(-1, 9)
    return dict(p, pt2d=np.ascontiguousarray(ba.synthetic.project(pts(p, xt)[p["pnt_idx1"] - 1], cams[p["cam_idx1"] - 1]).ravel()))


def with_outliers(ba, p, **how):
    pt2d, out = ba.synthetic.add_point_outliers(p, seed=OUTLIER_SEED, **how)
    return dict(p, pt2d=np.ascontiguousarray(pt2d.ravel())), out


def form(ba, name, kind):
    """(the scene with the displaced detections, the boolean outlier mask)"""
    def build():
        p = scene(ba, name)
        return with_outliers(ba, reprojected(ba, p) if kind == "exact" else p, fraction=FRACTION)
    return cached(("form", name, kind), build)


def boundary(ba, wrong):
    """the boundary scene with 0, 1 or floor(d / 3) wrong detections per point (noisy detections)"""
    def build():
        p = scene(ba, "boundary")
        d = np.array(BOUNDARY_DEGREES)
        return with_outliers(ba, p, n_per_point={"none": 0 * d, "one": 0 * d + 1, "third": d // 3}[wrong])
    return cached(("boundary", wrong), build)


def start(p, fixed=None):
    """the true cameras; the free points NaN: they are never read"""
    x = np.array(p["x_true"], dtype=np.float64, copy=True)
    X = pts(p, x)
    X[np.ones(p["npnts"], dtype=bool) if fixed is None else ~np.asarray(fixed)] = np.nan
    return x


def opts(kind, **over):
    return dict(dict(KINDS[kind], hypotheses=128, seed=0), **over)


def ref_kw(o):
    return dict(threshold=o["threshold"], hypotheses=o.get("hypotheses", 0), refits=o.get("refits", -1), min_inliers=o.get("min_inliers", 0),
                seed=o.get("seed", 0))


def consensus(ba, name, kind):
    p, _ = form(ba, name, kind)
    return cached(("consensus", name, kind), lambda: qr.consensus(p, p["x_true"], **ref_kw(opts(kind))))


def truth_of(p, outlier):
    return np.bincount(p["pnt_idx1"] - 1, weights=(~outlier).astype(float), minlength=p["npnts"]).astype(int)


def comparable(p, con, outlier):
    """(the points whose outcome rounding cannot change: the winner is clean, counts every true inlier and leads every
    contaminated hypothesis by 2 or more; the smallest such lead)"""
    truth = truth_of(p, outlier)
    ok, lead = np.zeros(p["npnts"], dtype=bool), []
    for i in np.flatnonzero(con["attempted"] & ~con["failed"]):
        cnt, b = con["counts"][i], con["best_hyp"][i]
        clean = np.array([s is not None and not outlier[s].any() for s in con["samples"][i]])
        dirty = cnt[~clean]
        lead.append(int(cnt[b] - (dirty.max() if dirty.size else -1)))
        ok[i] = clean[b] and cnt[b] == truth[i] and lead[-1] >= 2
    return ok, min(lead)


def of_points(p, sel):
    """the observations of the selected points"""
    return np.asarray(sel)[p["pnt_idx1"] - 1]


def sigma_of(inlier):
    return np.where(inlier, 1.0, np.inf)


def run(ba, p, x, ransac, **kw):
    m = _model(ba, p)
    try:
        return ba.refine_points(m, x, triangulate=True, ransac=ransac, **kw)
    finally:
        m.close()


def winning_pair(con_or_info, p, i, H, seed=0, used=None):
    """the two observations of point i's winning hypothesis, from the rule of the header"""
    o = np.flatnonzero(p["pnt_idx1"] - 1 == i)
    d, h = len(o), int(con_or_info[i])
    if d * (d - 1) // 2 <= H:
        return o[qr.pairs_of(d)[h]]
    return o[nr.sample(seed, h, d, None if used is None else used[o], 2)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_keyword_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    for name in ("ba_ransac_points", "ba_ransac_points_dev"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header and f":{name}" in julia
    assert "function ransac_points!(" in julia
    good = lib.RansacOpts(1.0, 0, 0, -1, 0, 0)
    tail = (None,) * 7
    assert L.ba_ransac_points(None, None, C.byref(good), -1, -1.0, -1.0, *tail) == 1 and b"null argument" in L.ba_last_error()
    assert L.ba_ransac_points_dev(None, None, C.byref(good), -1, -1.0, -1.0, *tail, None) == 1
    assert L.ba_ransac_points(None, None, None, -1, -1.0, -1.0, *tail) == 1 and b"options" in L.ba_last_error()
    for bad, word in ((dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=np.nan), b"threshold"),
                      (dict(threshold=np.inf), b"threshold"), (dict(hypotheses=4097), b"hypotheses"), (dict(sample=3), b"sample"),
                      (dict(sample=1), b"sample"), (dict(refits=9), b"refits"), (dict(min_inliers=1), b"min_inliers")):
        o = lib.RansacOpts(**dict(dict(threshold=1.0, hypotheses=0, sample=0, refits=-1, min_inliers=0, seed=0), **bad))
        for fn, extra in ((L.ba_ransac_points, ()), (L.ba_ransac_points_dev, (None,))):
            assert fn(None, None, C.byref(o), -1, -1.0, -1.0, *tail, *extra) == 1
            msg = L.ba_last_error()
            assert word in msg and b"ba_ransac_points" in msg, (bad, msg)
    kwd = ba.refine_points.__kwdefaults__
    assert kwd["ransac"] is None and kwd["triangulate"] is False
    x = np.zeros(3)
    with pytest.raises(ValueError, match="triangulate=True"):
        ba.refine_points(None, x, ransac=dict(threshold=1.0))
    for bad in (dict(), dict(threshold=0.0), dict(threshold=-2.0), dict(threshold=float("nan")), dict(threshold=1.0, sample=3),
                dict(threshold=1.0, min_inliers=1), dict(threshold=1.0, hypotheses=4097), dict(threshold=1.0, refits=9),
                dict(threshold=1.0, tau=2.0), dict(threshold=1.0, seed=-1), 4.0):
        with pytest.raises(ValueError):
            ba.refine_points(None, x, triangulate=True, ransac=bad)
    o = lib.ransac_opts(dict(threshold=2.5, sample=2, min_inliers=3), least=2, most=2, least_set=2)
    assert (o.threshold, o.hypotheses, o.sample, o.refits, o.min_inliers, o.seed) == (2.5, 0, 2, -1, 3, 0)


def test_add_point_outliers(ba):
    """exactly the flagged detections move, each by r_min..r_max; the counts per point are as asked; the fraction form rounds
    down; add_outliers, which now shares the helper, returns the bits it returned before (sha256 recorded on the parent commit)"""
    p = small_scene(ba)
    pnt0 = p["pnt_idx1"] - 1
    deg = np.bincount(pnt0, minlength=p["npnts"])
    want = np.minimum(np.arange(p["npnts"]) % 3, deg)
    pt2d, out = ba.synthetic.add_point_outliers(p, n_per_point=want, seed=3, r_min=100.0, r_max=500.0)
    d = np.linalg.norm(pt2d - p["pt2d"].reshape(-1, 2), axis=1)
    assert pt2d.shape == (p["nobs"], 2) and out.dtype == np.bool_ and np.array_equal(np.bincount(pnt0[out], minlength=p["npnts"]), want)
    assert np.array_equal(bits(pt2d[~out]), bits(p["pt2d"].reshape(-1, 2)[~out]))
    assert (d[out] >= 100.0 * (1 - 1e-12)).all() and (d[out] <= 500.0 * (1 + 1e-12)).all()
    pt2, out2 = ba.synthetic.add_point_outliers(p, fraction=FRACTION, seed=3)
    assert np.array_equal(np.bincount(pnt0[out2], minlength=p["npnts"]), np.floor(FRACTION * deg).astype(int))
    again = ba.synthetic.add_point_outliers(p, fraction=FRACTION, seed=3)
    assert np.array_equal(pt2, again[0]) and np.array_equal(out2, again[1]) and not np.shares_memory(pt2, p["pt2d"])
    for bad in (dict(), dict(n_per_point=1, fraction=0.1), dict(fraction=1.5), dict(n_per_point=10 ** 6), dict(n_per_point=1, r_min=5.0, r_max=1.0)):
        with pytest.raises(ValueError):
            ba.synthetic.add_point_outliers(p, **bad)
    q = scene(ba, "tracks")
    a, b = ba.synthetic.add_outliers(q, fraction=0.3, seed=5)
    c, e = ba.synthetic.add_outliers(q, n_per_camera=3, seed=9, r_min=50, r_max=60)
    assert hashlib.sha256(a.tobytes() + b.tobytes() + c.tobytes() + e.tobytes()).hexdigest() == \
        "b808f7f7289ccb228a3aac5864ca9303a0ebccfce55be13c81a60490ce730b7a"


def test_unranking(ba):
    """the rank order of the header against np.triu_indices, and the sampling of two against ba_ransac_sample's rule"""
    assert [tuple(ab) for ab in qr.pairs_of(4)] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    used = np.array([True, False, True, True, False] * 4)
    for h in range(50):
        s = nr.sample(3, h, 20, used, 2)
        assert s is not None and len(set(s)) == 2 and used[s].all()
        key, taken = nr.mix(nr.mix(3) ^ h), []
        for j in range(64):
            pos = ((nr.mix(key ^ j) >> 32) * 20) >> 32
            if used[pos] and pos not in taken:
                taken.append(pos)
        assert s == taken[:2]


@pytest.mark.parametrize("kind", ["noisy", "exact"])
@pytest.mark.parametrize("name", ["tracks", "high"])
def test_reference_conditions(ba, name, kind):
    """What the device comparison rests on, asserted on the reference alone: it ends on the true inlier set for every attempted
    point with two true inliers or more; every such point is comparable (the winner is clean, counts every true inlier and leads
    every contaminated hypothesis by >= 2; at most 10 % may miss that); no used observation's residual under the final linear
    point lies within 10 % of tau.  Measured: tracks 80 of 80, lead 2, margin 0.64 (exact 1.0); high 60 of 60, lead 7, margin 0.48."""
    p, outlier = form(ba, name, kind)
    con = consensus(ba, name, kind)
    truth = truth_of(p, outlier)
    deg = np.bincount(p["pnt_idx1"] - 1, minlength=p["npnts"])
    assert con["attempted"].all() and (truth >= 2).all() and not con["failed"].any()
    if name == "high":
        assert all((deg == d).any() for d in (TIER, TIER + 1, 64, 65)) and (deg * (deg - 1) // 2 <= 128).any() and deg.max() == 100
    else:
        assert deg.min() == 2 and (deg * (deg - 1) // 2 <= 128).all()
    ok, lead = comparable(p, con, outlier)
    on_truth = np.array([np.array_equal(con["inlier"][p["pnt_idx1"] - 1 == i], ~outlier[p["pnt_idx1"] - 1 == i]) for i in range(p["npnts"])])
    print(f"{name} {kind}: on the true set {on_truth.sum()} of {p['npnts']}, comparable {ok.sum()}, smallest lead {lead}, smallest margin "
          f"{con['margin'].min():.2f}, adopted refits {con['adopted'].sum()}, outliers {outlier.sum()} of {p['nobs']}")
    assert on_truth.all() and np.array_equal(con["n_inliers"], truth)
    assert (~ok).sum() <= 0.1 * p["npnts"]
    assert con["margin"][ok].min() >= 0.1


@pytest.mark.parametrize("wrong", ["none", "one", "third"])
def test_reference_on_the_boundary_scene(ba, wrong):
    """the boundary scene on the reference, H = 128: the point of degree 2 with one wrong detection fails with a best count of 0;
    every other point ends on its true set; no residual under a final point lies within 10 % of tau"""
    p, outlier = boundary(ba, wrong)
    con = cached(("boundary-ref", wrong, 128), lambda: qr.consensus(p, p["x_true"], **ref_kw(opts("noisy"))))
    fails = truth_of(p, outlier) < 2
    assert np.array_equal(con["failed"], fails) and fails.sum() == (1 if wrong == "one" else 0)
    keep = of_points(p, ~fails)
    assert np.array_equal(con["inlier"][keep], ~outlier[keep]) and not con["inlier"][~keep].any()
    assert (con["n_inliers"][fails] == 0).all() and con["margin"][~fails].min() >= 0.1


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "noisy"])
@pytest.mark.parametrize("name", ["tracks", "high"])
def test_consensus_against_the_reference(ba, gpu_ok, name, kind):
    """masks, set sizes and winners equal to the reference's on every comparable point (the cap on the others is asserted on the
    reference first); the states equal; the points within 100 xtol (1 + |X_ref|) of the reference's finish run to xtol = 1e-13
    (the bound of test_refine_points._check_parity); the point entries of x are NaN"""
    p, outlier = form(ba, name, kind)
    o = opts(kind)
    con = consensus(ba, name, kind)
    ok, _ = comparable(p, con, outlier)
    assert (~ok).sum() <= 0.1 * p["npnts"]
    x0 = start(p)
    x, info = run(ba, p, x0, o, xtol=XTOL)
    info_ref = nr.masked_info(p, con["inlier"])
    _, st_ref, cost_ref, _ = pr.refine(p, p["x_true"], init=1, info=info_ref, xtol=XTOL)
    x_ref = pr.refine(p, p["x_true"], init=1, info=info_ref, xtol=XTOL_REF)[0]
    sel = of_points(p, ok)
    assert np.array_equal(info["inliers"][sel], con["inlier"][sel])
    assert np.array_equal(info["n_inliers"][ok], con["n_inliers"][ok]) and np.array_equal(info["best_hypothesis"][ok], con["best_hyp"][ok])
    assert np.array_equal(codes(ba, info)[ok], st_ref[ok]), (codes(ba, info), st_ref)
    err = np.linalg.norm(pts(p, x) - pts(p, x_ref), axis=1) / (1.0 + np.linalg.norm(pts(p, x_ref), axis=1))
    print(f"{name} {kind}: {ok.sum()} of {p['npnts']} comparable, max |X - X_ref| / (1 + |X_ref|) = {err[ok].max():.3e}, trials {info['iters_max']}")
    assert err[ok].max() <= 100 * XTOL
    assert np.allclose(info["cost_after"][ok], cost_ref[ok, 1], rtol=1e-8, atol=1e-12)
    assert np.array_equal(bits(x[3 * p["npnts"]:]), bits(x0[3 * p["npnts"]:]))
    assert sum(info["counts"][s] for s in ba._lib.POINT_STATES) == p["npnts"]


@pytest.mark.gpu
@pytest.mark.parametrize("wrong", ["none", "one", "third"])
def test_boundaries_of_the_enumeration_and_the_tiers(ba, gpu_ok, wrong):
    """degrees around the exhaustive / sampled switch and the tier switch, hypothesis counts around a wave's 64 lanes: every point
    gives the masks, the set sizes and the winners of the reference; degree 2 with one wrong detection fails"""
    p, outlier = boundary(ba, wrong)
    x0 = start(p)
    m = _model(ba, p)
    try:
        got = {H: ba.refine_points(m, x0, triangulate=True, ransac=opts("noisy", hypotheses=H), xtol=XTOL) for H in BOUNDARY_H}
    finally:
        m.close()
    for H in BOUNDARY_H:
        con = cached(("boundary-ref", wrong, H), lambda: qr.consensus(p, p["x_true"], **ref_kw(opts("noisy", hypotheses=H))))
        x, info = got[H]
        print(f"{wrong}, H = {H}: winners {info['best_hypothesis']}, sets {info['n_inliers']}, adopted {con['adopted']}, margin {con['margin'].min():.2e}")
        assert np.array_equal(info["inliers"], con["inlier"]), H
        assert np.array_equal(info["n_inliers"], con["n_inliers"]) and np.array_equal(info["best_hypothesis"], con["best_hyp"]), H
        assert np.array_equal(info["status"] == "degenerate", con["failed"]), H
        if wrong == "one":
            assert con["failed"][0] and info["n_inliers"][0] == 0 and info["status"][0] == "degenerate" and np.isnan(pts(p, x)[0]).all()
            assert info["cost_before"][0] == 0 and info["cost_after"][0] == 0 and not info["behind"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tracks", "high"])
def test_refits_that_are_adopted(ba, gpu_ok, name):
    """tau = 0.75 px against 0.5 px of noise: a pair's point leaves true inliers outside and the refits bring them in -- on the
    reference 1 point of tracks adopts one refit, 20 points of high adopt 27, 7 of them two (lane tier: the set in a register;
    wave tier: the set in the inlier bytes).  The device gives the reference's masks, sizes and winners on every point.  (No
    residual under a final point lies within 4e-4 tau of tau, measured on the reference; rounding moves one by 1e-12.)"""
    p, _ = form(ba, name, "noisy")
    o = opts("noisy", threshold=0.75)
    con = cached(("tight", name), lambda: qr.consensus(p, p["x_true"], **ref_kw(o)))
    con0 = cached(("tight0", name), lambda: qr.consensus(p, p["x_true"], **ref_kw(dict(o, refits=0))))
    assert con["adopted"].max() == (2 if name == "high" else 1) and con["margin"].min() >= 1e-4 and not con["failed"].any()
    assert con["n_inliers"].sum() > con0["n_inliers"].sum()
    _, info = run(ba, p, start(p), o, xtol=XTOL)
    _, info0 = run(ba, p, start(p), dict(o, refits=0), xtol=XTOL)
    print(f"{name}: adopted refits {con['adopted'].sum()}, set sizes {con0['n_inliers'].sum()} -> {con['n_inliers'].sum()}")
    for got, want in ((info, con), (info0, con0)):
        assert np.array_equal(got["inliers"], want["inlier"])
        assert np.array_equal(got["n_inliers"], want["n_inliers"]) and np.array_equal(got["best_hypothesis"], want["best_hyp"])


def _term(ba, p, what):
    rng = np.random.default_rng(17)
    if what == "huber":
        return dict(loss="huber", f_scale=0.5, max_iter=1000)
    if what == "prior":
        idx = np.array([2, 9, 30])
        mu = pts(p, p["x_true"])[idx] + rng.normal(0, 0.01, (len(idx), 3))
        A = rng.normal(0, 1, (len(idx), 3, 3))
        Lam = 4e4 * np.einsum("kij,klj->kil", A, A)
        return dict(point_priors=(idx + 1, mu, 0.5 * (Lam + Lam.transpose(0, 2, 1))))
    if what == "info":
        return dict(obs_info=random_info(p, 5))
    if what == "max_iter0":
        return dict(max_iter=0)
    return {}


@pytest.mark.gpu
@pytest.mark.parametrize("name,what", [("tracks", "plain"), ("high", "plain"), ("tracks", "huber"), ("tracks", "prior"), ("tracks", "info"),
                                       ("high", "info"), ("tracks", "max_iter0")])
def test_bits_of_the_finish(ba, gpu_ok, name, what):
    """x, status and cost are those of refine_points(triangulate=True) under an information that drops the returned outliers, bit
    for bit: plain, under a loss, with a point prior, with a caller's information (zeroed and rank-one entries among it: an
    unused observation is in no set and in no winning sample) and at max_iter = 0 (the linear triangulation on the set)"""
    p, outlier = form(ba, name, "noisy")
    kw = _term(ba, p, what)
    o = opts("noisy")
    x0 = start(p)
    m = _model(ba, p)
    try:
        x, info = ba.refine_points(m, x0, triangulate=True, ransac=o, xtol=XTOL, **kw)
        if what == "info":
            masked = np.array(kw["obs_info"], copy=True)
            masked[~info["inliers"]] = 0.0
        else:
            masked = sigma_of(info["inliers"])
        x2, info2 = ba.refine_points(m, x0, triangulate=True, xtol=XTOL, **dict(kw, obs_info=masked))
    finally:
        m.close()
    assert np.array_equal(bits(x), bits(x2)) and np.array_equal(codes(ba, info), codes(ba, info2))
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key]), bits(info2[key]))
    assert info["iters_max"] == info2["iters_max"] and info["counts"] == info2["counts"]
    if what == "max_iter0":
        assert (info["status"] == "max_iter").all() and info["iters_max"] == 0
    if what == "info":
        used = np.abs(kw["obs_info"]).reshape(p["nobs"], -1).max(axis=1) > 0
        assert (~used).any() and not info["inliers"][~used].any()
        for i in np.flatnonzero(info["best_hypothesis"] >= 0):
            assert used[winning_pair(info["best_hypothesis"], p, i, 128, used=used)].all(), i
        assert (info["best_hypothesis"] >= 0).sum() >= 0.9 * p["npnts"]
    else:  # an outlier raises no flag and the sets are the truth
        assert np.array_equal(info["inliers"], ~outlier) and not info["behind"].any()
        assert info["n_inliers"].min() >= 2 and not np.isnan(pts(p, x)).any()


@pytest.mark.gpu
def test_points_that_are_not_attempted_or_cannot_be(ba, gpu_ok):
    """fixed points: FIXED, bit-unchanged, their set is their used observations, best -1; a point without an observation, a point
    with one, and a point whose used observations number fewer than two: degenerate, bit-unchanged, no set, cost 0"""
    q = ba.synthetic.make_problem(5, 40, 80, seed=3)
    pnt = q["pnt_idx1"]
    keep = pnt != 8
    keep[np.flatnonzero(pnt == 21)[0]] = False  # point 8 (1-based) unobserved, point 21 seen once
    p = dict(q, cam_idx1=q["cam_idx1"][keep], pnt_idx1=pnt[keep], pt2d=np.ascontiguousarray(q["pt2d"].reshape(-1, 2)[keep].ravel()),
             nobs=int(keep.sum()))
    fx = np.zeros(p["npnts"], dtype=bool)
    fx[::9] = True
    sig = np.ones(p["nobs"])
    o12 = np.flatnonzero(p["pnt_idx1"] == 12)
    sig[o12[1:]] = np.inf  # point 12 keeps one used observation
    o1 = np.flatnonzero(p["pnt_idx1"] == 1)  # (fixed) one unused among its own
    sig[o1[0]] = np.inf
    x0 = start(p, fixed=fx)
    x, info = run(ba, p, x0, dict(threshold=4.0), fixed_points=fx, obs_info=sig, xtol=XTOL)
    pnt0 = p["pnt_idx1"] - 1
    deg_used = np.bincount(pnt0, weights=np.isfinite(sig).astype(float), minlength=p["npnts"]).astype(int)
    assert (info["status"][fx] == "fixed").all() and np.array_equal(bits(pts(p, x)[fx]), bits(pts(p, x0)[fx]))
    assert np.array_equal(info["n_inliers"][fx], deg_used[fx]) and (info["best_hypothesis"][fx] == -1).all()
    assert np.array_equal(info["inliers"][fx[pnt0]], np.isfinite(sig)[fx[pnt0]]) and not info["inliers"][o1[0]]
    for i in (7, 20, 11):
        assert not fx[i] and info["status"][i] == "degenerate" and info["n_inliers"][i] == 0 and info["best_hypothesis"][i] == -1, i
        assert np.isnan(pts(p, x)[i]).all() and info["cost_before"][i] == 0 and info["cost_after"][i] == 0 and not info["behind"][i]
        assert not info["inliers"][pnt0 == i].any()
    rest = ~fx
    rest[[7, 20, 11]] = False
    assert (info["status"][rest] == "converged").all() and (info["n_inliers"][rest] == 2).all() and (info["best_hypothesis"][rest] == 0).all()
    assert not info["inliers"][~np.isfinite(sig)].any()
    # a third view asked for, where every point has two: none is confirmed
    _, i3 = run(ba, p, x0, dict(threshold=4.0, min_inliers=3), fixed_points=fx, xtol=XTOL)
    assert (i3["status"][~fx] == "degenerate").all() and (i3["n_inliers"][rest] == 2).all() and not i3["inliers"][~fx[pnt0]].any()


@pytest.mark.gpu
def test_determinism_isolation_and_the_next_step(ba, gpu_ok):
    """Two calls, and the host and the device-resident entry, give the same bits; a point's outputs do not change when the other
    points' detections are corrupted; the cameras of x come back bit-identical; the next lm_step has the bits it has without
    the call"""
    p, outlier = form(ba, "high", "noisy")
    n, nvar, nobs = p["npnts"], len(p["x_true"]), p["nobs"]
    o = opts("noisy")
    x0 = start(p)
    L, lib = ba._lib.lib(), ba._lib
    q = small_scene(ba)
    watch = np.array([0, 17, n - 1])
    mine = of_points(p, np.isin(np.arange(n), watch))
    other = dict(p, pt2d=np.ascontiguousarray(np.where(mine[:, None], p["pt2d"].reshape(-1, 2), 7.0 - 3.0 * p["pt2d"].reshape(-1, 2)).ravel()))
    m, mo, ms, plain = _model(ba, p), _model(ba, other), _model(ba, q), _model(ba, q)
    try:
        x1, i1 = ba.refine_points(m, x0, triangulate=True, ransac=o, xtol=XTOL)
        x2, i2 = ba.refine_points(m, x0, triangulate=True, ransac=o, xtol=XTOL)
        x3, i3 = ba.refine_points(mo, x0, triangulate=True, ransac=o, xtol=XTOL)
        d = [C.c_void_p() for _ in range(6)]
        sizes = (8 * nvar, n, 16 * n, nobs, 4 * n, 4 * n)
        for ptr_, size in zip(d, sizes):
            lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        host = [x0.copy(), np.zeros(n, dtype=np.uint8), np.zeros((n, 2)), np.zeros(nobs, dtype=np.uint8), np.zeros(n, dtype=np.int32),
                np.zeros(n, dtype=np.int32)]
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        lib.check(L.ba_memcpy_h2d(m.handle, d[0], lib.ptr(host[0]), 8 * nvar))
        lib.check(L.ba_ransac_points_dev(m.handle, d[0], C.byref(lib.ransac_opts(o, least=2, most=2, least_set=2)), -1, XTOL, -1.0, d[1], d[2],
                                         lib.ptr(counts), C.byref(its), d[3], d[4], d[5], None))
        for a, ptr_, size in zip(host, d, sizes):
            lib.check(L.ba_memcpy_d2h(m.handle, lib.ptr(a), ptr_, size))
            lib.check(L.ba_dev_free(m.handle, ptr_))
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.refine_points(ms, start(q), triangulate=True, ransac=dict(threshold=4.0), xtol=XTOL)
        after = ba.lm_step(ms, q["x0"], 3.0)
    finally:
        for mm in (m, mo, ms, plain):
            mm.close()
    assert np.array_equal(bits(x1), bits(x2)) and np.array_equal(bits(x1), bits(host[0]))
    for key in ("cost_before", "cost_after", "inliers", "n_inliers", "best_hypothesis", "status", "behind"):
        assert np.array_equal(i1[key], i2[key])
    assert np.array_equal(bits(i1["cost_before"]), bits(host[2][:, 0])) and np.array_equal(bits(i1["cost_after"]), bits(host[2][:, 1]))
    assert np.array_equal(codes(ba, i1), host[1]) and its.value == i1["iters_max"] and counts[0] == i1["counts"]["converged"]
    assert np.array_equal(i1["inliers"], host[3] != 0) and np.array_equal(i1["n_inliers"], host[4]) and np.array_equal(i1["best_hypothesis"], host[5])
    assert np.array_equal(bits(x1[3 * n:]), bits(x0[3 * n:]))
    assert np.array_equal(bits(pts(p, x3)[watch]), bits(pts(p, x1)[watch])) and np.array_equal(i3["inliers"][mine], i1["inliers"][mine])
    for key in ("cost_before", "cost_after", "n_inliers", "best_hypothesis", "status"):
        assert np.array_equal(i3[key][watch], i1[key][watch])
    assert not np.array_equal(i3["inliers"][~mine], i1["inliers"][~mine])
    for a, b, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c_))


def _sigma_bound(p, keep):
    """per point 0.5 px x sqrt(trace (sum J'J)^-1) at the true point over the observations `keep`: the standard deviation the
    generator's 0.5 px Gaussian noise gives the point (Gauss-Newton covariance)"""
    info = np.tile(np.eye(2), (p["nobs"], 1, 1))
    info[~keep] = 0.0
    H = pr.evaluate(pr.Scene(p, p["x_true"], info), pts(p, p["x_true"]))[1]
    Hm = np.zeros((p["npnts"], 3, 3))
    for k, (i, j) in enumerate(pr._PACK):
        Hm[:, i, j] = Hm[:, j, i] = H[:, k]
    return 0.5 * np.sqrt(np.trace(np.linalg.inv(Hm), axis1=1, axis2=2))


@pytest.mark.gpu
def test_what_it_is_for(ba, gpu_ok):
    """The tracks scene at 34 % wrong detections per track.  Errors are |X - X_true|; a point's bound is 5 sigma_i, sigma_i the
    standard deviation 0.5 px of noise gives it on its true detections (_sigma_bound) -- the clean run's own errors reach
    2.4 sigma_i.  Measured on the reference (points_ref / points_ransac_ref) before any device ran:
      triangulate=True alone      median error 203 x the clean scene's (4.2e-1 against 2.1e-3), 72 of 80 points beyond 5 sigma
      ... under loss="cauchy"     median 1.3 x the clean scene's -- the loss pulls most points back, so the median does NOT
                                  stay above 10 x as it does under the linear loss -- but 2 points stay ruined, at 196 sigma_i
                                  (4.4 against a largest clean error of 2.0e-2), and nothing says which
      ransac=                     every point within 2.7 sigma_i, median 1.3 x the clean scene's (a third of the rays is gone)
    Asserted: the linear-loss median above 10 x the clean one; under cauchy a point beyond 100 sigma_i; with ransac= -- linear
    loss -- every point within 5 sigma_i."""
    p, outlier = form(ba, "tracks", "noisy")
    clean = scene(ba, "tracks")
    Xt = pts(p, p["x_true"])
    err = lambda x: np.linalg.norm(pts(p, x) - Xt, axis=1)  # noqa: E731
    x0 = start(p)
    m, mc = _model(ba, p), _model(ba, clean)
    try:
        e_clean = err(ba.refine_points(mc, x0, triangulate=True, xtol=XTOL)[0])
        e_plain = err(ba.refine_points(m, x0, triangulate=True, xtol=XTOL)[0])
        e_cauchy = err(ba.refine_points(m, x0, triangulate=True, loss="cauchy", xtol=XTOL)[0])
        x, info = ba.refine_points(m, x0, triangulate=True, ransac=opts("noisy"), xtol=XTOL)
    finally:
        m.close()
        mc.close()
    s_clean, s_in = _sigma_bound(clean, np.ones(p["nobs"], dtype=bool)), _sigma_bound(p, ~outlier)
    e = err(x)
    print(f"median error: clean {np.median(e_clean):.3e}, plain {np.median(e_plain):.3e}, cauchy {np.median(e_cauchy):.3e}, ransac {np.median(e):.3e}; "
          f"largest error / sigma: clean {(e_clean / s_clean).max():.2f}, plain {(e_plain / s_in).max():.1f}, cauchy {(e_cauchy / s_in).max():.1f}, "
          f"ransac {(e / s_in).max():.2f}")
    assert (e_clean <= 5 * s_clean).all()
    assert np.median(e_plain) > 10 * np.median(e_clean)
    assert (e_cauchy / s_in).max() > 100
    assert (e <= 5 * s_in).all() and np.array_equal(info["inliers"], ~outlier)
