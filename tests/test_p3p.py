"""P3P minimal samples for the consensus stage of the camera resection (ba_ransac_cameras_p3p, ba_p3p, include/ba_hip.h; DESIGN
§5r; refine_cameras(resect=True, ransac=..., minimal="p3p"), p3p).  The reference is tests/helpers/p3p_ref.py: the header
restated in numpy (np.roots where the kernel runs the Aberth-Ehrlich iteration) on top of ransac_ref's sampling, inlier test,
selection and refits.  The first tests need no device; the rest run on the GPU.

Scenes: isolated cameras (refine_util._isolated), the true points held, the pose entries NaN, the intrinsics true.
  triples  300 exact triples of three cameras of degree 300 (scene seed 69, draws of default_rng(1)).
  exact    the construction of test_ransac_cameras.py: degrees 5 .. 600 with its outliers (100..500 px), the other detections
           re-projected; tau = 1 px, refits = 0.  Degree 5 fails (fewer than six for the finish), and so does the camera that
           keeps 4 inliers of 12.
  high     degrees 64, 120, 200 with 65 % of the detections displaced (41, 78, 130), exact otherwise; H = 128, tau = 1 px.
  noisy    the cameras of test_ransac_cameras.py's noisy form: 0.5 px Gaussian on the other detections; tau = 4 px, refits = 2.
The seeds were chosen on the reference, never on the device; the conditions under which the device can be held to the
reference's masks are asserted on the reference first.

Bounds (from the reference alone).  Solver: 100 x the reference's own spread under the permutations of the three points,
measured here as 2.201e-12 (relative pose distance) on the comparable triples, so SOLVER_BOUND = 2.3e-10; a returned pose
reprojects its three points within the same bound.  Noisy form: the recipe of test_ransac_cameras.py (DESIGN §5m's table) --
cost 100 x spread with the floor 1e-13, parameters 10 x spread with the floor 100 xtol, re-measured here on the reference: the
spreads are 1.308e-14 and 3.016e-9, so the bounds are 1.3e-12 and 3.0e-8, the figures of the six-point form (no bound moved)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_run import attach_loopback, loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cameras_ref as cr  # noqa: E402
import p3p_ref as pr  # noqa: E402
import ransac_ref as nr  # noqa: E402
import resect_ref as rr  # noqa: E402
from block_ref import undistort  # noqa: E402
from refine_util import _isolated, _model, bits, codes, only_camera, rel_cost, scaled, small_scene  # noqa: E402

XTOL, XTOL_REF, MAX_ITER = 1e-10, 1e-13, 400
SCENE_SEED, OUTLIER_SEED = 69, 5
DEGREES = (5, 6, 7, 12, 12, 63, 64, 65, 255, 256, 257, 600)
OUTLIERS = (0, 0, 1, 3, 8, 19, 19, 20, 76, 77, 77, 180)
KEEP_NOISY = [3, 5, 6, 7, 8, 9, 10, 11]
HIGH_DEGREES, HIGH_OUTLIERS, HIGH_OUTLIER_SEED = (64, 120, 200), (41, 78, 130), 0
FORMS = {"exact": dict(degrees=DEGREES, outliers=OUTLIERS, tau=1.0, refits=0, seed=0, outlier_seed=OUTLIER_SEED),
         "high": dict(degrees=HIGH_DEGREES, outliers=HIGH_OUTLIERS, tau=1.0, refits=0, seed=0, outlier_seed=HIGH_OUTLIER_SEED),
         "noisy": dict(degrees=tuple(DEGREES[i] for i in KEEP_NOISY), outliers=tuple(OUTLIERS[i] for i in KEEP_NOISY), tau=4.0,
                       refits=2, seed=0, outlier_seed=OUTLIER_SEED)}
SOLVER_SPREAD, SOLVER_BOUND = 2.3e-12, 2.3e-10
N_TRIPLES = 300
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
        if kind != "noisy":
            n = p["npnts"]
            X, Cm = np.asarray(xt[:3 * n]).reshape(n, 3), cr.cameras(p, xt)
            p = dict(p, pt2d=np.ascontiguousarray(ba.synthetic.project(X[p["pnt_idx1"] - 1], Cm[p["cam_idx1"] - 1]).ravel()))
        pt2d, out = ba.synthetic.add_outliers(p, n_per_camera=np.array(f["outliers"]), seed=f["outlier_seed"])
        return dict(p, pt2d=np.ascontiguousarray(pt2d.ravel())), xt, out
    return cached(("form", kind), build)


def opts(kind, **over):
    f = FORMS[kind]
    return dict(dict(threshold=f["tau"], hypotheses=128, refits=f["refits"], seed=f["seed"]), **over)


def ref_kw(o):
    return dict(threshold=o["threshold"], hypotheses=o.get("hypotheses", 0), refits=o.get("refits", -1), min_inliers=o.get("min_inliers", 0),
                seed=o.get("seed", 0))


def consensus(ba, kind, **over):
    p, base, _ = form(ba, kind)
    return cached(("consensus", kind, tuple(sorted(over.items()))), lambda: pr.consensus(p, nan_poses(p, base), **ref_kw(opts(kind, **over))))


def clean_hypotheses(p, con, outlier):
    """(ncams, H) boolean: the hypothesis has a sample, and no outlier in it"""
    H = con["counts"].shape[1]
    return np.array([[s is not None and not outlier[s].any() for s in con["samples"][c]] for c in range(p["ncams"])]).reshape(p["ncams"], H)


def comparable(p, con, outlier, min_inliers=6):
    """(full, state): the cameras whose outcome rounding cannot change.  A clean hypothesis on exact data counts exactly the true
    inliers (residuals of 1e-9 px against tau = 1 px); only the count of a contaminated one can move with rounding.  A contaminated
    P3P hypothesis fits its own three points, so it scores at least 3 -- the rule stays: the winner is clean, counts every true
    inlier and leads every contaminated hypothesis by 3 or more (full: mask, count, winner and state are compared).  A camera
    that failed is compared on its state and mask when every contaminated hypothesis scores <= min_inliers - 3, and on its count
    and winner as well (full) when the best hypothesis is clean and leads the contaminated ones by 3 or more."""
    clean = clean_hypotheses(p, con, outlier)
    cam0 = p["cam_idx1"] - 1
    truth = np.bincount(cam0, weights=(~outlier).astype(float), minlength=p["ncams"]).astype(int)
    full, state = np.zeros(p["ncams"], dtype=bool), np.zeros(p["ncams"], dtype=bool)
    for c in np.flatnonzero(con["attempted"]):
        cnt = con["counts"][c]
        b = con["best_hyp"][c]
        dirty = cnt[~clean[c]]
        leads = b >= 0 and clean[c, b] and (dirty.size == 0 or dirty.max() <= cnt[b] - 3)
        if con["failed"][c]:
            state[c] = dirty.size == 0 or dirty.max() <= min_inliers - 3
            full[c] = state[c] and (leads or cnt.max() < 0)
        else:
            full[c] = state[c] = leads and cnt[b] == truth[c]
    return full, state


def pose_err(a, b):
    return np.linalg.norm(a - b, axis=-1) / (1.0 + np.linalg.norm(b, axis=-1))


def run(ba, p, x, ransac, minimal="p3p", **kw):
    m = _model(ba, p)
    try:
        return ba.refine_cameras(m, x, resect=True, ransac=ransac, minimal=minimal, **kw)
    finally:
        m.close()


def triples(ba):
    """(q (n, 3, 2), X (n, 3, 3), the true poses (n, 6)) of N_TRIPLES exact triples, then the constructed cases"""
    def build():
        p = _isolated(ba, (300,) * 3, SCENE_SEED)
        xt, n = p["x_true"], p["npnts"]
        X, Cm = np.asarray(xt[:3 * n]).reshape(n, 3), cr.cameras(p, xt)
        cam0, pnt0 = p["cam_idx1"] - 1, p["pnt_idx1"] - 1
        m = ba.synthetic.project(X[pnt0], Cm[cam0])
        rng = np.random.default_rng(1)
        q, XX, truth = [], [], []
        for i in range(N_TRIPLES):
            c = i % 3
            s = rng.choice(np.flatnonzero(cam0 == c), 3, replace=False)
            q.append(undistort(m[s], *Cm[c, 6:]))
            XX.append(X[pnt0[s]])
            truth.append(Cm[c, :6])
        return np.array(q), np.array(XX), np.array(truth)
    return cached("triples", build)


def constructed():
    """(q, X, n_sol expected or None) of the constructed cases: collinear, two equal points, a NaN entry, a plane parallel to the image"""
    q0 = np.array([[0.1, 0.05], [-0.2, 0.1], [0.05, -0.15]])
    line = np.array([[0.0, 0.0, -5.0], [1.0, 1.0, -6.0], [2.0, 2.0, -7.0]])
    equal = np.array([[0.0, 0.0, -5.0], [0.0, 0.0, -5.0], [1.0, 0.0, -5.0]])
    nan = np.array([[0.0, 0.0, -5.0], [1.0, np.nan, -6.0], [2.0, 0.0, -7.0]])
    # the camera at the identity pose (r = (1e-12, 0, 0)), the three points in the plane z = -4: q = -X.xy / X.z
    flat = np.array([[0.4, 0.2, -4.0], [-0.8, 0.4, -4.0], [0.2, -0.6, -4.0]])
    qflat = -flat[:, :2] / flat[:, 2:3]
    return np.array([q0, q0, q0, qflat]), np.array([line, equal, nan, flat]), [0, 0, 0, None]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_keyword_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    for name in ("ba_ransac_cameras_p3p", "ba_ransac_cameras_p3p_dev", "ba_p3p"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header and f"(:{name}, libba)" in julia
    assert "function ransac_cameras_p3p!(" in julia and "function p3p(" in julia and "p3p" in ba.__all__
    good = lib.RansacOpts(1.0, 0, 0, -1, 0, 0)
    tail = (None,) * 7
    assert L.ba_ransac_cameras_p3p(None, None, C.byref(good), -1, -1.0, -1.0, *tail) == 1 and b"null argument" in L.ba_last_error()
    assert L.ba_ransac_cameras_p3p_dev(None, None, C.byref(good), -1, -1.0, -1.0, *tail, None) == 1
    for fn, extra in ((L.ba_ransac_cameras_p3p, ()), (L.ba_ransac_cameras_p3p_dev, (None,))):
        assert fn(None, None, None, -1, -1.0, -1.0, *tail, *extra) == 1
        assert b"null options" in L.ba_last_error() and b"ba_ransac_cameras_p3p" in L.ba_last_error()
    for bad, word in ((dict(sample=2), b"sample must be 3"), (dict(sample=4), b"sample must be 3"), (dict(sample=6), b"sample must be 3"),
                      (dict(min_inliers=5), b"min_inliers must be >= 6"), (dict(hypotheses=4097), b"hypotheses"), (dict(refits=9), b"refits"),
                      (dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=np.nan), b"threshold"),
                      (dict(threshold=np.inf), b"threshold")):
        o = lib.RansacOpts(**dict(dict(threshold=1.0, hypotheses=0, sample=0, refits=-1, min_inliers=0, seed=0), **bad))
        for fn, extra in ((L.ba_ransac_cameras_p3p, ()), (L.ba_ransac_cameras_p3p_dev, (None,))):
            assert fn(None, None, C.byref(o), -1, -1.0, -1.0, *tail, *extra) == 1
            msg = L.ba_last_error()
            assert word in msg and b"ba_ransac_cameras_p3p" in msg, (bad, msg)
    for o in (lib.RansacOpts(1.0, 0, 3, -1, 6, 0), good):  # (accepted: the next refusal is the null handle)
        assert L.ba_ransac_cameras_p3p(None, None, C.byref(o), -1, -1.0, -1.0, *tail) == 1 and b"null argument" in L.ba_last_error()
    assert L.ba_p3p(None, 0, None, None, None, None) == 1 and b"ba_p3p" in L.ba_last_error()
    # ba_ransac_sample keeps refusing m < 6
    pos, n = np.zeros(16, dtype=np.int64), C.c_int(0)
    assert L.ba_ransac_sample(0, 0, 10, None, 3, lib.ptr(pos), C.byref(n)) == 1
    # the keyword
    kwd = ba.refine_cameras.__kwdefaults__
    assert kwd["minimal"] is None and kwd["ransac"] is None
    x = np.zeros(3)
    for kw, word in ((dict(minimal="p3p"), "needs resect=True"), (dict(minimal="p3p", resect=True), "ransac="),
                     (dict(minimal="p3p", ransac=dict(threshold=1.0)), "needs resect=True"),
                     (dict(minimal="p3p", resect=True, estimate_focal=True, ransac=dict(threshold=1.0)), "estimate_focal"),
                     (dict(minimal="p4p", resect=True, ransac=dict(threshold=1.0)), "minimal must be"),
                     (dict(minimal=True, resect=True, ransac=dict(threshold=1.0)), "minimal must be"),
                     (dict(minimal=3, resect=True, ransac=dict(threshold=1.0)), "minimal must be"),
                     (dict(minimal="p3p", resect=True, ransac=dict(threshold=1.0, sample=6)), "sample must be 3"),
                     (dict(minimal="p3p", resect=True, ransac=dict(threshold=1.0, sample=2)), "sample must be 3"),
                     (dict(minimal="p3p", resect=True, ransac=dict(threshold=1.0, min_inliers=5)), "min_inliers must be >= 6"),
                     (dict(minimal="p3p", resect=True, ransac=dict(threshold=0.0)), "threshold"),
                     (dict(resect=True, ransac=dict(threshold=1, sample=5)), "sample must lie in 6..16"),
                     (dict(resect=True, ransac=dict(threshold=1, sample=3)), "sample must lie in 6..16")):
        with pytest.raises(ValueError, match=word):
            ba.refine_cameras(None, x, **kw)
    o = lib.ransac_opts(dict(threshold=2.0, sample=3, min_inliers=6), least=3, most=3, least_set=6)
    assert (o.sample, o.min_inliers) == (3, 6)
    for bad in ((np.zeros((2, 3, 3)), np.zeros((2, 3, 3))), (np.zeros((2, 3, 2)), np.zeros((3, 3, 3))), (np.zeros((3, 2)), np.zeros((3, 3)))):
        with pytest.raises(ValueError, match="p3p"):
            ba.p3p(None, *bad)


def test_reference_against_itself(ba):
    """On exact triples the true pose is among the reference's solutions; at most 5 % of the triples are not comparable; on the
    comparable ones the reference's result does not change under a permutation of the three points beyond SOLVER_SPREAD; the
    constructed degenerate cases have no solution and the fronto-parallel one holds its true pose."""
    q, X, truth = triples(ba)
    worst, spread, comp = 0.0, 0.0, 0
    for i in range(N_TRIPLES):
        s = pr.solve(q[i], X[i])
        assert 1 <= len(s) <= 4
        worst = max(worst, pose_err(s, truth[i]).min())
        if not pr.comparable_triple(q[i], X[i]):
            continue
        comp += 1
        for perm in ([1, 2, 0], [2, 0, 1], [1, 0, 2]):
            s2 = pr.solve(q[i][perm], X[i][perm])
            assert len(s2) == len(s)
            spread = max(spread, max(pose_err(s2, a).min() for a in s))
    print(f"true pose among the solutions within {worst:.3e}; {comp} of {N_TRIPLES} comparable; spread under permutation {spread:.3e}")
    assert worst <= 1e-9 and comp >= 0.95 * N_TRIPLES and spread <= SOLVER_SPREAD
    cq, cX, want = constructed()
    for qq, XX, n in zip(cq, cX, want):
        s = pr.solve(qq, XX)
        if n is not None:
            assert len(s) == n
        else:
            ident = np.array([1e-12, 0, 0, 0, 0, 0])
            assert len(s) >= 1 and np.abs(s - ident).max(axis=1).min() <= 1e-9


def test_high_outlier_scene_condition(ba):
    """Why the feature exists: at 65 % displaced detections and H = 128, ransac_ref.sample gives no all-inlier sample of 6 for any
    of the three cameras and at least two of 3 (the sample of 3 is the prefix of the sample of 6 for the same (seed, h)).  The
    six-point reference therefore does not return the true mask for any camera, and the P3P reference returns it for all."""
    p, base, outlier = form(ba, "high")
    cam0 = p["cam_idx1"] - 1
    o = opts("high")
    assert np.array_equal(np.bincount(cam0[outlier]), HIGH_OUTLIERS) and all(k >= 0.64 * d for k, d in zip(HIGH_OUTLIERS, HIGH_DEGREES))
    clean = {3: [], 6: []}
    for c, d in enumerate(HIGH_DEGREES):
        out_c = outlier[cam0 == c]
        for m in (3, 6):
            samples = [nr.sample(o["seed"], h, d, None, m) for h in range(o["hypotheses"])]
            assert all(s is not None for s in samples)
            clean[m].append(sum(not out_c[s].any() for s in samples))
        assert all(nr.sample(o["seed"], h, d, None, 6)[:3] == nr.sample(o["seed"], h, d, None, 3) for h in range(o["hypotheses"]))
    print(f"clean samples among {o['hypotheses']} hypotheses: of 6 {clean[6]}, of 3 {clean[3]}")
    assert max(clean[6]) == 0 and min(clean[3]) >= 2
    six = cached("six", lambda: nr.consensus(p, nan_poses(p, base), threshold=o["threshold"], hypotheses=o["hypotheses"], sample_size=6,
                                             refits=o["refits"], seed=o["seed"]))
    con = consensus(ba, "high")
    for c in range(p["ncams"]):
        assert not np.array_equal(six["inlier"][cam0 == c], ~outlier[cam0 == c])
    assert np.array_equal(con["inlier"], ~outlier) and not con["failed"].any() and comparable(p, con, outlier)[0].all()


@pytest.mark.parametrize("kind", ["exact", "noisy"])
def test_reference_conditions(ba, kind):
    """What the device comparison rests on, asserted on the P3P reference: the winner of every camera that does not fail is an
    all-inlier sample and leads every contaminated hypothesis by 3 or more; no used observation's residual under the final linear
    pose lies within 10 % of tau; the final mask is the truth (noisy: after the refits).  exact: degree 5 and the 4-inlier camera
    fail, every other camera is comparable."""
    p, base, outlier = form(ba, kind)
    cam0 = p["cam_idx1"] - 1
    truth = np.bincount(cam0, weights=(~outlier).astype(float), minlength=p["ncams"]).astype(int)
    con = consensus(ba, kind)
    clean = clean_hypotheses(p, con, outlier)
    fails = truth < 6
    assert con["attempted"].all() and np.array_equal(con["failed"], fails)
    b = con["best_hyp"]
    good = np.flatnonzero(~fails)
    lead = [int(con["counts"][c, b[c]] - con["counts"][c][~clean[c]].max()) if (~clean[c]).any() else 999 for c in good]
    print(f"{kind}: winners {b}, clean hypotheses {clean.sum(1)}, lead over contaminated {lead}, adopted {con['adopted']}, "
          f"margin {con['margin'][good].min():.3f}, candidates per hypothesis {np.bincount(con['n_cand'].ravel())}")
    assert all(clean[c, b[c]] for c in good) and min(lead) >= 3
    assert con["margin"][good].min() >= 0.1
    assert np.array_equal(con["inlier"][~fails[cam0]], ~outlier[~fails[cam0]]) and not con["inlier"][fails[cam0]].any()
    assert np.array_equal(con["n_inliers"][good], truth[good])
    if kind == "exact":
        full, state = comparable(p, con, outlier)
        assert full[good].all() and state.all() and full[0] and con["failed"][0] and con["best_hyp"][0] >= 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_solver_alone(ba, gpu_ok):
    """ba_p3p on the 300 exact triples and the constructed cases: on the comparable triples n_sol and the poses, in their order,
    are the reference's within SOLVER_BOUND; every returned pose reprojects its three points within the bound, in front; the
    degenerate cases have no solution; one problem alone gives the bits it has inside the batch; two calls give the same bits."""
    q, X, truth = triples(ba)
    cq, cX, want = constructed()
    allq, allX = np.concatenate([q, cq]), np.concatenate([X, cX])
    m = _model(ba, small_scene(ba))
    try:
        poses, n_sol = ba.p3p(m, allq, allX)
        again = ba.p3p(m, allq, allX)
        alone = [ba.p3p(m, allq[i:i + 1], allX[i:i + 1]) for i in (0, 7, N_TRIPLES + 3)]
        empty = ba.p3p(m, np.zeros((0, 3, 2)), np.zeros((0, 3, 3)))
    finally:
        m.close()
    assert poses.shape == (len(allq), 4, 6) and n_sol.dtype == np.int32 and empty[0].shape == (0, 4, 6)
    assert np.array_equal(bits(poses), bits(again[0])) and np.array_equal(n_sol, again[1])
    for i, (pa, na) in zip((0, 7, N_TRIPLES + 3), alone):
        assert np.array_equal(bits(pa[0]), bits(poses[i])) and na[0] == n_sol[i]
    worst, reproj, comp = 0.0, 0.0, 0
    for i in range(len(allq)):
        n = n_sol[i]
        assert 0 <= n <= 4 and np.isfinite(poses[i, :n]).all() and np.isnan(poses[i, n:]).all()
        for s in range(n):
            qq, z = pr.project_q(poses[i, s], allX[i])
            assert (z < 0).all()
            reproj = max(reproj, np.abs(qq - allq[i]).max())
        if i < N_TRIPLES and pr.comparable_triple(q[i], X[i]):
            comp += 1
            ref = pr.solve(q[i], X[i])
            assert n == len(ref), (i, n, len(ref))
            worst = max(worst, pose_err(poses[i, :n], ref).max())
            assert pose_err(poses[i, :n], truth[i]).min() <= 1e-9
    print(f"{comp} of {N_TRIPLES} compared: poses {worst:.3e}, reprojection {reproj:.3e} (bound {SOLVER_BOUND:.1e})")
    assert comp >= 0.95 * N_TRIPLES and worst <= SOLVER_BOUND and reproj <= SOLVER_BOUND
    assert list(n_sol[N_TRIPLES:N_TRIPLES + 3]) == [0, 0, 0] and n_sol[N_TRIPLES + 3] >= 1
    ident = np.array([1e-12, 0, 0, 0, 0, 0])
    assert np.abs(poses[N_TRIPLES + 3, :n_sol[N_TRIPLES + 3]] - ident).max(axis=1).min() <= 1e-9


def _compare_consensus(p, info, con, full, state):
    cam0 = p["cam_idx1"] - 1
    assert np.array_equal(info["inliers"][state[cam0]], con["inlier"][state[cam0]])
    assert np.array_equal((info["status"] == "degenerate")[state], con["failed"][state])
    assert np.array_equal(info["n_inliers"][full], con["n_inliers"][full]) and np.array_equal(info["best_hypothesis"][full], con["best_hyp"][full])


@pytest.mark.gpu
@pytest.mark.parametrize("H", [128, 1, 3, 4, 5, 129])
def test_exact_masks(ba, gpu_ok, H):
    """exact, max_iter = 0, refits = 0, H = 128 and around the four waves of a workgroup: on the comparable cameras (at H = 128
    every one but the 4-inlier camera, whose count of 4 does not lead the contaminated hypotheses' 3) the masks, counts, winners
    and states of the reference, on every camera its mask and state; degree 5 fails."""
    p, base, outlier = form(ba, "exact")
    con = consensus(ba, "exact", hypotheses=H)
    full, state = comparable(p, con, outlier)
    print(f"H = {H}: {int(full.sum())} / {int(state.sum())} of {int(con['attempted'].sum())} cameras compared, failed {np.flatnonzero(con['failed'])}")
    assert state.all() and (full.sum() == 11 and not full[4] if H >= 128 else full.sum() >= 4)  # (H = 1: one hypothesis, clean for 4 cameras)
    x0 = nan_poses(p, base)
    x, info = run(ba, p, x0, opts("exact", hypotheses=H), max_iter=0)
    _compare_consensus(p, info, con, full, state)
    assert info["status"][0] == "degenerate" and np.array_equal(bits(cr.cameras(p, x)[0]), bits(cr.cameras(p, x0)[0]))
    if H == 128:
        done = ~con["failed"]
        assert np.isfinite(cr.cameras(p, x)[done]).all() and info["counts"]["degenerate"] == 2 and info["iters_max"] == 0


@pytest.mark.gpu
def test_high_outlier_ratio(ba, gpu_ok):
    """65 % displaced detections, H = 128: minimal="p3p" returns the true mask and CONVERGED for every camera, where the six-point
    hypotheses hold no clean sample (asserted on the reference in test_high_outlier_scene_condition)."""
    p, base, outlier = form(ba, "high")
    con = consensus(ba, "high")
    assert np.array_equal(con["inlier"], ~outlier) and comparable(p, con, outlier)[0].all()
    x, info = run(ba, p, nan_poses(p, base), opts("high"), xtol=XTOL, max_iter=MAX_ITER)
    assert np.array_equal(info["inliers"], ~outlier) and (info["status"] == "converged").all()
    _compare_consensus(p, info, con, np.ones(p["ncams"], dtype=bool), np.ones(p["ncams"], dtype=bool))
    err = pose_err(cr.cameras(p, x)[:, :6], cr.cameras(p, base)[:, :6]).max()
    print(f"high: pose against the truth {err:.3e}")
    assert err <= 1e-8


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
    assert np.array_equal(info["n_inliers"], con["n_inliers"])
    e_after, e_par = rel_cost(info["cost_after"], cost1).max(), scaled(D, cr.cameras(p, x), cr.cameras(p, x1)).max()
    print(f"noisy: spreads {s1:.3e}, {s2:.3e}; cost_after {e_after:.3e} (bound {cost_bound:.1e}), parameters {e_par:.3e} (bound {par_bound:.1e}), "
          f"trials {info['iters_max']} (reference {tr1.max()})")
    assert np.array_equal(codes(ba, info), st1) and e_after <= cost_bound and e_par <= par_bound
    assert (info["cost_after"] <= info["cost_before"]).all() and not info["behind"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,what", [("exact", "plain"), ("noisy", "plain"), ("noisy", "huber"), ("noisy", "intrinsics")])
def test_bits_of_the_resection_on_the_inliers(ba, gpu_ok, kind, what):
    """x, status and cost equal bit for bit those of refine_cameras(resect=True, obs_info=sigma) with sigma = 1 on the returned
    inliers and inf elsewhere: plain, with Huber, and with held intrinsics."""
    p, base, outlier = form(ba, kind)
    x0 = nan_poses(p, base)
    kw = dict(huber=dict(loss="huber", f_scale=2.0), intrinsics=dict(fixed_camera_params=("k1", "k2", "f"))).get(what, {})
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, ransac=opts(kind), minimal="p3p", xtol=XTOL, max_iter=MAX_ITER, **kw)
        sig = np.where(info["inliers"][:, None], 1.0, np.inf) * np.ones((p["nobs"], 2))
        y, iy = ba.refine_cameras(m, x0, resect=True, xtol=XTOL, max_iter=MAX_ITER, **dict(kw, obs_info=sig))
    finally:
        m.close()
    assert np.array_equal(bits(x), bits(y)) and np.array_equal(codes(ba, info), codes(ba, iy))
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key]), bits(iy[key]))
    assert info["iters_max"] == iy["iters_max"] and info["counts"] == iy["counts"]
    moved = np.isin(info["status"], ("converged", "max_iter", "stalled"))
    assert moved.sum() == (10 if kind == "exact" else 8) and np.isfinite(cr.cameras(p, x)[moved]).all()
    assert np.array_equal(info["inliers"][moved[p["cam_idx1"] - 1]], ~outlier[moved[p["cam_idx1"] - 1]])


@pytest.mark.gpu
def test_cameras_that_are_not_attempted(ba, gpu_ok):
    """A camera with one pose component held starts from x with the bits of ba_refine_cameras, a fixed camera is FIXED: for both
    inlier = the used observations, best_hypothesis = -1.  A camera whose f is NaN is degenerate and bit-unchanged."""
    p, base, outlier = form(ba, "exact")
    nc = p["ncams"]
    cam0 = p["cam_idx1"] - 1
    held = np.zeros((nc, 9), dtype=bool)
    held[6, 1] = True  # degree 64
    held[8] = True     # degree 255
    from_x = held[:, :6].any(axis=1)
    x0 = nan_poses(p, base, ~from_x)
    cr.cameras(p, x0)[9, 8] = np.nan  # degree 256: no focal length
    kw = dict(fixed_camera_params=held, xtol=XTOL, max_iter=MAX_ITER)
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, ransac=opts("exact"), minimal="p3p", **kw)
        xp, ip = ba.refine_cameras(m, x0, resect=False, **kw)
    finally:
        m.close()
    Cd, Cp, C0 = cr.cameras(p, x), cr.cameras(p, xp), cr.cameras(p, x0)
    assert np.array_equal(bits(Cd[from_x]), bits(Cp[from_x])) and np.array_equal(codes(ba, info)[from_x], codes(ba, ip)[from_x])
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key][from_x]), bits(ip[key][from_x]))
    assert info["status"][8] == "fixed" and info["status"][6] != "degenerate" and (info["best_hypothesis"][from_x] == -1).all()
    assert info["inliers"][from_x[cam0]].all() and np.array_equal(info["n_inliers"][from_x], np.array(DEGREES)[from_x])
    fails = np.array([0, 4, 9])
    assert (info["status"][fails] == "degenerate").all() and np.array_equal(bits(Cd[fails]), bits(C0[fails])) and np.isnan(Cd[fails, :6]).all()
    assert (info["cost_before"][fails] == 0).all() and (info["cost_after"][fails] == 0).all() and not info["behind"][fails].any()
    assert not info["inliers"][np.isin(cam0, fails)].any() and info["best_hypothesis"][9] == -1 and info["n_inliers"][9] == 0
    rest = ~from_x & ~np.isin(np.arange(nc), fails)
    assert (info["status"][rest] == "converged").all() and np.array_equal(info["inliers"][rest[cam0]], ~outlier[rest[cam0]])


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """Two calls, and the host and the device-resident entry, give the same bits; cameras of degree 12, 255 and 600 give the same
    bits alone as inside the scene; the next lm_step has the bits it has without the call; a communicator is refused with the
    entry's name, and ba_p3p runs on such a handle."""
    p, base, outlier = form(ba, "noisy")
    nc, nvar, nobs = p["ncams"], len(base), p["nobs"]
    x0 = nan_poses(p, base)
    L, lib = ba._lib.lib(), ba._lib
    q = small_scene(ba)
    o = opts("noisy")
    tq, tX, _ = triples(ba)
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    try:
        x1, i1 = ba.refine_cameras(m, x0, resect=True, ransac=o, minimal="p3p", xtol=XTOL, max_iter=MAX_ITER)
        x2, i2 = ba.refine_cameras(m, x0, resect=True, ransac=o, minimal="p3p", xtol=XTOL, max_iter=MAX_ITER)
        d = [C.c_void_p() for _ in range(6)]
        sizes = (8 * nvar, nc, 16 * nc, nobs, 4 * nc, 4 * nc)
        for ptr_, size in zip(d, sizes):
            lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        host = [x0.copy(), np.zeros(nc, dtype=np.uint8), np.zeros((nc, 2)), np.zeros(nobs, dtype=np.uint8), np.zeros(nc, dtype=np.int32),
                np.zeros(nc, dtype=np.int32)]
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        lib.check(L.ba_memcpy_h2d(m.handle, d[0], lib.ptr(host[0]), 8 * nvar))
        lib.check(L.ba_ransac_cameras_p3p_dev(m.handle, d[0], C.byref(lib.ransac_opts(o, least=3, most=3, least_set=6)), MAX_ITER, XTOL, -1.0,
                                              d[1], d[2], lib.ptr(counts), C.byref(its), d[3], d[4], d[5], None))
        for a, ptr_, size in zip(host, d, sizes):
            lib.check(L.ba_memcpy_d2h(m.handle, lib.ptr(a), ptr_, size))
            lib.check(L.ba_dev_free(m.handle, ptr_))
        alone = {}
        for c in (0, 4, nc - 1):  # degrees 12, 255 and 600
            pc = only_camera(p, c)
            alone[c] = run(ba, pc, nan_poses(pc, pc["x_true"]), o, xtol=XTOL, max_iter=MAX_ITER)
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.refine_cameras(ms, nan_poses(q, q["x0"]), resect=True, ransac=dict(threshold=4.0), minimal="p3p", xtol=XTOL)
        ba.p3p(ms, tq[:5], tX[:5])
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.refine_cameras(mc, x0, resect=True, ransac=o, minimal="p3p")
                with_comm = ba.p3p(mc, tq[:5], tX[:5])
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_ransac_cameras_p3p" in str(e.value) and "communicator" in str(e.value) and (with_comm[1] >= 1).all()
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
