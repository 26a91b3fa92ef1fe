"""Relative pose of camera pairs (ba_pair_matches, ba_relative_pose, include/ba_hip.h; pair_matches, relative_pose and
compose_relative of the package).  The reference is tests/helpers/pair_ref.py: the header restated in numpy (np.linalg.eigh and
svd where the kernels run Jacobi sweeps).  The first tests need no device; the rest run on the GPU.

Scenes: pair k is the cameras (2k, 2k + 1) of the generator's geometry (unit ball seen from distance 5..7); they share exactly
n_k points, each camera sees 5 points of its own, and the observations are shuffled, so the matches are not index-aligned.
  exact  n_k = 7, 8, 9, 63, 64, 65, 255, 256, 257, 600 (the wave and workgroup boundaries of the strided passes); the detections
         re-projected; 0, 0, 0, 20, 20, 21, 78, 78, 78, 181 detections of camera 2k + 1 displaced by 100..500 px
         (synthetic.add_outliers: about 30 % of the matches); tau = 1 px, refits = 0.  7 matches: FEW_MATCHES.
  noisy  the seven pairs with n_k >= 63, as many outliers, the other detections re-projected + 0.05 px Gaussian; tau = 2 px, up to
         4 refits.  (On this narrow field the eight-point fit is only a start on noisy data, a property of the method: the
         reference ends on the true set for 5 and 6 of the 7 pairs at 0.05 px (the two seeds used here) and for 2 to 4 at 0.1 px,
         whatever the refits.)
"Truth" for a mask is the set of used matches that pass the inlier test under the TRUE relative pose, not "the undisplaced
ones": a displacement along the epipolar line leaves a wrong match consistent.  The conditions under which the device can be
held to the reference's masks are asserted on the reference first (test_reference_conditions).  Seeds, noise level and tau were
chosen on the reference, never on the device.

Bounds (from the reference alone): a pose -- |R - R_ref|_F + |t - t_ref| within 100 x the reference's own spread under a
permutation of the set's matches, floor 1e-12 (the recipe of test_resect_cameras); the seeded points -- 100 x the spread of the
reference's own pipeline under that permutation, floor 1e-10."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_run import attach_loopback, loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_ref as br  # noqa: E402
import pair_ref as pf  # noqa: E402
import points_ref as ptr_ref  # noqa: E402
import resect_ref as rr  # noqa: E402
from refine_util import _model, bits, small_scene  # noqa: E402
from scenes import _scene_from_lists  # noqa: E402

COUNTS = (7, 8, 9, 63, 64, 65, 255, 256, 257, 600)
OUTLIERS = (0, 0, 0, 20, 20, 21, 78, 78, 78, 181)
KEEP_NOISY = [3, 4, 5, 6, 7, 8, 9]
OWN = 5
SCENE_SEED, NOISE_SEED = 42, 9
FORMS = {"exact": dict(keep=list(range(len(COUNTS))), tau=1.0, refits=0, sigma=0.0, outlier_seed=5),
         "noisy": dict(keep=KEEP_NOISY, tau=2.0, refits=4, sigma=0.05, outlier_seed=6)}
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def pair_scene(ba, counts, seed, twice=False):
    """the scene of the module's header for the shared counts `counts` (twice: camera 0 observes its first shared point a
    second time, later in its list)"""
    cam0, pnt0, base = [], [], 0
    for k, n in enumerate(counts):
        for c, ids in ((2 * k, range(base, base + n + OWN)), (2 * k + 1, list(range(base, base + n)) + list(range(base + n + OWN, base + n + 2 * OWN)))):
            cam0 += [c] * len(ids)
            pnt0 += list(ids)
        base += n + 2 * OWN
    if twice:
        cam0.append(0)
        pnt0.append(0)
    perm = np.random.default_rng(seed).permutation(len(cam0))
    cam0, pnt0 = np.array(cam0, dtype=np.int64)[perm], np.array(pnt0, dtype=np.int64)[perm]
    p = _scene_from_lists(ba, 2 * len(counts), base, pnt0, cam0, seed)
    n = p["npnts"]
    X, Cm = p["x_true"][:3 * n].reshape(n, 3), pf.cameras(p, p["x_true"])
    return dict(p, pt2d=np.ascontiguousarray(ba.synthetic.project(X[pnt0], Cm[cam0]).ravel()))


def pairs_of(p):
    return np.stack([np.arange(1, p["ncams"], 2), np.arange(2, p["ncams"] + 1, 2)], axis=1).astype(np.int64)


def form(ba, kind):
    """(problem with noise and outliers in pt2d, x with the true intrinsics and NaN elsewhere, the pairs (1-based))"""
    def build():
        f = FORMS[kind]
        p = pair_scene(ba, [COUNTS[i] for i in f["keep"]], SCENE_SEED)
        pt2d = p["pt2d"].reshape(-1, 2) + np.random.default_rng(NOISE_SEED).normal(0.0, 1.0, (p["nobs"], 2)) * f["sigma"]
        per_cam = np.zeros(p["ncams"], dtype=np.int64)
        per_cam[1::2] = [OUTLIERS[i] for i in f["keep"]]
        pt2d, _ = ba.synthetic.add_outliers(dict(p, pt2d=pt2d.ravel()), n_per_camera=per_cam, seed=f["outlier_seed"])
        return dict(p, pt2d=np.ascontiguousarray(pt2d.ravel())), intrinsics_only(p), pairs_of(p)
    return cached(("form", kind), build)


def intrinsics_only(p):
    x = np.full(len(p["x_true"]), np.nan)
    pf.cameras(p, x)[:, 6:] = pf.cameras(p, p["x_true"])[:, 6:]
    return x


def opts(kind, **over):
    f = FORMS[kind]
    return dict(dict(threshold=f["tau"], hypotheses=128, sample=8, refits=f["refits"], seed=0), **over)


def ref_kw(o):
    return dict(threshold=o["threshold"], hypotheses=o.get("hypotheses", 0), sample_size=o.get("sample", 0), refits=o.get("refits", -1),
                min_inliers=o.get("min_inliers", 0), seed=o.get("seed", 0))


def reference(ba, kind, **over):
    p, x, pairs = form(ba, kind)
    return cached(("reference", kind, tuple(sorted(over.items()))), lambda: pf.relative_pose(p, x, pairs, **ref_kw(opts(kind, **over))))


def truth(ba, kind):
    """per match: it is used and passes the inlier test under the true relative pose"""
    def build():
        p, x, pairs = form(ba, kind)
        ptr, _, _, data = pf.rays(p, x, pairs)
        out = np.zeros(ptr[-1], dtype=bool)
        for k, (qa, qb, used, fa, fb) in enumerate(data):
            R, t, _ = pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)
            out[ptr[k]:ptr[k + 1]] = pf.inliers(rr.rotation_vector(R), t, qa, qb, used, fa, fb, FORMS[kind]["tau"])
        return out
    return cached(("truth", kind), build)


def clean_hypotheses(con, tr):
    """(npairs, H) boolean: the hypothesis has a sample, and every match of it is in the truth"""
    n, H = con["counts"].shape
    ptr = con["match_ptr"]
    return np.array([[s is not None and tr[ptr[k] + s].all() for s in con["samples"][k]] for k in range(n)]).reshape(n, H)


def comparable(con, tr, min_inliers=8):
    """the pairs whose outcome rounding cannot change: too few matches; or no consensus with every count <= min_inliers - 3; or the
    winner is an all-inlier sample that counts the whole truth and leads every contaminated hypothesis by 3 or more (a
    contaminated hypothesis whose cheirality vote was won by less than 3 is taken at the largest count any of its four candidates
    reaches), the cheirality votes of the all-inlier hypotheses, the refits and the final fit were won by 3 or more, and no
    lambda_2 / lambda_9 lies within a factor 100 of 1e-10.  Or, where refits grow the set (noisy data: no sample counts the whole
    truth), the chain from the winner on is stable: the winner leads every other hypothesis by 3 or more (each at the largest count
    it could reach), its vote and those of the refits and the final fit were won by 3 or more, and under the winner's pose and
    every refit's pose no used match lies within 1e-4 tau of tau -- four orders above what 100 x the spread of a fit (1e-8 at
    most) can move a distance."""
    clean = clean_hypotheses(con, tr)
    ptr = con["match_ptr"]
    ok = np.zeros(len(con["status"]), dtype=bool)
    with np.errstate(invalid="ignore"):
        near = ((con["ratio"] > 1e-12) & (con["ratio"] < 1e-8)).any(axis=1) if con["ratio"].shape[1] else np.zeros(len(ok), dtype=bool)
    for k, st in enumerate(con["status"]):
        cnt, hi = con["counts"][k], con["counts_hi"][k]
        if st == pf.FEW_MATCHES:
            ok[k] = True
        elif st == pf.NO_CONSENSUS:
            ok[k] = hi.max() <= min_inliers - 3 and not near[k]
        elif st == pf.OK:
            b, dirty = con["best_hyp"][k], hi[~clean[k]]
            by_truth = (clean[k, b] and cnt[b] == tr[ptr[k]:ptr[k + 1]].sum() and (dirty.size == 0 or dirty.max() <= cnt[b] - 3)
                        and con["hyp_lead"][k][clean[k]].min() >= 3)
            by_chain = con["runner_lead"][k] >= 3 and con["hyp_lead"][k, b] >= 3 and con["chain_margin"][k] >= 1e-4
            final = np.array_equal(con["inlier"][ptr[k]:ptr[k + 1]], tr[ptr[k]:ptr[k + 1]])  # the final mask is the truth
            ok[k] = (by_truth or by_chain) and final and con["lead"][k] >= 3 and con["margin"][k] >= 0.1 and not near[k]
    return ok


def fit_spread(con, p, x, pairs, k, seed=3):
    """the reference's linear fit on pair k's final set against itself with the matches permuted: the pose error, and both poses"""
    _, _, _, data = pf.rays(p, x, pairs[[k]])
    qa, qb = data[0][0], data[0][1]
    M = np.flatnonzero(con["inlier"][con["match_ptr"][k]:con["match_ptr"][k + 1]])
    perm = np.random.default_rng(seed).permutation(len(M))
    r1, t1, _ = pf.linear_fit(qa[M], qb[M])
    r2, t2, _ = pf.linear_fit(qa[M[perm]], qb[M[perm]])
    return float(pf.pose_error(r1, t1, r2, t2)[0]), (r2, t2)


def run(ba, p, x, pairs, ransac, **kw):
    m = _model(ba, p)
    try:
        return ba.relative_pose(m, x, pairs, ransac=ransac, **kw)
    finally:
        m.close()


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_pair_matches", "ba_relative_pose"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header
    assert "enum { BA_RP_OK = 0, BA_RP_FEW_MATCHES = 1, BA_RP_DEGENERATE = 2, BA_RP_NO_CONSENSUS = 3, BA_RP_STATES = 4 };" in header
    for word in ("five-point", "only a start", "lambda_2 <= 1e-10 lambda_9", "communicator"):
        assert word in header
    assert lib.PAIR_STATES == ("ok", "few_matches", "degenerate", "no_consensus")
    good = lib.RansacOpts(1.0, 0, 0, -1, 0, 0)
    tail = (None,) * 7
    assert L.ba_relative_pose(None, None, 0, None, None, C.byref(good), *tail) == 1
    assert b"ba_relative_pose" in L.ba_last_error() and b"null argument" in L.ba_last_error()
    assert L.ba_relative_pose(None, None, 0, None, None, None, *tail) == 1 and b"null argument" in L.ba_last_error()
    # the options are checked first: every refusal of the header through the C entry, by its message
    for bad, word in ((dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=np.nan), b"threshold"),
                      (dict(threshold=np.inf), b"threshold"), (dict(hypotheses=4097), b"hypotheses"), (dict(sample=7), b"sample"),
                      (dict(sample=17), b"sample"), (dict(refits=9), b"refits"), (dict(min_inliers=7), b"min_inliers")):
        o = lib.RansacOpts(**dict(dict(threshold=1.0, hypotheses=0, sample=0, refits=-1, min_inliers=0, seed=0), **bad))
        assert L.ba_relative_pose(None, None, 0, None, None, C.byref(o), *tail) == 1
        msg = L.ba_last_error()
        assert word in msg and b"ba_relative_pose" in msg, (bad, msg)
    # Python: ValueError before any device call (the model is never touched: None stands in for it)
    kwd = ba.relative_pose.__kwdefaults__
    assert kwd == dict(ransac=None, obs_info=None)
    x = np.zeros(3)
    for bad in (dict(), dict(threshold=0.0), dict(threshold=float("nan")), dict(threshold="a"), dict(threshold=1.0, hypotheses=4097),
                dict(threshold=1.0, sample=7), dict(threshold=1.0, sample=6), dict(threshold=1.0, sample=17), dict(threshold=1.0, refits=9),
                dict(threshold=1.0, min_inliers=7), dict(threshold=1.0, seed=-1), dict(threshold=1.0, tau=2.0), 4.0):
        with pytest.raises(ValueError):
            ba.relative_pose(None, x, [[1, 2]], ransac=bad)
    with pytest.raises(ValueError, match="obs_info"):
        ba.relative_pose(None, x, [[1, 2]], obs_info=np.array([-1.0]))
    p = small_scene(ba)

    class Sizes:  # what relative_pose reads of a model before it calls the library
        ncams, npnts, nobs = p["ncams"], p["npnts"], p["nobs"]
    for bad in ([[1, 1]], [[0, 2]], [[1, p["ncams"] + 1]], [1, 2], [[1.0, 2.0]], [[1, 2, 3]]):
        with pytest.raises(ValueError, match="pair"):
            ba.relative_pose(Sizes, x, bad)
        with pytest.raises(ValueError, match="pair"):
            ba.pair_matches(p, bad)
    o = lib.ransac_opts(dict(threshold=2.5, sample=8, min_inliers=8), least=8)
    assert (o.threshold, o.hypotheses, o.sample, o.refits, o.min_inliers, o.seed) == (2.5, 0, 8, -1, 8, 0)
    assert lib.ransac_opts(dict(threshold=1.0, sample=6)).sample == 6  # (the resection's range is unchanged)


def test_pair_matches_against_dictionaries(ba):
    """ba_pair_matches (host only) against the dictionary walk of pair_ref.matches: the scenes of this module, a camera that
    observes a point twice, a pair that shares nothing, (a, b) against (b, a), a repeated pair, the counting form, the refusals."""
    L, lib = ba._lib.lib(), ba._lib
    p = pair_scene(ba, COUNTS, SCENE_SEED, twice=True)
    nc = p["ncams"]
    pairs = np.concatenate([pairs_of(p), pairs_of(p)[:, ::-1], [[1, 4], [2, 1], [2, 1], [nc, 1]]]).astype(np.int64)
    mp, oa, ob = ba.pair_matches(p, pairs)
    rp, ra, rb = pf.matches(p, pairs)
    assert np.array_equal(mp, rp) and np.array_equal(oa, ra) and np.array_equal(ob, rb)
    n = len(COUNTS)
    assert np.array_equal(np.diff(mp)[:n], COUNTS) and np.array_equal(np.diff(mp)[n:2 * n], COUNTS) and np.diff(mp)[2 * n] == 0
    cam0, pnt0 = p["cam_idx1"] - 1, p["pnt_idx1"] - 1
    for k, (a, b) in enumerate(pairs - 1):
        ia, ib = oa[mp[k]:mp[k + 1]], ob[mp[k]:mp[k + 1]]
        assert (cam0[ia] == a).all() and (cam0[ib] == b).all() and np.array_equal(pnt0[ia], pnt0[ib])
        assert (np.diff(ia) > 0).all() and len(set(pnt0[ia])) == len(ia)  # ordered by a's list; a point gives one match
    # the point camera 0 observes twice: its first observation is the match, in both directions
    twice = np.flatnonzero((cam0 == 0) & (pnt0 == 0))
    assert len(twice) == 2 and twice[0] in oa[mp[0]:mp[1]] and twice[1] not in oa and twice[0] in ob[mp[n]:mp[n + 1]] and twice[1] not in ob
    # (a, b) against (b, a): the same point set, ordered by the other list
    fwd, bwd = slice(mp[3], mp[4]), slice(mp[n + 3], mp[n + 4])
    assert set(zip(oa[fwd], ob[fwd])) == set(zip(ob[bwd], oa[bwd])) and not np.array_equal(oa[fwd], ob[bwd])
    assert np.array_equal(oa[mp[-4]:mp[-3]], oa[mp[-3]:mp[-2]])  # a pair may repeat
    # a model gives what its arrays give; the counting form; no pair at all
    cam, pnt = np.ascontiguousarray(p["cam_idx1"], dtype=np.int64), np.ascontiguousarray(p["pnt_idx1"], dtype=np.int64)
    a1, b1 = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    cnt = np.zeros(len(pairs) + 1, dtype=np.int64)
    args = (nc, p["npnts"], p["nobs"], lib.ptr(cam), lib.ptr(pnt))
    assert L.ba_pair_matches(*args, len(pairs), lib.ptr(a1), lib.ptr(b1), lib.ptr(cnt), None, None) == 0 and np.array_equal(cnt, mp)
    one = np.full(1, -1, dtype=np.int64)
    assert L.ba_pair_matches(*args, 0, None, None, lib.ptr(one), None, None) == 0 and one[0] == 0
    # every refusal
    two = np.zeros(2, dtype=np.int64)
    buf = np.zeros(mp[-1], dtype=np.int64)
    for a, b in ((1, 1), (0, 2), (1, nc + 1), (nc + 1, 1)):
        pa, pb = np.array([a], dtype=np.int64), np.array([b], dtype=np.int64)
        assert L.ba_pair_matches(*args, 1, lib.ptr(pa), lib.ptr(pb), lib.ptr(two), None, None) == 1 and b"ba_pair_matches" in L.ba_last_error()
    pa, pb = np.array([1], dtype=np.int64), np.array([2], dtype=np.int64)
    good = (1, lib.ptr(pa), lib.ptr(pb))
    assert L.ba_pair_matches(*args, *good, None, None, None) == 1
    assert L.ba_pair_matches(*args, 1, None, lib.ptr(pb), lib.ptr(two), None, None) == 1
    assert L.ba_pair_matches(*args, 1, lib.ptr(pa), None, lib.ptr(two), None, None) == 1
    assert L.ba_pair_matches(*args, *good, lib.ptr(two), lib.ptr(buf), None) == 1
    assert L.ba_pair_matches(*args, *good, lib.ptr(two), None, lib.ptr(buf)) == 1
    assert L.ba_pair_matches(nc, p["npnts"], p["nobs"], None, lib.ptr(pnt), *good, lib.ptr(two), None, None) == 1
    assert L.ba_pair_matches(nc, p["npnts"], p["nobs"], lib.ptr(cam), None, *good, lib.ptr(two), None, None) == 1
    assert L.ba_pair_matches(nc, p["npnts"], -1, lib.ptr(cam), lib.ptr(pnt), *good, lib.ptr(two), None, None) == 1
    assert L.ba_pair_matches(nc - 1, p["npnts"], p["nobs"], lib.ptr(cam), lib.ptr(pnt), *good, lib.ptr(two), None, None) == 1  # (a camera index out of range)
    assert L.ba_pair_matches(nc, p["npnts"] - 1, p["nobs"], lib.ptr(cam), lib.ptr(pnt), *good, lib.ptr(two), None, None) == 1
    assert L.ba_pair_matches(*args, *good, lib.ptr(two), None, None) == 0 and two[1] == COUNTS[0]


@pytest.mark.parametrize("kind", ["exact", "noisy"])
def test_reference_conditions(ba, kind):
    """What the device comparison rests on, asserted on pair_ref alone: the winner of every pair that does not fail is an
    all-inlier sample; every contaminated hypothesis scores at least 3 below it; no hypothesis has lambda_2 / lambda_9 within a
    factor 100 of 1e-10; the winning cheirality candidate leads the runner-up by at least 3 on every compared set; no used match
    has a Sampson distance within 10 % of tau under the final pose; the final mask is the truth.  exact: the seeds 0, 1, 2, every
    pair comparable at H = 128, 7 matches FEW_MATCHES; noisy: two seeds, at least half of the pairs comparable."""
    p, x, pairs = form(ba, kind)
    tr = truth(ba, kind)
    for seed in ((0, 1, 2) if kind == "exact" else (0, 1)):
        con = reference(ba, kind, seed=seed)
        ptr = con["match_ptr"]
        clean = clean_hypotheses(con, tr)
        good = np.flatnonzero(con["status"] == pf.OK)
        b = con["best_hyp"]
        lead = [int(con["counts"][k, b[k]] - con["counts_hi"][k][~clean[k]].max()) if (~clean[k]).any() else 999 for k in good]
        with np.errstate(invalid="ignore"):
            near = (con["ratio"] > 1e-12) & (con["ratio"] < 1e-8)
        sel = comparable(con, tr)
        print(f"{kind}, seed {seed}: states {con['status']}, winners {b}, clean hypotheses {clean.sum(1)}, lead over contaminated {lead}, "
              f"cheirality lead {con['lead']}, adopted {con['adopted']}, margin {con['margin'][good].min():.3f}, lambda_2 / lambda_9 "
              f"{np.nanmin(con['ratio']):.1e} .. {np.nanmax(con['ratio']):.1e}, comparable {int(sel.sum())} of {len(sel)}")
        if kind == "exact":
            assert con["status"][0] == pf.FEW_MATCHES and (con["status"][1:] == pf.OK).all() and sel.all()
        else:
            assert (con["status"] == pf.OK).all() and 2 * sel.sum() >= len(sel)
        keep = good[sel[good]]
        assert not near[keep].any() and con["lead"][keep].min() >= 3 and con["margin"][keep].min() >= 0.1
        if kind == "exact":
            assert all(clean[k, b[k]] for k in keep) and min(lead[i] for i, k in enumerate(good) if sel[k]) >= 3
            assert min(con["hyp_lead"][k][clean[k]].min() for k in keep) >= 3
        for k in keep:
            assert np.array_equal(con["inlier"][ptr[k]:ptr[k + 1]], tr[ptr[k]:ptr[k + 1]]), k
            assert con["n_inliers"][k] == tr[ptr[k]:ptr[k + 1]].sum()
        assert not con["inlier"][ptr[0]:ptr[1]].any() or kind == "noisy"
        if kind == "noisy":
            assert con["adopted"].max() <= FORMS[kind]["refits"]


def test_compose_relative(ba):
    """with the true relative pose and baseline compose_relative reproduces camera b to 1e-12; a canonical camera a gives
    (R, baseline t); the rule of the rotation vector at theta -> 0; the refusals"""
    p = small_scene(ba)
    n, xt = p["npnts"], p["x_true"]
    Cm = pf.cameras(p, xt)
    for a, b in ((0, 1), (5, 2), (11, 10)):
        R, t, base = pf.true_relative(p, xt, a, b)
        x = np.array(xt, copy=True)
        pf.cameras(p, x)[b, :6] = np.nan
        y = ba.compose_relative(x, n, a + 1, b + 1, rr.rotation_vector(R), t, baseline=base)
        assert np.abs(pf.cameras(p, y)[b] - Cm[b]).max() <= 1e-12 and np.array_equal(bits(np.delete(y, slice(3 * n + 9 * b, 3 * n + 9 * b + 6))),
                                                                                 bits(np.delete(x, slice(3 * n + 9 * b, 3 * n + 9 * b + 6))))
        assert np.isnan(x[3 * n + 9 * b]) and not np.shares_memory(x, y)
    x = np.array(xt, copy=True)
    pf.cameras(p, x)[0, :6] = [1e-12, 0, 0, 0, 0, 0]
    R, t, _ = pf.true_relative(p, xt, 3, 4)
    y = pf.cameras(p, ba.compose_relative(x, n, 1, 2, rr.rotation_vector(R), t, baseline=2.5))[1]
    assert np.abs(br.rotations(y[None, :3])[0] - R).max() <= 1e-12 and np.abs(y[3:6] - 2.5 * t).max() <= 1e-12
    y = pf.cameras(p, ba.compose_relative(x, n, 1, 2, np.array([-1e-12, 0, 0]), np.array([0, 0, 1.0])))[1]  # (R R_a = I)
    assert np.array_equal(y[:6], [1e-12, 0, 0, 0, 0, 1.0])
    for bad in (dict(a=1, b=1), dict(a=0), dict(b=p["ncams"] + 1), dict(a=1.0), dict(r=np.zeros(2)), dict(t=np.zeros((3, 1))), dict(x=xt[:-1])):
        kw = dict(dict(x=xt, a=1, b=2, r=np.array([0.1, 0, 0]), t=np.array([0, 0, 1.0])), **bad)
        with pytest.raises(ValueError, match="compose_relative"):
            ba.compose_relative(kw["x"], n, kw["a"], kw["b"], kw["r"], kw["t"])


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _compare(info, con, sel):
    ptr = con["match_ptr"]
    assert np.array_equal(info["match_ptr"], ptr) and info["inliers"].dtype == np.bool_
    assert np.array_equal(info["status"][sel], np.array(["ok", "few_matches", "degenerate", "no_consensus"])[con["status"]][sel])
    assert np.array_equal(info["n_inliers"][sel], con["n_inliers"][sel]) and np.array_equal(info["best_hypothesis"][sel], con["best_hyp"][sel])
    for k in np.flatnonzero(sel):
        assert np.array_equal(info["inliers"][ptr[k]:ptr[k + 1]], con["inlier"][ptr[k]:ptr[k + 1]]), k


def _pose_within_bound(info, con, p, x, pairs, sel, what):
    worst = 0.0
    for k in np.flatnonzero(sel & (con["status"] == pf.OK)):
        spread, _ = fit_spread(con, p, x, pairs, k)
        err = float(pf.pose_error(info["r"][k], info["t"][k], con["r"][k], con["t"][k])[0])
        bound = max(100 * spread, 1e-12)
        print(f"{what}: pair {k}: pose error {err:.3e} (bound {bound:.1e})")
        assert err <= bound, k
        assert abs(np.linalg.norm(info["t"][k]) - 1.0) <= 1e-14
        worst = max(worst, err)
    return worst


@pytest.mark.gpu
def test_exact_masks_and_linear_pose(ba, gpu_ok):
    """exact, refits = 0: the masks, counts, winners and states of the reference; the pose within the bound; a pair that fails
    leaves its six entries of pose as the caller filled them (the C entry, a sentinel)."""
    p, x, pairs = form(ba, "exact")
    con = reference(ba, "exact")
    sel = comparable(con, truth(ba, "exact"))
    assert sel.all()
    info = run(ba, p, x, pairs, opts("exact"))
    _compare(info, con, sel)
    _pose_within_bound(info, con, p, x, pairs, sel, "exact")
    assert info["counts"] == dict(ok=9, few_matches=1, degenerate=0, no_consensus=0) and np.isnan(info["r"][0]).all()
    L, lib = ba._lib.lib(), ba._lib
    n = len(pairs)
    pose, status = np.full((n, 6), 77.0), np.zeros(n, dtype=np.uint8)
    a1, b1 = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    m = _model(ba, p)
    try:
        o = lib.ransac_opts(dict(opts("exact"), min_inliers=30), least=8)
        lib.check(L.ba_relative_pose(m.handle, lib.ptr(x), n, lib.ptr(a1), lib.ptr(b1), C.byref(o), lib.ptr(pose), lib.ptr(status), None, None,
                                     None, None, None))
    finally:
        m.close()
    assert list(status) == [1, 3, 3] + [0] * 7  # 8 and 9 matches are fewer than 30 inliers
    assert (pose[:3] == 77.0).all() and np.array_equal(bits(pose[3:, :3]), bits(info["r"][3:])) and np.array_equal(bits(pose[3:, 3:]), bits(info["t"][3:]))


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 4, 5, 129])
def test_hypothesis_counts_around_a_workgroup(ba, gpu_ok, H):
    """H around the four waves of a workgroup: the pairs whose reference outcome rounding cannot change (comparable) are at least
    half of those attempted, and on them the device gives the reference's masks, counts, winners and states."""
    p, x, pairs = form(ba, "exact")
    con = reference(ba, "exact", hypotheses=H)
    sel = comparable(con, truth(ba, "exact"))
    print(f"H = {H}: {int(sel.sum())} of {len(sel)} pairs compared, states {con['status']}")
    assert 2 * sel.sum() >= len(sel)
    _compare(run(ba, p, x, pairs, opts("exact", hypotheses=H)), con, sel)


@pytest.mark.gpu
def test_noisy_end_to_end(ba, gpu_ok):
    """noisy, up to 4 refits: on the comparable pairs the final mask is the truth and the reference's, and the pose lies within
    the bound against the reference's fit on the true set."""
    p, x, pairs = form(ba, "noisy")
    con, tr = reference(ba, "noisy"), truth(ba, "noisy")
    sel = comparable(con, tr)
    assert 2 * sel.sum() >= len(sel)
    info = run(ba, p, x, pairs, opts("noisy"))
    _compare(info, con, sel)
    ptr = con["match_ptr"]
    for k in np.flatnonzero(sel):
        assert np.array_equal(info["inliers"][ptr[k]:ptr[k + 1]], tr[ptr[k]:ptr[k + 1]])
    _pose_within_bound(info, con, p, x, pairs, sel, "noisy")


@pytest.mark.gpu
def test_without_consensus(ba, gpu_ok):
    """ransac=None is the linear fit on all used matches: with an obs_info that is inf on the displaced detections it gives the
    pose of the consensus call's final fit bit for bit (and inlier = used); (a, b) and (b, a) are inverse poses within the bound."""
    p, x, pairs = form(ba, "exact")
    con = reference(ba, "exact")
    ptr, oa, ob = con["match_ptr"], con["obs_a"], con["obs_b"]
    m = _model(ba, p)
    try:
        with_ransac = ba.relative_pose(m, x, pairs, ransac=opts("exact"))
        sigma = np.ones(p["nobs"])
        sigma[ob[~with_ransac["inliers"]]] = np.inf  # (every observation is in at most one match here)
        plain = ba.relative_pose(m, x, pairs, obs_info=sigma)
        back = ba.relative_pose(m, x, pairs[:, ::-1], obs_info=sigma)
        everything = ba.relative_pose(m, x, pairs[[9]])
    finally:
        m.close()
    ok = with_ransac["status"] == "ok"
    assert ok.sum() == 9 and np.array_equal(plain["status"], with_ransac["status"]) and (plain["best_hypothesis"] == -1).all()
    assert np.array_equal(bits(plain["r"][ok]), bits(with_ransac["r"][ok])) and np.array_equal(bits(plain["t"][ok]), bits(with_ransac["t"][ok]))
    for k in np.flatnonzero(ok):
        assert np.array_equal(plain["inliers"][ptr[k]:ptr[k + 1]], with_ransac["inliers"][ptr[k]:ptr[k + 1]])
    assert np.array_equal(plain["n_inliers"][ok], with_ransac["n_inliers"][ok]) and not plain["inliers"][ptr[0]:ptr[1]].any()
    # all matches of the largest pair, the displaced ones included: every match is used, and the pose is off
    assert everything["inliers"].all() and everything["n_inliers"][0] == COUNTS[9]
    assert pf.pose_error(everything["r"][0], everything["t"][0], con["r"][9], con["t"][9])[0] > 1e-3
    # (b, a): R' and -R't
    for k in np.flatnonzero(ok):
        spread, _ = fit_spread(con, p, x, pairs, k)
        R = br.rotations(plain["r"][[k]])[0]
        err = float(pf.pose_error(back["r"][k], back["t"][k], rr.rotation_vector(R.T), -R.T @ plain["t"][k])[0])
        print(f"pair {k}: (b, a) against the inverse of (a, b) {err:.3e} (bound {max(100 * spread, 1e-12):.1e})")
        assert back["status"][k] == "ok" and err <= max(100 * spread, 1e-12)


@pytest.mark.gpu
def test_seeding_end_to_end(ba, gpu_ok):
    """exact form: camera a true, everything else NaN -> relative_pose -> compose_relative with the true baseline ->
    refine_points(triangulate=True, max_iter=0) on the inlier observations of the pairs: the shared points come out within 100 x
    the spread of the reference's own pipeline (floor 1e-10) of the reference's, and no point is flagged behind."""
    p, x, pairs = form(ba, "exact")
    con = reference(ba, "exact")
    n, ptr, oa, ob = p["npnts"], con["match_ptr"], con["obs_a"], con["obs_b"]
    Ct = pf.cameras(p, p["x_true"])
    info = run(ba, p, x, pairs, opts("exact"))
    ok = np.flatnonzero(info["status"] == "ok")

    def seeded(r, t):
        y = np.array(x, copy=True)
        pf.cameras(p, y)[0::2] = Ct[0::2]
        for k in ok:
            y = ba.compose_relative(y, n, 2 * k + 1, 2 * k + 2, r[k], t[k], baseline=pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)[2])
        return y
    sigma = np.full(p["nobs"], np.inf)
    keep = np.concatenate([np.flatnonzero(info["inliers"][ptr[k]:ptr[k + 1]]) + ptr[k] for k in ok])
    sigma[oa[keep]] = sigma[ob[keep]] = 1.0
    shared = np.unique(p["pnt_idx1"][oa[keep]] - 1)
    r2, t2 = con["r"].copy(), con["t"].copy()
    for k in ok:
        r2[k], t2[k] = fit_spread(con, p, x, pairs, k)[1]
    info_ref = np.zeros((p["nobs"], 2, 2))
    info_ref[np.isfinite(sigma)] = np.eye(2)
    fill = lambda y: np.where(np.isnan(y), 1.0, y)  # noqa: E731  (the cameras that stay NaN observe no kept detection)
    X1 = ptr_ref.refine(p, fill(seeded(con["r"], con["t"])), init=1, max_iter=0, info=info_ref)[0][:3 * n].reshape(n, 3)
    X2 = ptr_ref.refine(p, fill(seeded(r2, t2)), init=1, max_iter=0, info=info_ref)[0][:3 * n].reshape(n, 3)
    bound = max(100 * np.abs(X1 - X2)[shared].max(), 1e-10)
    m = _model(ba, p)
    try:
        y, ip = ba.refine_points(m, seeded(info["r"], info["t"]), triangulate=True, max_iter=0, obs_info=sigma)
    finally:
        m.close()
    X = y[:3 * n].reshape(n, 3)
    err = np.abs(X - X1)[shared].max()
    # against the true points, on the pairs whose set holds no wrong match (a displaced detection that stays within tau of its
    # epipolar line is in the truth, bends the linear pose by 1e-2 and triangulates to a wrong point: the reference's pose tells)
    pure = [k for k in ok if pf.pose_error(con["r"][k], con["t"][k], rr.rotation_vector(pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)[0]),
                                           pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)[1])[0] < 1e-9]
    of_pure = np.unique(p["pnt_idx1"][oa[np.concatenate([np.flatnonzero(info["inliers"][ptr[k]:ptr[k + 1]]) + ptr[k] for k in pure])]] - 1)
    far = np.abs(X - p["x_true"][:3 * n].reshape(n, 3))[of_pure].max()
    print(f"seeding: {len(shared)} points, against the reference {err:.3e} (bound {bound:.1e}); pairs {pure}: {len(of_pure)} points within "
          f"{far:.3e} of the true ones")
    assert len(shared) == tr_count(ba, ok) and err <= bound and len(pure) >= 5 and far <= 1e-6
    assert not ip["behind"][shared].any() and not np.isin(ip["status"][shared], ("degenerate", "nonfinite", "fixed")).any()


def tr_count(ba, ok):
    ptr, tr = reference(ba, "exact")["match_ptr"], truth(ba, "exact")
    return int(sum(tr[ptr[k]:ptr[k + 1]].sum() for k in ok))


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """Two calls give the same bits; a pair alone gives the bits it gives inside the scene; a repeated pair gives identical rows;
    the next lm_step has the bits it has without the call; a communicator is refused with the entry's name; npairs = 0 is fine;
    min_inliers above every count: NO_CONSENSUS with no inlier."""
    p, x, pairs = form(ba, "noisy")
    o = opts("noisy")
    q = small_scene(ba)
    qpairs = np.array([[1, 2], [3, 4], [2, 1]])
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    try:
        i1 = ba.relative_pose(m, x, pairs, ransac=o)
        i2 = ba.relative_pose(m, x, pairs, ransac=o)
        alone = {k: ba.relative_pose(m, x, pairs[[k]], ransac=o) for k in (0, 3, 6)}
        twice = ba.relative_pose(m, x, pairs[[6, 1, 6]], ransac=o)
        none = ba.relative_pose(m, x, np.zeros((0, 2), dtype=np.int64), ransac=o)
        high = ba.relative_pose(m, x, pairs, ransac=dict(o, min_inliers=1000))
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.relative_pose(ms, q["x0"], qpairs, ransac=dict(threshold=4.0))
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.relative_pose(mc, x, pairs, ransac=o)
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_relative_pose" in str(e.value) and "communicator" in str(e.value)
    for key in ("r", "t"):
        assert np.array_equal(bits(i1[key]), bits(i2[key]))
    for key in ("status", "match_ptr", "inliers", "n_inliers", "best_hypothesis"):
        assert np.array_equal(i1[key], i2[key])
    assert (i1["status"] == "ok").all() and i1["counts"]["ok"] == len(pairs)
    ptr = i1["match_ptr"]
    for k, ia in alone.items():
        assert np.array_equal(bits(ia["r"][0]), bits(i1["r"][k])) and np.array_equal(bits(ia["t"][0]), bits(i1["t"][k])), k
        assert np.array_equal(ia["inliers"], i1["inliers"][ptr[k]:ptr[k + 1]]) and ia["best_hypothesis"][0] == i1["best_hypothesis"][k]
    for key in ("r", "t"):
        assert np.array_equal(bits(twice[key][0]), bits(twice[key][2])) and np.array_equal(bits(twice[key][0]), bits(i1[key][6]))
        assert np.array_equal(bits(twice[key][1]), bits(i1[key][1]))
    tp = twice["match_ptr"]
    assert np.array_equal(twice["inliers"][tp[0]:tp[1]], twice["inliers"][tp[2]:tp[3]])
    assert none["r"].shape == (0, 3) and list(none["match_ptr"]) == [0] and none["counts"]["ok"] == 0
    assert (high["status"] == "no_consensus").all() and not high["inliers"].any() and np.isnan(high["r"]).all() and (high["best_hypothesis"] >= 0).all()
    assert np.array_equal(high["n_inliers"], [max(0, c) for c in high["n_inliers"]]) and (high["n_inliers"] < 1000).all()
    for a, b, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c_))
