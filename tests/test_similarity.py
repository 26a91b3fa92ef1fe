"""Similarity alignment of reconstructions (ba_similarity, include/ba_hip.h; similarity, apply_similarity and
camera_centres of the package).  The reference is tests/helpers/similarity_ref.py: the header restated in numpy (np.linalg.svd
where the kernels run Jacobi, the sampling of ransac_ref.sample).  The first tests need no device; the rest run on the GPU.

Scenes: problem k has n_k rows, n_k = 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 600 (the wave and workgroup boundaries of the strided
passes); all problems go in one call, the rows of each in random order.  src is uniform in the unit ball, dst = s Q src + T with s in
0.5..40 (one draw per scene: the threshold of a call is one number in the units of dst), a random Q and |T| ~ 10 per problem.
About n / 20 rows are unused, half by their byte and half by a NaN; where n_k >= 63, 30 % of the rows are displaced by 0.5..3
radii (s x radius in the units of dst).  Four geometries:
  general  as drawn
  planar   src projected onto a random plane through the ball: must still be ok
  line     src on a line: no_consensus with ransac (every sample is collinear), degenerate without
  far      src -> 1e3 src + (1e4, -2e4, 3e4): the sums about the first row (radius 1e3)
Two forms: exact (no noise, tau = 1e-6 s radius, refits 0) and noisy (Gaussian, sigma = 1 % of the radius per coordinate of dst,
tau = 3 sigma, up to 4 refits); 128 hypotheses of 3 rows.  "Truth" for a mask is the set of used rows that pass the test under
the TRUE transform.  The conditions under which the device can be held to the reference's masks are asserted on the reference
first.  Seeds, sigma and tau were chosen on the reference, never on the device.

Bounds (from the reference alone): s (relative), R (absolute, largest entry), the image of the set's centroid and rms (relative
to s x radius) within 100 x the reference's own spread under a permutation of the set's rows, floor 1e-12; the georeferenced
points within 100 x the RMS the reference's own pipeline reaches, floor 1e-10."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_ref import residual
from _lm_run import attach_loopback, loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import similarity_ref as sr  # noqa: E402
from refine_util import _model, bits, small_scene  # noqa: E402

COUNTS = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 600)
GEOMETRIES = ("general", "planar", "line", "far")
FORMS = {"exact": dict(refits=0, sigma=0.0), "noisy": dict(refits=4, sigma=0.01)}
SCENE_SEED = 3
HYPOTHESES = 128
GRID = ((1, 3), (3, 3), (4, 3), (5, 3), (129, 3), (128, 16))  # (hypotheses, sample): the grid's rounding of H / 4
MARGIN = 1e-6
_CACHE = {}


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def random_rotation(rng):
    axis = rng.normal(size=3)
    return sr.rotation_of(axis / np.linalg.norm(axis) * rng.uniform(0.1, 3.0))


def scene(geometry, kind, counts=COUNTS):
    """dict of the module's header: src, dst (n, 3), offsets, used (bytes), tau, radius, s, and per problem Q, T; displaced and
    clean (n, bool): the rows that were moved, the used rows that pass the test under the true transform"""
    def build():
        f = FORMS[kind]
        rng = np.random.default_rng([SCENE_SEED, GEOMETRIES.index(geometry), list(FORMS).index(kind)])
        s, radius = rng.uniform(0.5, 40.0), 1e3 if geometry == "far" else 1.0
        sigma = f["sigma"] * s * radius
        tau = 3.0 * sigma if sigma > 0 else 1e-6 * s * radius
        src, dst, used, displaced, clean, Qs, Ts = [], [], [], [], [], [], []
        for n in counts:
            v = rng.normal(size=(n, 3))
            a = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, size=(n, 1)) ** (1 / 3)
            if geometry == "planar":
                nw, o = rng.normal(size=3), rng.uniform(-0.3, 0.3, size=3)
                nw /= np.linalg.norm(nw)
                a = a - np.outer((a - o) @ nw, nw)
            elif geometry == "line":
                u, o = rng.normal(size=3), rng.uniform(-0.3, 0.3, size=3)
                a = o + np.outer(rng.uniform(-1, 1, size=n), u / np.linalg.norm(u))
            elif geometry == "far":
                a = 1e3 * a + np.array([1e4, -2e4, 3e4])
            Q, T = random_rotation(rng), rng.normal(size=3)
            T *= 10.0 / np.linalg.norm(T)
            b = s * (a @ Q.T) + T
            truth = b.copy()
            b = b + rng.normal(size=(n, 3)) * sigma
            moved = np.zeros(n, dtype=bool)
            if n >= 63:
                moved[rng.choice(n, size=(3 * n) // 10, replace=False)] = True
                w = rng.normal(size=(n, 3))
                b[moved] += (w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, size=(n, 1)) * s * radius)[moved]
            byte = np.ones(n, dtype=np.uint8)
            off = rng.choice(n, size=n // 20, replace=False)
            byte[off[::2]] = 0
            a, b = a.copy(), b.copy()
            for i in off[1::2]:
                (a if i % 2 else b)[i, i % 3] = np.nan
            u = sr.used_rows(a, b, byte)
            with np.errstate(invalid="ignore"):
                ok = u & (((b - truth) ** 2).sum(axis=1) <= tau * tau)
            src.append(a), dst.append(b), used.append(byte), displaced.append(moved), clean.append(ok), Qs.append(Q), Ts.append(T)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return dict(src=np.concatenate(src), dst=np.concatenate(dst), used=np.concatenate(used), offsets=offsets, tau=tau, radius=radius,
                    s=s, Q=Qs, T=Ts, displaced=np.concatenate(displaced), clean=np.concatenate(clean), refits=f["refits"])
    return cached(("scene", geometry, kind, counts), build)


def opts(sc, hypotheses=HYPOTHESES, sample=3, seed=1):
    return dict(threshold=sc["tau"], hypotheses=hypotheses, sample=sample, refits=sc["refits"], seed=seed)


def reference(geometry, kind, hypotheses=HYPOTHESES, sample=3):
    """the reference's results on a scene, computed once and never changed"""
    def build():
        sc = scene(geometry, kind)
        return sr.many(sc["src"], sc["dst"], sc["offsets"], sc["used"], opts(sc, hypotheses, sample))
    return cached(("reference", geometry, kind, hypotheses, sample), build)


def rows_of(sc, k):
    return slice(int(sc["offsets"][k]), int(sc["offsets"][k + 1]))


def call(ba, m, sc, ransac, **kw):
    return ba.similarity(m, sc["src"], sc["dst"], offsets=sc["offsets"], used=sc["used"] != 0, ransac=ransac, **kw)


def assert_masks_equal(got, ref, sc):
    """status, inliers, n_inliers, best_hypothesis and counts equal the reference's exactly"""
    assert list(got["status"]) == [q["status"] for q in ref]
    assert np.array_equal(got["inliers"], np.concatenate([q["inlier"] for q in ref]))
    assert np.array_equal(got["n_inliers"], [q["n_inliers"] for q in ref])
    assert np.array_equal(got["best_hypothesis"], [q["best_hyp"] for q in ref])
    assert got["counts"] == {s: sum(q["status"] == s for q in ref) for s in sr.STATES}


def distances(f, g, src_set, scale):
    """(s relative, R absolute, image of the centroid and rms relative to `scale`) between two fits (s, R, t, rms)"""
    c = src_set.mean(axis=0)
    return np.array([abs(f[0] - g[0]) / abs(g[0]), np.abs(f[1] - g[1]).max(),
                     np.linalg.norm((f[0] * f[1] @ c + f[2]) - (g[0] * g[1] @ c + g[2])) / scale, abs(f[3] - g[3]) / scale])


def assert_fits_close(got, ref, sc, label, scale_flag=True):
    """every ok problem within 100 x the reference's own spread under a permutation of the set's rows, floor 1e-12"""
    worst_d, worst_s = np.zeros(4), np.zeros(4)
    rng = np.random.default_rng(77)
    for k, q in enumerate(ref):
        if q["status"] != "ok":
            assert np.isnan(got["s"][k]) and np.isnan(got["r"][k]).all() and np.isnan(got["t"][k]).all() and np.isnan(got["rms"][k])
            continue
        sl = rows_of(sc, k)
        a, b = sc["src"][sl][q["inlier"]], sc["dst"][sl][q["inlier"]]
        perm = rng.permutation(len(a))
        f2 = sr.fit(a[perm], b[perm], scale_flag)
        e2 = sr.residuals(a, b, f2)
        scale = q["s"] * sc["radius"]
        spread = distances((*f2, np.sqrt((e2 * e2).sum() / len(a))), (q["s"], q["R"], q["t"], q["rms"]), a, scale)
        dist = distances((got["s"][k], sr.rotation_of(got["r"][k]), got["t"][k], got["rms"][k]), (q["s"], q["R"], q["t"], q["rms"]), a, scale)
        worst_d, worst_s = np.maximum(worst_d, dist), np.maximum(worst_s, spread)
        assert np.isfinite(dist).all() and (dist <= np.maximum(100.0 * spread, 1e-12)).all(), (label, k, dist, spread)
    print(f"similarity[{label}]: worst distance to the reference (s, R, centroid, rms) {worst_d}, worst spread of the reference {worst_s}")


# ---- no device ------------------------------------------------------------------------------------------------------------------------

def test_symbols_header_julia_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    assert "ba_similarity" in lib.SYMBOLS and hasattr(L, "ba_similarity")
    assert "(:ba_similarity, libba)" in julia and "function similarity(" in julia
    for fn in ("similarity", "apply_similarity", "camera_centres"):
        assert fn in ba.__all__ and callable(getattr(ba, fn))
    assert "enum { BA_SM_OK = 0, BA_SM_FEW_ROWS = 1, BA_SM_DEGENERATE = 2, BA_SM_NO_CONSENSUS = 3, BA_SM_STATES = 4 };" in header
    for word in ("similarity alignment", "sigma_2 <= 1e-10 sigma_1", "sum b a' (9)", "Coplanar rows are", "communicator", "reflections",
                 "|s R src + t - dst|^2 <= tau^2"):
        assert word in header, word
    assert lib.SIMILARITY_STATES == ("ok", "few_rows", "degenerate", "no_consensus")
    good = lib.RansacOpts(1.0, 0, 0, -1, 0, 0)
    tail = (None,) * 7
    who = b"ba_similarity"
    head = (None, 0, None, None, None, None)
    assert L.ba_similarity(*head, C.byref(good), 1, *tail) == 1
    assert who in L.ba_last_error() and b"null argument" in L.ba_last_error()
    assert L.ba_similarity(*head, None, 1, *tail) == 1 and b"null argument" in L.ba_last_error()
    for bad, word in ((dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=np.nan), b"threshold"),
                      (dict(threshold=np.inf), b"threshold"), (dict(hypotheses=4097), b"hypotheses"), (dict(sample=2), b"sample in 3..16"),
                      (dict(sample=17), b"sample in 3..16"), (dict(refits=9), b"refits"), (dict(min_inliers=2), b"min_inliers")):
        o = lib.RansacOpts(**dict(dict(threshold=1.0, hypotheses=0, sample=0, refits=-1, min_inliers=0, seed=0), **bad))
        assert L.ba_similarity(*head, C.byref(o), 1, *tail) == 1
        msg = L.ba_last_error()
        assert word in msg and who in msg, (bad, msg)
    for o in (lib.RansacOpts(1.0, 16, 3, 0, 3, 3), lib.RansacOpts(1.0, 4096, 16, 8, 0, 3)):  # good options reach the argument check
        assert L.ba_similarity(*head, C.byref(o), 1, *tail) == 1 and b"null argument" in L.ba_last_error()
    # the siblings' refusals are what they were
    o = lib.RansacOpts(1.0, 0, 3, -1, 0, 0)
    assert L.ba_homography(None, None, 0, None, None, C.byref(o), *tail) == 1 and b"sample in 4..16" in L.ba_last_error()
    assert L.ba_relative_pose(None, None, 0, None, None, C.byref(o), *tail) == 1 and b"sample in 8..16" in L.ba_last_error()


def test_python_value_errors(ba):
    """ValueError before any device call (None stands in for the model)"""
    assert ba.similarity.__kwdefaults__ == dict(offsets=None, used=None, ransac=None, scale=True)
    a = np.zeros((5, 3))
    for kw in (dict(src=np.zeros((5, 2))), dict(dst=np.zeros((4, 3))), dict(src=np.zeros(15)), dict(src=[["a"] * 3] * 5),
               dict(offsets=[0, 3]), dict(offsets=[1, 5]), dict(offsets=[0, 4, 3, 5]), dict(offsets=np.array([0.0, 5.0])), dict(offsets=[[0, 5]]),
               dict(used=np.ones(4, dtype=bool)), dict(used=np.ones(5)), dict(scale=1), dict(ransac=3.0), dict(ransac=dict()),
               dict(ransac=dict(threshold=0.0)), dict(ransac=dict(threshold=1.0, sample=2)), dict(ransac=dict(threshold=1.0, sample=17)),
               dict(ransac=dict(threshold=1.0, min_inliers=2)), dict(ransac=dict(threshold=1.0, hypotheses=4097)),
               dict(ransac=dict(threshold=1.0, refits=9)), dict(ransac=dict(threshold=1.0, tau=1.0))):
        args = dict(dict(src=a, dst=a), **kw)
        with pytest.raises(ValueError):
            ba.similarity(None, args.pop("src"), args.pop("dst"), **args)
    x = np.zeros(3 * 4 + 9 * 2)
    for args, kw in (((x[:-1], 4, 1.0, [0.1, 0, 0], [0, 0, 0]), {}), ((x, 4, 0.0, [0.1, 0, 0], [0, 0, 0]), {}), ((x, 4, np.nan, [0.1, 0, 0], [0, 0, 0]), {}),
                     ((x, 4, 1.0, [0.1, 0], [0, 0, 0]), {}), ((x, 4, 1.0, [0.1, 0, 0], [0, np.inf, 0]), {}), ((x, 4, 1.0, [0.0, 0, 0], [0, 0, 0]), {}),
                     ((x, 4, 1.0, [0.1, 0, 0], [0, 0, 0]), dict(cameras=[0])), ((x, 4, 1.0, [0.1, 0, 0], [0, 0, 0]), dict(cameras=[3])),
                     ((x, 4, 1.0, [0.1, 0, 0], [0, 0, 0]), dict(points=[5])), ((x, 4, 1.0, [0.1, 0, 0], [0, 0, 0]), dict(points=[1.0]))):
        with pytest.raises(ValueError):
            ba.apply_similarity(*args, **kw)
    with pytest.raises(ValueError):
        ba.camera_centres(x[:-1], 4)


def test_apply_similarity_and_camera_centres(ba, orc, small_prob):
    p = small_prob
    npnts, x = p["npnts"], np.asarray(p["x0"], dtype=np.float64)
    s, r, t = 37.0, np.array([1.2, -1.0, 1.2]) / np.linalg.norm([1.2, -1.0, 1.2]) * 2.0, np.array([30.0, -24.0, 32.0])
    assert abs(np.linalg.norm(t) - 50.0) < 1e-12
    Q = sr.rotation_of(r)
    y = ba.apply_similarity(x, npnts, s, r, t)
    assert y is not x and y.shape == x.shape
    r0, r1 = residual(orc, p, x), residual(orc, p, y)
    assert abs(r0 @ r0 - r1 @ r1) <= 1e-9 * (r0 @ r0)  # the similarity changes no reprojection
    assert np.abs(r0 - r1).max() <= 1e-9 * np.abs(r0).max()
    assert np.array_equal(y[3 * npnts:].reshape(-1, 9)[:, 6:], x[3 * npnts:].reshape(-1, 9)[:, 6:])  # the intrinsics are untouched
    c0, c1 = ba.camera_centres(x, npnts), ba.camera_centres(y, npnts)
    assert c0.shape == (p["ncams"], 3)
    want = s * c0 @ Q.T + t
    assert np.abs(c1 - want).max() <= 1e-12 * np.abs(want).max()
    cams = x[3 * npnts:].reshape(-1, 9)
    assert np.allclose(c0[3], -sr.rotation_of(cams[3, :3]).T @ cams[3, 3:6], rtol=0, atol=1e-14)
    assert np.abs(y[:3 * npnts].reshape(-1, 3) - (s * x[:3 * npnts].reshape(-1, 3) @ Q.T + t)).max() <= 1e-12 * 50
    # a subset moves only its cameras and points, bit for bit elsewhere
    ci, pi = np.array([2, 5, 11]), np.array([1, 7, 8, 400])
    z = ba.apply_similarity(x, npnts, s, r, t, cameras=ci, points=pi)
    zc, yc, xc = (v[3 * npnts:].reshape(-1, 9) for v in (z, y, x))
    zp, yp, xp = (v[:3 * npnts].reshape(-1, 3) for v in (z, y, x))
    mc, mp = np.zeros(p["ncams"], dtype=bool), np.zeros(npnts, dtype=bool)
    mc[ci - 1], mp[pi - 1] = True, True
    assert same(zc[mc], yc[mc]) and same(zc[~mc], xc[~mc]) and same(zp[mp], yp[mp]) and same(zp[~mp], xp[~mp])
    none = ba.apply_similarity(x, npnts, s, r, t, cameras=[], points=np.zeros(0, dtype=np.int64))
    assert same(none, x)
    # (s, r, t) and then its inverse: X = Q' (Y - t) / s
    back = ba.apply_similarity(y, npnts, 1.0 / s, -r, -(Q.T @ t) / s)
    np3 = 3 * npnts
    assert np.abs(back[:np3] - x[:np3]).max() <= 1e-12 * np.abs(x[:np3]).max()
    bc = back[np3:].reshape(-1, 9)
    assert np.abs(bc[:, :3] - cams[:, :3]).max() <= 1e-12 * np.abs(cams[:, :3]).max()
    assert np.abs(bc[:, 3:6] - cams[:, 3:6]).max() <= 1e-12 * np.abs(cams[:, 3:6]).max()
    assert np.array_equal(bc[:, 6:], cams[:, 6:])


def test_reference_fit_recovers_the_truth():
    """the reference itself: exact rows give the transform back, with and without scale, on general, coplanar and far rows; collinear
    rows and fewer than three are refused"""
    rng = np.random.default_rng(5)
    for trial in range(20):
        a = rng.normal(size=(7, 3))
        if trial % 3 == 1:
            a[:, 2] = 0.25  # coplanar
        if trial % 3 == 2:
            a = 1e3 * a + np.array([1e4, -2e4, 3e4])
        s, Q, T = (rng.uniform(0.5, 40.0) if trial % 2 else 1.0), random_rotation(rng), rng.normal(size=3) * 10
        f = sr.fit(a, s * a @ Q.T + T, scale=bool(trial % 2))
        assert abs(f[0] - s) <= 1e-12 * s and np.abs(f[1] - Q).max() <= 1e-11 and abs(np.linalg.det(f[1]) - 1) <= 1e-12
        assert np.abs(sr.residuals(a, s * a @ Q.T + T, f)).max() <= 1e-9 * s * np.abs(a).max()
    line = np.outer(np.arange(5.0), [1.0, 2.0, -1.0]) + 3.0
    assert sr.fit(line, 2.0 * line) is None
    assert sr.one(line, 2.0 * line)["status"] == "degenerate" and sr.one(line[:2], line[:2])["status"] == "few_rows"
    mirror = rng.normal(size=(6, 3))
    f = sr.fit(mirror, mirror * np.array([1.0, 1.0, -1.0]))  # a reflection is out of scope: the nearest proper rotation comes back
    assert f is not None and abs(np.linalg.det(f[1]) - 1) <= 1e-12


@pytest.mark.parametrize("kind", list(FORMS))
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_reference_conditions(geometry, kind):
    """the conditions of the GPU tests, on the reference alone"""
    sc, ref = scene(geometry, kind), reference(geometry, kind)
    assert ref[0]["status"] == "few_rows" and ref[0]["n_inliers"] == 0 and not ref[0]["inlier"].any()
    if geometry == "line":
        assert all(q["status"] == "no_consensus" and q["best_hyp"] == -1 and q["n_inliers"] == 0 for q in ref[1:])
        plain = sr.many(sc["src"], sc["dst"], sc["offsets"], sc["used"], None)
        assert [q["status"] for q in plain] == ["few_rows"] + ["degenerate"] * (len(COUNTS) - 1)
        return
    adopted, margin, share = 0, np.inf, 1.0
    for k, q in enumerate(ref):
        if k == 0:
            continue
        sl = rows_of(sc, k)
        assert q["status"] == "ok", (geometry, kind, k, q["status"])
        assert not (q["inlier"] & sc["displaced"][sl]).any(), (geometry, kind, k)  # no displaced row is in a final set
        clean = sc["clean"][sl]
        share = min(share, (q["inlier"] & clean).sum() / clean.sum())
        assert (q["inlier"] & clean).sum() >= 0.95 * clean.sum(), (geometry, kind, k, (q["inlier"] & clean).sum(), clean.sum())
        adopted += q["adopted"] > 0
        margin = min(margin, q["margin"])
        assert abs(q["s"] - sc["s"]) <= 0.05 * sc["s"] and np.abs(q["R"] - sc["Q"][k]).max() <= 0.2
    print(f"similarity reference[{geometry}, {kind}]: {adopted} problems adopt a refit, smallest margin {margin:.3e} tau, "
          f"smallest share of the clean rows {share:.3f}")
    assert margin > MARGIN, margin
    if kind == "noisy":
        assert adopted >= 4, adopted


@pytest.mark.parametrize("hs", GRID)
def test_reference_conditions_of_the_grid(hs):
    """the (hypotheses, sample) cases of the GPU test keep the margin that lets the device be held to the reference's masks"""
    ref = reference("general", "noisy", *hs)
    margin = min(q["margin"] for q in ref)
    print(f"similarity reference[grid {hs}]: states {[q['status'] for q in ref]}, smallest margin {margin:.3e} tau")
    assert margin > MARGIN
    assert ref[0]["status"] == "few_rows" and all(q["status"] in ("ok", "no_consensus") for q in ref[1:])
    if hs[1] == 16:  # a sample of 16 does not fit into 3, 4 or 5 rows
        assert [q["status"] for q in ref[1:4]] == ["no_consensus"] * 3


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(ba, gpu_ok):
    m = _model(ba, small_scene(ba))
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(FORMS))
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_against_the_reference(ba, model, geometry, kind):
    sc, ref = scene(geometry, kind), reference(geometry, kind)
    got = call(ba, model, sc, opts(sc))
    assert_masks_equal(got, ref, sc)
    assert_fits_close(got, ref, sc, f"{geometry}, {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("hs", GRID)
def test_hypothesis_counts_and_samples(ba, model, hs):
    sc, ref = scene("general", "noisy"), reference("general", "noisy", *hs)
    got = call(ba, model, sc, opts(sc, *hs))
    assert_masks_equal(got, ref, sc)
    assert_fits_close(got, ref, sc, f"grid {hs}")


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_without_ransac_on_clean_rows(ba, model, geometry):
    """ransac=None: the fit on all used rows; a line is degenerate"""
    sc = scene(geometry, "exact")
    keep = (sc["used"] != 0) & ~sc["displaced"]
    ref = cached(("plain", geometry), lambda: sr.many(sc["src"], sc["dst"], sc["offsets"], keep, None))
    got = ba.similarity(model, sc["src"], sc["dst"], offsets=sc["offsets"], used=keep)
    assert_masks_equal(got, ref, sc)
    assert [q["status"] for q in ref] == ["few_rows"] + ["degenerate" if geometry == "line" else "ok"] * (len(COUNTS) - 1)
    assert (got["best_hypothesis"] == -1).all()
    assert np.array_equal(got["inliers"][sc["offsets"][1]:], sr.used_rows(sc["src"], sc["dst"], keep)[sc["offsets"][1]:])
    assert_fits_close(got, ref, sc, f"{geometry}, no ransac")
    if geometry != "line":
        for k in range(1, len(COUNTS)):
            assert abs(got["s"][k] - sc["s"]) <= 1e-9 * sc["s"] and np.abs(sr.rotation_of(got["r"][k]) - sc["Q"][k]).max() <= 1e-9
            assert got["rms"][k] <= 1e-9 * sc["s"] * sc["radius"]


@pytest.mark.gpu
def test_scale_false(ba, model):
    """scale=False on a rigid scene gives s = 1 exactly; on a scaled scene it is still ok with s = 1"""
    sc = scene("general", "exact")
    keep = (sc["used"] != 0) & ~sc["displaced"]
    shifted = np.concatenate([sc["src"][rows_of(sc, k)] @ sc["Q"][k].T + sc["T"][k] for k in range(len(COUNTS))])
    a = ba.similarity(model, sc["src"], shifted, offsets=sc["offsets"], used=keep, scale=False)
    assert list(a["status"]) == ["few_rows"] + ["ok"] * (len(COUNTS) - 1)
    assert (a["s"][1:] == 1.0).all() and (a["rms"][1:] <= 1e-12).all()
    for k in range(1, len(COUNTS)):
        assert np.abs(sr.rotation_of(a["r"][k]) - sc["Q"][k]).max() <= 1e-12 and np.abs(a["t"][k] - sc["T"][k]).max() <= 1e-11
    b = call(ba, model, dict(sc, src=sc["src"], dst=shifted), dict(threshold=1e-9, refits=0, seed=2), scale=False)
    assert list(b["status"]) == ["few_rows"] + ["ok"] * (len(COUNTS) - 1) and (b["s"][1:] == 1.0).all()
    c = ba.similarity(model, sc["src"], sc["dst"], offsets=sc["offsets"], used=keep, scale=False)  # a scaled scene
    ref = sr.many(sc["src"], sc["dst"], sc["offsets"], keep, None, scale=False)
    assert list(c["status"]) == ["few_rows"] + ["ok"] * (len(COUNTS) - 1) and (c["s"][1:] == 1.0).all()
    assert_fits_close(c, ref, sc, "general, scale=False", scale_flag=False)


@pytest.mark.gpu
def test_offsets_and_used(ba, model):
    """the eleven problems in one call give, problem by problem, the bits of eleven calls; `used` as bytes equals the same rows set
    to NaN"""
    sc = scene("planar", "noisy")
    o = opts(sc)
    got = call(ba, model, sc, o)
    for k in range(len(COUNTS)):
        sl = rows_of(sc, k)
        one = ba.similarity(model, sc["src"][sl], sc["dst"][sl], used=sc["used"][sl] != 0, ransac=o)
        for key in ("s", "r", "t", "rms", "n_inliers", "best_hypothesis"):
            assert same(one[key][0], got[key][k]), (k, key)
        assert one["status"][0] == got["status"][k] and np.array_equal(one["inliers"], got["inliers"][sl])
    src = sc["src"].copy()
    src[sc["used"] == 0, 1] = np.nan
    nan = ba.similarity(model, src, sc["dst"], offsets=sc["offsets"], ransac=o)
    for key in ("s", "r", "t", "rms", "n_inliers", "best_hypothesis", "inliers"):
        assert same(nan[key], got[key]), key
    assert (nan["status"] == got["status"]).all() and nan["counts"] == got["counts"]
    empty = ba.similarity(model, np.zeros((0, 3)), np.zeros((0, 3)), offsets=[0, 0, 0])
    assert list(empty["status"]) == ["few_rows"] * 2 and empty["counts"]["few_rows"] == 2


@pytest.mark.gpu
def test_refusals_on_a_handle(ba, gpu_ok):
    """NULL sim or status, a decreasing row_ptr, nprob == 0, and a handle with a communicator"""
    L, lib = ba._lib.lib(), ba._lib
    p = small_scene(ba)
    a = np.random.default_rng(1).normal(size=(6, 3))
    m = _model(ba, p)
    try:
        ptr3, sim, st = np.array([0, 3, 6], dtype=np.int64), np.zeros(14), np.zeros(2, dtype=np.uint8)
        tail = (None,) * 5
        head = (m.handle, 2, lib.ptr(ptr3), lib.ptr(a), lib.ptr(a), None, None, 1)
        assert L.ba_similarity(*head, None, lib.ptr(st), *tail) == 1 and b"null argument" in L.ba_last_error()
        assert L.ba_similarity(*head, lib.ptr(sim), None, *tail) == 1 and b"null argument" in L.ba_last_error()
        assert L.ba_similarity(m.handle, 2, lib.ptr(ptr3), None, lib.ptr(a), None, None, 1, lib.ptr(sim), lib.ptr(st), *tail) == 1
        assert b"null argument" in L.ba_last_error()
        for bad in ([0, 4, 3], [1, 3, 6]):
            down = np.array(bad, dtype=np.int64)
            assert L.ba_similarity(m.handle, 2, lib.ptr(down), lib.ptr(a), lib.ptr(a), None, None, 1, lib.ptr(sim), lib.ptr(st), *tail) == 1
            assert b"ba_similarity" in L.ba_last_error() and b"row_ptr" in L.ba_last_error()
        assert L.ba_similarity(m.handle, 0, None, None, None, None, None, 1, None, None, *tail) == 0  # nprob == 0
        assert L.ba_similarity(*head, lib.ptr(sim), lib.ptr(st), *tail) == 0 and list(st) == [0, 0]
    finally:
        m.close()
    with loopback_world(1, 1 << 20) as (LL, loop):
        mc = _model(ba, p)
        try:
            attach_loopback(ba, mc, LL, loop, 0, 1)
            with pytest.raises(ba.BAArgError) as e1:
                ba.similarity(mc, a, a)
        finally:
            mc.close()
    assert "ba_similarity" in str(e1.value) and "communicator" in str(e1.value)


def georeference(ba, p, fit_of):
    """small_scene moved by a large similarity and brought back through its camera centres, of which 25 % are displaced in the
    target: the RMS of all points against x_true.  fit_of(src, dst) -> (s, r, t)"""
    lib = ba._lib
    npnts, xt = p["npnts"], np.asarray(p["x_true"], dtype=np.float64)
    r = np.array([-0.6, 1.9, 0.4])
    moved = lib.apply_similarity(xt, npnts, 37.0, r, np.array([400.0, -300.0, 120.0]))
    gps = lib.camera_centres(xt, npnts)
    rng = np.random.default_rng(8)
    bad = rng.choice(p["ncams"], size=p["ncams"] // 4, replace=False)
    w = rng.normal(size=(len(bad), 3))
    gps[bad] += w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, size=(len(bad), 1))
    s, rv, t = fit_of(lib.camera_centres(moved, npnts), gps)
    back = lib.apply_similarity(moved, npnts, s, rv, t)
    d = (back[:3 * npnts] - xt[:3 * npnts]).reshape(-1, 3)
    return float(np.sqrt((d * d).sum(axis=1).mean()))


@pytest.mark.gpu
def test_georeferencing_end_to_end(ba, model):
    p = small_scene(ba)
    o = dict(threshold=1e-6, seed=4)

    def by_reference(ransac):
        def fit_of(src, dst):
            q = sr.one(src, dst, None, ransac)
            assert q["status"] == "ok"
            return q["s"], q["r"], q["t"]
        return fit_of

    def by_device(ransac):
        def fit_of(src, dst):
            q = ba.similarity(model, src, dst, ransac=ransac)
            assert q["status"][0] == "ok" and (q["n_inliers"][0] == p["ncams"] - p["ncams"] // 4 or ransac is None)
            return q["s"][0], q["r"][0], q["t"][0]
        return fit_of

    rms_ref = georeference(ba, p, by_reference(o))
    bound = max(100.0 * rms_ref, 1e-10)
    rms_dev, rms_plain = georeference(ba, p, by_device(o)), georeference(ba, p, by_device(None))
    print(f"similarity georeferencing: RMS of the points, reference {rms_ref:.3e}, device {rms_dev:.3e}, device without ransac {rms_plain:.3e}")
    assert rms_ref <= 1e-10  # the reference's pipeline itself comes back to the true frame
    assert rms_dev <= bound
    assert rms_plain > bound and rms_plain > 1e-3  # the consensus stage is what does it


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """two calls give the same bits; an LM step and an LM solve after the calls give the bits they give before"""
    sc = scene("general", "noisy")
    o = opts(sc)
    q = small_scene(ba)
    ms, plain = _model(ba, q), _model(ba, q)
    try:
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        before = ba.lm_step(ms, q["x0"], 3.0)
        a = call(ba, ms, sc, o)
        b = call(ba, ms, sc, o)
        c = call(ba, plain, sc, o)
        for key in ("s", "r", "t", "rms", "inliers", "n_inliers", "best_hypothesis"):
            assert same(a[key], b[key]) and same(a[key], c[key]), key
        assert (a["status"] == b["status"]).all() and a["counts"] == b["counts"]
        ba.similarity(ms, sc["src"], sc["dst"])
        after = ba.lm_step(ms, q["x0"], 3.0)
        for u, v, w in zip(ref_step, before, after):
            assert np.array_equal(np.asarray(u), np.asarray(v)) and np.array_equal(np.asarray(v), np.asarray(w))
        s0 = ba.Levenberg_Marquardt(ba.FeasibilityResidual(plain), "LDL", "AMD", "None", False)
        call(ba, ms, sc, o)
        s1 = ba.Levenberg_Marquardt(ba.FeasibilityResidual(ms), "LDL", "AMD", "None", False)
        assert same(s0.solution, s1.solution) and s0.iter == s1.iter and same([s0.objective], [s1.objective])
    finally:
        ms.close()
        plain.close()
