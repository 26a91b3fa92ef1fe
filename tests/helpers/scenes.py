"""Scenes the package's generator never draws by itself (test code; synthetic.make_problem and its random draws are untouched):
several problems merged into one -- a camera graph with several connected components -- and cameras that share no point with
any other camera (tests/test_block_sparse_scenes.py); and observation graphs given point by point or camera pair by camera pair,
so that a point's number of observations, where its rows fall against the kernels' 64-row batches and 64-point waves, and the
length of a camera pair's task list are chosen, not drawn (tests/test_graph_boundaries.py); and seeded arrays of per-observation
information matrices with zero and rank-one blocks among them (tests/test_obs_info.py)."""
import functools

import numpy as np

KEYS = ("cam_idx1", "pnt_idx1", "pt2d", "x0", "x_true", "ncams", "npnts", "nobs")


def merge_scenes(parts):
    """Several problem dicts (as synthetic.make_problem returns them) as ONE problem: the cameras and points of part i are
    numbered after those of the parts before it, so no camera of one part shares a point with a camera of another.  pt2d is
    concatenated; x0 / x_true are all point blocks followed by all camera blocks (the layout of x is points first).  Every part
    is in BAL order (by point, then camera) and the points of a later part have higher numbers: so is the result."""
    parts = list(parts)
    out = {"ncams": 0, "npnts": 0, "nobs": 0}
    cam, pnt = [], []
    for p in parts:
        cam.append(np.asarray(p["cam_idx1"], dtype=np.int64) + out["ncams"])
        pnt.append(np.asarray(p["pnt_idx1"], dtype=np.int64) + out["npnts"])
        for key in ("ncams", "npnts", "nobs"):
            out[key] += int(p[key])
    out["cam_idx1"], out["pnt_idx1"] = np.concatenate(cam), np.concatenate(pnt)
    out["pt2d"] = np.ascontiguousarray(np.concatenate([np.asarray(p["pt2d"], dtype=np.float64) for p in parts]))
    for key in ("x0", "x_true"):
        out[key] = np.concatenate([np.asarray(p[key])[: 3 * p["npnts"]] for p in parts] + [np.asarray(p[key])[3 * p["npnts"]:] for p in parts])
    assert len(out["cam_idx1"]) == out["nobs"] and len(out["pt2d"]) == 2 * out["nobs"] and len(out["x0"]) == 3 * out["npnts"] + 9 * out["ncams"]
    same = out["pnt_idx1"][1:] == out["pnt_idx1"][:-1]
    assert np.all(np.diff(out["pnt_idx1"]) >= 0) and np.all(out["cam_idx1"][1:][same] > out["cam_idx1"][:-1][same]), "not in BAL order"
    return out


def isolated_cameras(ba, n, k, seed):
    """n cameras with k points each, every point seen once and only by its own camera: a camera graph without an edge.  The
    geometry (x0, x_true) is that of make_problem(n, n k, 2 n k, seed); point j belongs to camera j % n; pt2d is the projection of
    x_true plus N(0, 0.5^2) px from a generator seeded with `seed`."""
    syn = ba.synthetic
    g = syn.make_problem(n, n * k, 2 * n * k, seed=seed)
    npnts = n * k
    pnt0 = np.arange(npnts, dtype=np.int64)
    cam0 = pnt0 % n
    pts = g["x_true"][: 3 * npnts].reshape(npnts, 3)
    cams = g["x_true"][3 * npnts:].reshape(n, 9)
    proj = syn.project(pts[pnt0], cams[cam0])
    pt2d = proj + np.random.default_rng(seed).normal(0.0, 0.5, size=proj.shape)
    return dict(cam_idx1=cam0 + 1, pnt_idx1=pnt0 + 1, pt2d=np.ascontiguousarray(pt2d.ravel()), x0=g["x0"], x_true=g["x_true"],
                ncams=int(n), npnts=int(npnts), nobs=int(npnts))


def _scene_from_lists(ba, ncams, npnts, pnt0, cam0, seed):
    """the problem dict of the observations (pnt0, cam0) (0-based, in BAL order): geometry of make_problem(ncams, npnts, 2 npnts,
    seed), pt2d the projection of x_true plus N(0, 0.5^2) px from a generator seeded with `seed`"""
    syn = ba.synthetic
    g = syn.make_problem(ncams, npnts, 2 * npnts, seed=seed)
    pts = g["x_true"][: 3 * npnts].reshape(npnts, 3)
    cams = g["x_true"][3 * npnts:].reshape(ncams, 9)
    proj = syn.project(pts[pnt0], cams[cam0])
    pt2d = proj + np.random.default_rng(seed).normal(0.0, 0.5, size=proj.shape)
    return dict(cam_idx1=cam0 + 1, pnt_idx1=pnt0 + 1, pt2d=np.ascontiguousarray(pt2d.ravel()), x0=g["x0"], x_true=g["x_true"],
                ncams=int(ncams), npnts=int(npnts), nobs=int(len(pnt0)))


def scene_from_degrees(ba, ncams, degrees, seed, window=None):
    """Point j is seen by degrees[j] consecutive cameras, (7 j + i) % window for i < degrees[j]; 0 observations are allowed.
    window (None: ncams) <= ncams: the cameras from `window` on see nothing.  In BAL order (by point, then camera)."""
    degrees = np.asarray(degrees, dtype=np.int64)
    window = int(ncams if window is None else window)
    npnts = len(degrees)
    assert 2 <= window <= ncams and np.all(degrees >= 0) and np.all(degrees <= window)
    pnt0 = np.repeat(np.arange(npnts, dtype=np.int64), degrees)
    within = np.arange(len(pnt0), dtype=np.int64) - np.repeat(np.cumsum(degrees) - degrees, degrees)
    cam0 = (7 * pnt0 + within) % window
    order = np.lexsort((cam0, pnt0))
    return _scene_from_lists(ba, ncams, npnts, pnt0, cam0[order], seed)


def scene_from_pair_lengths(ba, ncams, lengths, seed):
    """lengths: {(a, b): L} over camera pairs a > b (0-based).  The scene has L points with 2 observations for every pair, seen
    by exactly a and b, the pairs in ascending order: the task list of key (a, b) of the reduced camera system has exactly L
    entries, that of key (a, a) as many as camera a has observations.  A camera in no pair (or only in pairs of length 0) sees
    nothing.  In BAL order."""
    pairs = sorted(lengths)
    assert all(0 <= b < a < ncams for a, b in pairs) and all(int(lengths[k]) >= 0 for k in pairs)
    L = np.array([int(lengths[k]) for k in pairs], dtype=np.int64)
    ab = np.array(pairs, dtype=np.int64).reshape(len(pairs), 2)
    npnts = int(L.sum())
    pnt0 = np.repeat(np.arange(npnts, dtype=np.int64), 2)
    cam0 = np.repeat(ab[:, ::-1], L, axis=0).ravel()  # (b, a) per point: ascending
    return _scene_from_lists(ba, ncams, npnts, pnt0, cam0, seed)


# ---- the scenes of tests/test_graph_boundaries.py ---------------------------------------------------------------------------
P_WINDOW, P_NCAMS = 200, 201  # scene P: the cameras 0..199 take part, camera 200 sees nothing
K_CYCLE16 = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 66, 95, 96, 97, 127, 128, 129, 130)
K_CYCLE128 = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 300)
K16_EXTRA = (1, 255, 256, 257)  # cameras 24..27 of K16: points shared with camera 1 only
K_CAMS, K128_FILL_CAMS = 24, 12


def p_degrees():
    """Scene P, 327 points (one workgroup of four 64-point waves, then a full wave and a wave of 7):
    0..62 one observation each (rows 0..62); 63: 65 observations (rows 63..127: starts on the last row of a 64-row batch, covers
    the whole next one, and wave 0 ends batch-aligned); 64, 65, 66: 128, 129, 200 (two whole batches, one row more, 200);
    67..127 and the whole wave 128..191: none; 192..255: 2 and 3 (their sum is no multiple of 64); 256..319: 2 to 5;
    320..326: small, the last 64."""
    d = np.zeros(327, dtype=np.int64)
    d[:63] = 1
    d[63:67] = (65, 128, 129, 200)
    d[192:256] = 2 + (np.arange(64) % 3 == 0)  # 22 threes: 150 rows
    d[256:320] = 2 + np.arange(64) % 4
    d[320:327] = (1, 2, 0, 3, 1, 2, 64)
    return d


def _cycled_pairs(ncams, cycle):
    """the ncams (ncams - 1) / 2 pairs a > b in the order (1, 0), (2, 0), (2, 1), ... with the lengths of `cycle` in turn"""
    pairs = [(a, b) for a in range(1, ncams) for b in range(a)]
    return {k: cycle[i % len(cycle)] for i, k in enumerate(pairs)}


def k16_lengths():
    lengths = _cycled_pairs(K_CAMS, K_CYCLE16)
    lengths.update({(K_CAMS + i, 1): L for i, L in enumerate(K16_EXTRA)})
    return lengths


def k128_fill_points():
    """points of K128's filler part (each seen by all 12 filler cameras: 78 tasks): the fewest that bring ntasks to 2^20, where
    build_tasks (csrc/ba_lm.hip) goes to chunk = 128"""
    directed = 3 * sum(_cycled_pairs(K_CAMS, K_CYCLE128).values())
    per = K128_FILL_CAMS * (K128_FILL_CAMS + 1) // 2
    return -((directed - (1 << 20)) // per)


def _k128(ba):
    n = k128_fill_points()
    return merge_scenes([scene_from_pair_lengths(ba, K_CAMS, _cycled_pairs(K_CAMS, K_CYCLE128), 43),
                         scene_from_degrees(ba, K128_FILL_CAMS, np.full(n, K128_FILL_CAMS), 44)])


BOUNDARY_SCENES = {
    "P": lambda ba: scene_from_degrees(ba, P_NCAMS, p_degrees(), 41, window=P_WINDOW),
    "K16": lambda ba: scene_from_pair_lengths(ba, K_CAMS + len(K16_EXTRA) + 1, k16_lengths(), 42),
    "K128": _k128,
}


def _band(ba, ncams, locality, seed):
    """A band of cameras with the density of the suite's two-run problem (1100 cameras, 6000 points, 30000 observations)."""
    npnts = max(200, round(ncams * 6000 / 1100))
    return ba.synthetic.make_problem(ncams, npnts, 5 * npnts, seed=seed, locality=locality)


# name -> (builder, at least 1024 cameras: the two-ended sequence is expected to win as generated)
SCENES = {
    "one band of 1100": (lambda ba: ba.synthetic.make_problem(1100, 6000, 30000, seed=35, locality=0.1), True),
    "two bands of 512": (lambda ba: merge_scenes([_band(ba, 512, 0.2, s) for s in (1, 2)]), True),
    "four bands of 256": (lambda ba: merge_scenes([_band(ba, 256, 0.3, s) for s in (1, 2, 3, 4)]), True),
    "band of 1200 + 256 isolated cameras": (lambda ba: merge_scenes([_band(ba, 1200, 0.1, 35), isolated_cameras(ba, 256, 6, 36)]), True),
    "256 isolated cameras + band of 800": (lambda ba: merge_scenes([isolated_cameras(ba, 256, 6, 36), _band(ba, 800, 0.1, 35)]), True),
    "two bands of 256": (lambda ba: merge_scenes([_band(ba, 256, 0.3, s) for s in (1, 2)]), False),
}


@functools.lru_cache(maxsize=None)
def _scene(ba, name, shuffled):
    p = (BOUNDARY_SCENES[name] if name in BOUNDARY_SCENES else SCENES[name][0])(ba)
    if shuffled:
        p, _ = ba.synthetic.shuffle_cameras(p, seed=8)
    for key in KEYS:
        if isinstance(p[key], np.ndarray):
            p[key].setflags(write=False)  # shared between tests: nobody changes it
    return p


def scene(ba, name, shuffled=False):
    """The scene `name` of SCENES or BOUNDARY_SCENES, as generated or with its cameras renumbered at random (shuffle_cameras(seed=8)); built once."""
    return _scene(ba, name, bool(shuffled))


# ---- seeded per-observation information matrices (tests/test_obs_info.py and the tests that combine the terms) --------------
def blocks(sig1, sig2, angle):
    """(n, 2, 2): rotations by `angle` of diag(1 / sig1^2, 1 / sig2^2), exactly symmetric"""
    c, s = np.cos(angle), np.sin(angle)
    a, b = 1.0 / np.asarray(sig1) ** 2, 1.0 / np.asarray(sig2) ** 2
    out = np.empty((len(angle), 2, 2))
    out[:, 0, 0] = c * c * a + s * s * b
    out[:, 1, 1] = s * s * a + c * c * b
    out[:, 0, 1] = out[:, 1, 0] = c * s * (a - b)
    return out


def random_info(p, seed, frac_zero=0.05, frac_rank1=0.05):
    """Anisotropic information of every observation of p: random rotations of diag(1 / s1^2, 1 / s2^2), s in [0.5, 4]; about
    frac_zero of them exactly 0 and about frac_rank1 rank one (u u' / s^2), drawn only among the observations a point can
    spare: every point keeps at least two full-rank observations (full_rank_per_point checks it)."""
    rng = np.random.default_rng(seed)
    n = p["nobs"]
    info = blocks(rng.uniform(0.5, 4.0, n), rng.uniform(0.5, 4.0, n), rng.uniform(0.0, np.pi, n))
    pnt = np.asarray(p["pnt_idx1"]) - 1
    spare = np.bincount(pnt, minlength=p["npnts"]) - 2  # observations a point can lose
    kind = rng.random(n)
    for o in rng.permutation(n):
        if kind[o] < frac_zero + frac_rank1 and spare[pnt[o]] > 0:
            spare[pnt[o]] -= 1
            if kind[o] < frac_zero:
                info[o] = 0.0
            else:
                th, s = rng.uniform(0.0, np.pi), rng.uniform(0.5, 4.0)
                u = np.array([np.cos(th), np.sin(th)])
                info[o] = np.outer(u, u) / s ** 2
    return clip_psd(info)


def clip_psd(info):
    """the blocks with xy moved towards 0 by as many ulps as it takes for xy^2 <= xx yy to hold in floating point (a rank-one
    block formed in floating point may miss it by one)"""
    bad = info[:, 0, 1] ** 2 > info[:, 0, 0] * info[:, 1, 1]
    while bad.any():
        info[bad, 0, 1] = info[bad, 1, 0] = np.nextafter(info[bad, 0, 1], 0.0)
        bad = info[:, 0, 1] ** 2 > info[:, 0, 0] * info[:, 1, 1]
    return info


def full_rank_per_point(p, info):
    """the smallest number of full-rank (det > 1e-8 trace^2) observations any point has"""
    det = info[:, 0, 0] * info[:, 1, 1] - info[:, 0, 1] ** 2
    tr = info[:, 0, 0] + info[:, 1, 1]
    full = det > 1e-8 * tr ** 2
    return int(np.bincount(np.asarray(p["pnt_idx1"]) - 1, weights=full.astype(float), minlength=p["npnts"]).min())
