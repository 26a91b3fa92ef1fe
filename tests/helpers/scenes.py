"""Scenes the package's generator never draws by itself (test code; synthetic.make_problem and its random draws are untouched):
several problems merged into one -- a camera graph with several connected components -- and cameras that share no point with
any other camera.  Used by tests/test_block_sparse_scenes.py."""
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
    p = SCENES[name][0](ba)
    if shuffled:
        p, _ = ba.synthetic.shuffle_cameras(p, seed=8)
    for key in KEYS:
        if isinstance(p[key], np.ndarray):
            p[key].setflags(write=False)  # shared between tests: nobody changes it
    return p


def scene(ba, name, shuffled=False):
    """The scene `name` of SCENES, as generated or with its cameras renumbered at random (shuffle_cameras(seed=8)); built once."""
    return _scene(ba, name, bool(shuffled))
