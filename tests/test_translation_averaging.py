"""Translation averaging over the view graph (ba_translation_loops, ba_average_translations, ba_transavg_lm_decide,
include/ba_hip.h; translation_loops, average_translations, translation_directions and camera_translations of the
package, synthetic.relative_translations).  The reference is tests/helpers/transavg_ref.py: the header restated in numpy.  The
first tests need no device; the rest run on the GPU.

Scenes (synthetic.relative_translations at 0.01 rad of noise, turned into world directions by translation_directions with the
true rotations; about half of the pairs are listed as (b, a)):
  K12       the complete graph on 12 cameras, no gross pair
  K16       the complete graph on 16 cameras, 20 % gross
  band24w8  24 cameras along a curve, each paired with its 8 neighbours on either side, 10 % gross
  hub       70 cameras: 2..70 in a band of +-2, camera 1 paired with all (degree 69: a wave strides its list twice); no gross pair
  two       cameras 1..10 in a band of +-3, camera 11 without a pair, cameras 12 and 13 with one pair: two components, one of
            a single pair, and an isolated camera; no gross pair
  line      cameras 1, 2, 3 on one line and 4, 5 off it, all pairs, no noise: of the triangles of 1, 2, 3 one has its arc
            shrunk to a point (|n| < 1e-6, d1 . d2 > 0) and two cannot be checked (d1 . d2 < 0)
Seeds were chosen on the reference, never on the device.

Bounds.  Full solves: B = max(100 x the largest distance of a camera between the reference's run and its run with the directed
edge list permuted, 1e-9) x the scene radius.  One solve: max(100 x the distance of the reference's own conjugate gradient to
a dense solve of its system, 1e-10 |delta|_inf)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import pair_ref  # noqa: E402
import rotavg_ref as ra  # noqa: E402
import transavg_ref as tr  # noqa: E402
from refine_util import _model, bits, small_scene  # noqa: E402

DEG = np.pi / 180.0
NOISE = 0.01
ROBUST = dict(loops=dict(threshold=5 * DEG, min_ratio=0.34), loss="huber", f_scale=0.05)
SEEDS = dict(K12=2, K16=3, band24w8=0, hub=0, two=0, line=0)
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def band(lo, n, w):
    return [(i, j) for i in range(lo, lo + n) for j in range(i + 1, min(lo + n, i + w + 1))]


def graph_of(name):
    """(ncams, pairs as listed before the orientation is mixed, gross share, noise)"""
    if name == "K12":
        return 12, band(1, 12, 12), 0.0, NOISE
    if name == "K16":
        return 16, band(1, 16, 16), 0.2, NOISE
    if name == "band24w8":
        return 24, band(1, 24, 8), 0.1, NOISE
    if name == "hub":
        return 70, sorted(set(band(2, 69, 2)) | {(1, j) for j in range(2, 71)}), 0.0, NOISE
    if name == "two":
        return 13, band(1, 10, 3) + [(12, 13)], 0.0, NOISE
    if name == "line":
        return 5, band(1, 5, 5), 0.0, 0.0
    raise KeyError(name)


def scene(ba, name):
    """dict(n, pairs, dirs, gross, C_true, r_true, radius)"""
    def build():
        n, pairs, frac, noise = graph_of(name)
        seed = SEEDS[name]
        rng = np.random.default_rng(seed)
        pairs = np.array(pairs, dtype=np.int64)
        flip = rng.random(len(pairs)) < 0.5
        pairs[flip] = pairs[flip][:, ::-1]
        r_true = rng.normal(size=(n, 3))
        if name in ("band24w8", "hub", "two"):
            i = np.arange(n, dtype=np.float64)
            centres = np.stack([0.4 * i, np.sin(0.5 * i), np.cos(0.3 * i)], axis=1) + 0.3 * rng.normal(size=(n, 3))
        elif name == "line":
            centres = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 4.0], [4.0, 8.0, 8.0], [1.0, -1.0, 0.5], [-2.0, 0.0, 3.0]])
        else:
            centres = rng.normal(size=(n, 3))
        T = ba.camera_translations(r_true, centres)
        x = np.concatenate([r_true, T, np.zeros((n, 3))], axis=1).ravel()
        t, gross = ba.synthetic.relative_translations(x, 0, pairs, noise=noise, outlier_fraction=frac, seed=seed + 100)
        dirs = ba.translation_directions(pairs, t, r_true)
        dirs = dirs * rng.uniform(0.5, 2.0, size=(len(dirs), 1))  # (not normalised: the device does that)
        return dict(n=n, pairs=pairs, dirs=dirs, t=t, x=x, gross=gross, C_true=centres, r_true=r_true,
                    radius=float(np.linalg.norm(centres - centres.mean(axis=0), axis=1).max()))
    return cached(("scene", name), build)


def model_of(ba, n):
    """a handle with n cameras: translation averaging reads the device, the stream and ncams of it"""
    return _model(ba, cached(("problem", n), lambda: ba.synthetic.make_problem(n, 4 * n, 12 * n, seed=1)))


def start_of(ba, name, seed=3):
    """a c0 for a scene: the true centres moved by 5 % of the radius each"""
    s = scene(ba, name)
    return s["C_true"] + 0.05 * s["radius"] * np.random.default_rng(seed).normal(size=(s["n"], 3))


def ref_run(ba, name, edge_seed=None, **kw):
    """the reference on a scene under the keywords of average_translations (fixed_cameras 1-based)"""
    def build():
        s = scene(ba, name)
        k = dict(kw)
        fixed = np.zeros(s["n"], dtype=bool)
        fixed[np.asarray(k.pop("fixed_cameras", []), dtype=np.int64) - 1] = True
        return tr.average(s["n"], s["pairs"], s["dirs"], loops_opt=k.pop("loops", None), fixed=fixed, loss=k.pop("loss", None) or "linear",
                          edge_seed=edge_seed, **k)
    key = ("ref", name, edge_seed, repr(sorted((q, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for q, v in kw.items())))
    return cached(key, build)


def spread(ba, name, **kw):
    a, b = ref_run(ba, name, **kw), ref_run(ba, name, edge_seed=7, **kw)
    live = a["component"] >= 0
    return float(np.linalg.norm(a["c"] - b["c"], axis=1)[live].max())


def bound(ba, name, **kw):
    return max(100.0 * spread(ba, name, **kw), 1e-9 * scene(ba, name)["radius"])


def dev_run(ba, name, **kw):
    s = scene(ba, name)
    m = model_of(ba, s["n"])
    try:
        return ba.average_translations(m, s["pairs"], s["dirs"], **kw)
    finally:
        m.close()


def recovery(s, o):
    """(gross pairs kept, share of the clean pairs dropped, worst camera error after a similarity alignment over the scene
    radius, largest residual of a kept clean pair in degrees, smallest residual of a dropped gross pair in degrees)"""
    used = np.isfinite(s["dirs"]).all(axis=1)
    err = np.linalg.norm(tr.align(o["c"], s["C_true"]) - s["C_true"], axis=1)
    res = o["residual"] / DEG
    dropped_gross = used & ~o["kept"] & s["gross"]
    return (int((o["kept"] & s["gross"]).sum()), float((used & ~o["kept"] & ~s["gross"]).sum() / max(1, (used & ~s["gross"]).sum())),
            float(np.nanmax(err) / s["radius"]), float(res[o["kept"] & ~s["gross"]].max()),
            float(np.nanmin(res[dropped_gross])) if dropped_gross.any() else np.inf)


def assert_recovered(s, o):
    kept_gross, dropped, err, res_clean, res_gross = recovery(s, o)
    print(f"gross kept {kept_gross}, clean dropped {100 * dropped:.1f} %, camera error {100 * err:.2f} % of the radius, kept clean "
          f"residual <= {res_clean:.2f} deg, dropped gross residual >= {res_gross:.1f} deg, {o['iterations']} iterations, "
          f"{o['cg_iterations']} CG iterations")
    assert kept_gross <= 2 and dropped <= 0.05 and err <= 0.05 and res_clean <= 5.0 and res_gross >= 5.0


SOLVE_SCENES = ("K12", "K16", "band24w8")


def solve_options(ba, name, loss, held):
    """the full solves run behind the loop filter under either loss: without it the gross pairs of K16 and band24w8 leave
    Levenberg-Marquardt wandering between wrong minima for all of its 50 iterations"""
    kw = dict(ROBUST) if loss == "huber" else dict(loops=ROBUST["loops"])
    if held:
        kw.update(c0=start_of(ba, name), fixed_cameras=[2, scene(ba, name)["n"] - 1])
    return kw


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_julia_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    for name in ("ba_translation_loops", "ba_average_translations"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header and f"(:{name}, libba)" in julia
    assert "ba_transavg_lm_decide" in lib.SYMBOLS and "int ba_transavg_lm_decide(" in header
    for fn in ("translation_loops", "average_translations"):
        assert f"function {fn}(" in julia and fn in ba.__all__ and callable(getattr(ba, fn))
    for fn in ("translation_directions", "camera_translations"):
        assert fn in ba.__all__ and callable(getattr(ba, fn))
    assert "enum { BA_TA_OK = 0, BA_TA_ROOT = 1, BA_TA_FIXED = 2, BA_TA_ISOLATED = 3, BA_TA_STATES = 4 };" in header
    assert "typedef struct ba_transavg_opts {" in header and "struct BaTransavgOpts" in julia
    assert lib.TRANSAVG_STATES == ("ok", "root", "fixed", "isolated")
    for word in ("translation averaging", "listed twice", "min(16, remaining)", "(double)support < min_ratio * (double)n_loops",
                 "1DSfM", "pairwise baseline lengths", "Float32", "several ranks", "ba_average_rotations onto the conjugate gradient",
                 "rho(4 / c^2)", "asin min(1, |d_k . n^|)"):
        assert word in header, word
    names = [f[0] for f in lib.TransavgOpts._fields_]
    body = header[header.index("typedef struct ba_transavg_opts {"):header.index("} ba_transavg_opts;")]
    assert [w.split("/*")[0].split()[-1].rstrip(";") for w in body.splitlines()[1:] if ";" in w.split("/*")[0]] == names
    jbody = julia[julia.index("struct BaTransavgOpts"):]
    assert [w.split()[0] for w in jbody[:jbody.index("\nend")].splitlines()[1:] if "::" in w] == names

    def opts(**over):
        return lib.TransavgOpts(**dict(dict(loss=0, loops=0, min_support=0, max_iterations=0, max_cg=0, f_scale=0.0, loop_threshold=0.0,
                                            min_ratio=0.0, ftol=0.0, cg_tol=0.0, lambda0=0.0), **over))
    who, tail = b"ba_average_translations", (None,) * 13
    # a null handle, null options, each bad option
    assert L.ba_average_translations(None, 0, None, None, None, None, None, None, None, C.byref(opts()), *tail) == 1
    assert who in L.ba_last_error() and b"null argument" in L.ba_last_error()
    assert L.ba_average_translations(None, 0, None, None, None, None, None, None, None, None, *tail) == 1 and b"null options" in L.ba_last_error()
    for bad, word in ((dict(loss=5), b"loss"), (dict(loss=-1), b"loss"), (dict(loss=1), b"f_scale"), (dict(loss=1, f_scale=-1.0), b"f_scale"),
                      (dict(loss=3, f_scale=np.nan), b"f_scale"), (dict(max_iterations=100001), b"max_iterations"), (dict(max_cg=100001), b"max_cg"),
                      (dict(ftol=np.nan), b"ftol"), (dict(cg_tol=np.inf), b"cg_tol"), (dict(lambda0=np.nan), b"lambda0"),
                      (dict(loops=1), b"loop_threshold"), (dict(loops=1, loop_threshold=np.inf), b"loop_threshold"),
                      (dict(loops=1, loop_threshold=0.1, min_ratio=1.5), b"min_ratio"), (dict(loops=1, loop_threshold=0.1, min_ratio=-0.1), b"min_ratio"),
                      (dict(loops=1, loop_threshold=0.1, min_ratio=np.nan), b"min_ratio")):
        assert L.ba_average_translations(None, 0, None, None, None, None, None, None, None, C.byref(opts(**bad)), *tail) == 1
        msg = L.ba_last_error()
        assert word in msg and who in msg, (bad, msg)
    for good in (opts(loss=1, f_scale=0.1, max_iterations=100000, max_cg=100000), opts(loops=1, loop_threshold=0.05, min_support=2, min_ratio=1.0)):
        assert L.ba_average_translations(None, 0, None, None, None, None, None, None, None, C.byref(good), *tail) == 1
        assert b"null argument" in L.ba_last_error()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert L.ba_translation_loops(None, 0, None, None, None, None, tau, None, None) == 1 and b"threshold" in L.ba_last_error()
    assert L.ba_translation_loops(None, 0, None, None, None, None, 0.1, None, None) == 1
    assert b"ba_translation_loops" in L.ba_last_error() and b"null argument" in L.ba_last_error()
    # Python: ValueError before any device call (None stands in for the model)
    assert ba.average_translations.__kwdefaults__ == dict(weights=None, used=None, loops=None, c0=None, fixed_cameras=None, loss=None,
                                                          f_scale=None, max_iterations=None, ftol=None, cg_tol=None, max_cg=None)
    assert ba.translation_loops.__kwdefaults__ == dict(used=None) and "threshold" in ba.translation_loops.__code__.co_varnames
    pairs, d = [[1, 2], [2, 3]], np.ones((2, 3))
    for bad in (dict(loss="huber"), dict(loss="tukey"), dict(loss="cauchy", f_scale=0.0), dict(loss="huber", f_scale=float("nan")),
                dict(max_iterations=0), dict(max_iterations=100001), dict(max_iterations=2.5), dict(max_cg=0), dict(max_cg=100001), dict(max_cg=True),
                dict(ftol=float("nan")), dict(ftol="a"), dict(ftol=0.0), dict(cg_tol=-1.0), dict(cg_tol=float("inf")),
                dict(loops=dict()), dict(loops=dict(threshold=0.0)), dict(loops=dict(threshold=0.1, tau=1)),
                dict(loops=dict(threshold=0.1, min_support=0)), dict(loops=dict(threshold=0.1, min_ratio=1.5)),
                dict(loops=dict(threshold=0.1, min_ratio=float("nan"))), dict(loops=dict(threshold=0.1, min_ratio=None)), dict(loops=0.1),
                dict(weights=[1.0, -1.0]), dict(weights=[1.0]), dict(weights=[1.0, float("inf")]), dict(used=[1, 0]), dict(used=[True]),
                dict(fixed_cameras=[1]), dict(fixed_cameras=[0], c0=np.zeros((3, 3))), dict(c0=np.zeros((3, 2))),
                dict(c0=np.array([[0.0, 0, 0], [np.nan, 0, 0], [0, 0, 0]])), dict(c0=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            ba.average_translations(None, pairs, d, **bad)
    for bad_pairs in ([[1, 2], [2, 1]], [[1, 2], [1, 2]], [[1, 1]], [[0, 1]], [1, 2], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            ba.average_translations(None, bad_pairs, np.ones((len(bad_pairs), 3)))
        with pytest.raises(ValueError):
            ba.translation_loops(None, bad_pairs, np.ones((len(bad_pairs), 3)), threshold=0.1)
    with pytest.raises(ValueError, match="directions must have shape"):
        ba.average_translations(None, pairs, np.ones((3, 3)))
    with pytest.raises(ValueError, match="directions must have shape"):
        ba.translation_loops(None, pairs, np.ones((2, 2)), threshold=0.1)
    for tau in (0.0, float("nan"), "a", None):
        with pytest.raises(ValueError, match="threshold"):
            ba.translation_loops(None, pairs, d, threshold=tau)
    for bad in (dict(t=np.ones((3, 3))), dict(r_abs=np.ones((3, 2))), dict(r_abs=np.ones((2, 3))), dict(t="a")):
        with pytest.raises(ValueError):
            ba.translation_directions(pairs, **dict(dict(t=np.ones((2, 3)), r_abs=np.zeros((3, 3))), **bad))
    with pytest.raises(ValueError):
        ba.camera_translations(np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        ba.synthetic.relative_translations(np.zeros(18), 0, [[1, 3]])
    with pytest.raises(ValueError):
        ba.synthetic.relative_translations(np.zeros(18), 0, [[1, 2]], noise=-1.0)

    class Sizes:
        ncams = 2
    with pytest.raises(ValueError, match="1..2"):
        ba.average_translations(Sizes, pairs, d)
    with pytest.raises(ValueError, match="1..2"):
        ba.translation_loops(Sizes, pairs, d, threshold=0.1)


def test_lm_control_on_scripted_costs(ba):
    """ba_transavg_lm_decide (csrc/ba_transavg_control.h) against the rule written out, and against the reference's copy"""
    L = ba._lib.lib()

    def decide(F, Ft, lam, it, max_it=50, ftol=1e-10):
        nxt, stop = C.c_double(0.0), C.c_int(-1)
        acc = L.ba_transavg_lm_decide(F, Ft, lam, it, max_it, ftol, C.byref(nxt), C.byref(stop))
        assert (bool(acc), stop.value, nxt.value) == tr.lm_decide(F, Ft, lam, it, max_it, ftol)
        return acc, stop.value, nxt.value
    assert decide(10.0, 5.0, 1e-3, 1) == (1, 0, 1e-3 / 3.0)             # a decrease: accepted, lambda / 3
    assert decide(10.0, 12.0, 1e-3, 1) == (0, 0, 4e-3)                  # an increase: rejected, 4 lambda
    assert decide(10.0, 10.0, 1e-3, 1) == (0, 1, 4e-3)                  # no change: not accepted, and the tolerance stops it
    assert decide(10.0, float("nan"), 1e-3, 1) == (0, 0, 4e-3)          # a NaN trial is rejected and stops nothing
    assert decide(10.0, float("inf"), 1e-3, 1) == (0, 0, 4e-3)
    assert decide(10.0, 9.0, 2e-9, 1) == (1, 0, 1e-9)                   # the floor of lambda
    assert decide(10.0, 10.0 - 5e-10, 1e-3, 1) == (1, 1, 1e-3 / 3.0)    # a relative decrease of 5e-11 < ftol: accepted, stop
    assert decide(10.0, 10.0 + 5e-10, 1e-3, 1) == (0, 1, 4e-3)          # an increase as small: rejected, stop
    assert decide(10.0, 10.0 - 5e-9, 1e-3, 1)[1] == 0                   # 5e-10 > ftol: go on
    assert decide(10.0, 11.0, 3e7, 7) == (0, 2, 1.2e8)                  # lambda passes 1e8
    assert decide(10.0, 11.0, 2.5e7, 7) == (0, 0, 1e8)                  # (1e8 itself does not)
    assert decide(10.0, 9.0, 1e-3, 50) == (1, 3, 1e-3 / 3.0)            # the last iteration
    assert decide(10.0, 9.0, 1e-3, 49)[1] == 0
    assert decide(10.0, 10.0, 3e7, 50)[1] == 1 and decide(10.0, 11.0, 3e7, 50)[1] == 2  # the first reason that holds
    assert decide(0.0, 0.0, 1e-3, 1) == (0, 1, 4e-3)                    # a zero cost stops at once
    assert L.ba_transavg_lm_decide(10.0, 5.0, 1e-3, 1, 50, 1e-10, None, None) == 1
    # a scripted solve: the sequence of lambdas and the iteration it stops at
    F, lam, seq = 100.0, 1e-3, []
    for it, Ft in enumerate([50.0, 60.0, 70.0, 20.0, 19.0, 19.0 - 1e-9], start=1):
        acc, stop, lam = decide(F, Ft, lam, it)
        seq.append((acc, stop))
        F = Ft if acc else F
    assert seq == [(1, 0), (0, 0), (0, 0), (1, 0), (1, 0), (1, 1)] and F == 19.0 - 1e-9
    assert abs(lam / (1e-3 / 3 * 16 / 27) - 1.0) < 1e-12


def test_directions_translations_and_the_generator(ba):
    """translation_directions and camera_translations against a scene's true poses; relative_translations without noise is the
    t of relative_pose (tests/helpers/pair_ref.true_relative)"""
    p = small_scene(ba)
    n, npnts = p["ncams"], p["npnts"]
    cams = pair_ref.cameras(p, p["x_true"])
    R = ra.exp_many(cams[:, :3])
    centres = -np.einsum("kji,kj->ki", R, cams[:, 3:6])
    assert np.abs(ba.camera_translations(cams[:, :3], centres) - cams[:, 3:6]).max() <= 1e-12 * np.abs(cams[:, 3:6]).max()
    pairs = np.array([(a, b) if (a + b) % 2 else (b, a) for a in range(1, n + 1) for b in range(a + 1, n + 1)], dtype=np.int64)
    t, gross = ba.synthetic.relative_translations(p["x_true"], npnts, pairs)
    assert not gross.any() and np.abs(np.linalg.norm(t, axis=1) - 1.0).max() <= 1e-15
    for k, (a, b) in enumerate(pairs):
        assert np.abs(t[k] - pair_ref.true_relative(p, p["x_true"], a - 1, b - 1)[1]).max() <= 1e-13
    d = ba.translation_directions(pairs, t, cams[:, :3])
    u = centres[pairs[:, 1] - 1] - centres[pairs[:, 0] - 1]
    assert np.abs(d - u / np.linalg.norm(u, axis=1)[:, None]).max() <= 1e-12
    # noise and gross pairs: the share, the size of the perturbation, unit length
    t2, gross2 = ba.synthetic.relative_translations(p["x_true"], npnts, pairs, noise=0.01, outlier_fraction=0.25, seed=4)
    assert gross2.sum() == len(pairs) // 4 and np.abs(np.linalg.norm(t2, axis=1) - 1.0).max() <= 1e-15
    off = np.arccos(np.clip((t * t2).sum(axis=1), -1, 1))
    assert 0.005 < np.median(off[~gross2]) < 0.03 and off[~gross2].max() < 0.06 and np.median(off[gross2]) > 0.5
    # a pair without a pose, a camera without a rotation: NaN
    t3, r3 = t.copy(), cams[:, :3].copy()
    t3[0], r3[pairs[1, 1] - 1] = np.nan, np.nan
    d3 = ba.translation_directions(pairs, t3, r3)
    assert np.isnan(d3[0]).all() and np.isnan(d3[1]).all() and np.isnan(ba.camera_translations(r3, centres)[pairs[1, 1] - 1]).all()


def test_reference_conditions(ba):
    """The conditions of the GPU tests, on the reference alone"""
    # the arc distance on the sphere, case by case
    x, y, z = np.eye(3)
    mid = (x + y) / np.sqrt(2.0)
    assert abs(tr.arc_distance(mid, x, y)) <= 1e-15                                         # on the arc
    up = (mid + 0.1 * z) / np.linalg.norm(mid + 0.1 * z)
    assert abs(tr.arc_distance(up, x, y) - np.arctan(0.1)) <= 1e-15                         # above the arc: the distance to its plane
    out = (x - 0.2 * y) / np.linalg.norm(x - 0.2 * y)
    assert abs(tr.arc_distance(out, x, y) - np.arctan(0.2)) <= 1e-15                        # past an end: the distance to that end
    assert abs(tr.arc_distance(-mid, x, y) - 0.75 * np.pi) <= 1e-15                         # the far side of the great circle
    assert abs(tr.arc_distance(z, x, x) - 0.5 * np.pi) <= 1e-15 and tr.arc_distance(z, x, -x) is None
    for name in ("K12", "K16", "band24w8", "hub", "line"):
        s = scene(ba, name)
        nl, sup, dist, unchecked = tr.loops(s["n"], s["pairs"], s["dirs"], 5 * DEG)
        assert dist.size and np.abs(dist - 5 * DEG).min() > 1e-6, name
        assert (unchecked > 0) == (name == "line")
    s = scene(ba, "line")
    nl, sup, dist, unchecked = tr.loops(s["n"], s["pairs"], s["dirs"], 5 * DEG)
    assert unchecked == 2 and nl.sum() == 3 * 10 - 2 and np.array_equal(nl, sup)
    on_line = [k for k, (a, b) in enumerate(s["pairs"]) if a <= 3 and b <= 3]
    assert sorted(nl[on_line]) == [2, 2, 3]
    for name in ("K16", "band24w8"):
        s = scene(ba, name)
        assert_recovered(s, ref_run(ba, name, **ROBUST))
    plain = recovery(scene(ba, "K16"), ref_run(ba, "K16"))
    print("K16, every pair and the linear loss:", plain)
    assert plain[2] > 0.05
    for name in SOLVE_SCENES:
        for loss in ("linear", "huber"):
            for held in (False, True):
                o = ref_run(ba, name, **solve_options(ba, name, loss, held))
                other = ref_run(ba, name, edge_seed=7, **solve_options(ba, name, loss, held))
                change = np.abs(o["F"] - o["trace"][:, 0]) / o["F"]
                print(f"{name} {loss} held={held}: {o['iterations']} iterations, {o['cg_iterations']} CG iterations, accepted "
                      f"{o['trace'][:, 3].astype(int).tolist()}, smallest change {change.min():.1e}, spread {spread(ba, name, **solve_options(ba, name, loss, held)):.1e}")
                assert o["iterations"] < 50 and o["trace"][:, 3].all() and change[-1] <= 1e-10 and (change[:-1] > 1e-10).all()
                # every decision is safe from rounding: F sums a few hundred terms, so two evaluations differ by about 1e-15 F, and
                # no change lies within 1 % of ftol (the last change is below ftol by construction: see DESIGN 5v)
                assert change.min() >= 1e-13 and np.abs(change / 1e-10 - 1.0).min() > 0.01
                for norms, r0 in o["solves"]:
                    assert len(norms) < 500 and norms[-1] <= 1e-6 * r0
                    assert np.abs(np.array(norms) / (1e-6 * r0) - 1.0).min() > 0.01
                assert np.array_equal(o["trace"][:, 2:], other["trace"][:, 2:])


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["K12", "K16", "band24w8", "hub", "line"])
def test_loop_counts(ba, gpu_ok, name):
    s = scene(ba, name)
    used = None
    if name == "K16":  # two pairs the caller has ruled out
        used = np.ones(len(s["pairs"]), dtype=bool)
        used[[3, 40]] = False
    m = model_of(ba, s["n"])
    try:
        n_loops, support = ba.translation_loops(m, s["pairs"], s["dirs"], threshold=5 * DEG, used=used)
        everything = ba.translation_loops(m, s["pairs"], s["dirs"], threshold=np.pi, used=used)
    finally:
        m.close()
    want = tr.loops(s["n"], s["pairs"], s["dirs"], 5 * DEG, used=used)
    assert np.array_equal(n_loops, want[0]) and np.array_equal(support, want[1])
    assert np.array_equal(everything[0], want[0]) and np.array_equal(everything[1], want[0])
    assert n_loops.max() == {"K12": 10, "K16": 14, "band24w8": 14, "hub": 4, "line": 3}[name]
    if used is not None:
        assert not n_loops[~used].any() and not support[~used].any()


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["linear", "huber"])
@pytest.mark.parametrize("name", ["K12", "K16", "band24w8", "hub"])
def test_one_solve(ba, gpu_ok, name, loss):
    """one linearisation and one conjugate-gradient solve at lambda = 1e-3, cg_tol 1e-12: with two held cameras and one
    iteration the result is c0 + delta"""
    s = scene(ba, name)
    kw = dict(c0=start_of(ba, name), fixed_cameras=[2, s["n"] - 1], max_iterations=1, cg_tol=1e-12)
    if loss == "huber":
        kw.update(loss="huber", f_scale=0.05)
    want = ref_run(ba, name, **kw)
    H, rhs, idx = want["first"]["H"]
    dense = np.zeros((s["n"], 3))
    dense[idx] = np.linalg.solve(H, rhs).reshape(-1, 3)
    own = np.abs(want["first"]["delta"] - dense).max()
    B = max(100.0 * own, 1e-10 * np.abs(dense).max())
    got = dev_run(ba, name, **kw)
    assert got["iterations"] == 1 and got["trace"][0, 3] == 1 and want["trace"][0, 3] == 1
    delta = got["c"] - kw["c0"]
    dist = np.abs(delta - dense).max()
    print(f"{name} {loss}: |delta| = {np.abs(dense).max():.2e}, reference PCG to dense {own:.2e}, device to dense {dist:.2e}, bound {B:.2e}, "
          f"CG iterations {got['cg_iterations']} (reference {want['cg_iterations']})")
    assert dist <= B
    assert same(got["c"][[1, -2]], kw["c0"][[1, -2]]) and list(got["status"][[1, -2]]) == ["fixed", "fixed"]


@pytest.mark.gpu
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("loss", ["linear", "huber"])
@pytest.mark.parametrize("name", SOLVE_SCENES)
def test_full_solve(ba, gpu_ok, name, loss, held):
    kw = solve_options(ba, name, loss, held)
    s, want, B = scene(ba, name), ref_run(ba, name, **kw), bound(ba, name, **kw)
    got = dev_run(ba, name, **kw)
    live = want["component"] >= 0
    dist = np.linalg.norm(got["c"] - want["c"], axis=1)[live].max()
    print(f"{name} {loss} held={held}: {got['iterations']} iterations (reference {want['iterations']}), CG {got['trace'][:, 2].astype(int).tolist()} "
          f"(reference {want['trace'][:, 2].astype(int).tolist()}), |c - c_ref| <= {dist:.2e}, B = {B:.2e}, radius {s['radius']:.2f}, "
          f"cost {got['cost_before']:.6e} -> {got['cost_after']:.6e}")
    assert got["iterations"] == want["iterations"] and np.array_equal(got["trace"][:, 3], want["trace"][:, 3])
    assert np.array_equal(got["trace"][:, 2], want["trace"][:, 2]) and got["cg_iterations"] == want["cg_iterations"]
    assert dist <= B
    assert (got["status"] == want["status"]).all() and np.array_equal(got["component"], want["component"])
    assert np.array_equal(got["kept"], want["kept"]) and got["counts"] == want["counts"]
    assert np.array_equal(got["n_loops"], want["n_loops"]) and np.array_equal(got["support"], want["support"])
    assert np.array_equal(np.isnan(got["residual"]), np.isnan(want["residual"]))
    rel = B / s["radius"] * 1e3  # (an angle moves by |dc| / |u|; the shortest baseline is above a thousandth of the radius)
    assert np.nanmax(np.abs(got["residual"] - want["residual"])) <= rel
    assert np.abs(got["trace"][:, :2] - want["trace"][:, :2]).max() <= rel * (1.0 + np.abs(want["trace"][:, :2]).max())
    for key in ("cost_before", "cost_after"):
        assert abs(got[key] - want[key]) <= rel * (1.0 + want[key])
    assert got["cost_after"] <= got["cost_before"]
    if held:
        assert same(got["c"][[1, -2]], kw["c0"][[1, -2]]) and "root" not in got["status"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["K16", "band24w8"])
def test_recovery(ba, gpu_ok, name):
    """The filtered robust call recovers every camera; the call on every pair under the linear loss does not"""
    s = scene(ba, name)
    assert_recovered(s, dev_run(ba, name, **ROBUST))
    if name == "K16":
        plain = recovery(s, dev_run(ba, name))
        print("every pair and the linear loss:", plain)
        assert plain[2] > 0.05


@pytest.mark.gpu
def test_gauge_and_components(ba, gpu_ok):
    s = scene(ba, "two")
    m = model_of(ba, s["n"])
    try:
        kw = dict(loss="huber", f_scale=0.05)
        a = ba.average_translations(m, s["pairs"], s["dirs"], **kw)
        want = ref_run(ba, "two", **kw)
        assert "n_loops" not in a  # (no loop filter asked for)
        roots = np.flatnonzero(a["status"] == "root")
        assert len(roots) == 2 and a["counts"] == dict(ok=10, root=2, fixed=0, isolated=1) and a["counts"] == want["counts"]
        assert same(a["c"][roots], np.zeros((2, 3)))  # the roots are back at their start
        assert np.isnan(a["c"][10]).all() and a["status"][10] == "isolated" and a["component"][10] == -1
        assert np.isfinite(np.delete(a["c"], 10, axis=0)).all()
        # the mean kept baseline is that of the start: 1 on the forest, and the reference's start elsewhere
        p0 = s["pairs"] - 1
        length = lambda c: np.linalg.norm(c[p0[:, 1]] - c[p0[:, 0]], axis=1)  # noqa: E731
        for gi in (0, 1):
            kk = a["kept"] & (a["component"][p0[:, 0]] == gi)
            assert abs(length(a["c"])[kk].mean() / length(want["c_start"])[kk].mean() - 1.0) <= 1e-14
        assert abs(length(a["c"])[-1] - 1.0) <= 1e-15  # the component of one pair: its baseline has length 1
        assert np.linalg.norm(a["c"] - want["c"], axis=1)[want["component"] >= 0].max() <= bound(ba, "two", **kw)
        # another direction in the second component: the first keeps its bits
        d2 = s["dirs"].copy()
        d2[-1] = [0.3, -0.5, 0.8]
        b = ba.average_translations(m, s["pairs"], d2, **kw)
        assert same(a["c"][:10], b["c"][:10]) and not same(a["c"][11:], b["c"][11:]) and same(a["residual"][:-1], b["residual"][:-1])
        # a pair across the two components is NaN while it is not used
        pairs3, d3 = np.concatenate([s["pairs"], [[4, 12]]]), np.concatenate([s["dirs"], [[np.nan] * 3]])
        c = ba.average_translations(m, pairs3, d3, **kw)
        assert np.isnan(c["residual"][-1]) and not c["kept"][-1] and same(c["c"], a["c"])
        zero = ba.average_translations(m, pairs3, np.concatenate([s["dirs"], [[0.0, 1e-13, 0.0]]]), **kw)  # (a norm below 1e-12)
        assert not zero["kept"][-1] and same(zero["c"], a["c"])
        # a start of its own: the roots return to it; the result as a start stops in one iteration
        c0 = start_of(ba, "two")
        d = ba.average_translations(m, s["pairs"], s["dirs"], c0=c0, **kw)
        roots = np.flatnonzero(d["status"] == "root")
        assert same(d["c"][roots], c0[roots]) and d["iterations"] > 1
        for gi in (0, 1):
            kk = d["kept"] & (d["component"][p0[:, 0]] == gi)
            assert abs(length(d["c"])[kk].mean() / length(c0)[kk].mean() - 1.0) <= 1e-14
        again = ba.average_translations(m, s["pairs"], s["dirs"], c0=np.where(np.isnan(d["c"]), 0.0, d["c"]), **kw)
        assert again["iterations"] == 1
        assert np.abs(again["c"] - d["c"])[d["component"] >= 0].max() <= 1e-6 * s["radius"]
    finally:
        m.close()


@pytest.mark.gpu
def test_determinism(ba, gpu_ok):
    """two calls give the same bits; max_cg does not change a solve that converges below it (batches of 16: 500 ends a batch
    early, 512 does not); a call between two LM solves on one handle leaves the second solve with the first's bits"""
    s = scene(ba, "K16")
    m = model_of(ba, s["n"])
    try:
        a = ba.average_translations(m, s["pairs"], s["dirs"], **ROBUST)
        b = ba.average_translations(m, s["pairs"], s["dirs"], **ROBUST)
        c = ba.average_translations(m, s["pairs"], s["dirs"], max_cg=512, **ROBUST)
        la, lb = (ba.translation_loops(m, s["pairs"], s["dirs"], threshold=5 * DEG) for _ in range(2))
    finally:
        m.close()
    for other in (b, c):
        for key in ("c", "residual", "edge_weight", "trace", "cost_before", "cost_after"):
            assert same(a[key], other[key]), key
        assert a["iterations"] == other["iterations"] and a["cg_iterations"] == other["cg_iterations"] and np.array_equal(a["kept"], other["kept"])
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
    assert (a["trace"][:, 2] % 16 != 0).any() and a["trace"][:, 2].max() < 500
    q, k12 = small_scene(ba), scene(ba, "K12")
    ms = _model(ba, q)
    try:
        solve = lambda: ba.Levenberg_Marquardt(ba.FeasibilityResidual(ms), "LDL", "AMD", "None", False, x=q["x0"], ite_max=4)  # noqa: E731
        first = solve()
        between = ba.average_translations(ms, k12["pairs"], k12["dirs"], **ROBUST)
        second = solve()
    finally:
        ms.close()
    assert same(first.solution, second.solution) and same(first.objective, second.objective) and first.iter == second.iter
    assert same(between["c"], dev_run(ba, "K12", **ROBUST)["c"])
