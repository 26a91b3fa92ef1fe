"""Rotation averaging over the view graph (ba_rotation_loops, ba_view_graph_forest, ba_average_rotations, include/ba_hip.h;
DESIGN §5u; rotation_loops, view_graph_forest and average_rotations of the package).  The reference is
tests/helpers/rotavg_ref.py: the header restated in numpy.  The first tests need no device; the rest run on the GPU.

Scenes (synthetic.relative_rotations at 0.5 degrees of noise; the cameras' true rotations are random; about half of the pairs
are listed as (b, a)):
  band24   24 cameras, each paired with its 4 neighbours on either side, 20 % gross; three more pairs are listed unused
  K12      the complete graph on 12 cameras, 20 % gross
  K70      the complete graph on 70 cameras, 30 % gross: adjacency lists longer than a wave
  hub      140 cameras: 1..139 in a band of +-2, camera 1 paired with all (degree 139), camera 140 with camera 1 alone
           (a pendant camera); no gross pair; one more pair has r = NaN and is unused by default
  ring24   an even ring (bipartite), no gross pair
  two      two bands of 10 cameras (+-3) and camera 11 between them without a pair: two components and an isolated camera
Seeds were chosen on the reference, never on the device (seed 0 everywhere: it passed every condition at the first try).

Bounds.  B(scene, options) = max(100 x the largest |R - R'|_F over the cameras between the reference's run and its run with
the directed edge list permuted, 1e-12); the floor: 40 sweeps of about 30 roundings at 1.1e-16 come to 1.3e-13.  R of the
device is Exp of the r it returns, and so is the reference's in that comparison (the rule writes (1e-12, 0, 0) at the identity).  delta[s] is held to B (1 + delta_ref[s]): a step is the difference of two rotations of
order 1, so its absolute error is that of R, and the relative form holds while delta is large against B -- after 40 sweeps
K70 has delta ~ 1e-9, where a purely relative bound of 1e-12 would ask for 1e-21."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import rotavg_ref as ra  # noqa: E402
from refine_util import _model, bits, small_scene  # noqa: E402

DEG = np.pi / 180.0
NOISE = 0.5 * DEG
ROBUST = dict(loops=dict(threshold=3 * DEG), loss="huber", f_scale=1 * DEG)
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
    """(ncams, pairs as listed before the orientation is mixed, gross share)"""
    if name == "band24":
        return 24, band(1, 24, 4), 0.2
    if name == "K12":
        return 12, band(1, 12, 12), 0.2
    if name == "K70":
        return 70, band(1, 70, 70), 0.3
    if name == "hub":
        return 140, sorted(set(band(1, 139, 2)) | {(1, j) for j in range(2, 141)}), 0.0
    if name == "ring24":
        return 24, [(i, i % 24 + 1) for i in range(1, 25)], 0.0
    if name == "two":
        return 21, band(1, 10, 3) + band(12, 10, 3), 0.0
    raise KeyError(name)


def scene(ba, name, seed=0):
    """dict(n, pairs, r, gross, used (None: the default), R_true)"""
    def build():
        n, pairs, frac = graph_of(name)
        rng = np.random.default_rng(seed)
        pairs = np.array(pairs, dtype=np.int64)
        flip = rng.random(len(pairs)) < 0.5
        pairs[flip] = pairs[flip][:, ::-1]
        x = np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 6))], axis=1).ravel()
        r, gross = ba.synthetic.relative_rotations(x, 0, pairs, noise=NOISE, outlier_fraction=frac, seed=seed + 100)
        used = None
        if name == "band24":  # three pairs the caller has ruled out: wrong rotations that must not be read
            extra = np.array([[1, 12], [20, 3], [5, 17]], dtype=np.int64)
            pairs, r = np.concatenate([pairs, extra]), np.concatenate([r, rng.normal(size=(3, 3))])
            gross, used = np.concatenate([gross, np.ones(3, dtype=bool)]), np.concatenate([np.ones(len(flip), dtype=bool), np.zeros(3, dtype=bool)])
        if name == "hub":  # a pair without a rotation: unused by default
            pairs, r, gross = np.concatenate([pairs, [[30, 90]]]), np.concatenate([r, np.full((1, 3), np.nan)]), np.concatenate([gross, [False]])
        return dict(n=n, pairs=pairs, r=r, gross=gross, used=used, R_true=ra.exp_many(x.reshape(n, 9)[:, :3]))
    return cached(("scene", name, seed), build)


def model_of(ba, n):
    """a handle with n cameras: rotation averaging reads the device, the stream and ncams of it"""
    return _model(ba, cached(("problem", n), lambda: ba.synthetic.make_problem(n, 4 * n, 12 * n, seed=1)))


def ref_run(ba, name, edge_seed=None, **kw):
    """the reference on a scene under the keywords of average_rotations (fixed_cameras 1-based)"""
    def build():
        s = scene(ba, name)
        k = dict(kw)
        fixed = np.zeros(s["n"], dtype=bool)
        fixed[np.asarray(k.pop("fixed_cameras", []), dtype=np.int64) - 1] = True
        return ra.average(s["n"], s["pairs"], s["r"], used=s["used"], loops_opt=k.pop("loops", None), fixed=fixed,
                          loss=k.pop("loss", None) or "linear", edge_seed=edge_seed, **k)
    key = ("ref", name, edge_seed, repr(sorted((q, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for q, v in kw.items())))
    return cached(key, build)


def bound(ba, name, **kw):
    a, b = ref_run(ba, name, **kw), ref_run(ba, name, edge_seed=7, **kw)
    live = a["component"] >= 0
    return max(100.0 * np.sqrt(((a["R"] - b["R"]) ** 2).sum(axis=(1, 2)))[live].max(), 1e-12)


def dev_run(ba, name, **kw):
    s = scene(ba, name)
    m = model_of(ba, s["n"])
    try:
        return ba.average_rotations(m, s["pairs"], s["r"], used=s["used"], **kw)
    finally:
        m.close()


def start_of(ba, name, seed=3):
    """an r0 for a scene: the true rotations turned by 2 degrees each"""
    s = scene(ba, name)
    noise = ra.exp_many(np.random.default_rng(seed).normal(size=(s["n"], 3)) * 2 * DEG)
    return np.array([ra.rotation_vector(M) for M in noise @ s["R_true"]])


def recovery(s, o, robust):
    """(gross pairs kept, largest camera error in degrees with the gauge aligned at the root, largest residual of a kept clean
    pair, smallest residual of a gross pair) of a result o (the reference's, or the device's with R = Exp r)"""
    R = o["R"] if "R" in o else ra.exp_many(o["r"])
    root = int(np.flatnonzero(np.asarray(o["status"]) == "root")[0])
    err = ra.camera_errors(R, s["R_true"], root) / DEG
    res = o["residual"] / DEG
    clean = o["kept"] & ~s["gross"]
    return int((o["kept"] & s["gross"]).sum()), err.max(), res[clean].max(), np.nanmin(res[s["gross"]]) if robust else np.nan


def assert_recovered(s, o):
    kept_gross, err, res_clean, res_gross = recovery(s, o, True)
    print(f"gross kept {kept_gross}, error {err:.3f} deg, clean residual <= {res_clean:.3f} deg, gross residual >= {res_gross:.2f} deg")
    assert kept_gross == 0 and err <= 2.0 and res_clean <= 5.0 and res_gross >= 15.0


STOP_SCENES = ("band24", "K70", "hub", "two")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_julia_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    for name in ("ba_rotation_loops", "ba_view_graph_forest", "ba_average_rotations"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header and f"(:{name}, libba)" in julia
    for fn in ("rotation_loops", "view_graph_forest", "average_rotations"):
        assert f"function {fn}(" in julia and fn in ba.__all__ and callable(getattr(ba, fn))
    assert "enum { BA_RA_OK = 0, BA_RA_ROOT = 1, BA_RA_FIXED = 2, BA_RA_ISOLATED = 3, BA_RA_STATES = 4 };" in header
    assert "typedef struct ba_rotavg_opts {" in header and "struct BaRotavgOpts" in julia
    assert lib.ROTAVG_STATES == ("ok", "root", "fixed", "isolated")
    for word in ("R_b = R_k R_a", "listed twice", "min(8, remaining)", "atan2(|w| / 2, (tr M - 1) / 2)", "radians"):
        assert word in header
    names = [f[0] for f in lib.RotavgOpts._fields_]
    body = header[header.index("typedef struct ba_rotavg_opts {"):header.index("} ba_rotavg_opts;")]
    assert [w.split("/*")[0].split()[-1].rstrip(";") for w in body.splitlines()[1:] if ";" in w.split("/*")[0]] == names
    jbody = julia[julia.index("struct BaRotavgOpts"):]
    assert [w.split()[0] for w in jbody[:jbody.index("\nend")].splitlines()[1:] if "::" in w] == names

    def opts(**over):
        return lib.RotavgOpts(**dict(dict(loss=0, max_sweeps=0, loops=0, min_support=0, f_scale=0.0, damping=0.0, xtol=1e-6,
                                          loop_threshold=0.0), **over))
    who, tail = b"ba_average_rotations", (None,) * 12
    # a null handle, null options, each bad option
    assert L.ba_average_rotations(None, 0, None, None, None, None, None, None, None, C.byref(opts()), *tail) == 1
    assert who in L.ba_last_error() and b"null argument" in L.ba_last_error()
    assert L.ba_average_rotations(None, 0, None, None, None, None, None, None, None, None, *tail) == 1 and b"null options" in L.ba_last_error()
    for bad, word in ((dict(loss=5), b"loss"), (dict(loss=-1), b"loss"), (dict(loss=1), b"f_scale"), (dict(loss=1, f_scale=-1.0), b"f_scale"),
                      (dict(loss=3, f_scale=np.nan), b"f_scale"), (dict(damping=1.5), b"damping"), (dict(damping=-0.1), b"damping"),
                      (dict(damping=np.nan), b"damping"), (dict(max_sweeps=100001), b"max_sweeps"), (dict(xtol=np.nan), b"xtol"),
                      (dict(xtol=np.inf), b"xtol"), (dict(loops=1), b"loop_threshold"), (dict(loops=1, loop_threshold=np.inf), b"loop_threshold")):
        assert L.ba_average_rotations(None, 0, None, None, None, None, None, None, None, C.byref(opts(**bad)), *tail) == 1
        msg = L.ba_last_error()
        assert word in msg and who in msg, (bad, msg)
    for good in (opts(loss=1, f_scale=0.1, damping=1.0, max_sweeps=100000, xtol=0.0), opts(loops=1, loop_threshold=0.05, min_support=2)):
        assert L.ba_average_rotations(None, 0, None, None, None, None, None, None, None, C.byref(good), *tail) == 1
        assert b"null argument" in L.ba_last_error()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert L.ba_rotation_loops(None, 0, None, None, None, None, tau, None, None) == 1 and b"threshold" in L.ba_last_error()
    assert L.ba_rotation_loops(None, 0, None, None, None, None, 0.1, None, None) == 1
    assert b"ba_rotation_loops" in L.ba_last_error() and b"null argument" in L.ba_last_error()
    # the host-only entry: its refusals need no handle
    a1, b1 = np.array([1, 2, 2], dtype=np.int64), np.array([2, 3, 1], dtype=np.int64)
    comp, par, order, roots = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    n_order, n_comp = C.c_int64(0), C.c_int64(0)
    outs = (lib.ptr(comp), lib.ptr(par), lib.ptr(order), C.byref(n_order), C.byref(n_comp), lib.ptr(roots))
    assert L.ba_view_graph_forest(3, 3, lib.ptr(a1), lib.ptr(b1), None, None, None, None, *outs) == 1
    assert b"ba_view_graph_forest" in L.ba_last_error() and b"listed twice" in L.ba_last_error()
    for bad_b, word in (([2, 3, 4], b"1..3"), ([2, 2, 1], b"two different cameras")):
        bb = np.array(bad_b, dtype=np.int64)
        assert L.ba_view_graph_forest(3, 3, lib.ptr(a1), lib.ptr(bb), None, None, None, None, *outs) == 1 and word in L.ba_last_error()
    b_ok, w_bad = np.array([2, 3, 3], dtype=np.int64), np.array([1.0, -1.0, 1.0])
    a_ok = np.array([1, 2, 1], dtype=np.int64)
    assert L.ba_view_graph_forest(3, 3, lib.ptr(a_ok), lib.ptr(b_ok), None, None, lib.ptr(w_bad), None, *outs) == 1 and b"weight" in L.ba_last_error()
    assert L.ba_view_graph_forest(3, 3, lib.ptr(a_ok), lib.ptr(b_ok), None, None, None, None, None, None, None, None, None, None) == 1
    assert b"null argument" in L.ba_last_error()
    assert L.ba_view_graph_forest(3, 3, lib.ptr(a_ok), lib.ptr(b_ok), None, None, None, None, *outs) == 0 and n_comp.value == 1
    # Python: ValueError before any device call (None stands in for the model)
    assert ba.average_rotations.__kwdefaults__ == dict(weights=None, used=None, loops=None, r0=None, fixed_cameras=None, loss=None,
                                                       f_scale=None, damping=None, max_sweeps=None, xtol=None)
    assert ba.rotation_loops.__kwdefaults__ == dict(used=None) and "threshold" in ba.rotation_loops.__code__.co_varnames
    pairs, r = [[1, 2], [2, 3]], np.zeros((2, 3))
    for bad in (dict(loss="huber"), dict(loss="tukey"), dict(loss="cauchy", f_scale=0.0), dict(loss="huber", f_scale=float("nan")),
                dict(damping=0.0), dict(damping=1.2), dict(damping="a"), dict(max_sweeps=0), dict(max_sweeps=100001), dict(max_sweeps=2.5),
                dict(xtol=float("nan")), dict(xtol="a"), dict(loops=dict()), dict(loops=dict(threshold=0.0)), dict(loops=dict(threshold=0.1, tau=1)),
                dict(loops=dict(threshold=0.1, min_support=0)), dict(loops=0.1), dict(weights=[1.0, -1.0]), dict(weights=[1.0]),
                dict(weights=[1.0, float("inf")]), dict(used=[1, 0]), dict(used=[True]), dict(fixed_cameras=[1]), dict(fixed_cameras=[0], r0=np.zeros((3, 3))),
                dict(r0=np.zeros((3, 2))), dict(r0=np.array([[0.0, 0, 0], [np.nan, 0, 0], [0, 0, 0]])), dict(r0=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            ba.average_rotations(None, pairs, r, **bad)
    for bad_pairs in ([[1, 2], [2, 1]], [[1, 2], [1, 2]], [[1, 1]], [[0, 1]], [1, 2], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            ba.average_rotations(None, bad_pairs, np.zeros((len(bad_pairs), 3)))
        with pytest.raises(ValueError):
            ba.rotation_loops(None, bad_pairs, np.zeros((len(bad_pairs), 3)), threshold=0.1)
        with pytest.raises(ValueError):
            ba.view_graph_forest(3, bad_pairs)
    with pytest.raises(ValueError, match="r must have shape"):
        ba.average_rotations(None, pairs, np.zeros((3, 3)))
    for tau in (0.0, float("nan"), "a", None):
        with pytest.raises(ValueError, match="threshold"):
            ba.rotation_loops(None, pairs, r, threshold=tau)
    for bad in (dict(ncams=2), dict(ncams=-1), dict(ncams=3, support=[1.0, 2.0]), dict(ncams=3, support=[1]), dict(ncams=3, fixed_cameras=[4]),
                dict(ncams=3, used=[True])):
        with pytest.raises(ValueError):
            ba.view_graph_forest(bad.pop("ncams"), pairs, **bad)

    class Sizes:
        ncams = 2
    with pytest.raises(ValueError, match="1..2"):
        ba.average_rotations(Sizes, pairs, r)
    with pytest.raises(ValueError, match="1..2"):
        ba.rotation_loops(Sizes, pairs, r, threshold=0.1)


def assert_forest(ba, n, pairs, **kw):
    got = ba.view_graph_forest(n, pairs, **kw)
    fixed = np.zeros(n, dtype=bool)
    fixed[np.asarray(kw.get("fixed_cameras", []), dtype=np.int64) - 1] = True
    want = ra.forest(n, pairs, used=kw.get("used"), support=kw.get("support"), weights=kw.get("weights"), fixed=fixed)
    for key in ("component", "parent_pair", "roots", "order"):
        assert np.array_equal(got[key], want[key]), key
    assert got["n_components"] == want["n_components"]
    return got


@pytest.mark.parametrize("name", ["band24", "K12", "K70", "hub", "ring24", "two"])
def test_forest_against_reference(ba, name):
    s = scene(ba, name)
    rng = np.random.default_rng(5)
    n = len(s["pairs"])
    used = np.isfinite(s["r"]).all(axis=1) if s["used"] is None else s["used"]
    assert_forest(ba, s["n"], s["pairs"], used=used)
    assert_forest(ba, s["n"], s["pairs"], used=used, weights=rng.integers(1, 5, n).astype(np.float64))  # tied weights
    got = assert_forest(ba, s["n"], s["pairs"], used=used, support=rng.integers(0, 3, n).astype(np.int32), weights=rng.random(n),
                        fixed_cameras=[3, s["n"] - 2])
    assert 3 in got["roots"]
    if name == "two":
        assert got["n_components"] == 2 and got["component"][10] == -1 and got["parent_pair"][10] == -1 and list(got["roots"]) == [3, 19]
        assert len(got["order"]) == 20 and 11 not in got["order"]


def test_forest_on_tied_keys_and_fixed_cameras(ba):
    """every key equal: the pair index decides; the root: the lowest fixed camera, else the largest weight sum, ties to the lowest"""
    pairs = np.array([[2, 1], [3, 2], [1, 3], [4, 3], [4, 1], [6, 5]], dtype=np.int64)
    got = assert_forest(ba, 7, pairs)
    assert list(got["parent_pair"]) == [-1, 0, 1, 3, -1, 5, -1] and list(got["roots"]) == [1, 5] and list(got["order"]) == [1, 2, 3, 4, 5, 6]
    assert list(got["component"]) == [0, 0, 0, 0, 1, 1, -1]
    got = assert_forest(ba, 7, pairs, weights=np.array([1.0, 1.0, 1.0, 5.0, 1.0, 1.0]))
    assert list(got["roots"]) == [3, 5] and got["parent_pair"][3] == 3
    got = assert_forest(ba, 7, pairs, fixed_cameras=[4, 2, 6], support=np.array([0, 0, 0, 0, 2, 0], dtype=np.int32))
    assert list(got["roots"]) == [2, 6] and list(got["order"]) == [2, 1, 3, 4, 6, 5]
    assert_forest(ba, 7, pairs, used=np.array([1, 0, 1, 0, 0, 1], dtype=bool))
    empty = ba.view_graph_forest(4, np.zeros((0, 2), dtype=np.int64))
    assert empty["n_components"] == 0 and list(empty["component"]) == [-1] * 4 and len(empty["order"]) == 0


def test_reference_conditions(ba):
    """The conditions of the GPU tests, on the reference alone"""
    for name in ("band24", "K12"):
        s = scene(ba, name)
        assert_recovered(s, ref_run(ba, name, **ROBUST))
    s = scene(ba, "band24")
    plain = recovery(s, ref_run(ba, "band24"), False)
    print("band24, every pair and the linear loss:", plain)
    assert plain[1] > 20.0
    assert ref_run(ba, "ring24")["sweeps"] < 1000
    full = ref_run(ba, "ring24", damping=1.0)
    assert full["sweeps"] == 1000 and full["delta"].min() > 1e-6
    for name in ("band24", "K12", "K70", "hub"):
        s = scene(ba, name)
        ang = ra.loops(s["n"], s["pairs"], s["r"], 3 * DEG, used=s["used"])[2]
        assert ang.size and np.abs(ang / (3 * DEG) - 1.0).min() > 1e-6
    for name in STOP_SCENES:
        for kw in (ROBUST, {}):
            d = ref_run(ba, name, **kw)["delta"]
            assert len(d) % 8 == 0 and len(d) < 1000
            per_batch = d.reshape(-1, 8).min(axis=1)
            assert np.abs(per_batch / 1e-6 - 1.0).min() > 0.01 and (per_batch[:-1] > 1e-6).all() and per_batch[-1] <= 1e-6


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["band24", "K12", "K70", "hub"])
def test_loop_counts(ba, gpu_ok, name):
    s = scene(ba, name)
    m = model_of(ba, s["n"])
    try:
        n_loops, support = ba.rotation_loops(m, s["pairs"], s["r"], threshold=3 * DEG, used=s["used"])
        everything = ba.rotation_loops(m, s["pairs"], s["r"], threshold=np.pi, used=s["used"])
    finally:
        m.close()
    want = ra.loops(s["n"], s["pairs"], s["r"], 3 * DEG, used=s["used"])
    assert np.array_equal(n_loops, want[0]) and np.array_equal(support, want[1])
    assert np.array_equal(everything[0], want[0]) and np.array_equal(everything[1], want[0])
    assert n_loops.max() == {"band24": 6, "K12": 10, "K70": 68, "hub": 4}[name]  # (K70: lists longer than a wave)
    unused = ~np.isfinite(s["r"]).all(axis=1) if s["used"] is None else ~s["used"]
    assert unused.any() == (name in ("band24", "hub")) and not n_loops[unused].any() and not support[unused].any()


@pytest.mark.gpu
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("loss", ["linear", "huber"])
@pytest.mark.parametrize("name", ["band24", "K70", "hub"])
def test_fixed_sweeps(ba, gpu_ok, name, loss, held):
    kw = dict(xtol=0.0, max_sweeps=40)
    if loss == "huber":
        kw.update(ROBUST)
    if held:
        kw.update(r0=start_of(ba, name), fixed_cameras=[2, scene(ba, name)["n"] - 1])
    want, B = ref_run(ba, name, **kw), bound(ba, name, **kw)
    got = dev_run(ba, name, **kw)
    assert got["sweeps"] == 40 and len(got["delta"]) == 40 and np.array_equal(got["kept"], want["kept"])
    R = ra.exp_many(got["r"])
    dist = np.sqrt(((R - ra.exp_many(want["r"])) ** 2).sum(axis=(1, 2)))  # (both through the rotation-vector rule: (1e-12, 0, 0) at I)
    d_err = np.abs(got["delta"] - want["delta"]) / (1.0 + want["delta"])
    print(f"{name} {loss} held={held}: B = {B:.2e}, |R - R_ref| <= {dist.max():.2e}, delta within {d_err.max():.2e}, delta[39] = {want['delta'][-1]:.2e}")
    assert dist.max() <= B and d_err.max() <= B
    assert np.abs(np.transpose(R, (0, 2, 1)) @ R - np.eye(3)).max() <= 1e-12
    if held:
        assert list(got["status"][[1, -2]]) == ["fixed", "fixed"]
        assert np.abs(R[[1, -2]] - ra.exp_many(kw["r0"][[1, -2]])).max() <= 1e-12  # (held at r0)
        assert "root" not in got["status"]


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("name", STOP_SCENES)
def test_stop_rule(ba, gpu_ok, name, robust):
    kw = dict(ROBUST) if robust else {}
    want, B = ref_run(ba, name, **kw), bound(ba, name, **kw)
    got = dev_run(ba, name, **kw)
    print(f"{name} robust={robust}: {got['sweeps']} sweeps (reference {want['sweeps']}), B = {B:.2e}, cost {got['cost_before']:.6e} -> {got['cost_after']:.6e}")
    assert got["sweeps"] == want["sweeps"] and len(got["delta"]) == got["sweeps"]
    assert (got["status"] == want["status"]).all() and np.array_equal(got["component"], want["component"])
    assert np.array_equal(got["kept"], want["kept"]) and got["counts"] == want["counts"]
    if robust:
        assert np.array_equal(got["n_loops"], want["n_loops"]) and np.array_equal(got["support"], want["support"])
    else:
        assert "n_loops" not in got
    assert np.array_equal(np.isnan(got["residual"]), np.isnan(want["residual"]))
    live = ~np.isnan(want["residual"])
    assert np.abs(got["residual"] - want["residual"])[live].max() <= B
    assert np.abs(got["edge_weight"] - want["edge_weight"]).max() <= B / (1 * DEG)  # (rho' of huber: 1 / (theta / c), theta within B)
    for key in ("cost_before", "cost_after"):
        assert abs(got[key] - want[key]) <= B * (1.0 + want[key])
    assert got["cost_after"] <= got["cost_before"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["band24", "K12"])
def test_recovery(ba, gpu_ok, name):
    """The robust call recovers every camera; the call on every pair under the linear loss does not"""
    s = scene(ba, name)
    assert_recovered(s, dev_run(ba, name, **ROBUST))
    if name == "band24":
        plain = recovery(s, dev_run(ba, name), False)
        print("every pair and the linear loss:", plain)
        assert plain[1] > 20.0


@pytest.mark.gpu
def test_gauge_and_components(ba, gpu_ok):
    s = scene(ba, "two")
    m = model_of(ba, s["n"])
    try:
        kw = dict(xtol=0.0, max_sweeps=24, loss="huber", f_scale=1 * DEG)
        a = ba.average_rotations(m, s["pairs"], s["r"], **kw)
        roots = np.flatnonzero(a["status"] == "root")
        assert len(roots) == 2 and a["counts"] == dict(ok=18, root=2, fixed=0, isolated=1)
        assert np.abs(a["r"][roots] - [1e-12, 0.0, 0.0]).max() <= 1e-12  # the roots are back at their start: the rule's identity
        assert np.isnan(a["r"][10]).all() and a["status"][10] == "isolated" and a["component"][10] == -1
        assert np.isfinite(np.delete(a["r"], 10, axis=0)).all()
        # other rotations, and one pair fewer, in the second component: the first keeps its bits
        second = (s["pairs"] >= 12).all(axis=1)
        r2 = np.where(second[:, None], s["r"][::-1], s["r"])
        used = np.ones(len(second), dtype=bool)
        used[np.flatnonzero(second)[4]] = False
        b = ba.average_rotations(m, s["pairs"], r2, used=used, **kw)
        assert same(a["r"][:10], b["r"][:10]) and not same(a["r"][11:], b["r"][11:])
        assert same(a["residual"][~second], b["residual"][~second])
        # a pair across the two components is NaN while it is not used, and is measured once it joins them
        pairs3, r3 = np.concatenate([s["pairs"], [[4, 15]]]), np.concatenate([s["r"], [[np.nan] * 3]])
        c = ba.average_rotations(m, pairs3, r3, **kw)
        assert np.isnan(c["residual"][-1]) and not c["kept"][-1] and same(c["r"], a["r"])
        # a start of its own: the roots return to it; the converged result as a start returns after the first batch
        r0 = start_of(ba, "two")
        d = ba.average_rotations(m, s["pairs"], s["r"], r0=r0, **ROBUST)
        roots = np.flatnonzero(d["status"] == "root")
        assert np.abs(ra.exp_many(d["r"][roots]) - ra.exp_many(r0[roots])).max() <= 1e-12 and d["sweeps"] > 8
        again = ba.average_rotations(m, s["pairs"], s["r"], r0=np.where(np.isnan(d["r"]), 0.0, d["r"]), **ROBUST)
        assert again["sweeps"] == 8 and again["delta"].min() <= 1e-6
        assert np.abs(ra.exp_many(again["r"][again["component"] >= 0]) - ra.exp_many(d["r"][d["component"] >= 0])).max() <= 1e-5
    finally:
        m.close()


@pytest.mark.gpu
def test_determinism(ba, gpu_ok):
    """two calls give the same bits; a call between two LM solves on one handle leaves the second solve with the first's bits"""
    s = scene(ba, "K70")
    m = model_of(ba, s["n"])
    try:
        a = ba.average_rotations(m, s["pairs"], s["r"], **ROBUST)
        b = ba.average_rotations(m, s["pairs"], s["r"], **ROBUST)
        la, lb = (ba.rotation_loops(m, s["pairs"], s["r"], threshold=3 * DEG) for _ in range(2))
    finally:
        m.close()
    for key in ("r", "residual", "edge_weight", "delta", "cost_before", "cost_after"):
        assert same(a[key], b[key]), key
    assert a["sweeps"] == b["sweeps"] and np.array_equal(a["kept"], b["kept"]) and np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
    q, k12 = small_scene(ba), scene(ba, "K12")
    ms = _model(ba, q)
    try:
        solve = lambda: ba.Levenberg_Marquardt(ba.FeasibilityResidual(ms), "LDL", "AMD", "None", False, x=q["x0"], ite_max=4)  # noqa: E731
        first = solve()
        between = ba.average_rotations(ms, k12["pairs"], k12["r"], **ROBUST)
        second = solve()
    finally:
        ms.close()
    assert same(first.solution, second.solution) and same(first.objective, second.objective) and first.iter == second.iter
    assert same(between["r"], dev_run(ba, "K12", **ROBUST)["r"])
