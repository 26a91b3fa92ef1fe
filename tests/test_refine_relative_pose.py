"""Non-linear refinement of the relative pose on its consensus set (ba_refine_relative_pose, include/ba_hip.h; DESIGN §5q;
refine_relative_pose and the refine= keyword of relative_pose* of the package).  The reference is
tests/helpers/pair_refine_ref.py: the header restated in numpy.  The first tests need no device; the rest run on the GPU.

Scenes: those of tests/test_five_point.py (its forms noisy005 and noisy05: the seven pairs with 63..600 matches, 30 % of the
detections displaced, tau = 2 px) refined from the result of the five-point reference with that form's options, so device and
reference start from the same pose and set; and the exact scene of test_relative_pose.pair_scene for its ten counts 7 .. 600 with
every detection re-projected and none displaced -- the set of "every used match" holds no wrong match there, which the condition
"the refined pose reaches the true one" needs -- started from the true pose moved by delta = (1e-2, ...) in all five parameters.

Bounds, all from the reference: a pose -- |R - R_ref|_F + |t - t_ref| within 100 x the reference's own spread between its run and
a run with every pair's match order permuted, the spread taken as the largest over the pairs of the call (where the iteration
stops moves with the rounding of the sums, by 1e-16 on most pairs and by 1e-9 on some, and which pairs those are changes with
the summation order: the largest is the honest figure for every pair), floor 100 x the largest |g| / |H| the reference leaves at
its results.  cost_after -- relative to the reference's within 100 x its relative spread under that permutation, floor 100 x the
rounding of the sum itself: sum over the set of |e| eps_e + eps_e^2 / 2 with eps_e = 16 eps |d_b|' |E| |d_a| / sqrt(D), the
rounding of e through the sixteen operations of n = d_b' E d_a (on the exact scene the cost is that rounding and nothing else).
Measured figures are in DESIGN §5q."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_ref as br  # noqa: E402
import pair_ref as pf  # noqa: E402
import pair_refine_ref as prr  # noqa: E402
import resect_ref as rr  # noqa: E402
import test_five_point as tfp  # noqa: E402
import test_relative_pose as trp  # noqa: E402
from refine_util import _model, bits, small_scene  # noqa: E402
from test_relative_pose import COUNTS, pair_scene  # noqa: E402
from test_five_point import form, reference  # noqa: E402

cached = trp.cached
TAU = 2.0
START = np.full(5, 1e-2)
NEAR = 1e-4           # a match within NEAR tau of tau under the reference's pose: its byte may differ
NEED_ROUNDS = 6       # of 7 pairs comparable through the rounds (the reference has all 7)
ORDER_SEED = 11


# ---- scenes, starts and the reference's runs ----------------------------------------------------------------------------------
def exact_scene(ba):
    def build():
        p = pair_scene(ba, COUNTS, trp.SCENE_SEED)
        return p, trp.intrinsics_only(p), trp.pairs_of(p)
    return cached(("refine_exact",), build)


def start(ba, kind):
    """(p, x, pairs, start): start holds r, t, status (codes), inlier (per match, None: every used match), match_ptr"""
    def build():
        if kind == "exact":
            p, x, pairs = exact_scene(ba)
            n = len(pairs)
            r, t = np.zeros((n, 3)), np.zeros((n, 3))
            for k in range(n):
                R, tt, _ = pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)
                R2, t[k] = prr.retract(R, tt, START)
                r[k] = rr.rotation_vector(R2)
            ptr = pf.matches(p, pairs)[0]
            return p, x, pairs, dict(r=r, t=t, status=np.zeros(n, dtype=np.uint8), inlier=None, match_ptr=ptr)
        p, x, pairs = form(ba, kind)
        con = reference(ba, kind)
        return p, x, pairs, dict(r=con["r"], t=con["t"], status=con["status"], inlier=con["inlier"], match_ptr=con["match_ptr"])
    return cached(("refine_start", kind), build)


def orders(ptr):
    rng = np.random.default_rng(ORDER_SEED)
    return [rng.permutation(int(ptr[k + 1] - ptr[k])) for k in range(len(ptr) - 1)]


def ref_run(ba, kind, every=False, **kw):
    """(the reference's run, its run with every pair's match order permuted); every: the set is every used match"""
    def build():
        p, x, pairs, s = start(ba, kind)
        args = dict(dict(status=s["status"], inlier=None if every else s["inlier"], threshold=TAU), **kw)
        return (prr.refine(p, x, pairs, s["r"], s["t"], **args), prr.refine(p, x, pairs, s["r"], s["t"], order=orders(s["match_ptr"]), **args))
    return cached(("refine_ref", kind, every, tuple(sorted(kw.items()))), build)


def cost_rounding(p, x, pairs, out):
    """per pair the rounding of cost_after as a sum: the module's header"""
    _, _, _, data = pf.rays(p, x, pairs)
    ptr, eps = out["match_ptr"], np.finfo(float).eps
    res = np.zeros(len(pairs))
    for k, (qa, qb, used, fa, fb) in enumerate(data):
        M = out["inlier"][ptr[k]:ptr[k + 1]] & used
        E = pf.essential(br.rotations(out["r"][k][None])[0], out["t"][k])
        with np.errstate(all="ignore"):
            n, D, _, _ = prr.parts(E, qa[M], qb[M], fa, fb)
            ee = 16 * eps * (np.abs(prr.rays3(qb[M])) @ np.abs(E) * np.abs(prr.rays3(qa[M]))).sum(1) / np.sqrt(D)
            res[k] = (np.abs(n / np.sqrt(D)) * ee + 0.5 * ee * ee).sum()
    return res


def bounds(p, x, pairs, a, b):
    """(pose bound of the call, relative cost bound per pair, the spread, the floor) from the reference's two runs"""
    run = a["state"] != prr.SKIPPED
    spread = float(pf.pose_error(a["r"][run], a["t"][run], b["r"][run], b["t"][run]).max())
    floor = 100 * float(a["grad"][run].max())
    with np.errstate(all="ignore"):
        rel = np.abs(a["cost"][:, 1] - b["cost"][:, 1]) / a["cost"][:, 1]
        cost = np.maximum(100 * np.where(np.isfinite(rel), rel, 0.0).max(), 100 * cost_rounding(p, x, pairs, a) / a["cost"][:, 1])
    return max(100 * spread, floor), cost, spread, floor


def dev_info(ba, s):
    names = np.array(ba._lib.PAIR_STATES)[s["status"]]
    ptr = s["match_ptr"]
    inl = np.ones(ptr[-1], dtype=bool) if s["inlier"] is None else s["inlier"]
    return dict(r=s["r"].copy(), t=s["t"].copy(), status=names, inliers=inl.copy(), match_ptr=ptr,
                n_inliers=np.array([inl[ptr[k]:ptr[k + 1]].sum() for k in range(len(ptr) - 1)], dtype=np.int32))


def run(ba, p, x, pairs, info, **kw):
    m = _model(ba, p)
    try:
        return ba.refine_relative_pose(m, x, pairs, info, **kw)
    finally:
        m.close()


def compare(ba, what, p, x, pairs, out, a, b, sets=True):
    """the device's dict against the reference's run a (b: its permuted run): states, pose, cost_after, and on the pairs where no
    match is near tau under the reference's pose, the sets and n_consistent"""
    bound, cbound, spread, floor = bounds(p, x, pairs, a, b)
    ptr = a["match_ptr"]
    assert list(out["refine_status"]) == [prr.STATES[s] for s in a["state"]]
    ran = np.flatnonzero(a["state"] != prr.SKIPPED)
    err = pf.pose_error(out["r"][ran], out["t"][ran], a["r"][ran], a["t"][ran])
    with np.errstate(all="ignore"):
        crel = np.abs(out["cost_after"] - a["cost"][:, 1])[ran] / a["cost"][ran, 1]
    print(f"{what}: reference spread {spread:.2e}, floor {floor:.1e}, pose bound {bound:.1e}, device distance {err.max():.2e}; cost_after "
          f"relative {np.nanmax(crel):.2e} (bounds {cbound[ran].min():.1e} .. {cbound[ran].max():.1e}); trials device {list(out['iters'])}, "
          f"reference {list(a['iters'])}")
    assert (err <= bound).all(), (err, bound)
    assert (crel <= cbound[ran]).all(), (crel, cbound[ran])
    assert np.abs(np.linalg.norm(out["t"][ran], axis=1) - 1.0).max() <= 1e-14
    assert (out["cost_after"][ran] <= out["cost_before"][ran]).all()
    clear = ran[a["margin"][ran] >= NEAR]
    if sets:
        for k in clear:
            assert out["n_consistent"][k] == a["n_consistent"][k] and out["n_inliers"][k] == a["n_inliers"][k], k
            assert np.array_equal(out["inliers"][ptr[k]:ptr[k + 1]], a["inlier"][ptr[k]:ptr[k + 1]]), k
    return clear


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_julia_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    name = "ba_refine_relative_pose"
    assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header and f"(:{name}, libba)" in julia
    assert "function refine_relative_pose(" in julia
    assert ("enum { BA_RR_CONVERGED = 0, BA_RR_STALLED = 1, BA_RR_MAX_ITER = 2, BA_RR_NONFINITE = 3, BA_RR_SKIPPED = 4, BA_RR_STATES = 5 };"
            in header)
    assert lib.PAIR_REFINE_STATES == ("converged", "stalled", "max_iter", "nonfinite", "skipped") == prr.STATES
    for word in ("typedef struct ba_pair_refine_opts", "[t]x [e_j]x R", "[b_j]x R", "ties to the lowest", "n_consistent", "communicator"):
        assert word in header
    assert "a non-linear refinement of the pair" not in header
    good = dict(max_iter=-1, xtol=0.0, lambda0=0.0, loss=0, f_scale=1.0, threshold=1.0, rounds=-1)
    tail = (None,) * 9
    who = name.encode()
    assert L.ba_refine_relative_pose(None, None, 0, None, None, C.byref(lib.PairRefineOpts(**good)), *tail) == 1
    assert who in L.ba_last_error() and b"null argument" in L.ba_last_error()
    assert L.ba_refine_relative_pose(None, None, 0, None, None, None, *tail) == 1
    assert who in L.ba_last_error() and b"null options" in L.ba_last_error()
    for bad, word in ((dict(xtol=np.nan), b"xtol"), (dict(xtol=np.inf), b"xtol"), (dict(lambda0=np.nan), b"lambda0"), (dict(lambda0=-np.inf), b"lambda0"),
                      (dict(threshold=np.nan), b"threshold"), (dict(threshold=np.inf), b"threshold"), (dict(threshold=0.0), b"threshold"),
                      (dict(threshold=-1.0), b"threshold"), (dict(rounds=9), b"rounds"), (dict(loss=5), b"loss"), (dict(loss=-1), b"loss"),
                      (dict(f_scale=0.0), b"f_scale"), (dict(f_scale=np.nan), b"f_scale")):
        o = lib.PairRefineOpts(**dict(good, **bad))
        assert L.ba_refine_relative_pose(None, None, 0, None, None, C.byref(o), *tail) == 1
        msg = L.ba_last_error()
        assert word in msg and who in msg, (bad, msg)
    # good options at their limits reach the argument check
    o = lib.PairRefineOpts(**dict(good, rounds=8, max_iter=0, loss=4, xtol=-1.0, lambda0=-1.0))
    assert L.ba_refine_relative_pose(None, None, 0, None, None, C.byref(o), *tail) == 1 and b"null argument" in L.ba_last_error()
    assert ba.refine_relative_pose.__kwdefaults__ == dict(max_iter=None, xtol=None, lam0=None, loss=None, f_scale=1.0, rounds=None, obs_info=None)
    # Python: ValueError before any device call (None stands in for the model)
    x = np.zeros(3)
    info = dict(r=np.zeros((1, 3)), t=np.zeros((1, 3)), status=np.array(["ok"]), inliers=np.zeros(0, dtype=bool))
    for bad in (dict(threshold=np.nan), dict(threshold=0.0), dict(threshold="a"), dict(threshold=1.0, xtol=np.nan), dict(threshold=1.0, lam0=np.inf),
                dict(threshold=1.0, rounds=9), dict(threshold=1.0, rounds=1.5), dict(threshold=1.0, loss="l2"), dict(threshold=1.0, f_scale=0.0),
                dict(threshold=1.0, max_iter=2.5)):
        with pytest.raises(ValueError):
            ba.refine_relative_pose(None, x, [[1, 2]], info, **bad)
    with pytest.raises(TypeError):
        ba.refine_relative_pose(None, x, [[1, 2]], info)  # (threshold is required)
    for bad in (4.0, dict(threshold=1.0, tau=2.0), dict(threshold=-1.0), dict(rounds=9), dict()):
        with pytest.raises(ValueError):
            ba.relative_pose(None, x, [[1, 2]], refine=bad)
    with pytest.raises(ValueError):
        ba.relative_pose_five_point(None, x, [[1, 2]], ransac=dict(threshold=1.0), refine=dict(rounds=9))
    with pytest.raises(TypeError):
        ba.relative_pose(None, x, [[1, 2]], refit=dict())
    o = lib.pair_refine_opts(threshold=2.5)
    assert (o.max_iter, o.xtol, o.lambda0, o.loss, o.f_scale, o.threshold, o.rounds) == (-1, 0.0, 0.0, 0, 1.0, 2.5, -1)
    assert lib.pair_refine_opts(threshold=1.0, loss="cauchy", f_scale=3.0, rounds=8).loss == lib.LOSSES["cauchy"]
    # an inlier array of the wrong length, an info without its keys, a status that is no state
    p = small_scene(ba)

    class Sizes:
        ncams, npnts, nobs = p["ncams"], p["npnts"], p["nobs"]
        cams_indices, pnts_indices = np.asarray(p["cam_idx1"], dtype=np.int64), np.asarray(p["pnt_idx1"], dtype=np.int64)

        class meta:
            nvar = 3 * p["npnts"] + 9 * p["ncams"]
    xs = np.zeros(Sizes.meta.nvar)
    n_match = int(ba.pair_matches(p, [[1, 2]])[0][-1])
    ok = dict(r=np.zeros((1, 3)), t=np.zeros((1, 3)), status=np.array(["ok"]), inliers=np.ones(n_match, dtype=bool))
    for bad, word in ((dict(ok, inliers=np.ones(n_match + 1, dtype=bool)), "inliers"), (dict(ok, r=np.zeros((2, 3))), "r and t"),
                      (dict(ok, status=np.array(["fine"])), "status"), ({k: v for k, v in ok.items() if k != "t"}, "info")):
        with pytest.raises(ValueError, match=word):
            ba.refine_relative_pose(Sizes, xs, [[1, 2]], bad, threshold=1.0)
    with pytest.raises(ValueError, match="pair"):
        ba.refine_relative_pose(Sizes, xs, [[1, 1]], ok, threshold=1.0)


def test_reference_jacobian():
    """the reference's analytic Jacobian against central differences of its own residual through its own retraction: every column,
    linear and Cauchy (the gradient of F), on random poses and matches and on a t with two equal smallest components (the basis
    takes the lower index)"""
    rng = np.random.default_rng(4)
    cases = [(rng.normal(size=3) * 0.4, rng.normal(size=3)) for _ in range(6)]
    cases += [(rng.normal(size=3) * 0.4, np.array([0.5, 0.5, np.sqrt(0.5)])), (rng.normal(size=3), np.array([-0.6, 0.6, np.sqrt(0.28)])),
              (rng.normal(size=3), np.array([0.0, 0.0, 1.0]))]
    assert np.allclose(prr.basis(np.array([0.5, 0.5, np.sqrt(0.5)]))[:, 0], np.cross([1, 0, 0], [0.5, 0.5, np.sqrt(0.5)]) / np.sqrt(0.75))
    assert np.array_equal(prr.basis(np.array([0.0, 0.0, 1.0]))[:, 0], [0.0, -1.0, 0.0])
    worst = worst_g = 0.0
    for r, t in cases:
        t = t / np.linalg.norm(t)
        R = br.rotations(r[None])[0]
        B = prr.basis(t)
        assert np.abs(B.T @ B - np.eye(2)).max() <= 1e-15 and np.abs(B.T @ t).max() <= 1e-15
        qa, qb = rng.normal(size=(40, 2)) * 0.2, rng.normal(size=(40, 2)) * 0.2
        fa, fb = rng.uniform(400, 1800, 2)
        e, J = prr.jacobian(R, t, qa, qb, fa, fb)
        Jn = prr.numeric_jacobian(R, t, qa, qb, fa, fb)
        scale = np.abs(J).max(axis=0)
        assert (scale > 0).all()
        worst = max(worst, (np.abs(J - Jn).max(axis=0) / scale).max())
        assert np.array_equal(e, prr.residual(R, t, qa, qb, fa, fb)) and np.allclose(e * e, pf.sampson(R, t, qa, qb, fa, fb), rtol=1e-12)
        for loss in ("linear", "cauchy"):
            _, g, _ = prr.normal_sums(R, t, qa, qb, fa, fb, loss, 1.0)
            gn = np.zeros(5)
            for j in range(5):
                d = np.zeros(5)
                d[j] = 1e-6
                gn[j] = (prr.cost(*prr.retract(R, t, d), qa, qb, fa, fb, loss, 1.0) - prr.cost(*prr.retract(R, t, -d), qa, qb, fa, fb, loss, 1.0)) / 2e-6
            worst_g = max(worst_g, np.abs(g - gn).max() / np.abs(g).max())
    print(f"Jacobian against central differences: worst column-relative difference {worst:.2e}, gradient of F {worst_g:.2e}")
    assert worst <= 1e-7 and worst_g <= 1e-6  # (central differences with h = 1e-6: h^2 and eps / h are both about 1e-10 .. 1e-9)


def test_reference_conditions(ba):
    """What the device comparison rests on, pinned on the reference alone, with the analytic Jacobian, rounds = 0, linear loss and
    the defaults: on noisy005 and noisy05 from the five-point reference's result all 7 pairs reach CONVERGED within 20 trials (4 to
    8 of them descend; the rest is the tail in which a step below the rounding of F is tried again, unchanged while lambda << 1,
    until lambda has shrunk it to nothing -- its length moves with the rounding, 18 in the central-difference prototype);
    at 0.5 px cost_after <= 0.25 cost_before on every pair (worst 0.208), the translation-direction error against the generator
    falls on all 7, every pair keeps its whole set (n_consistent >= |M|) where the unrefined pose keeps <= 3 of |M| on six pairs.
    Rounds: at 0.5 px all 7 pairs are comparable (no used match within 1e-4 tau of tau under any round's pose); NEED_ROUNDS is 6.
    Robust loss: on every used match of noisy05 (30 % wrong) from the same poses, Cauchy with c = 1 ends within 1 degree of the
    true direction on all 7 pairs and the linear loss ends farther on all 7."""
    for kind in ("noisy005", "noisy05"):
        p, x, pairs, s = start(ba, kind)
        a, _ = ref_run(ba, kind, rounds=0)
        ratio = a["cost"][:, 1] / a["cost"][:, 0]
        before = np.array([prr.angles(p, p["x_true"], k, s["r"][k], s["t"][k]) for k in range(7)])
        after = np.array([prr.angles(p, p["x_true"], k, a["r"][k], a["t"][k]) for k in range(7)])
        print(f"{kind}: states {a['state']}, trials {a['iters']}, cost ratio {np.round(ratio, 4)}, n_inliers {a['n_inliers']}, n_consistent "
              f"{a['n_consistent']}, rotation error {np.round(before[:, 0], 3)} -> {np.round(after[:, 0], 3)}, direction error "
              f"{np.round(before[:, 1], 3)} -> {np.round(after[:, 1], 3)}, margin {a['margin']}")
        assert (s["status"] == pf.OK).all() and (a["state"] == prr.CONVERGED).all() and a["iters"].max() <= 20
        assert (ratio < 1).all()
        if kind == "noisy05":
            _, _, _, data = pf.rays(p, x, pairs)
            kept = np.array([pf.inliers(s["r"][k], s["t"][k], *data[k], TAU)[s["inlier"][s["match_ptr"][k]:s["match_ptr"][k + 1]]].sum() for k in range(7)])
            print(f"  the unrefined pose keeps {kept} of {a['n_inliers']}")
            assert ratio.max() <= 0.25 and (after[:, 1] < before[:, 1]).all()
            assert (a["n_consistent"] >= a["n_inliers"]).all() and (kept <= 3).sum() >= 6
            assert list(a["n_consistent"]) == [44, 45, 46, 178, 180, 181, 422]
    for rounds in (2, 8):
        a, b = ref_run(ba, "noisy05", rounds=rounds)
        print(f"rounds = {rounds}: adopted {a['adopted']}, n_inliers {a['n_inliers']}, n_consistent {a['n_consistent']}, margin {a['margin']}")
        assert (a["margin"] >= NEAR).sum() >= NEED_ROUNDS and np.array_equal(a["inlier"], b["inlier"]) and a["adopted"].max() >= 1
    p = start(ba, "noisy05")[0]
    c, _ = ref_run(ba, "noisy05", every=True, rounds=0, loss="cauchy", f_scale=1.0)
    l, _ = ref_run(ba, "noisy05", every=True, rounds=0)
    tc = np.array([prr.angles(p, p["x_true"], k, c["r"][k], c["t"][k])[1] for k in range(7)])
    tl = np.array([prr.angles(p, p["x_true"], k, l["r"][k], l["t"][k])[1] for k in range(7)])
    print(f"every used match: direction error Cauchy {np.round(tc, 3)}, linear {np.round(tl, 1)}; states {c['state']}, {l['state']}")
    assert (c["state"] == prr.CONVERGED).all() and (tc < 1.0).all() and (tl > tc).all() and (c["margin"] >= NEAR).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "noisy005", "noisy05"])
def test_device_against_reference(ba, gpu_ok, kind):
    """rounds = 0: states, pose, cost_after, sets and n_consistent against the reference within the module's bounds; exact: the sets
    are every used match of 7 .. 600 (the wave and the workgroup boundaries of the strided passes) and the refined pose reaches the
    true one within the pose bound"""
    p, x, pairs, s = start(ba, kind)
    a, b = ref_run(ba, kind, rounds=0)
    out = run(ba, p, x, pairs, dev_info(ba, s), threshold=TAU, rounds=0)
    clear = compare(ba, kind, p, x, pairs, out, a, b)
    assert len(clear) == len(pairs)
    assert out["refine_counts"] == dict(converged=len(pairs), stalled=0, max_iter=0, nonfinite=0, skipped=0)
    if kind == "exact":
        bound = bounds(p, x, pairs, a, b)[0]
        truth = [pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1) for k in range(len(pairs))]
        err = np.array([pf.pose_error(out["r"][k], out["t"][k], rr.rotation_vector(R), t)[0] for k, (R, t, _) in enumerate(truth)])
        ref = np.array([pf.pose_error(a["r"][k], a["t"][k], rr.rotation_vector(R), t)[0] for k, (R, t, _) in enumerate(truth)])
        print(f"exact: distance to the true pose: device {err.max():.2e}, reference {ref.max():.2e} (bound {bound:.1e})")
        assert (err <= bound).all()
        assert list(out["n_inliers"]) == list(COUNTS) == list(out["n_consistent"])


@pytest.mark.gpu
def test_robust_loss_on_a_contaminated_set(ba, gpu_ok):
    """noisy05, every used match (30 % wrong), from the five-point reference's poses: Cauchy with c = 1 against the reference as
    above; the linear loss on the same call ends with the larger direction error on the pairs where the reference's does (all 7)"""
    p, x, pairs, s = start(ba, "noisy05")
    a, b = ref_run(ba, "noisy05", every=True, rounds=0, loss="cauchy", f_scale=1.0)
    info = dev_info(ba, dict(s, inlier=None))
    m = _model(ba, p)
    try:
        out = ba.refine_relative_pose(m, x, pairs, info, threshold=TAU, rounds=0, loss="cauchy", f_scale=1.0)
        lin = ba.refine_relative_pose(m, x, pairs, info, threshold=TAU, rounds=0)
    finally:
        m.close()
    compare(ba, "cauchy on every used match", p, x, pairs, out, a, b)
    l, _ = ref_run(ba, "noisy05", every=True, rounds=0)
    ang = lambda o, k: prr.angles(p, p["x_true"], k, o["r"][k], o["t"][k])[1]  # noqa: E731
    where = [k for k in range(7) if ang(l, k) > ang(a, k)]
    assert len(where) == 7
    for k in where:
        assert ang(lin, k) > ang(out, k), k


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [2, 8])
def test_rounds(ba, gpu_ok, rounds):
    """noisy05 with re-scoring rounds: sets, n_inliers, n_consistent and pose against the reference on the pairs where no used match
    lies within 1e-4 tau of tau under any round's pose (at least NEED_ROUNDS of 7; the reference adopts a set on two pairs)"""
    p, x, pairs, s = start(ba, "noisy05")
    a, b = ref_run(ba, "noisy05", rounds=rounds)
    out = run(ba, p, x, pairs, dev_info(ba, s), threshold=TAU, rounds=rounds)
    clear = compare(ba, f"rounds = {rounds}", p, x, pairs, out, a, b)
    assert len(clear) >= NEED_ROUNDS and a["adopted"][clear].max() >= 1
    assert (out["n_consistent"][clear] >= out["n_inliers"][clear]).all()


@pytest.mark.gpu
def test_states(ba, gpu_ok):
    """SKIPPED (an incoming status that is not OK, f = 0, a set of 4) with pose and inlier bytes bit-unchanged; a set of exactly 5
    runs; max_iter = 0 evaluates only; a NaN start is NONFINITE and untouched"""
    p, x, pairs, s = start(ba, "noisy05")
    info = dev_info(ba, s)
    ptr = s["match_ptr"]
    info["status"][0] = "degenerate"
    x2 = x.copy()
    pf.cameras(p, x2)[2, 8] = 0.0   # camera a of pair 1
    for k, keep in ((2, 4), (3, 5)):
        members = np.flatnonzero(info["inliers"][ptr[k]:ptr[k + 1]]) + ptr[k]
        info["inliers"][members[keep:]] = False
    info["r"][4] = np.nan
    info["n_inliers"] = np.array([info["inliers"][ptr[k]:ptr[k + 1]].sum() for k in range(7)], dtype=np.int32)
    m = _model(ba, p)
    try:
        out = ba.refine_relative_pose(m, x2, pairs, info, threshold=TAU, rounds=0)
        ev = ba.refine_relative_pose(m, x, pairs, dev_info(ba, s), threshold=TAU, rounds=0, max_iter=0)
    finally:
        m.close()
    assert list(out["refine_status"][:5]) == ["skipped", "skipped", "skipped", out["refine_status"][3], "nonfinite"]
    assert out["refine_status"][3] in ("converged", "stalled", "max_iter") and out["refine_status"][5] == out["refine_status"][6] == "converged"
    for k in (0, 1, 2, 4):
        assert np.array_equal(bits(out["r"][k]), bits(info["r"][k])) and np.array_equal(bits(out["t"][k]), bits(info["t"][k])), k
        assert np.array_equal(out["inliers"][ptr[k]:ptr[k + 1]], info["inliers"][ptr[k]:ptr[k + 1]]) and out["n_inliers"][k] == info["n_inliers"][k]
    for k in (0, 1, 2):
        assert out["cost_before"][k] == 0.0 == out["cost_after"][k] and out["iters"][k] == 0 and out["n_consistent"][k] == 0
    assert out["n_inliers"][3] == 5 and out["iters"][3] >= 1 and out["cost_after"][3] <= out["cost_before"][3]
    assert not np.isfinite(out["cost_before"][4]) and out["iters"][4] == 0
    assert out["refine_counts"]["skipped"] == 3 and out["refine_counts"]["nonfinite"] == 1
    a, _ = ref_run(ba, "noisy05", rounds=0)
    assert list(ev["refine_status"]) == ["max_iter"] * 7 and (ev["iters"] == 0).all()
    assert np.array_equal(bits(ev["r"]), bits(s["r"])) and np.array_equal(bits(ev["t"]), bits(s["t"]))
    assert np.array_equal(bits(ev["cost_before"]), bits(ev["cost_after"])) and np.allclose(ev["cost_before"], a["cost"][:, 0], rtol=1e-9)
    assert np.array_equal(ev["inliers"], s["inlier"])


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """two calls give the same bytes in every output; a pair alone gives its bits inside the call of seven; an obs_info that drops
    matches equals the call on a mask without them; the next lm_step on the handle is bit-equal to one without the call; a
    communicator is refused with the entry's name; npairs = 0 is fine"""
    from _lm_run import attach_loopback, loopback_world
    p, x, pairs, s = start(ba, "noisy05")
    info = dev_info(ba, s)
    ptr, oa, ob = s["match_ptr"], *pf.matches(p, pairs)[1:]
    kw = dict(threshold=TAU, rounds=2, loss="huber", f_scale=1.5)
    drop = np.zeros(ptr[-1], dtype=bool)
    drop[ptr[1]:ptr[2]:5] = True
    drop[ptr[5] + 1:ptr[6]:3] = True
    sigma = np.ones(p["nobs"])
    half = np.flatnonzero(drop)
    sigma[oa[half[::2]]] = np.inf
    sigma[ob[half[1::2]]] = np.inf
    masked = dict(info, inliers=info["inliers"] & ~drop)
    q = small_scene(ba)
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    keys = ("r", "t", "cost_before", "cost_after")
    try:
        i1 = ba.refine_relative_pose(m, x, pairs, info, **kw)
        i2 = ba.refine_relative_pose(m, x, pairs, info, **kw)
        sub = lambda k: dict(r=info["r"][[k]], t=info["t"][[k]], status=info["status"][[k]], inliers=info["inliers"][ptr[k]:ptr[k + 1]],  # noqa: E731
                             n_inliers=info["n_inliers"][[k]])
        alone = {k: ba.refine_relative_pose(m, x, pairs[[k]], sub(k), **kw) for k in (0, 3, 6)}
        none = ba.refine_relative_pose(m, x, np.zeros((0, 2), dtype=np.int64),
                                       dict(r=np.zeros((0, 3)), t=np.zeros((0, 3)), status=np.zeros(0, dtype="<U2"), inliers=np.zeros(0, dtype=bool)), **kw)
        by_info = ba.refine_relative_pose(m, x, pairs, info, obs_info=sigma, threshold=TAU, rounds=0)
        by_mask = ba.refine_relative_pose(m, x, pairs, masked, threshold=TAU, rounds=0)
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        rp = ba.relative_pose(ms, q["x0"], np.array([[1, 2], [3, 4], [2, 1]]))
        ba.refine_relative_pose(ms, q["x0"], np.array([[1, 2], [3, 4], [2, 1]]), rp, threshold=4.0)
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.refine_relative_pose(mc, x, pairs, info, **kw)
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_refine_relative_pose" in str(e.value) and "communicator" in str(e.value)
    for key in keys:
        assert np.array_equal(bits(i1[key]), bits(i2[key])), key
    for key in ("refine_status", "inliers", "n_inliers", "n_consistent", "iters"):
        assert np.array_equal(i1[key], i2[key]), key
    for k, ia in alone.items():
        for key in keys:
            assert np.array_equal(bits(ia[key][0]), bits(i1[key][k])), (k, key)
        assert np.array_equal(ia["inliers"], i1["inliers"][ptr[k]:ptr[k + 1]]) and ia["refine_status"][0] == i1["refine_status"][k]
        assert ia["n_inliers"][0] == i1["n_inliers"][k] and ia["n_consistent"][0] == i1["n_consistent"][k] and ia["iters"][0] == i1["iters"][k]
    assert none["r"].shape == (0, 3) and none["refine_counts"]["converged"] == 0
    for key in keys:
        assert np.array_equal(bits(by_info[key]), bits(by_mask[key])), key
    for key in ("refine_status", "inliers", "n_inliers", "iters"):
        assert np.array_equal(by_info[key], by_mask[key]), key
    assert not by_info["inliers"][drop].any() and by_info["n_inliers"][1] < info["n_inliers"][1]
    for a_, b_, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a_), np.asarray(b_)) and np.array_equal(np.asarray(b_), np.asarray(c_))


@pytest.mark.gpu
def test_refine_keyword(ba, gpu_ok):
    """relative_pose_five_point(..., refine=dict(...)) equals the two separate calls bit for bit (threshold from the ransac
    options); refine=None equals the C entry called directly, the unchanged path, on the three forms of test_five_point"""
    L, lib = ba._lib.lib(), ba._lib
    for kind in ("exact", "noisy005", "noisy05"):
        p, x, pairs = form(ba, kind)
        o = tfp.opts(kind)
        m = _model(ba, p)
        try:
            plain = ba.relative_pose_five_point(m, x, pairs, ransac=o, refine=None)
            n = len(pairs)
            a1, b1 = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
            pose, status = np.full((n, 6), np.nan), np.zeros(n, dtype=np.uint8)
            inl, n_in = np.zeros(int(plain["match_ptr"][-1]), dtype=np.uint8), np.zeros(n, dtype=np.int32)
            ro = lib.ransac_opts(o, least=5, most=5, least_set=8)
            lib.check(L.ba_relative_pose_five_point(m.handle, lib.ptr(x), n, lib.ptr(a1), lib.ptr(b1), C.byref(ro), lib.ptr(pose), lib.ptr(status),
                                                    None, lib.ptr(inl), lib.ptr(n_in), None, None))
            if kind == "noisy05":
                both = ba.relative_pose_five_point(m, x, pairs, ransac=o, refine=dict(rounds=1, loss="soft_l1"))
                two = ba.refine_relative_pose(m, x, pairs, plain, threshold=o["threshold"], rounds=1, loss="soft_l1")
                eight = ba.relative_pose(m, x, pairs, refine=dict(threshold=2.0, rounds=0))
        finally:
            m.close()
        assert np.array_equal(bits(plain["r"]), bits(pose[:, :3])) and np.array_equal(bits(plain["t"]), bits(pose[:, 3:]))
        assert np.array_equal(plain["inliers"], inl != 0) and np.array_equal(plain["n_inliers"], n_in)
        assert list(plain["status"]) == [lib.PAIR_STATES[c] for c in status] and "refine_status" not in plain
    assert set(both) == set(two) and "refine_status" in both and "refine_status" in eight
    for key in ("r", "t", "cost_before", "cost_after"):
        assert np.array_equal(bits(both[key]), bits(two[key])), key
    for key in ("status", "refine_status", "inliers", "n_inliers", "n_consistent", "iters", "best_hypothesis", "match_ptr"):
        assert np.array_equal(both[key], two[key]), key
    assert both["refine_counts"] == two["refine_counts"] and both["refine_counts"]["skipped"] == 0
