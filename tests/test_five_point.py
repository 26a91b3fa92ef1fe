"""The five-point essential matrix as the minimal solver of the two-view consensus stage (ba_five_point,
ba_relative_pose_five_point, include/ba_hip.h; five_point and relative_pose_five_point of the package).  The reference
is tests/helpers/five_point_ref.py: the header restated in numpy (np.linalg.eigh, np.linalg.solve, np.roots and svd where the
kernel runs Jacobi sweeps, Gauss-Jordan and a simultaneous complex iteration).  The first tests need no device.

Tuples of the solver tests: pair k of a scene of test_relative_pose.pair_scene in which every pair shares exactly five points
(the generator's geometry: unit ball seen from distance 5..7, f in 400..1800); the first 200 re-projected exactly, the last 100
with 0.5 px Gaussian noise on every detection; TUPLE_SEED = 77.
Consensus scenes: those of tests/test_relative_pose.py (its counts and outlier counts, its seeds), in three forms: exact (tau = 1
px, refits 0), and the seven pairs with n >= 63 at 0.05 px and at 0.5 px of noise (tau = 2 px, up to 4 refits).  Seeds, noise
levels and tau were chosen on the reference, never on the device.  exact and 0.05 px are the scenes of test_relative_pose to the
bit (its scene, noise and outlier seeds) with the consensus seed 0 and 1; with its seeds the 0.5 px form has 2 comparable pairs
(ties between all-inlier hypotheses, and displaced detections within 10 % of tau under the final pose), so that form draws its
noise with seed 0 and its outliers with seed 0 and uses the consensus seed 1, found by a search on the reference over 1300
combinations of seeds: 4 of 7 pairs comparable, 5 of 7 end on the truth, the eight-point reference on none.

Bounds, all from the reference:
  residuals  a device solution satisfies the five epipolar equations, det E = 0 and the trace constraint within 100 x the
             reference's own largest residual on that tuple, floor: that quantity's maximum over the file's tuples.
  solutions  a reference solution whose nearest other reference solution is farther than 1e-3 has a device solution within
             100 x the reference's spread on that tuple under a permutation of the five, floor: 10 x the largest difference over
             the file's tuples between the reference's two formulations of the null space, svd(A) against eigh(A'A) (computed in
             test_reference_solver and printed there: 2.3e-9 at most on these tuples, 99th percentile 7.5e-10, so the floor is
             2.3e-8, far below the 1e-3 at which two solutions count as distinct; test_reference_solver asserts that it stays
             below 1e-6).  The reference's largest residual on these tuples is 1.5e-11, its largest spread 3.7e-10.
             Measured on the device: the worst distance to a reference solution is 2.3e-9, the worst residual 4.6e-12.
  poses      |R - R_ref|_F + |t - t_ref| within 100 x the reference's spread under a permutation of the final set's matches,
             floor 1e-12; seeded points: 100 x the spread of the reference's own pipeline, floor 1e-10 (test_relative_pose)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import five_point_ref as f5  # noqa: E402
import pair_ref as pf  # noqa: E402
import points_ref as ptr_ref  # noqa: E402
import resect_ref as rr  # noqa: E402
import test_relative_pose as trp  # noqa: E402
from refine_util import _model, bits, small_scene  # noqa: E402

TUPLES, EXACT_TUPLES, TUPLE_SEED, TUPLE_SIGMA = 300, 200, 77, 0.5
SEPARATED, IMAG_CLEAR = 1e-3, 1e-6
FORMS = {"exact": dict(keep=list(range(len(trp.COUNTS))), tau=1.0, refits=0, sigma=0.0, outlier_seed=5, noise_seed=trp.NOISE_SEED, seed=0),
         "noisy005": dict(keep=trp.KEEP_NOISY, tau=2.0, refits=4, sigma=0.05, outlier_seed=6, noise_seed=trp.NOISE_SEED, seed=1),
         "noisy05": dict(keep=trp.KEEP_NOISY, tau=2.0, refits=4, sigma=0.5, outlier_seed=0, noise_seed=0, seed=1)}
NEED_COMPARABLE = {"exact": 7, "noisy005": 5, "noisy05": 4}
cached = trp.cached


# ---- the tuples of the solver tests ---------------------------------------------------------------------------------------
def tuples(ba):
    """(qa, qb (TUPLES, 5, 2), the true E of every tuple with norm 1)"""
    def build():
        p = trp.pair_scene(ba, [5] * TUPLES, TUPLE_SEED)
        pt2d = p["pt2d"].reshape(-1, 2).copy()
        noisy = (p["cam_idx1"] - 1) >= 2 * EXACT_TUPLES
        pt2d[noisy] += np.random.default_rng(TUPLE_SEED + 1).normal(0.0, TUPLE_SIGMA, (int(noisy.sum()), 2))
        p = dict(p, pt2d=np.ascontiguousarray(pt2d.ravel()))
        _, _, _, data = pf.rays(p, p["x_true"], trp.pairs_of(p))
        Et = []
        for k in range(TUPLES):
            R, t, _ = pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)
            Et.append(pf.essential(R, t) / np.linalg.norm(pf.essential(R, t)))
        return np.array([d[0] for d in data]), np.array([d[1] for d in data]), np.array(Et)
    return cached(("tuples",), build)


def planar_tuple():
    """five points of the plane z = 0.3 x - 0.2 y seen by two cameras of the generator's geometry"""
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (5, 3))
    X[:, 2] = 0.3 * X[:, 0] - 0.2 * X[:, 1]
    out = []
    for r, c in ((np.array([0.05, -0.1, 0.02]), np.array([0.3, 0.1, 6.0])), (np.array([-0.1, 0.15, 0.05]), np.array([-0.8, 0.4, 5.5]))):
        R = pf.br.rotations(r[None])[0]
        P = (X - c) @ R.T  # (the camera at c looks down -z at the points)
        out.append(-P[:, :2] / P[:, 2:3])
    return out[0], out[1]


def solver_reference(ba):
    """per tuple: the reference's solutions, its residual, its spread under a permutation of the five, the difference between its two
    null-space formulations, and whether n_sol is comparable"""
    def build():
        qa, qb, _ = tuples(ba)
        rng = np.random.default_rng(3)
        ref = []
        for k in range(TUPLES):
            E, st = f5.solve(qa[k], qb[k])
            perm = rng.permutation(5)
            while np.array_equal(perm, np.arange(5)):
                perm = rng.permutation(5)
            Ep, _ = f5.solve(qa[k][perm], qb[k][perm])
            Es, _ = f5.solve(qa[k], qb[k], how="svd")
            sep = [min((f5.distance(F, G) for j, G in enumerate(E) if j != i), default=np.inf) for i, F in enumerate(E)]
            ref.append(dict(E=E, n_perm=len(Ep), sep=np.array(sep), resid=max((max(f5.residuals(F, qa[k], qb[k])) for F in E), default=0.0),
                            spread=max((f5.nearest(F, Ep) for F in E), default=0.0) if len(Ep) == len(E) else np.inf,
                            forms=max((f5.nearest(F, Es) for F in E), default=0.0) if len(Es) == len(E) else np.inf,
                            ratio=st["ratio"], imag=st["imag"]))
        for r in ref:
            r["count_ok"] = bool((r["sep"] > SEPARATED).all() and r["imag"] > IMAG_CLEAR
                                 and not (f5.NULL_RATIO / 100 < r["ratio"] < f5.NULL_RATIO * 100))
        return ref
    return cached(("solver_reference",), build)


# ---- the consensus scenes ---------------------------------------------------------------------------------------------------
def form(ba, kind):
    """test_relative_pose.form with this module's forms"""
    def build():
        f = FORMS[kind]
        p = trp.pair_scene(ba, [trp.COUNTS[i] for i in f["keep"]], trp.SCENE_SEED)
        pt2d = p["pt2d"].reshape(-1, 2) + np.random.default_rng(f["noise_seed"]).normal(0.0, 1.0, (p["nobs"], 2)) * f["sigma"]
        per_cam = np.zeros(p["ncams"], dtype=np.int64)
        per_cam[1::2] = [trp.OUTLIERS[i] for i in f["keep"]]
        pt2d, _ = ba.synthetic.add_outliers(dict(p, pt2d=pt2d.ravel()), n_per_camera=per_cam, seed=f["outlier_seed"])
        return dict(p, pt2d=np.ascontiguousarray(pt2d.ravel())), trp.intrinsics_only(p), trp.pairs_of(p)
    return cached(("form5", kind), build)


def opts(kind, **over):
    f = FORMS[kind]
    return dict(dict(threshold=f["tau"], hypotheses=128, refits=f["refits"], seed=f["seed"]), **over)


def reference(ba, kind, info=None, key=None, **over):
    p, x, pairs = form(ba, kind)
    o = opts(kind, **over)
    return cached(("reference5", kind, key, tuple(sorted(over.items()))),
                  lambda: f5.relative_pose(p, x, pairs, o["threshold"], hypotheses=o["hypotheses"], refits=o["refits"],
                                           min_inliers=o.get("min_inliers", 0), seed=o["seed"], info=info))


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
    return cached(("truth5", kind), build)


def comparable(con, tr, min_inliers=8):
    """test_relative_pose.comparable with a lead of 3 in place of every tie, extended by the candidates of a hypothesis: too few
    matches; or no consensus with every count (at the largest any candidate reaches) <= min_inliers - 3; or an OK pair that is
    stable by the truth or by its chain.  By the truth: the winner is an all-inlier sample that counts the whole truth, every
    hypothesis before it and every contaminated hypothesis reaches at most that count - 3 (each at the largest count any (R, t) of
    any of its solutions reaches: a tie with a later all-inlier hypothesis goes to the winner, the lower h).  By the chain: the
    winner leads every other hypothesis by 3 or more, counted in the same way.  Either way the winner's best candidate leads its
    other candidates by 3 or more, its cheirality vote and those of the refits and the final fit were won by 3 or more, under the
    winner's pose and every refit's pose no used match lies within 1e-4 tau of tau, under the final pose none within 10 %, and no
    lambda_5 / lambda_9 lies within a factor 100 of 1e-12."""
    clean = trp.clean_hypotheses(con, tr)
    ptr = con["match_ptr"]
    ok = np.zeros(len(con["status"]), dtype=bool)
    with np.errstate(invalid="ignore"):
        near = ((con["ratio"] > f5.NULL_RATIO / 100) & (con["ratio"] < f5.NULL_RATIO * 100)).any(axis=1)
    for k, st in enumerate(con["status"]):
        cnt, hi = con["counts"][k], con["counts_hi"][k]
        if st == pf.FEW_MATCHES:
            ok[k] = True
        elif st == pf.NO_CONSENSUS:
            ok[k] = hi.max() <= min_inliers - 3 and not near[k]
        elif st == pf.OK:
            b = con["best_hyp"][k]
            rivals = np.concatenate([hi[:b], hi[b + 1:][~clean[k, b + 1:]]])
            by_truth = clean[k, b] and cnt[b] == tr[ptr[k]:ptr[k + 1]].sum() and (rivals.size == 0 or rivals.max() <= cnt[b] - 3)
            by_chain = con["runner_lead"][k] >= 3
            ok[k] = ((by_truth or by_chain) and con["cand_lead"][k, b] >= 3 and con["hyp_lead"][k, b] >= 3
                     and con["chain_margin"][k] >= 1e-4 and con["lead"][k] >= 3 and con["margin"][k] >= 0.1 and not near[k])
    return ok


def final_is_truth(con, tr):
    ptr = con["match_ptr"]
    return np.array([st == pf.OK and np.array_equal(con["inlier"][ptr[k]:ptr[k + 1]], tr[ptr[k]:ptr[k + 1]]) for k, st in enumerate(con["status"])])


def run(ba, p, x, pairs, ransac, **kw):
    m = _model(ba, p)
    try:
        return ba.relative_pose_five_point(m, x, pairs, ransac=ransac, **kw)
    finally:
        m.close()


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_julia_and_refusals(ba):
    L, lib = ba._lib.lib(), ba._lib
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "BALHIP.jl")).read()
    for name in ("ba_relative_pose_five_point", "ba_five_point"):
        assert name in lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header and f"(:{name}, libba)" in julia
    assert "function relative_pose_five_point(" in julia and "function five_point(" in julia
    for word in ("five-point", "only a start", "lambda_5 <= 1e-12 lambda_9", "ba_relative_pose_five_point"):
        assert word in header
    tail = (None,) * 7
    good = lib.RansacOpts(1.0, 0, 0, -1, 0, 0)
    who = b"ba_relative_pose_five_point"
    assert L.ba_relative_pose_five_point(None, None, 0, None, None, C.byref(good), *tail) == 1
    assert who in L.ba_last_error() and b"null argument" in L.ba_last_error()
    assert L.ba_relative_pose_five_point(None, None, 0, None, None, None, *tail) == 1
    assert who in L.ba_last_error() and b"null options" in L.ba_last_error()
    for bad, word in ((dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=np.nan), b"threshold"),
                      (dict(threshold=np.inf), b"threshold"), (dict(hypotheses=4097), b"hypotheses"), (dict(sample=4), b"sample"),
                      (dict(sample=6), b"sample"), (dict(sample=8), b"sample"), (dict(refits=9), b"refits"), (dict(min_inliers=7), b"min_inliers")):
        o = lib.RansacOpts(**dict(dict(threshold=1.0, hypotheses=0, sample=0, refits=-1, min_inliers=0, seed=0), **bad))
        assert L.ba_relative_pose_five_point(None, None, 0, None, None, C.byref(o), *tail) == 1
        msg = L.ba_last_error()
        assert word in msg and who in msg, (bad, msg)
    # a good set of options reaches the argument check: sample 5 and min_inliers 8 are taken
    o = lib.RansacOpts(1.0, 16, 5, 0, 8, 3)
    assert L.ba_relative_pose_five_point(None, None, 0, None, None, C.byref(o), *tail) == 1 and b"null argument" in L.ba_last_error()
    one = np.zeros(90)
    n1 = np.zeros(1, dtype=np.int32)
    for args in ((None, 0, None, None, None, None), (None, 1, lib.ptr(one), lib.ptr(one), lib.ptr(one), lib.ptr(n1))):
        assert L.ba_five_point(*args) == 1 and b"ba_five_point" in L.ba_last_error() and b"null argument" in L.ba_last_error()
    # the siblings' refusals are what they were
    o = lib.RansacOpts(1.0, 0, 7, -1, 0, 0)
    assert L.ba_relative_pose(None, None, 0, None, None, C.byref(o), *tail) == 1 and b"sample in 8..16" in L.ba_last_error()
    o = lib.RansacOpts(1.0, 0, 5, -1, 0, 0)
    assert L.ba_relative_pose(None, None, 0, None, None, C.byref(o), *tail) == 1 and b"sample in 8..16" in L.ba_last_error()
    pos, taken = np.zeros(16, dtype=np.int64), C.c_int(0)
    assert L.ba_ransac_sample(0, 0, 100, None, 5, lib.ptr(pos), C.byref(taken)) == 1 and b"ba_ransac_sample" in L.ba_last_error()
    assert ba.relative_pose.__kwdefaults__ == dict(ransac=None, obs_info=None)
    assert ba.relative_pose_five_point.__kwdefaults__ == dict(obs_info=None)
    # Python: ValueError before any device call (None stands in for the model)
    x = np.zeros(3)
    for bad in (None, dict(), dict(threshold=0.0), dict(threshold=float("nan")), dict(threshold="a"), dict(threshold=1.0, hypotheses=4097),
                dict(threshold=1.0, sample=4), dict(threshold=1.0, sample=6), dict(threshold=1.0, sample=8), dict(threshold=1.0, refits=9),
                dict(threshold=1.0, min_inliers=7), dict(threshold=1.0, min_inliers=5), dict(threshold=1.0, seed=-1),
                dict(threshold=1.0, tau=2.0), dict(threshold=1.0, five_point=True), 4.0):
        with pytest.raises(ValueError):
            ba.relative_pose_five_point(None, x, [[1, 2]], ransac=bad)
    with pytest.raises(ValueError, match="obs_info"):
        ba.relative_pose_five_point(None, x, [[1, 2]], ransac=dict(threshold=1.0), obs_info=np.array([-1.0]))
    p = small_scene(ba)

    class Sizes:
        ncams, npnts, nobs = p["ncams"], p["npnts"], p["nobs"]
    for bad in ([[1, 1]], [[0, 2]], [[1, p["ncams"] + 1]], [1, 2], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="pair"):
            ba.relative_pose_five_point(Sizes, x, bad, ransac=dict(threshold=1.0))
    for qa, qb in ((np.zeros((2, 5, 3)), np.zeros((2, 5, 3))), (np.zeros((2, 4, 2)), np.zeros((2, 4, 2))), (np.zeros((2, 5, 2)), np.zeros((3, 5, 2))),
                   (np.zeros((5, 2)), np.zeros((5, 2)))):
        with pytest.raises(ValueError, match="five_point"):
            ba.five_point(None, qa, qb)
    o = lib.ransac_opts(dict(threshold=2.5), least=5, most=5, least_set=8)
    assert (o.threshold, o.hypotheses, o.sample, o.refits, o.min_inliers, o.seed) == (2.5, 0, 0, -1, 0, 0)
    assert lib.ransac_opts(dict(threshold=1.0, sample=5, min_inliers=8), least=5, most=5, least_set=8).sample == 5
    assert lib.ransac_opts(dict(threshold=1.0, sample=6)).sample == 6 and lib.ransac_opts(dict(threshold=1.0, sample=16), least=8).sample == 16
    with pytest.raises(ValueError, match=r"sample must lie in 8\.\.16"):
        lib.ransac_opts(dict(threshold=1.0, sample=7), least=8)


def test_reference_solver(ba):
    """The reference alone: every solution satisfies the five epipolar equations, det E = 0 and the trace constraint; the true E is
    among the solutions of every exact tuple; the number of solutions does not change under a permutation of the five; at least
    80 % of the tuples qualify for the comparison of n_sol; the special tuples (two identical matches, all NaN) have none."""
    qa, qb, Et = tuples(ba)
    ref = solver_reference(ba)
    resid = max(r["resid"] for r in ref)
    miss = max(f5.nearest(Et[k], ref[k]["E"]) for k in range(EXACT_TUPLES))
    forms = np.array([r["forms"] for r in ref])
    counts = np.bincount([len(r["E"]) for r in ref], minlength=11)
    qualify = sum(r["count_ok"] for r in ref)
    print(f"solutions per tuple {counts}, largest residual {resid:.2e}, the true E missed by at most {miss:.2e}, svd against eigh "
          f"{np.max(forms[np.isfinite(forms)]):.2e} (99th percentile {np.percentile(forms[np.isfinite(forms)], 99):.1e}), lambda_5 / lambda_9 from "
          f"{min(r['ratio'] for r in ref):.1e}, {qualify} of {TUPLES} tuples qualify for n_sol")
    assert resid <= 1e-9 and miss <= 1e-6
    assert 10 * forms.max() <= 1e-6  # (the floor of the solution bound stays three orders below SEPARATED)
    assert all(len(r["E"]) >= 1 for r in ref[:EXACT_TUPLES])
    assert all(r["n_perm"] == len(r["E"]) for r in ref if r["count_ok"])
    assert 10 * qualify >= 8 * TUPLES
    assert np.isfinite(forms).sum() >= 0.95 * TUPLES
    twin_a, twin_b = qa[0].copy(), qb[0].copy()
    twin_a[3], twin_b[3] = twin_a[1], twin_b[1]
    assert len(f5.solve(twin_a, twin_b)[0]) == 0 and len(f5.solve(np.full((5, 2), np.nan), np.full((5, 2), np.nan))[0]) == 0
    pa, pb = planar_tuple()
    for E in f5.solve(pa, pb)[0]:
        assert max(f5.residuals(E, pa, pb)) <= 1e-6


@pytest.mark.parametrize("kind", ["exact", "noisy005", "noisy05"])
def test_reference_conditions(ba, kind):
    """What the device comparison rests on, asserted on five_point_ref alone (the seeds of FORMS).  exact: 7 matches FEW_MATCHES, every
    other pair OK, at least 7 of the 10 comparable (9 are: the winner of the pair of 8 matches leads its second candidate by 2),
    and the final mask of every comparable pair the truth.  0.05 px: at least 5 of the 7 pairs comparable.  0.5 px: at least 4 of
    7 comparable, at least 4 of 7 end with the final mask equal to the truth, and the eight-point reference (pair_ref, same scene,
    same options, samples of 8) reaches the truth on fewer pairs than the five-point reference."""
    con, tr = reference(ba, kind), truth(ba, kind)
    sel, fin = comparable(con, tr), final_is_truth(con, tr)
    good = np.flatnonzero(con["status"] == pf.OK)
    b = con["best_hyp"]
    print(f"{kind}: states {con['status']}, winners {b}, counts {[int(con['counts'][k, b[k]]) for k in good]}, runner lead {con['runner_lead']}, "
          f"candidate lead {[int(con['cand_lead'][k, b[k]]) for k in good]}, cheirality lead {con['lead']}, adopted {con['adopted']}, chain margin "
          f"{con['chain_margin']}, margin {con['margin']}, lambda_5 / lambda_9 from {np.nanmin(con['ratio']):.1e}, comparable {sel.astype(int)}, "
          f"final == truth {fin.astype(int)}")
    if kind == "exact":
        assert con["status"][0] == pf.FEW_MATCHES and (con["status"][1:] == pf.OK).all() and sel[0] and sel.sum() >= NEED_COMPARABLE[kind]
        assert fin[sel][1:].all()
        return
    assert (con["status"] == pf.OK).all() and sel.sum() >= NEED_COMPARABLE[kind]
    assert con["adopted"].max() <= FORMS[kind]["refits"]
    if kind == "noisy05":
        p, x, pairs = form(ba, kind)
        o = opts(kind)
        eight = pf.relative_pose(p, x, pairs, threshold=o["threshold"], hypotheses=o["hypotheses"], sample_size=8, refits=o["refits"], seed=o["seed"])
        fin8 = final_is_truth(eight, tr)
        print(f"final == truth: five-point {int(fin.sum())} of 7, eight-point {int(fin8.sum())} of 7 (states {eight['status']})")
        assert fin.sum() >= 4 and fin8.sum() < fin.sum()


# ---- GPU: the solver alone -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_solver_against_reference(ba, gpu_ok):
    """five_point on the 300 tuples and the special ones, in calls of 1, 3, 4, 5, 257 and all tuples: the bounds of the module's
    header; n_sol equals the reference's on every tuple that qualifies; two calls give the same bytes and a tuple alone gives the
    bytes it gives among 257."""
    qa, qb, _ = tuples(ba)
    ref = solver_reference(ba)
    twin_a, twin_b = qa[0].copy(), qb[0].copy()
    twin_a[3], twin_b[3] = twin_a[1], twin_b[1]
    pa, pb = planar_tuple()
    nan = np.full((5, 2), np.nan)
    qa_all, qb_all = np.concatenate([qa, [twin_a, nan, pa]]), np.concatenate([qb, [twin_b, nan, pb]])
    m = _model(ba, small_scene(ba))
    try:
        E, ns = ba.five_point(m, qa_all, qb_all)
        E2, ns2 = ba.five_point(m, qa_all, qb_all)
        parts = {n: ba.five_point(m, qa_all[:n], qb_all[:n]) for n in (1, 3, 4, 5, 257)}
        last = ba.five_point(m, qa_all[256:257], qb_all[256:257])
        none = ba.five_point(m, np.zeros((0, 5, 2)), np.zeros((0, 5, 2)))
    finally:
        m.close()
    assert E.shape == (TUPLES + 3, 10, 3, 3) and ns.dtype == np.int32 and none[0].shape == (0, 10, 3, 3)
    assert np.array_equal(bits(E), bits(E2)) and np.array_equal(ns, ns2)
    for n, (En, nn) in parts.items():
        assert np.array_equal(bits(En), bits(E[:n])) and np.array_equal(nn, ns[:n]), n
    assert np.array_equal(bits(last[0][0]), bits(E[256])) and last[1][0] == ns[256]
    assert ((ns >= 0) & (ns <= 10)).all()
    for k in range(len(ns)):
        assert np.isfinite(E[k, :ns[k]]).all() and np.isnan(E[k, ns[k]:]).all(), k
        assert np.abs(np.linalg.norm(E[k, :ns[k]].reshape(-1, 9), axis=1) - 1.0).max(initial=0.0) <= 1e-14
    assert ns[TUPLES] == 0 and ns[TUPLES + 1] == 0
    floor_resid = max(r["resid"] for r in ref)
    forms = np.array([r["forms"] for r in ref])
    floor_sol = 10 * forms[np.isfinite(forms)].max()
    worst_resid = worst_sol = worst_abs = worst_res_abs = 0.0
    compared = counted = 0
    for k, r in enumerate(ref):
        bound = max(100 * r["resid"], floor_resid)
        for s in range(ns[k]):
            res = max(f5.residuals(E[k, s], qa[k], qb[k]))
            worst_resid, worst_res_abs = max(worst_resid, res / bound), max(worst_res_abs, res)
            assert res <= bound, (k, s, res, bound)
        if np.isfinite(r["spread"]):
            bound = max(100 * r["spread"], floor_sol)
            for i, F in enumerate(r["E"]):
                if r["sep"][i] > SEPARATED:
                    d = f5.nearest(F, E[k, :ns[k]])
                    worst_sol, worst_abs = max(worst_sol, d / bound), max(worst_abs, d)
                    compared += 1
                    assert d <= bound, (k, i, d, bound)
        if r["count_ok"]:
            counted += 1
            assert ns[k] == len(r["E"]), (k, ns[k], len(r["E"]))
    ref_planar = [max(f5.residuals(F, pa, pb)) for F in f5.solve(pa, pb)[0]]
    for s in range(ns[TUPLES + 2]):
        assert max(f5.residuals(E[TUPLES + 2, s], pa, pb)) <= max(100 * max(ref_planar, default=0.0), floor_resid)
    print(f"solver: {compared} reference solutions compared, worst distance {worst_abs:.2e}, worst distance / bound {worst_sol:.3f} (floor "
          f"{floor_sol:.1e}), worst residual {worst_res_abs:.2e}, worst residual / bound {worst_resid:.3f} (floor {floor_resid:.1e}), n_sol compared on {counted} tuples, planar tuple: {ns[TUPLES + 2]} solutions")
    assert 10 * counted >= 8 * TUPLES and compared >= 2 * TUPLES


# ---- GPU: the consensus stage ----------------------------------------------------------------------------------------------
def _pose_within_bound(info, con, p, x, pairs, sel, what):
    for k in np.flatnonzero(sel & (con["status"] == pf.OK)):
        spread, _ = trp.fit_spread(con, p, x, pairs, k)
        err = float(pf.pose_error(info["r"][k], info["t"][k], con["r"][k], con["t"][k])[0])
        bound = max(100 * spread, 1e-12)
        print(f"{what}: pair {k}: pose error {err:.3e} (bound {bound:.1e})")
        assert err <= bound, k
        assert abs(np.linalg.norm(info["t"][k]) - 1.0) <= 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "noisy005", "noisy05"])
def test_consensus_against_reference(ba, gpu_ok, kind):
    """every comparable pair has the reference's status, winner, count and mask, and its pose lies within the bound; exact: 7 matches
    are FEW_MATCHES, and 9 of the 10 pairs are comparable on the reference (the pair of 8 matches is not: its winner's best
    candidate leads the second by 2), of which the assertion asks for 7"""
    p, x, pairs = form(ba, kind)
    con = reference(ba, kind)
    sel = comparable(con, truth(ba, kind))
    assert sel.sum() >= NEED_COMPARABLE[kind] and (kind != "exact" or sel[0])
    info = run(ba, p, x, pairs, opts(kind))
    trp._compare(info, con, sel)
    _pose_within_bound(info, con, p, x, pairs, sel, kind)
    if kind == "exact":
        assert info["counts"] == dict(ok=9, few_matches=1, degenerate=0, no_consensus=0) and np.isnan(info["r"][0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 4, 5, 129])
def test_hypothesis_counts_around_a_workgroup(ba, gpu_ok, H):
    """H around the four waves of a workgroup, exact form: on the comparable pairs the device gives the reference's masks, counts,
    winners and states"""
    p, x, pairs = form(ba, "exact")
    con = reference(ba, "exact", hypotheses=H)
    sel = comparable(con, truth(ba, "exact"))
    print(f"H = {H}: {int(sel.sum())} of {len(sel)} pairs compared, states {con['status']}")
    assert 2 * sel.sum() >= len(sel)
    trp._compare(run(ba, p, x, pairs, opts("exact", hypotheses=H)), con, sel)


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """two calls give the same bits in every output; a pair alone gives its bits inside a call of many; the next lm_step on the
    handle is bit-equal to one without the call; a communicator is refused with the entry's name; npairs = 0 is fine"""
    from _lm_run import attach_loopback, loopback_world
    p, x, pairs = form(ba, "noisy05")
    o = opts("noisy05")
    q = small_scene(ba)
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    try:
        i1 = ba.relative_pose_five_point(m, x, pairs, ransac=o)
        i2 = ba.relative_pose_five_point(m, x, pairs, ransac=o)
        alone = {k: ba.relative_pose_five_point(m, x, pairs[[k]], ransac=o) for k in (0, 3, 6)}
        none = ba.relative_pose_five_point(m, x, np.zeros((0, 2), dtype=np.int64), ransac=o)
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.relative_pose_five_point(ms, q["x0"], np.array([[1, 2], [3, 4], [2, 1]]), ransac=dict(threshold=4.0))
        ba.five_point(ms, *tuples(ba)[:2])
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.relative_pose_five_point(mc, x, pairs, ransac=o)
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_relative_pose_five_point" in str(e.value) and "communicator" in str(e.value)
    for key in ("r", "t"):
        assert np.array_equal(bits(i1[key]), bits(i2[key]))
    for key in ("status", "match_ptr", "inliers", "n_inliers", "best_hypothesis"):
        assert np.array_equal(i1[key], i2[key])
    ptr = i1["match_ptr"]
    for k, ia in alone.items():
        assert np.array_equal(bits(ia["r"][0]), bits(i1["r"][k])) and np.array_equal(bits(ia["t"][0]), bits(i1["t"][k])), k
        assert np.array_equal(ia["inliers"], i1["inliers"][ptr[k]:ptr[k + 1]]) and ia["best_hypothesis"][0] == i1["best_hypothesis"][k]
        assert ia["n_inliers"][0] == i1["n_inliers"][k] and ia["status"][0] == i1["status"][k]
    assert none["r"].shape == (0, 3) and list(none["match_ptr"]) == [0] and none["counts"]["ok"] == 0
    for a, b, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c_))


@pytest.mark.gpu
def test_obs_info_drops_matches(ba, gpu_ok):
    """an obs_info that drops observations of either camera: a match is used iff both of its observations are; counts and masks
    follow the reference with the same information (exact form; the pair with 9 matches falls to FEW_MATCHES)"""
    p, x, pairs = form(ba, "exact")
    base = reference(ba, "exact")
    ptr, oa, ob = base["match_ptr"], base["obs_a"], base["obs_b"]
    sigma = np.ones(p["nobs"])
    drop = np.zeros(ptr[-1], dtype=bool)
    drop[ptr[2]:ptr[2] + 2] = True   # 9 matches - 2: FEW_MATCHES
    drop[ptr[5] + 1:ptr[6]:7] = True
    drop[ptr[8]:ptr[9]:3] = True
    half = np.flatnonzero(drop)
    sigma[oa[half[::2]]] = np.inf   # (camera a's observation of some, camera b's of the others)
    sigma[ob[half[1::2]]] = np.inf
    info_ref = np.zeros((p["nobs"], 2, 2))
    info_ref[np.isfinite(sigma)] = np.eye(2)
    con = reference(ba, "exact", info=info_ref, key="dropped")
    sel = comparable(con, truth(ba, "exact") & ~drop)
    print(f"obs_info: states {con['status']}, comparable {sel.astype(int)}")
    assert con["status"][2] == pf.FEW_MATCHES and sel.sum() >= 8 and sel[[2, 5, 8]].all()
    info = run(ba, p, x, pairs, opts("exact"), obs_info=sigma)
    trp._compare(info, con, sel)
    assert not info["inliers"][drop].any()
    for k in (5, 8):
        assert info["n_inliers"][k] < base["n_inliers"][k]


@pytest.mark.gpu
def test_seeding_end_to_end(ba, gpu_ok):
    """0.5 px, the comparable OK pairs: relative_pose_five_point -> compose_relative with the true baseline ->
    refine_points(triangulate=True, max_iter=0) on the inlier observations: the shared points come out within 100 x the spread of
    the reference's own pipeline (floor 1e-10) of the reference's"""
    kind = "noisy05"
    p, x, pairs = form(ba, kind)
    con = reference(ba, kind)
    sel = comparable(con, truth(ba, kind)) & (con["status"] == pf.OK)
    n, ptr, oa, ob = p["npnts"], con["match_ptr"], con["obs_a"], con["obs_b"]
    Ct = pf.cameras(p, p["x_true"])
    info = run(ba, p, x, pairs, opts(kind))
    ok = np.flatnonzero(sel)
    assert len(ok) >= NEED_COMPARABLE[kind] and (info["status"][ok] == "ok").all()

    def seeded(r, t):
        y = np.array(x, copy=True)
        pf.cameras(p, y)[0::2] = Ct[0::2]
        for k in ok:
            y = ba.compose_relative(y, n, 2 * k + 1, 2 * k + 2, r[k], t[k], baseline=pf.true_relative(p, p["x_true"], 2 * k, 2 * k + 1)[2])
        return y
    sigma = np.full(p["nobs"], np.inf)
    keep = np.concatenate([np.flatnonzero(info["inliers"][ptr[k]:ptr[k + 1]]) + ptr[k] for k in ok])
    assert np.array_equal(keep, np.concatenate([np.flatnonzero(con["inlier"][ptr[k]:ptr[k + 1]]) + ptr[k] for k in ok]))
    sigma[oa[keep]] = sigma[ob[keep]] = 1.0
    shared = np.unique(p["pnt_idx1"][oa[keep]] - 1)
    r2, t2 = con["r"].copy(), con["t"].copy()
    for k in ok:
        r2[k], t2[k] = trp.fit_spread(con, p, x, pairs, k)[1]
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
    err = np.abs(y[:3 * n].reshape(n, 3) - X1)[shared].max()
    print(f"seeding at 0.5 px: pairs {list(ok)}, {len(shared)} points, against the reference {err:.3e} (bound {bound:.1e})")
    assert err <= bound
    assert not np.isin(ip["status"][shared], ("degenerate", "nonfinite", "fixed")).any()
