"""Linear camera resection as the start of the per-camera refinement (ba_resect_cameras, include/ba_hip.h; DESIGN §5l;
refine_cameras(resect=True)).  The reference is tests/helpers/resect_ref.py (np.linalg.eigh and np.linalg.svd where the kernel
runs Jacobi sweeps), carried on by tests/helpers/cameras_ref.py.  The first tests need no device; the rest run on the GPU.

Scene `resect_boundary`: isolated cameras of degree 0, 1, 5, 6, 7, 8, 12, 63, 64, 65, 255, 256, 257, 600 (6 is the minimal case,
5 the first degenerate one, the others sit around the wave and workgroup widths), in two forms: *exact* -- pt2d re-projected
from x_true, the points of x_true held -- and *noisy* -- the generator's 0.5 px on pt2d, the points of x0 held (0.02 of noise).
In every start vector the pose entries of the cameras to be resected are NaN.

Bounds (from the reference alone, measured per scene, never from the device):
  linear pose (max_iter = 0): 100 x the reference against itself with the observations permuted, floor 1e-12, on
      |dC_pose| / (1 + |C_pose|) per camera;
  refined result: the recipe of test_refine_cameras.bounds -- cost 100 x spread (1) with the floor 1e-13, parameters 10 x spread
      (2) with the floor 100 xtol -- where the two paths are the reference from the resected start and the reference from a 1e-3
      perturbation of the true pose (cameras of degree >= 8; at degree 6 and 7 the noisy problem has several minima, and the
      second path starts from a 1e-3 perturbation of the resected pose: see spreads()).
Measured spreads and the device's achieved maxima: DESIGN §5l."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_run import attach_loopback, loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cameras_ref as cr  # noqa: E402
import points_ref as pr  # noqa: E402
import resect_ref as rr  # noqa: E402
from refine_util import _isolated, _model, bits, cam_prior_on, codes, only_camera, rel_cost, scaled, small_scene  # noqa: E402

XTOL, XTOL_REF = 1e-10, 1e-13
MAX_ITER = 400
DEGREES = (0, 1, 5, 6, 7, 8, 12, 63, 64, 65, 255, 256, 257, 600)
DEG = np.array(DEGREES)
# The accuracy of a linear pose is that of an eigenvector, eps lambda_12 / lambda_2, and at degree 6 to 8 lambda_2 / lambda_12 is
# whatever the seed draws (1e-6 to 2e-4 over the seeds 60..71).  The reference alone, on exact data, met the figures the tests
# below hold it to (1e-9 px RMS, 1e-12 relative in t on the far form) at 4 of these 12 seeds; 69 is the one with the widest
# margin (1.9e-10 px, 5.6e-13).  The choice was made on the reference, before any device run.
SEED = 69
POSE = np.array([True] * 6 + [False] * 3)
FAR_SCALE, FAR_SHIFT = 1e3, np.array([1e4, -2e4, 3e4])
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def nan_poses(p, x, which=None):
    """x with the pose entries of the cameras `which` (boolean, None: all) overwritten with NaN"""
    x = np.array(x, dtype=np.float64, copy=True)
    C9 = cr.cameras(p, x)
    sel = np.ones(p["ncams"], dtype=bool) if which is None else np.asarray(which)
    C9[np.ix_(sel, POSE)] = np.nan
    return x


def reproject(ba, p, x):
    """pt2d of p re-projected from x"""
    n = p["npnts"]
    X, Cm = np.asarray(x[:3 * n]).reshape(n, 3), cr.cameras(p, x)
    return np.ascontiguousarray(ba.synthetic.project(X[p["pnt_idx1"] - 1], Cm[p["cam_idx1"] - 1]).ravel())


def similarity(p, x, scale, shift):
    """x under X' = scale X + shift with the cameras transformed to match: t' = scale t - R shift (the projections stay)"""
    n = p["npnts"]
    x = np.array(x, dtype=np.float64, copy=True)
    x[:3 * n] = (scale * x[:3 * n].reshape(n, 3) + shift).ravel()
    Cm = cr.cameras(p, x)
    Cm[:, 3:6] = scale * Cm[:, 3:6] - np.einsum("cij,j->ci", cr.rotations(Cm[:, :3]), shift)
    return x


def form(ba, kind):
    """(problem, the base vector: the held points and the true / generated cameras) of a form of resect_boundary:
    `exact`, `noisy`, `far` (exact under the similarity X' = 1e3 X + (1e4, -2e4, 3e4))"""
    def build():
        p = cached("scene", lambda: _isolated(ba, DEGREES, SEED))
        if kind == "noisy":
            return p, p["x0"]
        xt = p["x_true"] if kind == "exact" else similarity(p, p["x_true"], FAR_SCALE, FAR_SHIFT)
        return dict(p, pt2d=reproject(ba, p, xt), x_true=xt), xt
    return cached(("form", kind), build)


def truth(ba, kind):
    """the true cameras in the frame of a form"""
    p, base = form(ba, kind)
    return cr.cameras(p, base if kind != "noisy" else p["x_true"])


def permuted(p, seed, info=None):
    perm = np.random.default_rng(seed).permutation(p["nobs"])
    q = dict(p, cam_idx1=p["cam_idx1"][perm], pnt_idx1=p["pnt_idx1"][perm], pt2d=np.ascontiguousarray(p["pt2d"].reshape(-1, 2)[perm].ravel()))
    return q, (None if info is None else info[perm])


def pose_err(Cm, C_ref):
    return np.linalg.norm((Cm - C_ref)[:, :6], axis=1) / (1.0 + np.linalg.norm(C_ref[:, :6], axis=1))


def linear_ref(p, x, info=None, **kw):
    """(x, flag, lambda_2 / lambda_12, spread against the permuted observations) of the reference's resection"""
    xs, flag, ratio = rr.resect(p, x, info, **kw)
    spread = 0.0
    for seed in (3,):
        q, qi = permuted(p, seed, info)
        x2, flag2, _ = rr.resect(q, x, qi, **kw)
        assert np.array_equal(flag, flag2)
        done = flag == rr.DONE
        if done.any():
            spread = max(spread, float(pose_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max()))
    return xs, flag, ratio, spread


def linear(ba, kind):
    p, base = form(ba, kind)
    return cached(("linear", kind), lambda: linear_ref(p, nan_poses(p, base)))


def linear_bound(spread):
    return max(100 * spread, 1e-12)


def terms(ba, what):
    """(keywords of refine_cameras, keywords of the reference) of the noisy form under one optional term"""
    p, _ = form(ba, "noisy")
    nc, nobs = p["ncams"], p["nobs"]
    dev, ref = {}, {}
    cam0 = p["cam_idx1"] - 1
    rng = np.random.default_rng(23)
    if what == "huber":
        dev.update(loss="huber", f_scale=5.0)
        ref.update(loss="huber", c=5.0)
    elif what == "cam_prior":
        pri = cam_prior_on(p, [6, 10], 7)  # degrees 12 and 255
        dev["camera_priors"], ref["cam_prior"] = (pri[0] + 1, pri[1], pri[2]), pri
    elif what == "ctr_prior":
        idx = np.array([5, 8, nc - 1])
        mu = np.stack([cr.centre(cam) for cam in truth(ba, "noisy")[idx]]) + rng.normal(0, 0.01, (3, 3))
        A = rng.normal(0, 1, (3, 3, 3))
        Lam = 1e4 * (np.eye(3) + 0.2 * np.einsum("kij,klj->kil", A, A))
        Lam = 0.5 * (Lam + Lam.transpose(0, 2, 1))
        dev["centre_priors"], ref["ctr_prior"] = (idx + 1, mu, Lam), (idx, mu, Lam)
    elif what == "info":  # sigma in [0.5, 3] px; Lambda = 0: degree 12 keeps 5, degree 63 keeps 6, degree 64 loses all
        s = rng.uniform(0.5, 3.0, nobs)
        info = np.zeros((nobs, 2, 2))
        info[:, 0, 0] = info[:, 1, 1] = 1.0 / s ** 2
        for deg, keep in ((12, 5), (63, 6), (64, 0)):
            o = np.flatnonzero(cam0 == int(np.flatnonzero(DEG == deg)[0]))
            kept = o[1:][np.linspace(0, deg - 2, keep).astype(int)] if keep else o[:0]  # spread over the list, its first one dropped
            info[np.setdiff1d(o, kept)] = 0.0
        dev.update(obs_info=info)
        ref.update(info=info)
    elif what != "plain":
        raise ValueError(what)
    return dev, ref


def perturbed_truth(ba, kind, seed=1):
    """the base vector with the true cameras' poses perturbed by 1e-3 relative (intrinsics: those of the base vector)"""
    p, base = form(ba, kind)
    x = np.array(base, copy=True)
    Cm = cr.cameras(p, x)
    Cm[:, :6] = truth(ba, kind)[:, :6] * (1.0 + np.random.default_rng(seed).normal(0.0, 1e-3, (p["ncams"], 6)))
    return x


def refined_ref(ba, kind, what, xtol, start="resect"):
    """the reference of a (form, term): from the resected start, or (start = "truth") cameras_ref.refine from the perturbed truth"""
    def run():
        p, base = form(ba, kind)
        kw = terms(ba, what)[1] if kind == "noisy" else {}
        if start == "resect":
            out = rr.refine(p, nan_poses(p, base), max_iter=MAX_ITER, xtol=xtol, **kw)
        else:
            out = cr.refine(p, perturbed_truth(ba, kind), max_iter=MAX_ITER, xtol=xtol, **kw)
        for a in out:
            a.setflags(write=False)
        return out
    return cached(("refined", kind, what, xtol, start), run)


def spreads(ba):
    """The noisy form's path dependence, both paths to xtol = 1e-13, over every camera the device is compared on.  Degree >= 8:
    the resected start against the 1e-3 perturbation of the true pose.  Degrees 6 and 7, where that second path may end in
    another minimum: the resected start against a 1e-3 perturbation of the resected pose, which must end in the same one
    (cost_after equal to 1e-6 relative, asserted).  These two cameras are the ill-conditioned ones and set spread (2):
    measured 6.1e-8 (degree 6) and 3.4e-8 (degree 7) against 6.5e-11 from degree 8 on."""
    def run():
        p, base = form(ba, "noisy")
        x1, st1, cost1, _, D = refined_ref(ba, "noisy", "plain", XTOL_REF)
        x2, st2, cost2, _, _ = refined_ref(ba, "noisy", "plain", XTOL_REF, "truth")
        ok = DEG >= 8
        assert ((st1 & 0x7F)[ok] == cr.CONVERGED).all() and ((st2 & 0x7F)[ok] == cr.CONVERGED).all()
        s1, s2 = rel_cost(cost2[:, 1], cost1)[ok].max(), scaled(D, cr.cameras(p, x2), cr.cameras(p, x1))[ok].max()
        low = (DEG >= 6) & ~ok
        xp = np.array(linear(ba, "noisy")[0], copy=True)
        cr.cameras(p, xp)[:, :6] *= 1.0 + np.random.default_rng(1).normal(0.0, 1e-3, (p["ncams"], 6))
        x3, st3, cost3, _, _ = cr.refine(p, np.where(np.isnan(xp), 1.0, xp), max_iter=MAX_ITER, xtol=XTOL_REF)
        assert ((st1 & 0x7F)[low] == cr.CONVERGED).all() and ((st3 & 0x7F)[low] == cr.CONVERGED).all()
        assert (np.abs(cost3[low, 1] - cost1[low, 1]) <= 1e-6 * cost1[low, 1]).all()
        s1 = max(s1, rel_cost(cost3[:, 1], cost1)[low].max())
        s2 = max(s2, scaled(D, cr.cameras(p, x3), cr.cameras(p, x1))[low].max())
        return float(s1), float(s2)
    return cached("spreads", run)


def bounds(ba):
    s1, s2 = spreads(ba)
    return max(100 * s1, 1e-13), max(10 * s2, 100 * XTOL)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_and_keyword(ba):
    L = ba._lib.lib()
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_resect_cameras", "ba_resect_cameras_dev"):
        assert name in ba._lib.SYMBOLS and hasattr(L, name)
        assert f"int {name}(" in header
    assert L.ba_resect_cameras(None, None, -1, -1.0, -1.0, None, None, None, None) == 1
    assert L.ba_resect_cameras_dev(None, None, -1, -1.0, -1.0, None, None, None, None, None) == 1
    assert "resect" in ba.refine_cameras.__kwdefaults__ and ba.refine_cameras.__kwdefaults__["resect"] is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            ba.refine_cameras(None, np.zeros(3), resect=bad)


@pytest.mark.parametrize("kind", ["exact", "far"])
def test_reference_on_exact_data(ba, kind):
    """Every camera of degree >= 6 is resected; at max_iter = 0 it reprojects to below 1e-9 px RMS (prototype: 4e-11, far 3e-10);
    after the refinement it equals the true pose to the noise-free bound of test_refine_cameras (3e-9, scaled).  far: the
    relative error of t against the truth is 1e-12 or below -- and without the normalisation the same resection does not get there
    (the sums cancel: it finds lambda_2 <= 1e-10 lambda_12 and calls every camera degenerate)."""
    p, base = form(ba, kind)
    xs, flag, ratio, spread = linear(ba, kind)
    assert np.array_equal(flag == rr.DONE, DEG >= 6) and (flag[DEG < 6] == rr.DEGENERATE).all()
    assert np.array_equal(bits(cr.cameras(p, xs)[DEG < 6]), bits(cr.cameras(p, nan_poses(p, base))[DEG < 6]))
    sc = cr.Scene(p, xs)
    f = cr.evaluate(sc, np.where(np.isnan(cr.cameras(p, xs)), 1.0, cr.cameras(p, xs)))[0]
    rms = np.sqrt(2 * f[DEG >= 6] / DEG[DEG >= 6])
    Ct = truth(ba, kind)
    terr = (np.linalg.norm((cr.cameras(p, xs) - Ct)[:, 3:6], axis=1) / np.linalg.norm(Ct[:, 3:6], axis=1))[DEG >= 6].max()
    print(f"{kind}: reprojection {rms.max():.3e} px RMS, relative t error {terr:.3e}, lambda_2 / lambda_12 {np.nanmin(ratio):.1e} .. "
          f"{np.nanmax(ratio):.1e}, spread under a permutation {spread:.3e}")
    assert rms.max() < 1e-9
    if kind == "far":
        assert terr <= 1e-12
        xu, flag_u, _ = rr.resect(p, nan_poses(p, base), normalise=False)
        got = (flag_u == rr.DONE) & (DEG >= 6)
        tu = np.linalg.norm((cr.cameras(p, xu) - Ct)[got, 3:6], axis=1) / np.linalg.norm(Ct[got, 3:6], axis=1)
        worst = tu.max() if got.any() else np.inf
        print(f"far, not normalised: {int(got.sum())} of {int((DEG >= 6).sum())} cameras resected, relative t error {worst:.3e}")
        assert not (got.sum() == (DEG >= 6).sum() and worst <= 1e-12)
    x1, st, cost, trials, D = refined_ref(ba, kind, "plain", XTOL_REF)
    ok = DEG >= 6
    err = scaled(D, cr.cameras(p, x1), Ct)[ok].max()
    print(f"{kind}: refined against the truth {err:.3e}, {trials.max()} trials")
    assert ((st & 0x7F)[ok] == cr.CONVERGED).all() and ((st & 0x7F)[~ok] == cr.DEGENERATE).all() and err <= 3e-9


def test_reference_on_noisy_data(ba):
    """Every camera of degree >= 8 ends CONVERGED within half of the GPU tests' max_iter and in the minimum the start at the true
    pose reaches (cost_after equal to 1e-6 relative); the path dependence is printed; degrees 6 and 7 are only required to end
    in a regular state."""
    p, base = form(ba, "noisy")
    xs, flag, ratio, spread = linear(ba, "noisy")
    assert np.array_equal(flag == rr.DONE, DEG >= 6)
    x1, st, cost, trials, D = refined_ref(ba, "noisy", "plain", XTOL_REF)
    x2, st2, cost2, trials2, _ = refined_ref(ba, "noisy", "plain", XTOL_REF, "truth")
    ok = DEG >= 8
    s1, s2 = spreads(ba)
    print(f"noisy: linear spread {spread:.3e} (bound {linear_bound(spread):.1e}), lambda_2 / lambda_12 {np.nanmin(ratio):.1e} .. "
          f"{np.nanmax(ratio):.1e}; refined: path dependence (1) {s1:.3e}, (2) {s2:.3e}; trials {trials[ok].max()} "
          f"(from the truth {trials2[ok].max()}); states of degree 6, 7: {st[3:5]}")
    assert ((st & 0x7F)[ok] == cr.CONVERGED).all() and trials[ok].max() <= MAX_ITER // 2
    assert (np.abs(cost[ok, 1] - cost2[ok, 1]) <= 1e-6 * cost2[ok, 1]).all()
    assert ((st & 0x7F)[DEG < 6] == cr.DEGENERATE).all() and (cost[DEG < 6] == 0).all() and (cost[:, 1] <= cost[:, 0]).all()
    assert np.isin((st & 0x7F)[(DEG >= 6) & ~ok], (cr.CONVERGED, cr.STALLED, cr.MAX_ITER)).all()


@pytest.mark.parametrize("what", ["plain", "huber", "cam_prior", "ctr_prior", "info"])
def test_reference_stays_inside_its_own_bounds(ba, what):
    """The reference holds itself inside the bounds the device is held to: the linear pose under a second permutation of the
    observations, and the refined result from the resected start against the one from the perturbed truth (degree >= 8, where
    both paths are expected in the same minimum)."""
    p, base = form(ba, "noisy")
    kw = terms(ba, what)[1]
    xs, flag, _, spread = cached(("linear", "noisy", what), lambda: linear_ref(p, nan_poses(p, base), kw.get("info")))
    q, qi = permuted(p, 4, kw.get("info"))
    x2, flag2, _ = rr.resect(q, nan_poses(p, base), qi)
    done = flag == rr.DONE
    e_lin = pose_err(cr.cameras(p, x2), cr.cameras(p, xs))[done].max()
    x1, st1, cost1, _, D = refined_ref(ba, "noisy", what, XTOL_REF)
    xt, stt, costt, _, _ = refined_ref(ba, "noisy", what, XTOL_REF, "truth")
    ok = (cr.Scene(p, base, kw.get("info")).nused >= 8) & done
    cost_bound, par_bound = bounds(ba)
    e1, e2 = rel_cost(costt[:, 1], cost1)[ok].max(), scaled(D, cr.cameras(p, xt), cr.cameras(p, x1))[ok].max()
    print(f"noisy {what}: linear {e_lin:.3e} of {linear_bound(spread):.1e}; (1) {e1:.3e} of {cost_bound:.1e}, (2) {e2:.3e} of {par_bound:.1e}")
    assert np.array_equal(flag, flag2) and e_lin <= linear_bound(spread)
    assert np.array_equal(st1[ok], stt[ok]) and e1 <= cost_bound and e2 <= par_bound
    if what == "info":
        assert flag[DEG == 12] == rr.DEGENERATE and flag[DEG == 63] == rr.DONE and flag[DEG == 64] == rr.DEGENERATE
        used = cr.Scene(p, base, kw["info"]).nused
        assert used[DEG == 12] == 5 and used[DEG == 63] == 6 and used[DEG == 64] == 0


def test_reference_builds_an_x0_from_points_alone(ba):
    """The condition of the GPU test, on the reference first: from NaN poses, the resection (intrinsics held) and three rounds of
    points / cameras end within 1 % of what the same alternation reaches from the generator's x0 (294.6)."""
    p = small_scene(ba)
    nc = p["ncams"]
    held = np.tile(~POSE, (nc, 1))
    total = lambda x: float(cr.evaluate(cr.Scene(p, x), cr.cameras(p, x))[0].sum())  # noqa: E731
    ends = []
    for start in ("nan", "x0"):
        if start == "nan":
            x = rr.refine(p, nan_poses(p, p["x0"]), xtol=XTOL, held=held)[0]
        else:
            x = np.array(p["x0"], copy=True)
        f = [total(x)]
        for _ in range(3):
            x = pr.refine(p, x, xtol=XTOL)[0]
            f.append(total(x))
            x = cr.refine(p, x, xtol=XTOL)[0]
            f.append(total(x))
        print(f"from {start}:", " ".join(f"{v:.6e}" for v in f))
        assert all(b <= a for a, b in zip(f, f[1:]))
        ends.append(f[-1])
    assert abs(ends[0] - ends[1]) <= 0.01 * ends[1]


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _run(ba, p, x, **kw):
    m = _model(ba, p)
    try:
        return ba.refine_cameras(m, x, resect=True, **kw)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "noisy"])
def test_linear_pose(ba, gpu_ok, kind):
    """resect=True, max_iter=0: the resected pose is written.  The cost entries are f_c at that pose: on the noisy form within 1e-13
    relative of the reference's f_c at the device's pose; on the exact form f_c is a sum of squared rounding errors (1e-22) that no
    two evaluation orders share a digit of, and it is held below the cost of 1e-9 px RMS instead.  Achieved on the MI355X:
    DESIGN §5l."""
    p, base = form(ba, kind)
    n = p["npnts"]
    xs, flag, _, spread = linear(ba, kind)
    x0 = nan_poses(p, base)
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, max_iter=0)
        others = [ba.refine_cameras(m, np.where(np.isnan(x0), fill, x0), resect=True, max_iter=0) for fill in (0.0, base)]
    finally:
        m.close()
    done = flag == rr.DONE
    st_ref = cr.refine(p, np.where(np.isnan(xs), 1.0, xs), max_iter=0)[1]
    st = codes(ba, info)
    assert np.array_equal(st[done], st_ref[done]) and (st[~done] == cr.DEGENERATE).all() and ((st & 0x7F)[done] == cr.MAX_ITER).all()
    assert np.array_equal(done, DEG >= 6)
    Cd, C0 = cr.cameras(p, x), cr.cameras(p, x0)
    assert np.array_equal(bits(Cd[~done]), bits(C0[~done])) and (info["cost_before"][~done] == 0).all() and (info["cost_after"][~done] == 0).all()
    err = pose_err(Cd, cr.cameras(p, xs))[done].max()
    cost_ref = cr.refine(p, np.where(np.isnan(x), 1.0, x), max_iter=0)[2][:, 0]
    nz = done & (cost_ref > 0)
    e_cost = (np.abs(info["cost_before"] - cost_ref)[nz] / cost_ref[nz]).max()
    print(f"{kind}: linear pose {err:.3e} (bound {linear_bound(spread):.1e}), cost {e_cost:.3e}, worst cost {info['cost_before'].max():.3e}")
    assert err <= linear_bound(spread)
    assert np.array_equal(bits(info["cost_before"]), bits(info["cost_after"])) and info["iters_max"] == 0
    if kind == "noisy":
        assert e_cost <= 1e-13
    else:
        assert (info["cost_before"][done] <= 0.5 * DEG[done] * 1e-18).all() and (cost_ref[done] <= 0.5 * DEG[done] * 1e-18).all()
    assert np.array_equal(bits(Cd[:, 6:]), bits(C0[:, 6:])) and np.array_equal(bits(x[:3 * n]), bits(x0[:3 * n]))
    for xo, io in others:  # the pose of x is not read
        assert np.array_equal(bits(cr.cameras(p, xo)[done]), bits(Cd[done])) and np.array_equal(bits(io["cost_after"]), bits(info["cost_after"]))
        assert np.array_equal(codes(ba, io), st)
    assert info["counts"]["degenerate"] == 3 and info["counts"]["max_iter"] == 11


def _check_refined(ba, what):
    p, base = form(ba, "noisy")
    dev_kw, ref_kw = terms(ba, what)
    x0 = nan_poses(p, base)
    x, info = _run(ba, p, x0, xtol=XTOL, max_iter=MAX_ITER, **dev_kw)
    x_ref, st_ref, cost_ref, trials_ref, D = refined_ref(ba, "noisy", what, XTOL_REF)
    cost_bound, par_bound = bounds(ba)
    st = codes(ba, info)
    assert np.array_equal(st, st_ref), (st, st_ref)
    moved = (st_ref & 0x7F) <= cr.MAX_ITER
    Cd, Cr, C0 = cr.cameras(p, x), cr.cameras(p, x_ref), cr.cameras(p, x0)
    e_before = np.max(np.abs(info["cost_before"] - cost_ref[:, 0])[moved] / cost_ref[moved, 0])
    e_after = rel_cost(info["cost_after"], cost_ref)[moved].max()
    e_par = scaled(D, Cd, Cr)[moved].max()
    print(f"noisy {what}: cost_before {e_before:.3e}, cost_after {e_after:.3e} (bound {cost_bound:.1e}), parameters {e_par:.3e} "
          f"(bound {par_bound:.1e}), trials {info['iters_max']} (reference {trials_ref.max()})")
    # cost_before is f_c at the resected pose: the device's pose differs from the reference's within the linear bound, and
    # f_c moves with it; it is held to the reference through test_linear_pose, here to the refined result only
    assert e_after <= cost_bound and e_par <= par_bound
    assert np.array_equal(bits(Cd[~moved]), bits(C0[~moved])) and (info["cost_before"][~moved] == 0).all() and (info["cost_after"][~moved] == 0).all()
    assert np.array_equal(bits(Cd[:, 6:][~moved]), bits(C0[:, 6:][~moved])) and np.array_equal(bits(x[:3 * p["npnts"]]), bits(x0[:3 * p["npnts"]]))
    assert (info["cost_after"] <= info["cost_before"]).all()
    assert sum(info["counts"][s] for s in ba._lib.POINT_STATES) == p["ncams"] and info["counts"]["behind"] == int(info["behind"].sum())
    for k, s in enumerate(ba._lib.POINT_STATES):
        assert info["counts"][s] == int(((st & 0x7F) == k).sum())
    return info, st_ref


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["plain", "huber", "cam_prior", "ctr_prior", "info"])
def test_end_to_end(ba, gpu_ok, what):
    """resect=True with the default refinement on the noisy form under the optional terms.  Achieved: DESIGN §5l."""
    info, st_ref = _check_refined(ba, what)
    want = DEG < 6
    if what == "info":
        want = want | (DEG == 12) | (DEG == 64)
    assert np.array_equal(info["status"] == "degenerate", want)
    assert (info["status"][DEG >= 65] == "converged").all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "far"])
def test_end_to_end_exact(ba, gpu_ok, kind):
    """Noise-free: the refinement from the resected pose ends at the true pose (3e-9 scaled, the noise-free bound of
    test_refine_cameras) with a cost below that of 1e-9 px RMS; far: the linear pose is within the linear bound of the reference."""
    p, base = form(ba, kind)
    x0 = nan_poses(p, base)
    xs, flag, _, spread = linear(ba, kind)
    m = _model(ba, p)
    try:
        xl, il = ba.refine_cameras(m, x0, resect=True, max_iter=0)
        x, info = ba.refine_cameras(m, x0, resect=True, xtol=XTOL, max_iter=MAX_ITER)
    finally:
        m.close()
    ok = DEG >= 6
    D = refined_ref(ba, kind, "plain", XTOL_REF)[4]
    e_lin = pose_err(cr.cameras(p, xl), cr.cameras(p, xs))[ok].max()
    err = scaled(D, cr.cameras(p, x), truth(ba, kind))[ok].max()
    print(f"{kind}: linear pose {e_lin:.3e} (bound {linear_bound(spread):.1e}); refined against the truth {err:.3e}; "
          f"cost_after {info['cost_after'].max():.3e}; trials {info['iters_max']}")
    assert e_lin <= linear_bound(spread)
    assert (info["status"][ok] == "converged").all() and (info["status"][~ok] == "degenerate").all() and not info["behind"].any()
    assert err <= 3e-9 and (info["cost_after"][ok] <= 0.5 * DEG[ok] * 1e-18).all()


@pytest.mark.gpu
def test_cameras_that_are_not_resected(ba, gpu_ok):
    """One pose bit held on two cameras, one camera fixed whole, (k1, k2, f) held on all, one group: the masked and the fixed
    cameras start from x and come back with the bits of resect=False; the group members are resected like the others."""
    p, base = form(ba, "noisy")
    nc = p["ncams"]
    held = np.tile(~POSE, (nc, 1))
    held[7, 1] = held[11, 4] = True  # degrees 63 and 256
    held[9] = True                    # degree 65
    members = np.array([6, 10, 13])   # degrees 12, 255, 600
    labels = np.zeros(nc, dtype=np.int64)
    labels[members] = 1
    from_x = held[:, :6].any(axis=1)
    x0 = nan_poses(p, base, ~from_x)
    kw = dict(fixed_camera_params=held, shared_intrinsics=[list(members + 1)], xtol=XTOL, max_iter=MAX_ITER)
    m = _model(ba, p)
    try:
        x, info = ba.refine_cameras(m, x0, resect=True, **kw)
        xp, ip = ba.refine_cameras(m, x0, resect=False, **kw)
    finally:
        m.close()
    x_ref, st_ref, cost_ref, _, D = rr.refine(p, x0, max_iter=MAX_ITER, xtol=XTOL_REF, held=held, groups=labels)
    Cd, Cp, C0 = cr.cameras(p, x), cr.cameras(p, xp), cr.cameras(p, x0)
    assert np.array_equal(bits(Cd[from_x]), bits(Cp[from_x])) and np.array_equal(codes(ba, info)[from_x], codes(ba, ip)[from_x])
    for key in ("cost_before", "cost_after"):
        assert np.array_equal(bits(info[key][from_x]), bits(ip[key][from_x]))
    assert info["status"][9] == "fixed" and (info["status"][[7, 11]] == "converged").all() and (ip["status"][~from_x & (DEG > 0)] == "nonfinite").all()
    assert np.array_equal(bits(Cd[:, 6:]), bits(C0[:, 6:])) and np.array_equal(bits(Cd[held]), bits(C0[held]))
    st = codes(ba, info)
    assert np.array_equal(st, st_ref) and (info["status"][members] == "converged").all()
    moved = (st_ref & 0x7F) <= cr.MAX_ITER
    cost_bound, par_bound = bounds(ba)
    e_after, e_par = rel_cost(info["cost_after"], cost_ref)[moved].max(), scaled(D, Cd, cr.cameras(p, x_ref))[moved].max()
    print(f"masked: cost_after {e_after:.3e} (bound {cost_bound:.1e}), parameters {e_par:.3e} (bound {par_bound:.1e})")
    assert e_after <= cost_bound and e_par <= par_bound


def _one(ba):
    """a single camera with 40 points, exact: (problem with re-projected pt2d, x_true)"""
    def build():
        p = only_camera(_isolated(ba, (40, 40), 53), 0)
        return dict(p, pt2d=reproject(ba, p, p["x_true"]))
    return cached("one", build)


def _flattened(ba, thickness):
    """`one` with its points moved towards the plane through their mean whose normal is the cloud's smallest principal
    direction, until the extent along the normal is `thickness` of what it was; pt2d re-projected"""
    p = _one(ba)
    x = np.array(p["x_true"], copy=True)
    X = x[:120].reshape(40, 3)
    mean = X.mean(0)
    nrm = np.linalg.svd(X - mean)[2][2]
    X -= (1.0 - thickness) * np.outer((X - mean) @ nrm, nrm)
    return dict(p, pt2d=reproject(ba, p, x), x_true=x), x


def _rotated(ba, r_new):
    """`one` seen by a camera of rotation vector r_new: the points are turned so that R X + t and the projections stay"""
    p = _one(ba)
    x = np.array(p["x_true"], copy=True)
    X, cam = x[:120].reshape(40, 3), x[120:]
    R0, R1 = cr.rotations(cam[None, :3])[0], cr.rotations(np.asarray(r_new, dtype=np.float64)[None])[0]
    X[:] = (X @ R0.T) @ R1
    cam[:3] = r_new
    return dict(p, pt2d=reproject(ba, p, x), x_true=x), x


@pytest.mark.gpu
def test_degenerate_geometry(ba, gpu_ok):
    """Points in a plane (relative thickness 0 and 1e-6: DEGENERATE; 1e-3: resected to the reference's pose), f = 0 and f = NaN
    (DEGENERATE, nothing written), a rotation of 1e-14 (finite, refines to CONVERGED) and one of pi - 1e-9 (compared as matrices)."""
    for th, want in ((0.0, "degenerate"), (1e-6, "degenerate"), (1e-3, "max_iter")):
        p, xt = _flattened(ba, th)
        x0 = nan_poses(p, xt)
        xs, flag, ratio, spread = linear_ref(p, x0)
        x, info = _run(ba, p, x0, max_iter=0)
        print(f"thickness {th:g}: lambda_2 / lambda_12 {ratio[0]:.2e}, {info['status'][0]}, spread {spread:.3e}")
        assert info["status"][0] == want and (flag[0] == rr.DONE) == (want != "degenerate")
        if want == "degenerate":
            assert np.array_equal(bits(x), bits(x0)) and info["cost_before"][0] == 0 and not info["behind"][0]
        else:
            e = pose_err(cr.cameras(p, x), cr.cameras(p, xs))[0]
            print(f"thickness {th:g}: linear pose {e:.3e} (bound {linear_bound(spread):.1e})")
            assert e <= linear_bound(spread)
    p = _one(ba)
    for f in (0.0, np.nan):
        x0 = nan_poses(p, p["x_true"])
        x0[-1] = f
        x, info = _run(ba, p, x0, max_iter=5)
        assert info["status"][0] == "degenerate" and np.array_equal(bits(x), bits(x0)) and info["cost_after"][0] == 0
        assert rr.resect(p, x0)[1][0] == rr.DEGENERATE
    # theta = 1e-14: below the threshold, r = (1e-12, 0, 0)
    p, xt = _rotated(ba, 1e-14 * np.array([0.6, 0.0, 0.8]))
    x0 = nan_poses(p, xt)
    xl, il = _run(ba, p, x0, max_iter=0)
    x, info = _run(ba, p, x0, xtol=XTOL, max_iter=MAX_ITER)
    assert np.isfinite(xl).all() and np.isfinite(x).all() and info["status"][0] == "converged" and np.isfinite(info["cost_after"][0])
    assert np.linalg.norm(xl[120:123]) <= 1e-11
    # theta = pi - 1e-9
    axis = np.array([0.48, -0.6, 0.64])
    p, xt = _rotated(ba, (np.pi - 1e-9) * axis)
    x0 = nan_poses(p, xt)
    xs, flag, _, spread = linear_ref(p, x0)
    x, info = _run(ba, p, x0, max_iter=0)
    Rd, Rr, Rt = (cr.rotations(v[None, 120:123])[0] for v in (x, xs, xt))
    e = np.abs(Rd - Rr).max()
    print(f"theta = pi - 1e-9: R against the reference {e:.3e} (bound {linear_bound(spread):.1e}), against the truth {np.abs(Rd - Rt).max():.3e}")
    assert flag[0] == rr.DONE and info["status"][0] == "max_iter" and e <= linear_bound(spread)
    assert abs(np.linalg.norm(x[120:123]) - np.pi) <= 1e-6


@pytest.mark.gpu
def test_determinism_and_isolation(ba, gpu_ok):
    """Two calls, and the host and the device-resident entry, give the same bits; a camera of degree 12, 255 and 600 gives the
    same bits inside its scene and alone; the next lm_step has the bits it has without the call; a communicator is refused."""
    p, base = form(ba, "noisy")
    nc, nvar = p["ncams"], len(base)
    x0 = nan_poses(p, base)
    L = ba._lib.lib()
    q = small_scene(ba)
    m, ms, plain = _model(ba, p), _model(ba, q), _model(ba, q)
    try:
        x1, i1 = ba.refine_cameras(m, x0, resect=True, xtol=XTOL, max_iter=MAX_ITER)
        x2, i2 = ba.refine_cameras(m, x0, resect=True, xtol=XTOL, max_iter=MAX_ITER)
        d = [C.c_void_p() for _ in range(3)]
        for ptr_, size in zip(d, (8 * nvar, nc, 16 * nc)):
            ba._lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        x3, st3, cost3 = x0.copy(), np.zeros(nc, dtype=np.uint8), np.zeros((nc, 2))
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        ba._lib.check(L.ba_memcpy_h2d(m.handle, d[0], ba._lib.ptr(x3), 8 * nvar))
        ba._lib.check(L.ba_resect_cameras_dev(m.handle, d[0], MAX_ITER, XTOL, -1.0, d[1], d[2], ba._lib.ptr(counts), C.byref(its), None))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(x3), d[0], 8 * nvar))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(st3), d[1], nc))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(cost3), d[2], 16 * nc))
        for ptr_ in d:
            ba._lib.check(L.ba_dev_free(m.handle, ptr_))
        alone = {}
        for c in (6, 10, nc - 1):  # degrees 12, 255 and 600
            pc = only_camera(p, c)
            alone[c] = _run(ba, pc, nan_poses(pc, pc["x0"]), xtol=XTOL, max_iter=MAX_ITER)
        ref_step = ba.lm_step(plain, q["x0"], 3.0)
        first = ba.lm_step(ms, q["x0"], 3.0)
        ba.refine_cameras(ms, nan_poses(q, q["x0"]), resect=True, xtol=XTOL)
        after = ba.lm_step(ms, q["x0"], 3.0)
        with loopback_world(1, 1 << 20) as (LL, loop):
            mc = _model(ba, p)
            try:
                attach_loopback(ba, mc, LL, loop, 0, 1)
                with pytest.raises(ba.BAArgError) as e:
                    ba.refine_cameras(mc, x0, resect=True)
            finally:
                mc.close()
    finally:
        m.close()
        ms.close()
        plain.close()
    assert "ba_resect_cameras" in str(e.value) and "communicator" in str(e.value)
    assert np.array_equal(bits(x1), bits(x2)) and np.array_equal(bits(x1), bits(x3))
    assert np.array_equal(bits(i1["cost_after"]), bits(i2["cost_after"])) and np.array_equal(bits(i1["cost_after"]), bits(cost3[:, 1]))
    assert np.array_equal(bits(i1["cost_before"]), bits(cost3[:, 0]))
    assert np.array_equal(codes(ba, i1), st3) and its.value == i1["iters_max"] and counts[0] == i1["counts"]["converged"]
    for c, (xa, ia) in alone.items():
        assert np.array_equal(bits(xa[-9:]), bits(cr.cameras(p, x1)[c])), c
        assert ia["cost_after"][0] == i1["cost_after"][c] and ia["cost_before"][0] == i1["cost_before"][c]
    for a, b, c_ in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c_))


@pytest.mark.gpu
def test_an_x0_from_points_alone(ba, gpu_ok):
    """Every camera pose of x0 is NaN: the resection with (k1, k2, f) held, then three rounds of refine_points and refine_cameras.
    The objective never rises after the first call and ends within 1 % of what the same alternation reaches from the generator's
    own x0 (294.6)."""
    p = small_scene(ba)
    m = _model(ba, p)
    try:
        ends = []
        for start in ("nan", "x0"):
            if start == "nan":
                x, info = ba.refine_cameras(m, nan_poses(p, p["x0"]), resect=True, fixed_camera_params=("k1", "k2", "f"), xtol=XTOL)
                assert (info["status"] == "converged").all()
            else:
                x = p["x0"]
            f = [m.robust_weights(x, "linear")[1]]
            for _ in range(3):
                for fn in (ba.refine_points, ba.refine_cameras):
                    x, _info = fn(m, x, xtol=XTOL)
                    f.append(m.robust_weights(x, "linear")[1])
            print(f"from {start}:", " ".join(f"{v:.6e}" for v in f))
            assert all(b <= a for a, b in zip(f, f[1:]))
            ends.append(f[-1])
    finally:
        m.close()
    assert abs(ends[0] - ends[1]) <= 0.01 * ends[1]
