"""Points with the cameras held (ba_refine_points, include/ba_hip.h): linear triangulation and the per-point
Marquardt refinement.  The reference is tests/helpers/points_ref.py, a numpy restatement of the header's text.  The first tests
need no device; the rest run on the GPU.  Scenes: every point of degree 2; small_prob; degrees 14..100 (both tiers of the kernel,
with degrees 32, 33, 64 and 65 present); one point; a point without and a point with one observation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _lm_run import solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import points_ref as pr  # noqa: E402
from refine_util import _model, codes, small_scene  # noqa: E402
from scenes import random_info  # noqa: E402

XTOL = 1e-10
TIER = 32  # PT_TIER of csrc/ba_point_kernels.hip
_SCENES, _REFS = {}, {}


def scene(ba, name):
    if name not in _SCENES:
        if name == "deg2":
            p = ba.synthetic.make_problem(5, 40, 80, seed=3)
        elif name == "small":
            p = small_scene(ba)
        elif name == "high":
            p = ba.synthetic.make_problem(100, 60, 2700, seed=11)
        elif name == "one":
            p = ba.synthetic.make_problem(4, 1, 3, seed=5)
        elif name == "ragged":  # deg2 with point 8 unobserved and point 21 seen once
            q = ba.synthetic.make_problem(5, 40, 80, seed=3)
            pnt = q["pnt_idx1"]
            keep = pnt != 8
            keep[np.flatnonzero(pnt == 21)[0]] = False
            p = dict(q, cam_idx1=q["cam_idx1"][keep], pnt_idx1=pnt[keep],
                     pt2d=np.ascontiguousarray(q["pt2d"].reshape(-1, 2)[keep].ravel()), nobs=int(keep.sum()))
        _SCENES[name] = p
    return _SCENES[name]


def ref(ba, name, tag="", **kw):
    """the reference run of a scene, computed once and shared"""
    key = (name, tag, kw.get("init", 0), kw.get("xtol", XTOL))
    if key not in _REFS:
        p = scene(ba, name)
        _REFS[key] = pr.refine(p, kw.pop("x", p["x0"]), **kw)
    return _REFS[key]


def pts(p, x):
    return np.asarray(x)[:3 * p["npnts"]].reshape(-1, 3)


def rel(p, a, b):
    A, B = pts(p, a), pts(p, b)
    return np.linalg.norm(A - B, axis=1) / (1.0 + np.linalg.norm(B, axis=1))


def noise_free(ba, p):
    n = p["npnts"]
    xt = p["x_true"]
    cams = xt[3 * n:].reshape(-1, 9)
    return dict(p, pt2d=np.ascontiguousarray(ba.synthetic.project(pts(p, xt)[p["pnt_idx1"] - 1], cams[p["cam_idx1"] - 1]).ravel()))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared(ba):
    L = ba._lib.lib()
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_refine_points", "ba_refine_points_dev"):
        assert name in ba._lib.SYMBOLS and hasattr(L, name)
        assert f"int {name}(" in header
    assert L.ba_refine_points(None, None, 0, -1, -1.0, -1.0, None, None, None, None) == 1
    assert "refine_points" in ba.__all__
    for kw in ("triangulate", "max_iter", "xtol", "lam0", "loss", "f_scale", "obs_info", "fixed_points", "point_priors"):
        assert kw in ba.refine_points.__kwdefaults__


_BAD = [dict(triangulate=1), dict(max_iter=-1), dict(max_iter=2.5), dict(xtol=0.0), dict(xtol=float("nan")), dict(xtol="a"),
        dict(lam0=-1.0), dict(lam0=float("inf")), dict(loss="l2"), dict(f_scale=0.0), dict(obs_info=-np.ones(7)),
        dict(fixed_points=[0]), dict(point_priors=([1], np.zeros((1, 3)), -np.ones((1, 3))))]


@pytest.mark.parametrize("bad", _BAD, ids=[next(iter(b)) + str(k) for k, b in enumerate(_BAD)])
def test_bad_arguments_refused_before_the_model(ba, bad):
    """No model exists here (None): the ValueError comes before anything looks at the model or the device."""
    with pytest.raises(ValueError):
        ba.refine_points(None, np.zeros(3), **bad)


@pytest.mark.parametrize("name,tri_tol", [("small", 1e-12), ("deg2", 1e-13)])
def test_reference_sanity(ba, name, tri_tol):
    """The reference on its own: triangulation of noise-free measurements under the true cameras recovers the true points
    (measured 3.0e-13 on small_prob, 2.8e-14 on the degree-2 scene: rounding of the 3 x 3 solve at |c| ~ 6); the noisy run ends
    CONVERGED everywhere within 22 trials, nothing DEGENERATE or BEHIND; the minimisers from x0 and from a start perturbed by
    sigma = 0.3 agree to 100 xtol (measured 1.5e-10 and 5.7e-11)."""
    p = scene(ba, name)
    q = noise_free(ba, p)
    X, ok = pr.triangulate(pr.Scene(q, p["x_true"]))
    Xt = pts(p, p["x_true"])
    err = np.max(np.linalg.norm(X - Xt, axis=1) / np.linalg.norm(Xt, axis=1))
    print(f"{name}: triangulation error {err:.3e}")
    assert ok.all() and err <= tri_tol
    x1, st, cost, trials = ref(ba, name)
    assert (st == pr.CONVERGED).all() and trials.max() <= 22 and (cost[:, 1] <= cost[:, 0]).all()
    assert (ref(ba, name, init=1)[1] == pr.CONVERGED).all()
    xp = p["x0"].copy()
    xp[:3 * p["npnts"]] += np.random.default_rng(0).normal(0.0, 0.3, 3 * p["npnts"])
    x2, st2, _, _ = pr.refine(p, xp)
    print(f"{name}: path dependence {rel(p, x2, x1).max():.3e}, {trials.max()} trials")
    assert (st2 == pr.CONVERGED).all() and rel(p, x2, x1).max() <= 100 * XTOL


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _check_parity(ba, name, tag, dev_kw, ref_kw, init):
    """a device run at xtol = 1e-10 against the reference: states equal to the reference's at the same xtol, every free point
    within 100 xtol (1 + |X_ref|) of the reference run to xtol = 1e-13; points the reference leaves are left bit for bit"""
    p = scene(ba, name)
    m = _model(ba, p)
    try:
        x, info = ba.refine_points(m, p["x0"], triangulate=bool(init), xtol=XTOL, **dev_kw)
    finally:
        m.close()
    _, st_ref, cost_ref, trials_ref = ref(ba, name, tag, init=init, **dict(ref_kw))
    x_ref = ref(ba, name, tag, init=init, xtol=1e-13, **dict(ref_kw))[0]
    st = codes(ba, info)
    assert np.array_equal(st, st_ref), (st, st_ref)
    moved = (st_ref & 0x7F) <= pr.MAX_ITER
    err = rel(p, x, x_ref)[moved].max() if moved.any() else 0.0
    print(f"{name} {tag} init {init}: max |X - X_ref| / (1 + |X_ref|) = {err:.3e}, trials {info['iters_max']} (reference {trials_ref.max()})")
    assert err <= 100 * XTOL
    same = ~moved
    assert np.array_equal(pts(p, x)[same].view(np.int64), pts(p, p["x0"])[same].view(np.int64))
    assert np.array_equal(x[3 * p["npnts"]:].view(np.int64), p["x0"][3 * p["npnts"]:].view(np.int64))
    assert (info["cost_after"] <= info["cost_before"]).all()
    assert np.allclose(info["cost_after"], cost_ref[:, 1], rtol=1e-8, atol=1e-12)
    assert sum(info["counts"][s] for s in ba._lib.POINT_STATES) == p["npnts"]
    assert info["counts"]["behind"] == int(info["behind"].sum())
    for k, s in enumerate(ba._lib.POINT_STATES):
        assert info["counts"][s] == int(((st & 0x7F) == k).sum())
    return x, info


@pytest.mark.gpu
@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("name", ["deg2", "small", "high", "one", "ragged"])
def test_parity_with_the_reference(ba, gpu_ok, name, init):
    p = scene(ba, name)
    if name == "high":
        deg = np.bincount(p["pnt_idx1"] - 1, minlength=p["npnts"])
        assert all((deg == d).any() for d in (TIER, TIER + 1, 64, 65))
    _, info = _check_parity(ba, name, "", {}, {}, init)
    if name == "ragged":  # point 8 has no observation; point 21 one: it cannot be triangulated, but it can be refined
        assert info["status"][7] == "degenerate"
        assert info["status"][20] == ("degenerate" if init else "converged")
        if not init:
            assert info["cost_after"][20] < info["cost_before"][20]


def _terms(ba, p, what):
    """(keywords of refine_points, keywords of the reference) of one optional term"""
    n, nobs = p["npnts"], p["nobs"]
    rng = np.random.default_rng(17)
    # (under a robust loss the first-order step converges linearly: the default 50 trials leave some points at MAX_ITER, where the
    # state would hang on the last bits; 1000 let every point converge -- the reference needs up to 151)
    if what in ("huber", "cauchy"):
        return dict(loss=what, f_scale=0.5, max_iter=1000), dict(loss=what, c=0.5, max_iter=1000)
    if what == "sigma":
        s = rng.uniform(0.5, 3.0, nobs)
        info = np.zeros((nobs, 2, 2))
        info[:, 0, 0] = info[:, 1, 1] = 1.0 / s ** 2
        return dict(obs_info=s), dict(info=info)
    if what == "info":  # full 2 x 2 blocks, some rank one, some exactly 0 (every point keeps two full-rank observations)
        info = random_info(p, 5)
        assert (np.abs(info).reshape(nobs, -1).max(axis=1) == 0).any()
        return dict(obs_info=info), dict(info=info)
    if what == "info_huber":
        info = random_info(p, 5)
        return dict(obs_info=info, loss="huber", f_scale=1.0, max_iter=1000), dict(info=info, loss="huber", c=1.0, max_iter=1000)
    if what == "prior":
        idx = np.array([2, 9, 30]) if n > 30 else np.array([0])
        mu = pts(p, p["x_true"])[idx] + rng.normal(0, 0.01, (len(idx), 3))
        A = rng.normal(0, 1, (len(idx), 3, 3))
        Lam = 4e4 * np.einsum("kij,klj->kil", A, A)
        Lam = 0.5 * (Lam + Lam.transpose(0, 2, 1))
        return dict(point_priors=(idx + 1, mu, Lam)), dict(prior=(idx, mu, Lam))
    if what == "fixed":
        fx = np.zeros(n, dtype=bool)
        fx[::7] = True
        return dict(fixed_points=fx), dict(fixed=fx)
    raise ValueError(what)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["huber", "cauchy", "sigma", "info", "info_huber", "prior", "fixed"])
@pytest.mark.parametrize("name", ["small", "high"])
def test_parity_under_terms(ba, gpu_ok, name, what):
    p = scene(ba, name)
    dev_kw, ref_kw = _terms(ba, p, what)
    if what in ("huber", "cauchy"):  # some weights are below 1 at the reference's solution
        x_ref = ref(ba, name, what, **dict(ref_kw))[0]
        w = pr.evaluate(pr.Scene(p, x_ref), pts(p, x_ref), ref_kw["loss"], ref_kw["c"])[6]
        assert (w < 1).any()
    for init in (0, 1):
        x, info = _check_parity(ba, name, what, dev_kw, ref_kw, init)
        if what == "fixed":
            fx = ref_kw["fixed"]
            assert (info["status"][fx] == "fixed").all() and not (info["status"][~fx] == "fixed").any()
            assert np.array_equal(pts(p, x)[fx].view(np.int64), pts(p, p["x0"])[fx].view(np.int64))


# Independent of the restatement: the point part of lm_step's J'r (the gradient the LM kernels compute) with every camera fixed,
# per point over sqrt(trace H_i).  Bound: 10 x the reference's own maximum at its xtol = 1e-10 result, measured on the CPU through
# the oracle's Jacobian: small_prob linear 7.9e-9, small_prob huber with 2 x 2 information 5.8e-8, the high-degree scene 1.9e-9.
_GRAD_LEVEL = {("small", "linear"): 7.9e-9, ("small", "info_huber"): 5.8e-8, ("high", "linear"): 1.9e-9}


@pytest.mark.gpu
@pytest.mark.parametrize("name,what", list(_GRAD_LEVEL))
def test_gradient_of_the_lm_kernels_vanishes(ba, gpu_ok, name, what):
    p = scene(ba, name)
    dev_kw, ref_kw = ({}, {}) if what == "linear" else _terms(ba, p, what)
    m = _model(ba, p)
    try:
        x, info = ba.refine_points(m, p["x0"], xtol=XTOL, **dev_kw)
        step_kw = {k: v for k, v in dev_kw.items() if k != "max_iter"}
        _, _, jtr = ba.lm_step(m, x, 3.0, fixed_cameras=np.arange(1, p["ncams"] + 1), **step_kw)
    finally:
        m.close()
    H = pr.evaluate(pr.Scene(p, x, ref_kw.get("info")), pts(p, x), ref_kw.get("loss", "linear"), ref_kw.get("c", 1.0))[1]
    ratio = np.linalg.norm(pts(p, jtr), axis=1) / np.sqrt(H[:, 0] + H[:, 2] + H[:, 5])
    print(f"{name} {what}: max |g_i| / sqrt(trace H_i) = {ratio.max():.3e} (reference {_GRAD_LEVEL[(name, what)]:.1e})")
    assert np.all(jtr[3 * p["npnts"]:] == 0) and ratio.max() <= 10 * _GRAD_LEVEL[(name, what)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "high"])
def test_noise_free_triangulation_recovers_the_points(ba, gpu_ok, name):
    """1e-10 relative: 250 x the reference's own 4e-13; a refinement from there moves the points by less than that"""
    p = noise_free(ba, scene(ba, name))
    m = _model(ba, p)
    try:
        x = p["x_true"].copy()
        x[:3 * p["npnts"]] = np.nan  # (the points of x are not read)
        xt, info = ba.refine_points(m, x, triangulate=True, max_iter=0)
        xr, info_r = ba.refine_points(m, xt)
    finally:
        m.close()
    Xt = pts(p, p["x_true"])
    err = np.max(np.linalg.norm(pts(p, xt) - Xt, axis=1) / np.linalg.norm(Xt, axis=1))
    move = np.max(np.linalg.norm(pts(p, xr) - pts(p, xt), axis=1) / np.linalg.norm(Xt, axis=1))
    print(f"{name}: triangulation error {err:.3e}, refinement moves it by {move:.3e}")
    assert err <= 1e-10 and move <= 1e-10
    assert (info["status"] == "max_iter").all() and not info["behind"].any() and info["iters_max"] == 0
    assert np.array_equal(xt[3 * p["npnts"]:].view(np.int64), p["x_true"][3 * p["npnts"]:].view(np.int64))


@pytest.mark.gpu
def test_against_the_fixed_camera_lm_solve(ba, gpu_ok, small_prob):
    """The old way: Levenberg_Marquardt with every camera fixed, run to tight tolerances, lands on the same points (1e-6
    relative); its one global stopping test is looser than a per-point one, so the objectives are compared too."""
    p = small_prob
    m = _model(ba, p)
    try:
        st = solve(ba, m, fixed_cameras=np.arange(1, p["ncams"] + 1), ite_max=200, oatol=0.0, ortol=0.0, atol=0.0, rtol=1e-12)
        x, info = ba.refine_points(m, p["x0"])
    finally:
        m.close()
    err = np.max(np.linalg.norm(pts(p, x) - pts(p, st.solution), axis=1) / np.linalg.norm(pts(p, x), axis=1))
    total = float(np.sum(info["cost_after"]))
    print(f"LM: {st.iter} iterations, status {st.status}, objective {st.objective!r}; refine_points {total!r}; points differ by {err:.3e}")
    assert err <= 1e-6
    assert total <= st.objective * (1 + 1e-12)


@pytest.mark.gpu
def test_unsorted_observations(ba, gpu_ok, small_prob):
    """The observations permuted at random: pt_obs keeps a point's observations in the caller's order, which the permutation
    changes, so the per-point sums run in another order: compared to 100 xtol, not bit for bit."""
    p = small_prob
    perm = np.random.default_rng(3).permutation(p["nobs"])
    q = dict(p, cam_idx1=p["cam_idx1"][perm], pnt_idx1=p["pnt_idx1"][perm],
             pt2d=np.ascontiguousarray(p["pt2d"].reshape(-1, 2)[perm].ravel()))
    out = []
    for prob in (p, q):
        m = _model(ba, prob)
        try:
            out.append(ba.refine_points(m, p["x0"], xtol=XTOL))
        finally:
            m.close()
    err = rel(p, out[1][0], out[0][0]).max()
    print(f"sorted against permuted observations: {err:.3e}")
    assert err <= 100 * XTOL and np.array_equal(out[0][1]["status"], out[1][1]["status"])


@pytest.mark.gpu
def test_max_iter_zero_evaluates_only(ba, gpu_ok, small_prob):
    p = small_prob
    n = p["npnts"]
    m = _model(ba, p)
    try:
        x, info = ba.refine_points(m, p["x0"], max_iter=0)
        r = m.cons(p["x0"])
        info3 = random_info(p, 5)
        _, info_t = ba.refine_points(m, p["x0"], max_iter=0, loss="cauchy", f_scale=0.7, obs_info=info3)
        _, f_t = m.robust_weights(p["x0"], "cauchy", 0.7, obs_info=info3)
    finally:
        m.close()
    assert np.array_equal(x.view(np.int64), p["x0"].view(np.int64))
    assert np.array_equal(info["cost_before"], info["cost_after"]) and info["iters_max"] == 0
    assert (info["status"] == "max_iter").all() and info["counts"]["max_iter"] == n
    per_point = 0.5 * np.bincount(p["pnt_idx1"] - 1, weights=r[0::2] ** 2 + r[1::2] ** 2, minlength=n)
    err = np.max(np.abs(info["cost_before"] - per_point) / per_point)
    tot = abs(np.sum(info_t["cost_before"]) - f_t) / f_t
    print(f"cost_before against 1/2 |r_i|^2: {err:.3e}; sum under cauchy and information against ba_robust_eval: {tot:.3e}")
    # 1e-13: a point's sum has at most 12 terms of like sign; 1e-12 for the 1800-term totals (two summation orders)
    assert err <= 1e-13 and tot <= 1e-12


@pytest.mark.gpu
def test_behind_flag(ba, gpu_ok, small_prob):
    """Point 5 mirrored through the centre of its first camera, X <- c + 2 (c - X): flagged, and no other point is."""
    p = small_prob
    n = p["npnts"]
    x = p["x0"].copy()
    cam = p["cam_idx1"][np.flatnonzero(p["pnt_idx1"] == 5)[0]] - 1
    C9 = x[3 * n + 9 * cam:3 * n + 9 * cam + 9]
    c = -pr.rotations(C9[None])[0].T @ C9[3:6]
    x[12:15] = c + 2.0 * (c - x[12:15])
    m = _model(ba, p)
    try:
        xo, info = ba.refine_points(m, x, max_iter=0)
    finally:
        m.close()
    assert info["behind"][4] and info["behind"].sum() == 1 and info["counts"]["behind"] == 1
    assert np.array_equal(xo.view(np.int64), x.view(np.int64))


@pytest.mark.gpu
def test_nonfinite_point_is_left(ba, gpu_ok, small_prob):
    p = small_prob
    x = p["x0"].copy()
    x[30] = np.nan
    m = _model(ba, p)
    try:
        xo, info = ba.refine_points(m, x)
    finally:
        m.close()
    assert info["status"][10] == "nonfinite" and info["counts"]["nonfinite"] == 1 and not info["behind"][10]
    assert np.array_equal(pts(p, xo)[10].view(np.int64), pts(p, x)[10].view(np.int64))
    assert (np.delete(info["status"], 10) == "converged").all()


@pytest.mark.gpu
def test_bit_guarantees(ba, gpu_ok, small_prob):
    """Two calls, and the host and the device-resident entry, give the same bits; the cameras come back untouched; an lm_step
    after a refinement gives the bits of one without it."""
    p = small_prob
    n, nvar = p["npnts"], len(p["x0"])
    L = ba._lib.lib()
    m, plain = _model(ba, p), _model(ba, p)
    try:
        ref_step = ba.lm_step(plain, p["x0"], 3.0)
        first = ba.lm_step(m, p["x0"], 3.0)
        x1, i1 = ba.refine_points(m, p["x0"], triangulate=True)
        x2, i2 = ba.refine_points(m, p["x0"], triangulate=True)
        after = ba.lm_step(m, p["x0"], 3.0)
        # the device-resident entry through ba_dev_malloc / ba_memcpy_*
        d = [C.c_void_p() for _ in range(3)]
        for ptr_, size in zip(d, (8 * nvar, n, 16 * n)):
            ba._lib.check(L.ba_dev_malloc(m.handle, size, C.byref(ptr_)))
        x3, st3, cost3 = p["x0"].copy(), np.zeros(n, dtype=np.uint8), np.zeros((n, 2))
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        ba._lib.check(L.ba_memcpy_h2d(m.handle, d[0], ba._lib.ptr(x3), 8 * nvar))
        ba._lib.check(L.ba_refine_points_dev(m.handle, d[0], 1, -1, -1.0, -1.0, d[1], d[2], ba._lib.ptr(counts), C.byref(its), None))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(x3), d[0], 8 * nvar))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(st3), d[1], n))
        ba._lib.check(L.ba_memcpy_d2h(m.handle, ba._lib.ptr(cost3), d[2], 16 * n))
        for ptr_ in d:
            ba._lib.check(L.ba_dev_free(m.handle, ptr_))
        # argument errors of the C entry
        for bad in ((2, -1.0, -1.0), (-1, -1.0, -1.0), (0, float("nan"), -1.0), (0, -1.0, float("inf"))):
            xb = p["x0"].copy()
            assert L.ba_refine_points(m.handle, ba._lib.ptr(xb), bad[0], -1, bad[1], bad[2], None, None, None, None) == 1
    finally:
        m.close()
        plain.close()
    assert np.array_equal(x1.view(np.int64), x2.view(np.int64)) and np.array_equal(x1.view(np.int64), x3.view(np.int64))
    assert np.array_equal(i1["cost_after"], i2["cost_after"]) and np.array_equal(i1["cost_after"], cost3[:, 1])
    assert np.array_equal(codes(ba, i1), st3) and its.value == i1["iters_max"] and counts[0] == i1["counts"]["converged"]
    assert np.array_equal(x1[3 * n:].view(np.int64), p["x0"][3 * n:].view(np.int64))
    assert (i1["cost_after"] <= i1["cost_before"]).all()
    for a, b, c in zip(ref_step, first, after):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(b), np.asarray(c))
