"""Shared camera intrinsics of the LM solve (ba_lm_set_shared_intrinsics, include/ba_hip.h): calibration groups whose
members share one (k1, k2, f), x = E z.  The reference is numpy (tests/_lm_ref.py): the oracle's residual and Jacobian,
the reweighting, mask and prior rows of tests/test_priors.py, E as a scipy sparse matrix, the dense solve over z and a dense LM
loop over z.  Step limit everywhere: max(tol, 100 kappa eps), the rule of tests/_lm_ref.py::limit, kappa the condition number
of the Jacobi-scaled reduced camera system over z; tol = STEP_TOL[lambda] for :LDL and PCG_TOL for pcg = (1e-12, 5000).  Model
value and gradient: the relative limits of tests/test_priors.py::test_prior_step_vs_dense_numpy (1e-10, 1e-12; the PCG step's own
model value 1e-7).  The first tests need no device; the rest run on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from _lm_ref import (PCG_TOL, STEP_TOL, bordered, centre, expansion, jac, labels, limit, lm_dense, residual, step, step_once, sym)
from _lm_run import arrays, attach_loopback, env, fixed_vector, lm_opts, loopback_world
from _util import bits_report, parity_record, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS_A = [[1, 2, 3, 4, 5], [7, 9, 11, 12]]      # scene A: (12, 400, 1800, seed 11), one tile, n = 108
GROUPS_B = [list(range(1, 41, 2)), [2, 4, 6]]      # scene B: (40, 400, 1800, seed 11), three tiles, the last one ragged
_cache = {}


def _scene(ba, which):
    """the scene with x0 tied (the members of a group hold the first member's intrinsics), and its groups"""
    if which not in _cache:
        p = dict(ba.synthetic.make_problem(12 if which == "A" else 40, 400, 1800, seed=11))
        groups = GROUPS_A if which == "A" else GROUPS_B
        p["x0"] = ba.tie_intrinsics(p["x0"], p["npnts"], groups)
        _cache[which] = (p, groups)
    return _cache[which]


def _plain(ba, orc, which, lam):
    """the step of scene `which` at x0 with its groups and no other term: shared between the tests, computed once"""
    p, groups = _scene(ba, which)
    return step_once(("shared", which, lam), orc, p, p["x0"], lam, groups=groups)


def _member_rows(p, groups):
    """(first, others): the x indices of (k1, k2, f) of every group's first member and of its other members"""
    lab = labels(groups, p["ncams"])
    np3 = 3 * p["npnts"]
    first, others = [], []
    for g in range(1, lab.max() + 1):
        mem = np.flatnonzero(lab == g)
        first.append(np3 + 9 * mem[0] + 6 + np.arange(3))
        others.append((np3 + 9 * mem[1:, None] + 6 + np.arange(3)[None, :]))
    return first, others


def _check_conventions(p, groups, d, jtr, g_full=None):
    """members' step intrinsics bit-equal; jtr exactly 0 at the non-first members and the group sum at the first"""
    first, others = _member_rows(p, groups)
    for f, o in zip(first, others):
        for row in o:
            assert not bits_report(d[row], d[f], "a member's step intrinsics vs the first member's")
        assert np.all(jtr[o] == 0.0), "gradient entries of non-first members are not exactly 0"
        if g_full is not None:
            want = g_full[f] + g_full[o].sum(axis=0)
            assert np.linalg.norm(jtr[f] - want) <= 1e-12 * np.linalg.norm(want), (jtr[f], want)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_keywords(ba):
    L = ba._lib.lib()
    header = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("ba_lm_set_shared_intrinsics", "ba_lm_get_shared_intrinsics", "ba_dense_ldl_solve_multi"):
        assert name in ba._lib.SYMBOLS and hasattr(L, name) and f"int {name}(" in header
    assert L.ba_lm_set_shared_intrinsics(None, None) == 1 and L.ba_lm_get_shared_intrinsics(None, None, None) == 1
    assert "shared_intrinsics" in ba.Levenberg_Marquardt.__kwdefaults__ and "shared_intrinsics" in ba.lm_step.__code__.co_varnames
    assert callable(ba.tie_intrinsics)


@pytest.mark.parametrize("bad", [np.array([0, -1, 1, 1]), np.array([0, 9, 9, 1]), np.array([1, 1, 3, 3]), np.array([0.5, 1.0]),
                                 [[1, 2], [2, 3]], [[0, 1]], [[1, 2], []], [[1, 2]] * 9, np.zeros((2, 2), dtype=int)])
def test_bad_groupings_refused_before_the_device(ba, bad):
    """No model exists here (None): the ValueError comes before anything looks at the model or the device."""
    with pytest.raises(ValueError, match="shared_intrinsics"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, shared_intrinsics=bad)
    with pytest.raises(ValueError, match="shared_intrinsics"):
        ba.lm_step(None, np.zeros(3), 1.0, shared_intrinsics=bad)


def test_refused_combinations_before_the_device(ba):
    g = [[1, 2]]
    with pytest.raises(ValueError, match="shared_intrinsics.*linesearch"):
        ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", True, shared_intrinsics=g)
    for ft in (np.float32, np.float16):
        with pytest.raises(ValueError, match="shared_intrinsics.*facto_type"):
            ba.Levenberg_Marquardt(None, "LDL", "AMD", "None", False, facto_type=ft, shared_intrinsics=g)
    for norm in ("J", ":A"):
        with pytest.raises(ValueError, match="shared_intrinsics.*normalize"):
            ba.Levenberg_Marquardt(None, "LDL", "AMD", norm, False, shared_intrinsics=g)
    with pytest.raises(ValueError, match="shared_intrinsics.*facto_type"):
        ba.lm_step(None, np.zeros(3), 1.0, facto_type=np.float32, shared_intrinsics=g)
    assert ba._lib.check_shared(g) and not ba._lib.check_shared(None) and not ba._lib.check_shared([[3]])
    assert not ba._lib.check_shared(np.zeros(5, dtype=int)) and ba._lib.check_shared(np.array([0, 2, 1, 1, 2]))


def test_label_forms_and_tie_intrinsics(ba):
    lab = ba._lib.shared_labels([[2, 5], [3], [1, 4]], 6)
    assert lab.dtype == np.int32 and lab.tolist() == [3, 1, 2, 3, 1, 0]
    assert ba._lib.shared_labels([[3]], 6) is None and ba._lib.shared_labels(np.zeros(6, dtype=int), 6) is None
    assert ba._lib.shared_labels(None, 6) is None
    with pytest.raises(ValueError, match="shape"):
        ba._lib.shared_labels(np.zeros(5, dtype=int), 6)
    with pytest.raises(ValueError, match="1..6"):
        ba._lib.shared_labels([[1, 7]], 6)
    x = np.arange(3 * 2 + 9 * 6, dtype=float)
    t = ba.tie_intrinsics(x, 2, [[2, 5], [3], [1, 4]])
    cams, tc = x[6:].reshape(6, 9), t[6:].reshape(6, 9)
    assert np.array_equal(t[:6], x[:6]) and np.array_equal(tc[:, :6], cams[:, :6])
    assert np.array_equal(tc[4, 6:], cams[1, 6:]) and np.array_equal(tc[3, 6:], cams[0, 6:])
    assert np.array_equal(tc[[0, 1, 2, 5], 6:], cams[[0, 1, 2, 5], 6:]) and x[6 + 9 * 4 + 6] == 48.0  # (a copy: x is untouched)
    assert np.array_equal(ba.tie_intrinsics(x, 2, lab), t)


def test_make_problem_default_is_unchanged_and_groups_share(ba, small_prob):
    """intrinsics_groups=None draws exactly the arrays of the call without the keyword (no rng call on the default path: the
    grouped call draws the same points, poses and observation graph too); with groups the members share (k1, k2, f) in x_true
    and x0, and pt2d is projected from them."""
    q = ba.synthetic.make_problem(12, 400, 1800, seed=11, intrinsics_groups=None)
    for k in ("cam_idx1", "pnt_idx1", "pt2d", "x0", "x_true"):
        assert np.array_equal(q[k], small_prob[k]), k
    g = ba.synthetic.make_problem(12, 400, 1800, seed=11, intrinsics_groups=GROUPS_A)
    np3 = 3 * 400
    for k in ("x0", "x_true"):
        cams = g[k][np3:].reshape(12, 9)
        for mem in GROUPS_A:
            assert np.all(cams[np.array(mem) - 1, 6:] == cams[mem[0] - 1, 6:]), k
        assert np.array_equal(g[k][:np3], small_prob[k][:np3])
        assert np.array_equal(cams[:, :6], small_prob[k][np3:].reshape(12, 9)[:, :6])
        assert np.array_equal(cams[[5, 7, 9]], small_prob[k][np3:].reshape(12, 9)[[5, 7, 9]])  # cameras 6, 8, 10: label 0
    assert np.array_equal(g["cam_idx1"], small_prob["cam_idx1"]) and not np.array_equal(g["pt2d"], small_prob["pt2d"])
    proj = ba.synthetic.project(g["x_true"][:np3].reshape(-1, 3)[g["pnt_idx1"] - 1], g["x_true"][np3:].reshape(12, 9)[g["cam_idx1"] - 1])
    assert np.abs(g["pt2d"] - proj.ravel()).max() < 5.0  # the 0.5 px noise of the generator around the tied cameras' projection


@pytest.mark.parametrize("which", ["A", "B"])
def test_reference_bordered_solve_agrees_with_dense_z(ba, orc, which):
    """_lm_ref.bordered -- the algebra the device runs -- against _lm_ref.step's dense solve over z, camera part of the
    step, at every lambda of STEP_TOL, within max(STEP_TOL[lambda], 100 kappa eps)"""
    p, groups = _scene(ba, which)
    np3 = 3 * p["npnts"]
    for lam, tol in STEP_TOL.items():
        ref = _plain(ba, orc, which, lam)
        a = bordered(ref["H"], ref["g"], lam, groups, p["ncams"], p["npnts"])
        e, lim = rel_err(a, ref["delta"][np3:]), limit(tol, ref["kappa"])
        print(f"bordered[{which}] lambda {lam:g}: kappa {ref['kappa']:.3e}  error {e:.3e} (limit {lim:.1e})")
        assert e <= lim


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["A", "B"])
def test_shared_step_vs_dense_numpy(ba, orc, gpu_ok, which):
    p, groups = _scene(ba, which)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            ref = _plain(ba, orc, which, lam)
            d, half, jtr = ba.lm_step(m, p["x0"], lam, shared_intrinsics=groups)
            dp, halfp, jtrp, its = ba.lm_step(m, p["x0"], lam, pcg=(1e-12, 5000), shared_intrinsics=groups)
            e, ep = rel_err(d, ref["delta"]), rel_err(dp, ref["delta"])
            em = abs(half - ref["model"]) / ref["model"]
            eg = float(np.linalg.norm(jtr - ref["grad"]) / np.linalg.norm(ref["grad"]))
            lim, limp = limit(tol, ref["kappa"]), limit(PCG_TOL, ref["kappa"])
            print(f"shared_step[{which}] lambda {lam:g}: kappa {ref['kappa']:.3e}  LDL {e:.3e} (limit {lim:.1e})  pcg {ep:.3e} "
                  f"({limp:.1e}, {its} its)  model {em:.3e}  jtr {eg:.3e}")
            parity_record(f"shared_step[{which}-{lam:g}]", kappa=ref["kappa"], ldl=e, ldl_limit=lim, pcg=ep, pcg_limit=limp, model=em,
                          jtr=eg, cg_iters=its)
            assert e <= lim, f"{which}, lambda {lam}: :LDL step {e:.3e} > {lim:.3e}"
            assert ep <= limp, f"{which}, lambda {lam}: PCG step {ep:.3e} > {limp:.3e}"
            assert em <= 1e-10, f"{which}, lambda {lam}: model value {half!r} vs {ref['model']!r}"
            assert abs(halfp - ref["model"]) <= 1e-7 * ref["model"]
            assert eg <= 1e-12, f"{which}, lambda {lam}: gradient {eg:.3e}"
            assert not bits_report(jtrp, jtr, "the gradient of the PCG entry vs the direct entry")
            _check_conventions(p, groups, d, jtr, ref["g"])
            _check_conventions(p, groups, dp, jtrp, ref["g"])
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", [1, 4, 25])
def test_dense_ldl_solve_multi_vs_numpy(ba, gpu_ok, nrhs):
    """n = 300 (three tiles, the last ragged).  Per column the bound of test_dense_ldl_vs_numpy; the nrhs = 1 column equals
    ba_dense_ldl_solve on the same input to that bound."""
    n = 300
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 8))
    A = G @ G.T + 0.5 * np.eye(n)
    B = rng.standard_normal((n, nrhs))
    X, _ = ba._lib.dense_ldl_solve_multi(A, B)
    ref = np.linalg.solve(A, B)
    bound = 1e-10 * np.linalg.cond(A) ** 0.5  # the bound of tests/test_gpu_parity.py::test_dense_ldl_vs_numpy
    for c in range(nrhs):
        err = np.linalg.norm(X[:, c] - ref[:, c]) / np.linalg.norm(ref[:, c])
        print(f"dense_ldl_solve_multi[{nrhs}] column {c}: {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (c, err)
    if nrhs == 1:
        x1, _ = ba._lib.dense_ldl_solve(A, B[:, 0])
        assert np.linalg.norm(X[:, 0] - x1) <= bound * np.linalg.norm(x1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128, 129, 300])
def test_dense_ldl_solve_multi_columns_are_independent(ba, gpu_ok, n):
    """One tile; two tiles, the second almost all padding; three with a ragged last.  Column c of the solve with four
    right-hand sides has the bits of the solve with column c alone: one workgroup per (tile, column), the column picked by
    the grid's y index and the stride, no atomics."""
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 8))
    A = G @ G.T + 0.5 * np.eye(n)
    B = rng.standard_normal((n, 4))
    X, _ = ba._lib.dense_ldl_solve_multi(A, B)
    assert np.all(np.isfinite(X)) and np.linalg.norm(A @ X - B) <= 1e-8 * np.linalg.norm(B)
    for c in range(4):
        x, _ = ba._lib.dense_ldl_solve_multi(A, B[:, c:c + 1])
        assert not bits_report(X[:, c], x[:, 0], f"n = {n}: column {c} of four vs alone")


@pytest.mark.gpu
def test_dense_ldl_solve_multi_zero_pivot(ba, gpu_ok):
    """The zero matrix: the exception of ba_dense_ldl_solve on it, type and message; a good matrix afterwards solves."""
    Z = np.zeros((4, 4))
    with pytest.raises(ba.SQDException) as single:
        ba._lib.dense_ldl_solve(Z, np.ones(4))
    with pytest.raises(ba.SQDException) as multi:
        ba._lib.dense_ldl_solve_multi(Z, np.ones((4, 1)))
    assert type(multi.value) is type(single.value) and str(multi.value) == str(single.value)
    assert "zero pivot" in str(multi.value)
    X, _ = ba._lib.dense_ldl_solve_multi(np.diag([1.0, 2.0, 4.0, 8.0]), np.ones((4, 1)))
    assert np.array_equal(X[:, 0], [1.0, 0.5, 0.25, 0.125])


@pytest.mark.gpu
def test_no_grouping_paths_give_the_plain_bits(ba, gpu_ok):
    """all labels 0, None and groups of one camera run the plain path: delta, model and jtr bit-identical to the call without
    the keyword; after a shared step and a clear the plain bits are back, for the direct and the PCG entry"""
    p, groups = _scene(ba, "A")
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for kw in ({}, {"pcg": (1e-10, 200)}):
            plain = ba.lm_step(m, p["x0"], 1.0, **kw)
            for none in (np.zeros(p["ncams"], dtype=int), None, [[3], [7]], np.array([1, 0, 2, 0, 0, 0, 3, 0, 0, 0, 0, 0])):
                got = ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=none, **kw)
                assert ba._lib.get_shared(m.handle) == (0, 0)
                for a, b, name in zip(got[:3], plain[:3], ("delta", "model", "jtr")):
                    assert not bits_report(np.atleast_1d(a), np.atleast_1d(b), f"{name} with shared_intrinsics={none!r}")
            shared = ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=groups, **kw)
            assert ba._lib.get_shared(m.handle) == (2, 9)
            assert rel_err(shared[0], plain[0]) > 1e-6
            again = ba.lm_step(m, p["x0"], 1.0, **kw)
            assert ba._lib.get_shared(m.handle) == (0, 0)
            for a, b, name in zip(again[:3], plain[:3], ("delta", "model", "jtr")):
                assert not bits_report(np.atleast_1d(a), np.atleast_1d(b), f"{name} after a shared step and a clear")
    finally:
        m.close()


@pytest.mark.gpu
def test_c_abi_label_checks(ba, gpu_ok):
    p, _ = _scene(ba, "A")
    L = ba._lib.lib()
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lab, text in (([0, -1] + [0] * 10, "must be 0"), ([9, 9] + [0] * 10, "must be 0"), ([1, 1, 3, 3] + [0] * 8, "gap")):
            a = np.array(lab, dtype=np.int32)
            assert L.ba_lm_set_shared_intrinsics(m.handle, ba._lib.ptr(a)) == 1
            assert text in L.ba_last_error().decode()
        a = np.array([2, 2, 1, 0, 3, 3, 3] + [0] * 5, dtype=np.int32)  # group 1 has one member: dropped
        assert L.ba_lm_set_shared_intrinsics(m.handle, ba._lib.ptr(a)) == 0 and ba._lib.get_shared(m.handle) == (2, 5)
        assert L.ba_lm_set_shared_intrinsics(m.handle, None) == 0 and ba._lib.get_shared(m.handle) == (0, 0)
    finally:
        m.close()


@pytest.mark.gpu
def test_shared_step_with_fixed_intrinsics(ba, orc, gpu_ok):
    """One group of all cameras with (k1, k2, f) fixed: the fixed step without sharing, within the limit.  Disagreeing mask
    bits inside a group: an error that names the camera."""
    p, _ = _scene(ba, "A")
    every = [list(range(1, p["ncams"] + 1))]
    x = ba.tie_intrinsics(p["x0"], p["npnts"], every)
    mask = dict(fixed_camera_params=("k1", "k2", "f"))
    fixed = fixed_vector(ba, p, mask)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            ref = step(orc, p, x, lam, groups=every, fixed=fixed)
            unshared = ba.lm_step(m, x, lam, **mask)
            for kw, t in (({}, tol), ({"pcg": (1e-12, 5000)}, PCG_TOL)):
                d, half, jtr = ba.lm_step(m, x, lam, shared_intrinsics=every, **mask, **kw)[:3]
                lim = limit(t, ref["kappa"])
                e, e_ref = rel_err(d, unshared[0]), rel_err(d, ref["delta"])
                print(f"shared_fixed lambda {lam:g} {'pcg' if kw else 'LDL'}: vs unshared {e:.3e}, vs numpy {e_ref:.3e} (limit {lim:.1e})")
                assert e <= lim and e_ref <= lim
                assert np.all(d[fixed] == 0.0) and np.all(jtr[fixed] == 0.0)
                assert abs(half - unshared[1]) <= (1e-10 if not kw else 1e-7) * unshared[1]
        comp = np.zeros((p["ncams"], 9), dtype=bool)
        comp[3, 8] = True  # f of camera 4 only, a member of the group
        for kw in ({}, {"pcg": (1e-8, 100)}):
            with pytest.raises(ValueError, match="camera 4 "):
                ba.lm_step(m, x, 1.0, shared_intrinsics=every, fixed_camera_params=comp, **kw)
        with pytest.raises(ValueError, match="camera 4 "):
            ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, x=x, shared_intrinsics=every,
                                   fixed_camera_params=comp)
    finally:
        m.close()


@pytest.mark.gpu
def test_shared_step_with_huber(ba, orc, gpu_ok):
    p, groups = _scene(ba, "A")
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            ref = step(orc, p, p["x0"], lam, groups=groups, loss="huber", c=1.0)
            d, half, jtr = ba.lm_step(m, p["x0"], lam, loss="huber", f_scale=1.0, shared_intrinsics=groups)
            e, lim = rel_err(d, ref["delta"]), limit(tol, ref["kappa"])
            em = abs(half - ref["model"]) / ref["model"]
            eg = float(np.linalg.norm(jtr - ref["grad"]) / np.linalg.norm(ref["grad"]))
            print(f"shared_huber lambda {lam:g}: kappa {ref['kappa']:.3e}  step {e:.3e} (limit {lim:.1e})  model {em:.3e}  jtr {eg:.3e}")
            parity_record(f"shared_huber[{lam:g}]", kappa=ref["kappa"], ldl=e, ldl_limit=lim, model=em, jtr=eg)
            assert e <= lim and em <= 1e-10 and eg <= 1e-12
            _check_conventions(p, groups, d, jtr, ref["g"])
        assert rel_err(d, _plain(ba, orc, "A", 1e-2)["delta"]) > 1e-6  # (not the linear step)
    finally:
        m.close()


@pytest.mark.gpu
def test_shared_step_with_priors(ba, orc, gpu_ok):
    """Scene B: a camera prior with a full 9 x 9 block on camera 7, a non-first member of group 1 (a calibration prior on one
    member is a prior on the group), plus two centre priors; :LDL and PCG against the reference"""
    p, groups = _scene(ba, "B")
    rng = np.random.default_rng(9)
    np3 = 3 * p["npnts"]
    cams = p["x_true"][np3:].reshape(-1, 9)
    Bm = rng.standard_normal((9, 9))
    scale = np.maximum(np.abs(cams[6]), 1e-3)
    info = sym((Bm @ Bm.T + 9 * np.eye(9)) / (0.01 * scale[:, None] * 0.01 * scale[None, :]))
    cidx = np.array([12, 31])
    pri = dict(camera_priors=(np.array([7]), cams[6][None] * (1 + 1e-3), info[None]),
               centre_priors=(cidx, np.stack([centre(cams[i - 1]) for i in cidx]) + 0.01, np.full((2, 3), 0.01)))
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for lam, tol in STEP_TOL.items():
            ref = step(orc, p, p["x0"], lam, groups=groups, priors=pri)
            d, half, jtr = ba.lm_step(m, p["x0"], lam, shared_intrinsics=groups, **pri)
            dp, halfp, jtrp, its = ba.lm_step(m, p["x0"], lam, pcg=(1e-12, 5000), shared_intrinsics=groups, **pri)
            e, ep = rel_err(d, ref["delta"]), rel_err(dp, ref["delta"])
            em = abs(half - ref["model"]) / ref["model"]
            eg = float(np.linalg.norm(jtr - ref["grad"]) / np.linalg.norm(ref["grad"]))
            lim, limp = limit(tol, ref["kappa"]), limit(PCG_TOL, ref["kappa"])
            print(f"shared_priors lambda {lam:g}: kappa {ref['kappa']:.3e}  LDL {e:.3e} (limit {lim:.1e})  pcg {ep:.3e} ({limp:.1e}, "
                  f"{its} its)  model {em:.3e}  jtr {eg:.3e}")
            parity_record(f"shared_priors[{lam:g}]", kappa=ref["kappa"], ldl=e, ldl_limit=lim, pcg=ep, pcg_limit=limp, model=em, jtr=eg)
            assert e <= lim and ep <= limp and em <= 1e-10 and eg <= 1e-12
            assert abs(halfp - ref["model"]) <= 1e-7 * ref["model"]
            _check_conventions(p, groups, d, jtr, ref["g"])
    finally:
        m.close()


@pytest.mark.gpu
def test_shared_step_block_sparse_schedule(ba, orc, gpu_ok):
    """The scene of tests/test_priors.py::test_prior_step_block_sparse_schedule with its cameras shuffled (the ordering has
    work to do) and three groups of 40 scattered cameras: BA_SPARSE_S=1 (list schedule, compressed tiles) and =0 (dense) both
    give numpy's step within the limit"""
    p, _ = ba.synthetic.shuffle_cameras(ba.synthetic.make_problem(300, 700, 3500, seed=5, locality=0.08), seed=1)
    pick = np.random.default_rng(2).permutation(300)[:120] + 1
    groups = [sorted(pick[:40].tolist()), sorted(pick[40:80].tolist()), sorted(pick[80:].tolist())]
    p = dict(p)
    p["x0"] = ba.tie_intrinsics(p["x0"], p["npnts"], groups)
    lam = 1.0
    ref = step(orc, p, p["x0"], lam, groups=groups)
    lim = limit(STEP_TOL[lam], ref["kappa"])
    for flag in ("1", "0"):
        def run():
            m = ba.BALNLPModel(arrays=arrays(p))
            try:
                return ba.lm_step(m, p["x0"], lam, shared_intrinsics=groups), ba.schur_pattern(m), ba.schur_ordering_used(m)[1]
            finally:
                m.close()

        (d, half, jtr), pat, order = env("BA_SPARSE_S", flag, run)
        assert pat[2] == (flag == "1"), "the schedule asked for was not used"
        e = rel_err(d, ref["delta"])
        print(f"shared_step_sparse[BA_SPARSE_S={flag}]: ordering {order}, kappa {ref['kappa']:.3e}  step {e:.3e} (limit {lim:.1e})")
        parity_record(f"shared_step_sparse[{flag}]", kappa=ref["kappa"], step=e, limit=lim)
        assert e <= lim
        assert abs(half - ref["model"]) <= 1e-10 * ref["model"]
        assert np.linalg.norm(jtr - ref["grad"]) <= 1e-12 * np.linalg.norm(ref["grad"])
        _check_conventions(p, groups, d, jtr, ref["g"])


def _fun(orc, p):
    def f(x):
        r, J = residual(orc, p, x), jac(orc, p, x).toarray()
        return 0.5 * (r @ r), J.T @ r, J.T @ J, lambda d: 0.5 * np.sum((J @ d + r) ** 2)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("variant,facto", [(1, "LDL"), (0, "LDL"), (1, "PCG"), (0, "PCG")])
def test_shared_solve(ba, orc, gpu_ok, variant, facto):
    """Scene A from the tied x0, oatol = ortol = 0: status and iteration count of _lm_ref.lm_dense (the dense loop over z
    with this variant's controller); objective and dual_feas against numpy at the returned x with the limits of
    tests/test_priors.py::test_prior_solve (1e-12, 1e-10), dual_feas being |E'g|; members bit-equal in the solution"""
    p, groups = _scene(ba, "A")
    key = ("solve", variant)
    if key not in _cache:
        _cache[key] = lm_dense(_fun(orc, p), p["x0"], groups=groups, ncams=p["ncams"], npnts=p["npnts"], variant=variant)
    x_ref, status_ref, it_ref, f_loop, g_loop = _cache[key]
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        args = (facto, "AMD", "None") + ((False,) if variant == 1 else ())
        kw = dict(pcg_tol=1e-13) if facto == "PCG" else {}
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), *args, oatol=0.0, ortol=0.0, shared_intrinsics=groups, **kw)
    finally:
        m.close()
    E, keep = expansion(groups, p["ncams"], p["npnts"])
    f, g, _, _ = _fun(orc, p)(st.solution)
    g_ref = float(np.linalg.norm(E.T @ g))
    feas = st.dual_feas if variant == 1 else st.primal_feas
    ef, eg = abs(st.objective - f) / f, abs(feas - g_ref) / g_ref
    print(f"shared_solve[{variant}-{facto}]: {st.status} after {st.iter} (numpy loop: {status_ref} after {it_ref}), objective {ef:.3e} "
          f"(vs the loop's {abs(st.objective - f_loop) / f_loop:.3e}), |E'g| {eg:.3e}, solution vs the loop's {rel_err(st.solution, x_ref):.3e}")
    parity_record(f"shared_solve[{variant}-{facto}]", objective=ef, dual_feas=eg, iter=st.iter, iter_ref=it_ref, status=st.status)
    assert (st.status, st.iter) == (status_ref, it_ref)
    assert ef <= 1e-12, f"objective {st.objective!r} vs numpy {f!r}"
    assert eg <= 1e-10, f"|E'g| {feas!r} vs numpy {g_ref!r}"
    assert not bits_report(ba.tie_intrinsics(st.solution, p["npnts"], groups), st.solution, "members of a group in the solution")
    assert f < 0.5 * np.sum(residual(orc, p, p["x0"]) ** 2)


@pytest.mark.gpu
def test_untied_x_is_refused(ba, gpu_ok):
    p, groups = _scene(ba, "A")
    x = np.array(p["x0"])
    x[3 * p["npnts"] + 9 * 8 + 7] *= 1 + 1e-15  # k2 of camera 9, a member of group 2
    lib = ba._lib.lib()
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        with pytest.raises(ValueError, match="camera 9 "):
            ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, x=x, shared_intrinsics=groups)
        with pytest.raises(ValueError, match="camera 9 "):
            ba.lm_step(m, x, 1.0, shared_intrinsics=groups)
        ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=groups)  # the grouping is on the handle now: the library itself
        d, half = np.empty_like(x), C.c_double(0)
        assert lib.ba_lm_step(m.handle, ba._lib.ptr(x), 1.0, ba._lib.ptr(d), C.byref(half), None) == 1
        assert "camera 9 " in lib.ba_last_error().decode()
        o = lm_opts(ba)
        st = ba._lib.LMStats()
        assert lib.ba_lm_solve(m.handle, C.byref(o), ba._lib.ptr(x), C.byref(st), C.cast(None, ba._lib.LOG_CB), None) == 1
        assert "camera 9 " in lib.ba_last_error().decode()
    finally:
        m.close()


@pytest.mark.gpu
def test_refused_combinations_on_the_device(ba, gpu_ok):
    """a communicator, facto_type Float32 / Float16, x_f32, normalize :J / :A, linesearch = 1 and ba_covariance: ValueError /
    BA_ERR_ARG, the message naming the combination; the handle steps as before afterwards"""
    p, groups = _scene(ba, "A")
    lib = ba._lib.lib()
    m = ba.BALNLPModel(arrays=arrays(p))
    m32 = ba.BALNLPModel(arrays=arrays(p), T=np.float32)
    try:
        before = ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=groups)
        with pytest.raises(ValueError, match="shared_intrinsics.*Float32 model"):
            ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), "LDL", "AMD", "None", False, shared_intrinsics=groups)
        assert ba._lib.get_shared(m.handle) == (2, 9)  # on the handle from the step above: the library itself
        x = np.array(p["x0"])
        for kw, text in ((dict(linesearch=1), "linesearch = true"), (dict(x_f32=1), "Float32 model"), (dict(facto_type=1), "facto_type"),
                         (dict(facto_type=2), "facto_type"), (dict(normalize=1), "normalize"), (dict(normalize=2), "normalize")):
            st = ba._lib.LMStats()
            o = lm_opts(ba, **kw)
            rc = lib.ba_lm_solve(m.handle, C.byref(o), ba._lib.ptr(x), C.byref(st), C.cast(None, ba._lib.LOG_CB), None)
            msg = lib.ba_last_error().decode()
            assert rc == 1 and "shared intrinsics" in msg and text in msg, (kw, rc, msg)
        d, half = np.empty_like(x), C.c_double(0)
        assert lib.ba_lm_step_f32(m.handle, ba._lib.ptr(x), 1.0, ba._lib.ptr(d), C.byref(half), None) == 1
        assert "shared intrinsics" in lib.ba_last_error().decode() and "Float32" in lib.ba_last_error().decode()
        with pytest.raises(ValueError, match="ba_covariance.*shared intrinsics"):
            ba._lib.check(lib.ba_covariance(m.handle, ba._lib.ptr(x), 1.0, -1.0, None, None, None))
        assert np.array_equal(x, p["x0"])
        after = ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=groups)
        assert not bits_report(after[0], before[0], "step after the refusals")
        with pytest.raises(ValueError, match="ba_covariance.*shared intrinsics"):  # (the grouping is still on the handle)
            ba.covariance(m, p["x0"], 1.0)
        ba.lm_step(m, p["x0"], 1.0)  # a call without the keyword clears it
        assert ba.covariance(m, p["x0"], 1.0, points=False)[0].shape == (p["ncams"], 9, 9)
    finally:
        m.close()
        m32.close()
    # a communicator (attached before the handle's first solve, as documented)
    mc = ba.BALNLPModel(arrays=arrays(p))
    with loopback_world(1, 16 << 20) as (L, loop):
        try:
            attach_loopback(ba, mc, L, loop, 0, 1)
            with pytest.raises(ba.BAArgError, match="shared intrinsics.*communicator"):
                ba.lm_step(mc, p["x0"], 1.0, shared_intrinsics=groups)
            with pytest.raises(ba.BAArgError, match="shared intrinsics.*communicator"):
                ba.lm_step(mc, p["x0"], 1.0, pcg=(1e-8, 100), shared_intrinsics=groups)
            with pytest.raises(ba.BAArgError, match="shared intrinsics.*communicator"):
                ba.Levenberg_Marquardt(ba.FeasibilityResidual(mc), "LDL", "AMD", "None", False, shared_intrinsics=groups)
            plain = ba.lm_step(mc, p["x0"], 1.0)
            assert np.all(np.isfinite(plain[0]))
        finally:
            mc.close()


@pytest.mark.gpu
def test_two_shared_steps_give_identical_bits(ba, gpu_ok):
    p, groups = _scene(ba, "B")
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        for kw in ({}, {"pcg": (1e-10, 500)}):
            a = ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=groups, **kw)
            b = ba.lm_step(m, p["x0"], 1.0, shared_intrinsics=groups, **kw)
            for u, v, name in zip(a[:3], b[:3], ("delta", "model", "jtr")):
                assert not bits_report(np.atleast_1d(u), np.atleast_1d(v), f"{name} of two shared steps")
    finally:
        m.close()
