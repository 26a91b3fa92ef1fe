"""Covariance at a solution (ba_covariance, include/ba_hip.h): the cameras' 9 x 9 and the points' 3 x 3 diagonal
blocks of (J~_F'J~_F + lambda I)^-1 from the selected inversion of the factored reduced camera matrix.  References: numpy --
the inverse of the full dense J_F'J_F (small scene), the inverse of the explicit Schur complement (scenes of many tile rows).
Bound of a block's relative error: c kappa eps with kappa the condition number of the Jacobi-scaled S and c <= 100.  The first
tests need no device (the Python layer refuses bad arguments before any device call); the rest run on the GPU."""
import ctypes as C

import numpy as np
import pytest

from _lm_ref import C_BOUND, EPS, block_errs, check_cov, hessian, kappa_jacobi, ref_dense, ref_schur, schur
from _lm_run import arrays, attach_loopback, env, fixed_vector, gauge_kw, loopback_world
from _util import bits_report, parity_record

INTRINSICS = ("k1", "k2", "f")


# ---- CPU: refusals before any device call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam="x"),
                                dict(rank_tol=-1e-3), dict(rank_tol=float("nan")), dict(loss="l2"), dict(f_scale=0.0),
                                dict(fixed_points=[0]), dict(fixed_camera_params=("q",))])
def test_covariance_refuses_bad_arguments_before_any_device_call(ba, kw):
    with pytest.raises(ValueError):
        ba.covariance(None, np.zeros(3), **kw)


def test_covariance_is_exported(ba):
    assert "covariance" in ba.__all__ and callable(ba.covariance)
    assert "ba_covariance" in ba._lib.SYMBOLS


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_covariance_gauge_fixed_matches_dense_inverse(ba, orc, small_prob, gpu_ok):
    p = small_prob
    kw = gauge_kw(p)
    fixed = fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cams, pts, piv = ba.covariance(m, p["x0"], 0.0, **kw)
    finally:
        m.close()
    H = hessian(orc, p, p["x0"], 0.0, fixed)
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    assert cams.shape == (p["ncams"], 9, 9) and pts.shape == (p["npnts"], 3, 3)
    check_cov("covariance_gauge_fixed", cams, pts, ref_c, ref_p, kappa_jacobi(S), fixed, p, min_rel_pivot=piv)
    assert piv > 1e-10


@pytest.mark.gpu
def test_covariance_damped_gauge_free(ba, orc, small_prob, gpu_ok):
    p = small_prob
    lam = 10.0
    fixed = np.zeros(9 * p["ncams"] + 3 * p["npnts"], dtype=bool)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cams, pts, piv = ba.covariance(m, p["x0"], lam)
    finally:
        m.close()
    H = hessian(orc, p, p["x0"], lam, fixed)
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    check_cov("covariance_damped", cams, pts, ref_c, ref_p, kappa_jacobi(S), fixed, p, lam=lam, min_rel_pivot=piv)


@pytest.mark.gpu
def test_covariance_gauge_free_is_refused(ba, small_prob, gpu_ok):
    """lambda = 0 with the similarity gauge free: S is singular, the rank check refuses (SQDException); min D_i / S_ii sits
    far below its value with the gauge fixed"""
    p = small_prob
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        with pytest.raises(ba.SQDException) as ei:
            ba.covariance(m, p["x0"], 0.0)
        free_piv = getattr(ei.value, "min_rel_pivot", None)
        _, _, fixed_piv = ba.covariance(m, p["x0"], 0.0, cameras=False, points=False, **gauge_kw(p))
    finally:
        m.close()
    parity_record("covariance_gauge_free_refused", min_rel_pivot_free=free_piv if free_piv is not None else float("nan"),
                  min_rel_pivot_gauge_fixed=fixed_piv)
    assert "gauge" in str(ei.value)
    assert fixed_piv > 1e-10
    if free_piv is not None:  # (an exactly zero pivot is refused before the ratio exists)
        assert free_piv <= 1e-10 and free_piv < 1e-4 * fixed_piv, (free_piv, fixed_piv)


@pytest.mark.gpu
def test_covariance_huber(ba, orc, small_prob, gpu_ok):
    p = small_prob
    kw = gauge_kw(p)
    fixed = fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cams, pts, _ = ba.covariance(m, p["x0"], 0.0, loss="huber", f_scale=1.0, **kw)
    finally:
        m.close()
    H = hessian(orc, p, p["x0"], 0.0, fixed, loss="huber", c=1.0)
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    check_cov("covariance_huber", cams, pts, ref_c, ref_p, kappa_jacobi(S), fixed, p)


@pytest.mark.gpu
def test_covariance_intrinsics_and_points_fixed(ba, orc, small_prob, gpu_ok):
    p = small_prob
    rng = np.random.default_rng(3)
    kw = dict(fixed_camera_params=INTRINSICS, fixed_points=np.sort(rng.choice(p["npnts"], p["npnts"] // 5, replace=False)) + 1)
    fixed = fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cams, pts, _ = ba.covariance(m, p["x0"], 0.0, **kw)
    finally:
        m.close()
    H = hessian(orc, p, p["x0"], 0.0, fixed)
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    check_cov("covariance_intrinsics_points_fixed", cams, pts, ref_c, ref_p, kappa_jacobi(S), fixed, p)


def _scene(ba, name):
    if name == "band AMD":
        return ba.synthetic.shuffle_cameras(ba.synthetic.make_problem(300, 900, 4500, seed=5, locality=0.08), seed=2)[0], "AMD"
    if name == "band Metis":
        return ba.synthetic.shuffle_cameras(ba.synthetic.make_problem(300, 900, 4500, seed=5, locality=0.08), seed=2)[0], "Metis"
    if name == "plane":
        return ba.synthetic.make_problem(300, 900, 4500, seed=14, plane_radius=0.15), "AMD"
    return ba.synthetic.make_problem(1100, 6000, 30000, seed=35, locality=0.1), "AMD"  # two-ended (test_block_sparse_two_chains)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["band AMD", "band Metis", "plane", "two-ended"])
def test_covariance_block_sparse_equals_dense_and_schur(ba, orc, gpu_ok, name):
    """scenes of many tile rows: the list schedule (BA_SPARSE_S=1, Z on the factor's pattern only) against the dense one
    (BA_SPARSE_S=0) and the inverse of the explicit Schur complement"""
    p, perm = _scene(ba, name)
    kw = gauge_kw(p)
    lam = 1.0
    fixed = fixed_vector(ba, p, kw)

    def run():
        m = ba.BALNLPModel(arrays=arrays(p))
        try:
            ba.set_ordering(m, perm)
            out = ba.covariance(m, p["x0"], lam, **kw)
            return out, ba.schur_pattern(m), ba.schur_ordering_used(m)[1]
        finally:
            m.close()

    (cs, ps, _), pat_s, order = env("BA_SPARSE_S", "1", run)
    (cd, pd, _), pat_d, _ = env("BA_SPARSE_S", "0", run)
    assert pat_s[2] and not pat_d[2], (pat_s, pat_d)
    if name == "two-ended":
        assert order == "two-ended", order
    H = hessian(orc, p, p["x0"], lam, fixed)
    ref_c, ref_p, S, Z = ref_schur(H, p, fixed)
    kappa = kappa_jacobi(S, Z)
    check_cov(f"covariance_sparse[{name}]", cs, ps, ref_c, ref_p, kappa, fixed, p, tile_fill=pat_s[0], order=order,
           sparse_vs_dense_cam=block_errs(cs, cd), sparse_vs_dense_pnt=block_errs(ps, pd))
    check_cov(f"covariance_dense[{name}]", cd, pd, ref_c, ref_p, kappa, fixed, p)
    assert block_errs(cs, cd) <= C_BOUND * kappa * EPS and block_errs(ps, pd) <= C_BOUND * kappa * EPS


@pytest.mark.gpu
def test_covariance_same_bits_and_handle_untouched(ba, small_prob, gpu_ok):
    """two calls give the same bits; an lm_step after a covariance call gives the bits of an lm_step alone"""
    p = small_prob
    kw = gauge_kw(p)
    a = ba.BALNLPModel(arrays=arrays(p))
    b = ba.BALNLPModel(arrays=arrays(p))
    try:
        ref = ba.lm_step(a, p["x0"], 10.0)
        c1 = ba.covariance(b, p["x0"], 0.0, loss="huber", **kw)
        c2 = ba.covariance(b, p["x0"], 0.0, loss="huber", **kw)
        got = ba.lm_step(b, p["x0"], 10.0)
        again = ba.lm_step(a, p["x0"], 10.0)
    finally:
        a.close()
        b.close()
    for x, y, what in ((c1[0], c2[0], "cam_cov"), (c1[1], c2[1], "pnt_cov")):
        assert not bits_report(x, y, what), bits_report(x, y, what)
    assert c1[2] == c2[2]
    for i, what in ((0, "delta"), (2, "jtr")):
        assert not bits_report(got[i], ref[i], what), bits_report(got[i], ref[i], what)
        assert not bits_report(again[i], ref[i], what), bits_report(again[i], ref[i], what)
    assert got[1] == ref[1]


@pytest.mark.gpu
def test_covariance_refuses_a_communicator_and_bad_c_arguments(ba, small_prob, gpu_ok):
    p = small_prob
    lib = ba._lib.lib()
    m = ba.BALNLPModel(arrays=arrays(p))
    x = np.ascontiguousarray(p["x0"])
    piv = C.c_double(0)
    try:
        for lam in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ba.BAArgError, match="lambda"):
                ba._lib.check(lib.ba_covariance(m.handle, ba._lib.ptr(x), lam, -1.0, None, None, C.byref(piv)))
        with loopback_world(1, 16 << 20) as (L, loop):
            try:
                attach_loopback(ba, m, L, loop, 0, 1)
                with pytest.raises(ba.BAArgError, match="communicator"):
                    ba.covariance(m, x, 1.0)
            finally:
                m.close()
    finally:
        m.close()
