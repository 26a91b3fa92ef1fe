"""Parity of the HIP path (through the C ABI) with the CPU oracle.  Needs an MI355X: run with -m gpu.
Tolerances (stated, fp64):
  * Jacobian pattern: bit-exact int64.
  * residuals: |r_gpu - r_oracle| <= eps * (8 |proj| + f / 2), f the camera's focal length: rounding differences in
    P1 (device sin/cos/sqrt/div differ from libm in the last bits) are amplified by f / |z| into pixels, so the error
    scale of a small coordinate is f, not the coordinate itself.  The reference's own fixture, test/runtests.jl:27, is
    matched to that bound, not to 0.
  * Jacobian values: <= 1e-12 relative to the inf-norm of the 2x12 block.
  * J'r: <= 1e-12 relative to max|J'r| (different, but fixed, summation order).
  * one LM step from identical (x, lambda): |delta - delta_ref| / |delta_ref| <= 1e-9 for lambda >= 1e-2 on the
    synthetic shapes; 1/2|J delta + r|^2 to 1e-9 relative.
  * LM run: identical accept/reject sequence and iteration count on the small shapes, final objective <= 1e-8 relative.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from _util import parity_record as _report  # noqa: E402
from lm_rows import _TIGHT, _compare_rows, _float32_rows, _hard_start, _test_name, _well_conditioned_prefix  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
RES_ULPS = 4  # residuals within 4 ulp of the projected coordinate (test/runtests.jl:15-27 fixture, measured: see the parity report)


@pytest.fixture(scope="module")
def nlp_small(ba, small_prob, gpu_ok):
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(small_prob), model_name="small")
    yield m
    m.close()


def _focal(x, cam_idx1, npnts):
    return np.repeat(np.abs(np.asarray(x)[3 * npnts + 9 * (np.asarray(cam_idx1) - 1) + 8]), 2)


def _res_tol(r_ref, pt2d, f):
    return EPS * (8 * np.abs(r_ref + pt2d) + 0.5 * f)


def test_library_is_the_hip_one(ba, gpu_ok):
    import ctypes
    assert ba._lib.lib()._name.endswith("libba_hip.so")
    n = ctypes.c_int(0)
    assert ba._lib.lib().ba_device_count(ctypes.byref(n)) == 0 and n.value >= 1


def test_runtests_fixture_through_c_abi(ba, fixture_runtests, gpu_ok):
    f = fixture_runtests
    m = ba.BALNLPModel(arrays=(f["cam_idx"], f["pnt_idx"], f["pt2d"], f["x"], 5, 1, 5))
    r = m.cons(f["x"])
    assert np.all(np.abs(r - f["true_residuals"]) <= _res_tol(f["true_residuals"], f["pt2d"], _focal(f["x"], f["cam_idx"], 1)))
    # the same comparison in the unit SURVEY 8d states: ulps of the PROJECTED coordinate (residual + observation), the
    # quantity the device's sin / cos / sqrt / division actually produce; the residual itself is a difference of two such
    # numbers, so its own ulp says nothing about the evaluation
    proj = np.abs(f["true_residuals"] + f["pt2d"])
    ulps = np.abs(r - f["true_residuals"]) / np.spacing(proj)
    print("test/runtests.jl:15-27 fixture: |r - true_residuals| in ulps of the projected coordinate:", ulps)
    _report("runtests_fixture_residual", max_ulps_of_projection=ulps.max(), bit_exact_entries=int(np.sum(r == f["true_residuals"])),
            entries=len(r))
    assert ulps.max() <= RES_ULPS, f"{ulps.max():.2f} ulps of the projection (bound {RES_ULPS})"
    m.close()


def test_residual_matches_reference_python_golden(ba, golden_scipy, gpu_ok):
    g = golden_scipy
    m = ba.BALNLPModel(arrays=(g["cam_idx1"], g["pnt_idx1"], g["pt2d"], g["x0"], int(g["ncams"]), int(g["npnts"]),
                               len(g["cam_idx1"])))
    for tag, x in (("x0", g["x0"]), ("xtrue", g["x_true"])):
        r = m.cons(x)
        assert np.all(np.abs(r - g["res_" + tag]) <= _res_tol(g["res_" + tag], g["pt2d"], _focal(x, g["cam_idx1"], int(g["npnts"]))))
    m.close()


def test_residual_vs_oracle(ba, orc, small_prob, nlp_small):
    p = small_prob
    r = nlp_small.cons(p["x0"])
    r_ref = orc.residuals(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["pt2d"], p["npnts"])
    err = np.abs(r - r_ref) / _res_tol(r_ref, p["pt2d"], _focal(p["x0"], p["cam_idx1"], p["npnts"]))
    print("residual max err / tolerance:", err.max())
    ulps = np.abs(r - r_ref) / np.spacing(np.abs(r_ref + p["pt2d"]))
    _report("residual_vs_oracle", max_err_over_tolerance=err.max(), max_ulps_of_projection=ulps.max(), median_ulps_of_projection=float(np.median(ulps)))
    assert err.max() <= 1


def test_jac_structure_bit_exact(ba, orc, small_prob, nlp_small):
    p = small_prob
    rows, cols = nlp_small.jac_structure()
    rr, cc = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    assert rows.dtype == np.int64 and np.array_equal(rows, rr) and np.array_equal(cols, cc)


def test_jac_coord_vs_oracle(ba, orc, small_prob, nlp_small):
    p = small_prob
    v = nlp_small.jac_coord(p["x0"]).reshape(-1, 24)
    v_ref = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["npnts"]).reshape(-1, 24)
    rel = np.abs(v - v_ref).max(1) / np.abs(v_ref).max(1)
    print("jacobian max block-relative err:", rel.max())
    _report("jac_coord_vs_oracle", max_block_relative_err=rel.max(), tolerance=1e-12)
    assert rel.max() <= 1e-12


def test_jtr_vs_oracle(ba, orc, small_prob, nlp_small):
    p = small_prob
    v_ref = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["npnts"])
    r_ref = orc.residuals(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["pt2d"], p["npnts"])
    rr, cc = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    ref = orc.mul_sparse(cc, rr, v_ref, r_ref, nlp_small.meta.nvar)  # lm.jl:57 (index arrays swapped)
    out = nlp_small.jtprod_coo(v_ref, r_ref)
    _report("jtr_vs_oracle", max_err_over_max=float(np.max(np.abs(out - ref)) / np.max(np.abs(ref))), tolerance=1e-12)
    assert np.max(np.abs(out - ref)) <= 1e-12 * np.max(np.abs(ref))


def test_f32_twins(ba, orc, small_prob, gpu_ok):
    p = small_prob
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p, np.float32), T=np.float32)
    x = p["x0"].astype(np.float32)
    r = m.cons(x)
    r_ref = orc.residuals(p["cam_idx1"], p["pnt_idx1"], x, p["pt2d"].astype(np.float32), p["npnts"])
    assert r.dtype == np.float32
    # Float32 ulp of |proj| ~ 1e3 is 6e-5; the device evaluates sin/cos in double and rounds like Julia
    assert np.max(np.abs(r - r_ref)) <= 64 * 1.2e-7 * np.max(np.abs(r_ref + p["pt2d"]))
    v = m.jac_coord(x).reshape(-1, 24)
    v_ref = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], x, p["npnts"]).reshape(-1, 24)
    assert v.dtype == np.float32
    rel = np.abs(v - v_ref).max(1) / np.abs(v_ref).max(1)
    assert rel.max() <= 1e-4
    m.close()


def test_edge_cases(ba, orc, gpu_ok):
    # empty problem
    m = ba.BALNLPModel(arrays=(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(12), 1, 1, 0))
    assert m.cons(np.zeros(12)).shape == (0,)
    assert m.jac_coord(np.zeros(12)).shape == (0,)
    m.close()
    # theta = 0 and z = 0: NaN residual, zero Jacobian block (src/BALNLPModels.jl:19-31,201)
    cam = np.array([1, 2], dtype=np.int64)
    pnt = np.array([1, 1], dtype=np.int64)
    x = np.array([0.1, 0.2, 0.0,
                  0, 0, 0, 0, 0, -5.0, 1e-7, 1e-12, 500.0,
                  0, 0, 0.3, 0, 0, 0.0, 1e-7, 1e-12, 500.0])
    m = ba.BALNLPModel(arrays=(cam, pnt, np.zeros(4), x, 2, 1, 2))
    r = m.cons(x)
    v = m.jac_coord(x)
    assert np.all(np.isnan(r[:2])) and not np.any(np.isfinite(r[2:]))
    assert np.all(v == 0)
    assert np.all(orc.jac_coord(cam, pnt, x, 1) == 0)
    m.close()
    # out-of-range index is refused, not a device fault
    with pytest.raises(ba.BAError):
        ba.BALNLPModel(arrays=(np.array([3], np.int64), np.array([1], np.int64), np.zeros(2), np.zeros(21), 2, 1, 1))


def test_unsorted_observations(ba, orc, small_prob, gpu_ok):
    """Ragged / shuffled observation order (not BAL order): every entry point must still agree."""
    p = small_prob
    perm = np.random.default_rng(3).permutation(p["nobs"])
    cam, pnt = p["cam_idx1"][perm], p["pnt_idx1"][perm]
    pt2d = p["pt2d"].reshape(-1, 2)[perm].ravel()
    m = ba.BALNLPModel(arrays=(cam, pnt, pt2d, p["x0"], p["ncams"], p["npnts"], p["nobs"]))
    r_ref = orc.residuals(cam, pnt, p["x0"], pt2d, p["npnts"])
    v_ref = orc.jac_coord(cam, pnt, p["x0"], p["npnts"])
    rr, cc = orc.jac_structure(cam, pnt, p["npnts"])
    assert np.array_equal(m.jac_structure()[1], cc)
    out = m.jtprod_coo(v_ref, r_ref)
    ref = orc.mul_sparse(cc, rr, v_ref, r_ref, m.meta.nvar)
    assert np.max(np.abs(out - ref)) <= 1e-12 * np.max(np.abs(ref))
    d, half, _ = ba.lm_step(m, p["x0"], 10.0)
    rc, d_ref, dr_ref, _ = orc.lm_step(p["ncams"], p["npnts"], cam, pnt, pt2d, p["x0"], 10.0)
    assert rc == 0
    assert np.linalg.norm(d - d_ref) <= 1e-9 * np.linalg.norm(d_ref)
    # facto = :PCG on unsorted observations: the product's point sweep falls back to the list-driven kernel
    dp, _, _, its = ba.lm_step(m, p["x0"], 10.0, pcg=(1e-13, 5000))
    assert 0 < its < 5000 and np.linalg.norm(dp - d_ref) <= 1e-8 * np.linalg.norm(d_ref)
    m.close()


@pytest.mark.parametrize("n", [5, 128, 200, 441, 700, 4480, 8100])
def test_dense_ldl_vs_numpy(ba, n, gpu_ok):
    """4480 (35 tile rows): the hoisted-diagonal schedule; 8100 (64 tile rows): the fused pair schedule (k_ldl_pairdiag
    hoisted beside the trailing update, k_ldl_pairtrsm) for the first pairs, then the hoisted one, then in order."""
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 8))
    A = G @ G.T + 0.5 * np.eye(n)
    # asymmetric right-hand side and a matrix with no special structure: a transposed fragment layout cannot pass
    b = rng.standard_normal(n)
    x, ms = ba._lib.dense_ldl_solve(A, b)
    x_ref = np.linalg.solve(A, b)
    # cond(A): eigenvalues of G G' + I / 2 lie in [0.5, (sqrt(n) + sqrt(n + 8))^2 + 0.5] -- about 8 n; the large cases take the
    # bound (the SVD of an 8100 x 8100 matrix is 100 s of host time)
    cond = np.linalg.cond(A) if n < 2000 else 8.0 * n + 70.0
    assert np.linalg.norm(x - x_ref) <= 1e-10 * np.linalg.norm(x_ref) * cond ** 0.5


@pytest.mark.parametrize("n", [64, 300, 1000])
def test_dense_ldl_f32(ba, n, gpu_ok):
    """Float32 factor/solve (facto_type = Float32): Float32-level accuracy against the Float64 solution."""
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 8))
    A = G @ G.T / n + np.eye(n)  # well conditioned
    b = rng.standard_normal(n)
    x, ms = ba._lib.dense_ldl_solve(A, b, f32=True)
    x_ref = np.linalg.solve(A, b)
    assert np.linalg.norm(x - x_ref) <= 1e-4 * np.linalg.norm(x_ref)


def test_dense_ldl_indefinite_and_zero_pivot(ba, gpu_ok):
    """Negative pivots on two tiles, a zero pivot at the first position of a 4 x 4 matrix.  Negative pivots in every tile of every
    schedule and zero pivots in every block, tile, zone and precision are in tests/test_dense_ldl_exact.py, on systems whose
    answer is known exactly."""
    # LDL' without pivoting accepts negative pivots (quasi-definite input), like src/ldl_aux.jl
    rng = np.random.default_rng(5)
    n = 150
    G = rng.standard_normal((n, n))
    A = G @ G.T + np.eye(n)
    A[:40, :40] *= -1.0
    A[:40, 40:] = 0.1 * A[:40, 40:]
    A[40:, :40] = A[:40, 40:].T
    b = rng.standard_normal(n)
    x, _ = ba._lib.dense_ldl_solve(A, b)
    assert np.linalg.norm(A @ x - b) <= 1e-8 * np.linalg.norm(b)
    Z = np.eye(4)
    Z[0, 0] = 0.0
    with pytest.raises(ba.SQDException):
        ba._lib.dense_ldl_solve(Z, np.ones(4))


def _cond_S(orc, p, x, lam):
    """2-norm condition number of the reduced camera system S = Hcc + lam I - W (Hpp + lam I)^-1 W' at x, formed densely on
    the host from the oracle's Jacobian (small problems only)."""
    vals = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], x, p["npnts"])
    rows, cols = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    nvar = 3 * p["npnts"] + 9 * p["ncams"]
    J = np.zeros((2 * p["nobs"], nvar))
    J[rows - 1, cols - 1] = vals
    H = J.T @ J + lam * np.eye(nvar)
    k = 3 * p["npnts"]
    S = H[k:, k:] - H[k:, :k] @ np.linalg.solve(H[:k, :k], H[:k, k:])
    return float(np.linalg.cond(S))


# one step from identical (x, lambda): the tolerance follows the conditioning (augmented LDL' vs Schur differ by
# 6e-15 at lambda = 1e3, 6e-13 at 1, 6e-10 at 1e-4 where cond(S) = 4e9 on this problem shape)
_STEP_TOL = {1e3: 1e-12, 30.0: 1e-11, 1.0: 1e-11, 1e-2: 1e-9, 1e-4: 1e-8}


@pytest.mark.parametrize("lam", [1e3, 30.0, 1.0, 1e-2, 1e-4])
def test_lm_step_vs_oracle(ba, orc, small_prob, nlp_small, lam):
    p = small_prob
    d, half, jtr = ba.lm_step(nlp_small, p["x0"], lam)
    rc, d_ref, dr_ref, jtr_ref = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], lam)
    assert rc == 0
    rel = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    cond = _cond_S(orc, p, p["x0"], lam)
    print(f"lambda {lam}: |d - d_ref|/|d_ref| = {rel:.2e}, cond(S) = {cond:.2e}, tolerance {_STEP_TOL[lam]:.0e}")
    _report(_test_name(), step_vs_oracle=rel, cond_S=cond, tolerance=_STEP_TOL[lam])
    assert rel <= _STEP_TOL[lam]
    assert abs(half - 0.5 * dr_ref @ dr_ref) <= 1e-9 * (0.5 * dr_ref @ dr_ref)
    assert np.max(np.abs(jtr - jtr_ref)) <= 1e-12 * np.max(np.abs(jtr_ref))


@pytest.mark.parametrize("variant", [1, 0])
def test_lm_solve_vs_oracle(ba, orc, small_prob, gpu_ok, variant):
    p = small_prob
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)
    if variant == 1:
        st = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False)
    else:
        st = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None")
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"],
                                              variant=variant)
    assert rc == 0
    print(st.status, st.iter, st.objective, "oracle:", st_ref.status, st_ref.iter, st_ref.objective)
    _report(_test_name(), iterations=st.iter, iterations_oracle=st_ref.iter, objective_rel_err=abs(st.objective - st_ref.objective) / st_ref.objective,
            solution_rel_err=float(np.linalg.norm(st.solution - x_ref) / np.linalg.norm(x_ref)),
            trace_max_rel_dev=float(np.max(np.abs(np.array([r[1] for r in st.log]) - log_ref[:len(st.log), 1]) / log_ref[:len(st.log), 1])) if len(st.log) == len(log_ref) else -1.0)
    assert st.iter == st_ref.iter
    assert st.status == orc.STATUS[st_ref.status]
    assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
    assert [r[7] for r in st.log] == [bool(v) for v in log_ref[:, 7]]
    f_gpu = np.array([r[1] for r in st.log])
    assert np.allclose(f_gpu, log_ref[:, 1], rtol=1e-6)
    assert np.linalg.norm(st.solution - x_ref) <= 1e-6 * np.linalg.norm(x_ref)
    assert m.counters.neval_jac == st.n_jacobian + 1
    m.close()


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("norm,code", [("J", 1), ("A", 2)])
def test_lm_normalize_vs_oracle(ba, orc, small_prob, gpu_ok, norm, code, variant):
    """normalize = :J / :A (src/lma_aux.jl:102-154): a preconditioning, same iterates up to rounding.  variant 0 is the
    `solve_ba.jl ... LDL AMD J|A` path: LevenbergMarquardt.jl scales at initialisation and after every accepted step
    (LevenbergMarquardt.jl:117-120,345-347); the device recomputes the same diagonal at every trial step."""
    p = small_prob
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    if variant == 1:
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", norm, False)
    else:
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", norm)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"],
                                              variant=variant, normalize=code)
    assert rc == 0 and st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
    assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
    assert [r[7] for r in st.log] == [bool(v) for v in log_ref[:, 7]]
    assert np.allclose([r[1] for r in st.log], log_ref[:, 1], rtol=1e-6)
    assert np.linalg.norm(st.solution - x_ref) <= 1e-6 * np.linalg.norm(x_ref)
    m.close()


@pytest.mark.parametrize("linesearch,nu_d,delta_d,want", [
    (False, 9.0, 2.0, "rej"),  # plain rejections: lambda = max(lambda, 1/|delta|) nu_m                 (lm.jl:308)
    (True, 9.0, 3.0, "ls"),    # line search with delta_d != 2: delta_r = (delta_r - r)/delta_d       (lm.jl:277)
    (True, 3.0, 3.0, "ls"),    # ... lambda /= nu_d^(ntimes-1)                                          (lm.jl:329-331)
    (True, 9.0, 1.5, "lbl"),   # delta_d < 2: the recursion's model value exceeds f: accepted, logged "rej" (lm.jl:260,292)
    (True, 9.0, 2.0, "any"),   # the reference's default delta_d
])
def test_lm_rejections_and_linesearch_vs_oracle(ba, orc, small_prob, gpu_ok, linesearch, nu_d, delta_d, want):
    """A start far from the minimum and a fast damping decrease: first-try rejections, the line-search loop and the ntimes
    powers run on the device and are compared with the oracle row by row (iteration, accepted flag, f, |J'r|, lambda,
    |delta|, rho: the log columns of src/lm.jl:304) over the well-conditioned prefix of the run, which must contain the
    event the case is for."""
    p = small_prob
    x0 = _hard_start(p)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    kw = dict(nu_d=nu_d, delta_d=delta_d, ite_max=40, **_TIGHT)
    st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", linesearch, x=x0, **kw)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], x0,
                                              variant=1, linesearch=linesearch, **kw)
    assert rc == 0
    n = _well_conditioned_prefix(log_ref)
    acc = [bool(v) for v in log_ref[:n, 7]]
    lam = log_ref[:, 4]
    # an accepted row after which lambda did not shrink: ntimes = 1 in lm.jl:329-331, i.e. the line search ran
    ls_rows = [k for k in range(min(n, len(lam) - 1)) if acc[k] and lam[k + 1] >= lam[k] * 0.999]
    print(f"oracle: {st_ref.iter} {orc.STATUS[st_ref.status]} f = {st_ref.objective!r}; prefix {n} rows "
          f"{''.join('a' if a else 'r' for a in acc)}, line-search rows {ls_rows}")
    print(f"device: {st.iter} {st.status} f = {st.objective!r} {''.join('a' if r[7] else 'r' for r in st.log)}")
    assert n >= 3
    if want == "rej":
        assert acc.count(False) >= 2 and not linesearch
    elif want == "ls":
        assert ls_rows
    elif want == "lbl":
        k = acc.index(False)
        assert lam[k + 1] < lam[k]  # logged "rej" (model value above f) yet the step was taken and lambda decreased
    _compare_rows(st, log_ref, n)
    if st_ref.status != 6:  # both converged: same minimum
        assert abs(st.objective - st_ref.objective) <= 1e-6 * st_ref.objective
    m.close()


def test_lm_qr_vs_oracle(ba, orc, gpu_ok):
    """facto = :QR (src/lm.jl:61-66,129-152, src/qr_aux.jl:13-55).  The reference factors A = [J; sqrt(lambda) I] with
    SuiteSparse SPQR (third party, absent from the image; the oracle restates it as a dense Householder QR, pinned by the
    reference's own check test/runtests.jl:111-128).  The device solves the same least-squares problem through the
    reduced camera system, so `QR` and `LDL` take the same steps; what distinguishes the branch is the model value
    inside the line search (QR recomputes |J delta + r|^2, lm.jl:273; LDL uses the recursion of lm.jl:277, which differs
    for delta_d != 2).  Compared with the oracle's :QR run: iterations, accept/reject sequence, objective trace."""
    p = ba.synthetic.make_problem(6, 80, 320, seed=9)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    for norm, code in (("None", 0), ("J", 1), ("A", 2)):
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "QR", "AMD", norm, False)
        rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"],
                                                  variant=1, normalize=code, facto="QR")
        assert rc == 0
        print(norm, st.iter, st.status, st.objective, "oracle QR:", st_ref.iter, orc.STATUS[st_ref.status], st_ref.objective)
        assert st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
        assert [r[7] for r in st.log] == [bool(v) for v in log_ref[:, 7]]
        assert np.allclose([r[1] for r in st.log], log_ref[:, 1], rtol=1e-6)
        assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
    # line search with delta_d = 3 from a hard start: in the well-conditioned prefix of the run the line search fires once
    # and there the QR and LDL model values differ (oracle: rho 0.877 against 0.506); each must follow its oracle twin
    x0 = _hard_start(p, 1.0, 0.3, 5)
    kw = dict(nu_d=5.0, delta_d=3.0, ite_max=25, **_TIGHT)
    rho = {}
    for facto in ("QR", "LDL"):
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), facto, "AMD", "None", True, x=x0, **kw)
        rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], x0,
                                                  variant=1, linesearch=True, facto=facto, **kw)
        assert rc == 0
        n = _well_conditioned_prefix(log_ref)
        print(facto, "prefix", n, "device rho", [round(r[6], 4) for r in st.log[:n]], "oracle rho", np.round(log_ref[:n, 6], 4))
        assert n >= 4
        _compare_rows(st, log_ref, n)
        rho[facto] = np.array([r[6] for r in st.log[:n]])
    assert np.max(np.abs(rho["QR"] - rho["LDL"])) > 0.1  # the branches really differ where the line search ran
    m.close()


def test_lm_solve_ladybug49_vs_oracle(ba, orc, gpu_ok):
    """BASELINE config 2's shape (LadyBug problem-49-7776: 31 843 observations, n = 441): the complete lm.jl run against
    the oracle -- SURVEY 8d tolerances: identical iteration count, status and accept/reject sequence, objective trace
    equal to 6 significant digits over (at least) the first 10 iterations, final objective <= 1e-8 relative.  Shape of the
    published run: benchmark/third/lm_linesearch.log:2-105 (real data, not available here: synthetic data of that shape)."""
    p = ba.synthetic.make_named("ladybug-49")
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p), model_name="LadyBug/problem-49-7776-pre")
    for variant, ls in ((1, False), (1, True), (0, None)):
        if variant == 1:
            st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", ls)
        else:
            st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None")
        rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"],
                                                  variant=variant, linesearch=bool(ls))
        assert rc == 0
        print(f"variant {variant} linesearch {ls}: device {st.iter} {st.status} {st.objective!r}; oracle {st_ref.iter} "
              f"{orc.STATUS[st_ref.status]} {st_ref.objective!r}")
        assert st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
        assert [r[7] for r in st.log] == [bool(v) for v in log_ref[:, 7]]
        f_gpu = np.array([r[1] for r in st.log])
        _report(f"lm_solve_ladybug49_variant{variant}_linesearch{ls}", iterations=st.iter, min_lambda=float(log_ref[:, 4].min()),
                objective_trace_max_rel_dev=float(np.max(np.abs(f_gpu - log_ref[:, 1]) / log_ref[:, 1])),
                lambda_trace_max_rel_dev=float(np.max(np.abs(np.array([r[4] for r in st.log]) - log_ref[:, 4]) / log_ref[:, 4])),
                objective_rel_err=abs(st.objective - st_ref.objective) / st_ref.objective,
                solution_rel_err=float(np.linalg.norm(st.solution - x_ref) / np.linalg.norm(x_ref)))
        assert np.allclose(f_gpu, log_ref[:, 1], rtol=1e-6, atol=0)          # objective trace, every iteration
        assert np.allclose([r[4] for r in st.log], log_ref[:, 4], rtol=1e-9)  # lambda: same branch taken every time
        assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
        assert np.linalg.norm(st.solution - x_ref) <= 1e-6 * np.linalg.norm(x_ref)
    m.close()


def test_lm_facto_f32(ba, orc, small_prob, gpu_ok):
    """facto_type = Float32 (src/lm.jl:170-173, src/diffprecsions.jl:39-41): the factorisation runs in Float32, the
    rest in Float64.  Float32 rounding of the step moves the iterates, so the oracle's Float32 run and the Float64 run
    are compared on what both must reach: the same final objective to Float32-level accuracy."""
    p = small_prob
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    st32 = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, facto_type=np.float32)
    st64 = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, facto_type=np.float64)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"],
                                              variant=1, facto_f32=True)
    print("f32:", st32.status, st32.iter, st32.objective, "f64:", st64.iter, st64.objective, "oracle f32:", st_ref.iter,
          st_ref.objective)
    assert rc == 0
    assert st32.status in ("first_order", "small_residual", "acceptable", "small_step")
    assert abs(st32.objective - st_ref.objective) <= 1e-3 * st_ref.objective
    assert abs(st32.objective - st64.objective) <= 1e-3 * st64.objective
    assert st32.objective != st64.objective or st32.iter != st64.iter or not np.array_equal(st32.solution, st64.solution)
    m.close()


def test_lm_facto_f16_and_two_stage_restart(ba, orc, small_prob, gpu_ok):
    """facto_type = Float16 (src/lm.jl:92-95,165-169; normalize_F16! / normalize_vect!, src/lma_aux.jl:30-52,90-95) and the
    two-stage scheme of src/benchmark_diffprec.jl:38-72: a Float16 stage with loose tolerances, then a restart in Float64
    from its solution (`x=`).  The oracle runs the reference's algorithm in emulated Float16 arithmetic (Float32 operation,
    result rounded to binary16, as Julia does); the device rounds the same inputs to Float16 and then works in Float32.
    Float16-level tolerance: per step |delta| to 2 %, objective to 1 % over the first rows, 10 % later (rounding noise of
    ~10^5 Float16 pivots in the oracle accumulates); the statuses the reference's own Float16 runs end with are allowed
    (benchmark/diffprec/lm_diffprec_F1632_64.log:55,1610: step too small, unhandled exception)."""
    p = small_prob
    x0 = _hard_start(p, 0.1, 0.02, 3)
    tol16 = dict(oatol=1e-2, ortol=1e-2, atol=1e-2, rtol=1e-1, satol=1e-5, srtol=1e-5, restol=1e-5)  # benchmark_diffprec.jl:46
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)
    st16 = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, x=x0, facto_type=np.float16, ite_max=30, **tol16)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], x0, variant=1,
                                              facto_f32=2, ite_max=30, **tol16)
    assert rc == 0
    print("device Float16 stage:", st16.iter, st16.status, st16.objective, "oracle:", st_ref.iter, orc.STATUS[st_ref.status],
          st_ref.objective)
    log = np.array([r[:7] + (float(r[7]),) for r in st16.log])
    n = min(len(log), len(log_ref))
    assert n >= 4
    print("f  device", log[:n, 1], "\nf  oracle", log_ref[:n, 1], "\n|d| device", log[:n, 5], "\n|d| oracle", log_ref[:n, 5])
    k = min(n, 5)
    assert [bool(v) for v in log[:k, 7]] == [bool(v) for v in log_ref[:k, 7]]
    assert np.allclose(log[:k, 4], log_ref[:k, 4], rtol=1e-9)   # lambda: same decisions
    assert np.allclose(log[:k, 5], log_ref[:k, 5], rtol=2e-2)   # |delta|
    assert np.allclose(log[:k, 1], log_ref[:k, 1], rtol=1e-2)   # objective
    assert np.allclose(log[:n, 1], log_ref[:n, 1], rtol=1e-1)
    assert st16.status in ("small_step", "acceptable", "first_order", "exception", "max_iter")
    f0 = 0.5 * float(np.sum(m.cons(x0) ** 2))
    assert st16.objective < 0.5 * f0  # the Float16 stage makes real progress ...
    tight = dict(rtol=1e-10, atol=1e-10, ortol=1e-13, oatol=0.0, restol=0.0, satol=0.0, srtol=1e-13)  # down to the minimum itself
    st64 = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, x=x0, **tight)
    assert st16.objective > 2 * st64.objective  # ... but stops far from the minimum (its steps are scaled by D_j / mu)
    # stage 2: restart in Float64 from the Float16 solution (benchmark_diffprec.jl:52)
    st2 = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, x=st16.solution, **tight)
    print("restart:", st2.iter, st2.status, st2.objective, " direct Float64:", st64.iter, st64.status, st64.objective)
    assert st2.status in ("first_order", "acceptable", "small_residual", "small_step")
    assert abs(st2.objective - st64.objective) <= 1e-6 * st64.objective
    # the reference's actual combination: a Float32 model with facto_type = Float16, restart with facto_type = Float32
    arr = list(ba.synthetic.as_arrays(p))
    arr32 = [arr[0], arr[1], arr[2].astype(np.float32), arr[3].astype(np.float32)] + arr[4:]
    m32 = ba.BALNLPModel(arrays=tuple(arr32), T=np.float32)
    s1 = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), "LDL", "Metis", "None", False, x=x0.astype(np.float32),
                                facto_type=np.float16, ite_max=30, **tol16)
    s2 = ba.Levenberg_Marquardt(fr, "LDL", "Metis", "None", False, x=s1.solution.astype(np.float64), facto_type=np.float32, **tight)
    print("Float32 model, Float16 stage:", s1.iter, s1.status, s1.objective, "-> Float32/64 stage:", s2.iter, s2.status, s2.objective)
    assert s1.objective < 0.5 * f0 and abs(s2.objective - st64.objective) <= 1e-3 * st64.objective
    with pytest.raises(ValueError):  # Float16 exists in the :LDL branch only (src/lm.jl:92-95)
        ba.Levenberg_Marquardt(fr, "QR", "AMD", "None", False, x=x0, facto_type=np.float16)
    m32.close()
    m.close()


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("norm,code", [("None", 0), ("J", 1)])
def test_lm_float32_model(ba, orc, small_prob, gpu_ok, variant, norm, code):
    """BALNLPModel(file, Float32) through Levenberg_Marquardt (eltype(x) = Float32, facto_type defaults to Float32,
    src/lm.jl:20-26; the reference's own Float32 experiment and its tolerances: src/diffprecsions.jl:19-24) against the
    oracle's T = Float32 loop (oracle/ba_oracle.c orc_lm_solve_f32: every scalar with the width Julia's promotion rules give
    it -- Float32 norms, obj, pred, ared; lambda a Float32 until lm.jl:337's Float64 literal promotes it; Float64 accept
    tests).  What differs by construction: the reference factors the AUGMENTED system in Float32, the device eliminates
    residual rows and points in Float64 and factors the reduced camera system in Float32 -- steps agree to Float32-solve
    accuracy, not to the bit.  No reference fixture pins a Float32 run: parity unpinned beyond the oracle."""
    p = small_prob
    arrays = list(ba.synthetic.as_arrays(p))
    arrays32 = [arrays[0], arrays[1], arrays[2].astype(np.float32), arrays[3].astype(np.float32)] + arrays[4:]
    m32 = ba.BALNLPModel(arrays=tuple(arrays32), T=np.float32)
    tol32 = dict(oatol=1e-4, ortol=1e-4, atol=1e-4, rtol=1e-5, satol=1e-6, srtol=1e-7)  # src/diffprecsions.jl:22
    args = ("LDL", "AMD", norm) + ((False,) if variant else ())
    st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), *args, **tol32)
    rc, x_ref, st_ref, log_ref = orc.lm_solve_f32(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], arrays32[2], arrays32[3],
                                                   variant=variant, normalize=code, **tol32)
    tag = f"variant {variant}, normalize {norm}"
    print(tag, "device:", st.status, st.iter, st.objective, " oracle:", orc.STATUS[st_ref.status], st_ref.iter, st_ref.objective)
    assert rc == 0
    assert st.solution.dtype == np.float32
    if variant == 1:  # lm.jl: lambda0 = max(30, 1e10 / |J'r|) keeps the damped system well conditioned: the whole run is compared
        assert st.iter == st_ref.iter, f"{tag}: {st.iter} iterations, oracle {st_ref.iter}"
        assert st.status == orc.STATUS[st_ref.status], f"{tag}: status {st.status}, oracle {orc.STATUS[st_ref.status]}"
        _float32_rows(st, log_ref, tag, f_rtol=1e-4)
        assert abs(st.objective - st_ref.objective) <= 1e-4 * st_ref.objective, f"{tag}: objective {st.objective!r} vs {st_ref.objective!r}"
        assert abs(st.lambda_final - st_ref.lambda_final) <= 1e-6 * st_ref.lambda_final, f"{tag}: final lambda {st.lambda_final!r} vs {st_ref.lambda_final!r}"
    else:
        # LevenbergMarquardt.jl starts at lambda = 0.1 and divides by 3 per accepted step: within a few iterations the
        # reference's Float32 factorisation of the AUGMENTED system is at its noise level (the Float32 oracle run itself
        # departs from the Float64 one by 2e-4 in f there), while the device eliminates in Float64 and only factors the reduced
        # camera system in Float32.  Rows are compared while lambda >= 1e-2; afterwards: same minimum to 1e-3, the iteration
        # counts may differ by one (the stop is the 1e-4 objective-change test).
        n = _well_conditioned_prefix(log_ref)
        assert n >= 2, f"{tag}: only {n} well-conditioned rows"
        # (|J'r| right after a step taken at lambda = 0.1 is the small difference of large terms: 1e-1)
        _float32_rows(st, log_ref, tag, n=n, f_rtol=1e-3, lam_rtol=1e-6, delta_rtol=5e-3, g_rtol=1e-1)
        assert abs(st.iter - st_ref.iter) <= 1, f"{tag}: {st.iter} iterations, oracle {st_ref.iter}"
        assert st.status in ("acceptable", "first_order", "small_step"), f"{tag}: status {st.status}"
        assert abs(st.objective - st_ref.objective) <= 1e-3 * st_ref.objective, f"{tag}: objective {st.objective!r} vs {st_ref.objective!r}"
    # the returned objective is the one of the returned (Float32) point, evaluated by the Float32 residual kernel
    r = m32.cons(st.solution)
    assert abs(0.5 * float(r.astype(np.float64) @ r.astype(np.float64)) - st.objective) <= 1e-5 * st.objective
    if variant == 1 and code == 0:
        # eps(Float32)-derived default tolerances: satol + srtol |x| stops a BAL problem at its first accepted step, in
        # the oracle as on the device
        st_def = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), "LDL", "AMD", "None", False)
        rc, _, sd_ref, _ = orc.lm_solve_f32(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], arrays32[2], arrays32[3], variant=1)
        assert rc == 0 and st_def.status == orc.STATUS[sd_ref.status] == "small_step" and st_def.iter == sd_ref.iter
    m32.close()


def test_lm_float32_model_rejections(ba, orc, small_prob, gpu_ok):
    """The Float32-model loop through rejected steps and the line search (far start, small initial damping): lambda goes
    through max(lambda, 1 / |delta|) * nu_m^(ntimes + 1) in Float32 before the first accepted step and in Float64 after."""
    p = small_prob
    x0 = _hard_start(p).astype(np.float32)
    arrays = list(ba.synthetic.as_arrays(p))
    arrays32 = [arrays[0], arrays[1], arrays[2].astype(np.float32), x0] + arrays[4:]
    m32 = ba.BALNLPModel(arrays=tuple(arrays32), T=np.float32)
    tol32 = dict(oatol=1e-4, ortol=1e-4, atol=1e-4, rtol=1e-5, satol=1e-6, srtol=1e-7)
    for ls in (False, True):
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m32), "LDL", "AMD", "None", ls, lam=1e-3, ite_max=12, **tol32)
        rc, _, st_ref, log_ref = orc.lm_solve_f32(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], arrays32[2], x0, variant=1,
                                                  linesearch=ls, lam=1e-3, ite_max=12, **tol32)
        assert rc == 0
        n = _well_conditioned_prefix(log_ref)
        log = np.array([r[:7] + (float(r[7]),) for r in st.log])
        print(f"linesearch={ls}: device {st.status} {st.iter} {st.objective}; oracle {orc.STATUS[st_ref.status]} {st_ref.iter} "
              f"{st_ref.objective}; rows compared {n}; rejected rows {int(np.sum(log_ref[:n, 7] == 0))}")
        assert n >= 3
        if not ls:  # (with the line search the halved steps are accepted inside the iteration: no rejected row)
            assert np.any(log_ref[:n, 7] == 0), "the start must produce rejected steps inside the compared prefix"
        acc, acc_ref = [bool(v) for v in log[:n, 7]], [bool(v) for v in log_ref[:n, 7]]
        assert acc == acc_ref, f"linesearch={ls}: accept/reject {acc} vs oracle {acc_ref}"
        err_f = np.abs(log[:n, 1] - log_ref[:n, 1]) / np.abs(log_ref[:n, 1])
        err_l = np.abs(log[:n, 4] - log_ref[:n, 4]) / np.abs(log_ref[:n, 4])
        # (from this far start the steps are large and a Float32 factorisation's error is amplified: f to 5e-3 over the prefix)
        assert err_f.max() <= 5e-3, f"linesearch={ls}: f differs by {err_f.max():.2e} at row {int(err_f.argmax())}"
        assert err_l.max() <= 5e-3, f"linesearch={ls}: lambda differs by {err_l.max():.2e} at row {int(err_l.argmax())}"
    m32.close()


def test_lm_linesearch_vs_oracle(ba, orc, small_prob, gpu_ok):
    """every step accepted at the first try here: the flag must then change nothing (the loop itself is covered by
    test_lm_rejections_and_linesearch_vs_oracle)"""
    p = small_prob
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "Metis", "None", True, lam=1e-3)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"],
                                              variant=1, linesearch=True, lam=1e-3)
    assert rc == 0 and st.iter == st_ref.iter
    assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
    m.close()


def test_lm_step_dubrovnik_shape_vs_oracle(ba, orc, gpu_ok):
    """BASELINE config 3's shape (Dubrovnik-356-226730: 1.26 M observations, n = 3204, 26 tile rows): one LM step against
    the oracle's LDL' of the augmented system (~40 s of single-threaded CPU factorisation, the largest size the oracle
    finishes in a test).  Tolerance: SURVEY 8d, |delta - delta_ref| <= 1e-9 |delta_ref|."""
    p = ba.synthetic.make_named("dubrovnik-356")
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    lam = 30.0
    d, half, jtr = ba.lm_step(m, p["x0"], lam)
    rc, d_ref, dr_ref, jtr_ref = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], lam)
    assert rc == 0
    rel = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    print(f"dubrovnik shape: |d - d_ref|/|d_ref| = {rel:.2e}, |d| = {np.linalg.norm(d_ref):.3e}")
    _report("lm_step_dubrovnik_shape", step_vs_oracle=rel, lam=lam, model_value_rel=abs(half - 0.5 * dr_ref @ dr_ref) / (0.5 * dr_ref @ dr_ref),
            jtr_max_err_over_max=float(np.max(np.abs(jtr - jtr_ref)) / np.max(np.abs(jtr_ref))))
    assert rel <= 1e-9
    assert abs(half - 0.5 * dr_ref @ dr_ref) <= 1e-9 * (0.5 * dr_ref @ dr_ref)
    assert np.max(np.abs(jtr - jtr_ref)) <= 1e-11 * np.max(np.abs(jtr_ref))
    m.close()


def test_many_cameras_step(ba, orc, gpu_ok):
    """Wide reduced camera system (600 cameras -> n = 5400, 43 tile rows) with few points: exercises the tile indexing
    of the Schur scatter, the paired-panel factorisation and the sweeps well beyond the other tests' sizes.  Reference:
    dense normal equations assembled from the oracle's Jacobian and solved by numpy."""
    p = ba.synthetic.make_problem(600, 500, 1800, seed=3)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    lam = 50.0
    d, half, jtr = ba.lm_step(m, p["x0"], lam)
    rows, cols = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
    vals = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["npnts"])
    r = orc.residuals(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["pt2d"], p["npnts"])
    nvar = m.meta.nvar
    J = np.zeros((2 * p["nobs"], nvar))
    J[rows - 1, cols - 1] = vals
    d_ref = np.linalg.solve(J.T @ J + lam * np.eye(nvar), -J.T @ r)
    assert np.linalg.norm(d - d_ref) <= 1e-9 * np.linalg.norm(d_ref)
    assert abs(half - 0.5 * np.sum((J @ d_ref + r) ** 2)) <= 1e-9 * half
    m.close()


def test_reader_to_model(ba, orc, small_prob, tmp_path, gpu_ok):
    p = small_prob
    path = str(tmp_path / "Synth" / "problem-12-400-pre.txt.bz2")
    ba.synthetic.write_bal(path, p)
    m = ba.BALNLPModel(path)
    assert (m.ncams, m.npnts, m.nobs) == (p["ncams"], p["npnts"], p["nobs"])
    assert np.array_equal(m.meta.x0, p["x0"]) and np.array_equal(m.pt2d, p["pt2d"])
    r = m.cons(m.meta.x0)
    r_ref = orc.residuals(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["pt2d"], p["npnts"])
    assert np.all(np.abs(r - r_ref) <= _res_tol(r_ref, p["pt2d"], _focal(p["x0"], p["cam_idx1"], p["npnts"])))
    m.close()


def test_jacobian_vs_oracle_two_million_observations(ba, orc, gpu_ok):
    """Every block of a 2 M-observation Jacobian against the oracle: catches sporadic corruption that a few thousand
    observations do not (an inline-asm store without its hazard wait state once corrupted 0.5 % of the blocks, only
    visible from ~10^6 observations up)."""
    p = ba.synthetic.make_problem(400, 400000, 2000000, seed=21)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    v = m.jac_coord(p["x0"]).reshape(-1, 24)
    v_ref = orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["npnts"]).reshape(-1, 24)
    rel = np.abs(v - v_ref).max(1) / np.abs(v_ref).max(1)
    assert rel.max() <= 1e-12, (rel.max(), int((rel > 1e-12).sum()))
    r = m.cons(p["x0"])
    r_ref = orc.residuals(p["cam_idx1"], p["pnt_idx1"], p["x0"], p["pt2d"], p["npnts"])
    assert np.all(np.abs(r - r_ref) <= _res_tol(r_ref, p["pt2d"], _focal(p["x0"], p["cam_idx1"], p["npnts"])))
    m.close()


def test_full_size_properties(ba, gpu_ok):
    """BASELINE-size shape (Dubrovnik-356: 1.26 M observations): size-independent properties instead of an oracle run.
    pattern == closed form (vectorised); J'r linear in r; residual at x_true minus noise-free projection ~ noise."""
    p = ba.synthetic.make_named("dubrovnik-356")
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    rows, cols = m.jac_structure()
    k = np.arange(p["nobs"])
    assert np.array_equal(rows.reshape(-1, 24)[:, 0], 2 * k + 1) and np.array_equal(rows.reshape(-1, 24)[:, 23], 2 * k + 2)
    assert np.array_equal(cols.reshape(-1, 24)[:, 2], 3 * (p["pnt_idx1"] - 1) + 3)
    assert np.array_equal(cols.reshape(-1, 24)[:, 23], 3 * p["npnts"] + 9 * p["cam_idx1"])
    assert np.array_equal(cols.reshape(-1, 24)[:, :12], cols.reshape(-1, 24)[:, 12:])
    r = m.cons(p["x_true"])
    assert abs(np.std(r) - 0.5) < 0.01  # pt2d = proj(x_true) + N(0, 0.5^2)
    vals = m.jac_coord(p["x0"])
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(2 * p["nobs"]), rng.standard_normal(2 * p["nobs"])
    ja, jb, jab = m.jtprod_coo(vals, a), m.jtprod_coo(vals, b), m.jtprod_coo(vals, 2 * a - 3 * b)
    assert np.max(np.abs(jab - (2 * ja - 3 * jb))) <= 1e-11 * np.max(np.abs(jab))
    # directional derivative: r(x + h d) - r(x - h d) ~ 2h J d, checked through d' J' w = (J d)' w
    d = rng.standard_normal(m.meta.nvar) * 1e-3
    h = 1e-4
    fd = (m.cons(p["x0"] + h * d) - m.cons(p["x0"] - h * d)) / (2 * h)
    w = rng.standard_normal(2 * p["nobs"])
    lhs = d @ m.jtprod_coo(vals, w)
    assert abs(lhs - fd @ w) <= 1e-5 * (np.linalg.norm(fd) * np.linalg.norm(w))
    m.close()


def test_lm_step_venice_size_normal_equations(ba, gpu_ok):
    """The metric's own size (Venice-1778 shape: 5.0 M observations, 120 M non-zeros, n = 16 002): the step returned by
    ba_lm_step must solve the reference's linear system, checked matrix-free with the Jacobian taken through the C ABI
    (jac_structure! / jac_coord!) -- (J'J + lambda I) delta = -J'r (lm.jl:154-238 in normal-equation form) and
    1/2 |J delta + r|^2 = the returned model value (lm.jl:229)."""
    import scipy.sparse as sp
    p = ba.synthetic.make_named("venice-1778")
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    lam = 30.0
    d, half, jtr = ba.lm_step(m, p["x0"], lam)
    rows, cols = m.jac_structure()
    vals = m.jac_coord(p["x0"])
    r = m.cons(p["x0"])
    J = sp.csr_matrix((vals, (rows - 1, cols - 1)), shape=(m.meta.ncon, m.meta.nvar))
    del rows, cols, vals
    g = J.T @ r
    assert np.max(np.abs(jtr - g)) <= 1e-11 * np.max(np.abs(g))
    Jd = J @ d
    lhs = J.T @ Jd + lam * d
    rel = np.linalg.norm(lhs + g) / np.linalg.norm(g)
    print(f"venice size: |(J'J + lam I) d + J'r| / |J'r| = {rel:.2e}")
    assert rel <= 1e-9
    model = 0.5 * float((Jd + r) @ (Jd + r))
    assert abs(half - model) <= 1e-10 * model
    m.close()


def _matfree_normal_check(m, p, x, d, lam):
    """|(J'J + lam I) d + J'r| / |J'r| and 1/2 |J d + r|^2 with J taken through the C ABI (jac_coord!) and applied
    matrix-free in numpy (24 entries per observation, the layout of src/BALNLPModels.jl:137-153,201)."""
    nobs, npnts, ncams = p["nobs"], p["npnts"], p["ncams"]
    pnt0 = np.asarray(p["pnt_idx1"]) - 1
    cam0 = np.asarray(p["cam_idx1"]) - 1
    vals = m.jac_coord(x).reshape(nobs, 2, 12)
    r = m.cons(x).reshape(nobs, 2)
    dp, dc = d[:3 * npnts].reshape(npnts, 3), d[3 * npnts:].reshape(ncams, 9)
    Jd = np.einsum("oac,oc->oa", vals[:, :, :3], dp[pnt0]) + np.einsum("oac,oc->oa", vals[:, :, 3:], dc[cam0])

    def jt(w):  # J' w
        gp = np.einsum("oac,oa->oc", vals[:, :, :3], w)
        gc = np.einsum("oac,oa->oc", vals[:, :, 3:], w)
        out = np.empty(3 * npnts + 9 * ncams)
        for c in range(3):
            out[c:3 * npnts:3] = np.bincount(pnt0, weights=gp[:, c], minlength=npnts)
        for c in range(9):
            out[3 * npnts + c::9] = np.bincount(cam0, weights=gc[:, c], minlength=ncams)
        return out

    g = jt(r)
    lhs = jt(Jd) + lam * d
    return np.linalg.norm(lhs + g) / np.linalg.norm(g), 0.5 * float(np.sum((Jd + r) ** 2)), g


def test_lm_step_f32_final_size(ba, gpu_ok):
    """BASELINE config 5 (Final problem-13682-4456117, `facto_type = Float32`: src/diffprecsions.jl:39-41,
    src/lm.jl:170-173) at its FULL shape on one GPU: 29.0 M observations, n = 123 138, the reduced camera system held as
    60.7 GB of Float64 tiles + 30.3 GB of Float32 tiles.  One linear LM step with the Float32 factorisation; the Jacobian
    is taken through the C ABI and the step is checked matrix-free in Float64 on the host:
       |(J'J + lambda I) delta + J'r| / |J'r|   at Float32 level (<= 2e-3; a Float64 factorisation gives ~1e-12), and
       the returned model value 1/2 |J delta + r|^2 equal to the host's to 1e-10 (that part is Float64 on the device).
    The size-independent property stands in for an oracle run (the CPU oracle would need days at this size)."""
    p = ba.synthetic.make_named("final-13682")
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p), model_name="Final/problem-13682-4456117-pre")
    lam = 30.0
    d, half, jtr = ba.lm_step(m, p["x0"], lam, facto_type=np.float32)
    assert np.all(np.isfinite(d))
    rel, model, g = _matfree_normal_check(m, p, p["x0"], d, lam)
    print(f"final-13682, Float32 factorisation: |(J'J + lam I) d + J'r| / |J'r| = {rel:.3e}; |d| = {np.linalg.norm(d):.4e}")
    assert np.max(np.abs(jtr - g)) <= 1e-10 * np.max(np.abs(g))
    assert rel <= 2e-3
    assert abs(half - model) <= 1e-10 * model
    # the step must be a descent direction of the Float64 objective and reduce it (what lm.jl:257-259 then tests)
    r0 = m.cons(p["x0"])
    r1 = m.cons(p["x0"] + d)
    assert g @ d < 0 and float(r1 @ r1) < float(r0 @ r0)
    m.close()


def test_dense_ldl_venice_size_all_schedules(ba, gpu_ok):
    """n = 16 002 (Venice's reduced camera system, 126 tile rows): the fused pair schedule, round 1's hoisted-diagonal
    schedule (BA_LDL_FUSE=0) and the strictly in-order one (BA_LDL_HOIST=0) must all solve the system (residual check:
    numpy's own solve of a 2 GB matrix is not needed) and agree with each other to rounding."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import __graft_entry__ as ge; ba = ge.load_package(); "
            "rng = np.random.default_rng(1); n = 16002; R = rng.standard_normal((n, n)); A = R + R.T; del R; "
            "A[np.diag_indices(n)] += 4 * np.sqrt(n); b = rng.standard_normal(n); x, ms = ba._lib.dense_ldl_solve(A, b); "
            "print('REL', np.linalg.norm(A @ x - b) / np.linalg.norm(b)); print('MS', ms); np.save(sys.argv[1], x)") % root
    xs = {}
    for tag, extra in (("fused", {}), ("hoist1", {"BA_LDL_FUSE": "0"}), ("inorder", {"BA_LDL_HOIST": "0"})):
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ba_ldl_{tag}_{os.getpid()}.npy")
        r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, env=dict(os.environ, **extra), timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        rel = float([l for l in r.stdout.splitlines() if l.startswith("REL")][0].split()[1])
        ms = float([l for l in r.stdout.splitlines() if l.startswith("MS")][0].split()[1])
        print(f"{tag}: residual {rel:.2e}, factor {ms:.2f} ms")
        assert rel < 1e-12, (tag, rel)
        xs[tag] = np.load(out)
        os.remove(out)
    for tag in ("hoist1", "inorder"):
        assert np.linalg.norm(xs[tag] - xs["fused"]) <= 1e-12 * np.linalg.norm(xs["fused"])


def test_dense_ldl_hoisted_schedule_and_its_fallback(ba, gpu_ok):
    """n = 4480 (35 tile rows) is the smallest size that takes the hoisted-diagonal schedule of dense_ldl_factor.  Run it
    normally, then with every kernel launch serialised by the runtime (AMD_SERIALIZE_KERNEL=3, what a counter-collecting
    profiler does): the hoisted kernel then waits for a flag nothing can raise, gives up after its bounded polling, and the
    host must redo the factorisation in order.  Both must solve the system."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import __graft_entry__ as ge; ba = ge.load_package(); "
            "rng = np.random.default_rng(0); n = int(sys.argv[1]); R = rng.standard_normal((n, n)); A = R + R.T; "
            "A[np.diag_indices(n)] += 4 * np.sqrt(n); b = rng.standard_normal(n); x, ms = ba._lib.dense_ldl_solve(A, b); "
            "print('REL', np.linalg.norm(A @ x - b) / np.linalg.norm(b))") % root
    # 4480: hoisted diagonal tile; 6800 (54 tile rows): the first pairs take the fused pair schedule (hoisted k_ldl_pairdiag)
    for n in (4480, 6800):
        for extra in ({}, {"AMD_SERIALIZE_KERNEL": "3"}):
            env = dict(os.environ, **extra)
            r = subprocess.run([sys.executable, "-c", code, str(n)], capture_output=True, text=True, env=env, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            rel = float([l for l in r.stdout.splitlines() if l.startswith("REL")][0].split()[1])
            assert rel < 1e-12, (n, extra, rel)


# ---- facto = :PCG (extension, SURVEY 8f: matrix-free conjugate gradients on the reduced camera system) ----------------------
@pytest.mark.parametrize("lam", [1e3, 30.0, 1.0])
def test_pcg_step_vs_oracle(ba, orc, small_prob, nlp_small, lam):
    """The reference has no iterative branch: what pins the PCG step is the DIRECT step of the oracle (ldl_aux.jl restated)
    from the same (x, lambda) -- solved to a relative residual of 1e-13 the CG step must reproduce it to 1e-8; a loose
    tolerance gives an inexact step whose DAMPED model value 1/2|J d + r|^2 + lambda/2 |d|^2 is larger, never smaller."""
    p = small_prob
    rc, d_ref, dr_ref, _ = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], lam)
    assert rc == 0
    d, half, jtr, its = ba.lm_step(nlp_small, p["x0"], lam, pcg=(1e-13, 5000))
    rel = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    half_ref = 0.5 * dr_ref @ dr_ref
    print(f"lambda {lam}: {its} CG iterations, |d - d_ref|/|d_ref| = {rel:.2e}")
    assert 0 < its < 5000 and rel <= 1e-8 and abs(half - half_ref) <= 1e-9 * half_ref
    d2, half2, _, its2 = ba.lm_step(nlp_small, p["x0"], lam, pcg=(1e-2, 5000))
    damped, damped_ref = half2 + 0.5 * lam * (d2 @ d2), half_ref + 0.5 * lam * (d_ref @ d_ref)
    assert its2 < its and damped >= damped_ref * (1 - 1e-12)
    # the direct entry still works on the same handle afterwards (the flag is per call)
    d3, half3, _ = ba.lm_step(nlp_small, p["x0"], lam)
    assert np.linalg.norm(d3 - d_ref) <= 1e-9 * np.linalg.norm(d_ref)


def test_pcg_step_many_cameras(ba, gpu_ok):
    """600 cameras (n = 5400): the CG step against the device's own direct step (itself checked against numpy and the oracle
    above) -- the Schur complement is applied through J, the direct path assembles and factors it."""
    big = ba.synthetic.make_problem(600, 4000, 30000, seed=3)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(big))
    d_ref, half_ref, _ = ba.lm_step(m, big["x0"], 10.0)
    d, half, _, its = ba.lm_step(m, big["x0"], 10.0, pcg=(1e-12, 5000))
    rel = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    print(f"{its} CG iterations, |d - d_ref|/|d_ref| = {rel:.2e}")
    assert its < 5000 and rel <= 1e-8 and abs(half - half_ref) <= 1e-9 * half_ref
    m.close()


def test_lm_pcg_run_reaches_the_direct_minimum(ba, small_prob, gpu_ok):
    """Complete lm.jl runs with facto = :PCG: solved tightly the run follows the :LDL run (same iterations, same accept /
    reject sequence, objective to 1e-8); with the default tolerance (1e-8) and a loose one (1e-2: truncated Newton) it still
    ends at the same minimum."""
    p = small_prob
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)
    ref = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False)
    tight = ba.Levenberg_Marquardt(fr, "PCG", "AMD", "None", False, pcg_tol=1e-13, pcg_max_iter=5000)
    print("LDL", ref.iter, ref.objective, "PCG tight", tight.iter, tight.objective, tight.n_cg)
    assert tight.iter == ref.iter and tight.status == ref.status and tight.n_cg > 0
    assert [r[7] for r in tight.log] == [r[7] for r in ref.log]
    assert abs(tight.objective - ref.objective) <= 1e-8 * ref.objective
    for kw in ({}, {"pcg_tol": 1e-2}):
        st = ba.Levenberg_Marquardt(fr, "PCG", "AMD", "None", False, **kw)
        print("PCG", kw, st.iter, st.objective, st.n_cg, st.status)
        assert st.status in ("first_order", "small_residual", "acceptable", "small_step")
        assert abs(st.objective - ref.objective) <= 1e-5 * ref.objective
    with pytest.raises(Exception):
        ba.Levenberg_Marquardt(fr, "PCG", "AMD", "None", False, facto_type=np.float16)
    # :PCG refuses what it would otherwise silently ignore: column scaling, an explicit Float32 factorisation type
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(fr, "PCG", "AMD", "J", False)
    with pytest.raises(ValueError):
        ba.Levenberg_Marquardt(fr, "PCG", "AMD", "None", False, facto_type=np.float32)
    o = ba._lib.LMOpts(variant=1, facto=2, normalize=1, linesearch=0, facto_type=0, ite_max=-1, verbose=0, x_f32=0, restol=-1, satol=-1,
                       srtol=-1, oatol=-1, ortol=-1, atol=-1, rtol=-1, nu_d=-1, nu_m=-1, lam=-1, delta_d=-1, max_time=-1, pcg_tol=-1,
                       pcg_max_iter=-1)
    st_c, x_c = ba._lib.LMStats(), np.array(p["x0"], dtype=np.float64)
    import ctypes as _C
    assert ba._lib.lib().ba_lm_solve(m.handle, _C.byref(o), ba._lib.ptr(x_c), _C.byref(st_c), _C.cast(None, ba._lib.LOG_CB), None) == 1  # BA_ERR_ARG
    m.close()


@pytest.mark.parametrize("linesearch", [False, True])
def test_lm_pcg_follows_the_oracle_through_rejections(ba, orc, small_prob, gpu_ok, linesearch):
    """The hard start of the rejection tests, facto = :PCG solved tightly: rejected steps, the lambda updates of lm.jl:308,
    329-337 and (with the line search, where :PCG re-evaluates the model value as :QR does, lm.jl:273) the rescaled steps
    follow the ORACLE's :QR / :LDL run row by row over the well-conditioned prefix."""
    p = small_prob
    x0 = _hard_start(p)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    kw = dict(nu_d=9.0, delta_d=2.0, ite_max=40, **_TIGHT)
    st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "PCG", "AMD", "None", linesearch, x=x0, pcg_tol=1e-13,
                                pcg_max_iter=5000, **kw)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], x0,
                                              variant=1, linesearch=linesearch, facto="QR" if linesearch else "LDL", **kw)
    assert rc == 0
    n = _well_conditioned_prefix(log_ref)
    print(f"oracle {st_ref.iter} rows, prefix {n}: {''.join('a' if v else 'r' for v in log_ref[:n, 7])}; device {st.iter} rows, "
          f"{st.n_cg} CG iterations")
    assert n >= 3 and (linesearch or [bool(v) for v in log_ref[:n, 7]].count(False) >= 1)
    _compare_rows(st, log_ref, n)
    m.close()


def test_pcg_only_handle_holds_nothing_of_the_size_of_S(ba, gpu_ok):
    """The tiles of S, the panel buffers and the Schur task list are allocated by the first DIRECT solve: a handle that only
    runs facto = :PCG must not grow by anything like n^2/2 doubles (2 000 cameras: S alone is 1.3 GB)."""
    import torch
    prob = ba.synthetic.make_problem(2000, 6000, 40000, seed=21)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(prob))
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    d, half, _, its = ba.lm_step(m, prob["x0"], 10.0, pcg=(1e-10, 2000))
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    grown = free0 - free1
    s_bytes = (9 * 2000) ** 2 // 2 * 8
    print(f"PCG step: {its} iterations, device memory grown by {grown / 1e6:.1f} MB (S would be {s_bytes / 1e6:.0f} MB)")
    assert 0 < its < 2000 and grown < s_bytes // 4
    d2, half2, _ = ba.lm_step(m, prob["x0"], 10.0)  # the direct solve then brings its workspace
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 - free2 > s_bytes // 2
    assert np.linalg.norm(d - d2) <= 1e-7 * np.linalg.norm(d2)
    m.close()


def test_handle_lifecycle_returns_its_device_memory(ba, gpu_ok):
    """Many cycles of: create a handle; LM runs under a robust loss, with fixed parameters, with facto_type = Float32 and
    with facto = :PCG, the camera ordering switched between them (each switch after a direct solve rebuilds the workspace);
    destroy the handle.  The device's free memory after the last cycle is back to within 1 MiB of its value after the first:
    every buffer, stream, event and recorded sequence of a handle and its workspaces is released with it.  (The first
    cycle warms the runtime's own pools up.  Before the owner types the robust loss's per-block partials, 16 KiB per
    workspace, were never released.)"""
    import time
    import torch
    p = ba.synthetic.make_problem(12, 400, 1800, seed=11)
    arrays = ba.synthetic.as_arrays(p)
    kw = dict(ite_max=2)

    def cycle():
        m = ba.BALNLPModel(arrays=arrays)
        try:
            fr = ba.FeasibilityResidual(m)
            ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, loss="huber", f_scale=2.0, **kw)
            ba.Levenberg_Marquardt(fr, "LDL", "Metis", "None", False, fixed_cameras=[1, 5], fixed_points=np.arange(1, 401, 9),
                                   **kw)
            ba.Levenberg_Marquardt(fr, "LDL", "natural", "J", False, facto_type=np.float32, **kw)
            ba.Levenberg_Marquardt(fr, "PCG", "AMD", "None", False, **kw)
        finally:
            m.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cycles = 150
    t0 = time.time()
    free_first = cycle()
    for _ in range(cycles - 1):
        free_last = cycle()
    lost = free_first - free_last
    print(f"{cycles} cycles in {time.time() - t0:.1f} s; free device memory after the first {free_first / 2**20:.1f} MiB, after "
          f"the last {free_last / 2**20:.1f} MiB ({lost / 2**10:.0f} KiB less)")
    assert lost <= 2**20, f"{lost / 2**10:.0f} KiB of device memory not returned over {cycles - 1} handle lifecycles"


def test_bench_line_contract(gpu_ok, tmp_path):
    """`python bench.py --full` prints ONE JSON line with the fields the driver reads (metric, value, unit, n_gpus, steps,
    warmup, ms_per_step, higher_is_better, scaling, vs_baseline, dtype, data, config.workload) plus roofline, cpu_baseline
    and the secondary facto = :PCG measurement; run here on a scaled-down Venice shape."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--scale", "0.05", "--steps", "4", "--warmup", "1",
                        "--cpu-seconds", "1", "--cpu-full", "none", "--full"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "pcg"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert "workload" in d["config"] and d["vs_baseline"] is None and d["data"] == "synthetic"
    roof = d["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and roof["peak"] > 0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    assert d["pcg"]["value"] > 0 and abs(d["pcg"]["objective"] - d["pcg"]["objective_direct"]) <= 1e-8 * d["pcg"]["objective_direct"]


def test_bench_plain_line_and_dump(gpu_ok, tmp_path):
    """A plain `python bench.py` (no --full) times the headline only: the same headline fields, none of the secondary
    measurements; --dump-outputs writes what the timed call returned -- the iterate after the last step and its statistics,
    float64 -- and the objective there is the one on the line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--scale", "0.05", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "lm"):
        assert key in d, key
    for key in ("host_boundary", "pcg", "roofline", "cpu_baseline", "cpu_baseline_full", "kernel_ms"):
        assert key not in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    x = np.load(out / "x.npy")
    assert x.dtype == np.float64 and np.all(np.isfinite(x))
    assert np.load(out / "objective.npy")[0] == d["lm"]["objective"]
    counts = np.load(out / "counts.npy")
    assert counts[0] == 3 and counts[1] == d["lm"]["accepted"] and counts[2] == d["lm"]["rejected"]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 * 10 ** 6


# ---- block-sparse reduced camera system (the reference's sparse LDL' exploits the same sparsity, ------------
# ---- src/ldl_aux.jl:82-201) ------------------------------------------------------------------------------------------------
def _with_env(key, value, fn):
    old = os.environ.get(key)
    if value is None:
        os.environ.pop(key, None)
    else:
        os.environ[key] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old


@pytest.mark.parametrize("locality", [0.15, 0.35])
def test_block_sparse_step_vs_oracle(ba, orc, gpu_ok, locality):
    """Cameras that only share points with their neighbours (synthetic.make_problem(locality=...)): S is block-banded, the
    tile pattern goes through the symbolic factorisation and the list-driven schedule skips every tile outside it.  The step
    must equal the oracle's ldl_aux.jl step (a sparse LDL' of the augmented system, which exploits the same sparsity) to
    1e-9, and the dense schedule's on the same problem to rounding; the Float32 factorisation to Float32 level."""
    p = ba.synthetic.make_problem(300, 3000, 15000, seed=21, locality=locality)  # n = 2700: 22 tile rows
    block_fill, tile_fill0 = ba.synthetic.schur_fill(p)
    lam = 5.0
    rc, d_ref, dr_ref, jtr_ref = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], lam)
    assert rc == 0

    def run(facto_type=None):
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
        d, half, _ = ba.lm_step(m, p["x0"], lam, facto_type=facto_type)
        pat = ba.schur_pattern(m)
        mem.append(ba.schur_memory(m))
        m.close()
        return d, half, pat

    mem = []
    d_s, half_s, pat_s = _with_env("BA_SPARSE_S", "1", run)
    d_d, half_d, pat_d = _with_env("BA_SPARSE_S", "0", run)
    # compressed storage: the list schedule allocates the pattern's tiles only; the dense schedule the whole triangle
    (full_s, held_s, _), (full_d, held_d, _) = mem[0], mem[1]
    assert full_s == full_d == 22 * 23 // 2 and held_d == full_d
    assert held_s == round(pat_s[0] * full_s), f"list schedule holds {held_s} tiles, pattern says {pat_s[0] * full_s:.1f} of {full_s}"
    d_a, half_a, pat_a = _with_env("BA_SPARSE_S", None, run)
    d32, _, _ = _with_env("BA_SPARSE_S", "1", lambda: run(np.float32))
    # the same list schedule with every pair update through the big tile-per-workgroup kernel (row lists + compressed
    # storage there too) instead of the row-split one these short updates take by default
    d_big, _, _ = _with_env("BA_LDL_UPDATE_RS_MAX", "0", lambda: _with_env("BA_SPARSE_S", "1", run))
    e = np.linalg.norm(d_big - d_s) / np.linalg.norm(d_s)
    assert e <= 1e-11, f"block-sparse schedule, big update kernel vs row-split: {e:.3e}"
    print(f"locality {locality}: block fill {block_fill:.3f}, tile fill of the keys {tile_fill0:.3f}, with factor fill "
          f"{pat_s[0]:.3f}, update tiles / dense {pat_s[1]:.3f}; automatic choice: {'sparse' if pat_a[2] else 'dense'}")
    assert pat_s[2] and not pat_d[2]
    assert pat_a[2] == (pat_s[1] <= 0.6), "automatic choice: list schedule iff its trailing updates are <= 60 % of the dense ones"
    assert pat_s[0] >= tile_fill0 - 1e-12 and pat_s[1] < 1.0
    e = np.linalg.norm(d_s - d_ref) / np.linalg.norm(d_ref)
    assert e <= 1e-9, f"block-sparse step vs oracle ldl_aux step: {e:.3e}"
    half_ref = 0.5 * float(dr_ref @ dr_ref)
    assert abs(half_s - half_ref) <= 1e-10 * half_ref
    e = np.linalg.norm(d_s - d_d) / np.linalg.norm(d_d)
    assert e <= 1e-11, f"block-sparse vs dense schedule: {e:.3e}"
    assert np.array_equal(d_a, d_s if pat_a[2] else d_d)
    e32 = np.linalg.norm(d32 - d_ref) / np.linalg.norm(d_ref)
    assert e32 <= 5e-3, f"block-sparse Float32 factorisation vs oracle: {e32:.3e}"


def test_block_sparse_lm_run_vs_oracle(ba, orc, gpu_ok):
    """A complete lm.jl run on a block-banded problem through the list schedule (recorded into hipGraphs like any small
    problem): iterations, status, accept/reject and the objective trace of the oracle's run."""
    p = ba.synthetic.make_problem(160, 1200, 6000, seed=22, locality=0.12)  # n = 1440: 12 tile rows
    m = _with_env("BA_SPARSE_S", "1", lambda: ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p)))
    st = _with_env("BA_SPARSE_S", "1", lambda: ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False))
    assert ba.schur_pattern(m)[2]
    rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], variant=1)
    assert rc == 0
    print("block-sparse run:", st.status, st.iter, st.objective, "oracle:", orc.STATUS[st_ref.status], st_ref.iter, st_ref.objective)
    assert st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
    n = _well_conditioned_prefix(log_ref)
    _compare_rows(st, log_ref, n)
    assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
    m.close()


def test_block_sparse_factor_time_follows_the_pattern(ba, gpu_ok):
    """Venice-shaped problem at 60 % of its size (1067 cameras: n = 9603, 76 tile rows; 3.0 M observations) with cameras
    sharing points inside a window of 13 % of the cameras: <= 25 % block fill.  The list schedule does the pattern's share of
    the dense factorisation's trailing-update tiles; what remains is the in-order panel chain (two diagonal tiles per pair),
    which no sparsity shortens.  Both schedules give the same step; their times (whole LM step, best of three) are recorded
    in the parity report, not asserted."""
    import time
    p = ba.synthetic.make_named("venice-1778", scale=0.6, locality=0.13)
    block_fill, _ = ba.synthetic.schur_fill(p)
    assert block_fill <= 0.25, block_fill

    def run():
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
        ba.lm_step(m, p["x0"], 30.0)  # workspace, task list, clocks
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            d, _, _ = ba.lm_step(m, p["x0"], 30.0, want_jtr=False)
            best = min(best, time.perf_counter() - t0)
        pat = ba.schur_pattern(m)
        m.close()
        return d, 1e3 * best, pat

    d_s, ms_s, pat = _with_env("BA_SPARSE_S", "1", run)
    d_d, ms_d, _ = _with_env("BA_SPARSE_S", "0", run)
    print(f"block fill {block_fill:.3f}; pattern: tile fill {pat[0]:.3f}, update tiles / dense {pat[1]:.3f}; LM step (host copies "
          f"included) {ms_s:.2f} ms with the list schedule, {ms_d:.2f} ms dense")
    assert pat[2] and pat[1] <= 0.6
    # (no assertion on milliseconds in a parity file: a slow or shared box must not turn the tests collected after this one
    # red under `pytest -x`; the times are recorded, the structural claim -- a fraction of the dense schedule's update tiles
    # -- is what is asserted)
    _report("block_sparse_factor_time", ms_list_schedule=ms_s, ms_dense_schedule=ms_d, update_tiles_over_dense=pat[1], tile_fill=pat[0])
    assert pat[1] <= 0.1, pat
    assert np.linalg.norm(d_s - d_d) <= 1e-10 * np.linalg.norm(d_d)


# ---- fill-reducing camera ordering: `perm` = :AMD / :Metis (src/lm.jl:84-88, src/LevenbergMarquardt.jl:106-110, consumed by
# ---- ldl_analyse, src/ldl_aux.jl:246-283).  AMD.jl / Metis.jl are third-party C libraries absent from the image: the
# ---- sequences themselves are parity unpinned; what is pinned is that the step does not depend on them ---------------------
@pytest.mark.parametrize("method", ["AMD", "Metis"])
def test_camera_ordering_on_a_randomly_numbered_problem(ba, orc, gpu_ok, method):
    """A block-banded problem (locality 0.13) whose cameras are renumbered at random: in the caller's numbering every tile of
    S is occupied and the factorisation is dense.  With `perm` the cameras are ordered inside the handle: tile fill within
    1.25 x of the well-numbered problem's, the list schedule chosen by itself, the step equal to the oracle's (whose
    ldl_analyse gets the same camera sequence as its permutation) to 1e-9 and to the well-numbered problem's step, mapped back,
    to 1e-10.  Every vector at the boundary stays in the caller's numbering."""
    p = ba.synthetic.make_problem(600, 6000, 30000, seed=23, locality=0.13)  # n = 5400: 43 tile rows
    q, sigma = ba.synthetic.shuffle_cameras(p, seed=1)
    lam = 5.0

    def run(prob, order):
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(prob))
        ba.set_ordering(m, order)
        d, half, jtr = ba.lm_step(m, prob["x0"], lam)
        pat = ba.schur_pattern(m)
        perm, name = ba.schur_ordering_used(m)
        m.close()
        return d, half, jtr, pat, perm, name

    d0, half0, jtr0, pat0, perm0, name0 = run(p, "natural")
    dn, halfn, _, patn, permn, _ = run(q, "natural")
    d1, half1, jtr1, pat1, perm1, name1 = run(q, method)
    print(f"{method}: tile fill {pat0[0]:.3f} as generated, {patn[0]:.3f} renumbered at random, {pat1[0]:.3f} with the ordering "
          f"('{name1}'); update tiles / dense {pat0[1]:.4f} / {patn[1]:.4f} / {pat1[1]:.4f}")
    assert np.array_equal(perm0, np.arange(1, 601)) and np.array_equal(permn, np.arange(1, 601))
    assert sorted(perm1.tolist()) == list(range(1, 601)) and name1 != "natural"
    assert patn[0] > 0.95 and not patn[2], "a random numbering fills S: dense schedule"
    assert pat1[0] <= 1.25 * pat0[0], (pat1, pat0)
    assert pat0[2] and pat1[2], "list schedule chosen automatically"
    # the host-only entry gives the same sequence and fill
    perm_h, tf_h, ff_h, _ = ba.schur_ordering(q["cam_idx1"], q["pnt_idx1"], q["ncams"], q["npnts"], method)
    assert np.array_equal(perm_h, perm1) and abs(tf_h - pat1[0]) < 1e-12 and abs(ff_h - pat1[1]) < 1e-12
    rc, d_ref, dr_ref, jtr_ref = orc.lm_step(q["ncams"], q["npnts"], q["cam_idx1"], q["pnt_idx1"], q["pt2d"], q["x0"], lam, cam_perm1=perm1)
    assert rc == 0
    e_orc = np.linalg.norm(d1 - d_ref) / np.linalg.norm(d_ref)
    e_back = np.linalg.norm(ba.synthetic.unshuffle_vector(d1, sigma, p["npnts"]) - d0) / np.linalg.norm(d0)
    e_dense = np.linalg.norm(d1 - dn) / np.linalg.norm(dn)
    _report("camera_ordering_" + method, step_vs_oracle=e_orc, step_vs_well_numbered=e_back, step_vs_dense_schedule=e_dense,
            tile_fill=pat1[0], tile_fill_well_numbered=pat0[0], sequence=name1)
    assert e_orc <= 1e-9, f"ordered step vs oracle: {e_orc:.3e}"
    assert e_back <= 1e-10, f"ordered step vs the well-numbered problem's: {e_back:.3e}"
    assert e_dense <= 1e-10, f"ordered (list schedule) vs unordered (dense schedule) on the same problem: {e_dense:.3e}"
    assert abs(half1 - 0.5 * float(dr_ref @ dr_ref)) <= 1e-10 * half1
    assert np.max(np.abs(jtr1 - jtr_ref)) <= 1e-10 * np.max(np.abs(jtr_ref))  # J'r stays in the caller's numbering


@pytest.mark.parametrize("facto_f32", [False, True])
def test_camera_ordering_of_a_scene_in_the_plane(ba, orc, gpu_ok, facto_f32):
    """Cameras standing in the plane, numbered without any structure (synthetic.make_problem(plane_radius=...)): the camera
    graph is a two-dimensional geometric graph, not a band in ANY numbering -- the ordered pattern has row lists with gaps, a
    wide frontier.  With `perm` the list schedule is chosen by itself, the step equals the
    oracle's (ldl_analyse handed the same camera sequence) and the unordered dense-schedule step; a complete lm.jl run follows
    the oracle's.  facto_f32: the same pattern through the Float32 factorisation (Float32 level)."""
    p = ba.synthetic.make_problem(480, 4000, 20000, seed=43, plane_radius=0.12)  # n = 4320: 34 tile rows
    lam = 2.0

    def run(order):
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
        ba.set_ordering(m, order)
        d, half, jtr = ba.lm_step(m, p["x0"], lam, facto_type=np.float32 if facto_f32 else None)
        pat, used = ba.schur_pattern(m), ba.schur_ordering_used(m)
        m.close()
        return d, pat, used

    dn, patn, _ = run("natural")
    d1, pat1, (perm1, name1) = run("AMD")
    print(f"plane: tile fill {patn[0]:.3f} as numbered -> {pat1[0]:.3f} ('{name1}'), update tiles / dense {pat1[1]:.4f}, list schedule {pat1[2]}")
    assert patn[0] > 0.95 and not patn[2] and pat1[0] < 0.6 and pat1[2]
    rc, d_ref, _, _ = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], lam, cam_perm1=perm1)
    assert rc == 0
    e_orc = np.linalg.norm(d1 - d_ref) / np.linalg.norm(d_ref)
    e_dense = np.linalg.norm(d1 - dn) / np.linalg.norm(dn)
    _report("camera_ordering_plane_" + ("f32" if facto_f32 else "f64"), step_vs_oracle=e_orc, step_vs_dense_schedule=e_dense,
            tile_fill=pat1[0], sequence=name1)
    tol_o, tol_d = (5e-4, 5e-4) if facto_f32 else (1e-9, 1e-10)  # measured 3.7e-5 / 7.9e-6 and 4.6e-12 / 4.0e-14 (800 cameras)
    assert e_orc <= tol_o, f"ordered step vs oracle: {e_orc:.3e}"
    assert e_dense <= tol_d, f"ordered (list schedule) vs unordered (dense schedule): {e_dense:.3e}"
    if not facto_f32:
        rc, x_ref, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], variant=1, ite_max=3)
        assert rc == 0
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "Metis", "None", False, ite_max=3)
        m.close()
        assert st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
        _compare_rows(st, log_ref, _well_conditioned_prefix(log_ref))
        assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective


def test_camera_ordering_through_levenberg_marquardt(ba, orc, gpu_ok):
    """`perm` reaches the device through Levenberg_Marquardt (ba_lm_opts.perm): complete lm.jl runs on a randomly numbered
    problem with :AMD, :Metis and with the caller's numbering agree with the oracle's run (iterations, status, rows), with
    :J scaling too (the column scaling lives in the order of S)."""
    p = ba.synthetic.make_problem(320, 2400, 12000, seed=24, locality=0.12)  # n = 2880: 23 tile rows
    q, _ = ba.synthetic.shuffle_cameras(p, seed=2)
    rc, x_ref, st_ref, log_ref = orc.lm_solve(q["ncams"], q["npnts"], q["cam_idx1"], q["pnt_idx1"], q["pt2d"], q["x0"], variant=1, ite_max=6)
    assert rc == 0
    n = _well_conditioned_prefix(log_ref)
    seen = {}
    for perm, norm in (("AMD", "None"), ("Metis", "None"), ("natural", "None"), ("AMD", "J")):
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(q))
        st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", perm, norm, False, ite_max=6)
        pat, used = ba.schur_pattern(m), ba.schur_ordering_used(m)
        m.close()
        print(perm, norm, st.status, st.iter, st.objective, pat, used[1])
        seen[(perm, norm)] = (st, pat, used)
        assert st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
        if norm == "None":
            _compare_rows(st, log_ref, n)
        assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective
    assert seen[("AMD", "None")][1][2] and seen[("Metis", "None")][1][2] and not seen[("natural", "None")][1][2]
    assert seen[("natural", "None")][2][1] == "natural"


def _irregular_problem(ba, ncams, npnts, nobs, seed, group=14):
    """A block-banded problem whose cameras are renumbered in whole groups of `group` (one tile's worth): in the caller's
    numbering the tile pattern is neither full nor a band -- row lists with gaps, tile column pairs that differ."""
    p = ba.synthetic.make_problem(ncams, npnts, nobs, seed=seed, locality=0.14)
    ng = ncams // group
    gperm = np.random.default_rng(seed).permutation(ng)
    sigma = np.arange(ncams)
    for g in range(ng):
        sigma[g * group:(g + 1) * group] = gperm[g] * group + np.arange(group)
    return ba.synthetic.shuffle_cameras(p, sigma=sigma)[0]


@pytest.mark.parametrize("ncams", [156, 310])
def test_block_sparse_irregular_pattern(ba, orc, gpu_ok, ncams):
    """Irregular tile pattern, odd number of tile rows (156 cameras: n = 1404, 11 tile rows; 310: n = 2790, 22 ... the last
    tile column pair single or full), caller's numbering kept: the list schedule over row lists with gaps and compressed
    storage against the dense schedule and the oracle, Float64 and Float32, row-split and big update kernels."""
    q = _irregular_problem(ba, ncams, 10 * ncams, 50 * ncams, seed=40 + ncams)
    lam = 3.0
    rc, d_ref, dr_ref, _ = orc.lm_step(q["ncams"], q["npnts"], q["cam_idx1"], q["pnt_idx1"], q["pt2d"], q["x0"], lam)
    assert rc == 0

    def run(facto_type=None):
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(q))
        ba.set_ordering(m, "natural")
        d, half, _ = ba.lm_step(m, q["x0"], lam, facto_type=facto_type)
        pat, mem = ba.schur_pattern(m), ba.schur_memory(m)
        m.close()
        return d, pat, mem

    d_s, pat_s, mem_s = _with_env("BA_SPARSE_S", "1", run)
    d_d, pat_d, mem_d = _with_env("BA_SPARSE_S", "0", run)
    d_big, _, _ = _with_env("BA_LDL_UPDATE_RS_MAX", "0", lambda: _with_env("BA_SPARSE_S", "1", run))
    d32_s, _, _ = _with_env("BA_SPARSE_S", "1", lambda: run(np.float32))
    d32_d, _, _ = _with_env("BA_SPARSE_S", "0", lambda: run(np.float32))
    nt = (9 * ncams + 127) // 128
    print(f"{ncams} cameras, {nt} tile rows: tile fill {pat_s[0]:.3f}, update tiles / dense {pat_s[1]:.3f}, tiles held {mem_s[1]} of {mem_s[0]}")
    assert pat_s[2] and not pat_d[2] and 0.2 < pat_s[0] < 0.95, "the pattern should be irregular, not full"
    assert mem_s[1] < mem_d[1] == mem_s[0] == nt * (nt + 1) // 2
    e = {"sparse_vs_oracle": np.linalg.norm(d_s - d_ref) / np.linalg.norm(d_ref),
         "sparse_vs_dense": np.linalg.norm(d_s - d_d) / np.linalg.norm(d_d),
         "big_kernel_vs_row_split": np.linalg.norm(d_big - d_s) / np.linalg.norm(d_s),
         "f32_sparse_vs_oracle": np.linalg.norm(d32_s - d_ref) / np.linalg.norm(d_ref),
         "f32_sparse_vs_f32_dense": np.linalg.norm(d32_s - d32_d) / np.linalg.norm(d32_d)}
    _report(f"block_sparse_irregular_{ncams}", **e)
    assert e["sparse_vs_oracle"] <= 1e-9 and e["sparse_vs_dense"] <= 1e-11 and e["big_kernel_vs_row_split"] <= 1e-11, e
    assert e["f32_sparse_vs_oracle"] <= 5e-3 and e["f32_sparse_vs_f32_dense"] <= 1e-4, e


@pytest.mark.parametrize("ncams", [10, 20, 40])
def test_block_sparse_forced_on_tiny_systems(ba, orc, gpu_ok, ncams):
    """One, two and three tile rows with the list schedule forced on (BA_SPARSE_S=1): the degenerate ends of every list."""
    p = ba.synthetic.make_problem(ncams, 40 * ncams, 160 * ncams, seed=50 + ncams)
    rc, d_ref, _, _ = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], 2.0)
    assert rc == 0

    def run(facto_type=None):
        m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
        d, _, _ = ba.lm_step(m, p["x0"], 2.0, facto_type=facto_type)
        pat = ba.schur_pattern(m)
        m.close()
        return d, pat

    d_s, pat = _with_env("BA_SPARSE_S", "1", run)
    d32, _ = _with_env("BA_SPARSE_S", "1", lambda: run(np.float32))
    assert pat[2]
    e = np.linalg.norm(d_s - d_ref) / np.linalg.norm(d_ref)
    e32 = np.linalg.norm(d32 - d_ref) / np.linalg.norm(d_ref)
    _report(f"block_sparse_tiny_{ncams}", step_vs_oracle=e, f32_step_vs_oracle=e32)
    assert e <= 1e-9 and e32 <= 5e-3, (e, e32)
