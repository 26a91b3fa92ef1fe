"""One LM step on observation graphs built to hit the boundaries of the Schur and point-side kernels (the builders and the
scenes: tests/helpers/scenes.py).  The kernels choose their code path from the length of a camera pair's task list (the number
of points the two cameras share), from the number of observations of a point and from where a point's rows fall against the
64-row batches and 64-point waves; synthetic.make_problem draws none of these deliberately.

  P     point degrees: 0, 1, 64, 65, 128, 129, 200; a point whose rows start on the last row of a batch; a wave of 64 points
        without a row; a camera nobody sees.  (The scene has 201 cameras, the last one unobserved: a point with 200 observations
        needs 200 cameras that see something.)
  K16   task lists of chosen lengths where build_tasks (csrc/ba_lm.hip) takes chunk = 16 and splits the keys above 32 tasks.
  K128  the same at chunk = 128 (ntasks >= 2^20), split above 256: unsplit keys of 65 .. 256 tasks, which take the second and
        later 64-task trips of schur_accumulate<PRE>.

CPU: every scene's properties are recounted from cam_idx1 / pnt_idx1 alone.  GPU: the step against a dense numpy step from the
oracle's Jacobian and residual (tests/_lm_ref.py), with the limits of test_prior_step_vs_dense_numpy."""
import os
import sys

import numpy as np
import pytest

from _lm_ref import F32_TOL, PCG_TOL, STEP_TOL, check_cov, hessian, jac, kappa_jacobi, limit, ref_dense, schur, step_once
from _lm_run import Ranks, arrays, fixed_vector, gauge_kw, loopback  # noqa: F401 -- loopback is a fixture
from _util import bits_report, parity_record, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import scenes  # noqa: E402

NAMES = list(scenes.BOUNDARY_SCENES)
LAMBDAS = (1.0, 30.0)
BATCH = 64  # rows of a batch of the point-side kernels, points of a wave


def chunk_of(ntasks):
    """build_tasks (csrc/ba_lm.hip): the chunk size is 16, doubled up to 128 while ntasks / (2 chunk) >= 8192; a key of more
    than 2 chunk tasks is split into chunks of `chunk` tasks (the last one shorter)."""
    ch = 16
    while ch < 128 and ntasks // (2 * ch) >= 8192:
        ch *= 2
    return ch


def recount(p):
    """(point degrees, camera degrees, {(a, b): tasks of key a > b}, ntasks) from cam_idx1 and pnt_idx1 alone (0-based)"""
    cam0, pnt0 = np.asarray(p["cam_idx1"]) - 1, np.asarray(p["pnt_idx1"]) - 1
    ncams, npnts = p["ncams"], p["npnts"]
    assert len(cam0) == len(pnt0) == p["nobs"] and cam0.min() >= 0 and cam0.max() < ncams and pnt0.min() >= 0 and pnt0.max() < npnts
    same = pnt0[1:] == pnt0[:-1]
    assert np.all(np.diff(pnt0) >= 0) and np.all(cam0[1:][same] > cam0[:-1][same]), "not in BAL order (by point, then camera)"
    deg = np.bincount(pnt0, minlength=npnts)
    cdeg = np.bincount(cam0, minlength=ncams)
    start = np.cumsum(deg) - deg
    codes = []
    for d in np.unique(deg[deg >= 2]):  # all points of one degree at once: their cameras ascend within a row
        cams = cam0[start[deg == d][:, None] + np.arange(d)[None, :]]
        lo, hi = np.triu_indices(d, 1)
        codes.append((cams[:, hi] * ncams + cams[:, lo]).ravel())
    code, count = np.unique(np.concatenate(codes), return_counts=True)
    pairs = {(int(c // ncams), int(c % ncams)): int(n) for c, n in zip(code, count)}
    ntasks = sum(pairs.values()) + int(cdeg.sum())  # the diagonal key (a, a) has one task per observation of camera a
    assert ntasks == int((deg * (deg + 1) // 2).sum())
    return deg, cdeg, pairs, ntasks


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_scene_p_has_its_point_degrees(ba):
    p = scenes.scene(ba, "P")
    deg, cdeg, pairs, ntasks = recount(p)
    start = np.cumsum(deg) - deg
    assert (p["ncams"], p["npnts"]) == (201, 327) and p["npnts"] == 5 * BATCH + 7
    assert np.array_equal(deg, scenes.p_degrees()) and chunk_of(ntasks) == 16
    assert np.all(deg[:63] == 1) and np.array_equal(start[:64], np.arange(64))
    assert deg[63] == 65 and start[63] % BATCH == BATCH - 1 and (start[63] + deg[63]) % BATCH == 0  # last row of a batch, all of the next
    assert start[64] == 2 * BATCH and tuple(deg[64:67]) == (2 * BATCH, 2 * BATCH + 1, 200)
    assert np.all(deg[67:128] == 0) and np.all(deg[128:192] == 0)  # the tail of wave 1, the whole of wave 2: no row
    assert set(deg[192:256]) == {2, 3} and deg[192:256].sum() % BATCH != 0
    assert set(deg[256:320]) == {2, 3, 4, 5}
    assert deg[326] == BATCH and deg[320:326].max() <= 3 and 0 in deg[320:326] and 1 in deg[320:326]
    assert cdeg[200] == 0 and np.all(cdeg[:200] > 0)


def test_scene_k16_has_its_key_lengths(ba):
    p = scenes.scene(ba, "K16")
    deg, cdeg, pairs, ntasks = recount(p)
    want = {k: L for k, L in scenes.k16_lengths().items() if L > 0}
    assert pairs == want and np.all(deg == 2) and p["ncams"] == 29
    ch = chunk_of(ntasks)
    assert ch == 16 and ntasks < 2 * 16 * 8192
    assert 13000 <= p["npnts"] <= 15000 and 39000 <= ntasks <= 45000
    hist = np.bincount(list(pairs.values()))
    assert all(hist[L] >= 9 for L in scenes.K_CYCLE16 if L > 0), "a length of the cycle is missing"
    n0 = sum(1 for L in scenes.k16_lengths().values() if L == 0)
    assert n0 >= 9 and len(pairs) == 276 + 4 - n0  # a pair of length 0 has no key
    # unsplit keys up to 2 chunk, exactly 2 chunk and one more; 63, 64, 65; a last chunk of one task
    assert {1, 2 * ch - 1, 2 * ch, 2 * ch + 1, 63, 64, 65} <= set(pairs.values())
    assert sorted(L for L in set(pairs.values()) if L > 2 * ch and L % ch == 1) == [33, 49, 65, 97, 129, 257]
    assert tuple(cdeg[24:29]) == (1, 255, 256, 257, 0)  # the extra cameras (their diagonal keys), the camera nobody sees
    assert all(pairs[(24 + i, 1)] == L for i, L in enumerate(scenes.K16_EXTRA))
    assert all(b == 1 for (a, b) in pairs if a >= 24)
    assert cdeg[:24].min() > 2 * ch  # every other diagonal key is split


def test_scene_k128_has_its_key_lengths(ba):
    p = scenes.scene(ba, "K128")
    deg, cdeg, pairs, ntasks = recount(p)
    ch = chunk_of(ntasks)
    per = 12 * 13 // 2
    assert ch == 128 and ntasks >= 1 << 20 and ntasks - per < 1 << 20, "the filler is sized to just above 2^20 tasks"
    assert chunk_of((1 << 20) - 1) == 64
    nfill = scenes.k128_fill_points()
    assert p["ncams"] == 36 and np.all(deg[:-nfill] == 2) and np.all(deg[-nfill:] == 12)
    directed = {k: L for k, L in pairs.items() if k[0] < 24}
    filler = {k: L for k, L in pairs.items() if k[0] >= 24}
    assert len(directed) == 276 and not any(b < 24 for (a, b) in filler)
    assert len(filler) == 66 and set(filler.values()) == {nfill} and np.all(cdeg[24:] == nfill) and nfill > 2 * ch
    hist = np.bincount(list(directed.values()))
    assert all(hist[L] >= 18 for L in scenes.K_CYCLE128) and set(directed.values()) == set(scenes.K_CYCLE128)
    # unsplit keys that take a second, third and fourth 64-task trip; exactly 2 chunk; one more: a last chunk of one task
    assert {65, 127, 128, 129, 191, 192, 193, 255, 256} <= {L for L in directed.values() if L <= 2 * ch}
    assert sorted(L for L in set(directed.values()) if L > 2 * ch) == [257, 258, 300] and 257 % ch == 1
    assert cdeg[:24].min() > 2 * ch


# ---- the dense numpy step -----------------------------------------------------------------------------------------------------
def reference(orc, p, name, lam):
    """dict(delta, model, grad, kappa) of the step (J'J + lam I) delta = -J'r through the explicit Schur complement
    (_lm_ref.step, solve="schur": scene K128 is too large for a dense solve); once per (scene, lambda), read-only"""
    return step_once(("graph_boundaries", name, lam), orc, p, p["x0"], lam, solve="schur")


def test_reference_step_solves_the_normal_equations(ba, orc):
    """The reference's own check (scene P, the smallest): its step satisfies (J'J + lam I) delta = -J'r to rounding, the points
    without an observation do not move, nor does the camera nobody sees."""
    p = scenes.scene(ba, "P")
    deg, cdeg, _, _ = recount(p)
    for lam in LAMBDAS:
        ref = reference(orc, p, "P", lam)
        J = jac(orc, p, p["x0"])
        res = J.T @ (J @ ref["delta"]) + lam * ref["delta"] + ref["grad"]
        assert np.linalg.norm(res) <= 1e-12 * np.linalg.norm(ref["grad"])
        assert np.all(ref["delta"][: 3 * p["npnts"]].reshape(-1, 3)[deg == 0] == 0.0)
        assert np.all(ref["delta"][3 * p["npnts"]:].reshape(-1, 9)[cdeg == 0] == 0.0)


def _check_step(tag, name, p, got, ref, lam, deg, cdeg):
    """one scene, one lambda: got = (LDL step, Float32-factor step, PCG step) as lm_step returns them"""
    (d, half, jtr), (d32, _, _), (dp, halfp, _, its) = got
    np3 = 3 * p["npnts"]
    kappa, d_ref = ref["kappa"], ref["delta"]
    lim, lim32, limp = limit(STEP_TOL[lam], kappa), limit(F32_TOL, kappa), limit(PCG_TOL, kappa)
    e, e32, ep = rel_err(d, d_ref), rel_err(d32, d_ref), rel_err(dp, d_ref)
    em = abs(half - ref["model"]) / ref["model"]
    emp = abs(halfp - ref["model"]) / ref["model"]
    eg = float(np.linalg.norm(jtr - ref["grad"]) / np.linalg.norm(ref["grad"]))
    lonely = np.flatnonzero(cdeg == 0)
    cams = lambda v: v[np3:].reshape(-1, 9)[lonely].ravel()  # noqa: E731
    ec, ec32, ecp = (float(np.linalg.norm(cams(v)) / np.linalg.norm(d_ref)) for v in (d, d32, dp))
    print(f"{tag} lambda {lam:g}: kappa {kappa:.3e}  LDL {e:.3e} (limit {lim:.1e})  f32 {e32:.3e} ({lim32:.1e})  pcg {ep:.3e} "
          f"({limp:.1e}, {its} its)  model {em:.3e}  pcg model {emp:.3e}  jtr {eg:.3e}  unobserved camera {ec:.3e} / {ec32:.3e} / {ecp:.3e}")
    parity_record(f"graph_boundaries[{tag}-{lam:g}]", kappa=kappa, ldl=e, ldl_limit=lim, f32=e32, f32_limit=lim32, pcg=ep, pcg_limit=limp,
                  model=em, pcg_model=emp, jtr=eg, cg_iters=its, unobserved_camera_ldl=ec, unobserved_camera_f32=ec32,
                  unobserved_camera_pcg=ecp)
    for what, v in (("LDL", d), ("Float32-factor", d32), ("PCG", dp), ("J'r", jtr)):
        assert np.all(np.isfinite(v)), f"{tag}, lambda {lam}: {what} has entries that are not finite"
        bad = np.flatnonzero(np.any(v[:np3].reshape(-1, 3)[deg == 0] != 0.0, axis=1))
        assert bad.size == 0, f"{tag}, lambda {lam}: {what} of {bad.size} points without an observation is not exactly 0"
    assert np.isfinite(half) and np.isfinite(halfp)
    assert e <= lim, f"{tag}, lambda {lam}: :LDL step {e:.3e} > {lim:.3e}"
    assert e32 <= lim32, f"{tag}, lambda {lam}: Float32-factor step {e32:.3e} > {lim32:.3e}"
    assert ep <= limp, f"{tag}, lambda {lam}: PCG step {ep:.3e} > {limp:.3e}"
    assert em <= 1e-10, f"{tag}, lambda {lam}: model value {half!r} vs {ref['model']!r}"
    assert emp <= 1e-7, f"{tag}, lambda {lam}: model value of the PCG step {halfp!r} vs {ref['model']!r}"
    assert eg <= 1e-12, f"{tag}, lambda {lam}: gradient {eg:.3e}"
    if lonely.size:
        assert ec <= lim and ec32 <= lim32 and ecp <= limp, f"{tag}, lambda {lam}: the unobserved camera moves: {ec:.3e} {ec32:.3e} {ecp:.3e}"


def _steps(ba, m, x, lam):
    return (ba.lm_step(m, x, lam), ba.lm_step(m, x, lam, facto_type=np.float32), ba.lm_step(m, x, lam, pcg=(1e-12, 5000)))


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_step_vs_dense_numpy(ba, orc, gpu_ok, name):
    """lm_step at lambda = 1 and 30 (normalize None): :LDL, facto_type = Float32, pcg = (1e-12, 5000) against the dense numpy
    step.  Limits: those of test_prior_step_vs_dense_numpy -- STEP_TOL / 5e-3 / 1e-8 or 100 kappa eps where that is larger, the
    model value to 1e-10 (1e-7 for the PCG step's own), J'r to 1e-12.  The step of a point without an observation is exactly
    0, that of a camera without one within the step's limit of 0."""
    p = scenes.scene(ba, name)
    deg, cdeg, _, _ = recount(p)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        got = {lam: _steps(ba, m, p["x0"], lam) for lam in LAMBDAS}
    finally:
        m.close()
    for lam in LAMBDAS:
        _check_step(name, name, p, got[lam], reference(orc, p, name, lam), lam, deg, cdeg)


@pytest.mark.gpu
def test_scene_p_unsorted_observations(ba, orc, gpu_ok):
    """Scene P with its observations permuted, as test_unsorted_observations does: the list-driven point kernels at the same
    degrees.  x keeps its layout, so the reference is the same step."""
    p = scenes.scene(ba, "P")
    deg, cdeg, _, _ = recount(p)
    perm = np.random.default_rng(3).permutation(p["nobs"])
    q = dict(p, cam_idx1=p["cam_idx1"][perm], pnt_idx1=p["pnt_idx1"][perm], pt2d=p["pt2d"].reshape(-1, 2)[perm].ravel())
    m = ba.BALNLPModel(arrays=arrays(q))
    try:
        got = {lam: _steps(ba, m, p["x0"], lam) for lam in LAMBDAS}
    finally:
        m.close()
    for lam in LAMBDAS:
        _check_step("P unsorted", "P", p, got[lam], reference(orc, p, "P", lam), lam, deg, cdeg)


@pytest.mark.gpu
def test_scene_p_covariance(ba, orc, gpu_ok):
    """ba.covariance with the gauge fixed (gauge_kw) and lambda = 1 against the inverse of the full dense matrix: the point
    blocks at 0, 1, ... 200 observations (a point nobody sees: I / lambda), the block of the camera nobody sees."""
    p = scenes.scene(ba, "P")
    lam = 1.0
    kw = gauge_kw(p)
    fixed = fixed_vector(ba, p, kw)
    m = ba.BALNLPModel(arrays=arrays(p))
    try:
        cams, pts, piv = ba.covariance(m, p["x0"], lam, **kw)
    finally:
        m.close()
    H = hessian(orc, p, p["x0"], lam, fixed)
    ref_c, ref_p = ref_dense(H, p, fixed)
    S, _, _ = schur(H, p)
    check_cov("graph_boundaries_covariance[P]", cams, pts, ref_c, ref_p, kappa_jacobi(S), fixed, p, lam=lam, min_rel_pivot=piv)


@pytest.mark.gpu
def test_scene_k16_loopback_two_ranks(ba, loopback):
    """Scene K16 sharded by point over 2 ranks of one process: the keys of a chunk of tile columns come through a list
    (k_schur_blocks' klist, k_schur_combine's slist).  The assertions of test_loopback_sharded_step_equals_one_rank."""
    p = scenes.scene(ba, "K16")
    ref = ba.BALNLPModel(arrays=arrays(p))
    try:
        d_ref, half_ref, _ = ba.lm_step(ref, p["x0"], 10.0)
    finally:
        ref.close()
    R = Ranks(ba, loopback, p, 2)
    try:
        d, cams, half = R.step(10.0)
        assert loopback.ba_loopback_ops(R.loop) > 0
    finally:
        R.close()
    e, em = rel_err(d, d_ref), abs(half - half_ref) / half_ref
    parity_record("graph_boundaries_loopback[K16]", step_vs_one_rank=e, model_vs_one_rank=em)
    assert e <= 1e-9, f"2 ranks, Float64: |delta - delta_one_rank| / |delta_one_rank| = {e:.3e} (limit 1e-9)"
    assert abs(half - half_ref) <= 1e-10 * half_ref, f"2 ranks: model value {half!r} vs {half_ref!r}"
    rep = bits_report(cams[0], cams[1], "camera step of rank 0 vs rank 1 (replicated solve)")
    assert not rep, rep
