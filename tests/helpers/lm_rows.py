"""Row-by-row comparison of an LM run's log with the oracle's, and the starts / tolerances the comparisons share: used by the
GPU parity tests (tests/test_gpu_parity.py) and by the controller's closed loop on the CPU (tests/test_lm_controller.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _util import parity_record as _report  # noqa: E402


def _hard_start(p, sp=1.0, sc=0.3, seed=5):
    """x0 far from the solution (points +N(0, sp^2), rotations +N(0, sc^2), translations +N(0, (5 sc)^2)): with it the
    oracle's lm.jl run rejects steps at the first try, so the line search and the ntimes powers of the damping updates
    (src/lm.jl:264-295,308,329-331) actually execute."""
    rng = np.random.default_rng(seed)
    x = p["x0"].copy()
    npnts, ncams = p["npnts"], p["ncams"]
    x[:3 * npnts] += rng.standard_normal(3 * npnts) * sp
    c = x[3 * npnts:].reshape(-1, 9)
    c[:, :3] += rng.standard_normal((ncams, 3)) * sc
    c[:, 3:6] += rng.standard_normal((ncams, 3)) * sc * 5
    return x


_TIGHT = dict(rtol=1e-9, atol=1e-9, ortol=1e-12, oatol=0.0, restol=0.0, satol=0.0, srtol=1e-12)


def _test_name():
    return os.environ.get("PYTEST_CURRENT_TEST", "unknown").split("::")[-1].split(" ")[0]


def _well_conditioned_prefix(log_ref, lam_min=1e-2):
    """rows of an oracle log up to the first one whose damping is below lam_min.  Bundle adjustment has a 7-dimensional
    gauge null space: once lambda is tiny the damped system is nearly singular and two correct solvers (augmented sparse
    LDL' there, Schur complement + dense LDL' here) return steps that differ in the 4th-9th digit; from a start this far
    from the minimum the traces then drift apart (same accept/reject pattern, same final objective -- printed below).
    SURVEY 8d states the step tolerance for lambda >= 1e-4 x typical; the row-by-row comparison is made where it holds."""
    lam = log_ref[:, 4]
    small = np.flatnonzero(lam < lam_min)
    return int(small[0]) if small.size else len(lam)


# Row-by-row tolerances of a complete run against the oracle's, by the damping of the row ("for lambda >= 1e-4 x
# typical"; SURVEY 7 measured what two correct solvers -- augmented sparse LDL' and Schur complement + dense LDL' -- differ
# by in ONE step: 6e-13 at lambda = 1, 6e-10 at 1e-4; test_lm_step_vs_oracle: 7.6e-10 at 1e-4, cond(S) = 5e10).  Along a
# run the differences compound (every iterate starts from the previous one's), so a row's tolerance is wider than a step's:
# f, |J'r|, lambda, |delta| to 1e-6 while lambda >= 1e-2; down to lambda >= 1e-4 the accept / reject sequence must still be
# the oracle's and the four columns agree to _BAND2_RTOL (measured from the hard start of the rejection tests: 3.2e-3 in the
# worst column, 1e-8 in the rows above 1e-2 -- the per-column figures of every run are in the parity report).
_BAND2_LAM, _BAND2_RTOL = 1e-4, 1e-2


def _compare_rows(st, log_ref, n):
    log = np.array([r[:7] + (float(r[7]),) for r in st.log])
    assert len(log) >= n
    assert [bool(v) for v in log[:n, 7]] == [bool(v) for v in log_ref[:n, 7]]
    assert np.allclose(log[:n, [1, 3, 4, 5]], log_ref[:n, [1, 3, 4, 5]], rtol=1e-6)   # f, |J'r|, lambda, |delta|
    assert np.allclose(log[:n, 6], log_ref[:n, 6], rtol=1e-4, atol=1e-7)               # rho = ared/pred (pred cancels)

    def dev(a, b):
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if len(a) else 0.0

    names = {1: "f", 3: "norm_Jtr", 4: "lambda", 5: "norm_delta"}
    rec = {"rows_lambda_ge_1e-2": n}
    for c, nm in names.items():
        rec[f"dev_{nm}_lambda_ge_1e-2"] = dev(log[:n, c], log_ref[:n, c])
    n2 = min(_well_conditioned_prefix(log_ref, _BAND2_LAM), len(log), len(log_ref))
    if n2 > n:  # the rows with 1e-4 <= lambda < 1e-2
        rec.update({"rows_lambda_ge_1e-4": n2, "min_lambda_compared": float(log_ref[n:n2, 4].min()),
                    "same_accept_reject_1e-4_band": [bool(v) for v in log[n:n2, 7]] == [bool(v) for v in log_ref[n:n2, 7]]})
        for c, nm in names.items():
            rec[f"dev_{nm}_1e-4_band"] = dev(log[n:n2, c], log_ref[n:n2, c])
    _report(_test_name(), **rec)
    if n2 > n:
        assert rec["same_accept_reject_1e-4_band"], rec
        assert max(rec[f"dev_{nm}_1e-4_band"] for nm in names.values()) <= _BAND2_RTOL, rec


def _float32_rows(st, log_ref, tag, n=None, f_rtol=2e-5, lam_rtol=1e-6, delta_rtol=2e-3, g_rtol=2e-3):
    """Row-by-row comparison of a Float32-model run with the oracle's T = Float32 loop over the first n rows (default: all,
    and then the row counts must agree): accept / reject sequence equal, lambda to 1e-6 wherever it comes from the discrete
    updates (a rejected step's max(lambda, 1/|delta|) carries |delta|: delta_rtol there), f and |J'r| to Float32 level,
    |delta| to the accuracy of a Float32 factorisation."""
    log = np.array([r[:7] + (float(r[7]),) for r in st.log])
    if n is None:
        assert len(log) == len(log_ref), f"{tag}: {len(log)} log rows, oracle {len(log_ref)}"
        n = len(log)
    assert len(log) >= n and len(log_ref) >= n, f"{tag}: {len(log)} / {len(log_ref)} log rows, {n} to compare"
    acc, acc_ref = [bool(v) for v in log[:n, 7]], [bool(v) for v in log_ref[:n, 7]]
    assert acc == acc_ref, f"{tag}: accept/reject sequence {acc} vs oracle {acc_ref}"
    # (|J'r| falls by five orders of magnitude on the way to the minimum: what is left there is Float32 noise of the
    # Jacobian, 1e-5 of its starting value; it is compared on that floor)
    for col, name, rtol in ((1, "f", f_rtol), (3, "|J'r|", g_rtol), (5, "|delta|", delta_rtol)):
        floor = 1e-5 * abs(log_ref[0, col]) if col == 3 else 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(log[:n, col] - log_ref[:n, col]) / (np.abs(log_ref[:n, col]) + floor / rtol)  # <= rtol  <=>  |a - b| <= rtol |b| + floor
        err = np.where(log[:n, col] == log_ref[:n, col], 0.0, err)  # (LevenbergMarquardt.jl logs |delta| = 0 in its first row)
        k = int(np.argmax(err))
        assert err[k] <= rtol, f"{tag}: {name} row {k}: {log[k, col]!r} vs oracle {log_ref[k, col]!r} (relative {err[k]:.2e} > {rtol:g})"
    for k in range(n):
        after_reject = k > 0 and not acc_ref[k - 1]
        rtol = delta_rtol if after_reject else lam_rtol
        e = abs(log[k, 4] - log_ref[k, 4]) / log_ref[k, 4]
        assert e <= rtol, f"{tag}: lambda row {k}: {log[k, 4]!r} vs oracle {log_ref[k, 4]!r} (relative {e:.2e} > {rtol:g})"
