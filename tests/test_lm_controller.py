"""The scalar controller of ba_lm_solve (csrc/ba_lm_controller.h) on the CPU: no test here needs a device.

The header is host only; tests/host/lm_controller_shim.cpp wraps it in a C ABI, compiled here into a temporary directory and
loaded with ctypes.  (a) what the header may include, (b) the defaults of src/lm.jl:20-26 and src/LevenbergMarquardt.jl:21-26
from the reference's formulas in numpy arithmetic, (c) scripted sums for the corners no real run reaches, (d) the closed loop:
the controller decides, a dense numpy Levenberg-Marquardt step built from the oracle's residuals and Jacobian provides the
sums, and the log is compared with the oracle's own run on the cases and with the tolerances of the GPU parity tests
(tests/test_gpu_parity.py), whose row comparisons are shared through tests/helpers/lm_rows.py."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from _util import parity_record as _report  # noqa: E402
from lm_rows import _TIGHT, _compare_rows, _float32_rows, _hard_start, _test_name, _well_conditioned_prefix  # noqa: E402

CSRC = os.path.join(ROOT, "bundleadjustment.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "ba_lm_controller.h")
ST = {"small_step": 0, "first_order": 1, "small_residual": 2, "acceptable": 3, "exception": 5, "max_iter": 6}  # BA_ST_*


class Sums(C.Structure):  # LMSums
    _fields_ = [(n, C.c_double) for n in ("rsq", "rtsq", "gsq", "xsq", "model", "rsq_trial", "deltasq")]


class Row(C.Structure):  # LMRow
    _fields_ = [("iter", C.c_int), ("f", C.c_double), ("df", C.c_double), ("norm_jtr", C.c_double), ("lam", C.c_double),
                ("norm_delta", C.c_double), ("rho", C.c_double), ("accepted", C.c_int)]


OPTIONS = ("restol", "satol", "srtol", "oatol", "ortol", "atol", "rtol", "nu_d", "nu_m", "delta_d")  # lmc_option's numbering


@pytest.fixture(scope="module")
def shim(ba, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    out = str(tmp_path_factory.mktemp("lm_controller") / "liblm_controller_shim.so")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", ROOT,
           os.path.join(ROOT, "tests", "host", "lm_controller_shim.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(out)
    vp, sp = C.c_void_p, C.POINTER(Sums)
    L.lmc_create.argtypes, L.lmc_create.restype = [C.POINTER(ba._lib.LMOpts), C.c_int, C.c_double], vp
    for name in ("destroy", "begin_iteration", "reject", "end_iteration"):
        getattr(L, "lmc_" + name).argtypes, getattr(L, "lmc_" + name).restype = [vp], None
    for name in ("done", "wants_halving", "accepted", "accept", "status", "iter", "lambda_width", "ite_max"):
        getattr(L, "lmc_" + name).argtypes, getattr(L, "lmc_" + name).restype = [vp], C.c_int
    for name in ("lambda", "c_r", "objective"):
        getattr(L, "lmc_" + name).argtypes, getattr(L, "lmc_" + name).restype = [vp], C.c_double
    L.lmc_start.argtypes, L.lmc_start.restype = [vp, sp, C.c_int], None
    L.lmc_judge.argtypes, L.lmc_judge.restype = [vp, sp], None
    L.lmc_refreshed.argtypes, L.lmc_refreshed.restype = [vp, sp], None
    L.lmc_step_norm.argtypes, L.lmc_step_norm.restype = [vp, sp], C.c_int
    L.lmc_halve.argtypes, L.lmc_halve.restype = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)], None
    L.lmc_row.argtypes, L.lmc_row.restype = [vp, C.POINTER(Row)], None
    L.lmc_option.argtypes, L.lmc_option.restype = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int
    return L


def _opts(ba, variant, linesearch=False, x_f32=False, ite_max=None, lam=None, **kw):
    """ba_lm_opts as Levenberg_Marquardt fills it: what is not given is the variant's default (negative)"""
    def d(name):
        return -1.0 if kw.get(name) is None else float(kw[name])
    assert set(kw) <= set(OPTIONS)
    return ba._lib.LMOpts(variant=variant, facto=0, normalize=0, linesearch=int(linesearch), facto_type=int(x_f32 and variant == 1),
                          ite_max=-1 if ite_max is None else ite_max, verbose=0, x_f32=int(x_f32), lam=-1.0 if lam is None else lam,
                          max_time=-1.0, pcg_tol=-1.0, pcg_max_iter=-1, perm=0, **{n: d(n) for n in OPTIONS})


class Controller:
    """one LMController behind the shim"""

    def __init__(self, L, opts, robust=False, cr0=1.0):
        self.L, self.h = L, L.lmc_create(C.byref(opts), int(robust), cr0)

    def __getattr__(self, name):
        fn = getattr(self.L, "lmc_" + name.rstrip("_"))  # (lambda_: the keyword)
        return lambda *a: fn(self.h, *a)

    def close(self):
        self.L.lmc_destroy(self.h)

    def option(self, name):
        v, w = C.c_double(), C.c_int()
        assert self.L.lmc_option(self.h, OPTIONS.index(name), C.byref(v), C.byref(w)) == 0
        return v.value, w.value

    def row_tuple(self):
        r = Row()
        self.L.lmc_row(self.h, C.byref(r))
        return (r.iter, r.f, r.df, r.norm_jtr, r.lam, r.norm_delta, r.rho, bool(r.accepted))


# ---- (a) what the controller may depend on -----------------------------------------------------------------------------------

def test_controller_header_is_host_only():
    text = open(HEADER).read()
    assert "#include <hip" not in text
    for word in ("ba_internal.h", "ba_lm_internal.h", "ba_problem", "LMWork", "hipStream_t"):
        assert word not in text, word
    assert "ts::" not in open(os.path.join(CSRC, "ba_lm.hip")).read()  # the typed scalar arithmetic lives in the header only


# ---- (b) defaults -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_defaults_follow_the_reference_formulas(ba, shim, variant, T):
    """src/lm.jl:20-26 and src/LevenbergMarquardt.jl:21-26 in numpy arithmetic of eltype(x) = T; a default is a T, a value the
    caller passes is a Float64 and wins."""
    eps = T(np.finfo(T).eps)
    sq = np.sqrt(eps)
    cbr = T(np.float64(eps) ** (1.0 / 3.0))  # eltype(x)(eps^(1/3)): a Float64 power, converted
    c100, c1000 = T(100) * sq, T(1000) * sq
    assert sq.dtype == c100.dtype == c1000.dtype == np.dtype(T)
    if variant == 1:
        want = dict(restol=cbr, satol=sq, srtol=sq, oatol=sq, ortol=cbr, atol=sq, rtol=cbr, nu_d=T(3), nu_m=T(3), delta_d=T(2))
        lam, ite_max = T(30), 200
    else:
        want = dict(restol=c100, satol=sq, srtol=sq, oatol=sq, ortol=c1000, atol=c100, rtol=c1000, nu_d=T(3), nu_m=T(3), delta_d=T(2))
        lam, ite_max = T(0.1), 100
    width = 32 if T is np.float32 else 64
    c = Controller(shim, _opts(ba, variant, x_f32=T is np.float32))
    for name, v in want.items():
        assert c.option(name) == (float(v), width), name
    assert (c.lambda_(), c.lambda_width(), c.ite_max()) == (float(lam), width, ite_max)
    c.close()
    given = {n: 0.5 + 0.015625 * k for k, n in enumerate(OPTIONS)}  # (0 is a value too: the tolerances of _TIGHT)
    given["restol"] = 0.0
    c = Controller(shim, _opts(ba, variant, x_f32=T is np.float32, ite_max=0, lam=0.7, **given))
    for name, v in given.items():
        assert c.option(name) == (v, 64), name
    assert (c.lambda_(), c.lambda_width(), c.ite_max()) == (0.7, 64, 0)
    c.close()


# ---- (c) scripted sums ----------------------------------------------------------------------------------------------------------

_QUIET = dict(restol=0.0, satol=0.0, srtol=0.0, oatol=0.0, ortol=0.0, atol=0.0, rtol=0.0)  # no stopping test can fire
_START = dict(rsq=4.0, rtsq=0.0, gsq=1e4, xsq=1.0, model=0.0, rsq_trial=0.0, deltasq=0.0)       # f = 2, |J'r| = 100
_GOOD = dict(_START, model=1.0, rsq_trial=0.25, deltasq=0.01)  # pred = 2 - 1/2, ared = 2 - 1/8: accepted
_BAD = dict(_START, model=1.0, rsq_trial=9.0, deltasq=1e-20)   # ared < 0: rejected, and 1 / |delta| = 1e10 above any lambda here


def _accepted_iteration(c, refreshed):
    c.begin_iteration()
    c.judge(Sums(**_GOOD))
    assert not c.wants_halving() and c.step_norm(Sums(**_GOOD)) and c.accepted()
    stop_known = c.accept()
    c.refreshed(Sums(**refreshed))
    c.end_iteration()
    return bool(stop_known)


@pytest.mark.parametrize("variant", [1, 0])
def test_all_fixed_returns_first_order_at_once(ba, shim, variant):
    c = Controller(shim, _opts(ba, variant, **_QUIET))
    c.start(Sums(**dict(_START, gsq=0.0)), 1)
    assert c.done() and c.status() == ST["first_order"] and c.iter() == 0  # the loop asks for no step
    assert np.isfinite(c.lambda_())  # (lm.jl:59's 1e10 / |J'r| is not formed from |J'r| = 0)
    c.close()


def test_nan_step_is_an_exception_status_not_an_error(ba, shim):
    c = Controller(shim, _opts(ba, 1, **_QUIET))
    c.start(Sums(**_START), 0)
    assert not c.done()
    c.begin_iteration()
    c.judge(Sums(**_GOOD))
    assert c.step_norm(Sums(**dict(_GOOD, deltasq=float("nan")))) == 0  # the device loop goes on to its loop test: no error code
    assert c.done() and c.status() == ST["exception"] and c.iter() == 1   # lm.jl:297-302,401-402: the iteration is counted
    c.close()


@pytest.mark.parametrize("variant", [1, 0])
def test_ite_max_zero_runs_exactly_one_iteration(ba, shim, variant):
    c = Controller(shim, _opts(ba, variant, ite_max=0, **_QUIET))
    c.start(Sums(**_START), 0)
    n = 0
    while not c.done() and n < 5:
        assert _accepted_iteration(c, _START)  # iter > ite_max is known before the refresh: no trial step goes out with it
        n += 1
    assert n == 1 and c.iter() == 1 and c.status() == ST["max_iter"]  # the test is iter > ite_max (lm.jl:382), not >=
    c.close()


@pytest.mark.parametrize("fire,status", [
    (dict(satol=10.0, atol=10.0), "small_step"),       # small_step and first_order
    (dict(atol=10.0, restol=1.0), "first_order"),      # first_order and small_residual
    (dict(restol=1.0, oatol=10.0), "small_residual"),  # small_residual and small_obj_change
    (dict(oatol=10.0, ite_max=0), "acceptable"),       # small_obj_change and tired
])
def test_two_stopping_tests_in_one_refresh_follow_the_reference_order(ba, shim, fire, status):
    """lm.jl:391-405: small_step, first_order, small_residual, acceptable, (exception,) max_iter.  From f = 2, |J'r| = 100 one
    accepted step to f = 1/8, |r| = 1/2, |delta| = 0.1, |J'r| = 1: each pair of options makes exactly its two tests fire."""
    c = Controller(shim, _opts(ba, 1, **dict(_QUIET, **fire)))
    c.start(Sums(**_START), 0)
    assert not c.done()
    _accepted_iteration(c, dict(_START, gsq=1.0))
    assert c.done() and c.status() == ST[status]
    c.close()


@pytest.mark.parametrize("linesearch", [False, True])
def test_float32_lambda_is_a_float32_until_the_first_accepted_step(ba, shim, linesearch):
    """lm.jl:59,308,337 for eltype(x) = Float32: lambda = T(max(30, 1e10 / |J'r|)); a rejected step multiplies in Float32,
    max(lambda, 1 / |delta|) * nu_m^(ntimes + 1); the Float64 literal of max(1.0e-8, lambda) promotes it at the first accept."""
    f32 = np.float32
    c = Controller(shim, _opts(ba, 1, linesearch=linesearch, x_f32=True, **_QUIET))
    c.start(Sums(**_START), 0)
    lam = f32(max(np.float64(30), np.float64(1e10) / np.float64(f32(np.sqrt(_START["gsq"])))))  # T(max(lambda, 1e10 / norm_Jtr))
    assert (c.lambda_(), c.lambda_width()) == (float(lam), 32)
    c.begin_iteration()
    c.judge(Sums(**_BAD))
    ntimes = 0
    while c.wants_halving():
        scale, c_r = C.c_double(), C.c_double()
        c.halve(C.byref(scale), C.byref(c_r))
        assert (scale.value, c_r.value) == (0.5, 1.0)  # delta_d = 2: the model recursion keeps c_r = 1 (lm.jl:275-277)
        c.judge(Sums(**_BAD))
        ntimes += 1
    assert ntimes == (4 if linesearch else 0)
    assert c.step_norm(Sums(**_BAD)) and not c.accepted()
    c.reject()
    c.end_iteration()
    norm_delta = f32(np.sqrt(_BAD["deltasq"]))
    lam = np.maximum(lam, f32(1) / norm_delta) * np.power(f32(3), f32(ntimes + 1))
    assert lam.dtype == np.dtype(f32) and lam > 1e10
    assert (c.lambda_(), c.lambda_width()) == (float(lam), 32)
    assert not _accepted_iteration(c, _START)
    lam = lam / f32(3) / f32(3)  # lm.jl:329-336: / nu_d, and once more as ared >= 0.9 pred; both still Float32 operations
    assert lam.dtype == np.dtype(f32)
    assert (c.lambda_(), c.lambda_width()) == (float(lam), 64)
    c.begin_iteration()
    c.judge(Sums(**_BAD))
    assert c.step_norm(Sums(**_BAD)) and not c.accepted()
    c.reject()
    assert (c.lambda_(), c.lambda_width()) == (max(float(lam), float(f32(1) / norm_delta)) * 3.0, 64)  # a Float64 product now
    c.close()


# ---- (d) closed loop against the oracle ---------------------------------------------------------------------------------------

class NumpyStep:
    """The sums a device iteration publishes, from a dense numpy Levenberg-Marquardt step on the oracle's residuals and
    Jacobian.  Float32 model: x is a Float32 vector, r and J come from the oracle's Float32 functions and are widened, the step
    is solved in Float64 and x + delta is rounded to Float32."""

    def __init__(self, orc, p, pt2d, x0):
        self.orc, self.p, self.pt2d, self.T = orc, p, pt2d, x0.dtype.type
        rows, cols = orc.jac_structure(p["cam_idx1"], p["pnt_idx1"], p["npnts"])
        self.rows, self.cols = rows - 1, cols - 1
        self.nequ, self.nvar = 2 * len(p["cam_idx1"]), len(x0)
        self.x = x0.copy()
        self.r = self.residual(self.x)
        self.linearise()

    def residual(self, x):
        p = self.p
        return self.orc.residuals(p["cam_idx1"], p["pnt_idx1"], x, self.pt2d, p["npnts"]).astype(np.float64)

    def linearise(self):
        p = self.p
        self.J = np.zeros((self.nequ, self.nvar))
        self.J[self.rows, self.cols] = self.orc.jac_coord(p["cam_idx1"], p["pnt_idx1"], self.x, p["npnts"]).astype(np.float64)
        self.g = self.J.T @ self.r
        self.H = self.J.T @ self.J
        x = self.x.astype(np.float64)
        self.lin = dict(rsq=float(self.r @ self.r), rtsq=0.0, gsq=float(self.g @ self.g), xsq=float(x @ x))

    def solve(self, lam):
        self.delta = np.linalg.solve(self.H + lam * np.eye(self.nvar), -self.g)

    def scale(self, s):
        self.delta = self.delta * s

    def sums(self, c_r=1.0, trial=True):
        if not trial:
            return Sums(model=0.0, rsq_trial=0.0, deltasq=0.0, **self.lin)
        self.x_trial = (self.x.astype(np.float64) + self.delta).astype(self.T)
        self.r_trial = self.residual(self.x_trial)
        m = self.J @ self.delta + c_r * self.r
        return Sums(model=float(m @ m), rsq_trial=float(self.r_trial @ self.r_trial), deltasq=float(self.delta @ self.delta), **self.lin)

    def accept(self):
        self.x, self.r = self.x_trial, self.r_trial
        self.linearise()


def closed_loop(ba, shim, step, opts):
    """the loop of lm_solve_impl with NumpyStep in the device's place: every decision is the controller's"""
    c = Controller(shim, opts)
    log = []
    c.start(step.sums(trial=False), 0)
    while not c.done():
        c.begin_iteration()
        if not opts.variant:
            log.append(c.row_tuple())
        step.solve(c.lambda_())
        s = step.sums(c.c_r())
        c.judge(s)
        while c.wants_halving():
            scale, c_r = C.c_double(), C.c_double()
            c.halve(C.byref(scale), C.byref(c_r))
            step.scale(scale.value)
            s = step.sums(c_r.value)
            c.judge(s)
        if not c.step_norm(s):
            continue
        if opts.variant:
            log.append(c.row_tuple())
        if not c.accepted():
            c.reject()
        else:
            c.accept()
            step.accept()
            c.refreshed(step.sums(trial=False))
        c.end_iteration()
    if not opts.variant:
        log.append(c.row_tuple())
    st = types.SimpleNamespace(log=log, iter=c.iter(), status=ba._lib.STATUS[c.status()], objective=c.objective(), lambda_final=c.lambda_())
    c.close()
    return st


def _acc(log):
    return "".join("a" if r[7] else "r" for r in log)


def _whole_run(st, st_ref, log_ref, orc):
    assert st.iter == st_ref.iter and st.status == orc.STATUS[st_ref.status]
    assert _acc(st.log) == _acc(log_ref)


CONVERGED = ("small_step", "first_order", "small_residual", "acceptable")


def _run64(ba, orc, shim, p, x0, variant, linesearch=False, **kw):
    rc, _, st_ref, log_ref = orc.lm_solve(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], x0, variant=variant,
                                          linesearch=linesearch, **kw)
    assert rc == 0
    st = closed_loop(ba, shim, NumpyStep(orc, p, p["pt2d"], x0), _opts(ba, variant, linesearch=linesearch, **kw))
    print(f"oracle: {st_ref.iter} {orc.STATUS[st_ref.status]} f = {st_ref.objective!r} {_acc(log_ref)}\n"
          f"closed loop: {st.iter} {st.status} f = {st.objective!r} {_acc(st.log)}")
    return st, st_ref, log_ref


@pytest.mark.parametrize("variant", [1, 0])
def test_closed_loop_float64_vs_oracle(ba, orc, shim, small_prob, variant):
    """test_lm_solve_vs_oracle's runs: the whole run is the oracle's, its rows to _compare_rows"""
    st, st_ref, log_ref = _run64(ba, orc, shim, small_prob, small_prob["x0"], variant)
    _whole_run(st, st_ref, log_ref, orc)
    _compare_rows(st, log_ref, _well_conditioned_prefix(log_ref))
    assert abs(st.objective - st_ref.objective) <= 1e-8 * st_ref.objective


@pytest.mark.parametrize("linesearch,nu_d,delta_d,want", [
    (False, 9.0, 2.0, "rej"),  # plain rejections: lambda = max(lambda, 1/|delta|) nu_m                 (lm.jl:308)
    (True, 9.0, 3.0, "ls"),    # line search with delta_d != 2: delta_r = (delta_r - r)/delta_d       (lm.jl:277)
    (True, 3.0, 3.0, "ls"),    # ... lambda /= nu_d^(ntimes-1)                                          (lm.jl:329-331)
    (True, 9.0, 1.5, "lbl"),   # delta_d < 2: the recursion's model value exceeds f: accepted, logged "rej" (lm.jl:260,292)
    (True, 9.0, 2.0, "any"),   # the reference's default delta_d
])
def test_closed_loop_rejections_and_linesearch_vs_oracle(ba, orc, shim, small_prob, linesearch, nu_d, delta_d, want):
    """test_lm_rejections_and_linesearch_vs_oracle's cases and `want` conditions.  delta_d = 1.5: two correct runs that part
    after the prefix (the oracle's sparse LDL' of the augmented system ends at max_iter after 41 iterations, the dense solve
    here converges in 16): there the prefix is compared, the run must end regularly and, if both converged, at the same
    minimum -- what the GPU test asks."""
    p = small_prob
    kw = dict(nu_d=nu_d, delta_d=delta_d, ite_max=40, **_TIGHT)
    st, st_ref, log_ref = _run64(ba, orc, shim, p, _hard_start(p), 1, linesearch, **kw)
    n = _well_conditioned_prefix(log_ref)
    acc = [bool(v) for v in log_ref[:n, 7]]
    lam = log_ref[:, 4]
    # an accepted row after which lambda did not shrink: ntimes = 1 in lm.jl:329-331, i.e. the line search ran
    ls_rows = [k for k in range(min(n, len(lam) - 1)) if acc[k] and lam[k + 1] >= lam[k] * 0.999]
    assert n >= 3
    if want == "rej":
        assert acc.count(False) >= 2 and not linesearch
    elif want == "ls":
        assert ls_rows
    elif want == "lbl":
        k = acc.index(False)
        assert lam[k + 1] < lam[k]  # logged "rej" (model value above f) yet the step was taken and lambda decreased
    _compare_rows(st, log_ref, n)
    if want == "lbl":
        assert st.status in CONVERGED + ("max_iter",)
    else:
        _whole_run(st, st_ref, log_ref, orc)
    if st_ref.status != 6 and st.status != "max_iter":  # both converged: same minimum
        assert abs(st.objective - st_ref.objective) <= 1e-6 * st_ref.objective


TOL32 = dict(oatol=1e-4, ortol=1e-4, atol=1e-4, rtol=1e-5, satol=1e-6, srtol=1e-7)  # src/diffprecsions.jl:22


def _run32(ba, orc, shim, p, x0, variant, linesearch=False, **kw):
    pt2d, x0 = p["pt2d"].astype(np.float32), x0.astype(np.float32)
    rc, _, st_ref, log_ref = orc.lm_solve_f32(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], pt2d, x0, variant=variant,
                                              linesearch=linesearch, **kw)
    assert rc == 0
    st = closed_loop(ba, shim, NumpyStep(orc, p, pt2d, x0), _opts(ba, variant, linesearch=linesearch, x_f32=True, **kw))
    print(f"oracle: {st_ref.iter} {orc.STATUS[st_ref.status]} f = {st_ref.objective!r} {_acc(log_ref)}\n"
          f"closed loop: {st.iter} {st.status} f = {st.objective!r} {_acc(st.log)}")
    return st, st_ref, log_ref


def _record32(st, log_ref, n):
    log = np.array([r[:7] + (float(r[7]),) for r in st.log])
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = {nm: float(np.nanmax(np.abs(log[:n, c] - log_ref[:n, c]) / np.abs(log_ref[:n, c])))
               for c, nm in ((1, "f"), (3, "norm_Jtr"), (4, "lambda"), (5, "norm_delta")) if np.any(log_ref[:n, c] != 0)}
    _report(_test_name(), rows=n, iterations=st.iter, **{f"dev_{nm}": v for nm, v in dev.items()})
    return log


@pytest.mark.parametrize("variant", [1, 0])
def test_closed_loop_float32_model_vs_oracle(ba, orc, shim, small_prob, variant):
    """test_lm_float32_model's runs (normalize :None) with its tolerances.  Variant 0 leaves the well-conditioned region within
    a few iterations (lambda = 0.1 / 3^k): the prefix is compared and the run must end converged, as the GPU test asks."""
    st, st_ref, log_ref = _run32(ba, orc, shim, small_prob, small_prob["x0"], variant, **TOL32)
    tag = f"variant {variant}"
    if variant == 1:
        _whole_run(st, st_ref, log_ref, orc)
        _record32(st, log_ref, len(log_ref))
        _float32_rows(st, log_ref, tag, f_rtol=1e-4)
        assert abs(st.objective - st_ref.objective) <= 1e-4 * st_ref.objective
        assert abs(st.lambda_final - st_ref.lambda_final) <= 1e-6 * st_ref.lambda_final
    else:
        n = _well_conditioned_prefix(log_ref)
        assert n >= 2, f"{tag}: only {n} well-conditioned rows"
        _record32(st, log_ref, n)
        _float32_rows(st, log_ref, tag, n=n, f_rtol=1e-3, lam_rtol=1e-6, delta_rtol=5e-3, g_rtol=1e-1)
        assert st.status in ("acceptable", "first_order", "small_step"), f"{tag}: status {st.status}"
        assert abs(st.objective - st_ref.objective) <= 1e-3 * st_ref.objective


def test_closed_loop_float32_defaults_stop_at_the_first_accepted_step(ba, orc, shim, small_prob):
    """eps(Float32)-derived default tolerances: satol + srtol |x| stops a BAL problem at its first accepted step"""
    st, st_ref, log_ref = _run32(ba, orc, shim, small_prob, small_prob["x0"], 1)
    _whole_run(st, st_ref, log_ref, orc)
    assert st.status == "small_step"


@pytest.mark.parametrize("linesearch", [False, True])
def test_closed_loop_float32_rejections_vs_oracle(ba, orc, shim, small_prob, linesearch):
    """test_lm_float32_model_rejections' runs with its tolerances"""
    p = small_prob
    st, st_ref, log_ref = _run32(ba, orc, shim, p, _hard_start(p), 1, linesearch, lam=1e-3, ite_max=12, **TOL32)
    n = _well_conditioned_prefix(log_ref)
    assert n >= 3
    if not linesearch:  # (with the line search the halved steps are accepted inside the iteration: no rejected row)
        assert np.any(log_ref[:n, 7] == 0), "the start must produce rejected steps inside the compared prefix"
    log = _record32(st, log_ref, min(n, len(st.log)))
    assert len(log) >= n
    assert [bool(v) for v in log[:n, 7]] == [bool(v) for v in log_ref[:n, 7]]
    err_f = np.abs(log[:n, 1] - log_ref[:n, 1]) / np.abs(log_ref[:n, 1])
    err_l = np.abs(log[:n, 4] - log_ref[:n, 4]) / np.abs(log_ref[:n, 4])
    assert err_f.max() <= 5e-3, f"f differs by {err_f.max():.2e} at row {int(err_f.argmax())}"
    assert err_l.max() <= 5e-3, f"lambda differs by {err_l.max():.2e} at row {int(err_l.argmax())}"
    _whole_run(st, st_ref, log_ref, orc)
