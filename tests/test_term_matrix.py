"""Which optional term of the LM problem is refused with which use of the handle: the whole matrix, cell by cell, at the Python
layer (before any device call) and at the C entries (ba_lm_solve, the three step entries, ba_covariance).  The expected matrix
is the literal below; it is not read from the package.  R: refused -- ValueError / BA_ERR_ARG naming the term and
the condition; -: accepted.  Every refusal returns before the device is used; the accepted cells of the device part run one LM
iteration (or one step) on small_prob."""
import ctypes as C

import numpy as np
import pytest

from _lm_run import arrays, attach_loopback, lm_opts, loopback_world
from _util import bits_report

CONDITIONS = ("linesearch", "x_f32", "facto_f32", "facto_f16", "normalize", "comm", "covariance")
#                        linesearch  Float32 model  facto Float32  facto Float16  normalize  communicator  ba_covariance
MATRIX = {
    "robust loss":      ("R",        "R",           "-",           "R",           "-",       "-",          "-"),
    "fixed parameters": ("-",        "-",           "-",           "R",           "-",       "-",          "-"),
    "priors":           ("R",        "R",           "-",           "R",           "-",       "R",          "-"),
    "shared intrinsics": ("R",       "R",           "R",           "R",           "R",       "R",          "R"),
}
# the condition's text in a C message, as the device tests of the terms spell it
TEXT = {"linesearch": ("linesearch = true",), "x_f32": ("Float32 model",), "facto_f32": ("facto_type", "Float32"),
        "facto_f16": ("facto_type", "Float16"), "normalize": ("normalize",), "comm": ("communicator",), "covariance": ("ba_covariance",)}
PY_NAME = {"robust loss": "robust loss", "fixed parameters": "fixed parameters", "priors": "priors",
           "shared intrinsics": "shared_intrinsics"}
GROUPS = [[1, 2]]


def _refused(term, cond):
    return MATRIX[term][CONDITIONS.index(cond)] == "R"


def _keyword(term):
    """the term's smallest valid keyword"""
    return {"robust loss": dict(loss="huber"), "fixed parameters": dict(fixed_cameras=[1]),
            "priors": dict(point_priors=(np.array([1]), np.zeros((1, 3)), np.ones((1, 3)))),
            "shared intrinsics": dict(shared_intrinsics=GROUPS)}[term]


def test_matrix_literal_is_complete():
    assert all(len(row) == len(CONDITIONS) and set(row) <= {"R", "-"} for row in MATRIX.values())
    assert sum(row.count("R") for row in MATRIX.values()) == 15


# ---- CPU: the Python layer, no model ---------------------------------------------------------------------------------------
# (condition, normalize, linesearch, facto_type) of the conditions that need no model
_PY_CASES = [("linesearch", "None", True, None), ("facto_f32", "None", False, np.float32), ("facto_f16", "None", False, np.float16),
             ("normalize", "J", False, None), ("normalize", ":A", False, None)]


@pytest.mark.parametrize("term", list(MATRIX))
@pytest.mark.parametrize("cond,normalize,linesearch,facto_type", _PY_CASES)
def test_levenberg_marquardt_refuses_the_matrix_before_the_model(ba, term, cond, normalize, linesearch, facto_type):
    """model=None: an R cell is a ValueError naming the term; a - cell gets past the term checks to the TypeError about the
    model."""
    def call():
        ba.Levenberg_Marquardt(None, "LDL", "AMD", normalize, linesearch, facto_type=facto_type, **_keyword(term))

    if _refused(term, cond):
        with pytest.raises(ValueError, match=PY_NAME[term]):
            call()
    else:
        with pytest.raises(TypeError, match="model must be"):
            call()


@pytest.mark.parametrize("term", list(MATRIX))
def test_lm_step_refuses_the_matrix_before_the_model(ba, term):
    """nlp=None, facto_type = Float32: the R cell is a ValueError naming the term; a - cell gets past the term checks and fails
    on the first look at the model (None has no attribute)."""
    if _refused(term, "facto_f32"):
        with pytest.raises(ValueError, match=PY_NAME[term]):
            ba.lm_step(None, np.zeros(3), 1.0, facto_type=np.float32, **_keyword(term))
    else:
        with pytest.raises((AttributeError, TypeError)):
            ba.lm_step(None, np.zeros(3), 1.0, facto_type=np.float32, **_keyword(term))


# ---- GPU: the C entries ----------------------------------------------------------------------------------------------------
def _set_term(ba, m, p, term):
    """`term` alone on the handle, through the per-term setters (None: no term)"""
    L, h = ba._lib, m.handle
    L.set_loss(h, "huber" if term == "robust loss" else "linear", 1.0)
    L.set_fixed(h, *L.fixed_masks(p["ncams"], p["npnts"], [1] if term == "fixed parameters" else None))
    pri = (np.array([1]), p["x0"][None, :3], np.ones((1, 3))) if term == "priors" else None
    L.set_priors(h, p["ncams"], p["npnts"], point_priors=pri)
    L.set_shared(h, L.shared_labels(GROUPS if term == "shared intrinsics" else None, p["ncams"]))


def _expect(ba, rc, term, cond, what):
    msg = ba._lib.lib().ba_last_error().decode()
    if _refused(term, cond):
        assert rc == 1, f"{what}: {term} x {cond} must be refused, rc = {rc}"
        assert term in msg and all(t in msg for t in TEXT[cond]), f"{what}: {term} x {cond}: {msg!r}"
    else:
        assert rc == 0, f"{what}: {term} x {cond} must be accepted, rc = {rc}: {msg!r}"


@pytest.mark.gpu
def test_c_entries_refuse_the_matrix(ba, small_prob, gpu_ok):
    p = small_prob
    lib = ba._lib.lib()
    x0 = ba.tie_intrinsics(p["x0"], p["npnts"], GROUPS)  # (what the grouping asks of x; valid for every other term too)
    no_cb = C.cast(None, ba._lib.LOG_CB)
    columns = [("linesearch", dict(linesearch=1)), ("x_f32", dict(x_f32=1)), ("facto_f32", dict(facto_type=1)),
               ("facto_f16", dict(facto_type=2)), ("normalize", dict(normalize=1)), ("comm", {})]

    def solve(m, **kw):
        x, o, st = x0.copy(), lm_opts(ba, ite_max=1, **kw), ba._lib.LMStats()
        rc = lib.ba_lm_solve(m.handle, C.byref(o), ba._lib.ptr(x), C.byref(st), no_cb, None)
        assert rc == 0 or np.array_equal(x, x0), "a refused solve changed x"
        return rc

    def step(m, entry):
        d, half, its = np.empty_like(x0), C.c_double(0), C.c_int(0)
        if entry == "ba_lm_step_pcg":
            return lib.ba_lm_step_pcg(m.handle, ba._lib.ptr(x0), 1.0, 1e-8, 100, ba._lib.ptr(d), C.byref(half), None, C.byref(its))
        return getattr(lib, entry)(m.handle, ba._lib.ptr(x0), 1.0, ba._lib.ptr(d), C.byref(half), None)

    m = ba.BALNLPModel(arrays=arrays(p))
    mc = ba.BALNLPModel(arrays=arrays(p))
    try:
        with loopback_world(1, 16 << 20) as (L, loop):
            try:
                attach_loopback(ba, mc, L, loop, 0, 1)  # before the handle's first solve, as documented
                before = ba.lm_step(m, x0, 1.0)
                for term in MATRIX:
                    _set_term(ba, m, p, term)
                    _set_term(ba, mc, p, term)
                    for cond, kw in columns:
                        _expect(ba, solve(mc if cond == "comm" else m, **kw), term, cond, "ba_lm_solve")
                    for entry in ("ba_lm_step", "ba_lm_step_pcg", "ba_lm_step_f32"):
                        _expect(ba, step(mc, entry), term, "comm", entry + " with a communicator")
                    _expect(ba, step(m, "ba_lm_step_f32"), term, "facto_f32", "ba_lm_step_f32")
                    _expect(ba, lib.ba_covariance(m.handle, ba._lib.ptr(x0), 1.0, -1.0, None, None, None), term, "covariance",
                            "ba_covariance")
                _set_term(ba, m, p, None)
                after = ba.lm_step(m, x0, 1.0)
                for a, b, name in zip(after, before, ("delta", "half_sq_model", "jtr")):
                    rep = bits_report(np.atleast_1d(a), np.atleast_1d(b), f"{name} of a plain step after the sweep vs before it")
                    assert not rep, rep
            finally:
                mc.close()  # (before its communicator goes)
    finally:
        m.close()
