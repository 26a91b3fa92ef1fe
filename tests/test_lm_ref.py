"""The numpy reference of the LM term tests (tests/_lm_ref.py) checked against itself, without a device."""
import numpy as np

from _lm_ref import step
from _util import bits_report


def test_neutral_elements_of_step_are_neutral(orc, small_prob):
    """Every term is an argument of step(): its neutral element -- identity information, no prior rows, nothing fixed, no group
    of two cameras -- gives the bits of the argument left out, one at a time and all together, at lambda = 1 and 30.  So a test that
    passes one term checks the neutral element of every other term, also of one added later."""
    p, x = small_prob, small_prob["x0"]
    eye = np.broadcast_to(np.eye(2), (p["nobs"], 2, 2)).copy()
    no_rows = dict(point_priors=(np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros((0, 3, 3))))
    nothing_fixed = np.zeros(len(x), dtype=bool)
    cases = [dict(info=eye), dict(priors=no_rows), dict(fixed=nothing_fixed), dict(groups=[[3], [7]]),
             dict(info=eye, priors={}, fixed=nothing_fixed, groups=[])]
    for lam in (1.0, 30.0):
        plain = step(orc, p, x, lam)
        for kw in cases:
            got = step(orc, p, x, lam, **kw)
            for name in ("delta", "model", "grad"):
                rep = bits_report(np.atleast_1d(got[name]), np.atleast_1d(plain[name]), f"lambda {lam:g}, {name} with {sorted(kw)}")
                assert not rep, rep
