"""Cost of Gaussian priors (ba_lm_set_priors) on BAL shapes: centre priors on every camera (GPS) and point priors on
1 % of the points (control points), against the same build without priors on the same handle.  Per shape: the time of the prior
kernels per launch scope (per-kernel event timing, ba_profile_get: k_prior, one scope per linearisation and two per linear step)
and the ms per LM iteration with and without priors (alternating, median of `reps` runs of `iters` iterations each, after a
warm-up solve).  One JSON object per shape on stdout; all of them to `out.json` when given.
usage: python tools/bench_priors.py [out.json] [iters] [reps] [shape ...]   (shapes default: ladybug-49 venice-1778)"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def centres(x, npnts, ncams):
    """c = -R(r)' t of every camera (numpy, vectorised)"""
    cams = x[3 * npnts:].reshape(ncams, 9)
    r, t = cams[:, :3], cams[:, 3:6]
    th = np.linalg.norm(r, axis=1, keepdims=True)
    k = r / th
    kt = np.cross(k, t)
    return -(np.cos(th) * t - np.sin(th) * kt + (1 - np.cos(th)) * np.sum(k * t, axis=1, keepdims=True) * k)


def measure(ba, shape, iters, reps):
    p = ba.synthetic.make_named(shape)
    ncams, npnts = p["ncams"], p["npnts"]
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)
    rng = np.random.default_rng(1)
    pidx = np.sort(rng.choice(npnts, max(1, npnts // 100), replace=False)) + 1
    pri = dict(centre_priors=(np.arange(1, ncams + 1), centres(p["x_true"], npnts, ncams) + 0.01 * rng.standard_normal((ncams, 3)),
                              np.full((ncams, 3), 0.01)),
               point_priors=(pidx, p["x_true"][:3 * npnts].reshape(-1, 3)[pidx - 1], np.full((len(pidx), 3), 0.005)))

    def solve(with_priors):
        return ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, ite_max=iters, log=False, **(pri if with_priors else {}))

    solve(True)  # warm-up: camera ordering, workspace, first factorisation
    m.profile(True)
    solve(True)
    ms, calls = m.profile_get()["k_prior"]
    m.profile(False)
    per = {"none": [], "priors": []}
    for _ in range(reps):
        for name in per:
            st = solve(name == "priors")
            per[name].append(1e3 * st.loop_time / max(1, st.iter))
    m.close()
    none, with_p = statistics.median(per["none"]), statistics.median(per["priors"])
    return {"shape": shape, "ncams": ncams, "npnts": npnts, "nobs": p["nobs"], "centre_priors": ncams, "point_priors": len(pidx),
            "k_prior_ms_per_scope": round(ms / calls, 4), "k_prior_scopes": calls, "iters_per_run": iters, "runs": reps,
            "ms_per_iter_none": round(none, 3), "ms_per_iter_priors": round(with_p, 3), "priors_over_none": round(with_p / none, 4),
            "ms_per_iter_none_all": [round(v, 3) for v in per["none"]], "ms_per_iter_priors_all": [round(v, 3) for v in per["priors"]]}


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else None
    iters = int(args.pop(0)) if args else 6
    reps = int(args.pop(0)) if args else 5
    shapes = args or ["ladybug-49", "venice-1778"]
    ba = ge.load_package()
    rows = []
    for shape in shapes:
        row = measure(ba, shape, iters, reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
