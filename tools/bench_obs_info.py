"""Cost of per-observation information (ba_lm_set_obs_info) on BAL shapes: the time of the per-observation pass k_obs_scale per call
(per-kernel event timing, ba_profile_get: class k_info_whiten) with an isotropic obs_info under the linear loss and under huber, beside
its time in a huber solve without information on the same handle (class k_robust_scale), and their algorithmic traffic (440 against 416 bytes
per observation: r and J read and written once, plus the three factors).  The pass also runs on the trial residual alone (40
bytes per observation); the two kinds of call are told apart by one lm_step (one call, r and J) beside a solve of `iters`
iterations.  One JSON object per shape on stdout; all of them to `out.json` when given.
usage: python tools/bench_obs_info.py [out.json] [iters] [shape ...]   (shapes default: venice-1778)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

BYTES_INFO, BYTES_ROBUST, BYTES_TRIAL = 440, 416, 40


def measure(ba, shape, iters, f_scale=2.0):
    p = ba.synthetic.make_named(shape)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)
    sigma = np.random.default_rng(0).choice([0.5, 1.0, 2.0, 4.0], p["nobs"])

    def profiled(name, ite_max, **kw):
        m.profile(True)
        st = ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, ite_max=ite_max, log=False, **kw)
        ms, calls = m.profile_get().get(name, (0.0, 0))
        m.profile(False)
        return ms, calls, st

    ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, ite_max=1, log=False)  # warm-up: ordering, workspace
    row = {"shape": shape, "nobs": p["nobs"], "f_scale": f_scale, "iters": iters}
    for loss in ("linear", "huber"):
        ba.lm_step(m, p["x0"], 1.0, want_jtr=False, loss=loss, f_scale=f_scale, obs_info=sigma)  # (first launch of this instantiation)
        m.profile(True)
        ba.lm_step(m, p["x0"], 1.0, want_jtr=False, loss=loss, f_scale=f_scale, obs_info=sigma)  # one linearisation, no trial point
        ms0, calls0 = m.profile_get()["k_info_whiten"]
        m.profile(False)
        ms, calls, st = profiled("k_info_whiten", iters, loss=loss, f_scale=f_scale, obs_info=sigma)
        full = ms0 / calls0
        n_full, n_trial = st.n_jacobian, st.n_factor
        trial = (ms - n_full * full) / n_trial if n_trial else 0.0
        row[f"k_info_whiten_{loss}_ms_per_call_r_and_J"] = round(full, 4)
        row[f"k_info_whiten_{loss}_TBps_r_and_J"] = round(BYTES_INFO * p["nobs"] / (full * 1e-3) / 1e12, 3)
        row[f"k_info_whiten_{loss}_ms_per_call_trial_residual"] = round(trial, 4)
        row[f"k_info_whiten_{loss}_calls"] = [int(calls0), int(calls), int(n_full), int(n_trial)]
    ba.lm_step(m, p["x0"], 1.0, want_jtr=False, loss="huber", f_scale=f_scale)  # (first launch of k_robust_scale)
    ms, calls, _ = profiled("k_robust_scale", iters, loss="huber", f_scale=f_scale)
    row["k_robust_scale_huber_ms_per_call"] = round(ms / calls, 4)
    row["k_robust_scale_huber_TBps"] = round(BYTES_ROBUST * p["nobs"] / (ms / calls * 1e-3) / 1e12, 3)
    row["k_robust_scale_calls"] = int(calls)
    m.close()
    return row


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else None
    iters = int(args.pop(0)) if args else 4
    shapes = args or ["venice-1778"]
    ba = ge.load_package()
    rows = []
    for shape in shapes:
        row = measure(ba, shape, iters)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
