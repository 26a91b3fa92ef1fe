"""Cost of a robust loss (ba_lm_set_loss) on BAL shapes: the time of the reweighting pass (k_obs_scale, profile class k_robust_scale) per call (per-kernel
event timing, ba_profile_get) and its algorithmic traffic (416 bytes per observation: r and J read and written once), and the
ms per LM iteration of a huber solve against a linear one on the same handle (alternating, median of `reps` runs of `iters`
iterations each, after a warm-up solve).  One JSON object per shape on stdout; all of them to `out.json` when given.
usage: python tools/bench_robust.py [out.json] [iters] [reps] [shape ...]   (shapes default: venice-1778 dubrovnik-356)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

BYTES_PER_OBS = 416  # 2 x (16 B of residual + 192 B of Jacobian block)


def measure(ba, shape, iters, reps, f_scale=2.0):
    p = ba.synthetic.make_named(shape)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)

    def solve(loss):
        return ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, ite_max=iters, loss=loss, f_scale=f_scale, log=False)

    solve("huber")  # warm-up: camera ordering, workspace, first factorisation
    m.profile(True)
    solve("huber")
    ms, calls = m.profile_get()["k_robust_scale"]
    m.profile(False)
    per = {"linear": [], "huber": []}
    for _ in range(reps):
        for loss in per:
            st = solve(loss)
            per[loss].append(1e3 * st.loop_time / max(1, st.iter))
    m.close()
    t = ms / calls
    lin, hub = statistics.median(per["linear"]), statistics.median(per["huber"])
    return {"shape": shape, "nobs": p["nobs"], "f_scale": f_scale, "k_robust_scale_ms_per_call": round(t, 4),
            "k_robust_scale_calls": calls, "bytes_per_obs": BYTES_PER_OBS,
            "k_robust_scale_TBps": round(BYTES_PER_OBS * p["nobs"] / (t * 1e-3) / 1e12, 3),
            "iters_per_run": iters, "runs": reps, "ms_per_iter_linear": round(lin, 3), "ms_per_iter_huber": round(hub, 3),
            "huber_over_linear": round(hub / lin, 4), "ms_per_iter_linear_all": [round(v, 3) for v in per["linear"]],
            "ms_per_iter_huber_all": [round(v, 3) for v in per["huber"]]}


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else None
    iters = int(args.pop(0)) if args else 6
    reps = int(args.pop(0)) if args else 3
    shapes = args or ["venice-1778", "dubrovnik-356"]
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
