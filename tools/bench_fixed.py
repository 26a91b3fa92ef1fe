"""Cost of fixed parameters (ba_lm_set_fixed) on the Venice shape: the time of the masking pass k_fix_mask per call (per-kernel
event timing, ba_profile_get) with its algorithmic traffic, and the ms per LM iteration of three solves on the same handle
(alternating, median of `reps` runs of `iters` iterations each, after a warm-up solve of each):
  none        no mask (the unmasked path: no k_fix_mask launch)
  intrinsics  k1, k2, f fixed on every camera
  cam1+50%    camera 1 whole and every other point
One JSON object per shape on stdout; all of them to `out.json` when given.
usage: python tools/bench_fixed.py [out.json] [iters] [reps] [shape ...]   (shapes default: venice-1778)"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def mask_bytes(p, kw, ba):
    """algorithmic bytes of one k_fix_mask launch: the int32 indices it reads (8 B per observation when both tables are
    present, 4 B otherwise), a table entry per observation (2 B camera, 1 B point), 8 B stored per fixed Jacobian entry"""
    cam, pnt = ba._lib.fixed_masks(p["ncams"], p["npnts"], kw.get("fixed_cameras"), kw.get("fixed_points"),
                                   kw.get("fixed_camera_params"))
    c0, p0 = p["cam_idx1"] - 1, p["pnt_idx1"] - 1
    has_c, has_p = bool(cam.any()), bool(pnt.any())
    per_obs = 4 * (has_c + has_p) + 2 * has_c + has_p
    cols = np.array([bin(int(m)).count("1") for m in cam])[c0] + 3 * pnt[p0].astype(np.int64)
    return int(per_obs * p["nobs"] + 2 * 8 * cols.sum())


def measure(ba, shape, iters, reps):
    p = ba.synthetic.make_named(shape)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    fr = ba.FeasibilityResidual(m)
    masks = {"none": {}, "intrinsics": dict(fixed_camera_params=("k1", "k2", "f")),
             "cam1+50%": dict(fixed_cameras=[1], fixed_points=np.arange(1, p["npnts"] + 1, 2))}

    def solve(kw):
        return ba.Levenberg_Marquardt(fr, "LDL", "AMD", "None", False, ite_max=iters, log=False, **kw)

    row = {"shape": shape, "nobs": p["nobs"], "iters_per_run": iters, "runs": reps}
    for name, kw in masks.items():
        solve(kw)  # warm-up: camera ordering, workspace, recorded sequences of this mask
        if name != "none":
            m.profile(True)  # (resets the counters)
            solve(kw)
            ms, calls = m.profile_get()["k_fix_mask"]
            m.profile(False)
            t = ms / calls
            b = mask_bytes(p, kw, ba)
            row[f"k_fix_mask_ms_{name}"] = round(t, 4)
            row[f"k_fix_mask_bytes_per_obs_{name}"] = round(b / p["nobs"], 1)
            row[f"k_fix_mask_TBps_{name}"] = round(b / (t * 1e-3) / 1e12, 3)
    per = {name: [] for name in masks}
    for _ in range(reps):
        for name, kw in masks.items():
            st = solve(kw)
            per[name].append(1e3 * st.loop_time / max(1, st.iter))
    m.close()
    base = statistics.median(per["none"])
    for name in masks:
        med = statistics.median(per[name])
        row[f"ms_per_iter_{name}"] = round(med, 3)
        row[f"ms_per_iter_{name}_all"] = [round(v, 3) for v in per[name]]
        if name != "none":
            row[f"{name}_over_none"] = round(med / base, 4)
    return row


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else None
    iters = int(args.pop(0)) if args else 6
    reps = int(args.pop(0)) if args else 5
    shapes = args or ["venice-1778"]
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
