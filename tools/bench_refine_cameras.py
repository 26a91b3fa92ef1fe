"""Cameras with the points held (ba_refine_cameras): time of the device-resident entry on the Dubrovnik and Venice
shapes, against the fixed-point LM solve on the same scene.

  refine   host clock around ba_refine_cameras_dev (no host copy, counts not fetched) + ba_synchronize, x restored before every
           call outside the timed window; median of `reps` after a warm-up; and the event time of the launch
           (profile class k_refine_cameras)
  lm       one Levenberg_Marquardt(..., fixed_points=all) solve from the same x0 with the small-step test at the same tolerance
           (srtol = xtol, every other test off): its loop time, iterations, and how far its cameras end from refine's (the
           largest relative difference of a camera block)

  --resect the same clocks around ba_resect_cameras_dev from an x0 whose camera poses are all NaN: the linear
           resection and the refinement from its poses; event times of both launches (profile classes k_resect_cameras and
           k_refine_cameras), the states, the most trials, and the sum of the cameras' costs against that of the refinement from
           the generator's x0.  No LM leg: nothing else starts from NaN poses.

  --ransac the same clocks around ba_ransac_cameras_dev (H = 128, m = 6, tau = 4 px, refits = 2) on the scene with 30 % of
           every camera's detections displaced by synthetic.add_outliers, the true points held, from NaN poses: event times of
           the consensus kernels (profile class k_ransac_cameras: hypotheses, select, rescore, mask), of the resections (the
           refits and the final one) and of the refinement; the share of cameras whose mask equals the truth; and beside it the
           --resect row of the outlier-free scene from the same session.

  --focal  with --resect (the default beside it) or --ransac: the _focal entries from an x0 whose cameras are NaN in all
           nine entries -- f is estimated by the linear stage and by every hypothesis (m = 8).  The same clocks and event times,
           and the relative error of f against the generator's cameras after the linear stage and after the refinement.

  --p3p    with --ransac: ba_ransac_cameras_p3p_dev (m = 3, everything else as --ransac) on the same scene, the same
           clocks, event times and shares; the outlier-free --resect row is left out (the --ransac run beside it has it).
  --outliers FRACTION   with --ransac: the share of every camera's detections that is displaced (default 0.3)
  --exact  with --ransac: the detections that are not displaced are the exact projections of the true scene, not the
           generator's (0.5 px of noise)

One JSON object per shape on stdout; all of them to profiles/refine_cameras_bench.json (--resect: profiles/resect_cameras_bench.json,
--ransac: profiles/ransac_cameras_bench.json, --focal: profiles/resect_focal_bench.json, --focal --ransac:
profiles/ransac_focal_bench.json, --ransac --p3p: profiles/ransac_p3p_run.json), or the file given.
usage: python tools/bench_refine_cameras.py [--resect | --ransac [--p3p] [--outliers FRACTION] [--exact]] [--focal] [out.json] [reps] [shape ...]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

XTOL = 1e-10
HBM_ACHIEVABLE_TBPS = 6.3


def measure(ba, name, reps):
    L, lib = ba._lib.lib(), ba._lib
    p = ba.synthetic.make_named(name)
    n, nc, nvar = p["npnts"], p["ncams"], len(p["x0"])
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    deg = np.bincount(p["cam_idx1"] - 1, minlength=nc)
    row = {"shape": name, "ncams": nc, "npnts": n, "nobs": p["nobs"], "xtol": XTOL, "degree_min": int(deg.min()),
           "degree_median": int(np.median(deg)), "degree_max": int(deg.max())}
    # one evaluation reads per observation its list entry, its point index, its measurement and its point (4 + 4 + 16 + 24 bytes)
    row["bytes_per_evaluation_MB"] = round(48.0 * p["nobs"] / 1e6, 2)
    d_x = C.c_void_p()
    lib.check(L.ba_dev_malloc(m.handle, 8 * nvar, C.byref(d_x)))
    x0 = np.ascontiguousarray(p["x0"])
    counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
    lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
    lib.check(L.ba_refine_cameras_dev(m.handle, d_x, -1, XTOL, -1.0, None, None, lib.ptr(counts), C.byref(its), None))  # warm-up
    wall = []
    for _ in range(reps):
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        t = time.perf_counter()
        lib.check(L.ba_refine_cameras_dev(m.handle, d_x, -1, XTOL, -1.0, None, None, None, None, None))
        lib.check(L.ba_synchronize(m.handle))
        wall.append(1e3 * (time.perf_counter() - t))
    m.profile(True)
    lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
    lib.check(L.ba_refine_cameras_dev(m.handle, d_x, -1, XTOL, -1.0, None, None, None, None, None))
    ev_ms = m.profile_get()["k_refine_cameras"][0]
    m.profile(False)
    lib.check(L.ba_dev_free(m.handle, d_x))
    med = statistics.median(wall)
    row["refine"] = {"call_ms_median": round(med, 3), "call_ms_all": [round(v, 3) for v in wall], "launch_event_ms": round(ev_ms, 3),
                     "iters_max": its.value, "counts": {k: int(v) for k, v in zip(lib.POINT_STATES + ("behind",), counts)},
                     "cameras_per_s": round(nc / (med * 1e-3))}
    # the time an HBM-bound kernel would need if every trial of the slowest camera streamed the whole scene once
    row["hbm_floor_ms"] = round((its.value + 1) * 48.0 * p["nobs"] / (HBM_ACHIEVABLE_TBPS * 1e12) * 1e3, 4)
    x_ref, info = ba.refine_cameras(m, x0, xtol=XTOL)
    row["objective_refine"] = float(np.sum(info["cost_after"]))
    t = time.perf_counter()
    st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, fixed_points=np.arange(1, n + 1),
                                srtol=XTOL, satol=0.0, oatol=0.0, ortol=0.0, atol=0.0, rtol=0.0, restol=0.0, ite_max=100, log=False)
    Cl, Cr = st.solution[3 * n:].reshape(-1, 9), x_ref[3 * n:].reshape(-1, 9)
    row["lm_fixed_points"] = {"status": st.status, "iterations": st.iter, "loop_ms": round(1e3 * st.loop_time, 2),
                              "call_ms": round(1e3 * (time.perf_counter() - t), 2),
                              "ms_per_iteration": round(1e3 * st.loop_time / max(st.iter, 1), 2), "objective": st.objective,
                              "cameras_differ_rel": float(np.max(np.linalg.norm(Cl - Cr, axis=1) / np.linalg.norm(Cr, axis=1)))}
    row["lm_loop_over_refine"] = round(row["lm_fixed_points"]["loop_ms"] / med, 1)
    row["refine_over_hbm_floor"] = round(ev_ms / row["hbm_floor_ms"], 1)
    m.close()
    return row


def focal_errors(x, p):
    """relative error of f against the generator's cameras: median and largest over the cameras with a finite f"""
    n, nc = p["npnts"], p["ncams"]
    f, ft = x[3 * n:].reshape(nc, 9)[:, 8], np.asarray(p["x_true"])[3 * n:].reshape(nc, 9)[:, 8]
    e = np.abs(f - ft)[np.isfinite(f)] / ft[np.isfinite(f)]
    return {"median": float(np.median(e)), "max": float(e.max()), "cameras": int(e.size)}


def measure_resect(ba, name, reps, focal=False):
    L, lib = ba._lib.lib(), ba._lib
    entry = L.ba_resect_cameras_focal_dev if focal else L.ba_resect_cameras_dev
    p = ba.synthetic.make_named(name)
    n, nc, nvar = p["npnts"], p["ncams"], len(p["x0"])
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    deg = np.bincount(p["cam_idx1"] - 1, minlength=nc)
    row = {"shape": name, "ncams": nc, "npnts": n, "nobs": p["nobs"], "xtol": XTOL, "degree_min": int(deg.min()),
           "degree_median": int(np.median(deg)), "degree_max": int(deg.max())}
    x0 = np.array(p["x0"], dtype=np.float64, copy=True)
    x0[3 * n:].reshape(nc, 9)[:, :(9 if focal else 6)] = np.nan
    d_x = C.c_void_p()
    lib.check(L.ba_dev_malloc(m.handle, 8 * nvar, C.byref(d_x)))
    counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
    lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
    lib.check(entry(m.handle, d_x, -1, XTOL, -1.0, None, None, lib.ptr(counts), C.byref(its), None))  # warm-up
    wall = []
    for _ in range(reps):
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        t = time.perf_counter()
        lib.check(entry(m.handle, d_x, -1, XTOL, -1.0, None, None, None, None, None))
        lib.check(L.ba_synchronize(m.handle))
        wall.append(1e3 * (time.perf_counter() - t))
    m.profile(True)
    lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
    lib.check(entry(m.handle, d_x, -1, XTOL, -1.0, None, None, None, None, None))
    prof = m.profile_get()
    m.profile(False)
    lib.check(L.ba_dev_free(m.handle, d_x))
    med = statistics.median(wall)
    row["resect"] = {"call_ms_median": round(med, 3), "call_ms_all": [round(v, 3) for v in wall],
                     "k_resect_cameras_event_ms": round(prof["k_resect_cameras"][0], 3),
                     "k_refine_cameras_event_ms": round(prof["k_refine_cameras"][0], 3), "iters_max": its.value,
                     "counts": {k: int(v) for k, v in zip(lib.POINT_STATES + ("behind",), counts)}}
    x1, info = ba.refine_cameras(m, x0, resect=True, estimate_focal=focal, xtol=XTOL)
    _, info0 = ba.refine_cameras(m, p["x0"], xtol=XTOL)
    if focal:
        row["focal"] = True
        row["f_error_linear"] = focal_errors(ba.refine_cameras(m, x0, resect=True, estimate_focal=True, max_iter=0)[0], p)
        row["f_error_refined"] = focal_errors(x1, p)
    row["objective_resect"] = float(np.sum(info["cost_after"]))
    row["objective_at_resected_poses"] = float(np.sum(info["cost_before"]))
    row["objective_refine_from_x0"] = float(np.sum(info0["cost_after"]))
    m.close()
    return row


RANSAC = dict(threshold=4.0, hypotheses=128, sample=6, refits=2, seed=0)
OUTLIER_FRACTION = 0.3


def measure_ransac(ba, name, reps, focal=False, p3p=False, fraction=OUTLIER_FRACTION, exact=False):
    L, lib = ba._lib.lib(), ba._lib
    entry = L.ba_ransac_cameras_p3p_dev if p3p else L.ba_ransac_cameras_focal_dev if focal else L.ba_ransac_cameras_dev
    options = dict(RANSAC, sample=3) if p3p else dict(RANSAC, sample=8) if focal else RANSAC
    p = ba.synthetic.make_named(name)
    n, nc, nvar, nobs = p["npnts"], p["ncams"], len(p["x0"]), p["nobs"]
    if exact:
        X, Cm = np.asarray(p["x_true"][:3 * n]).reshape(n, 3), np.asarray(p["x_true"][3 * n:]).reshape(nc, 9)
        p = dict(p, pt2d=np.ascontiguousarray(ba.synthetic.project(X[p["pnt_idx1"] - 1], Cm[p["cam_idx1"] - 1]).ravel()))
    pt2d, is_out = ba.synthetic.add_outliers(p, fraction=fraction, seed=1)
    q = dict(p, pt2d=np.ascontiguousarray(pt2d.ravel()))
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(q))
    cam0 = p["cam_idx1"] - 1
    deg = np.bincount(cam0, minlength=nc)
    row = {"shape": name, "ncams": nc, "npnts": n, "nobs": nobs, "xtol": XTOL, "degree_min": int(deg.min()),
           "degree_median": int(np.median(deg)), "degree_max": int(deg.max()), "outlier_fraction": fraction,
           "outliers": int(is_out.sum()), "options": options, "focal": focal, "p3p": p3p, "exact": exact}
    x0 = np.array(p["x_true"], dtype=np.float64, copy=True)  # the true points are held
    x0[3 * n:].reshape(nc, 9)[:, :(9 if focal else 6)] = np.nan
    opts = lib.ransac_opts(options, least=3, most=3, least_set=6) if p3p else lib.ransac_opts(options)
    d_x = C.c_void_p()
    lib.check(L.ba_dev_malloc(m.handle, 8 * nvar, C.byref(d_x)))
    counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
    tail = (None, None, None, None)

    def call(cnt=None, it=None):
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        t = time.perf_counter()
        lib.check(entry(m.handle, d_x, C.byref(opts), -1, XTOL, -1.0, None, None, cnt, it, *tail))
        lib.check(L.ba_synchronize(m.handle))
        return 1e3 * (time.perf_counter() - t)

    call(lib.ptr(counts), C.byref(its))  # warm-up
    wall = [call() for _ in range(reps)]
    m.profile(True)
    call()
    prof = m.profile_get()
    m.profile(False)
    lib.check(L.ba_dev_free(m.handle, d_x))
    med = statistics.median(wall)
    x, info = ba.refine_cameras(m, x0, resect=True, estimate_focal=focal, ransac=options, minimal="p3p" if p3p else None, xtol=XTOL)
    same = np.bincount(cam0, weights=(info["inliers"] != ~is_out).astype(float), minlength=nc) == 0
    C1, Ct = x[3 * n:].reshape(nc, 9), np.asarray(p["x_true"])[3 * n:].reshape(nc, 9)
    row["ransac"] = {"call_ms_median": round(med, 3), "call_ms_all": [round(v, 3) for v in wall],
                     "k_ransac_cameras_event_ms": round(prof["k_ransac_cameras"][0], 3), "k_ransac_cameras_scopes": int(prof["k_ransac_cameras"][1]),
                     "k_resect_cameras_event_ms": round(prof["k_resect_cameras"][0], 3), "k_resect_cameras_launches": int(prof["k_resect_cameras"][1]),
                     "k_refine_cameras_event_ms": round(prof["k_refine_cameras"][0], 3), "iters_max": its.value,
                     "counts": {k: int(v) for k, v in zip(lib.POINT_STATES + ("behind",), counts)},
                     "cameras_with_the_true_mask": int(same.sum()), "share_with_the_true_mask": round(float(same.mean()), 4),
                     "inliers_missed": int((~info["inliers"] & ~is_out).sum()), "outliers_kept": int((info["inliers"] & is_out).sum()),
                     "pose_error_rel_max": float(np.max(np.linalg.norm((C1 - Ct)[:, :6], axis=1) / np.linalg.norm(Ct[:, :6], axis=1))),
                     "objective": float(np.sum(info["cost_after"]))}
    if focal:
        row["f_error_refined"] = focal_errors(x, p)
    m.close()
    if not p3p:
        row["resect_outlier_free"] = measure_resect(ba, name, reps, focal)["resect"]
    return row


def main():
    args = sys.argv[1:]
    resect, ransac, focal, p3p, exact = ("--" + w in args for w in ("resect", "ransac", "focal", "p3p", "exact"))
    resect = resect or (focal and not ransac)
    fraction = OUTLIER_FRACTION
    if "--outliers" in args:
        at = args.index("--outliers")
        fraction = float(args[at + 1])
        del args[at:at + 2]
    if (p3p or exact or fraction != OUTLIER_FRACTION) and not ransac:
        sys.exit("bench_refine_cameras: --p3p, --outliers and --exact go with --ransac")
    if p3p and focal:
        sys.exit("bench_refine_cameras: --p3p needs the focal length (no --focal)")
    args = [a for a in args if a not in ("--resect", "--ransac", "--focal", "--p3p", "--exact")]
    default = "ransac_cameras_bench.json" if ransac else "resect_cameras_bench.json" if resect else "refine_cameras_bench.json"
    if focal:
        default = "ransac_focal_bench.json" if ransac else "resect_focal_bench.json"
    if p3p:
        default = "ransac_p3p_run.json"
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", default)
    reps = int(args.pop(0)) if args and args[0].isdigit() else 5
    shapes = args or ["dubrovnik-356", "venice-1778"]
    ba = ge.load_package()
    if ba.device_count() < 1:
        sys.exit("bench_refine_cameras: no HIP device visible (nothing is measured without one)")
    rows = []
    for name in shapes:
        row = measure_ransac(ba, name, reps, focal, p3p, fraction, exact) if ransac else measure_resect(ba, name, reps, focal) if resect else measure(ba, name, reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
