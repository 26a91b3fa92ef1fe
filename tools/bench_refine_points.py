"""Points with the cameras held (ba_refine_points): time of the device-resident entry on the Dubrovnik and Venice
shapes from two starts -- the points of x0, and triangulate=True -- beside the only way the library had before: one
Levenberg_Marquardt solve with every camera fixed, run to the same step tolerance on the same scene.
  refine   host clock around ba_refine_points_dev (no host copy, counts not fetched) + ba_synchronize, x restored before every
           repetition outside the timed window; median of `reps` after a warm-up call; and the event time of the launch pair
           (profile class k_refine_points: k_cam_pre + k_refine_points)
  lm       Levenberg_Marquardt(..., fixed_cameras=all, srtol=xtol, every other tolerance 0): its loop time and iterations
  floor    the bytes the kernel must fetch from HBM once (indices, measurements, points in and out: the camera rows, 128 B x
           ncams, stay in L2) over the achievable 6.3 TB/s: what an HBM-bound kernel would take
One JSON object per shape on stdout; all of them to profiles/refine_points_bench.json (or the file given).
--ransac measures the consensus stage instead (ba_ransac_points): the same shapes under their true cameras with 30 % of
every track displaced by 100..500 px (synthetic.add_point_outliers), tau = 4 px, H = 128, refits 2.
  ransac   host clock around ba_ransac_points_dev + ba_synchronize as above, and the event times of its two profile classes:
           k_ransac_points (k_cam_pre + k_ransac_points + k_ransac_mask_info) and k_refine_points (the finish)
  plain    ba_refine_points_dev(init = 1) on the same scene, outliers and all: the code that existed before, the yardstick
  true_set the share of points whose final set is exactly their undisplaced detections; hypotheses: the pairs the call scores
           (min(d (d - 1) / 2, H) per point) and the projections that takes (times d)
All of them to profiles/ransac_points_bench.json (or the file given).  --hypotheses N and --refits N replace H and the refits
(where the time of the consensus stage goes: fewer sampled pairs, no refit passes).
usage: python tools/bench_refine_points.py [--ransac [--hypotheses N] [--refits N]] [out.json] [reps] [shape ...]"""
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
    n, nvar = p["npnts"], len(p["x0"])
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    deg = np.bincount(p["pnt_idx1"] - 1, minlength=n)
    row = {"shape": name, "ncams": p["ncams"], "npnts": n, "nobs": p["nobs"], "xtol": XTOL, "degree_max": int(deg.max()),
           "points_above_tier_32": int((deg > 32).sum())}
    hbm_bytes = 24.0 * p["nobs"] + (4 + 4 + 2 * 24) * n
    row["hbm_floor_ms"] = round(hbm_bytes / (HBM_ACHIEVABLE_TBPS * 1e12) * 1e3, 4)
    row["camera_rows_MB"] = round(128 * p["ncams"] / 1e6, 3)
    d_x = C.c_void_p()
    lib.check(L.ba_dev_malloc(m.handle, 8 * nvar, C.byref(d_x)))
    x0 = np.ascontiguousarray(p["x0"])
    for start, init in (("x0", 0), ("triangulate", 1)):
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        lib.check(L.ba_refine_points_dev(m.handle, d_x, init, -1, XTOL, -1.0, None, None, lib.ptr(counts), C.byref(its), None))  # warm-up
        wall = []
        for _ in range(reps):
            lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
            t = time.perf_counter()
            lib.check(L.ba_refine_points_dev(m.handle, d_x, init, -1, XTOL, -1.0, None, None, None, None, None))
            lib.check(L.ba_synchronize(m.handle))
            wall.append(1e3 * (time.perf_counter() - t))
        m.profile(True)
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        lib.check(L.ba_refine_points_dev(m.handle, d_x, init, -1, XTOL, -1.0, None, None, None, None, None))
        ev_ms = m.profile_get()["k_refine_points"][0]
        m.profile(False)
        row[start] = {"call_ms_median": round(statistics.median(wall), 3), "call_ms_all": [round(v, 3) for v in wall],
                      "launch_pair_event_ms": round(ev_ms, 3), "iters_max": its.value,
                      "counts": {k: int(v) for k, v in zip(lib.POINT_STATES + ("behind",), counts)},
                      "points_per_s": round(n / (statistics.median(wall) * 1e-3))}
    lib.check(L.ba_dev_free(m.handle, d_x))
    x_ref, info = ba.refine_points(m, x0, xtol=XTOL)
    row["objective_refine"] = float(np.sum(info["cost_after"]))
    t = time.perf_counter()
    st = ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), "LDL", "AMD", "None", False, fixed_cameras=np.arange(1, p["ncams"] + 1),
                                srtol=XTOL, satol=0.0, oatol=0.0, ortol=0.0, atol=0.0, rtol=0.0, restol=0.0, ite_max=100, log=False)
    row["lm_fixed_cameras"] = {"status": st.status, "iterations": st.iter, "loop_ms": round(1e3 * st.loop_time, 2),
                               "call_ms": round(1e3 * (time.perf_counter() - t), 2), "ms_per_iteration": round(1e3 * st.loop_time / max(st.iter, 1), 2),
                               "objective": st.objective,
                               "points_differ_rel": float(np.max(np.linalg.norm((st.solution - x_ref)[:3 * n].reshape(-1, 3), axis=1)
                                                                 / np.linalg.norm(x_ref[:3 * n].reshape(-1, 3), axis=1)))}
    row["lm_loop_over_refine"] = round(row["lm_fixed_cameras"]["loop_ms"] / row["x0"]["call_ms_median"], 1)
    row["refine_over_hbm_floor"] = round(row["x0"]["launch_pair_event_ms"] / row["hbm_floor_ms"], 1)
    m.close()
    return row


RANSAC = dict(threshold=4.0, hypotheses=128, refits=2, seed=0)
OUTLIER_FRACTION = 0.3


def measure_ransac(ba, name, reps):
    L, lib = ba._lib.lib(), ba._lib
    p = ba.synthetic.make_named(name)
    n, nvar, nobs = p["npnts"], len(p["x0"]), p["nobs"]
    pt2d, outlier = ba.synthetic.add_point_outliers(p, fraction=OUTLIER_FRACTION, seed=0)
    p = dict(p, pt2d=np.ascontiguousarray(pt2d.ravel()))
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    pnt0 = p["pnt_idx1"] - 1
    deg = np.bincount(pnt0, minlength=n)
    pairs = np.minimum(deg * (deg - 1) // 2, RANSAC["hypotheses"])
    row = {"shape": name, "ncams": p["ncams"], "npnts": n, "nobs": nobs, "xtol": XTOL, "degree_max": int(deg.max()),
           "points_above_tier_32": int((deg > 32).sum()), "outlier_fraction": OUTLIER_FRACTION, "outliers": int(outlier.sum()),
           "options": RANSAC, "hypotheses_scored": int(pairs.sum()), "projections_scored": int((pairs * deg).sum()),
           "points_sampled_not_exhaustive": int((deg * (deg - 1) // 2 > RANSAC["hypotheses"]).sum())}
    x0 = np.ascontiguousarray(p["x_true"])  # (the true cameras; the points are not read)
    opts = lib.ransac_opts(RANSAC, least=2, most=2, least_set=2)
    d_x, d_in = C.c_void_p(), C.c_void_p()
    lib.check(L.ba_dev_malloc(m.handle, 8 * nvar, C.byref(d_x)))
    lib.check(L.ba_dev_malloc(m.handle, nobs, C.byref(d_in)))

    def call(which, counts=None, its=None):
        if which == "ransac":
            return L.ba_ransac_points_dev(m.handle, d_x, C.byref(opts), -1, XTOL, -1.0, None, None, counts, its, d_in, None, None, None)
        return L.ba_refine_points_dev(m.handle, d_x, 1, -1, XTOL, -1.0, None, None, counts, its, None)

    for which in ("ransac", "plain"):
        counts, its = np.zeros(7, dtype=np.int64), C.c_int(0)
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        lib.check(call(which, lib.ptr(counts), C.byref(its)))  # warm-up
        wall = []
        for _ in range(reps):
            lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
            t = time.perf_counter()
            lib.check(call(which))
            lib.check(L.ba_synchronize(m.handle))
            wall.append(1e3 * (time.perf_counter() - t))
        m.profile(True)
        lib.check(L.ba_memcpy_h2d(m.handle, d_x, lib.ptr(x0), 8 * nvar))
        lib.check(call(which))
        prof = m.profile_get()
        m.profile(False)
        row[which] = {"call_ms_median": round(statistics.median(wall), 3), "call_ms_all": [round(v, 3) for v in wall],
                      "finish_event_ms": round(prof["k_refine_points"][0], 3), "iters_max": its.value,
                      "counts": {k: int(v) for k, v in zip(lib.POINT_STATES + ("behind",), counts)}}
        if which == "ransac":
            row[which]["consensus_event_ms"] = round(prof["k_ransac_points"][0], 3)
            inl = np.zeros(nobs, dtype=np.uint8)
            lib.check(L.ba_memcpy_d2h(m.handle, lib.ptr(inl), d_in, nobs))
            wrong = np.bincount(pnt0, weights=((inl != 0) == outlier).astype(float), minlength=n)
            row["true_set_share"] = round(float((wrong == 0).mean()), 5)
            row["outliers_kept"] = int(((inl != 0) & outlier).sum())
            row["inliers_dropped"] = int(((inl == 0) & ~outlier).sum())
        x = np.empty(nvar)
        lib.check(L.ba_memcpy_d2h(m.handle, lib.ptr(x), d_x, 8 * nvar))
        err = np.linalg.norm((x - p["x_true"])[:3 * n].reshape(-1, 3), axis=1)
        row[which]["point_error_median"] = float(np.nanmedian(err))
        row[which]["point_error_p99"] = float(np.nanquantile(err, 0.99))
    lib.check(L.ba_dev_free(m.handle, d_x))
    lib.check(L.ba_dev_free(m.handle, d_in))
    row["ransac_over_plain"] = round(row["ransac"]["call_ms_median"] / row["plain"]["call_ms_median"], 2)
    row["consensus_ns_per_projection"] = round(1e6 * row["ransac"]["consensus_event_ms"] / max(row["projections_scored"], 1), 4)
    m.close()
    return row


def main():
    args = sys.argv[1:]
    ransac = "--ransac" in args
    if ransac:
        args.remove("--ransac")
    for key in ("hypotheses", "refits"):
        if "--" + key in args:
            at = args.index("--" + key)
            RANSAC[key] = int(args[at + 1])
            del args[at:at + 2]
    default = "ransac_points_bench.json" if ransac else "refine_points_bench.json"
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", default)
    reps = int(args.pop(0)) if args and args[0].isdigit() else 5
    shapes = args or ["dubrovnik-356", "venice-1778"]
    ba = ge.load_package()
    if ba.device_count() < 1:
        sys.exit("bench_refine_points: no HIP device visible (nothing is measured without one)")
    rows = []
    for name in shapes:
        row = (measure_ransac if ransac else measure)(ba, name, reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
