"""Relative pose of camera pairs (ba_relative_pose; with --five-point ba_relative_pose_five_point): time
of the host entry, GPU only.

  all-pairs    every camera pair of the Dubrovnik-shaped scene that shares 8 points or more (the generator draws a point's cameras
               uniformly: tens of matches per pair, tens of thousands of pairs), H = 128, m = 8, tau = 2 px, 2 refits
  few-pairs    8 pairs of a 16-camera scene in which every camera sees every point (thousands of matches per pair), H = 1024

Both with 30 % of every camera's detections displaced (synthetic.add_outliers) and the generator's 0.5 px noise.  Host clock
around ba_relative_pose (the match lists on the host, the uploads, the five kernels, the copies back), median of `reps` after a
warm-up; beside it the host time of ba_pair_matches alone, hypotheses per second (pairs x H / call), the states, and the share of
the pairs with a pose whose rotation lies within 1 degree of the generator's.

--five-point: the same shapes, scenes and options through relative_pose_five_point (samples of 5), to
profiles/relative_pose_five_point_bench.json.

One JSON object per shape on stdout; all of them to profiles/relative_pose_bench.json, or the file given.
usage: python tools/bench_relative_pose.py [--five-point] [out.json] [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _benchlib  # noqa: E402

OUTLIER_FRACTION = 0.3


def rotations(r):
    th = np.sqrt((r * r).sum(1))
    k = r / th[:, None]
    K = np.zeros((len(r), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    return c * np.eye(3) + s * K + (1 - c) * k[:, :, None] * k[:, None, :]


def measure(ba, name, p, pairs, options, reps, five=False):
    pt2d, _ = ba.synthetic.add_outliers(p, fraction=OUTLIER_FRACTION, seed=1)
    q = dict(p, pt2d=np.ascontiguousarray(pt2d.ravel()))
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(q))
    n, nc = p["npnts"], p["ncams"]
    x = np.full(len(p["x_true"]), np.nan)
    Ct = np.asarray(p["x_true"])[3 * n:].reshape(nc, 9)
    x[3 * n:].reshape(nc, 9)[:, 6:] = Ct[:, 6:]
    t = time.perf_counter()
    mp, _, _ = ba.pair_matches(q, pairs)
    match_ms = 1e3 * (time.perf_counter() - t)
    if five:
        options = dict(options, sample=5)
    entry = ba.relative_pose_five_point if five else ba.relative_pose
    info = entry(m, x, pairs, ransac=options)  # warm-up
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        info = entry(m, x, pairs, ransac=options)
        wall.append(1e3 * (time.perf_counter() - t))
    m.close()
    med = statistics.median(wall)
    ok = info["status"] == "ok"
    Ra, Rb = rotations(Ct[pairs[ok, 0] - 1, :3]), rotations(Ct[pairs[ok, 1] - 1, :3])
    Rt = np.einsum("kij,klj->kil", Rb, Ra)
    Re = rotations(info["r"][ok])
    angle = np.degrees(np.arccos(np.clip(0.5 * (np.einsum("kij,kij->k", Re, Rt) - 1.0), -1.0, 1.0)))
    H = options["hypotheses"]
    per = np.diff(mp)
    return {"shape": name, "entry": "relative_pose_five_point" if five else "relative_pose", "ncams": nc, "npnts": n, "nobs": p["nobs"], "pairs": int(len(pairs)), "matches": int(mp[-1]),
            "matches_per_pair_min": int(per.min()), "matches_per_pair_median": int(np.median(per)), "matches_per_pair_max": int(per.max()),
            "outlier_fraction": OUTLIER_FRACTION, "options": options, "call_ms_median": round(med, 3), "call_ms_all": [round(v, 3) for v in wall],
            "pair_matches_host_ms": round(match_ms, 3), "hypotheses_per_s": round(len(pairs) * H / (med * 1e-3)),
            "pairs_per_s": round(len(pairs) / (med * 1e-3)), "counts": info["counts"],
            "inlier_share_median": round(float(np.median(info["n_inliers"][ok] / per[ok])), 4) if ok.any() else None,
            "share_within_1_degree": round(float((angle < 1.0).mean()), 4) if ok.any() else None,
            "rotation_error_degrees_median": round(float(np.median(angle)), 4) if ok.any() else None}


def main():
    args = sys.argv[1:]
    five = "--five-point" in args
    args = [a for a in args if a != "--five-point"]
    default = "relative_pose_five_point_bench.json" if five else "relative_pose_bench.json"
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", default)
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    ba, _ = _benchlib.load()
    if ba.device_count() < 1:
        sys.exit("bench_relative_pose: no HIP device visible (nothing is measured without one)")
    rows = []
    p = ba.synthetic.make_named("dubrovnik-356")
    nc = p["ncams"]
    every = np.array([(a, b) for a in range(1, nc + 1) for b in range(a + 1, nc + 1)], dtype=np.int64)
    shared = np.diff(ba.pair_matches(p, every)[0])
    rows.append(measure(ba, "dubrovnik-356 all pairs sharing >= 8", p, every[shared >= 8], dict(threshold=2.0, hypotheses=128, sample=8, refits=2, seed=0), reps, five))
    print(json.dumps(rows[-1]), flush=True)
    g = ba.synthetic.make_problem(16, 4000, 8000, seed=3)  # its geometry; every camera sees every point
    pnt0, cam0 = np.repeat(np.arange(4000), 16), np.tile(np.arange(16), 4000)
    proj = ba.synthetic.project(g["x_true"][:12000].reshape(4000, 3)[pnt0], g["x_true"][12000:].reshape(16, 9)[cam0])
    pt2d = proj + np.random.default_rng(3).normal(0.0, 0.5, proj.shape)
    p = dict(g, cam_idx1=cam0 + 1, pnt_idx1=pnt0 + 1, pt2d=np.ascontiguousarray(pt2d.ravel()), nobs=len(pnt0))
    few = np.stack([np.arange(1, 16, 2), np.arange(2, 17, 2)], axis=1).astype(np.int64)
    rows.append(measure(ba, "16 cameras x 4000 points, 8 pairs", p, few, dict(threshold=2.0, hypotheses=1024, sample=8, refits=2, seed=0), reps, five))
    print(json.dumps(rows[-1]), flush=True)
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
