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

--refine (with or without --five-point): the same shapes, scenes and options, then refine_relative_pose on the result
(linear loss, tau = the ransac threshold, 2 rounds, the defaults).  Per shape one row for the unrefined and one for the refined
result: the call time (the consensus entry; the refinement alone), the median rotation error and the median error of the
translation direction against the generator, the share of the OK pairs within 1 degree in both, the median n_consistent /
n_inliers (for the unrefined pose from an evaluate-only call, max_iter = 0) and the state counts.  To
profiles/relative_pose_refine_bench.json, where the rows of the other generator are kept.

--homography: the same shapes, scenes and options through homography (samples of 4) next to relative_pose (samples of
8) and relative_pose_five_point (samples of 5) on one handle -- wall time of each call, the event time of the homography's
kernels (profile class k_homography) and the wall time of homography_pose on its result -- to profiles/homography_bench.json.
These scenes are general, not planar: the times are what the stage costs, the counts say how rarely it finds a consensus there.

One JSON object per shape on stdout; all of them to profiles/relative_pose_bench.json, or the file given.
usage: python tools/bench_relative_pose.py [--five-point] [--refine] [--homography] [out.json] [reps]"""
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


def prepare(ba, p):
    """(the scene with its outliers, its model, x with the intrinsics alone, the true cameras)"""
    pt2d, _ = ba.synthetic.add_outliers(p, fraction=OUTLIER_FRACTION, seed=1)
    q = dict(p, pt2d=np.ascontiguousarray(pt2d.ravel()))
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(q))
    n, nc = p["npnts"], p["ncams"]
    x = np.full(len(p["x_true"]), np.nan)
    Ct = np.asarray(p["x_true"])[3 * n:].reshape(nc, 9)
    x[3 * n:].reshape(nc, 9)[:, 6:] = Ct[:, 6:]
    return q, m, x, Ct


def timed(call, reps):
    """(the last result, the median of `reps` calls after a warm-up in ms, all of them)"""
    out = call()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t))
    return out, statistics.median(wall), wall


def pose_errors(Ct, pairs, r, t):
    """(rotation error, error of the translation direction) in degrees against the generator, per pair"""
    Ra, Rb = rotations(Ct[pairs[:, 0] - 1, :3]), rotations(Ct[pairs[:, 1] - 1, :3])
    Rt = np.einsum("kij,klj->kil", Rb, Ra)
    tt = Ct[pairs[:, 1] - 1, 3:6] - np.einsum("kij,kj->ki", Rt, Ct[pairs[:, 0] - 1, 3:6])
    tt /= np.linalg.norm(tt, axis=1)[:, None]
    rot = np.degrees(np.arccos(np.clip(0.5 * (np.einsum("kij,kij->k", rotations(r), Rt) - 1.0), -1.0, 1.0)))
    return rot, np.degrees(np.arccos(np.clip((t * tt).sum(1) / np.linalg.norm(t, axis=1), -1.0, 1.0)))


def measure_refine(ba, name, p, pairs, options, reps, five):
    q, m, x, Ct = prepare(ba, p)
    if five:
        options = dict(options, sample=5)
    entry = ba.relative_pose_five_point if five else ba.relative_pose
    info, med, wall = timed(lambda: entry(m, x, pairs, ransac=options), reps)
    tau = options["threshold"]
    scored = ba.refine_relative_pose(m, x, pairs, info, threshold=tau, max_iter=0, rounds=0)  # (n_consistent of the unrefined pose)
    fine, rmed, rwall = timed(lambda: ba.refine_relative_pose(m, x, pairs, info, threshold=tau), reps)
    m.close()
    ok = info["status"] == "ok"
    rows = []
    for what, res, ms, all_ms, con in (("unrefined", info, med, wall, scored["n_consistent"]), ("refined", fine, rmed, rwall, fine["n_consistent"])):
        rot, tra = pose_errors(Ct, pairs[ok], res["r"][ok], res["t"][ok])
        row = {"shape": name, "entry": entry.__name__, "result": what, "pairs": int(len(pairs)), "ok": int(ok.sum()), "options": options,
               "call_ms_median": round(ms, 3), "call_ms_all": [round(v, 3) for v in all_ms],
               "rotation_error_degrees_median": round(float(np.median(rot)), 4), "direction_error_degrees_median": round(float(np.median(tra)), 4),
               "share_within_1_degree": round(float(((rot < 1.0) & (tra < 1.0)).mean()), 4),
               "share_rotation_within_1_degree": round(float((rot < 1.0).mean()), 4),
               "consistent_share_median": round(float(np.median(con[ok] / np.maximum(res["n_inliers"][ok], 1))), 4), "counts": info["counts"]}
        if what == "refined":
            row.update(refine_options=dict(threshold=tau, rounds=2, loss="linear"), refine_counts=fine["refine_counts"],
                       iters_median=int(np.median(fine["iters"][ok])), iters_max=int(fine["iters"].max()),
                       cost_ratio_median=round(float(np.median(fine["cost_after"][ok] / fine["cost_before"][ok])), 5),
                       rotation_error_rose_share=round(float((rot > pose_errors(Ct, pairs[ok], info["r"][ok], info["t"][ok])[0]).mean()), 4))
        rows.append(row)
    return rows


def measure_homography(ba, name, p, pairs, options, reps, five=False):
    q, m, x, Ct = prepare(ba, p)
    mp, _, _ = ba.pair_matches(q, pairs)
    row = {"shape": name, "entry": "homography", "pairs": int(len(pairs)), "matches": int(mp[-1]), "outlier_fraction": OUTLIER_FRACTION,
           "hypotheses": options["hypotheses"], "refits": options["refits"], "threshold": options["threshold"]}
    for key, entry, sample in (("eight_point", ba.relative_pose, 8), ("five_point", ba.relative_pose_five_point, 5), ("homography", ba.homography, 4)):
        info, med, wall = timed(lambda: entry(m, x, pairs, ransac=dict(options, sample=sample)), reps)
        row[key] = {"sample": sample, "call_ms_median": round(med, 3), "call_ms_all": [round(v, 3) for v in wall], "counts": info["counts"],
                    "hypotheses_per_s": round(len(pairs) * options["hypotheses"] / (med * 1e-3))}
    m.profile(True)
    info = ba.homography(m, x, pairs, ransac=dict(options, sample=4))
    ms, calls = m.profile_get()["k_homography"]
    m.profile(False)
    row["homography"]["kernels_event_ms"] = round(ms, 3)
    _, med, wall = timed(lambda: ba.homography_pose(m, x, pairs, info, threshold=options["threshold"]), reps)
    row["homography_pose"] = {"call_ms_median": round(med, 3), "call_ms_all": [round(v, 3) for v in wall]}
    m.close()
    return row


def measure(ba, name, p, pairs, options, reps, five=False):
    q, m, x, Ct = prepare(ba, p)
    n, nc = p["npnts"], p["ncams"]
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
    five, refine, hom = "--five-point" in args, "--refine" in args, "--homography" in args
    args = [a for a in args if a not in ("--five-point", "--refine", "--homography")]
    default = "homography_bench.json" if hom else "relative_pose_refine_bench.json" if refine else "relative_pose_five_point_bench.json" if five else "relative_pose_bench.json"
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", default)
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    ba, _ = _benchlib.load()
    if ba.device_count() < 1:
        sys.exit("bench_relative_pose: no HIP device visible (nothing is measured without one)")
    rows = []
    if refine and os.path.exists(out):  # (the rows of the other generator stay)
        mine = "relative_pose_five_point" if five else "relative_pose"
        rows = [r for r in json.load(open(out)) if r.get("entry") != mine]

    def add(*a):
        new = [measure_homography(ba, *a)] if hom else measure_refine(ba, *a) if refine else [measure(ba, *a)]
        for row in new:
            print(json.dumps(row), flush=True)
        rows.extend(new)
    p = ba.synthetic.make_named("dubrovnik-356")
    nc = p["ncams"]
    every = np.array([(a, b) for a in range(1, nc + 1) for b in range(a + 1, nc + 1)], dtype=np.int64)
    shared = np.diff(ba.pair_matches(p, every)[0])
    add("dubrovnik-356 all pairs sharing >= 8", p, every[shared >= 8], dict(threshold=2.0, hypotheses=128, sample=8, refits=2, seed=0), reps, five)
    g = ba.synthetic.make_problem(16, 4000, 8000, seed=3)  # its geometry; every camera sees every point
    pnt0, cam0 = np.repeat(np.arange(4000), 16), np.tile(np.arange(16), 4000)
    proj = ba.synthetic.project(g["x_true"][:12000].reshape(4000, 3)[pnt0], g["x_true"][12000:].reshape(16, 9)[cam0])
    pt2d = proj + np.random.default_rng(3).normal(0.0, 0.5, proj.shape)
    p = dict(g, cam_idx1=cam0 + 1, pnt_idx1=pnt0 + 1, pt2d=np.ascontiguousarray(pt2d.ravel()), nobs=len(pnt0))
    few = np.stack([np.arange(1, 16, 2), np.arange(2, 17, 2)], axis=1).astype(np.int64)
    add("16 cameras x 4000 points, 8 pairs", p, few, dict(threshold=2.0, hypotheses=1024, sample=8, refits=2, seed=0), reps, five)
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
