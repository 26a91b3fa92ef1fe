"""Rotation averaging over the view graph (ba_rotation_loops, ba_view_graph_forest, ba_average_rotations): time of the
stages, GPU only.

  dubrovnik-356 all pairs     356 cameras, 63 190 pairs
  venice-1778 all pairs       1778 cameras, 1 579 753 pairs
  venice-1778 window 20       1778 cameras, each paired with its 20 neighbours on either side (35 350 pairs): a graph with a
                              diameter of 89, where the simultaneous update needs many sweeps (max_sweeps = 20000 here)

The cameras' rotations are those of a generated scene with that many cameras; the relative rotations come from
synthetic.relative_rotations at 0.5 degrees of noise with 20 % of the pairs gross.  Per shape: the wall time of rotation_loops
(median of `reps` after a warm-up), of view_graph_forest on its support (host only) and of average_rotations under the loop
filter (3 degrees) and the huber loss (1 degree) -- that call runs the loop counts and the forest again --, the event time of
its kernels (profile class k_rotation_averaging), the sweeps, the gross pairs kept, and the error of the cameras against the
generator in degrees (gauge aligned at the root of the largest component).

One JSON object per shape on stdout; all of them to profiles/rotation_averaging_bench.json, or the file given.
usage: python tools/bench_rotation_averaging.py [out.json] [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _benchlib  # noqa: E402

DEG = np.pi / 180.0
NOISE, GROSS = 0.5 * DEG, 0.2
OPTIONS = dict(loops=dict(threshold=3 * DEG), loss="huber", f_scale=1 * DEG)


def timed(call, reps):
    """(the last result, the median of `reps` calls after a warm-up in ms, all of them)"""
    out = call()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t))
    return out, statistics.median(wall), wall


def measure(ba, name, ncams, pairs, reps, max_sweeps):
    p = ba.synthetic.make_problem(ncams, 4 * ncams, 12 * ncams, seed=1)  # (the handle and the cameras' rotations: nothing else is read)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    r, gross = ba.synthetic.relative_rotations(p["x_true"], p["npnts"], pairs, noise=NOISE, outlier_fraction=GROSS, seed=2)
    R_true = ba.synthetic.rotation_matrices(np.asarray(p["x_true"])[3 * p["npnts"]:].reshape(ncams, 9)[:, :3])
    (n_loops, support), loops_ms, loops_all = timed(lambda: ba.rotation_loops(m, pairs, r, threshold=OPTIONS["loops"]["threshold"]), reps)
    _, forest_ms, _ = timed(lambda: ba.view_graph_forest(ncams, pairs, support=support), reps)
    info, avg_ms, avg_all = timed(lambda: ba.average_rotations(m, pairs, r, max_sweeps=max_sweeps, **OPTIONS), reps)
    m.profile(True)
    ba.average_rotations(m, pairs, r, max_sweeps=max_sweeps, **OPTIONS)
    kernels_ms, _ = m.profile_get()["k_rotation_averaging"]
    m.profile(False)
    m.close()
    comp = info["component"]
    big = np.bincount(comp[comp >= 0]).argmax()
    mem = np.flatnonzero(comp == big)
    root = mem[info["status"][mem] == "root"][0]
    R = ba.synthetic.rotation_matrices(info["r"][mem])
    G = ba.synthetic.rotation_matrices(info["r"][[root]])[0].T @ R_true[root]
    err = np.degrees(np.sqrt((ba.synthetic.rotation_vectors((R @ G) @ np.transpose(R_true[mem], (0, 2, 1))) ** 2).sum(axis=1)))
    res = np.degrees(info["residual"])
    return {"shape": name, "ncams": int(ncams), "pairs": int(len(pairs)), "noise_degrees": 0.5, "gross_share": GROSS,
            "options": {"loops_threshold_degrees": 3.0, "loss": "huber", "f_scale_degrees": 1.0, "damping": 0.8, "xtol": 1e-6,
                        "max_sweeps": max_sweeps},
            "rotation_loops_ms_median": round(loops_ms, 3), "rotation_loops_ms_all": [round(v, 3) for v in loops_all],
            "triangles": int(n_loops.sum()) // 3, "view_graph_forest_host_ms_median": round(forest_ms, 3),
            "average_rotations_ms_median": round(avg_ms, 3), "average_rotations_ms_all": [round(v, 3) for v in avg_all],
            "kernels_event_ms": round(kernels_ms, 3), "sweeps": int(info["sweeps"]), "kept": int(info["kept"].sum()),
            "gross": int(gross.sum()), "gross_kept": int((info["kept"] & gross).sum()), "components": int(comp.max()) + 1,
            "counts": info["counts"], "cost_before": info["cost_before"], "cost_after": info["cost_after"],
            "camera_error_degrees_max": round(float(err.max()), 4), "camera_error_degrees_median": round(float(np.median(err)), 4),
            "clean_residual_degrees_max": round(float(np.nanmax(res[~gross])), 4),
            "gross_residual_degrees_min": round(float(np.nanmin(res[gross])), 4)}


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "rotation_averaging_bench.json")
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    ba, _ = _benchlib.load()
    if ba.device_count() < 1:
        sys.exit("bench_rotation_averaging: no HIP device visible (nothing is measured without one)")

    def every(n):
        a, b = np.triu_indices(n, 1)
        return np.stack([a + 1, b + 1], axis=1).astype(np.int64)

    def window(n, w):
        return np.array([(a, b) for a in range(1, n + 1) for b in range(a + 1, min(n, a + w) + 1)], dtype=np.int64)
    rows = []
    for name, n, pairs, max_sweeps in (("dubrovnik-356 all pairs", 356, every(356), 1000), ("venice-1778 all pairs", 1778, every(1778), 1000),
                                       ("venice-1778 window 20", 1778, window(1778, 20), 20000)):
        rows.append(measure(ba, name, n, pairs, reps, max_sweeps))
        print(json.dumps(rows[-1]), flush=True)
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
