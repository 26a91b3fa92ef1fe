"""Translation averaging over the view graph (ba_translation_loops, ba_average_translations): time of the stages, GPU
only.  The shapes of bench_rotation_averaging.py:

  dubrovnik-356 all pairs     356 cameras, 63 190 pairs
  venice-1778 all pairs       1778 cameras, 1 579 753 pairs
  venice-1778 window 20       1778 cameras, each paired with its 20 neighbours on either side (35 350 pairs): a graph with a
                              diameter of 89 (max_cg = 2000 here)

The cameras' poses are those of a generated scene with that many cameras; the baselines come from
synthetic.relative_translations at 0.01 rad of noise with 10 % of the pairs gross, turned into world directions by
translation_directions with the true rotations.  Per shape: the wall time of translation_loops (median of `reps` after a
warm-up) and of average_translations under the loop filter (5 degrees, ratio 0.34) and the huber loss (0.05) -- that call runs
the loop counts and the forest again --, the event time of its kernels (profile class k_translation_averaging), the
Levenberg-Marquardt and conjugate-gradient iterations, the gross pairs kept, and the worst distance of a camera from the
generator's after a similarity alignment, as a share of the scene radius.

One JSON object per shape on stdout; all of them to profiles/translation_averaging_bench.json, or the file given.
usage: python tools/bench_translation_averaging.py [out.json] [reps]"""
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
NOISE, GROSS = 0.01, 0.1
OPTIONS = dict(loops=dict(threshold=5 * DEG, min_ratio=0.34), loss="huber", f_scale=0.05)


def timed(call, reps):
    """(the last result, the median of `reps` calls after a warm-up in ms, all of them)"""
    out = call()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t))
    return out, statistics.median(wall), wall


def aligned_error(c, c_true):
    """the distance of every camera to c_true after the best similarity (Umeyama) over the finite rows"""
    ok = np.isfinite(c).all(axis=1)
    x, y = c[ok], c_true[ok]
    mx, my = x.mean(axis=0), y.mean(axis=0)
    U, S, Vt = np.linalg.svd((y - my).T @ (x - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    s = (S * np.diag(D)).sum() / ((x - mx) ** 2).sum()
    return np.linalg.norm(s * (x - mx) @ (U @ D @ Vt).T + my - y, axis=1)


def measure(ba, name, ncams, pairs, reps, max_cg):
    p = ba.synthetic.make_problem(ncams, 4 * ncams, 12 * ncams, seed=1)  # (the handle and the cameras' poses: nothing else is read)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    cams = np.asarray(p["x_true"])[3 * p["npnts"]:].reshape(ncams, 9)
    R = ba.synthetic.rotation_matrices(cams[:, :3])
    centres = -np.einsum("kji,kj->ki", R, cams[:, 3:6])
    t, gross = ba.synthetic.relative_translations(p["x_true"], p["npnts"], pairs, noise=NOISE, outlier_fraction=GROSS, seed=2)
    dirs = ba.translation_directions(pairs, t, cams[:, :3])
    (n_loops, support), loops_ms, loops_all = timed(lambda: ba.translation_loops(m, pairs, dirs, threshold=OPTIONS["loops"]["threshold"]), reps)
    info, avg_ms, avg_all = timed(lambda: ba.average_translations(m, pairs, dirs, max_cg=max_cg, **OPTIONS), reps)
    m.profile(True)
    ba.average_translations(m, pairs, dirs, max_cg=max_cg, **OPTIONS)
    kernels_ms, _ = m.profile_get()["k_translation_averaging"]
    m.profile(False)
    m.close()
    radius = float(np.linalg.norm(centres - centres.mean(axis=0), axis=1).max())
    err = aligned_error(info["c"], centres) / radius
    res = np.degrees(info["residual"])
    return {"shape": name, "ncams": int(ncams), "pairs": int(len(pairs)), "noise_rad": NOISE, "gross_share": GROSS,
            "options": {"loops_threshold_degrees": 5.0, "min_ratio": 0.34, "loss": "huber", "f_scale": 0.05, "max_iterations": 50,
                        "ftol": 1e-10, "cg_tol": 1e-6, "max_cg": max_cg},
            "translation_loops_ms_median": round(loops_ms, 3), "translation_loops_ms_all": [round(v, 3) for v in loops_all],
            "checked_triangles": int(n_loops.sum()) // 3,
            "average_translations_ms_median": round(avg_ms, 3), "average_translations_ms_all": [round(v, 3) for v in avg_all],
            "kernels_event_ms": round(kernels_ms, 3), "lm_iterations": int(info["iterations"]), "cg_iterations": int(info["cg_iterations"]),
            "accepted": int(info["trace"][:, 3].sum()), "kept": int(info["kept"].sum()), "gross": int(gross.sum()),
            "gross_kept": int((info["kept"] & gross).sum()), "clean_dropped": int((~info["kept"] & ~gross).sum()),
            "components": int(info["component"].max()) + 1, "counts": info["counts"], "cost_before": info["cost_before"],
            "cost_after": info["cost_after"], "camera_error_share_of_radius_max": round(float(err.max()), 5),
            "camera_error_share_of_radius_median": round(float(np.median(err)), 5),
            "kept_clean_residual_degrees_max": round(float(np.nanmax(res[info["kept"] & ~gross])), 4)}


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "translation_averaging_bench.json")
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    ba, _ = _benchlib.load()
    if ba.device_count() < 1:
        sys.exit("bench_translation_averaging: no HIP device visible (nothing is measured without one)")

    def every(n):
        a, b = np.triu_indices(n, 1)
        return np.stack([a + 1, b + 1], axis=1).astype(np.int64)

    def window(n, w):
        return np.array([(a, b) for a in range(1, n + 1) for b in range(a + 1, min(n, a + w) + 1)], dtype=np.int64)
    rows = []
    for name, n, pairs, max_cg in (("dubrovnik-356 all pairs", 356, every(356), 500), ("venice-1778 all pairs", 1778, every(1778), 500),
                                   ("venice-1778 window 20", 1778, window(1778, 20), 2000)):
        rows.append(measure(ba, name, n, pairs, reps, max_cg))
        print(json.dumps(rows[-1]), flush=True)
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
