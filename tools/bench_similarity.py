"""Similarity alignment of reconstructions (ba_similarity): time of the entry, GPU only.  Three shapes:

  one problem of 1 778 rows        the camera centres of venice-1778 against GPS
  one problem of 1 000 000 rows    two models joined through a million shared points: one workgroup in the select and fit
                                   kernels, 32 in the hypothesis kernel
  512 problems of 2 000 rows       the sub-models of a partitioned reconstruction, merged in one call

src is uniform in the unit ball, dst = s Q src + T with s in 0.5..40, a random Q and |T| = 10 per problem, Gaussian noise at 1 %
of the radius (s, in the units of dst) on every coordinate of dst, and 30 % of the rows displaced by 0.5..3 radii.  The call:
128 hypotheses of 3 rows, tau = 3 sigma, 2 refits.  Per shape: the wall time of `similarity` (median of `reps` after a warm-up;
it holds the packing of the row records on the host and the copies), the event time of its kernels (profile class
k_similarity), the displaced rows in a final set, and the worst clean row against the generator (|s R src + t - truth| under
the returned fit, as a share of the radius).

One JSON object per shape on stdout; all of them to profiles/similarity_bench.json, or the file given.
usage: python tools/bench_similarity.py [out.json] [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _benchlib  # noqa: E402

NOISE, DISPLACED = 0.01, 0.3
RANSAC = dict(hypotheses=128, sample=3, refits=2, seed=0)


def timed(call, reps):
    """(the last result, the median of `reps` calls after a warm-up in ms, all of them)"""
    out = call()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t))
    return out, statistics.median(wall), wall


def rotation(v):
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * np.outer(k, k)


def rows(nprob, n, seed):
    """(src, dst, offsets, the exact images s Q src + T, the displaced rows, s): one s for the call (tau is one number)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.5, 40.0)
    v = rng.normal(size=(nprob * n, 3))
    src = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, size=(nprob * n, 1)) ** (1 / 3)
    truth = np.empty_like(src)
    for k in range(nprob):
        axis, T = rng.normal(size=3), rng.normal(size=3)
        Q = rotation(axis / np.linalg.norm(axis) * rng.uniform(0.1, 3.0))
        truth[k * n:(k + 1) * n] = s * src[k * n:(k + 1) * n] @ Q.T + 10.0 * T / np.linalg.norm(T)
    dst = truth + rng.normal(size=truth.shape) * (NOISE * s)
    moved = rng.uniform(size=nprob * n) < DISPLACED
    w = rng.normal(size=(int(moved.sum()), 3))
    dst[moved] += w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, size=(len(w), 1)) * s
    return src, dst, np.arange(nprob + 1, dtype=np.int64) * n, truth, moved, s


def measure(ba, m, name, nprob, n, reps):
    src, dst, offsets, truth, moved, s = rows(nprob, n, seed=nprob + n)
    ransac = dict(RANSAC, threshold=3.0 * NOISE * s)
    info, wall_ms, wall_all = timed(lambda: ba.similarity(m, src, dst, offsets=offsets, ransac=ransac), reps)
    m.profile(True)
    ba.similarity(m, src, dst, offsets=offsets, ransac=ransac)
    kernels_ms, _ = m.profile_get()["k_similarity"]
    m.profile(False)
    worst = 0.0
    for k in range(nprob):
        sl = slice(k * n, (k + 1) * n)
        th = np.linalg.norm(info["r"][k])
        Q = rotation(info["r"][k]) if th > 0 else np.eye(3)
        e = np.linalg.norm(info["s"][k] * src[sl] @ Q.T + info["t"][k] - truth[sl], axis=1)
        worst = max(worst, float(e.max()) / s)
    return {"shape": name, "problems": int(nprob), "rows_per_problem": int(n), "noise_share_of_radius": NOISE, "displaced_share": DISPLACED,
            "options": dict(ransac, threshold_in_sigma=3.0), "similarity_ms_median": round(wall_ms, 3),
            "similarity_ms_all": [round(v, 3) for v in wall_all], "kernels_event_ms": round(kernels_ms, 3), "counts": info["counts"],
            "displaced": int(moved.sum()), "displaced_in_a_set": int((info["inliers"] & moved).sum()),
            "clean_in_a_set": int((info["inliers"] & ~moved).sum()), "rms_share_of_radius_max": round(float(np.nanmax(info["rms"])) / s, 6),
            "row_error_share_of_radius_max": round(worst, 6)}


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "similarity_bench.json")
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    ba, _ = _benchlib.load()
    if ba.device_count() < 1:
        sys.exit("bench_similarity: no HIP device visible (nothing is measured without one)")
    p = ba.synthetic.make_problem(6, 60, 240, seed=7)  # (the handle: the device, the stream and the buffers; no model data is read)
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    result = []
    for name, nprob, n in (("one problem of 1 778 rows", 1, 1778), ("one problem of 1 000 000 rows", 1, 1000000),
                           ("512 problems of 2 000 rows", 512, 2000)):
        result.append(measure(ba, m, name, nprob, n, reps))
        print(json.dumps(result[-1]), flush=True)
        with open(out, "w") as fh:
            json.dump(result, fh, indent=1)
    m.close()


if __name__ == "__main__":
    main()
