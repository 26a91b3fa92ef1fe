"""Cost of the covariance estimate (ba_covariance) by phase, from the per-kernel event timing (ba_profile_get):
  assembly   k_schur_prep + k_schur_blocks (the reduced camera system with the damping vector of the mask)
  factor     the k_ldl_* classes (the Float64 LDL' as the LM step runs it)
  inversion  k_cov_selinv (diag(S) and the rank check, then the selected inversion Z = S^-1 on the factor's pattern)
  cameras    k_cov_cams, points  k_cov_points
with the flop count of the inversion's tile products and the gather bytes of k_cov_points computed from the shape and the
pattern, and the wall time of a whole call (profiling off; median of `reps`, after a warm-up call).  The gauge is fixed as
the tests fix it (camera 1's pose, the first translation component of camera 2), lambda = 0 unless the shape says otherwise.
One JSON object per shape on stdout; all of them to `out.json` when given.
usage: python tools/bench_covariance.py [out.json] [reps] [shape ...]
  shape: a name of synthetic.SHAPES, optionally with :locality=<w> or :plane=<r>, and :lam=<lambda> (default: venice-1778)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

NB = 128
F64_MFMA_PEAK_TFLOPS = 78.6  # MI355X (gfx950) dense Float64 matrix peak
PHASES = {"assembly": ("k_schur_prep", "k_schur_blocks"),
          "factor": ("k_ldl_diag", "k_ldl_trsm", "k_ldl_col", "k_ldl_update", "k_ldl_update_rs"),
          "inversion": ("k_cov_selinv",), "cameras": ("k_cov_cams",), "points": ("k_cov_points",)}


def parse(spec):
    """name[:locality=w][:plane=r][:lam=l] -> (name, make_named keywords, lambda)"""
    name, *opts = spec.split(":")
    kw, lam = {}, 0.0
    for opt in opts:
        key, _, val = opt.partition("=")
        if key == "locality":
            kw["locality"] = float(val)
        elif key == "plane":
            kw["plane_radius"] = float(val)
        elif key == "lam":
            lam = float(val)
    return name, kw, lam


def row_lists(ba, p, perm1, sparse):
    """tile rows of every tile column of S (below the diagonal) as the inversion takes them: all rows for the dense
    schedule, the symbolic factorisation's pair lists ({k+1} + U_q, U_q) for the list schedule"""
    ncams = p["ncams"]
    nt = max(1, -(-9 * ncams // NB))
    if not sparse:
        return [nt - 1 - k for k in range(nt)]
    pos = np.empty(ncams, dtype=np.int64)
    pos[perm1 - 1] = np.arange(ncams)
    import scipy.sparse as sps
    c0, p0 = pos[p["cam_idx1"] - 1], p["pnt_idx1"] - 1
    rows = np.r_[p0, p0]
    cols = np.r_[9 * c0 // NB, (9 * c0 + 8) // NB]  # a camera's 9 rows may straddle two tiles
    B = sps.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(p["npnts"], nt))
    B.data[:] = 1.0
    occ = (B.T @ B).toarray() > 0
    occ = np.tril(occ)
    m = []
    for q in range((nt + 1) // 2):
        k = 2 * q
        U = [i for i in range(k + 2, nt) if occ[i, k] or (k + 1 < nt and occ[i, k + 1])]
        for a in U:
            occ[a, U] = True
        occ = np.tril(occ)
        m.append(len(U) + (1 if k + 1 < nt else 0))
        if k + 1 < nt:
            m.append(len(U))
    return m


def measure(ba, spec, reps):
    name, kw, lam = parse(spec)
    t0 = time.time()
    p = ba.synthetic.make_named(name, **kw)
    gen_s = time.time() - t0
    m = ba.BALNLPModel(arrays=ba.synthetic.as_arrays(p))
    comp = np.zeros((p["ncams"], 9), dtype=bool)
    comp[0, :6] = True
    comp[1, 3] = True
    fix = dict(fixed_camera_params=comp)
    x = p["x0"]
    row = {"shape": spec, "ncams": p["ncams"], "npnts": p["npnts"], "nobs": p["nobs"], "n": 9 * p["ncams"], "lambda": lam, "gen_s": round(gen_s, 1)}
    _, _, piv = ba.covariance(m, x, lam, **fix)  # warm-up: ordering, pattern, workspace
    row["min_rel_pivot"] = piv
    tf, ff, sparse = ba.schur_pattern(m)
    perm1, order = ba.schur_ordering_used(m)
    row.update(tile_fill=round(tf, 4), flop_fill=round(ff, 4), sparse_schedule=sparse, ordering=order)
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        ba.covariance(m, x, lam, **fix)
        wall.append(1e3 * (time.perf_counter() - t))
    row["call_ms_median"] = round(statistics.median(wall), 2)
    row["call_ms_all"] = [round(v, 2) for v in wall]
    m.profile(True)
    ba.covariance(m, x, lam, **fix)
    prof = m.profile_get()
    m.profile(False)
    m.close()
    ms = {ph: sum(prof.get(k, (0.0, 0))[0] for k in ks) for ph, ks in PHASES.items()}
    row.update({f"{ph}_ms": round(v, 3) for ph, v in ms.items()})
    row["inversion_over_factor"] = round(ms["inversion"] / ms["factor"], 3) if ms["factor"] > 0 else None
    # tile products of the inversion: B_k^-1 (nt), per column k with m rows: panel (m), bulk (m^2), diagonal (m)
    mt = np.array(row_lists(ba, p, perm1, sparse), dtype=np.float64)
    tile_flop = 2.0 * NB ** 3
    inv_flop = tile_flop * (len(mt) + (mt * mt).sum() + 2 * mt.sum())
    row["inversion_gflop"] = round(inv_flop / 1e9, 1)
    row["inversion_bulk_gflop"] = round(tile_flop * (mt * mt).sum() / 1e9, 1)
    if ms["inversion"] > 0:
        row["inversion_TFLOPs"] = round(inv_flop / (ms["inversion"] * 1e-3) / 1e12, 2)
        row["inversion_of_f64_mfma_peak"] = round(row["inversion_TFLOPs"] / F64_MFMA_PEAK_TFLOPS, 3)
    # k_cov_points: one 9 x 9 block of Z (648 B) per observation pair o >= o' of a point
    d = np.bincount(p["pnt_idx1"] - 1, minlength=p["npnts"]).astype(np.float64)
    gb = 648.0 * (d * (d + 1) / 2).sum() / 1e9
    row["points_gather_GB"] = round(gb, 2)
    if ms["points"] > 0:
        row["points_GBps"] = round(gb / (ms["points"] * 1e-3), 1)
    return row


def main():
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else None
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    shapes = args or ["venice-1778"]
    ba = ge.load_package()
    rows = []
    for spec in shapes:
        row = measure(ba, spec, reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if out:
        old = []
        if os.path.exists(out):
            with open(out) as fh:
                old = [r for r in json.load(fh) if r.get("shape") not in {r2["shape"] for r2 in rows}]
        with open(out, "w") as fh:
            json.dump(old + rows, fh, indent=1)


if __name__ == "__main__":
    main()
