"""Block-sparse LDL' on scenes whose camera graph is NOT one connected band or disc: several problems merged into one, and
cameras that share no point with any other camera (tests/helpers/scenes.py).  At a component boundary that falls on a tile
column pair's boundary the pair has no row below its own two tile rows: its row list is {k+1} alone (or empty for the single
last column), U_q is empty -- a "short" pair.  The two-run phase of dense_ldl_factor_sparse (csrc/ba_dense_ldl.hip) launches
the panel solves of pair i of run A and pair split + i of run B together and has no form for a short pair; the symbolic phase
(tile_pattern_build, csrc/ba_order.cpp) therefore ends a run before its first short pair.

CPU: csrc/ba_order.cpp (host only) compiled with g++ and a small driver, as tests/test_tile_enumeration.py and
tests/test_dense_ldl_schedule.py do for the header's arithmetic; the driver goes through what order_cameras / ensure_dense do and
re-derives the independence of the two runs from the pattern's row lists by brute force.  GPU: the factorisation on these
scenes against the oracle, the one-chain schedule and the dense schedule."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from _lm_run import env
from _util import bits_report, rel_err
from _util import parity_record as _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import scenes  # noqa: E402

CSRC = os.path.join(ROOT, "bundleadjustment.jl_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>
#include "ba_order.h"
typedef std::set<std::pair<int, int>> Tiles;
// every tile pair q reads or writes: its two diagonal tiles, (k+1, k), the panels (i, k), (i, k+1) over U_q, the lower tiles of U_q x U_q
static void pair_tiles(const TilePattern &pat, int q, Tiles *out) {
  const int k = 2 * q, l0 = pat.prow_ptr[(size_t)q], l1 = pat.prow_ptr[(size_t)q + 1];
  out->insert({k, k});
  if (k + 1 < (int)pat.nt) {
    out->insert({k + 1, k + 1});
    out->insert({k + 1, k});
  }
  for (int a = l0 + 1; a < l1; a++) {
    const int i = pat.prow[(size_t)a];
    out->insert({i, k});
    out->insert({i, k + 1});
    for (int b = l0 + 1; b <= a; b++) out->insert({i, pat.prow[(size_t)b]});
  }
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *fh = fopen(argv[1], "r");
  const int method = !strcmp(argv[2], "AMD") ? BA_ORDER_AMD : BA_ORDER_METIS, nb = 128;
  long long ncams, npnts, nobs;
  if (!fh || fscanf(fh, "%lld %lld %lld", &ncams, &npnts, &nobs) != 3) return 2;
  std::vector<int> cam0((size_t)nobs), pnt0((size_t)nobs), ptr((size_t)npnts + 1, 0), obs((size_t)nobs);
  for (long long k = 0; k < nobs; k++) {
    long long c, p;
    if (fscanf(fh, "%lld %lld", &c, &p) != 2 || c < 0 || c >= ncams || p < 0 || p >= npnts) return 2;
    cam0[(size_t)k] = (int)c;
    pnt0[(size_t)k] = (int)p;
    ptr[(size_t)p + 1]++;
  }
  fclose(fh);
  for (long long i = 0; i < npnts; i++) ptr[(size_t)i + 1] += ptr[(size_t)i];
  std::vector<int> cur(ptr.begin(), ptr.end() - 1);
  for (long long k = 0; k < nobs; k++) obs[(size_t)cur[(size_t)pnt0[(size_t)k]]++] = (int)k;
  CamGraph g;
  cam_graph_build(ncams, npnts, ptr.data(), obs.data(), cam0.data(), &g);
  std::vector<int> perm, pos((size_t)ncams);
  const char *chosen = "?";
  int split = 0;
  cam_order(g, method, nb, &perm, &chosen, &split);
  if ((long long)perm.size() != ncams) return 3;
  for (long long k = 0; k < ncams; k++) pos[(size_t)perm[(size_t)k]] = (int)k;
  const int64_t nt = (9 * ncams + nb - 1) / nb;
  std::vector<unsigned char> occ;
  cam_tile_occupancy(g, pos, nt, nb, &occ);
  TilePattern pat;
  tile_pattern_build(nt, occ, &pat, split);
  const int npairs = (int)pat.prow_ptr.size() - 1;
  printf("chosen %s\n", chosen);
  printf("shape %lld %d %d %d %d\n", (long long)nt, npairs, pat.split, pat.a_clean, pat.b_clean);
  printf("rows");
  for (int q = 0; q < npairs; q++) printf(" %d", pat.prow_ptr[(size_t)q + 1] - pat.prow_ptr[(size_t)q]);
  printf("\nperm");
  for (long long k = 0; k < ncams; k++) printf(" %d", perm[(size_t)k]);
  // the two runs, from the row lists alone: no tile in common, and no pair before the split with a row among run B's columns
  int shared = 0, crossing = 0;
  if (pat.a_clean > 0 || pat.b_clean > 0) {
    if (pat.split <= 0 || pat.a_clean > pat.split || pat.split + pat.b_clean > npairs) return 4;
    Tiles A, B;
    for (int q = 0; q < pat.a_clean; q++) pair_tiles(pat, q, &A);
    for (int q = pat.split; q < pat.split + pat.b_clean; q++) pair_tiles(pat, q, &B);
    for (const auto &t : A) shared += (int)B.count(t);
    for (int q = 0; q < pat.split; q++)
      for (int l = pat.prow_ptr[(size_t)q]; l < pat.prow_ptr[(size_t)q + 1]; l++)
        crossing += pat.prow[(size_t)l] >= 2 * pat.split && pat.prow[(size_t)l] < 2 * (pat.split + pat.b_clean);
  }
  printf("\nindependent %d %d\n", shared, crossing);
  return 0;
}
"""

NUMBERINGS = [False, True]  # as generated, shuffle_cameras(seed=8)
METHODS = ["AMD", "Metis"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("order_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src), os.path.join(CSRC, "ba_order.cpp")], check=True)
    cache = {}

    def run(ba, name, shuffled, method):
        """-> dict(chosen, nt, npairs, split, a_clean, b_clean, rows, perm, shared, crossing); one run per combination"""
        key = (name, shuffled, method)
        if key not in cache:
            p = scenes.scene(ba, name, shuffled)
            f = d / f"scene{list(scenes.SCENES).index(name)}_{int(shuffled)}.txt"
            if not f.exists():
                with open(f, "w") as fh:
                    fh.write(f"{p['ncams']} {p['npnts']} {p['nobs']}\n")
                    np.savetxt(fh, np.column_stack([p["cam_idx1"] - 1, p["pnt_idx1"] - 1]), fmt="%d")
            out = subprocess.run([str(exe), str(f), method], capture_output=True, text=True)
            assert out.returncode == 0, f"driver failed ({out.returncode}): {out.stdout[-300:]} {out.stderr[-300:]}"
            lines = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] if " " in ln else "" for ln in out.stdout.splitlines()}
            nt, npairs, split, ac, bc = (int(v) for v in lines["shape"].split())
            shared, crossing = (int(v) for v in lines["independent"].split())
            cache[key] = dict(chosen=lines["chosen"], nt=nt, npairs=npairs, split=split, a_clean=ac, b_clean=bc,
                              rows=[int(v) for v in lines["rows"].split()], perm=np.array(lines["perm"].split(), dtype=np.int64),
                              shared=shared, crossing=crossing)
            assert len(cache[key]["rows"]) == npairs and sorted(cache[key]["perm"].tolist()) == list(range(p["ncams"]))
        return cache[key]

    return run


def _describe(name, shuffled, method, r):
    short = [q for q, c in enumerate(r["rows"]) if c < 2]
    return (f"{name}, {'shuffled' if shuffled else 'as generated'}, {method}: {r['chosen']}, nt {r['nt']}, split / a_clean / b_clean "
            f"{r['split']} / {r['a_clean']} / {r['b_clean']}, short pairs {short}")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shuffled", NUMBERINGS, ids=["as-generated", "shuffled"])
@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_no_short_pair_inside_a_joint_step(ba, driver, name, shuffled, method):
    """(a) Every joint step i < min(a_clean, b_clean) of the two-run phase handles pair i and pair split + i in the same
    launches; both need at least 2 rows ({k+1} and a non-empty U_q), because the second panel solve gives a run 4 c2 workgroups
    and y_{k+1} comes from the run's own first workgroup.
    (b) The two runs are independent, re-derived by the driver from the row lists: the tile sets of the pairs [0, a_clean) and
    [split, split + b_clean) are disjoint and no pair before the split has a row in [2 split, 2 (split + b_clean))."""
    r = driver(ba, name, shuffled, method)
    print(_describe(name, shuffled, method, r))
    both = min(r["a_clean"], r["b_clean"])
    bad = [(i, r["rows"][i], r["rows"][r["split"] + i]) for i in range(both) if r["rows"][i] < 2 or r["rows"][r["split"] + i] < 2]
    assert not bad, f"joint steps with a short pair (step, rows of pair i, rows of pair split + i): {bad} -- " + _describe(name, shuffled, method, r)
    assert r["shared"] == 0 and r["crossing"] == 0, f"the runs share {r['shared']} tiles, {r['crossing']} rows of run A's side cross into run B's columns"
    if both:
        assert r["chosen"] == "two-ended" and 0 < r["a_clean"] <= r["split"] and r["split"] + r["b_clean"] <= r["npairs"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", [n for n, (_, big) in scenes.SCENES.items() if big and n != "one band of 1100"])
def test_disconnected_scenes_keep_their_two_runs(ba, driver, name, method):
    """(c) The scenes are not vacuous: as generated the two-ended sequence still wins and at least 4 joint steps remain; a short
    pair exists, and where it belongs to a run it sits at or after the end of that run (the run was cut there, not switched off)."""
    r = driver(ba, name, False, method)
    print(_describe(name, False, method, r))
    assert r["chosen"] == "two-ended" and min(r["a_clean"], r["b_clean"]) >= 4, _describe(name, False, method, r)
    short = [q for q, c in enumerate(r["rows"][:-1]) if c < 2]  # (the last pair never has a row below it)
    assert short, "no short pair before the last one: the scene does not reach the case"
    for q in short:
        assert q >= r["a_clean"] if q < r["split"] else q - r["split"] >= r["b_clean"], (q, _describe(name, False, method, r))


def test_one_chain_scene_has_a_short_pair_mid_chain(ba, driver):
    """Two bands of 256 cameras (18 tile rows each): the numbering as generated wins, one chain, and pair 8 (the last of the
    first band: no camera of tile rows 16, 17 shares a point with one below) is short in the middle of the chain."""
    for method in METHODS:
        r = driver(ba, "two bands of 256", False, method)
        print(_describe("two bands of 256", False, method, r))
        assert r["chosen"] == "natural" and r["split"] == 0 and r["a_clean"] == 0 and r["b_clean"] == 0
        assert r["nt"] == 36 and r["rows"][8] == 1 and r["rows"][7] >= 2 and r["rows"][9] >= 2


# (d) the symbolic result for the suite's two-run problem at the parent of the change that introduced the cut: split / a_clean /
# b_clean and the sha1 of the sequence (int64, 0-based), from the same driver built against that commit's ba_order.cpp
BAND_1100 = {
    (False, "AMD"): ((18, 14, 17), "d89e9d578e27faff0ffedf58430e85ac3d50992c"),
    (False, "Metis"): ((18, 14, 17), "d89e9d578e27faff0ffedf58430e85ac3d50992c"),
    (True, "AMD"): ((18, 14, 17), "0937c004b3a263f247fa3968e79389cdbe90a8e4"),
    (True, "Metis"): ((18, 14, 17), "0937c004b3a263f247fa3968e79389cdbe90a8e4"),
}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shuffled", NUMBERINGS, ids=["as-generated", "shuffled"])
def test_band_without_a_short_pair_is_untouched(ba, driver, shuffled, method):
    """(d) A pattern without a short pair keeps its runs and its sequence: the band of 1100 cameras of
    test_block_sparse_two_chains gives what it gave before the runs were cut at short pairs."""
    r = driver(ba, "one band of 1100", shuffled, method)
    print(_describe("one band of 1100", shuffled, method, r), hashlib.sha1(r["perm"].tobytes()).hexdigest())
    shape, sha = BAND_1100[(shuffled, method)]
    assert r["chosen"] == "two-ended" and (r["split"], r["a_clean"], r["b_clean"]) == tuple(shape)
    assert hashlib.sha1(r["perm"].tobytes()).hexdigest() == sha
    assert all(c >= 2 for c in r["rows"][:-1])


# ---- the factorisation on these scenes (GPU) ---------------------------------------------------------------------------------
GPU_CASES = [("two bands of 512", False), ("four bands of 256", False), ("band of 1200 + 256 isolated cameras", False),
             ("band of 1200 + 256 isolated cameras", True), ("256 isolated cameras + band of 800", False), ("two bands of 256", False)]
LM_RUN_CASE = "two bands of 512"  # the complete runs (recorded graphs against plain launches) on one two-run case only


@pytest.mark.gpu
@pytest.mark.parametrize("name,shuffled", GPU_CASES, ids=[f"{n}{' shuffled' if s else ''}" for n, s in GPU_CASES])
def test_block_sparse_disconnected_scenes(ba, orc, gpu_ok, name, shuffled):
    """One LM step (lambda = 10) through the list schedule on a scene with several components.  The short pairs -- the last pair
    of a component that ends on a pair boundary -- follow the two runs in order (two-run scenes) or sit in the middle of the one
    chain (two bands of 256, where the backward sweep also meets an empty column list mid-chain): their y_{k+1} comes from the
    stand-alone forward step, never from a panel solve without a workgroup.
    Two steps on a fresh handle give the same bits (a y_{k+1} nobody wrote would be uninitialised memory in the first step and
    the first step's value in the second); the step equals the oracle's (its ldl_analyse handed the handle's own camera sequence)
    to 1e-9 and its model value to 1e-10, the one-chain schedule's (BA_SPARSE_TWO_RUNS=0) to 1e-11, the dense schedule's
    (BA_SPARSE_S=0: other kernels, other storage) to 1e-10 -- the limits of test_block_sparse_two_chains and
    test_block_sparse_factor_time_follows_the_pattern at these sizes; the look-ahead forced on and the backward sweep one pair
    per launch give the same bits; the Float32 factorisation the same bits twice and the oracle's step to 5e-3."""
    p = scenes.scene(ba, name, shuffled)
    arrays = ba.synthetic.as_arrays(p)
    big = scenes.SCENES[name][1]
    lam = 10.0
    m = ba.BALNLPModel(arrays=arrays)
    try:
        step = lambda ft=None: ba.lm_step(m, p["x0"], lam, facto_type=ft)[:2]  # noqa: E731
        (a1, ha1), (a2, ha2) = step(), step()  # first: a fresh handle
        pat, (perm, chosen) = ba.schur_pattern(m), ba.schur_ordering_used(m)
        b1, _ = env("BA_SPARSE_TWO_RUNS", "0", step)
        l1, _ = env("BA_SPARSE_LOOKAHEAD_MIN", "1", step)
        w1, _ = env("BA_SPARSE_BWD2", "0", step)
        (f1, _), (f2, _) = step(np.float32), step(np.float32)
    finally:
        m.close()
    assert pat[2], f"the list schedule is the one under test: {pat}"
    if big:
        assert chosen == "two-ended", chosen

    def dense():
        md = ba.BALNLPModel(arrays=arrays)
        try:
            d, _, _ = ba.lm_step(md, p["x0"], lam)
            assert not ba.schur_pattern(md)[2]
            return d
        finally:
            md.close()

    d_dense = env("BA_SPARSE_S", "0", dense)
    assert np.all(np.isfinite(a1)) and np.all(np.isfinite(f1))
    for tag, (x, y) in {"Float64 step twice on a fresh handle": (a1, a2), "look-ahead forced vs default threshold": (a1, l1),
                        "backward sweep, two groups per launch vs one pair per launch": (a1, w1), "Float32-factor step twice": (f1, f2)}.items():
        rep = bits_report(x, y, f"{name}: {tag}")
        assert not rep, rep
    assert ha1 == ha2, f"model value differs between two steps on one handle: {ha1!r} {ha2!r}"
    rc, d_ref, dr_ref, _ = orc.lm_step(p["ncams"], p["npnts"], p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], lam, cam_perm1=perm)
    assert rc == 0
    half_ref = 0.5 * float(dr_ref @ dr_ref)
    e_orc, e_one, e_dense, e32, e_half = rel_err(a1, d_ref), rel_err(a1, b1), rel_err(a1, d_dense), rel_err(f1, d_ref), abs(ha1 - half_ref) / ha1
    tag = f"{name}{', shuffled' if shuffled else ''}"
    print(f"{tag} ({chosen}, pattern {pat}): vs oracle {e_orc:.2e}, model value {e_half:.2e}, vs one chain {e_one:.2e}, vs dense schedule "
          f"{e_dense:.2e}, Float32 vs oracle {e32:.2e}")
    _report(f"block_sparse_disconnected_scenes[{tag}]", step_vs_oracle=e_orc, model_value_vs_oracle=e_half, vs_one_chain=e_one,
            vs_dense_schedule=e_dense, f32_vs_oracle=e32, ordering=chosen)
    assert e_orc <= 1e-9, f"step vs oracle: {e_orc:.3e}"
    assert abs(ha1 - half_ref) <= 1e-10 * ha1, f"model value vs oracle: {e_half:.3e}"
    assert e_one <= 1e-11, f"two runs vs one chain: {e_one:.3e}"
    assert e_dense <= 1e-10, f"list schedule vs dense schedule: {e_dense:.3e}"
    assert e32 <= 5e-3, f"Float32 factorisation vs oracle: {e32:.3e}"
    if name != LM_RUN_CASE:
        return

    def run(graph):
        mr = ba.BALNLPModel(arrays=arrays)
        try:
            return env("BA_LM_GRAPH", graph, lambda: ba.Levenberg_Marquardt(ba.FeasibilityResidual(mr), "LDL", "AMD", "None", False, ite_max=4))
        finally:
            mr.close()

    s_graph, s_plain = run(None), run("0")
    assert s_graph.iter == s_plain.iter and s_graph.log == s_plain.log
    rep = bits_report(s_graph.solution, s_plain.solution, f"{name}: solution of a 4-iteration run, recorded graphs vs plain launches")
    assert not rep, rep
