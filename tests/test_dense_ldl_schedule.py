"""The schedule of the dense LDL' around its bulk update (csrc/ba_dense_ldl.hip): the ticketed pair update (persistent
workgroups drawing tiles from one queue per XCD, BA_LDL_TICKETS) and the look-ahead below the fused zone (lead strip on the
main stream, the rest of the update beside the next pair's chain, BA_LDL_TAIL_LOOKAHEAD).  Neither changes which
arithmetic a tile receives or in which order: every switch must give the same BITS, and the map from tickets to tiles
(ticket_tile, csrc/ba_internal.h) must hand every tile out exactly once whatever the order of the draws."""
import os
import re
import subprocess

import numpy as np
import pytest

from _lm_run import env
from _util import bits_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "bundleadjustment.jl_amd", "csrc", "ba_internal.h")

# ---- the ticket map, as arithmetic (CPU) -------------------------------------------------------------------------------------
MAIN = r"""
#include <cstdio>
#include <vector>
// one workgroup: its XCD, the index of the source it draws from, whether it has left
struct WG { int xcd, src; bool done; };
// a draw of workgroup g, as the kernel makes it: from an empty source on to the next, -1 when every source is empty
static int draw(WG &g, std::vector<int> &cnt, int nblk, int ready) {
  for (; g.src <= TICKET_QUEUES; g.src++) {
    const int q = ticket_source(g.xcd, g.src);
    const int t = ticket_tile(nblk, ready, q, cnt[q]++);
    if (t >= 0) return t;
  }
  g.done = true;
  return -1;
}
static int check(const char *what, int nblk, int ready, std::vector<WG> wgs, bool round_robin) {
  std::vector<int> cnt(TICKET_SLOTS, 0), seen(nblk, 0);
  int got = 0;
  auto take = [&](WG &g) {
    const int t = draw(g, cnt, nblk, ready);
    if (t < 0) return;
    if (t >= nblk) { std::printf("%s nblk=%d ready=%d: tile %d out of range\n", what, nblk, ready, t); got = -1000000000; return; }
    seen[t]++;
    got++;
  };
  if (round_robin) {
    for (bool any = true; any;) {
      any = false;
      for (WG &g : wgs)
        if (!g.done) { take(g); any = true; }
    }
  } else {
    for (WG &g : wgs)  // each workgroup alone until everything it can reach is empty
      while (!g.done) take(g);
  }
  for (const WG &g : wgs)
    if (!g.done) { std::printf("%s: a workgroup never left\n", what); return 1; }
  for (int t = 0; t < nblk; t++)
    if (seen[t] != 1) { std::printf("%s nblk=%d ready=%d: tile %d handed out %d times\n", what, nblk, ready, t, seen[t]); return 1; }
  if (got != nblk) { std::printf("%s nblk=%d ready=%d: %d tiles\n", what, nblk, ready, got); return 1; }
  return 0;
}
int main() {
  // the static chunked map's ranges: queue q covers tiles [q per, (q + 1) per) less the ready tiles
  for (int nblk : {1, 3, 7, 8, 9, 320, 321, 7750})
    for (int ready : {0, 1, 3}) {
      const int per = (nblk + 7) / 8, nr = ready < nblk ? ready : nblk;
      for (int q = 0; q < TICKET_QUEUES; q++)
        for (int n = 0; n < per + 2; n++) {
          const int t = ticket_tile(nblk, ready, q, n);
          if (t >= 0 && (t < q * per || t >= (q + 1) * per || t >= nblk || t < nr)) { std::printf("queue %d leaves its range: %d\n", q, t); return 1; }
        }
      for (int n = 0; n < 5; n++)
        if (ticket_tile(nblk, ready, TICKET_READY, n) != (n < nr ? n : -1)) { std::printf("ready counter wrong\n"); return 1; }
      std::vector<WG> one = {{5, 0, false}}, rr, same;
      for (int g = 0; g < 512; g++) rr.push_back({g % 8, 0, false});
      for (int g = 0; g < 512; g++) same.push_back({3, 0, false});
      if (check("one queue drains all", nblk, ready, one, false)) return 1;
      if (check("round robin", nblk, ready, rr, true)) return 1;
      if (check("all on one XCD", nblk, ready, same, true)) return 1;
      if (check("all on one XCD, one after the other", nblk, ready, same, false)) return 1;
    }
  std::printf("ok\n");
  return 0;
}
"""


def test_ticket_map_hands_every_tile_out_once(tmp_path):
    """ticket_tile / ticket_source compiled with g++ from the header's own text (as tests/test_tile_enumeration.py does for
    tri_blocked): for nblk in {1, 3, 7, 8, 9, 320, 321, 7750} and 0 / 1 / 3 ready tiles, under three arrival patterns -- one
    workgroup draining every queue, 512 workgroups over the 8 XCDs in strict round robin, all 512 on one XCD -- every tile comes
    out exactly once, every workgroup leaves, and a queue never leaves the range the static map gives its XCD."""
    text = open(HDR).read()
    m = re.search(r"constexpr int TICKET_QUEUES = .*?\n__host__ __device__ inline int ticket_source\(.*?\n", text, re.S)
    assert m, "ticket_tile / ticket_source not found in ba_internal.h"
    src = tmp_path / "ticket.cpp"
    src.write_text("#define __host__\n#define __device__\n" + m.group(0) + MAIN)
    exe = tmp_path / "ticket"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- the factorisation under every switch (GPU) ------------------------------------------------------------------------------
SIZES = [(1700, "14 tile rows, n not a multiple of 128: padding, last single column, row-split updates, short rests"),
         (3330, "27 tile rows (odd): in order, every pair eligible for the look-ahead"),
         (4480, "35 tile rows: first size with a hoisted workgroup"),
         (6800, "54 tile rows: fused pairs above, look-ahead below, the transition between them")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,what", SIZES)
def test_dense_ldl_switches_same_bits(ba, gpu_ok, n, what):
    """A = R + R' + 4 sqrt(n) I: the solve's residual below 1e-12, and the same bits in x with the tickets off, with the
    look-ahead off, with the look-ahead forced onto rests of any length, and from the default run twice.
    Which sizes reach the ticketed kernel (updates of more than 320 tiles that are not split by the look-ahead): 1700 never;
    3330 only with the look-ahead off; 4480 its first pair and, with the look-ahead off, the others; 6800 its fused pairs
    under every switch.  At the other sizes the BA_LDL_TICKETS=0 comparison checks only that the switch changes nothing."""
    rng = np.random.default_rng(0)
    R = rng.standard_normal((n, n))
    A = R + R.T
    del R
    A[np.diag_indices(n)] += 4 * np.sqrt(n)
    b = rng.standard_normal(n)

    def solve():
        return ba._lib.dense_ldl_solve(A, b)[0]

    x = solve()
    res = np.linalg.norm(A @ x - b) / np.linalg.norm(b)
    print(f"n = {n} ({what}): residual {res:.3e}")
    assert res < 1e-12, f"n = {n}: residual {res:.3e}"
    others = {"default, second run": solve(),
              "BA_LDL_TICKETS=0": env("BA_LDL_TICKETS", "0", solve),
              "BA_LDL_TAIL_LOOKAHEAD=0": env("BA_LDL_TAIL_LOOKAHEAD", "0", solve),
              "BA_LDL_TAIL_LOOKAHEAD_MIN=1": env("BA_LDL_TAIL_LOOKAHEAD_MIN", "1", solve),
              "BA_LDL_TAIL_LOOKAHEAD_MIN=1, BA_LDL_TICKETS=0": env("BA_LDL_TICKETS", "0", lambda: env("BA_LDL_TAIL_LOOKAHEAD_MIN", "1", solve)),
              "both off": env("BA_LDL_TICKETS", "0", lambda: env("BA_LDL_TAIL_LOOKAHEAD", "0", solve))}
    for tag, y in others.items():
        rep = bits_report(x, y, f"n = {n}, default vs {tag}")
        assert not rep, rep


@pytest.mark.gpu
def test_lm_step_recorded_lookahead_same_bits(ba, gpu_ok):
    """One LM step on a dense synthetic problem of 250 cameras (n = 2250, 18 tile rows): the factorisation is recorded into
    a graph with the look-ahead's fork and joins in it.  Plain launches (BA_LM_GRAPH=0) and either new switch off give the
    same step to the bit.  (Its updates have at most 136 tiles: the row-split kernel, never the ticketed one -- BA_LDL_TICKETS=0
    is compared here only because it must change nothing.)"""
    p = ba.synthetic.make_problem(250, 3000, 30000, seed=5)
    arrays = ba.synthetic.as_arrays(p)

    def step():
        m = ba.BALNLPModel(arrays=arrays)
        d, half, _ = ba.lm_step(m, p["x0"], 30.0)
        pat = ba.schur_pattern(m)
        m.close()
        return d, half, pat

    d, half, pat = step()
    assert np.all(np.isfinite(d)) and not pat[2], "the dense schedule is the one under test"
    for name, value in (("BA_LM_GRAPH", "0"), ("BA_LDL_TICKETS", "0"), ("BA_LDL_TAIL_LOOKAHEAD", "0"), ("BA_LDL_TAIL_LOOKAHEAD_MIN", "1")):
        d2, half2, _ = env(name, value, step)
        rep = bits_report(d, d2, f"LM step, default vs {name}={value}")
        assert not rep, rep
        assert half == half2
