"""The dense LDL' (csrc/ba_dense_ldl.hip) on systems whose answer is known to the last bit.  tests/helpers/exact_ldl.py builds
A = L D L' from a unit lower triangular L with entries in {-1, 0, +1} and a diagonal D of signed powers of two: every number the
blocked factorisation and the sweeps form is then a small integer or dyadic rational, exact in Float64 and (below 2^24, which
the helper asserts) in Float32 whatever the order of summation.  So every schedule and both precisions must return the integer
X0 of B = A X0 exactly, and with D[j] = 0 pivot j is exactly zero and the call must raise.  No tolerance is involved, and no
change of schedule can legitimately break these tests.  The first tests need no device: they show with the numpy reference alone
that the systems are exact in the precision they are used in."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _lm_run import env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "helpers")
sys.path.insert(0, HELPERS)
import exact_ldl  # noqa: E402
from exact_ldl import NB, blocked_ldl_ref, exact_system  # noqa: E402

HDR = os.path.join(ROOT, "bundleadjustment.jl_amd", "csrc", "ba_internal.h")

SMALL = (1, 2, 16, 17, 127, 128, 129, 256, 257, 300)
ZONES = [(1700, "14 tile rows, ragged: row-split updates, look-ahead"),
         (3330, "27 tile rows, odd: the ticketed update once the look-ahead is off"),
         (4480, "35 tile rows: the smallest with a hoisted diagonal tile"),
         (6800, "54 tile rows, last tile 16 real columns: fused pairs 2, 4, 6, hoisted single, look-ahead")]
SWITCHES = [("BA_LDL_TICKETS", "0"), ("BA_LDL_TAIL_LOOKAHEAD", "0"), ("BA_LDL_TAIL_LOOKAHEAD_MIN", "1"), ("BA_LDL_UPDATE_RS_MAX", "1000000")]
MULTI = [(129, 25), (1700, 3)]
# (n, j, the place pivot j sits in)
ZERO_300 = [(300, 0, "tile 0, first lane"), (300, 5, "tile 0, inside block 0"), (300, 15, "tile 0, last pivot of block 0"),
            (300, 16, "tile 0, first pivot of block 1"), (300, 50, "tile 0, a middle block"), (300, 127, "tile 0, last pivot of the tile"),
            (300, 128, "second tile of the first pair"), (300, 200, "third tile"), (300, 299, "last real column of a ragged tile")]
ZERO_LARGE = [(1700, 128 * 5 + 77, "look-ahead zone, second tile of a pair"), (1700, 128 * 6 + 16, "look-ahead zone, first tile of a pair"),
              (1700, 1699, "last real column"),
              (4480, 128 * 2 + 40, "the hoisted tile 2 (k_ldl_diag with wait_ready)"), (4480, 128 * 3 + 40, "its pair partner"),
              (4480, 128 * 20 + 3, "in order below the hoisted zone"), (4480, 4479, "last pivot of all"),
              (6800, 128 * 2 + 9, "first tile of a hoisted k_ldl_pairdiag"), (6800, 128 * 3 + 100, "second tile of a hoisted k_ldl_pairdiag"),
              (6800, 128 * 7 + 31, "last fused pair, its second tile"), (6800, 128 * 8 + 31, "first pair after the fused zone"),
              (6800, 128 * 30 + 64, "look-ahead zone"), (6800, 6799, "last real column")]
ZERO_F32_LARGE = [(1700, 128 * 6 + 16, "look-ahead zone"), (4480, 128 * 2 + 40, "the hoisted tile 2"),
                  (6800, 128 * 3 + 100, "second tile of a hoisted k_ldl_pairdiag")]


def _zid(case):
    return f"{case[0]}-{case[1]}"


def system(n, f32=False, nrhs=1, zero_at=None):
    """the helper's system of size n (seed = n)"""
    return exact_system(n, n, f32=f32, nrhs=nrhs, zero_at=zero_at)


def assert_same(x, x0, tag):
    """x == x0 by value (-0.0 equals 0.0, NaN equals nothing); the message counts and locates, it never dumps an array"""
    x, x0 = np.asarray(x), np.asarray(x0)
    assert x.shape == x0.shape, f"{tag}: shape {x.shape}, expected {x0.shape}"
    if np.array_equal(x, x0):
        return
    bad = np.argwhere(~(x == x0))
    first = tuple(int(v) for v in bad[0])
    row = first[0]
    col = f", right-hand side {first[1]}" if len(first) > 1 else ""
    raise AssertionError(f"{tag}: {len(bad)} of {x.size} entries differ from the exact answer; the first is entry {row} (tile row "
                         f"{row // NB}, column {row % NB} of the tile{col}): {float(x[first])!r}, expected {float(x0[first])!r}")


# ---- the systems and the reference (CPU) -----------------------------------------------------------------------------------------
def test_tile_size_is_the_kernels():
    """The generator's layered diagonal tiles must be the tiles the kernel inverts: its NB against constexpr int NB of
    csrc/ba_internal.h.  With another tile size the tile inverses are no longer bounded and the device tests would run on an
    input the guard does not describe: this fails first."""
    m = re.search(r"^constexpr int NB = (\d+);", open(HDR).read(), re.M)
    assert m, "constexpr int NB not found in ba_internal.h"
    assert int(m.group(1)) == NB == 128


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [129, 300, 1700])
def test_reference_is_exact(n, dtype):
    """blocked_ldl_ref (plain numpy: unblocked diagonal tile, explicit tile inverse, V = S L_kk^-T, L = V / d, trailing update,
    both sweeps) in Float32 and in Float64 returns D, L and X0 themselves: the systems are exact without any device."""
    A, L, D, X0, B = system(n, f32=dtype is np.float32)
    d, l, x = blocked_ldl_ref(A, B, dtype)
    assert d.dtype == dtype and x.dtype == dtype
    assert_same(d, D, f"n = {n}, {dtype.__name__}: D")
    assert np.array_equal(l, L), f"n = {n}, {dtype.__name__}: {np.count_nonzero(l != L)} entries of L differ"
    assert_same(x, X0, f"n = {n}, {dtype.__name__}: x")


def test_reference_is_exact_with_several_right_hand_sides():
    """the reference's sweeps on 25 columns at once (n = 129), Float64"""
    A, L, D, X0, B = system(129, nrhs=25)
    assert len({tuple(c) for c in X0.T}) == 25, "the columns of X0 must be distinct"
    assert_same(blocked_ldl_ref(A, B, np.float64)[2], X0, "n = 129, 25 right-hand sides")


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("n", SMALL + tuple(n for n, _ in ZONES))
def test_guard_passes(n, f32):
    """Every (n, precision) the device tests use satisfies the helper's sufficient conditions for exactness (they are asserted
    while the system is built); the figures are printed."""
    A, L, D, X0, B = system(n, f32=f32)
    assert np.array_equal(A, A.T) and np.array_equal(np.diag(L), np.ones(n)) and np.all(np.isin(np.abs(D), (1.0, 2.0, 4.0)))
    if n >= 2 * NB:
        assert (D[:NB] < 0).any() and (D[:NB] > 0).any() and (D[-NB:] < 0).any() and (D[-NB:] > 0).any(), "A must be indefinite in every tile"
    got = exact_ldl.measured_bounds(n, n, f32=f32)
    print(f"n = {n}, {'Float32' if f32 else 'Float64'}: " + ", ".join(f"{k} {v:.2e}" for k, v in got.items()))
    assert max(got.values()) < exact_ldl.LIMIT[f32]


@pytest.mark.parametrize("n,nrhs", MULTI)
def test_guard_passes_with_several_right_hand_sides(n, nrhs):
    """the same for the systems of the multi-right-hand-side tests, whose columns must be distinct"""
    A, L, D, X0, B = system(n, nrhs=nrhs)
    assert X0.shape == B.shape == (n, nrhs) and len({tuple(c) for c in X0.T}) == nrhs
    assert max(exact_ldl.measured_bounds(n, n, f32=False, nrhs=nrhs).values()) < exact_ldl.LIMIT[False]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ZERO_300, ids=_zid)
def test_zero_at_gives_an_exactly_zero_pivot(case, dtype):
    """zero_at = j: the reference's pivot j is exactly 0.0 in either precision, the pivots before it are those of D, and the
    cached system without the zero is untouched."""
    n, j, _ = case
    A, L, D, X0, B = system(n, f32=dtype is np.float32, zero_at=j)
    d = blocked_ldl_ref(A, B, dtype)[0]
    assert d[j] == 0.0 and D[j] == 0.0
    assert np.array_equal(d[:j], D[:j]) and not np.any(D[:j] == 0.0)
    A1, _, D1, _, _ = system(n, f32=dtype is np.float32)
    assert D1[j] != 0.0 and not np.array_equal(A, A1) and np.array_equal(A1, (L * D1) @ L.T)


# ---- the device (GPU) --------------------------------------------------------------------------------------------------------
def _solve(ba, n, f32):
    A, _, _, X0, B = system(n, f32=f32)
    return ba._lib.dense_ldl_solve(A, B[:, 0], f32=f32)[0], X0[:, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n", SMALL)
def test_exact_solve_small_and_ragged(ba, gpu_ok, n, f32):
    """One pivot, one 16 x 16 block, the block boundary (16 | 17), one full tile (127 | 128 | 129: a second tile that is padding
    but for one row), two and three tiles: k_ldl_diag (pivots_mfma in Float64, the rank-1 pivots in Float32, row_solves,
    block_update, the tile inverse), k_ldl_trsm / the pair kernels, the row-split k_ldl_update, and the sweeps k_fwd_step (riding
    with the factorisation) and k_bwd_step.  x must be the integer x0."""
    x, x0 = _solve(ba, n, f32)
    assert_same(x, x0, f"n = {n}, {'Float32' if f32 else 'Float64'}")


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,what", ZONES)
def test_exact_solve_through_every_zone(ba, gpu_ok, n, what, f32):
    """The sizes of test_dense_ldl_schedule.py, for the reasons given there: 1700 row-split updates and the look-ahead; 3330 the
    in-order schedule at 27 tile rows; 4480 the hoisted k_ldl_diag (wait_ready) and the ticketed update of its first pair;
    6800 the hoisted k_ldl_pairdiag with k_ldl_pairtrsm for pairs 2, 4, 6, then the hoisted single tile, then the look-ahead,
    with a last tile of 16 real columns.  In Float32 none of the zones above 8 tile rows has run outside one LM-level test.
    x must be the integer x0 in both precisions."""
    x, x0 = _solve(ba, n, f32)
    assert_same(x, x0, f"n = {n} ({what}), {'Float32' if f32 else 'Float64'}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{k}={v}" for k, v in SWITCHES])
@pytest.mark.parametrize("n", [3330, 6800])
def test_exact_solve_under_every_switch(ba, gpu_ok, n, name, value):
    """Float64 under each switch that is read per call: BA_LDL_TICKETS=0 (the ticketed k_ldl_update replaced by the static
    one), BA_LDL_TAIL_LOOKAHEAD=0 (no lead strip: 3330 then reaches the ticketed update), BA_LDL_TAIL_LOOKAHEAD_MIN=1 (the
    look-ahead on rests of any length), BA_LDL_UPDATE_RS_MAX=1000000 (every update row-split).  The bit-for-bit tests compare
    these with each other; here each must give x0 itself."""
    x, x0 = env(name, value, lambda: _solve(ba, n, False))
    assert_same(x, x0, f"n = {n}, {name}={value}")


CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import __graft_entry__ as ge; ba = ge.load_package(); "
         "from exact_ldl import exact_system; n = int(sys.argv[1]); A, L, D, X0, B = exact_system(n, n, f32=False); "
         "x = ba._lib.dense_ldl_solve(A, B[:, 0])[0]; bad = np.flatnonzero(~(x == X0[:, 0])); "
         "print('WRONG', bad.size, *((int(bad[0]), x[bad[0]], X0[bad[0], 0]) if bad.size else ()))") % (ROOT, HELPERS)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["BA_LDL_FUSE", "BA_LDL_HOIST"])
def test_exact_solve_fallback_schedules(ba, gpu_ok, switch):
    """BA_LDL_FUSE=0 (the hoisted single k_ldl_diag where pairs would be fused) and BA_LDL_HOIST=0 (strictly in order) are read
    once per process: one fresh child per setting builds the n = 6800 system from the helper, solves in Float64 and prints how
    many entries differ from x0 -- none may.  (Elsewhere these fallbacks run at n = 16002 only, checked by a residual.)"""
    r = subprocess.run([sys.executable, "-c", CHILD, "6800"], capture_output=True, text=True, env=dict(os.environ, **{switch: "0"}), timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("WRONG")][0].split()
    assert int(line[1]) == 0, (f"{switch}=0, n = 6800: {line[1]} entries differ from the exact answer; the first is entry {line[2]} (tile row "
                               f"{int(line[2]) // NB}, column {int(line[2]) % NB} of the tile): {line[3]}, expected {line[4]}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,nrhs", MULTI)
def test_exact_solve_multi(ba, gpu_ok, n, nrhs):
    """dense_ldl_solve_multi (Float64; the factorisation without a riding right-hand side, then k_fwd_step / k_bwd_step over all
    columns): 25 columns on two tiles of which the second has one real row, 3 columns on 14 tile rows, distinct integer columns.
    X is X0 exactly, and column 0 is what dense_ldl_solve returns for it."""
    A, _, _, X0, B = system(n, nrhs=nrhs)
    X = ba._lib.dense_ldl_solve_multi(A, B)[0]
    assert_same(X, X0, f"n = {n}, {nrhs} right-hand sides")
    assert_same(ba._lib.dense_ldl_solve(A, B[:, 0])[0], X[:, 0], f"n = {n}: dense_ldl_solve on column 0 against dense_ldl_solve_multi")


def _zero_pivot_case(ba, case, f32, multi=False):
    """pivot j exactly zero: the call raises SQDException "zero pivot"; the next call on the same size without a zero solves
    exactly -- the flag, the ready counters and the hoisting are left as a first call finds them"""
    n, j, place = case
    A, _, _, _, B = system(n, f32=f32, nrhs=2 if multi else 1, zero_at=j)
    tag = f"n = {n}, zero pivot {j} (tile {j // NB}, column {j % NB}: {place}), {'Float32' if f32 else 'Float64'}"
    with pytest.raises(ba.SQDException, match="zero pivot"):
        if multi:
            ba._lib.dense_ldl_solve_multi(A, B)
        else:
            ba._lib.dense_ldl_solve(A, B[:, 0], f32=f32)
        pytest.fail(f"{tag}: no exception", pytrace=False)
    del A, B
    A, _, _, X0, B = system(n, f32=f32, nrhs=2 if multi else 1)
    X = ba._lib.dense_ldl_solve_multi(A, B)[0] if multi else ba._lib.dense_ldl_solve(A, B[:, 0], f32=f32)[0][:, None]
    assert_same(X, X0, f"{tag}: the solve without a zero that follows")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ZERO_300 + ZERO_LARGE, ids=_zid)
def test_zero_pivot_everywhere_f64(ba, gpu_ok, case):
    """Float64: the flag is raised in pivots_mfma of diag_tile.  n = 300: every position within tile 0 (first lane, inside a
    block, both sides of a block edge, a middle block, the tile's last pivot), the second tile of the pair (k_ldl_diag /
    k_ldl_pairdiag in order), the third tile, the last real column of a ragged tile.  1700: both tiles of a pair in the look-ahead
    zone.  4480: the hoisted k_ldl_diag (wait_ready) of tile 2, its partner, the in-order zone.  6800: both tiles of a hoisted
    k_ldl_pairdiag, the last fused pair, the first pair below the fused zone, the look-ahead zone.  In the hoisted zones the flag
    shares its int with the value 2 ("hoisted wait abandoned").  The kernels carry on over NaNs, the flag is read at the end."""
    _zero_pivot_case(ba, case, False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ZERO_300 + ZERO_F32_LARGE, ids=_zid)
def test_zero_pivot_everywhere_f32(ba, gpu_ok, case):
    """Float32: the flag is raised in the rank-1 pivots form of diag_tile, which nothing had asked to report before.  Every
    n = 300 position, and one case each in the look-ahead zone (1700), the hoisted k_ldl_diag (4480) and the second tile of a
    hoisted k_ldl_pairdiag (6800)."""
    _zero_pivot_case(ba, case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ZERO_300, ids=_zid)
def test_zero_pivot_everywhere_multi(ba, gpu_ok, case):
    """dense_ldl_solve_multi (two right-hand sides, no riding forward sweep) at every n = 300 position: the same exception,
    no sweep afterwards, and the next call solves exactly."""
    _zero_pivot_case(ba, case, False, multi=True)
