"""Symmetric indefinite systems whose blocked LDL' is exact in floating point, and the plain numpy factorisation they are checked
with (tests/test_dense_ldl_exact.py; the device code is csrc/ba_dense_ldl.hip).

A = L D L' with L unit lower triangular with entries in {-1, 0, +1} and D a diagonal of signed powers of two.  Every number a
right-looking blocked LDL' without pivoting forms from such an A -- trailing sums, V = L D, the explicit inverse of a diagonal
tile and of its 16 x 16 blocks, both triangular sweeps -- is an integer or a dyadic rational of small magnitude, hence exact in
Float64 and, below 2^24, in Float32, whatever the order of summation.  With B = A X0 for an integer X0 the solve must return
X0 to the last bit; with D[j] = 0 pivot j is exactly zero.

The construction (parameters below; they hold for every size the tests use, none had to be changed per case):
  diagonal tiles of L   128 x 128, aligned with the kernel's tiles.  Every row draws a level in {0 .. LEVELS-1}; N[i, j] is
                        -1 or +1 with probability TILE_P where j < i and level[j] < level[i], else 0; L_kk = I + N.  Then
                        N^LEVELS = 0 and L_kk^-1 = I - N + N^2 - N^3 stays small (a random integer unit lower tile's inverse
                        grows exponentially), while the updated diagonal tile L_kk D_k L_kk' is dense.
  below the diagonal    -1 or +1 with density OFF_P, else 0.
  D                     drawn from {1, 2, 4} with a random sign: powers of two, whose reciprocal the kernel's Newton step gives
                        exactly (3 fl(1/3) sits on a rounding tie); both signs in every tile, so A is indefinite everywhere.
  X0                    nonzero integers in [-3, 3]; for Float32 at n >= F32_SPARSE_N entries in {-1, 0, +1} with one in eight nonzero,
                        which keeps the sweeps' sums small.

LEVELS = 4, TILE_P = 0.5, OFF_P = 0.25, seed = n.  What guard() measured with them (Float32 limit 2^24 = 1.68e7); the last
three columns are for the dense X0 / the sparse Float32 X0:

     n   |L||D||L|'   panel solve   tile inverse   max |L_kk^-1|   |L||D||L|'|X0|    forward sweep     backward sweep
   300     2.2e2        4.7e2          2.0e2            13          1.8e4             2.6e4             1.7e3
  1700     1.1e3        8.0e2          3.2e2            24          4.9e5             9.3e4             2.6e3
  3330     2.2e3        7.4e2          3.1e2            29          1.8e6 / 1.1e5     1.4e5 / 2.1e4     3.0e3 / 2.4e2
  4480     2.8e3        9.3e2          3.4e2            28          3.2e6 / 2.0e5     1.9e5 / 2.9e4     2.7e3 / 2.5e2
  6800     4.2e3        9.0e2          3.4e2            29          7.3e6 / 4.9e5     2.4e5 / 4.0e4     3.9e3 / 3.2e2
(forward / backward: the larger of the sweep's own sums and of its multiplication with a tile's explicit inverse)
"""
import functools

import numpy as np

NB = 128  # the kernel's tile size (constexpr int NB, csrc/ba_internal.h; test_dense_ldl_exact.py checks that they agree): the
          # layered diagonal tiles must coincide with the tiles the kernel inverts
LEVELS, TILE_P, OFF_P = 4, 0.5, 0.25
F32_SPARSE_N = 3330
LIMIT = {True: 2.0 ** 24, False: 2.0 ** 53}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _factors(n, seed):
    """L, D, A = L D L' and what of the guard does not depend on X0 -> (L, D, A, bounds)"""
    rng = np.random.default_rng(seed)
    u = rng.random((n, n))
    L = np.where(u < OFF_P / 2, -1.0, np.where(u < OFF_P, 1.0, 0.0))
    del u
    L = np.tril(L, -1)
    linv_max, tiles = 0.0, []
    for k0 in range(0, n, NB):
        k1 = min(k0 + NB, n)
        m = k1 - k0
        level = rng.integers(0, LEVELS, m)
        sign = np.where(rng.random((m, m)) < 0.5, -1.0, 1.0)
        N = sign * (rng.random((m, m)) < TILE_P) * (level[None, :] < level[:, None])
        N = np.tril(N, -1)
        L[k0:k1, k0:k1] = N
        Li, P = np.eye(m), np.eye(m)
        for _ in range(LEVELS - 1):
            P = -(P @ N)
            Li += P
        assert np.array_equal((np.eye(m) + N) @ Li, np.eye(m)), f"tile {k0 // NB}: I - N + N^2 - ... is not the inverse"
        linv_max = max(linv_max, float(np.abs(Li).max()))
        tiles.append(Li)
    L[np.diag_indices(n)] = 1.0
    D = rng.choice([1.0, 2.0, 4.0], n) * rng.choice([-1.0, 1.0], n)
    A = (L * D) @ L.T
    aL = np.abs(L)
    trailing = float(((aL * np.abs(D)) @ aL.T).max())
    del aL
    panel = inverse = 0.0
    for t, Li in enumerate(tiles):
        k0, k1 = t * NB, min((t + 1) * NB, n)
        Lkk, aLi = L[k0:k1, k0:k1], np.abs(Li)
        # the updated panel below tile k is exactly L_ik D_k L_kk'; the kernel multiplies it with L_kk^-T
        S = (L[k1:, k0:k1] * D[k0:k1]) @ Lkk.T
        if S.size:
            panel = max(panel, float((np.abs(S) @ aLi.T).max()))
        # the tile's inverse is put together from those of its 16 x 16 blocks: products of the form L^-1 L L^-1
        inverse = max(inverse, float((aLi @ np.abs(Lkk) @ aLi).max()))
    bounds = dict(trailing=trailing, panel=panel, inverse=inverse, linv_max=linv_max, linv=tuple(tiles))
    return _frozen(L, D, A) + (bounds,)


def _tilewise(L, linv, v, transpose):
    """max over the tiles k of |L_kk^-1| |L_kk| |v_k| (transposed: of |L_kk^-1|' |L_kk|' |v_k|): the partial sums of a sweep's
    multiplication with the tile's explicit inverse"""
    worst = 0.0
    for t, Li in enumerate(linv):
        k0, k1 = t * NB, min((t + 1) * NB, len(L))
        Lkk, aLi = np.abs(L[k0:k1, k0:k1]), np.abs(Li)
        w = aLi.T @ (Lkk.T @ v[k0:k1]) if transpose else aLi @ (Lkk @ v[k0:k1])
        worst = max(worst, float(w.max()))
    return worst


def guard(L, D, X0, bounds, f32):
    """Sufficient conditions, all in absolute values so that no order of summation can exceed them, for the blocked LDL' of
    L D L' and the solve with B = L D L' X0 to be exact below LIMIT[f32].  Asserts them -> the measured figures."""
    limit = LIMIT[f32]
    aL, aD, aX = np.abs(L), np.abs(D)[:, None], np.abs(X0)
    B = L @ (D[:, None] * (L.T @ X0))
    y = D[:, None] * (L.T @ X0)  # the forward sweep's result
    got = dict(trailing=bounds["trailing"], panel=bounds["panel"], inverse=bounds["inverse"], linv_max=bounds["linv_max"],
               rhs=float((aL @ (aD * (aL.T @ aX))).max()),
               forward=float(np.abs(B).max() + (aL @ np.abs(y)).max()),
               forward_tile=_tilewise(L, bounds["linv"], np.abs(y), False),
               backward=float(np.abs(L.T @ X0).max() + (aL.T @ aX).max()),
               backward_tile=_tilewise(L, bounds["linv"], aX, True))
    for name, value in got.items():
        assert value < limit, f"n = {len(L)}, {'Float32' if f32 else 'Float64'}: {name} bound {value:.3e} reaches {limit:.3e}"
    return got


@functools.lru_cache(maxsize=None)
def _system(n, seed, f32, nrhs):
    L, D, A, bounds = _factors(n, seed)
    rng = np.random.default_rng([seed, nrhs, int(f32)])
    if f32 and n >= F32_SPARSE_N:
        X0 = rng.choice([-1.0, 1.0], (n, nrhs)) * (rng.random((n, nrhs)) < 0.125)
    else:
        X0 = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (n, nrhs))  # no zero: at n = 1 a zero x0 would test nothing
    measured = guard(L, D, X0, bounds, f32)
    B = A @ X0
    return _frozen(X0, B) + (measured,)


def exact_system(n, seed, *, f32, nrhs=1, zero_at=None):
    """-> A, L, D, X0, B with A = L D L' and B = A X0 (X0, B: (n, nrhs)), guarded for Float32 (f32) or Float64.  zero_at = j:
    D[j] = 0, which makes pivot j of the factorisation exactly zero and leaves every bound where it was or lower.  The arrays
    without a zero are built once per process and read-only."""
    L, D, A, _ = _factors(n, seed)
    X0, B, _ = _system(n, seed, bool(f32), nrhs)
    if zero_at is None:
        return A, L, D, X0, B
    j = zero_at
    A, D = A.copy(), D.copy()
    A[j:, j:] -= D[j] * np.outer(L[j:, j], L[j:, j])  # (column j of L is zero above row j)
    D[j] = 0.0
    return A, L, D, X0, A @ X0


def measured_bounds(n, seed, *, f32, nrhs=1):
    """what guard() measured for exact_system(n, seed, f32=f32, nrhs=nrhs)"""
    return dict(_system(n, seed, bool(f32), nrhs)[2])


def blocked_ldl_ref(A, B, dtype):
    """Right-looking blocked LDL' without pivoting of the lower triangle of A in `dtype`, as the device orders it: the diagonal
    tile unblocked, its unit factor inverted explicitly, V = S_ik L_kk^-T, L_ik = V / d, trailing update S_ij -= L_ik V_jk';
    then the forward sweep, the division by D and the backward sweep, each through the tiles' explicit inverses.
    -> (D (n,), L (n, n) unit lower, X like B).  A zero pivot is kept as 0.0 in D; what follows it is not finite."""
    S = np.tril(np.asarray(A)).astype(dtype)
    n = len(S)
    X = np.array(B, dtype=dtype).reshape(n, -1)
    d, linv = np.zeros(n, dtype), []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k0 in range(0, n, NB):
            k1 = min(k0 + NB, n)
            T, m = S[k0:k1, k0:k1], k1 - k0
            for j in range(m):
                d[k0 + j] = T[j, j]
                x = T[j + 1:, j].copy()  # column j of L D
                T[j + 1:, j] = x / T[j, j]
                T[j + 1:, j + 1:] -= np.outer(T[j + 1:, j], x)
            T[:] = np.tril(T, -1) + np.eye(m, dtype=dtype)
            Li = np.eye(m, dtype=dtype)
            for i in range(1, m):  # row i of L_kk^-1 by forward substitution
                Li[i, :i] = -(T[i, :i] @ Li[:i, :i])
            linv.append(Li)
            V = S[k1:, k0:k1] @ Li.T
            S[k1:, k0:k1] = V / d[k0:k1]
            S[k1:, k1:] -= S[k1:, k0:k1] @ V.T
        for t, k0 in enumerate(range(0, n, NB)):
            k1 = min(k0 + NB, n)
            X[k0:k1] = linv[t] @ X[k0:k1]
            X[k1:] -= S[k1:, k0:k1] @ X[k0:k1]
        X /= d[:, None]
        for t, k0 in reversed(list(enumerate(range(0, n, NB)))):
            k1 = min(k0 + NB, n)
            X[k0:k1] = linv[t].T @ X[k0:k1]
            X[:k0] -= S[k0:k1, :k0].T @ X[k0:k1]
    return d, np.tril(S), X.reshape(np.shape(B))
