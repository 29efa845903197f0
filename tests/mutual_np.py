"""The mutual nearest-neighbour binarisation of EarlyFusion restated in numpy from the definition in
include/acoss_hip.h ("mutual") -- TEST INFRASTRUCTURE ONLY, shared by test_mutual_host.py and the
GPU tests (test_gpu_mutual*.py).

For a float32 M x N matrix D and kappa:
  count(kappa, n) = int(np.round(kappa * n)) for kappa < 1 (float64 product, half to even), else
      int(kappa), clamped to n as the C ABI clamps it; nn_r = count(kappa, N), nn_c = count(kappa, M);
      kappa == 0 gives all ones.
  R(i, j) = 1 iff fewer than nn_r cells of row i come before (i, j) in (value ascending, column ascending)
  C(i, j) = 1 iff fewer than nn_c cells of column j come before (i, j) in (value ascending, row ascending)
  B = R & C.
mutual_largest: the same on a float64 matrix with "value descending" in both rules (early SNF).
Nothing here calls oracle.ef_binarize: the ranks come from np.lexsort alone.
"""
import numpy as np


def count(kappa, n):
    nn = int(np.round(np.float64(kappa) * n)) if kappa < 1 else int(kappa)
    return min(nn, int(n))


def _line_ranks(V):
    """rank[i, j] = how many cells of row i come before (i, j) in (value ascending, index ascending)."""
    M, N = V.shape
    rank = np.empty((M, N), np.int64)
    idx = np.arange(N)
    for i in range(M):
        order = np.lexsort((idx, V[i]))  # last key first: by value, then by index
        rank[i, order] = idx
    return rank


def _both(V, kappa):
    """(R, C) uint8 of a matrix whose SMALLEST values are the neighbours."""
    M, N = V.shape
    if kappa == 0:
        one = np.ones((M, N), np.uint8)
        return one, one.copy()
    R = (_line_ranks(V) < count(kappa, N)).astype(np.uint8)
    C = (_line_ranks(np.ascontiguousarray(V.T)) < count(kappa, M)).T.astype(np.uint8)
    return R, np.ascontiguousarray(C)


def rows_smallest(D, kappa):
    return _both(np.asarray(D, np.float32), kappa)[0]


def cols_smallest(D, kappa):
    return _both(np.asarray(D, np.float32), kappa)[1]


def mutual_smallest(D, kappa):
    R, C = _both(np.asarray(D, np.float32), kappa)
    return R & C


def rows_largest(X, kappa):
    return _both(-np.asarray(X, np.float64), kappa)[0]


def mutual_largest(X, kappa):
    """The early-SNF form: float64, the LARGEST values (negation is exact and turns the order round;
    -0 and +0 compare equal in lexsort, as the definition has them)."""
    R, C = _both(-np.asarray(X, np.float64), kappa)
    return R & C


# ---- the matrices the host and the GPU tests share -------------------------------------------------
SHAPES_HOST = [(1, 1), (1, 7), (7, 1), (4, 30), (30, 4), (15, 17), (25, 25)]
KAPPAS = (0.1, 0.3, 0, 5, 1000)


def tie_matrices(M, N, seed):
    """[random float32, integers 0..3, constant, constant columns] of one shape."""
    rng = np.random.default_rng([M, N, seed])
    return [rng.standard_normal((M, N)).astype(np.float32),
            rng.integers(0, 4, size=(M, N)).astype(np.float32),
            np.full((M, N), 2.5, np.float32),
            np.repeat(rng.standard_normal((1, N)).astype(np.float32), M, 0)]
