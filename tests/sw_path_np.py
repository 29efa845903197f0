"""TEST INFRASTRUCTURE: numpy restatement of the located and traced constrained Smith-Waterman
alignment (acoss_sw_locate / acoss_sw_path and, per matrix, acoss_earlyfusion_locate /
acoss_earlyfusion_path). Not a test module.

Contract (include/acoss_hip.h states the same). B is a binary M x N matrix, S the score matrix of
oracle/crp_oracle.cpp or_sw_constrained, all arithmetic float64. Cells are named in B's own
coordinates: the reference's score_matrix[i][j] is the cell X = (i - 1, j - 1) here.
  scored cells: 2 <= r <= M - 2 and 2 <= c <= N - 2; every other cell holds 0.
  m(X) = +1 if B[X] else -1; pen(P) = 0 if B[P] else -0.7.
  predecessors of X = (r, c) in this fixed order: a (r-1, c-1), b (r-2, c-1), c (r-1, c-2), each
    with the value x_k = (S[P_k] + m(X)) + pen(P_k), in exactly that association.
  S[X] = max(x_a, x_b, x_c, 0).
  chosen predecessor: the FIRST of a, b, c attaining the maximum (strictly greater replaces, equal
    does not). A cell with S[X] == 0 has none; a cell whose chosen predecessor scores 0 begins a
    path, and that predecessor is not on the path.
  score = max S; end cell: the first cell in row-major order holding it.
  path: from the end cell follow chosen predecessors while S[P] > 0; reported origin to end. Steps
    (1, 1), (2, 1), (1, 2); every cell in [2, M-2] x [2, N-2] with S > 0; misses may lie on it; at
    most path_bound(M, N) = max(0, min(M, N) - 3) cells.
  segment: (r0, c0, r1, c1) = (origin, end), (-1, -1, -1, -1) and an empty path where the score is 0
    (always for M < 4 or N < 4).

sw_path is one vectorised step per row that fills a plane of codes (0 = none or the path begins
here, 1 / 2 / 3 = a / b / c) and walks it back; sw_path_cells is the definition cell by cell with
the predecessor order exposed; resum re-accumulates a path's score.
"""
from collections import namedtuple

import numpy as np

NONE = (-1, -1, -1, -1)
EMPTY = np.zeros((0, 2), np.int32)
PRED = {1: (1, 1), 2: (2, 1), 3: (1, 2)}   # code -> (dr, dc) back to P
STEPS = set(PRED.values())
PEN = -0.7

# score: float; path: (n, 2) int32 of (r, c), origin first; seg: (r0, c0, r1, c1); S: the score
# matrix in B's coordinates; choice: per cell 1 / 2 / 3, the first predecessor attaining the
# maximum (also where code is 0); code: the plane the walk back follows
Result = namedtuple("Result", "score path seg S choice code")


def path_bound(M, N):
    """The most cells a path can have: they lie in [2, min(M, N) - 2] and climb in both coordinates."""
    return max(0, min(M, N) - 3)


def _walk(code, end):
    path, x = [end], end
    while code[x]:
        d = PRED[int(code[x])]
        x = (x[0] - d[0], x[1] - d[1])
        path.append(x)
    return np.array(path[::-1], np.int32)


def _result(best, end, S, choice, code):
    if end is None:
        return Result(0.0, EMPTY, NONE, S, choice, code)
    path = _walk(code, end)
    return Result(float(best), path, (int(path[0, 0]), int(path[0, 1]), end[0], end[1]), S, choice, code)


def sw_path(B):
    """Result of a binary matrix, one vectorised step per row."""
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    S = np.zeros((M, N), np.float64)
    choice = np.zeros((M, N), np.uint8)
    code = np.zeros((M, N), np.uint8)
    best, end = 0.0, None
    if M < 4 or N < 4:
        return _result(best, end, S, choice, code)
    pen = np.where(B, 0.0, PEN)
    for r in range(2, M - 1):
        m = np.where(B[r, 2:N - 1], 1.0, -1.0)
        Sp = np.stack([S[r - 1, 1:N - 2], S[r - 2, 1:N - 2], S[r - 1, 0:N - 3]])            # a, b, c
        x = (Sp + m[None, :]) + np.stack([pen[r - 1, 1:N - 2], pen[r - 2, 1:N - 2], pen[r - 1, 0:N - 3]])
        k = np.argmax(x, axis=0)                                                          # first maximum
        v = np.maximum(np.take_along_axis(x, k[None, :], 0)[0], 0.0)
        sp = np.take_along_axis(Sp, k[None, :], 0)[0]
        S[r, 2:N - 1] = v
        choice[r, 2:N - 1] = k + 1
        code[r, 2:N - 1] = np.where((v > 0) & (sp > 0), k + 1, 0)
        if v.max() > best:                                                                # first row, then first column
            best, end = v.max(), (r, int(np.argmax(v)) + 2)
    return _result(best, end, S, choice, code)


def sw_path_cells(B, order=(0, 1, 2)):
    """The definition cell by cell. order: the predecessor priority, a permutation of (0, 1, 2) =
    (a, b, c), exposed so a test can show that a matrix tells the orders apart."""
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    S = np.zeros((M, N), np.float64)
    choice = np.zeros((M, N), np.uint8)
    code = np.zeros((M, N), np.uint8)
    best, end = 0.0, None
    for r in range(2, M - 1):
        for c in range(2, N - 1):
            m = 1.0 if B[r, c] else -1.0
            pred = [(r - 1, c - 1), (r - 2, c - 1), (r - 1, c - 2)]
            x = [(S[p] + m) + (0.0 if B[p] else PEN) for p in pred]
            k = order[0]
            for t in order[1:]:
                if x[t] > x[k]:
                    k = t
            v = x[k] if x[k] > 0.0 else 0.0
            S[r, c] = v
            choice[r, c] = k + 1
            if v > 0 and S[pred[k]] > 0:
                code[r, c] = k + 1
            if v > best:
                best, end = v, (r, c)
    return _result(best, end, S, choice, code)


def resum(B, path, first):
    """The score re-accumulated along a path, origin to end, from 0 at the origin's chosen predecessor
    (`first`: its code 1 / 2 / 3, Result.choice at the origin; that cell is not on the path):
    s = (s + m(X)) + pen(P) per cell X, P the cell before it."""
    B = np.asarray(B).astype(bool)
    s = 0.0
    d = PRED[int(first)]
    P = (int(path[0][0]) - d[0], int(path[0][1]) - d[1])
    for r, c in path:
        X = (int(r), int(c))
        s = (s + (1.0 if B[X] else -1.0)) + (0.0 if B[P] else PEN)
        P = X
    return s


def tie_cells(B, res):
    """The cells of res.path where two predecessors are equal on x, both at the maximum, and differ
    in S[P]: there the tie rule alone decides where the walk goes."""
    B = np.asarray(B).astype(bool)
    out = []
    for r, c in res.path:
        r, c = int(r), int(c)
        m = 1.0 if B[r, c] else -1.0
        pred = [(r - 1, c - 1), (r - 2, c - 1), (r - 1, c - 2)]
        x = [(res.S[p] + m) + (0.0 if B[p] else PEN) for p in pred]
        top = [t for t in range(3) if x[t] == max(x)]
        if len(top) > 1 and len({res.S[pred[t]] for t in top}) > 1:
            out.append((r, c))
    return out


def miss_cells(B, res):
    """The cells of res.path that are not set in B: the gaps the -1 paid for."""
    B = np.asarray(B).astype(bool)
    return [(int(r), int(c)) for r, c in res.path if not B[int(r), int(c)]]


def crosses_row(res, row):
    """Whether res.path has a cell before row `row` and one at or after it."""
    return len(res.path) > 0 and int(res.path[0, 0]) < row <= int(res.path[-1, 0])


# --------------------------------------------------------------------------------------------
# The matrices the host and the GPU tests share.
# --------------------------------------------------------------------------------------------
def make_matrix(M, N, density, plant, seed):
    """A random binary M x N uint8 matrix; plant = None, or the row where a noisy diagonal starts (at
    column 2): nine cells in ten set, now and then a (2, 1) or (1, 2) step, to the matrix's edge."""
    rng = np.random.default_rng([M, N, int(density * 100), 0 if plant is None else plant + 1, seed])
    B = (rng.random((M, N)) < density).astype(np.uint8)
    if plant is not None:
        r, c = plant, 2
        while r < M - 1 and c < N - 1:
            B[r, c] = rng.random() < 0.9
            u = rng.random()
            r += 2 if u < 0.08 else 1
            c += 2 if 0.08 <= u < 0.16 else 1
    return B


# rows per lane and per band of the kernels (sw.hip): the tests assert that paths straddle both
LANE_ROWS, BAND_ROWS = 8, 512

# (M, N, the rows a diagonal is planted at). 1030 x 40: one diagonal across each band boundary.
# 530 x 24: the 16-row score kernel in one band with 34 of 64 lanes holding rows, the tracing DP in
# two, a diagonal across row 512. 2050 x 24: the score kernel in three bands (boundaries at rows 1024
# and 2048), the tracing DP in five, a diagonal across each of the score kernel's boundaries.
SHAPES = [(3, 9, (2,)), (9, 3, (2,)), (4, 4, (2,)), (5, 9, (2,)), (14, 47, (2,)), (47, 14, (3,)), (33, 40, (2,)),
          (64, 65, (5,)), (130, 70, (40,)), (260, 70, (150,)), (1030, 40, (500, 1005)), (530, 24, (505,)),
          (2050, 24, (1015, 2040))]
DENSITIES = (0.1, 0.3, 0.6)

# (M, N, density, plant): every shape at every density, bare and with each planted diagonal
CASES = [(M, N, d, p) for M, N, plants in SHAPES for d in DENSITIES for p in (None,) + plants]

_CACHE = {}


def expected(M, N, density, plant, seed=0):
    """(matrix, Result) of one case; computed once per process and shared."""
    key = (M, N, density, plant, seed)
    if key not in _CACHE:
        B = make_matrix(M, N, density, plant, seed)
        _CACHE[key] = (B, sw_path(B))
    return _CACHE[key]
