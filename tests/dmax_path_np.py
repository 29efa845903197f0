"""TEST INFRASTRUCTURE: numpy restatement of the located and traced dmax (chen17) alignment
(acoss_crp_locate_dmax / acoss_locate_crp_dmax / acoss_crp_path_dmax / acoss_path_crp_dmax). Not a
test module. The matrices are those of tests/qmax_trace_np.py (SHAPES, SEEDS, GAMMAS, make_matrix).

Contract (include/acoss_hip.h states the same). C is a binary M x N matrix, D the chen17 score
matrix of oracle/crp_oracle.cpp or_align(which = 1), all arithmetic float32, cells with i < 2 or
j < 2 hold 0, g(c) = gamma_open if c is set else gamma_ext. For X = (i, j), i, j >= 2, the
predecessors in this fixed order, each with the cell it steps over and its raw value:
    a: P = (i-1, j-1), no intermediate,  D[P]
    b: P = (i-2, j-1), I = (i-1, j),     D[P] + C[I]
    c: P = (i-1, j-2), I = (i, j-1),     D[P] + C[I]
  score: hit D[X] = max(raw) + 1; miss D[X] = max(0, max_k (raw_k - g(C[P_k]))).
  chosen predecessor: the FIRST of a, b, c attaining the maximum (raw values on a hit, penalised
    values on a miss; strictly greater replaces, equal does not). A hit whose maximum is 0 has none
    (a path starts at X), nor has a cell with D[X] == 0.
  path: the chain from the end cell backwards. At X with chosen k: if I exists and C[I] is set, I is
    on the path; if D[P] > 0 the chain continues at P, otherwise the path begins at I (then a hit).
    A P in row or column 0 or 1 has D = 0; an I may lie in row 1 or column 1 and is reported.
  end cell: the first cell in row-major order holding dmax. segment: (first path cell, end cell) or
    (-1, -1, -1, -1) if dmax is 0.
  order, steps: origin to end; (1, 1), (2, 1), (1, 2) and, exactly after an intermediate, (1, 0) and
    (0, 1). At most path_bound(M, N) = floor(2 (M + N) / 3) - 2 cells (M, N >= 3).

dmax_path is one vectorised step per row (rows i-1 and i-2 suffice) that fills a plane of codes
(0 = none, 1 / 2 / 3 = a / b / c) and walks it back, returning the segment too; dmax_path_cells is
the definition cell by cell with the predecessor order exposed; resum re-accumulates a path's score.
"""
import numpy as np

from qmax_trace_np import GAMMAS, SEEDS, SHAPES, make_matrix  # noqa: F401  (shared with the Qmax tests)

F = np.float32
NONE = (-1, -1, -1, -1)
EMPTY = np.zeros((0, 2), np.int32)
PRED = {1: (1, 1), 2: (2, 1), 3: (1, 2)}   # code -> (di, dj) back to P
INTER = {2: (1, 0), 3: (0, 1)}             # code -> (di, dj) back to I
STEPS = {(1, 1), (2, 1), (1, 2), (1, 0), (0, 1)}


def path_bound(M, N):
    """The most cells a path can have (the proof: csrc/crp_internal.hpp dmax_path_bound)."""
    return 0 if M < 3 or N < 3 else 2 * (M + N) // 3 - 2


def _walk(C, code, positive, end):
    """The chain from `end` backwards over a plane of codes; positive(P): D[P] > 0."""
    path, x = [end], end
    while code[x]:
        k, (i, j) = int(code[x]), x
        P = (i - PRED[k][0], j - PRED[k][1])
        if k in INTER:
            I = (i - INTER[k][0], j - INTER[k][1])
            if C[I]:
                path.append(I)
        if not positive(P):
            break
        path.append(P)
        x = P
    return np.array(path[::-1], np.int32)


def dmax_path(C, gamma_open=0.5, gamma_ext=0.5):
    """(dmax as float, path (n, 2) int32 of (i, j), origin first, segment (i0, j0, i1, j1))."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    if M < 3 or N < 3:
        return 0.0, EMPTY, NONE
    go, ge = F(gamma_open), F(gamma_ext)
    d1, d2 = np.zeros(N, F), np.zeros(N, F)  # rows i-1, i-2
    code = np.zeros((M, N), np.uint8)
    pos = np.zeros((M, N), bool)             # D > 0
    best, end = F(0), None
    for i in range(2, M):
        hit = C[i, 2:]
        raw = np.stack([d1[1:N - 1],                                   # a
                        d2[1:N - 1] + C[i - 1, 2:].astype(F),          # b: + C[i-1, j]
                        d1[0:N - 2] + C[i, 1:N - 1].astype(F)])        # c: + C[i, j-1]
        Cp = np.stack([C[i - 1, 1:N - 1], C[i - 2, 1:N - 1], C[i - 1, 0:N - 2]])
        pen = (raw - np.where(Cp, go, ge).astype(F)).astype(F)
        P = np.where(hit[None, :], raw, pen)
        k = np.argmax(P, axis=0)                                       # first maximum
        mx = np.take_along_axis(P, k[None, :], 0)[0]
        v = np.where(hit, mx + F(1), np.maximum(mx, F(0))).astype(F)
        c = np.where(hit & (mx == 0), 0, k + 1)
        code[i, 2:] = np.where(v > 0, c, 0)
        pos[i, 2:] = v > 0
        d0 = np.zeros(N, F)
        d0[2:] = v
        rm = v.max()
        if rm > best:                                                  # first row, then first column
            best, end = rm, (i, int(np.argmax(v)) + 2)
        d2, d1 = d1, d0
    if end is None:
        return 0.0, EMPTY, NONE
    path = _walk(C, code, lambda p: bool(pos[p]), end)
    return float(best), path, (int(path[0, 0]), int(path[0, 1]), end[0], end[1])


def dmax_path_cells(C, gamma_open=0.5, gamma_ext=0.5, order=(0, 1, 2)):
    """The definition cell by cell: (dmax, path, score matrix D). order: the predecessor priority, a
    permutation of (0, 1, 2) = (a, b, c), exposed so a test can show that the shared matrices tell
    the orders apart on the path itself."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    go, ge = F(gamma_open), F(gamma_ext)
    D = np.zeros((M, N), F)
    code = np.zeros((M, N), np.uint8)
    best, end = F(0), None
    for i in range(2, M):
        for j in range(2, N):
            pred = [(i - 1, j - 1), (i - 2, j - 1), (i - 1, j - 2)]
            raw = [D[pred[0]], F(D[pred[1]] + F(C[i - 1, j])), F(D[pred[2]] + F(C[i, j - 1]))]
            vals = raw if C[i, j] else [F(raw[t] - (go if C[pred[t]] else ge)) for t in range(3)]
            k = order[0]
            for t in order[1:]:
                if vals[t] > vals[k]:
                    k = t
            if C[i, j]:
                v = F(vals[k] + F(1))
                has = vals[k] != 0
            else:
                v = max(F(0), vals[k])
                has = v > 0
            if has:
                code[i, j] = k + 1
            D[i, j] = v
            if v > best:
                best, end = v, (i, j)
    if end is None:
        return 0.0, EMPTY, D
    return float(best), _walk(C, code, lambda p: D[p] > 0, end), D


def resum(C, path, gamma_open=0.5, gamma_ext=0.5):
    """The score re-accumulated in float32 along a path, origin to end: +1 per intermediate cell (a
    cell left by a (1, 0) or (0, 1) step: the bonus), +1 per other cell that is a hit, -g(C[P]) per
    other cell that is a miss, P taken geometrically from the step into that cell ((1, 1), (2, 1),
    (1, 2) back from it, reached over the intermediate or not), since it may be off the path: a
    path that begins on an intermediate has its first P outside. A miss with no cell before it
    cannot begin a path."""
    C = np.asarray(C).astype(bool)
    go, ge = F(gamma_open), F(gamma_ext)
    n = len(path)
    s = F(0)
    t = 0
    while t < n:
        i, j = (int(x) for x in path[t])
        if t + 1 < n and (int(path[t + 1][0]) - i, int(path[t + 1][1]) - j) in ((1, 0), (0, 1)):
            # an intermediate: the cell after it is the DP cell X, P lies behind the pair
            s = F(s + F(1))
            xi, xj = (int(x) for x in path[t + 1])
            P = (xi - 2, xj - 1) if (xi - i, xj - j) == (1, 0) else (xi - 1, xj - 2)
            t += 1
        else:
            xi, xj = i, j
            if t == 0:
                P = None
            else:
                pi, pj = (int(x) for x in path[t - 1])
                P = (pi, pj)
        if C[xi, xj]:
            s = F(s + F(1))
        else:
            s = F(s - (go if C[P] else ge))
        t += 1
    return float(s)


def make_staircase(M, N, start, pattern):
    """An M x N uint8 matrix that holds one planted alignment and nothing else: the hit `start`
    = (i, j), then step after step of `pattern` (a string over "abc", repeated) while the next cell
    fits, each step setting its DP cell X and, for b ((2, 1)) and c ((1, 2)), the intermediate cell
    it passes, so a b / c staircase gains 2 per step and its path has two cells per step."""
    C = np.zeros((M, N), np.uint8)
    i, j = start
    C[i, j] = 1
    t = 0
    while True:
        s = pattern[t % len(pattern)]
        t += 1
        di, dj = {"a": (1, 1), "b": (2, 1), "c": (1, 2)}[s]
        if i + di >= M or j + dj >= N:
            return C
        if s != "a":
            C[i + 1, j + 1] = 1   # the intermediate: (X.i - 1, X.j) of a b step, (X.i, X.j - 1) of a c step
        i, j = i + di, j + dj
        C[i, j] = 1


_CACHE = {}


def expected_path(M, N, density, run, seed, go, ge):
    """(matrix, dmax, path, segment) of one case of SHAPES x SEEDS x GAMMAS; computed once per
    process and shared."""
    key = (M, N, density, run, seed, go, ge)
    if key not in _CACHE:
        C = make_matrix(M, N, density, run, seed)
        _CACHE[key] = (C,) + dmax_path(C, go, ge)
    return _CACHE[key]


# Staircases planted over a sparse background, so that a b step's predecessor and intermediate lie
# on either side of a lane, strip or band edge of both rows-per-lane choices (rows 32 / 64, 512,
# 1024, 2048). The pattern "bcb" advances 5 rows per period, so along ~90 rows every residue of the
# 8- and 16-row lane edges is met by a P, an I and an X. (M, N, first row, first column, seed)
STAIRS = [(70, 70, 3, 4, 0), (560, 120, 470, 5, 1), (1060, 100, 985, 3, 2), (2100, 90, 2005, 4, 0)]


def expected_stairs(M, N, i0, j0, seed):
    """(matrix, dmax, path, segment) of one STAIRS case at the default gammas; cached."""
    key = ("stairs", M, N, i0, j0, seed)
    if key not in _CACHE:
        C = make_matrix(M, N, 0.03, None, seed)
        S = np.zeros_like(C)
        rows, cols = min(M - i0, 95), N - j0
        S[i0:i0 + rows, j0:j0 + cols] = make_staircase(rows, cols, (0, 0), "bcb")
        C = C | S
        _CACHE[key] = (C,) + dmax_path(C)
    return _CACHE[key]
