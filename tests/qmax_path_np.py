"""TEST INFRASTRUCTURE: numpy restatement of the Qmax alignment path (acoss_crp_path /
acoss_path_crp). Not a test module.

Contract: that of tests/qmax_trace_np.py (its matrices, scores and segments are shared), with the
chosen predecessor of every cell kept instead of its origin. Q is the serra09 score matrix, the
predecessors of (i, j) in the fixed order a = (i-1, j-1), b = (i-2, j-1), c = (i-1, j-2); the
chosen one is the FIRST attaining the maximum (raw values on a hit, penalised values on a miss).
A hit whose predecessors are all 0 has none (a path starts there), nor has a cell with Q == 0.
The path is the chain of chosen predecessors from the end cell (the first cell in row-major order
with Q == Qmax) back to a cell without one, reported from origin to end; empty if Qmax is 0.

qmax_path is one vectorised step per row that fills a direction plane (0 = none, 1 / 2 / 3 =
a / b / c) and then walks it back; qmax_path_cells is the definition cell by cell, with the
predecessor order exposed.
"""
import numpy as np

F = np.float32
STEP = {1: (1, 1), 2: (2, 1), 3: (1, 2)}  # code -> (di, dj) back to the predecessor
EMPTY = np.zeros((0, 2), np.int32)


def qmax_path(C, gamma_open=0.5, gamma_ext=0.5):
    """(Qmax as float, path (n, 2) int32 of (i, j), origin first) of a binary matrix."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    if M < 3 or N < 3:
        return 0.0, EMPTY
    go, ge = F(gamma_open), F(gamma_ext)
    q1, q2 = np.zeros(N, F), np.zeros(N, F)  # rows i-1, i-2
    D = np.zeros((M, N), np.uint8)
    best, end = F(0), None
    for i in range(2, M):
        hit = C[i, 2:]
        Q = np.stack([q1[1:N - 1], q2[1:N - 1], q1[0:N - 2]])                # a, b, c
        Cp = np.stack([C[i - 1, 1:N - 1], C[i - 2, 1:N - 1], C[i - 1, 0:N - 2]])
        pen = (Q - np.where(Cp, go, ge).astype(F)).astype(F)
        P = np.where(hit[None, :], Q, pen)
        k = np.argmax(P, axis=0)                                             # first maximum
        mx = np.take_along_axis(P, k[None, :], 0)[0]
        v = np.where(hit, mx + F(1), np.maximum(mx, F(0))).astype(F)
        code = np.where(hit & (mx == 0), 0, k + 1)
        D[i, 2:] = np.where(v > 0, code, 0)
        q0 = np.zeros(N, F)
        q0[2:] = v
        rm = v.max()
        if rm > best:                                                        # first row, then first column
            best, end = rm, (i, int(np.argmax(v)) + 2)
        q2, q1 = q1, q0
    if end is None:
        return 0.0, EMPTY
    path = [end]
    while D[path[-1]]:
        (i, j), (di, dj) = path[-1], STEP[int(D[path[-1]])]
        path.append((i - di, j - dj))
    return float(best), np.array(path[::-1], np.int32)


def qmax_path_cells(C, gamma_open=0.5, gamma_ext=0.5, order=(0, 1, 2)):
    """The definition cell by cell. order: the predecessor priority, a permutation of
    (0, 1, 2) = (a, b, c), exposed so a test can show that the shared matrices tell the orders
    apart on the path itself."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    go, ge = F(gamma_open), F(gamma_ext)
    Q = np.zeros((M, N), F)
    prev = {}
    best, end = F(0), None
    for i in range(2, M):
        for j in range(2, N):
            pred = [(i - 1, j - 1), (i - 2, j - 1), (i - 1, j - 2)]
            if C[i, j]:
                vals = [Q[p] for p in pred]
            else:
                vals = [F(Q[p] - (go if C[p] else ge)) for p in pred]
            k = order[0]
            for t in order[1:]:
                if vals[t] > vals[k]:
                    k = t
            if C[i, j]:
                v = F(vals[k] + F(1))
                if vals[k] != 0:
                    prev[i, j] = pred[k]
            else:
                v = max(F(0), vals[k])
                if v > 0:
                    prev[i, j] = pred[k]
            Q[i, j] = v
            if v > best:
                best, end = v, (i, j)
    if end is None:
        return 0.0, EMPTY
    path = [end]
    while path[-1] in prev:
        path.append(prev[path[-1]])
    return float(best), np.array(path[::-1], np.int32)


_CACHE = {}


def expected_path(M, N, density, run, seed, go, ge):
    """(matrix, score, path) of one case of qmax_trace_np's SHAPES x SEEDS x GAMMAS; computed once
    per process and shared."""
    import qmax_trace_np as qt
    key = (M, N, density, run, seed, go, ge)
    if key not in _CACHE:
        C = qt.make_matrix(M, N, density, run, seed)
        _CACHE[key] = (C,) + qmax_path(C, go, ge)
    return _CACHE[key]


def score_matrix(C, gamma_open=0.5, gamma_ext=0.5):
    """The whole serra09 score matrix Q (float32), row by row; for checks of Q along a path."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    Q = np.zeros((M, N), F)
    if M < 3 or N < 3:
        return Q
    go, ge = F(gamma_open), F(gamma_ext)
    for i in range(2, M):
        q1, q2 = Q[i - 1], Q[i - 2]
        hit = C[i, 2:]
        Qs = np.stack([q1[1:N - 1], q2[1:N - 1], q1[0:N - 2]])
        Cp = np.stack([C[i - 1, 1:N - 1], C[i - 2, 1:N - 1], C[i - 1, 0:N - 2]])
        pen = (Qs - np.where(Cp, go, ge).astype(F)).astype(F)
        mx = np.where(hit[None, :], Qs, pen).max(axis=0)
        Q[i, 2:] = np.where(hit, mx + F(1), np.maximum(mx, F(0)))
    return Q
