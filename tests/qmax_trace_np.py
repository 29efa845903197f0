"""TEST INFRASTRUCTURE: numpy restatement of the located Qmax (acoss_crp_locate / acoss_locate_crp)
and the binary matrices the locate tests share. Not a test module.

Contract. C is a binary M x N matrix, Q the serra09 score matrix of oracle/crp_oracle.cpp or_align
(which = 0), all arithmetic float32, cells with i < 2 or j < 2 are 0, gamma(c) = gamma_open if c is
set else gamma_ext. The predecessors of (i, j) in this fixed order: a = (i-1, j-1), b = (i-2, j-1),
c = (i-1, j-2).
  hit:   Q = max(Qa, Qb, Qc) + 1;   miss:  Q = max(0, Qa - g(Ca), Qb - g(Cb), Qc - g(Cc))
  origin O (where Q > 0): a hit whose max(Qa, Qb, Qc) is 0 starts a path, O = (i, j); otherwise
  the origin of the FIRST predecessor (order a, b, c) attaining the maximum, taken over the raw
  values on a hit and over the penalised values on a miss.
  end cell: the first cell in row-major order with Q == Qmax.   segment: (O[end], end), or
  (-1, -1, -1, -1) if Qmax is 0.

qmax_trace is one vectorised step per row (row i needs rows i-1 and i-2 only; np.argmax over the
three stacked predecessor rows is "first maximum wins"); qmax_trace_cells is the same definition
cell by cell, kept to check the vectorised form on small matrices.
"""
import numpy as np

NONE = (-1, -1, -1, -1)
F = np.float32


def qmax_trace(C, gamma_open=0.5, gamma_ext=0.5):
    """(Qmax as float, (i0, j0, i1, j1)) of a binary matrix."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    if M < 3 or N < 3:
        return 0.0, NONE
    go, ge = F(gamma_open), F(gamma_ext)
    q1, q2 = np.zeros(N, F), np.zeros(N, F)              # rows i-1, i-2
    o1, o2 = np.full(N, -1, np.int64), np.full(N, -1, np.int64)  # their origins, i0 * 65536 + j0
    cols = np.arange(2, N, dtype=np.int64)
    best, end, org = F(0), None, None
    for i in range(2, M):
        hit = C[i, 2:]
        Q = np.stack([q1[1:N - 1], q2[1:N - 1], q1[0:N - 2]])                # a, b, c
        O = np.stack([o1[1:N - 1], o2[1:N - 1], o1[0:N - 2]])
        Cp = np.stack([C[i - 1, 1:N - 1], C[i - 2, 1:N - 1], C[i - 1, 0:N - 2]])
        pen = (Q - np.where(Cp, go, ge).astype(F)).astype(F)
        P = np.where(hit[None, :], Q, pen)
        k = np.argmax(P, axis=0)                                             # first maximum
        mx = np.take_along_axis(P, k[None, :], 0)[0]
        o = np.take_along_axis(O, k[None, :], 0)[0]
        v = np.where(hit, mx + F(1), np.maximum(mx, F(0))).astype(F)
        o = np.where(hit & (mx == 0), i * 65536 + cols, o)
        o = np.where(v > 0, o, -1)
        q0, o0 = np.zeros(N, F), np.full(N, -1, np.int64)
        q0[2:], o0[2:] = v, o
        rm = v.max()
        if rm > best:                                                        # first row, then first column
            j = int(np.argmax(v))
            best, end, org = rm, (i, j + 2), int(o[j])
        q2, o2, q1, o1 = q1, o1, q0, o0
    if end is None:
        return 0.0, NONE
    return float(best), (org >> 16, org & 0xffff, end[0], end[1])


def qmax_trace_cells(C, gamma_open=0.5, gamma_ext=0.5, order=(0, 1, 2), last_end=False):
    """The definition cell by cell. order / last_end are the two tie rules, exposed so a test can
    show that the shared matrices tell the rules apart (order: the predecessor priority, a
    permutation of (0, 1, 2) = (a, b, c); last_end: the last maximal cell instead of the first)."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    go, ge = F(gamma_open), F(gamma_ext)
    Q = np.zeros((M, N), F)
    O = {}
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
                O[i, j] = (i, j) if vals[k] == 0 else O[pred[k]]
            else:
                v = max(F(0), vals[k])
                if v > 0:
                    O[i, j] = O[pred[k]]
            Q[i, j] = v
            if v > best or (last_end and v == best and v > 0):
                best, end = v, (i, j)
    if end is None:
        return 0.0, NONE
    return float(best), O[end] + end


# ---- the binary matrices of the locate tests (host and GPU) ----
GAMMAS = [(0.5, 0.5), (0.0, 0.0), (0.7, 0.3), (1.0, 0.5)]
SEEDS = [0, 1, 2]
# (M, N, density, planted run (a, b, L) or None)
SHAPES = [
    (1, 1, 0.15, None), (2, 9, 0.15, None), (3, 40, 0.15, None), (5, 5, 0.5, None),           # degenerate
    (33, 70, 0.15, None), (70, 45, 0.15, None), (40, 300, 0.15, None), (530, 60, 0.15, None),  # dense, tie-rich
    (300, 257, 0.15, None),
    # sparse with a planted run across every row a band, lane or strip edge can fall on
    (560, 120, 0.03, (500, 30, 45)),     # row 512
    (1060, 100, 0.03, (1010, 20, 40)),   # row 1024
    (2100, 90, 0.03, (2030, 25, 40)),    # row 2048
    (100, 1100, 0.03, (30, 1000, 50)),   # many columns, few rows
    (70, 70, 0.03, (20, 25, 30)),        # strip edges at rows 32 and 64
]


def make_matrix(M, N, density, run, seed):
    rng = np.random.Generator(np.random.PCG64(1000 * seed + M + 7 * N))
    C = rng.random((M, N)) < density
    if run is not None:
        a, b, L = run
        keep = rng.random(L) < 0.85
        t = np.flatnonzero(keep)
        C[a + t, b + t] = True
    return C.astype(np.uint8)


_CACHE = {}


def expected(M, N, density, run, seed, go, ge):
    """(matrix, score, segment) of one case; computed once per process and shared."""
    key = (M, N, density, run, seed, go, ge)
    if key not in _CACHE:
        C = make_matrix(M, N, density, run, seed)
        _CACHE[key] = (C,) + qmax_trace(C, go, ge)
    return _CACHE[key]
