"""TEST INFRASTRUCTURE: numpy restatement of the cross-recurrence quantification (acoss_crp_rqa /
acoss_rqa_crp) and the binary matrices the RQA tests share. Not a test module.

Contract (include/acoss_hip.h, acoss_crp_rqa). C is a binary M x N matrix; all M rows and N columns
count. A diagonal line is a maximal run of set cells (i, j), (i+1, j+1), ..., bounded on each side by
an unset cell or the matrix edge; H[l] = the number of lines of length l, 1 <= l <= min(M, N).
  n_rec = set cells = sum l H[l];  n_lines = sum H[l];  n_lines_min = sum_{l >= lmin} H[l];
  n_pts_min = sum_{l >= lmin} l H[l];  lmax = the largest l with H[l] > 0 (0 for an empty matrix)
  RR = n_rec / (M N);  DET = n_pts_min / n_rec;  LMEAN = n_pts_min / n_lines_min  (0 where the
  denominator is 0; one float64 division each)
  ENTR = - sum_{l >= lmin, H[l] > 0} p ln p,  p = H[l] / n_lines_min  (0 when n_lines_min = 0)
  Smax: S = 0 where i < 2 or j < 2 and on a miss; on a hit S = max(S[i-1, j-1], S[i-2, j-1],
  S[i-1, j-2]) + 1; Smax = max S. Equal to qmax_trace_np.qmax_trace(C, inf, inf)[0].

line_hist is vectorised: the difference of the zero-padded matrix along its diagonals (np.diff of
every padded diagonal at once) is +1 where a line starts and -1 one cell past its end; on a diagonal
the k-th start goes with the k-th end. line_hist_cells is the same definition cell by cell, kept to
check the vectorised form on small matrices.
"""
import math

import numpy as np

import qmax_trace_np as qt

COUNT_KEYS = ("n_rec", "n_lines", "n_lines_min", "n_pts_min")
STAT_KEYS = ("rr", "det", "lmean", "entr")
LMINS = (1, 2, 5)


def line_hist(C):
    """H as an int64 array of min(M, N) + 1 bins (bin 0 stays 0)."""
    C = np.asarray(C).astype(np.int8)
    M, N = C.shape
    H = np.zeros(min(M, N) + 1, np.int64)
    if M == 0 or N == 0:
        return H
    P = np.zeros((M + 2, N + 2), np.int8)
    P[1:-1, 1:-1] = C
    d = P[1:, 1:] - P[:-1, :-1]            # d[i, j] = C[i, j] - C[i-1, j-1] in matrix coordinates
    si, sj = np.nonzero(d == 1)            # a line starts on (i, j)
    ei, ej = np.nonzero(d == -1)           # a line ended on (i-1, j-1)
    so = np.lexsort((si, sj - si))         # by diagonal, then along it
    eo = np.lexsort((ei, ej - ei))
    assert np.array_equal((sj - si)[so], (ej - ei)[eo])
    length = ei[eo] - si[so]
    assert (length >= 1).all()
    return np.bincount(length, minlength=len(H)).astype(np.int64)


def line_hist_cells(C):
    """The definition cell by cell."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    H = np.zeros(min(M, N) + 1, np.int64)
    for i in range(M):
        for j in range(N):
            if C[i, j] and not (i > 0 and j > 0 and C[i - 1, j - 1]):
                n = 0
                while i + n < M and j + n < N and C[i + n, j + n]:
                    n += 1
                H[n] += 1
    return H


def smax_cells(C):
    """Smax cell by cell."""
    C = np.asarray(C).astype(bool)
    M, N = C.shape
    S = np.zeros((M, N), np.int64)
    for i in range(2, M):
        for j in range(2, N):
            if C[i, j]:
                S[i, j] = max(S[i - 1, j - 1], S[i - 2, j - 1], S[i - 1, j - 2]) + 1
    return float(S.max()) if S.size else 0.0


def measures(H, M, N, lmin):
    """The integers and the four float64 measures from a histogram."""
    H = np.asarray(H, np.int64)
    ls = np.arange(len(H), dtype=np.int64)
    n_rec = int((ls * H).sum())
    n_lines = int(H.sum())
    n_lines_min = int(H[lmin:].sum())
    n_pts_min = int((ls * H)[lmin:].sum())
    nz = np.flatnonzero(H)
    entr = 0.0
    for l in range(lmin, len(H)):          # ascending order, float64
        if H[l] > 0:
            p = float(H[l]) / float(n_lines_min)
            entr -= p * math.log(p)
    return {
        "n_rec": n_rec, "n_lines": n_lines, "n_lines_min": n_lines_min, "n_pts_min": n_pts_min,
        "lmax": int(nz[-1]) if len(nz) else 0,
        "rr": float(n_rec) / float(M * N) if M * N else 0.0,
        "det": float(n_pts_min) / float(n_rec) if n_rec else 0.0,
        "lmean": float(n_pts_min) / float(n_lines_min) if n_lines_min else 0.0,
        "entr": entr,
    }


def smax(C):
    return qt.qmax_trace(C, np.inf, np.inf)[0]


def rqa(C, lmin):
    """Everything acoss_rqa_crp returns for C: measures(...) plus 'hist' and 'smax'."""
    C = np.asarray(C)
    H = line_hist(C)
    out = measures(H, C.shape[0], C.shape[1], lmin)
    out["hist"] = H
    out["smax"] = smax(C)
    return out


# ---- the shared matrices ----
def _noise(M, N, density, seed):
    rng = np.random.Generator(np.random.PCG64(7000 + 31 * seed + M + 7 * N))
    return (rng.random((M, N)) < density).astype(np.uint8)


def _plant(C, runs):
    for a, b, L in runs:
        t = np.arange(L)
        assert a + L <= C.shape[0] and b + L <= C.shape[1]
        C[a + t, b + t] = 1                # unbroken
    return C


_FILL = [(3, 8, 3), (9, 15, 4)]   # short planted runs, so that a sparse case still fills four bins


def _lanes_full(M, N):
    C = _noise(M, N, 0.15, 5)
    C[M - 1, ::2] = 1                       # hits in the last row of the last lane
    C[M - 1, N - 1] = 1
    return C


# name -> (builder, planted length or None)
CASES = {
    "1x1": (lambda: np.ones((1, 1), np.uint8), None),
    "1x1_empty": (lambda: np.zeros((1, 1), np.uint8), None),
    "2x9": (lambda: _noise(2, 9, 0.5, 1), None),
    "5x5_dense": (lambda: _noise(5, 5, 0.8, 2), None),
    "zeros_70x45": (lambda: np.zeros((70, 45), np.uint8), None),
    "ones_70x45": (lambda: np.ones((70, 45), np.uint8), None),
    "rand_33x70": (lambda: _noise(33, 70, 0.15, 0), None),
    "rand_530x60": (lambda: _noise(530, 60, 0.15, 1), None),
    "rand_300x257": (lambda: _noise(300, 257, 0.15, 2), None),
    # sparse, with an unbroken planted diagonal across every edge the walk has
    "rows32_64_70x70": (lambda: _plant(_noise(70, 70, 0.03, 0), _FILL + [(20, 25, 45)]), 45),
    "row512_560x120": (lambda: _plant(_noise(560, 120, 0.03, 1), _FILL + [(500, 30, 45)]), 45),
    "row1024_1060x100": (lambda: _plant(_noise(1060, 100, 0.03, 2), _FILL + [(1010, 20, 40)]), 40),
    "row2048_2100x90": (lambda: _plant(_noise(2100, 90, 0.03, 3), _FILL + [(2030, 25, 40)]), 40),
    "columns_100x1100": (lambda: _plant(_noise(100, 1100, 0.03, 4), _FILL + [(2, 1000, 95)]), 95),
    # one run each at an edge of the matrix
    "from_row0": (lambda: _plant(_noise(45, 50, 0.15, 5), [(0, 10, 9)]), 9),
    "from_col0": (lambda: _plant(_noise(45, 50, 0.15, 6), [(12, 0, 9)]), 9),
    "to_last_row": (lambda: _plant(_noise(45, 50, 0.15, 7), [(36, 5, 9)]), 9),
    "to_last_col": (lambda: _plant(_noise(45, 50, 0.15, 8), [(3, 41, 9)]), 9),
    "to_corner": (lambda: _plant(_noise(45, 50, 0.15, 9), [(36, 41, 9)]), 9),
    "diag_257x257": (lambda: _plant(_noise(257, 257, 0.03, 10), _FILL + [(0, 0, 257)]), 257),
    # row counts that exactly fill the lanes at 8, 16 and 32 rows per lane
    "lanes_512x40": (lambda: _lanes_full(512, 40), None),
    "lanes_1024x40": (lambda: _lanes_full(1024, 40), None),
    "lanes_2048x40": (lambda: _lanes_full(2048, 40), None),
}
SMALL = ("1x1", "1x1_empty", "2x9", "5x5_dense", "zeros_70x45", "ones_70x45", "rand_33x70", "rows32_64_70x70",
         "from_row0", "from_col0", "to_last_row", "to_last_col", "to_corner")  # cell by cell in the host test

_CACHE = {}


def matrix(name):
    if ("C", name) not in _CACHE:
        _CACHE["C", name] = CASES[name][0]()
    return _CACHE["C", name]


def expected(name, lmin):
    """rqa(matrix(name), lmin); computed once per process and shared."""
    key = (name, lmin)
    if key not in _CACHE:
        C = matrix(name)
        if ("H", name) not in _CACHE:
            _CACHE["H", name] = (line_hist(C), smax(C))
        H, s = _CACHE["H", name]
        out = measures(H, C.shape[0], C.shape[1], lmin)
        out["hist"], out["smax"] = H, s
        _CACHE[key] = out
    return _CACHE[key]
