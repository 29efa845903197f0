"""The SiMPle matrix profile and its index, restated from oracle/crp_oracle.cpp or_simple_sim.

A helper, not a test. Every operation is the oracle's, in the oracle's order, in float64: the
frame dot is the product of bin 0 followed by an fma chain over the reference's own bins 1..11
(paired with the query's bin (j + k) mod 12), frame norms likewise, window sums are sequential
adds, dist = (sb[j] + sa[i]) - 2 qt, and the row minimum keeps the first of equal distances (the
loop's `dist < mn`). numpy has no fma: it is emulated exactly in rational arithmetic (CPython
rounds int / int correctly). What the oracle reduces to a median is returned whole:

    mp[i]  = min_j dist(i, j), NaN where no distance is below +inf
    mpi[i] = the smallest j attaining it, -1 where there is none

which is the definition of acoss_simple_profile (include/acoss_hip.h).
"""
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """round(a * b + c), one rounding."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c  # NaN or inf either way; no test depends on which
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c  # a * b == -c is exact then, and the float sum has the sign fma gives
    return float(r)


def _chain(U, V):
    """sum_d U[d] * V[d] per column: the product for d = 0, then the fma chain d = 1..11."""
    out = np.empty(U.shape[1:], np.float64)
    for idx in np.ndindex(*out.shape):
        acc = U[(0,) + idx] * V[(0,) + idx]
        for d in range(1, 12):
            acc = fma(U[(d,) + idx], V[(d,) + idx], acc)
        out[idx] = acc
    return out


def frame_dots(A, B, k=0):
    """ga[x, y] = <A[:, x], roll(B, k)[:, y]> in the canonical order; depends on no sslen."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    Ak = A[(np.arange(12) + k) % 12]  # row d: the query bin paired with the reference's bin d
    na, nb = A.shape[1], B.shape[1]
    return _chain(np.broadcast_to(Ak[:, :, None], (12, na, nb)), np.broadcast_to(B[:, None, :], (12, na, nb)))


def _window_sums(v, L, n):
    acc = np.zeros(max(n, 0), np.float64)
    for t in range(L):
        acc = acc + v[t:t + n]
    return acc


def simple_profile_np(A, B, L=10, k=0, ga=None):
    """(mp float64 (P,), mpi int32 (P,)) of query A against reference B rolled by k; (12, n) blocks.
    P = na - L + 1 rows (none if that is <= 0); with Q = nb - L + 1 <= 0 every row is (NaN, -1)."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    na, nb = A.shape[1], B.shape[1]
    P, Q = na - L + 1, nb - L + 1
    if P <= 0:
        return np.zeros(0, np.float64), np.zeros(0, np.int32)
    mp = np.full(P, np.nan)
    mpi = np.full(P, -1, np.int32)
    if Q <= 0:
        return mp, mpi
    if ga is None:
        ga = frame_dots(A, B, k)
    sa = _window_sums(_chain(A, A), L, P)
    sb = _window_sums(_chain(B, B), L, Q)
    qt = np.zeros((P, Q), np.float64)
    for t in range(L):
        qt = qt + ga[t:t + P, t:t + Q]
    with np.errstate(invalid="ignore"):
        dist = (sb[None, :] + sa[:, None]) - 2.0 * qt
    for i in range(P):
        mn = np.inf
        for j in range(Q):
            if dist[i, j] < mn:
                mn = dist[i, j]
                mpi[i] = j
        if mpi[i] >= 0:
            mp[i] = mn
    return mp, mpi


def unit_columns(rng, n):
    """(12, n) non-negative columns of unit L2 norm, as SiMPle features are."""
    F = np.abs(rng.standard_normal((12, n)))
    return F / np.linalg.norm(F, axis=0, keepdims=True)


def dist_matrix(A, B, L, k=0):
    """The (P x Q) distance matrix in plain float64 numpy (BLAS dots, no canonical order): within
    about 40 roundings of values of magnitude <= 20 of the canonical one, 9e-14 per entry."""
    A = np.asarray(A, np.float64)
    B = np.roll(np.asarray(B, np.float64), k, axis=0)
    P, Q = A.shape[1] - L + 1, B.shape[1] - L + 1
    G = A.T @ B
    qt = np.zeros((P, Q))
    for t in range(L):
        qt += G[t:t + P, t:t + Q]
    sa = _window_sums((A * A).sum(0), L, P)
    sb = _window_sums((B * B).sum(0), L, Q)
    return (sb[None, :] + sa[:, None]) - 2.0 * qt
