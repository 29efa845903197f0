"""The SiMPle self-join restated in numpy: the definition of acoss_simple_self_profile
(include/acoss_hip.h) with its loops written out.

A helper, not a test. The distance is simple_profile_np's canonical one (frame dots by the fma
chain in rational arithmetic, sequential window sums, dist = (s[j] + s[i]) - 2 qt) with query =
reference = the track and no roll; the row minimum runs over the columns with |i - j| > excl and
keeps the first of equal distances (`dist < mn`).
"""
import numpy as np

from simple_profile_np import _chain, _window_sums, frame_dots


def self_dist_np(A, L, ga=None):
    """The (P x P) canonical distance matrix of track A (12, n) against itself; P = n - L + 1 > 0.
    ga: frame_dots(A, A) if already formed (it depends on no L)."""
    A = np.asarray(A, np.float64)
    P = A.shape[1] - L + 1
    if ga is None:
        ga = frame_dots(A, A)
    s = _window_sums(_chain(A, A), L, P)
    qt = np.zeros((P, P), np.float64)
    for t in range(L):
        qt = qt + ga[t:t + P, t:t + P]
    with np.errstate(invalid="ignore"):
        return (s[None, :] + s[:, None]) - 2.0 * qt


def masked_profile_np(dist, excl):
    """(mp, mpi) of a (P x P) distance matrix without the band |i - j| <= excl: the definition's
    loops. NaN and -1 where a row has no admissible distance below +inf."""
    P = dist.shape[0]
    mp = np.full(P, np.nan)
    mpi = np.full(P, -1, np.int32)
    for i in range(P):
        mn = np.inf
        for j in range(P):
            if abs(i - j) > excl and dist[i, j] < mn:
                mn = dist[i, j]
                mpi[i] = j
        if mpi[i] >= 0:
            mp[i] = mn
    return mp, mpi


def simple_self_np(A, L, excl, ga=None):
    """(mp float64 (P,), mpi int32 (P,)) of the self-join of A; empty when P = n - L + 1 <= 0."""
    A = np.asarray(A, np.float64)
    if A.shape[1] - L + 1 <= 0:
        return np.zeros(0, np.float64), np.zeros(0, np.int32)
    return masked_profile_np(self_dist_np(A, L, ga), excl)


def motif_discord_np(mp, mpi):
    """((i*, mpi[i*]), discord): i* the smallest row attaining the minimum of mp over its rows that
    are not NaN, discord the smallest row attaining their maximum; ((-1, -1), -1) without one."""
    mp = np.asarray(mp, np.float64)
    best = worst = -1
    for i in range(len(mp)):
        if np.isnan(mp[i]):
            continue
        if best < 0 or mp[i] < mp[best]:
            best = i
        if worst < 0 or mp[i] > mp[worst]:
            worst = i
    if best < 0:
        return (-1, -1), -1
    return (best, int(mpi[best])), worst
