"""TEST INFRASTRUCTURE: restatement of the ranked OTI and of best-of-n (include/acoss_hip.h,
acoss_crp_params3) on the CPU oracle, and the inputs the ranked-OTI tests share. Not a test module.

The definition, for a pair (query X, reference Y) with profiles pq = oracle.profile(X), pr =
oracle.profile(Y):
  dot_k = the float32 chain acc = fmaf(pq[c], pr[(c - k + 12) % 12], acc), c = 0 .. 11 from acc = 0.
    Restated exactly: product and sum in exact rationals (fractions.Fraction), ONE round-to-nearest-
    even to float32 per step. (A float64 product and sum rounded to float32 rounds twice.)
  order = the twelve shifts sorted by dot_k descending, equal dots keeping the smaller shift first.
  pick r applies order[r] where the OTI is applied: the percentile CRP at that shift is crp_at, the
    OTI-binary CRP is otib_np.otib's definition with g = order[r].
  best of n: the maximum over picks 0 .. n - 1, folded in pick order with a strict >.
The scores of a mask come from oracle.align, the segments, paths and CRQA values from otib_np.aligned.
"""
from fractions import Fraction

import numpy as np

import oracle
import otib_np


def _rn32(x):
    """The float32 nearest to the rational x, ties to even (finite, no overflow)."""
    if x == 0:
        return np.float32(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)                                            # below: the subnormal spacing
    ulp = Fraction(2) ** (e - 23)
    n = round(a / ulp)                                          # Fraction.__round__: ties to even
    v = np.float32(float(n * ulp))                              # exact: n < 2^25, a power-of-two scale
    return -v if x < 0 else v


def dots(pq, pr):
    """float32[12]: dot_k of two float32 profiles, the fmaf chain restated exactly."""
    pq = [Fraction(float(v)) for v in np.asarray(pq, np.float32)]
    pr = [Fraction(float(v)) for v in np.asarray(pr, np.float32)]
    out = np.zeros(12, np.float32)
    for k in range(12):
        acc = np.float32(0.0)
        for c in range(12):
            acc = _rn32(pq[c] * pr[(c - k + 12) % 12] + Fraction(float(acc)))
        out[k] = acc
    return out


def ranked(pq, pr):
    """(order int32[12], dots float32[12]) of two profiles."""
    d = dots(pq, pr)
    order = sorted(range(12), key=lambda k: (-float(d[k]), k))
    return np.array(order, np.int32), d


def ranked_tracks(X, Y):
    return ranked(oracle.profile(X), oracle.profile(Y))


def crp_at(X, Y, shift, m=9, tau=1, kappa=0.095):
    """The percentile CRP of the pair with the reference rolled by `shift`: {'oti', 'dist', 'thr_row',
    'thr_col', 'crp'} as acoss_crp_pair reports them."""
    D = oracle.crp_dist(X, Y, int(shift), m, tau)
    tr, tc = oracle.crp_thresholds(D, kappa)
    C = ((D <= tr[:, None]) & (D <= tc[None, :])).astype(np.uint8)
    return {"oti": int(shift), "dist": D, "thr_row": tr, "thr_col": tc, "crp": C}


def otib_at(X, Y, g, m=9, tau=1, oti_rank=1):
    """otib_np.otib's definition with g given: {'oti', 'dist', 'closer', 'crp'}."""
    D = [oracle.crp_dist(X, Y, (int(g) + k) % 12, m, tau) for k in range(12)]
    closer = np.zeros(D[0].shape, np.uint8)
    for k in range(1, 12):
        closer += D[k] < D[0]
    return {"oti": int(g), "dist": D[0], "closer": closer, "crp": (closer < oti_rank).astype(np.uint8)}


def pick_at(X, Y, pick, m=9, tau=1, kappa=0.095, binarize="percentile", oti_rank=1, order=None):
    """What acoss_crp_pair3 reports at `pick`."""
    order = ranked_tracks(X, Y)[0] if order is None else order
    if binarize == "oti":
        return otib_at(X, Y, order[pick], m, tau, oti_rank)
    return crp_at(X, Y, order[pick], m, tau, kappa)


def scored_picks(X, Y, n, m=9, tau=1, kappa=0.095, binarize="percentile", oti_rank=1, gamma_open=0.5, gamma_ext=0.5):
    """[{'oti', 'crp', 'qmax', 'dmax'}] of picks 0 .. n - 1."""
    order = ranked_tracks(X, Y)[0]
    rows = []
    for r in range(n):
        at = pick_at(X, Y, r, m, tau, kappa, binarize, oti_rank, order)
        rows.append({"oti": at["oti"], "crp": at["crp"], "qmax": oracle.align(at["crp"], gamma_open, gamma_ext, 0),
                     "dmax": oracle.align(at["crp"], gamma_open, gamma_ext, 1)})
    return rows


def best_of(rows, key, n=None):
    """(score, shift, pick) of the best of rows[:n] by rows[r][key]: picks folded in order, a strict >."""
    n = len(rows) if n is None else n
    best = 0
    for r in range(1, n):
        if np.float32(rows[r][key]) > np.float32(rows[best][key]):
            best = r
    return np.float32(rows[best][key]), int(rows[best]["oti"]), best


# ---- shared inputs ----
def hard_cut(a, nq, b, nr):
    """Tracks a and b of otib_np.hard_tracks(200, 5) cut to their first nq and nr frames."""
    tracks, _ = otib_np.hard_tracks(200, 5)
    return np.ascontiguousarray(tracks[a][:nq]), np.ascontiguousarray(tracks[b][:nr])


def constant_pair():
    K = otib_np.constant_track()
    return K, K


def roll6_invariant_track(n=60, seed=6):
    """Frames with x[c] == x[c + 6]: the track is its own roll by 6, so against itself dot_0 and dot_6
    are the same chain of the same products."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h = rng.random((n, 6)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([h, h], axis=1))
