"""TEST INFRASTRUCTURE: restatement of the OTI-binary CRP (Serra08; include/acoss_hip.h,
acoss_crp_params2) on the CPU oracle, and the inputs the OTI-binary tests share. Not a test module.

The definition, for a pair (query X, reference Y), m, tau, oti and oti_rank in 1 .. 12:
  g = the pair's global OTI as under the percentile CRP (oracle.oti of the two track profiles), 0
    when oti is off.
  D_k = oracle.crp_dist(X, Y, (g + k) % 12, m, tau), k = 0 .. 11: the canonical float32 stacked
    distances with every reference frame rolled by (g + k) mod 12.
  closer(i, j) = #{k in 1 .. 11 : D_k(i, j) < D_0(i, j)}, strict, on those float32 values.
  C(i, j) = 1 iff closer(i, j) < oti_rank.
Twelve oracle.crp_dist calls per pair, nothing else. The scores of a mask come from oracle.align,
the segments, paths and CRQA values from qmax_trace_np, qmax_path_np, dmax_path_np and rqa_np
applied to that mask.
"""
import numpy as np

import oracle
import dmax_path_np
import qmax_path_np
import qmax_trace_np
import rqa_np
from acoss import synthetic


def global_oti(X, Y, oti=True):
    return oracle.oti(oracle.profile(X), oracle.profile(Y)) if oti else 0


def otib(X, Y, m=9, tau=1, oti=True, oti_rank=1):
    """{'oti': g, 'dist': D_0, 'closer': uint8 (M' x N'), 'crp': uint8 (M' x N')} of one pair."""
    if not 1 <= oti_rank <= 12:
        raise ValueError("oti_rank must lie in 1 .. 12")
    g = global_oti(X, Y, oti)
    D = [oracle.crp_dist(X, Y, (g + k) % 12, m, tau) for k in range(12)]
    closer = np.zeros(D[0].shape, np.uint8)
    for k in range(1, 12):
        closer += D[k] < D[0]
    return {"oti": g, "dist": D[0], "closer": closer, "crp": (closer < oti_rank).astype(np.uint8)}


def otib_ranks(X, Y, m=9, tau=1, oti=True, ranks=(1, 2, 12)):
    """{rank: otib(..., oti_rank=rank)} from one set of twelve distance matrices."""
    one = otib(X, Y, m, tau, oti, 1)
    return {k: dict(one, crp=(one["closer"] < k).astype(np.uint8)) for k in ranks}


def density(C):
    return float(np.mean(C)) if C.size else 0.0


def aligned(C, gamma_open=0.5, gamma_ext=0.5, lmin=2):
    """What the seven entries report for a mask: Qmax and dmax (oracle.align), the located segments,
    the paths and the CRQA values of the four restatements."""
    qseg = qmax_trace_np.qmax_trace(C, gamma_open, gamma_ext)[1]
    _, qpath = qmax_path_np.qmax_path(C, gamma_open, gamma_ext)
    _, dpath, dseg = dmax_path_np.dmax_path(C, gamma_open, gamma_ext)
    return {"qmax": oracle.align(C, gamma_open, gamma_ext, 0), "dmax": oracle.align(C, gamma_open, gamma_ext, 1),
            "qseg": tuple(int(v) for v in qseg), "dseg": tuple(int(v) for v in dseg), "qpath": qpath, "dpath": dpath,
            "rqa": rqa_np.rqa(C, lmin)}


# ---- shared inputs: tracks of the hard corpus (phrases in random keys, covers rolled by a random
# number of bins: transposed material) cut to length ----
_POOL = {}


def hard_tracks(frames=400, seed=5):
    if (frames, seed) not in _POOL:
        _POOL[frames, seed] = synthetic.make_hard_corpus("covers80", frames=frames, seed=seed, fixed_length=True)
    return _POOL[frames, seed]


def cut_pair(nq, nr, which=0):
    """A query of nq and a reference of nr frames: a song of the hard corpus and a cover of it (the
    cover is rolled on the chroma axis), cut to length."""
    tracks, labels = hard_tracks()
    members = np.flatnonzero(labels == labels[np.flatnonzero(np.bincount(labels) > 1)[which]])
    X, Y = tracks[members[0]], tracks[members[1]]
    return np.ascontiguousarray(X[:nq]), np.ascontiguousarray(Y[len(Y) - nr:])


def frames_for(stacked, m=9, tau=1):
    """The fewest frames whose stacked length is `stacked`."""
    return (stacked - 1) * tau + m * tau + 1


# ---- the constructed tie cases ----
def roll5_track(n=60, seed=2):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.random((n, 12)).astype(np.float32)
    return X, np.ascontiguousarray(np.roll(X, 5, axis=1))


def zero_block_track(n=80, start=20, length=12, seed=3):
    """A track with `length` >= m tau + 1 zero frames from `start` on (m = 9, tau = 1: stacked frames
    start .. start + length - 9 are all zero)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.random((n, 12)).astype(np.float32)
    X[start:start + length] = 0.0
    return X


def constant_track(n=50, value=0.25):
    return np.full((n, 12), value, np.float32)
