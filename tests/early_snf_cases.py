"""Cases of acoss_earlyfusion_snf shared by its GPU tests (test_gpu_early_snf*.py) and by the host
test that checks the inputs alone (test_early_snf_host.py) -- TEST INFRASTRUCTURE ONLY.

A case is (feats, pairs, refs): block features per track, an int32 (P, 2) pair list, and per pair the
reference record of the numpy restatement (early_snf_np.py):
  canon   es.early_snf under es.CANON (the kernels' operations in their order)
  numpy   es.early_snf under es.NUMPY (numpy's float32 exp, pairwise row sums)
  bound   8 x the largest relative deviation between the two cross blocks; None where the
          reference cannot fuse the pair (es.pair_ok)
  stable  equal binaries under both, and the top-nn gap of every row of canon's cross above bound
Nothing here reads GPU output: bounds and stability come from the restatement's own two evaluations.

Two feature makers. EXACT: the integer-exact blocks of test_gpu_earlyfusion_pin.py (every float32
distance exact in any summation order; distances from es.distances). FLOAT: general float32 blocks,
whose distances must come from oracle.ef_csm, the kernels' canonical order (es.distances sums in
BLAS order, which is not theirs).
"""
import functools
from collections import namedtuple

import numpy as np

import early_snf_np as es
import oracle
from test_gpu_earlyfusion_pin import _clique_blocks, _cover

DIMS = {"mfccs": 1000, "ssms": 1225, "chromas": 480}


def rel_dev(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- feature makers --------------------------------------------------------------------------------
def _exact_cover(rng, base, nb):
    bf = _cover(rng, base, nb)
    bf["chroma_med"] = rng.permutation(12).astype(np.float32)
    return bf


def _float_base(rng, nb):
    out = {k: rng.standard_normal((nb, d)).astype(np.float32) for k, d in DIMS.items()}
    out["ssms"], out["chromas"] = np.abs(out["ssms"]), np.abs(out["chromas"])
    return out


def _float_cover(rng, base, nb):
    """The base resampled to nb blocks from a random start, plus 0.3 x normal noise (ssms and chromas
    kept non-negative); chroma_med the abs of a normal draw."""
    n0 = len(base["mfccs"])
    idx = np.minimum((np.arange(nb) * (n0 / nb) + rng.integers(0, 5)).astype(np.int64), n0 - 1)
    out = {k: (base[k][idx] + 0.3 * rng.standard_normal((nb, d))).astype(np.float32) for k, d in DIMS.items()}
    out["ssms"], out["chromas"] = np.abs(out["ssms"]), np.abs(out["chromas"])
    out["chroma_med"] = np.abs(rng.standard_normal(12)).astype(np.float32)
    return out


def canon_distances(f1, f2):
    """es.distances' [(SSMA, SSMB, CSM)] in the kernels' summation order (oracle.ef_csm): euclid for
    mfccs and ssms, cosine for chromas; self distances with no roll, the CSM with both medians."""
    out = []
    for key in ("mfccs", "ssms"):
        out.append((oracle.ef_csm(f1[key], f1[key], 0), oracle.ef_csm(f2[key], f2[key], 0),
                    oracle.ef_csm(f1[key], f2[key], 0)))
    c1, c2 = f1["chromas"], f2["chromas"]
    out.append((oracle.ef_csm(c1, c1, 1), oracle.ef_csm(c2, c2, 1),
                oracle.ef_csm(c1, c2, 1, f1["chroma_med"], f2["chroma_med"])))
    return out


Maker = namedtuple("Maker", "base cover distances")
EXACT = Maker(_clique_blocks, _exact_cover, es.distances)
FLOAT = Maker(_float_base, _float_cover, canon_distances)


# ---- tracks and references -------------------------------------------------------------------------
def pair_tracks(shapes, seed, maker=EXACT):
    """(feats, pairs): for each (M, N) a base of max(M, N) + 10 blocks and two covers of it, tracks
    2 s and 2 s + 1, and the pair of them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    feats, pairs = [], []
    for M, N in shapes:
        base = maker.base(rng, max(M, N) + 10)
        for nb in (M, N):
            feats.append(maker.cover(rng, base, nb))
        pairs.append((len(feats) - 2, len(feats) - 1))
    return feats, pairs


def bank_tracks(blocks, seed, maker=EXACT):
    """feats: covers of ONE base of max(blocks) + 10 blocks, one track per entry of `blocks`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = maker.base(rng, max(blocks) + 10)
    return [maker.cover(rng, base, nb) for nb in blocks]


def reference(d, kappa, K, niters, mu=0.5, reg_diag=1.0):
    """The reference record of one pair from its distances d = [(SSMA, SSMB, CSM)] * 3."""
    canon = es.early_snf(d, kappa, K, niters, mu, reg_diag, ev=es.CANON)
    other = es.early_snf(d, kappa, K, niters, mu, reg_diag, ev=es.NUMPY)
    r = {"canon": canon, "numpy": other, "bound": None, "stable": False}
    if canon["binary"] is not None:
        r["bound"] = 8 * rel_dev(other["cross"], canon["cross"])
        gap = float("inf")  # kappa = 0: every cell is a one, no boundary
        if kappa != 0:
            nn = es.nneighbs(kappa, canon["cross"].shape[1])
            s = -np.sort(-canon["cross"], 1)
            gap = float(np.min((s[:, nn - 1] - s[:, nn]) / np.abs(s[:, nn - 1])))
        r["stable"] = bool(np.array_equal(canon["binary"], other["binary"]) and gap > r["bound"])
    return r


def references(feats, pairs, kappa, K, niters, mu=0.5, reg_diag=1.0, distances=es.distances, dcache=None):
    """refs[p] for every pair of the list; a pair listed twice shares one record. dcache: a dict that
    keeps the distances per (a, b) across calls (parameter rows over the same tracks)."""
    refs, cache = [], {}
    dcache = {} if dcache is None else dcache
    for a, b in np.asarray(pairs).reshape(-1, 2):
        key = (int(a), int(b))
        if key not in cache:
            if key not in dcache:
                dcache[key] = distances(feats[a], feats[b])
            cache[key] = reference(dcache[key], kappa, K, niters, mu, reg_diag)
        refs.append(cache[key])
    return refs


def shape_of(feats, pair):
    return len(feats[pair[0]]["mfccs"]), len(feats[pair[1]]["mfccs"])


# ---- the bank classes (test_gpu_early_snf_banks.py) ------------------------------------------------
BANK_K, BANK_KAPPA = 10, 0.1
# name: (blocks per track, seed, niters); ld = the longest track rounded up to 4
BANKS = {"tiny": ((12, 16, 20), 21, 5),
         "short": ((14, 22, 23, 31, 47), 22, 5),
         "mid": ((30, 64, 65, 101, 128), 23, 5),
         "long": ((40, 300, 512), 24, 1)}
LONG_PAIRS = [(2, 2), (1, 2), (2, 1), (0, 0)]  # n = 1024, 812, 812, 80
# general float32 features: (blocks per track, seed, pairs)
FLOAT_BANKS = {"short": ((14, 47, 22, 23, 31), 31, [(0, 1), (1, 0), (2, 3), (4, 4), (3, 2), (0, 4), (4, 1)]),
               "mid": ((64, 101, 128, 100, 30), 32, [(0, 1), (2, 3), (4, 2), (1, 0), (4, 0), (3, 1), (0, 0)])}


@functools.lru_cache(maxsize=None)
def bank_case(name):
    """tiny, short, mid: all T^2 ordered pairs (self pairs, both orders, runs of one query, every
    track in 2 T pairs); long: LONG_PAIRS."""
    blocks, seed, niters = BANKS[name]
    feats = bank_tracks(blocks, seed)
    T = len(blocks)
    pairs = LONG_PAIRS if name == "long" else [(i, j) for i in range(T) for j in range(T)]
    pairs = np.array(pairs, np.int32)
    return feats, pairs, references(feats, pairs, BANK_KAPPA, BANK_K, niters)


@functools.lru_cache(maxsize=None)
def float_case(name):
    blocks, seed, pairs = FLOAT_BANKS[name]
    feats = bank_tracks(blocks, seed, FLOAT)
    pairs = np.array(pairs, np.int32)
    return feats, pairs, references(feats, pairs, BANK_KAPPA, BANK_K, 5, distances=canon_distances)


# ---- the parameter rows (test_gpu_early_snf_params.py) ---------------------------------------------
PARAM_SHAPES = [(14, 47), (47, 14), (22, 23), (23, 23), (40, 40), (60, 62), (64, 70)]  # ld = 72
PARAM_SEED = 41
Row = namedtuple("Row", "K niters mu reg_diag kappa")
_BASE = Row(10, 5, 0.5, 1.0, 0.1)
PARAM_ROWS = ([_BASE._replace(K=k) for k in (2, 3, 11, 50, 64)] + [_BASE._replace(niters=i) for i in (1, 2)] +
              [_BASE._replace(mu=m) for m in (0.3, 1.0)] + [_BASE._replace(reg_diag=r) for r in (0.0, 0.25)] +
              [_BASE._replace(kappa=k) for k in (0.3, 3, 0.0)])
# The shapes the reference refuses at each K, worked out by hand from k1 = int(K M / (M + N)),
# k2 = K - k1, 1 <= k1 <= M - 2, 1 <= k2 <= N - 2, K < M + N:
#   K = 2   k1 = int(28 / 61) = int(44 / 45) = int(120 / 122) = int(128 / 134) = 0
#   K = 3   k1 = int(42 / 61) = 0
#   K = 50  50 >= 45 and 50 >= 46; (14, 47): k1 = 11 <= 12, k2 = 39 <= 45; (47, 14): k2 = 12 <= 12
#   K = 64  64 >= 61, 45, 46; (40, 40): k1 = k2 = 32 <= 38
PARAM_REFUSED = {2: [(14, 47), (22, 23), (60, 62), (64, 70)], 3: [(14, 47)],
                 50: [(22, 23), (23, 23)], 64: [(14, 47), (47, 14), (22, 23), (23, 23)]}


def row_id(row):
    return "K%d-it%d-mu%g-reg%g-kappa%g" % row


@functools.lru_cache(maxsize=None)
def param_tracks():
    feats, pairs = pair_tracks(PARAM_SHAPES, PARAM_SEED)
    return feats, np.array(pairs, np.int32), {}


@functools.lru_cache(maxsize=None)
def param_case(row):
    feats, pairs, dcache = param_tracks()
    return feats, pairs, references(feats, pairs, row.kappa, row.K, row.niters, row.mu, row.reg_diag, dcache=dcache)


@functools.lru_cache(maxsize=None)
def k_above_blocks_case(K):
    """Two 40-block tracks, max_blocks = 40: K = 50 and 64 exceed it, and the pair fuses."""
    feats, pairs = pair_tracks([(40, 40)], 43)
    pairs = np.array(pairs, np.int32)
    return feats, pairs, references(feats, pairs, BANK_KAPPA, K, 5)


@functools.lru_cache(maxsize=None)
def duplicate_block_case():
    """Track 0: one block twelve times (its self distances are all zero: MeanDist = 0 and Denom = 0 -> 1
    in getW); track 1 an ordinary 20-block track; the two pairs of them. Track 0 is not paired with
    itself: that CSM is all zeros, getWCSM gives 0 / 0, and NaN affinities have no defined order."""
    rng = np.random.Generator(np.random.PCG64(44))
    one = _clique_blocks(rng, 1)
    dup = {k: np.repeat(one[k], 12, 0) for k in one}
    dup["chroma_med"] = rng.permutation(12).astype(np.float32)
    other = _exact_cover(rng, _clique_blocks(rng, 30), 20)
    feats = [dup, other]
    pairs = np.array([(0, 1), (1, 0)], np.int32)
    return feats, pairs, references(feats, pairs, BANK_KAPPA, BANK_K, 5)


# ---- the conditions on the inputs alone (host) -----------------------------------------------------
def check_inputs(feats, pairs, refs, K, refused=(), share=0.7, label=""):
    """canon's cross finite on every fusable pair, pair_ok as expected, at least `share` of the
    fusable pairs stable, some stable score above 0."""
    fusable = []
    for p, pr in enumerate(pairs):
        M, N = shape_of(feats, pr)
        ok = es.pair_ok(M, N, K)
        assert ok == ((M, N) not in refused), (label, p, M, N, K)
        assert (refs[p]["bound"] is not None) == ok, (label, p)
        if ok:
            fusable.append(p)
            assert refs[p]["canon"]["cross"].shape == (M, N) and np.isfinite(refs[p]["canon"]["cross"]).all(), (label, p)
            assert np.isfinite(refs[p]["numpy"]["cross"]).all() and np.isfinite(refs[p]["bound"]), (label, p)
    stable = [p for p in fusable if refs[p]["stable"]]
    assert fusable and len(stable) >= share * len(fusable), (label, len(stable), len(fusable))
    assert any(refs[p]["canon"]["score"] > 0 for p in stable), label


# ---- the GPU side ----------------------------------------------------------------------------------
def make_bank(feats):
    import torch
    nb = np.array([len(f["mfccs"]) for f in feats], np.int32)
    off = np.zeros(len(feats), np.int64)
    off[1:] = np.cumsum(nb[:-1])
    host = {k: np.concatenate([f[k] for f in feats]).astype(np.float32) for k in ("mfccs", "ssms", "chromas")}
    host["chroma_med"] = np.stack([f["chroma_med"] for f in feats]).astype(np.float32)
    host["nb"], host["off"] = nb, off
    bank = {k: torch.as_tensor(host[k]).cuda() for k in host}
    bank["nb_host"], bank["max_blocks"] = nb, int(nb.max())
    return bank, host


def run_snf(bank, pairs, kappa, K, niters, mu=0.5, reg_diag=1.0, want_cross=True):
    """(score (P,), [cross of pair p, flat]) on the host; the list is None without want_cross."""
    from acoss import _lib
    r = _lib.earlyfusion_snf(bank, pairs, kappa, K, niters, reg_diag=reg_diag, want_cross=want_cross, mu=mu)
    score = r["score"].cpu().numpy()
    if not want_cross:
        assert r["cross"] is None and r["cross_off"] is None
        return score, None
    off = r["cross_off"].cpu().numpy()
    cross = r["cross"].cpu().numpy()
    return score, [cross[off[p]:off[p + 1]] for p in range(len(pairs))]


def same_bits(x, y):
    """Two run_snf results hold the same bits (NaN equal to NaN)."""
    return np.array_equal(x[0], y[0], equal_nan=True) and len(x[1]) == len(y[1]) and all(
        np.array_equal(a, b, equal_nan=True) for a, b in zip(x[1], y[1]))


def check_against_restatement(feats, pairs, refs, got, kappa, share=0.7, label=""):
    """The three comparisons of a GPU run `got` = run_snf(...) with the reference records, and NaN
    exactly on the refused pairs:
      1. every fusable pair's cross within that pair's bound of canon's (printed per pair);
      2. every fusable pair's score == Smith-Waterman of the top-nn binarisation of its OWN cross;
      3. score == canon's on every stable pair, the stable ones at least `share` of the fusable.
    Returns the largest deviation / bound ratio seen."""
    score, cross = got
    fusable = [p for p, r in enumerate(refs) if r["bound"] is not None]
    worst = 0.0
    for p, pr in enumerate(pairs):
        M, N = shape_of(feats, pr)
        assert cross[p].size == M * N, (label, p)
        if refs[p]["bound"] is None:
            assert np.isnan(score[p]) and np.isnan(cross[p]).all(), (label, p)
            continue
        assert np.isfinite(score[p]) and np.isfinite(cross[p]).all(), (label, p)
        want = refs[p]["canon"]["cross"]
        own = cross[p].reshape(M, N)
        dev = rel_dev(own, want)
        print("%s pair %d %s: bound %.3e, deviation %.3e%s" % (label, p, (M, N), refs[p]["bound"], dev,
                                                              "" if refs[p]["stable"] else " (not stable)"))
        assert dev <= refs[p]["bound"], (label, p, (M, N), dev, refs[p]["bound"])
        worst = max(worst, dev / refs[p]["bound"]) if refs[p]["bound"] > 0 else worst
        assert score[p] == oracle.sw_constrained(es.binarize_top(own, kappa)), (label, p, (M, N))
    stable = [p for p in fusable if refs[p]["stable"]]
    assert len(stable) >= share * len(fusable), (label, len(stable), len(fusable))
    for p in stable:
        assert score[p] == refs[p]["canon"]["score"], (label, p, shape_of(feats, pairs[p]))
    return worst
