"""acoss_earlyfusion_snf (the per-pair similarity network fusion of EarlyFusion) on the GPU against
the numpy restatement tests/early_snf_np.py.

The block features are built the way test_gpu_earlyfusion_pin.py builds them (integer-exact MFCC /
SSM blocks, 0/1 chroma blocks with 16 ones), so every float32 distance matrix is exact in any
summation order and both sides start from the same bits. The whole pair list goes in one call,
again in a permuted order and again with a tiny ACOSS_EF_BYTES (one pair per chunk): all three runs
must return identical bits.

Shapes (M, N): (12, 12), (14, 47), (47, 14); n = 64 and 65; the LDS regime's largest n = 101 and
102 (the first pair of the workspace regime); one long pair (200, 180); (4, 60), which breaks the
k1 condition at K = 10 and must come back NaN; a duplicated pair.

Bound of check 1, measured by the test itself per pair: 8 x the largest relative deviation between
the restatement's two admissible evaluations (numpy's float32 exp and pairwise row sums, against
canon_expf and sequential row sums). Measured on these pairs (CPU): deviations of 1.7e-8 .. 8.4e-8,
so bounds of 1.4e-7 .. 6.7e-7; the kernels mirror the canonical evaluation operation for operation.
"""
import os

import numpy as np
import pytest

import early_snf_np as es
import oracle
from early_snf_cases import make_bank, pair_tracks, references, rel_dev
from test_gpu_earlyfusion_pin import _clique_blocks, _cover

pytestmark = pytest.mark.gpu

KAPPA, K, NITERS = 0.1, 10, 5
# (M, N) of each pair; a clique base of max(M, N) + 10 blocks and two covers of it
SHAPES = [(12, 12), (14, 47), (47, 14), (32, 32), (32, 33), (50, 51), (51, 51), (200, 180), (4, 60)]
SEED = 7


def top_binary(cross, kappa):
    return es.binarize_top(cross, kappa)


def build_case():
    """(feats, pairs, refs): refs[p] = {"canon", "numpy": early_snf results, "bound", "stable"}
    (early_snf_cases.py)."""
    feats, pairs = pair_tracks(SHAPES, SEED)
    pairs.append(pairs[1])  # a duplicated pair
    pairs = np.array(pairs, np.int32)
    return feats, pairs, references(feats, pairs, KAPPA, K, NITERS)


@pytest.fixture(scope="module")
def case():
    return build_case()


@pytest.fixture(scope="module")
def runs(case):
    """The three runs: the whole list, a permutation of it, one pair per chunk."""
    from acoss import _lib
    feats, pairs, _ = case
    bank, host = make_bank(feats)

    def run(pp):
        r = _lib.earlyfusion_snf(bank, pp, KAPPA, K, NITERS, want_cross=True)
        off = r["cross_off"].cpu().numpy()
        cross = r["cross"].cpu().numpy()
        return r["score"].cpu().numpy(), [cross[off[p]:off[p + 1]] for p in range(len(pp))]

    whole = run(pairs)
    perm = np.random.default_rng(3).permutation(len(pairs))
    sp, cp = run(pairs[perm])
    inv = np.argsort(perm)
    permuted = (sp[inv], [cp[i] for i in inv])
    old = os.environ.get("ACOSS_EF_BYTES")
    os.environ["ACOSS_EF_BYTES"] = "1"
    try:
        chunked = run(pairs)
    finally:
        if old is None:
            del os.environ["ACOSS_EF_BYTES"]
        else:
            os.environ["ACOSS_EF_BYTES"] = old
    return bank, host, whole, permuted, chunked


def test_restatement_alone_is_stable(case):
    """At least 70 % of the pairs are stable under the restatement's own two evaluations."""
    _, pairs, refs = case
    assert sum(r["stable"] for r in refs) >= 0.7 * len(pairs)


def test_same_bits_in_any_order_and_chunking(runs):
    _, _, whole, permuted, chunked = runs
    for other in (permuted, chunked):
        assert np.array_equal(whole[0], other[0], equal_nan=True)
        for a, b in zip(whole[1], other[1]):
            assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(whole[0][1], whole[0][-1]) and np.array_equal(whole[1][1], whole[1][-1])  # the duplicate


def test_cross_within_measured_bound(case, runs):
    _, pairs, refs = case
    score, cross = runs[2]
    for p, r in enumerate(refs):
        if r["bound"] is None:
            continue
        want = r["canon"]["cross"]
        got = cross[p].reshape(want.shape)
        dev = rel_dev(got, want)
        print("pair %d %s: bound %.3e, deviation %.3e" % (p, want.shape, r["bound"], dev))
        assert dev <= r["bound"], (p, dev, r["bound"])


def test_score_is_sw_of_own_cross(case, runs):
    """The tail, exact: the score is the constrained Smith-Waterman of the stable top-nn
    binarisation of the GPU's own cross output, on every pair."""
    feats, pairs, refs = case
    score, cross = runs[2]
    for p, (a, b) in enumerate(pairs):
        if refs[p]["bound"] is None:
            continue
        M, N = len(feats[a]["mfccs"]), len(feats[b]["mfccs"])
        assert score[p] == oracle.sw_constrained(top_binary(cross[p].reshape(M, N), KAPPA)), p


def test_score_equals_restatement_on_stable_pairs(case, runs):
    _, pairs, refs = case
    score = runs[2][0]
    stable = [p for p, r in enumerate(refs) if r["stable"]]
    assert len(stable) >= 0.7 * len(pairs)
    for p in stable:
        assert score[p] == refs[p]["canon"]["score"], p
    assert any(refs[p]["canon"]["score"] > 0 for p in stable)


def test_refused_pair_is_nan(case, runs):
    _, pairs, refs = case
    score, cross = runs[2]
    bad = [p for p, r in enumerate(refs) if r["bound"] is None]
    assert bad == [SHAPES.index((4, 60))]
    for p in range(len(pairs)):
        if p in bad:
            assert np.isnan(score[p]) and np.isnan(cross[p]).all() and cross[p].size == 4 * 60
        else:
            assert np.isfinite(score[p]) and np.isfinite(cross[p]).all()


def test_both_regimes_same_bits(case, runs, monkeypatch):
    """Every pair through the workspace kernels (no LDS regime) returns the bits of the mixed run."""
    from acoss import _lib
    _, pairs, _ = case
    bank, _, whole = runs[0], runs[1], runs[2]
    monkeypatch.setenv("ACOSS_EFS_LDS_N", "0")
    r = _lib.earlyfusion_snf(bank, pairs, KAPPA, K, NITERS, want_cross=True)
    assert np.array_equal(r["score"].cpu().numpy(), whole[0], equal_nan=True)
    assert np.array_equal(r["cross"].cpu().numpy(), np.concatenate(whole[1]), equal_nan=True)


def test_niters_zero_and_bad_offsets(case, runs):
    """niters = 0 is the mean of the three P; a cross_off that leaves a pair too little room is
    refused naming the pair, before anything is written."""
    import ctypes
    import torch
    from acoss import _lib
    feats, pairs, _ = case
    bank = runs[0]
    p = 0
    a, b = pairs[p]
    d = es.distances(feats[a], feats[b])
    want = es.early_snf(d, KAPPA, K, 0)
    r = _lib.earlyfusion_snf(bank, pairs[p:p + 1], KAPPA, K, 0, want_cross=True)
    got = r["cross"].cpu().numpy().reshape(want["cross"].shape)
    assert rel_dev(got, want["cross"]) <= 8 * rel_dev(es.early_snf(d, KAPPA, K, 0, ev=es.NUMPY)["cross"], want["cross"])
    assert float(r["score"][0]) == oracle.sw_constrained(top_binary(got, KAPPA))
    lib = _lib.load_library()
    off = _lib.ef_snf_cross_offsets(bank["nb_host"], pairs[:3])
    total = int(off[-1])
    off[2] -= 1  # pair 1 is one element short
    off_d = torch.as_tensor(off).cuda()
    out = torch.full((total,), 7.0, dtype=torch.float64, device="cuda")
    sc = torch.empty(3, dtype=torch.float64, device="cuda")
    pd = torch.as_tensor(pairs[:3]).cuda()
    rc = lib.acoss_earlyfusion_snf(_lib._ptr(bank["mfccs"]), _lib._ptr(bank["ssms"]), _lib._ptr(bank["chromas"]),
                                   _lib._ptr(bank["chroma_med"]), _lib._ptr(bank["off"]), _lib._ptr(bank["nb"]),
                                   len(feats), int(bank["max_blocks"]), 1000, 1225, 480, _lib._ptr(pd), 3, KAPPA, K, 0.5,
                                   NITERS, 1.0, _lib._ptr(sc), _lib._ptr(off_d), total, _lib._ptr(out),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"pair 1" in lib.acoss_last_error()
    assert bool((out == 7.0).all())


def test_existing_scores_keep_their_bits(case, runs):
    """acoss_earlyfusion on the same pairs (the refused one left out: it raises there) still
    returns the canonical oracle's four scores, before and after the new call."""
    from acoss import _lib
    _, pairs, refs = case
    bank, host = runs[0], runs[1]
    ok = np.array([p for p, r in enumerate(refs) if r["bound"] is not None])
    want = oracle.ef_batch(host, pairs[ok], KAPPA, K=K)
    got = _lib.earlyfusion(bank, pairs[ok], KAPPA, K).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    _lib.earlyfusion_snf(bank, pairs, KAPPA, K, NITERS)
    np.testing.assert_array_equal(_lib.earlyfusion(bank, pairs[ok], KAPPA, K).cpu().numpy(), want)


def test_plugin_early_snf(tmp_path, monkeypatch):
    """EarlyFusion(early_snf=True): Ds["early_snf"] is the binding's score, the four other matrices
    are those of early_snf=False, and pair_fusion returns the pair's cross block."""
    from acoss import _lib, synthetic
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    from acoss.features_io import save_features
    rng = np.random.Generator(np.random.PCG64(5))
    feats = []
    for c in range(3):
        base = _clique_blocks(rng, int(rng.integers(30, 45)))
        for v in range(2):
            bf = dict(base) if v == 0 else _cover(rng, base, int(rng.integers(25, 45)))
            bf["chroma_med"] = rng.permutation(12).astype(np.float32)
            feats.append(bf)
    n = len(feats)
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), [np.zeros((8, 12), np.float32)] * n,
                                                np.arange(n) // 2)
    monkeypatch.chdir(tmp_path)
    Ds = {}
    for flag in (False, True):
        ef = EarlyFusion(csv, fdir, shortname="snf%d" % flag, cachedir=str(tmp_path / "cache"), early_snf=flag)
        for i, bf in enumerate(feats):
            save_features("%s_%i.h5" % (ef.get_cacheprefix(), i), bf)
        ef.all_pairwise(symmetric=True)
        Ds[flag] = {k: np.array(ef.Ds[k]) for k in ef.Ds}
        assert list(ef.Ds) == ["mfccs", "ssms", "chromas", "early"] + (["early_snf"] if flag else [])
    for k in ("mfccs", "ssms", "chromas", "early"):
        np.testing.assert_array_equal(Ds[True][k], Ds[False][k], err_msg=k)
    up = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
    bank, _ = make_bank(feats)
    want = _lib.earlyfusion_snf(bank, up, ef.kappa, ef.K, ef.niters, want_cross=True)
    np.testing.assert_array_equal(Ds[True]["early_snf"][up[:, 0], up[:, 1]],
                                  want["score"].cpu().numpy().astype(np.float32))
    assert np.count_nonzero(Ds[True]["early_snf"]) > 0
    cross, binary = ef.pair_fusion(0, 1)
    off = want["cross_off"].cpu().numpy()
    np.testing.assert_array_equal(cross.ravel(), want["cross"].cpu().numpy()[off[0]:off[1]])
    assert binary.shape == cross.shape and (binary.sum(1) == es.nneighbs(ef.kappa, cross.shape[1])).all()
    assert oracle.sw_constrained(binary) == float(want["score"][0])
