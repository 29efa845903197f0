"""The numpy restatement of the per-pair similarity network fusion (tests/early_snf_np.py) against
the reference's own run (tests/golden/early_snf_golden.npz, made by make_golden_early_snf.py), the
pair conditions, the binding's argument checks, and the inputs of the GPU tests' cases
(early_snf_cases.py: finite restatement, the refused pairs, the stable share). No GPU.

The golden inputs are float64, so the reference and the restatement differ only in numpy's
summation order (np.partition's order inside np.mean, pairwise np.sum): affinities and fused
matrices agree within 1e-10 relative; binary matrices and scores are equal.
"""
import os

import numpy as np
import pytest

import early_snf_np as es

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "early_snf_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _dists(g, s):
    return [(g["s%d_f%d_ssma" % (s, f)], g["s%d_f%d_ssmb" % (s, f)], g["s%d_f%d_csm" % (s, f)]) for f in range(3)]


@pytest.mark.parametrize("ev", [es.CANON, es.NUMPY], ids=["sequential", "pairwise"])
def test_restatement_reproduces_the_reference(golden, ev):
    g = golden
    kappa = float(g["kappa"])
    assert [tuple(s) for s in g["shapes"]] == [(12, 12), (9, 20), (20, 9)]
    assert list(g["Ks"]) == [4, 10] and list(g["niters"]) == [0, 1, 5]
    for s, (M, N) in enumerate(g["shapes"]):
        d = _dists(g, s)
        assert d[0][2].dtype == np.float64 and d[0][2].shape == (M, N)
        for K in g["Ks"]:
            W = np.stack([es.getWCSMSSM(A, B, C, int(K), ev=ev) for A, B, C in d])
            np.testing.assert_allclose(W, g["s%d_K%d_W" % (s, K)], rtol=1e-10, atol=0)
            for it in g["niters"]:
                key = "s%d_K%d_it%d_" % (s, K, it)
                r = es.early_snf(d, kappa, int(K), int(it), ev=ev)
                np.testing.assert_allclose(r["F"], g[key + "F"], rtol=1e-10, atol=0)
                np.testing.assert_allclose(r["cross"], g[key + "cross"], rtol=1e-10, atol=0)
                np.testing.assert_array_equal(r["binary"], g[key + "binary"])
                assert r["score"] == float(g[key + "score"])
    assert any(float(g[k]) > 0 for k in g.files if k.endswith("score"))


def test_float32_inputs_follow_numpys_dtype_rule(golden):
    """float32 distances give float32 affinities, held exactly in the float64 parent."""
    d = [tuple(x.astype(np.float32) for x in t) for t in _dists(golden, 1)]
    for ev in (es.CANON, es.NUMPY):
        W = es.getWCSMSSM(*d[0], 10, ev=ev)
        assert W.dtype == np.float64 and np.array_equal(W, W.astype(np.float32))
        assert np.array_equal(W[:9, 9:], W[9:, :9].T)
    a = es.early_snf(d, 0.25, 10, 5, ev=es.CANON)["cross"]
    b = es.early_snf(d, 0.25, 10, 5, ev=es.NUMPY)["cross"]
    assert 0 < np.max(np.abs(a - b) / np.abs(b)) < 1e-5  # the two admissible evaluations: float32 exp


def test_pair_conditions_map_to_nan():
    from acoss import _lib
    for M, N, K, ok in [(12, 12, 10, True), (4, 60, 10, False), (60, 4, 10, True), (60, 2, 10, False),
                        (14, 47, 10, True), (3, 3, 4, False), (4, 4, 4, True), (5, 5, 10, False),
                        (12, 12, 1, False), (4, 40, 10, False), (5, 40, 10, True)]:
        assert es.pair_ok(M, N, K) == ok, (M, N, K)
        assert bool(_lib.ef_snf_pair_ok(M, N, K)) == ok, (M, N, K)
    # k1 = 0 at (4, 60): getW would divide by zero
    assert es.split(4, 60, 10) == (0, 10)
    rng = np.random.default_rng(0)
    d = [(rng.random((4, 4)), rng.random((60, 60)), rng.random((4, 60))) for _ in range(3)]
    r = es.early_snf(d, 0.1, 10, 5)
    assert np.isnan(r["score"]) and r["cross"].shape == (4, 60) and np.isnan(r["cross"]).all()
    M = np.arange(1, 80)
    ok = _lib.ef_snf_pair_ok(M[:, None], M[None, :], 10)
    assert all(bool(ok[m - 1, n - 1]) == es.pair_ok(m, n, 10) for m in M for n in M)


def test_binding_rejects_bad_arguments_without_a_gpu():
    from acoss import _lib
    bank = {"max_blocks": 40}  # nothing on a device: the checks come first
    pairs = np.array([[0, 1]], np.int32)
    for kw in ({"niters": -1}, {"niters": 2.5}, {"reg_diag": -0.5}, {"reg_diag": float("nan")}, {"K": 0}, {"K": 65},
               {"kappa": -0.1}):
        args = {"kappa": 0.1, "K": 10, "niters": 5, "reg_diag": 1.0}
        args.update(kw)
        with pytest.raises(ValueError):
            _lib.earlyfusion_snf(bank, pairs, args["kappa"], args["K"], args["niters"], reg_diag=args["reg_diag"])
    with pytest.raises(ValueError, match="512"):
        _lib.earlyfusion_snf({"max_blocks": 513}, pairs, 0.1, 10, 5)
    nb = np.array([5, 7, 3])
    np.testing.assert_array_equal(_lib.ef_snf_cross_offsets(nb, [[0, 1], [2, 2], [1, 0]]), [0, 35, 44, 79])
    with pytest.raises(ValueError):
        _lib.ef_snf_cross_offsets(nb, [[0, 3]])
    assert "acoss_earlyfusion_snf" in _lib.SIGNATURES and len(_lib.SIGNATURES["acoss_earlyfusion_snf"]) == 23


def test_k_is_weighed_per_pair_not_against_max_blocks():
    """K = 50 on a 47-block bank and K = 64 on two 40-block tracks fuse in the reference's terms; the
    host check holds K to [1, 64] whatever max_blocks is."""
    from acoss import _lib
    assert es.pair_ok(47, 47, 50) and es.pair_ok(40, 40, 64) and es.split(40, 40, 64) == (32, 32)
    assert bool(_lib.ef_snf_pair_ok(47, 47, 50)) and bool(_lib.ef_snf_pair_ok(40, 40, 64))
    for K, mb in ((50, 47), (64, 40), (64, 1)):
        _lib.ef_snf_check_args(0.1, K, 5, 1.0, mb)
    with pytest.raises(ValueError):
        _lib.ef_snf_check_args(0.1, 65, 5, 1.0, 512)


# ---- the inputs of test_gpu_early_snf_banks.py and test_gpu_early_snf_params.py, checked without a
# GPU: what those tests conclude rests on these conditions of the restatement alone
@pytest.mark.parametrize("name", ["tiny", "short", "mid", "long"])
def test_bank_cases_rest_on_sound_inputs(name):
    import early_snf_cases as ec
    feats, pairs, refs = ec.bank_case(name)
    blocks = ec.BANKS[name][0]
    assert [len(f["mfccs"]) for f in feats] == list(blocks)
    if name == "long":
        assert [sum(ec.shape_of(feats, p)) for p in pairs] == [1024, 812, 812, 80]
    else:
        assert len(pairs) == len(blocks) ** 2 and len({tuple(p) for p in pairs}) == len(pairs)
    ec.check_inputs(feats, pairs, refs, ec.BANK_K, label=name)  # K = 10 refuses none of these shapes


@pytest.mark.parametrize("name", ["short", "mid"])
def test_float_bank_cases_rest_on_sound_inputs(name):
    import early_snf_cases as ec
    feats, pairs, refs = ec.float_case(name)
    shapes = [ec.shape_of(feats, p) for p in pairs]
    want = {"short": [(14, 47), (47, 14), (22, 23), (31, 31)], "mid": [(64, 101), (128, 100), (30, 128)]}[name]
    assert 6 <= len(pairs) <= 9 and all(s in shapes for s in want)
    for f in feats:  # general float32 values, not the integer-exact ones
        assert f["mfccs"].dtype == np.float32 and not np.array_equal(f["mfccs"], np.rint(f["mfccs"]))
        assert (f["ssms"] >= 0).all() and (f["chromas"] >= 0).all() and (f["chroma_med"] >= 0).all()
    ec.check_inputs(feats, pairs, refs, ec.BANK_K, label="float-" + name)


def test_parameter_rows_rest_on_sound_inputs():
    import early_snf_cases as ec
    assert len(ec.PARAM_ROWS) == 14 and len(set(ec.PARAM_ROWS)) == 14
    assert sorted({r.K for r in ec.PARAM_ROWS}) == [2, 3, 10, 11, 50, 64]
    for row in ec.PARAM_ROWS:
        feats, pairs, refs = ec.param_case(row)
        assert [ec.shape_of(feats, p) for p in pairs] == ec.PARAM_SHAPES
        ec.check_inputs(feats, pairs, refs, row.K, refused=ec.PARAM_REFUSED.get(row.K, ()), label=ec.row_id(row))
    for K in (50, 64):
        feats, pairs, refs = ec.k_above_blocks_case(K)
        ec.check_inputs(feats, pairs, refs, K, label="K above max_blocks")


def test_duplicate_block_case_stays_finite_in_the_restatement():
    import early_snf_cases as ec
    feats, pairs, refs = ec.duplicate_block_case()
    d = es.distances(feats[0], feats[1])
    assert all(not t[0].any() for t in d)  # the twelve identical blocks: all self distances zero
    for r in refs:
        assert r["bound"] is not None and np.isfinite(r["bound"])
        assert np.isfinite(r["canon"]["cross"]).all() and np.isfinite(r["numpy"]["cross"]).all()
        assert all(np.isfinite(W).all() for W in r["canon"]["W"])


def test_plugin_option_is_off_by_default():
    import inspect
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    sig = inspect.signature(EarlyFusion.__init__)
    assert sig.parameters["early_snf"].default is False
    assert list(sig.parameters)[-1] == "early_snf"  # the reference's positional arguments keep their places
    assert hasattr(EarlyFusion, "pair_fusion")
