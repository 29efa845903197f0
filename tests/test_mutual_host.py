"""The mutual nearest-neighbour binarisation without a GPU: the numpy restatement (mutual_np.py)
against the CPU oracle's row rule on both axes, the properties the definition promises, a condition
on the test inputs (so that a `mutual` flag that is ignored cannot pass the GPU tests), and the
Python layer's argument handling."""
import numpy as np
import pytest

import early_snf_cases as ec
import early_snf_np as es
import mutual_np as mn
import oracle


def _oracle_mutual(D, kappa):
    return oracle.ef_binarize(D, kappa) & oracle.ef_binarize(np.ascontiguousarray(D.T), kappa).T


def _in_range(kappa, M, N):
    """oracle.ef_binarize restates csm_to_binary, which needs a count below the line length."""
    return kappa != 0 and es.nneighbs(kappa, N) < N and es.nneighbs(kappa, M) < M


@pytest.mark.parametrize("M,N", mn.SHAPES_HOST)
def test_restatement_equals_the_oracle_on_both_axes(M, N):
    seen = 0
    for D in mn.tie_matrices(M, N, 3):
        for kappa in (0.1, 0.3, 0.45, 1, 2, 5):
            if not _in_range(kappa, M, N):
                continue
            want = _oracle_mutual(D, kappa)
            assert np.array_equal(mn.mutual_smallest(D, kappa), want), (M, N, kappa)
            assert np.array_equal(mn.rows_smallest(D, kappa), oracle.ef_binarize(D, kappa)), (M, N, kappa)
            assert np.array_equal(mn.cols_smallest(D, kappa),
                                  oracle.ef_binarize(np.ascontiguousarray(D.T), kappa).T), (M, N, kappa)
            # the largest form is the smallest form of the negated matrix, ties the same way
            assert np.array_equal(mn.mutual_largest(-D.astype(np.float64), kappa), want), (M, N, kappa)
            seen += 1
    assert seen or min(M, N) == 1


@pytest.mark.parametrize("M,N", mn.SHAPES_HOST)
def test_properties_of_the_definition(M, N):
    for D in mn.tie_matrices(M, N, 4):
        for kappa in mn.KAPPAS:
            B, R = mn.mutual_smallest(D, kappa), mn.rows_smallest(D, kappa)
            assert B.dtype == np.uint8 and B.shape == (M, N)
            assert not (B & ~R).any()  # B is a subset of R
            assert np.array_equal(mn.mutual_smallest(np.ascontiguousarray(D.T), kappa), B.T)  # transpose closure
            if kappa == 0:
                assert B.all()
                continue
            assert B.sum(1).max() <= mn.count(kappa, N) and B.sum(0).max() <= mn.count(kappa, M)
            assert (R.sum(1) == mn.count(kappa, N)).all()
        prev = np.zeros((M, N), np.uint8)
        for k in range(1, max(M, N) + 2):  # count-valued kappa: nested masks, all ones once both clamp
            B = mn.mutual_smallest(D, k)
            assert not (prev & ~B).any(), (M, N, k)
            prev = B
        assert prev.all()


def test_counts_round_half_to_even_and_the_short_query_is_empty():
    assert [mn.count(0.1, n) for n in (5, 15, 25)] == [0, 2, 2]
    assert mn.count(1000, 7) == 7 and mn.count(5, 30) == 5 and mn.count(0.3, 64) == 19
    D = mn.tie_matrices(4, 30, 5)[0]
    assert mn.count(0.1, 30) == 3 and mn.count(0.1, 4) == 0
    assert mn.rows_smallest(D, 0.1).sum() == 12 and not mn.mutual_smallest(D, 0.1).any()
    assert oracle.sw_constrained(mn.mutual_smallest(D, 0.1)) == 0.0


# the issue's own CPU trial: (masks that differ, scores that differ) of (pair, matrix) cases
RECORDED = {"tiny": (24, 7, 27), "short": (72, 34, 75), "mid": (75, 50, 75)}


@pytest.mark.parametrize("name", ["tiny", "short", "mid"])
def test_the_banks_tell_the_two_rules_apart(name):
    """On the integer-exact banks at kappa = 0.1, all T^2 ordered pairs, the three CSMs: the mutual
    mask differs from the row mask in at least half of the (pair, matrix) cases and the
    Smith-Waterman score in at least a fifth."""
    blocks, seed, _ = ec.BANKS[name]
    feats = ec.bank_tracks(blocks, seed)
    T = len(blocks)
    masks = scores = total = 0
    for i in range(T):
        for j in range(T):
            for _, _, C in es.distances(feats[i], feats[j]):
                R, B = mn.rows_smallest(C, ec.BANK_KAPPA), mn.mutual_smallest(C, ec.BANK_KAPPA)
                masks += not np.array_equal(R, B)
                scores += oracle.sw_constrained(R) != oracle.sw_constrained(B)
                total += 1
    print("%s: %d masks and %d scores of %d differ" % (name, masks, scores, total))
    assert total == 3 * T * T
    assert 2 * masks >= total and 5 * scores >= total
    assert (masks, scores, total) == RECORDED[name]


# ---- the Python layer ------------------------------------------------------------------------------
def test_check_ef_binarize():
    from acoss import _lib
    assert _lib.check_ef_binarize(False) == 0 and _lib.check_ef_binarize(True) == 1
    assert _lib.EF_BINARIZE == {"rows": 0, "mutual": 1}
    assert _lib.ef_mutual_suffix() == "" and _lib.ef_mutual_suffix(True) == "-mutual"
    for bad in (1, 0, "mutual", None, 2.0):
        with pytest.raises(ValueError, match="mutual must be True or False"):
            _lib.check_ef_binarize(bad)


def test_the_query_side_refusal():
    from acoss import _lib
    # a 4-block query at kappa = 5: the rows (30 columns) are fine, the columns (4 rows) are not
    assert _lib.ef_neighbour_error([4], [30], 5, 2) is None
    err = _lib.ef_neighbour_error([4], [30], 5, 2, mutual=True)
    assert isinstance(err, ValueError) and str(err) == "kth(=5) out of bounds (4)"
    assert str(_lib.ef_neighbour_error([30], [4], 5, 2, mutual=True)) == "kth(=5) out of bounds (4)"  # the row side first
    assert _lib.ef_neighbour_error([40], [30], 0.1, 10, mutual=True) is None
    assert _lib.ef_neighbour_error([4], [30], 0, 2, mutual=True) is None  # kappa == 0: all ones
    assert str(_lib.ef_neighbour_error([4], [30], 0.1, 10, mutual=True)) == "kth(=10) out of bounds (4)"
    bank = {"nb_host": np.array([4, 30], np.int32)}
    _lib._check_ef_neighbours(bank, np.array([[0, 1]], np.int32), 5, 2)
    with pytest.raises(ValueError, match=r"kth\(=5\) out of bounds \(4\)"):
        _lib._check_ef_neighbours(bank, np.array([[0, 1]], np.int32), 5, 2, mutual=True)


def test_names_and_command_line():
    from acoss import coverid
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    from acoss.algorithms.utils import cross_recurrence
    assert EarlyFusion.algorithm_name() == "EarlyFusionTraile"
    assert EarlyFusion.algorithm_name(mutual=True) == "EarlyFusionTraile-mutual"
    assert coverid.parser_args(["--mutual"]).mutual is True and coverid.parser_args([]).mutual is False
    assert coverid.algorithm_names == ["Serra09", "EarlyFusionTraile", "LateFusionChen", "FTM2D", "SiMPle"]
    for algorithm in ("Serra09", "LateFusionChen", "FTM2D", "SiMPle"):
        with pytest.raises(ValueError, match="mutual is supported by EarlyFusionTraile only"):
            coverid.benchmark("none.csv", "none", algorithm=algorithm, mutual=True)
    assert "csm_to_binary_mutual" in cross_recurrence.__all__
    assert cross_recurrence.csm_to_binary_mutual(np.zeros((3, 5), np.float32), 0).tolist() == np.ones((3, 5)).tolist()
    with pytest.raises(ValueError, match=r"kth\(=5\) out of bounds \(4\)"):
        cross_recurrence.csm_to_binary_mutual(np.zeros((4, 30), np.float32), 5)
    with pytest.raises(ValueError, match=r"kth\(=5\) out of bounds \(4\)"):
        cross_recurrence.csm_to_binary_mutual(np.zeros((30, 4), np.float32), 5)


def test_signatures_hold_the_new_entries():
    from acoss import _lib
    S = _lib.SIGNATURES
    for name in ("acoss_earlyfusion", "acoss_earlyfusion_locate", "acoss_earlyfusion_path"):
        assert S[name + "2"] == S[name][:16] + [_lib._i32] + S[name][16:]  # binarize directly after mu
        assert S[name][15] is _lib._f32
    snf, snf2 = S["acoss_earlyfusion_snf"], S["acoss_earlyfusion_snf2"]
    assert snf2 == snf[:16] + [_lib._i32] + snf[16:-1] + [_lib._vp, _lib._vp]  # binary_out before the stream
    assert len(S["acoss_binarize_mutual"]) == 11
    import inspect
    for fn in (_lib.earlyfusion, _lib.earlyfusion_locate, _lib.earlyfusion_path, _lib.earlyfusion_snf):
        assert inspect.signature(fn).parameters["mutual"].default is False
    assert inspect.signature(_lib.binarize_mutual).parameters["mutual"].default is True
    assert inspect.signature(_lib.earlyfusion_snf).parameters["want_binary"].default is False
