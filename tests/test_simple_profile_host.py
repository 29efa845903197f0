"""CPU tests of the SiMPle matrix-profile layer: the numpy restatement the GPU tests compare
against (tests/simple_profile_np.py) pinned to the committed C oracle, its tie rule, and the
host-only helpers of the Python layer (profile offsets, subsequence -> frame ranges)."""
import numpy as np
import pytest

import oracle
from simple_profile_np import simple_profile_np, unit_columns


@pytest.mark.parametrize("na,nb,L", [(37, 45, 10), (45, 37, 10), (10, 23, 10), (64, 70, 10), (30, 41, 7)])
def test_restatement_median_is_the_oracle(na, nb, L):
    """median(mp) of the restatement == or_simple_sim bit for bit, under the oracle's own OTI roll."""
    rng = np.random.default_rng(100 * na + nb)
    A, B = unit_columns(rng, na), unit_columns(rng, nb)
    k = oracle.simple_oti(A, B)
    mp, mpi = simple_profile_np(A, B, L, k)
    assert len(mp) == na - L + 1 and mpi.min() >= 0 and mpi.max() <= nb - L
    assert np.median(mp) == oracle.simple_sim(A, B, L, k=k)


def test_restatement_degenerate_shapes():
    rng = np.random.default_rng(1)
    A, B = unit_columns(rng, 9), unit_columns(rng, 23)
    mp, mpi = simple_profile_np(A, B, 10)
    assert len(mp) == 0 and len(mpi) == 0
    mp, mpi = simple_profile_np(B, A, 10)  # rows without a column: NaN and -1
    assert len(mp) == 14 and np.isnan(mp).all() and (mpi == -1).all()
    assert np.isnan(oracle.simple_sim(B, A, 10))


def test_ties_take_the_smallest_column():
    """A reference made of one 25-column block twice: column j and column j + 25 hold the same bits
    wherever both windows lie inside a copy, and the index is the first of them."""
    rng = np.random.default_rng(2)
    A, blk = unit_columns(rng, 40), unit_columns(rng, 25)
    B = np.concatenate([blk, blk], axis=1)
    mp, mpi = simple_profile_np(A, B, 10)
    assert (mpi < 25).all()
    _, mpi_first = simple_profile_np(A, blk, 10)  # the first copy alone
    tied = mpi < 16  # windows 0..15 of the block recur at +25
    assert tied.sum() >= 1
    assert np.array_equal(mpi[tied], mpi_first[tied])


def test_self_pair_is_zero_on_the_diagonal():
    A = unit_columns(np.random.default_rng(3), 37)
    mp, mpi = simple_profile_np(A, A, 10)
    assert np.array_equal(mp, np.zeros(28)) and np.array_equal(mpi, np.arange(28))


def test_subsequence_frames_by_hand():
    from acoss.engine import subsequence_frames
    # win 200, hop 100, sslen 10: subsequence i covers [100 i, 100 (i + 9) + 200)
    got = subsequence_frames([0, 3, 15, -1, 14], 10, 200, 100, 2450)
    # n = 2450 is no multiple of the hop: 24 columns, the last subsequence (15) ends at 2600 > n
    assert got.dtype == np.int64
    assert got.tolist() == [[0, 1100], [300, 1400], [1500, 2450], [-1, -1], [1400, 2450]]
    # per-row frame counts; a window wider than the hop by an odd amount; sslen 1
    got = subsequence_frames(np.array([2, 2, -1]), 1, 7, 3, np.array([100, 10, 5]))
    assert got.tolist() == [[6, 13], [6, 10], [-1, -1]]
    assert subsequence_frames(np.zeros(0, np.int32), 10, 200, 100, 5).shape == (0, 2)


def test_simple_profile_offsets():
    from acoss._lib import simple_profile_offsets
    lens = [30, 9, 10, 12]
    pairs = [(0, 1), (1, 0), (2, 3), (3, 3), (1, 1), (0, 0)]
    off = simple_profile_offsets(lens, pairs, 10)
    # rows = query length - 9, none for the 9-column track (a zero-length range)
    assert off.dtype == np.int64 and off.tolist() == [0, 21, 21, 22, 25, 25, 46]
    assert simple_profile_offsets(lens, pairs, 7).tolist() == [0, 24, 27, 31, 37, 40, 64]
    assert simple_profile_offsets(lens, np.zeros((0, 2), np.int32), 10).tolist() == [0]
    with pytest.raises(ValueError):
        simple_profile_offsets(lens, [(0, 4)], 10)
