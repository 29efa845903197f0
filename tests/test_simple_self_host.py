"""CPU tests of the SiMPle self-join layer: the numpy restatement the GPU tests compare against
(tests/simple_self_np.py) pinned cell by cell to the oracle-pinned simple_profile_np, its symmetry,
its edges, and the host-only helpers of the Python layer."""
import numpy as np
import pytest

from simple_profile_np import frame_dots, simple_profile_np, unit_columns
from simple_self_np import masked_profile_np, motif_discord_np, self_dist_np, simple_self_np


@pytest.fixture(scope="module")
def track():
    A = unit_columns(np.random.default_rng(22), 22)
    return A, frame_dots(A, A)


def test_cells_are_the_pinned_distance(track):
    """dist[i, j] is simple_profile_np's only distance of block i against block j (P = Q = 1)."""
    A, ga = track
    L = 7
    dist = self_dist_np(A, L, ga)
    assert dist.shape == (16, 16)
    for i in range(16):
        for j in range(16):
            mp, mpi = simple_profile_np(A[:, i:i + L], A[:, j:j + L], L)
            assert mpi[0] == 0 and mp[0] == dist[i, j], (i, j)


@pytest.mark.parametrize("L", [7, 10])
def test_symmetric_with_a_zero_diagonal(track, L):
    A, ga = track
    dist = self_dist_np(A, L, ga)
    assert np.array_equal(dist.view(np.int64), dist.T.view(np.int64))
    assert np.array_equal(np.diag(dist).view(np.int64), np.zeros(len(dist), np.int64))  # +0, bit for bit


def test_excl_zero_only_drops_the_diagonal(track):
    A, ga = track
    dist = self_dist_np(A, 7, ga)
    mp, mpi = simple_self_np(A, 7, 0, ga)
    D = dist.copy()
    np.fill_diagonal(D, np.inf)
    assert np.array_equal(mp, D.min(1)) and np.array_equal(mpi, D.argmin(1))
    assert (mp > 0).all() and (mpi != np.arange(16)).all()


def test_edges(track):
    A, ga = track
    P = 16
    mp, mpi = simple_self_np(A, 7, P - 1, ga)
    assert len(mp) == P and np.isnan(mp).all() and (mpi == -1).all()
    mp, mpi = simple_self_np(A, 7, P + 5, ga)
    assert np.isnan(mp).all() and (mpi == -1).all()
    mp, mpi = simple_self_np(A, 7, P - 2, ga)  # only (0, P - 1) and (P - 1, 0) are admissible
    assert mpi.tolist() == [P - 1] + [-1] * (P - 2) + [0]
    assert np.isnan(mp[1:-1]).all() and mp[0] == mp[-1] == self_dist_np(A, 7, ga)[0, P - 1]
    for n in (6, 3, 0):  # P <= 0: no rows
        mp, mpi = simple_self_np(A[:, :n], 7, 3)
        assert mp.shape == (0,) and mpi.shape == (0,) and mpi.dtype == np.int32
    assert motif_discord_np(*simple_self_np(A, 7, P - 1, ga)) == ((-1, -1), -1)
    assert motif_discord_np(*simple_self_np(A, 7, P - 2, ga)) == ((0, P - 1), 0)


def test_nan_column_rows_have_no_answer():
    A = unit_columns(np.random.default_rng(5), 30)
    A[:, 12] = np.nan
    mp, mpi = simple_self_np(A, 7, 3)
    hit = np.zeros(24, bool)
    hit[6:13] = True
    assert np.isnan(mp[hit]).all() and (mpi[hit] == -1).all()
    assert not np.isnan(mp[~hit]).any() and not hit[mpi[~hit]].any()


def test_motif_discord_tie_rules():
    mp = np.array([np.nan, 3.0, 1.0, 5.0, 1.0, 5.0, np.nan, 0.0 + 1.0])
    mpi = np.array([-1, 7, 6, 5, 4, 3, -1, 1], np.int32)
    assert motif_discord_np(mp, mpi) == ((2, 6), 3)  # the first of the equal minima and of the equal maxima
    assert motif_discord_np(np.array([-0.0, 0.0]), np.array([1, 0], np.int32)) == ((0, 1), 0)  # -0 == +0
    assert motif_discord_np(np.array([np.nan, np.nan]), np.array([-1, -1], np.int32)) == ((-1, -1), -1)
    assert motif_discord_np(np.zeros(0), np.zeros(0, np.int32)) == ((-1, -1), -1)
    assert motif_discord_np(np.array([np.nan, 2.0]), np.array([-1, 0], np.int32)) == ((1, 0), 1)


def test_masked_profile_first_of_equals():
    D = np.zeros((6, 6))
    mp, mpi = masked_profile_np(D, 1)
    assert np.array_equal(mp, np.zeros(6)) and mpi.tolist() == [2, 3, 0, 0, 0, 0]


def test_simple_self_profile_offsets():
    from acoss._lib import simple_self_profile_offsets
    lens = [30, 9, 10, 12]
    off = simple_self_profile_offsets(lens, [0, 1, 2, 3, 1, 0], 10)
    assert off.dtype == np.int64 and off.tolist() == [0, 21, 21, 22, 25, 25, 46]
    assert simple_self_profile_offsets(lens, [3, 3], 7).tolist() == [0, 6, 12]
    assert simple_self_profile_offsets(lens, np.zeros(0, np.int32), 10).tolist() == [0]
    with pytest.raises(ValueError):
        simple_self_profile_offsets(lens, [4], 10)
    with pytest.raises(ValueError):
        simple_self_profile_offsets(lens, [-1], 10)


def test_negative_excl_is_refused_before_the_gpu():
    """ValueError before anything touches the GPU: it is raised on a machine without one."""
    from acoss import _lib
    A = unit_columns(np.random.default_rng(6), 20)
    with pytest.raises(ValueError):
        _lib.simple_self_profile([A], excl=-1)
    with pytest.raises(ValueError):
        _lib.simple_self_profile_packed(A.ravel(), [0], [20], [0], excl=-3)


def test_frames_of_minus_one():
    from acoss.engine import subsequence_frames
    motif = np.array([[2, 14], [-1, -1]], np.int32)
    got = subsequence_frames(motif.reshape(-1), 10, 200, 100, np.repeat([2450, 900], 2)).reshape(-1, 2, 2)
    assert got.tolist() == [[[200, 1300], [1400, 2450]], [[-1, -1], [-1, -1]]]
    assert subsequence_frames(np.array([-1, 0]), 10, 200, 100, np.array([50, 5000])).tolist() == [[-1, -1], [0, 1100]]
