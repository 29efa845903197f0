"""Host tests of the Qmax alignment path: the numpy restatement (tests/qmax_path_np.py) pinned to
the located Qmax's restatement (score and both end cells), to the path's own invariants and to
hand-derived paths, and engine.path_frames against values worked out by hand. No GPU."""
import numpy as np
import pytest

import qmax_path_np as qp
import qmax_trace_np as qt
from qmax_trace_np import GAMMAS, NONE, SEEDS, SHAPES

SMALL = [s for s in SHAPES if s[0] * s[1] <= 6000]
STEPS = {(1, 1), (2, 1), (1, 2)}


def _mat(M, N, hits):
    C = np.zeros((M, N), np.uint8)
    for i, j in hits:
        C[i, j] = 1
    return C


def _cases(shapes):
    for M, N, density, run in shapes:
        for seed in SEEDS:
            for go, ge in GAMMAS:
                yield M, N, density, run, seed, go, ge


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s[:2])
def test_row_form_equals_cell_form(shape):
    for case in _cases([shape]):
        C, score, path = qp.expected_path(*case)
        s2, p2 = qp.qmax_path_cells(C, case[5], case[6])
        assert score == s2, case
        assert path.tolist() == p2.tolist(), case


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_path_against_the_located_qmax(shape):
    """Score and both ends are the located Qmax's; the steps are of the three kinds; Q > 0 on
    every cell of the path; no more than min(M, N) cells."""
    for case in _cases([shape]):
        C, score, path = qp.expected_path(*case)
        _, want_score, seg = qt.expected(*case)
        assert score == want_score, case
        if len(path) == 0:
            assert seg == NONE, case
            continue
        assert tuple(path[0]) + tuple(path[-1]) == seg, case
        assert len(path) <= min(C.shape), case
        assert {tuple(d) for d in np.diff(path, axis=0).tolist()} <= STEPS, case
        Q = qp.score_matrix(C, case[5], case[6])
        assert (Q[path[:, 0], path[:, 1]] > 0).all(), case
        assert Q[path[-1, 0], path[-1, 1]] == np.float32(score), case


def test_shared_matrices_are_not_vacuous():
    """Counted with this restatement: 24 empty paths (the degenerate shapes), 120 paths of at
    least 20 cells, 101 that use all three step kinds and pass through a miss cell."""
    empty = long = rich = 0
    for case in _cases(SHAPES):
        C, score, path = qp.expected_path(*case)
        empty += len(path) == 0
        long += len(path) >= 20
        if len(path) > 1:
            kinds = {tuple(d) for d in np.diff(path, axis=0).tolist()}
            rich += kinds == STEPS and not C[path[:, 0], path[:, 1]].all()
    print("empty %d, >= 20 cells %d, three step kinds and a miss %d" % (empty, long, rich))
    assert long >= 120 and empty <= 24 and rich >= 1, (empty, long, rich)


def test_shared_matrices_tell_the_predecessor_orders_apart_on_the_path():
    """Another predecessor order changes the path on some shared matrices while both end cells
    stay: only a test of the whole path catches a kernel with that order (measured: 62 of the 252
    (case, order) combinations; 81 differ at all)."""
    differ = same_ends = 0
    for case in _cases(SMALL):
        C, score, path = qp.expected_path(*case)
        for order in ((1, 0, 2), (2, 1, 0), (0, 2, 1)):
            _, other = qp.qmax_path_cells(C, case[5], case[6], order=order)
            if other.tolist() != path.tolist():
                differ += 1
                same_ends += (len(other) > 0 and len(path) > 0 and other[0].tolist() == path[0].tolist()
                              and other[-1].tolist() == path[-1].tolist())
    print("paths that differ %d, of them with both ends equal %d" % (differ, same_ends))
    assert same_ends >= 1, (differ, same_ends)


def test_clean_diagonal_run():
    C = _mat(9, 8, [(3, 2), (4, 3), (5, 4), (6, 5)])
    score, path = qp.qmax_path(C, 0.5, 0.5)
    assert score == 4.0 and path.tolist() == [[3, 2], [4, 3], [5, 4], [6, 5]]


def test_gap_bridged_passes_through_the_miss():
    # (2,2) = 1, (3,3) = 2, the miss (4,4) = 1.5 with predecessor a = (3,3), (5,5) = 2.5, (6,6) = 3.5
    C = _mat(9, 9, [(2, 2), (3, 3), (5, 5), (6, 6)])
    want = [[2, 2], [3, 3], [4, 4], [5, 5], [6, 6]]
    for go, ge in ((0.5, 0.5), (0.7, 0.3)):
        score, path = qp.qmax_path(C, go, ge)
        assert path.tolist() == want
        assert qp.qmax_path_cells(C, go, ge)[1].tolist() == want
    assert qp.qmax_path(C, 0.5, 0.5)[0] == 3.5
    # steps of the other two kinds: (2,2) = 1 is b of the hit (4,3) = 2, which is c of the hit (5,5) = 3
    # (its a = (4,4) holds 0 and its b = (3,4) holds 0.5)
    C = _mat(8, 8, [(2, 2), (4, 3), (5, 5)])
    score, path = qp.qmax_path(C, 0.5, 0.5)
    assert score == 3.0 and path.tolist() == [[2, 2], [4, 3], [5, 5]]


def test_tie_between_a_and_b_takes_a():
    # (5,5) is a hit; a = (4,4) and b = (3,4) are both path starts with score 1, c = (4,3) is 0
    C = _mat(8, 8, [(3, 4), (4, 4), (5, 5)])
    score, path = qp.qmax_path(C, 0.5, 0.5)
    assert score == 2.0 and path.tolist() == [[4, 4], [5, 5]]
    assert qp.qmax_path_cells(C, 0.5, 0.5, order=(2, 1, 0))[1].tolist() == [[3, 4], [5, 5]]  # the wrong order's


def test_no_alignment():
    for C in (np.zeros((6, 7), np.uint8), np.ones((2, 9), np.uint8), np.ones((9, 2), np.uint8)):
        score, path = qp.qmax_path(C)
        assert score == 0.0 and path.shape == (0, 2)
    C = np.zeros((6, 7), np.uint8)
    C[:2, :] = 1
    C[:, :2] = 1
    score, path = qp.qmax_path(C)
    assert score == 0.0 and path.shape == (0, 2)
    assert qp.qmax_path_cells(C)[1].shape == (0, 2)


def test_path_frames_by_hand():
    from acoss.engine import path_frames, segment_frames
    # tau = 1, factor = 40: row 3 starts at original frame 120, column 2 at 80
    f = path_frames([[3, 2], [4, 3], [6, 4]], 1, 40)
    assert f.dtype == np.int64 and f.tolist() == [[120, 80], [160, 120], [240, 160]]
    # tau = 2, factor = 10: row 7 starts at downsampled frame 14, original frame 140
    assert path_frames(np.array([[1, 0], [7, 3]], np.int32), 2, 10).tolist() == [[20, 0], [140, 60]]
    assert path_frames(np.zeros((0, 2), np.int32), 1, 40).shape == (0, 2)
    # the first cell of a path maps to the lower ends of its segment's ranges
    q, r = segment_frames([[3, 2, 6, 4]], 9, 1, 40, 2000, 2000)
    assert [q[0, 0], r[0, 0]] == f[0].tolist()
