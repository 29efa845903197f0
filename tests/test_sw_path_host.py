"""The numpy restatement of the located and traced constrained Smith-Waterman alignment
(tests/sw_path_np.py) against the CPU oracle and against hand-written answers, and
engine.block_frames. No GPU."""
import numpy as np
import pytest

import oracle
import sw_path_np as sp
from acoss.engine import block_frames


def mat(M, N, cells):
    B = np.zeros((M, N), np.uint8)
    for rc in cells:
        B[rc] = 1
    return B


@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: "%dx%d-d%g-%s" % c)
def test_score_is_the_oracles(case):
    """Every matrix of the GPU test's list: score, length bound, cells, steps, and the re-summed path."""
    B, res = sp.expected(*case)
    M, N = B.shape
    assert res.score == oracle.sw_constrained(B)
    assert len(res.path) <= sp.path_bound(M, N)
    if res.score == 0:
        assert len(res.path) == 0 and res.seg == sp.NONE
        return
    p = res.path
    assert res.seg == (p[0, 0], p[0, 1], p[-1, 0], p[-1, 1])
    assert p[:, 0].min() >= 2 and p[:, 0].max() <= M - 2 and p[:, 1].min() >= 2 and p[:, 1].max() <= N - 2
    assert all(res.S[r, c] > 0 for r, c in p)
    assert {(int(a), int(b)) for a, b in np.diff(p, axis=0)} <= sp.STEPS
    assert sp.resum(B, p, res.choice[p[0, 0], p[0, 1]]) == res.score  # bit for bit
    # the end cell is the first in row-major order that holds the maximum
    assert (int(p[-1, 0]), int(p[-1, 1])) == tuple(int(v) for v in np.argwhere(res.S == res.S.max())[0])


@pytest.mark.parametrize("case", [c for c in sp.CASES if c[0] * c[1] <= 64 * 65], ids=lambda c: "%dx%d-d%g-%s" % c)
def test_two_forms_agree(case):
    B, res = sp.expected(*case)
    cells = sp.sw_path_cells(B)
    assert cells.score == res.score and cells.seg == res.seg
    assert np.array_equal(cells.path, res.path)
    assert np.array_equal(cells.S, res.S) and np.array_equal(cells.code, res.code)


def test_the_hard_cases_are_met():
    """What tests/test_gpu_sw_path.py asserts of its inputs holds for the shared list."""
    got = [sp.expected(*c) for c in sp.CASES]
    assert any(sp.tie_cells(B, r) for B, r in got)
    assert any(sp.miss_cells(B, r) for B, r in got)
    assert any(sp.crosses_row(r, 512) for _, r in got) and any(sp.crosses_row(r, 1024) for _, r in got)


def test_single_cell():
    """4 x 4 with only (2, 2) set: the one scored cell, a path of itself. Its predecessors are all
    unset, so the match pays the gap: (0 + 1) - 0.7; with (1, 1) set as well it scores 1."""
    for cells, score in (([(2, 2)], (0.0 + 1.0) + -0.7), ([(1, 1), (2, 2)], 1.0)):
        B = mat(4, 4, cells)
        for res in (sp.sw_path(B), sp.sw_path_cells(B)):
            assert res.score == score == oracle.sw_constrained(B)
            assert res.path.tolist() == [[2, 2]] and res.seg == (2, 2, 2, 2)


def test_clean_diagonal():
    B = mat(8, 8, [(k, k) for k in range(1, 7)])
    res = sp.sw_path(B)
    assert res.score == 5.0 == oracle.sw_constrained(B)
    assert res.path.tolist() == [[k, k] for k in range(2, 7)]
    assert res.seg == (2, 2, 6, 6)


def test_gap_bridged_by_a_two_one_step():
    B = mat(10, 10, [(1, 1), (2, 2), (3, 3), (5, 4), (6, 5), (7, 6)])
    res = sp.sw_path(B)
    assert res.score == 5.0 == oracle.sw_constrained(B)
    assert res.path.tolist() == [[2, 2], [3, 3], [5, 4], [6, 5], [7, 6]]


def test_row_major_first_end_wins():
    """Two diagonals of score 3, ending at (4, 8) and (8, 4)."""
    B = mat(12, 12, [(1 + k, 5 + k) for k in range(4)] + [(5 + k, 1 + k) for k in range(4)])
    res = sp.sw_path(B)
    assert res.S[4, 8] == res.S[8, 4] == res.score == 3.0
    assert res.seg == (2, 6, 4, 8) and res.path.tolist() == [[2, 6], [3, 7], [4, 8]]


TIE = np.array([[0, 1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1, 0], [1, 0, 1, 0, 0, 0, 0, 1, 0],
                [1, 0, 0, 0, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 1, 1, 0],
                [1, 1, 0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0, 1, 0]], np.uint8)


def test_tie_between_a_and_b_goes_to_a():
    """At (5, 6) the predecessors a = (4, 5) and b = (3, 5) are equal on x and differ in S; a wins, and
    the path tells: with b before a it would come through (3, 5)."""
    res = sp.sw_path(TIE)
    S = res.S
    xa = (S[4, 5] + 1.0) + (0.0 if TIE[4, 5] else -0.7)
    xb = (S[3, 5] + 1.0) + (0.0 if TIE[3, 5] else -0.7)
    assert TIE[5, 6] and xa == xb == S[5, 6] and S[4, 5] != S[3, 5] and S[4, 5] > 0 and S[3, 5] > 0
    assert (5, 6) in sp.tie_cells(TIE, res)
    assert res.path.tolist() == [[2, 2], [3, 4], [4, 5], [5, 6], [6, 7]]
    assert sp.sw_path_cells(TIE).path.tolist() == res.path.tolist()
    assert sp.sw_path_cells(TIE, order=(1, 0, 2)).path.tolist() == [[3, 5], [5, 6], [6, 7]]
    assert res.score == oracle.sw_constrained(TIE)


@pytest.mark.parametrize("M,N,bound", [(3, 9, 0), (4, 4, 1), (5, 9, 2), (47, 14, 11), (2, 2, 0), (130, 70, 67)])
def test_path_bound(M, N, bound):
    assert sp.path_bound(M, N) == bound == max(0, min(M, N) - 3)
    # met by the full diagonal
    if bound:
        B = mat(M, N, [(k, k) for k in range(1, min(M, N) - 1)])
        assert len(sp.sw_path(B).path) == bound


def test_block_frames():
    onsets = np.array([0, 10, 20, 31, 40, 52, 60, 70], np.int64)  # 8 onsets, blocksize 3: 5 blocks
    # block b covers [o[b], min(o[b + 3], n_frames))
    assert block_frames([0, 1, 4], onsets, 3, 1000).tolist() == [[0, 31], [10, 40], [40, 70]]
    # a range of blocks: the first block's start to the last block's end
    assert block_frames([[0, 4], [1, 2], [3, 3]], onsets, 3, 1000).tolist() == [[0, 70], [10, 52], [31, 60]]
    # the clamp to the frame count
    assert block_frames([[2, 4]], onsets, 3, 65).tolist() == [[20, 65]]
    # no alignment
    assert block_frames([[-1, -1], [0, 0]], onsets, 3, 1000).tolist() == [[-1, -1], [0, 31]]
    assert block_frames(np.zeros((0, 2), np.int64), onsets, 3, 10).shape == (0, 2)
    assert block_frames([[-1, -1]], [], 3, 10).tolist() == [[-1, -1]]
    with pytest.raises(ValueError):
        block_frames([[0, 5]], onsets, 3, 1000)
