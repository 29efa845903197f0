"""Host tests of the located Qmax: the numpy restatement (tests/qmax_trace_np.py) pinned to the
CPU oracle's score and to hand-derived answers, and engine.segment_frames against values worked
out by hand. No GPU."""
import numpy as np
import pytest

import oracle
import qmax_trace_np as qt
from qmax_trace_np import GAMMAS, NONE, SEEDS, SHAPES


def _mat(M, N, hits):
    C = np.zeros((M, N), np.uint8)
    for i, j in hits:
        C[i, j] = 1
    return C


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_restatement_score_is_the_oracles(shape):
    """The restatement's score equals oracle.align(C, go, ge, 0) on every matrix the GPU test uses."""
    M, N, density, run = shape
    for seed in SEEDS:
        for go, ge in GAMMAS:
            C, score, seg = qt.expected(M, N, density, run, seed, go, ge)
            assert score == oracle.align(C, go, ge, 0), (seed, go, ge)
            assert (seg == NONE) == (score == 0)
            if score > 0:
                i0, j0, i1, j1 = seg
                assert 2 <= i0 <= i1 < M and 2 <= j0 <= j1 < N
                assert C[i0, j0] == 1 and C[i1, j1] == 1  # a path starts and its maximum sits on a hit


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] * s[1] <= 5000], ids=lambda s: "%dx%d" % s[:2])
def test_row_form_equals_cell_form(shape):
    M, N, density, run = shape
    for seed in SEEDS:
        for go, ge in GAMMAS:
            C, score, seg = qt.expected(M, N, density, run, seed, go, ge)
            assert (score, seg) == qt.qmax_trace_cells(C, go, ge), (seed, go, ge)


def test_shared_matrices_tell_the_tie_rules_apart():
    """A reversed predecessor order and a "last maximum" end rule each change the answer on some of
    the shared dense matrices, so a kernel with either rule wrong cannot pass on them."""
    order = last = 0
    for M, N, density, run in [s for s in SHAPES if s[:2] in ((33, 70), (70, 45))]:
        for seed in SEEDS:
            for go, ge in GAMMAS:
                C, score, seg = qt.expected(M, N, density, run, seed, go, ge)
                order += qt.qmax_trace_cells(C, go, ge, order=(2, 1, 0))[1] != seg
                last += qt.qmax_trace_cells(C, go, ge, last_end=True)[1] != seg
    assert order > 0 and last > 0, (order, last)


def test_clean_diagonal_run():
    C = _mat(9, 8, [(3, 2), (4, 3), (5, 4), (6, 5)])  # 1, 2, 3, 4 along the diagonal
    assert qt.qmax_trace(C, 0.5, 0.5) == (4.0, (3, 2, 6, 5))


def test_gap_bridged():
    # (2,2) = 1, (3,3) = 2, the miss (4,4) = 2 - 0.5 = 1.5 (its a-predecessor is set: gamma_open),
    # (5,5) = 2.5, (6,6) = 3.5; the side cells (3,4) and (4,3) hold 0.5 and never win
    C = _mat(9, 9, [(2, 2), (3, 3), (5, 5), (6, 6)])
    assert qt.qmax_trace(C, 0.5, 0.5) == (3.5, (2, 2, 6, 6))
    # gamma_open = 0.7 is the one that applies (the predecessor of the gap is a hit)
    score, seg = qt.qmax_trace(C, 0.7, 0.3)
    assert score == float(np.float32(np.float32(np.float32(2) - np.float32(0.7)) + np.float32(2)))
    assert seg == (2, 2, 6, 6)


def test_equal_runs_first_end_in_row_major_order_wins():
    upper = [(2, 5), (3, 6), (4, 7)]   # ends at (4, 7) with 3
    lower = [(5, 2), (6, 3), (7, 4)]   # ends at (7, 4) with 3: smaller column, larger row
    assert qt.qmax_trace(_mat(10, 10, upper + lower), 0.5, 0.5) == (3.0, (2, 5, 4, 7))
    # two ends in one row: the smaller column wins
    left = [(2, 2), (3, 3), (4, 4)]
    right = [(2, 7), (3, 8), (4, 9)]
    assert qt.qmax_trace(_mat(7, 12, left + right), 0.5, 0.5) == (3.0, (2, 2, 4, 4))


def test_tie_between_a_and_b_takes_a():
    # (5,5) is a hit; a = (4,4) and b = (3,4) are both path starts with score 1, c = (4,3) is 0
    C = _mat(8, 8, [(3, 4), (4, 4), (5, 5)])
    assert qt.qmax_trace(C, 0.5, 0.5) == (2.0, (4, 4, 5, 5))
    assert qt.qmax_trace_cells(C, 0.5, 0.5, order=(2, 1, 0))[1] == (3, 4, 5, 5)  # what the wrong order gives


def test_no_alignment():
    assert qt.qmax_trace(np.zeros((6, 7), np.uint8)) == (0.0, NONE)
    C = np.zeros((6, 7), np.uint8)
    C[:2, :] = 1
    C[:, :2] = 1
    assert qt.qmax_trace(C) == (0.0, NONE)
    assert qt.qmax_trace(np.ones((2, 9), np.uint8)) == (0.0, NONE)
    assert qt.qmax_trace(np.ones((9, 2), np.uint8)) == (0.0, NONE)


def test_segment_frames_by_hand():
    from acoss.engine import segment_frames
    # m = 9, tau = 1, factor = 40: row 3 starts at frame 3 * 40 = 120; row 6 ends with downsampled
    # frame 6 + 8 = 14, i.e. before original frame 15 * 40 = 600; columns 2..5: 80 .. 14 * 40 = 560
    q, r = segment_frames([[3, 2, 6, 5]], 9, 1, 40, 2000, 600)
    assert q.tolist() == [[120, 600]] and r.tolist() == [[80, 560]]
    # the clamp at the track end (the last downsampled frame is short), per pair lengths, an empty one
    q, r = segment_frames([[3, 2, 6, 5], [-1, -1, -1, -1], [0, 0, 0, 0]], 9, 1, 40, [590, 2000, 350],
                          [530, 2000, 2000])
    assert q.tolist() == [[120, 590], [-1, -1], [0, 350]]
    assert r.tolist() == [[80, 530], [-1, -1], [0, 360]]
    # tau = 2, m = 4, factor = 10: row 7 ends with downsampled frame (7 + 3) * 2 = 20 -> 210
    q, r = segment_frames(np.array([[1, 0, 7, 3]]), 4, 2, 10, 10000, 10000)
    assert q.tolist() == [[20, 210]] and r.tolist() == [[0, 130]]
    q, r = segment_frames(np.zeros((0, 4), np.int32), 9, 1, 40, [], [])
    assert q.shape == (0, 2) and r.shape == (0, 2)


def test_stacked_len_is_the_c_formula():
    """engine.stacked_len against common.hpp's stacked_len written out (C division truncates; the
    operands are positive where it is reached), and against the two expressions that crp_pair and
    crp_path once spelled out inline."""
    from acoss.engine import stacked_len
    for tau in range(1, 4):
        for m in range(1, 11):
            for n in range(0, 61):
                inc = m * tau
                c = 0 if (n <= inc or tau <= 0) else int((n - inc + tau - 1) / tau)
                pair = max(0, -(-(n - m * tau) // tau)) if n > m * tau else 0
                path = 0 if n <= m * tau else (n - m * tau + tau - 1) // tau
                assert stacked_len(n, m, tau) == c == pair == path, (n, m, tau)
    assert stacked_len(300) == 291  # the defaults are the reference's m = 9, tau = 1
