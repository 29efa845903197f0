"""Host tests of the dmax (chen17) alignment path: the numpy restatement (tests/dmax_path_np.py)
pinned to the CPU oracle's chen17 score, to its own cell-by-cell form, to the path's invariants
and to hand-derived paths, one per way a path can start. No GPU."""
import numpy as np
import pytest

import dmax_path_np as dp
import oracle
import qmax_path_np as qp
from dmax_path_np import GAMMAS, NONE, SEEDS, SHAPES

SMALL = [s for s in SHAPES if s[0] * s[1] <= 25000]
OTHER_ORDERS = [(0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


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


_CELLS = {}


def _cells(case, order=(0, 1, 2)):
    """The cell-by-cell form of one small case, once per process."""
    key = case + (order,)
    if key not in _CELLS:
        _CELLS[key] = dp.dmax_path_cells(dp.expected_path(*case)[0], case[5], case[6], order)
    return _CELLS[key]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s[:2])
def test_row_form_equals_cell_form(shape):
    for case in _cases([shape]):
        C, score, path, seg = dp.expected_path(*case)
        s2, p2, _ = _cells(case)
        assert score == s2, case
        assert path.tolist() == p2.tolist(), case
        assert seg == (tuple(path[0]) + tuple(path[-1]) if len(path) else NONE), case


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_score_is_the_oracles_and_the_path_adds_up_to_it(shape):
    """dmax equals or_align(which = 1) on every shared matrix; the steps are of the five kinds, the
    two short ones exactly after an intermediate; every intermediate and every first cell is a hit;
    the float32 re-accumulation along the path gives dmax; no more cells than the bound."""
    for case in _cases([shape]):
        C, score, path, seg = dp.expected_path(*case)
        assert np.float32(score) == np.float32(oracle.align(C, case[5], case[6], which=1)), case
        if len(path) == 0:
            assert score == 0.0 and seg == NONE, case
            continue
        steps = [tuple(d) for d in np.diff(path, axis=0).tolist()]
        assert set(steps) <= dp.STEPS, case
        assert all(a not in ((1, 0), (0, 1)) or b not in ((1, 0), (0, 1)) for a, b in zip(steps, steps[1:])), case
        mids = [t for t, s in enumerate(steps) if s in ((1, 0), (0, 1))]
        assert all(C[tuple(path[t])] for t in mids) and C[tuple(path[0])], case
        assert path[0].min() >= 1 and (len(path) == 1 or path[1:].min() >= 2), case
        assert len(path) <= dp.path_bound(*C.shape), case
        assert np.float32(dp.resum(C, path, case[5], case[6])) == np.float32(score), case


def test_shared_matrices_are_not_vacuous():
    """On the small shapes: paths that begin on an intermediate cell, intermediates inside paths,
    paths that differ from the Qmax path of the same matrix, and, for each of the five other
    predecessor orders, a path that changes under it (looked for on the matrices of at most 6,000
    cells: the cell-by-cell form is slow)."""
    start_mid = mids = differ = nonempty = 0
    changed = {o: 0 for o in OTHER_ORDERS}
    for case in _cases(SMALL):
        C, score, path, seg = dp.expected_path(*case)
        if len(path) == 0:
            continue
        nonempty += 1
        first = tuple(path[0])
        start_mid += int(min(first) < 2 or len(path) > 1 and tuple(path[1] - path[0]) in ((1, 0), (0, 1)))
        mids += sum(tuple(d) in ((1, 0), (0, 1)) for d in np.diff(path, axis=0).tolist())
        differ += int(qp.qmax_path(C, case[5], case[6])[1].tolist() != path.tolist())
        for o in OTHER_ORDERS if C.size <= 6000 else ():
            s2, p2, _ = _cells(case, o)
            assert s2 == score, (case, o)
            changed[o] += int(p2.tolist() != path.tolist())
    print("non-empty %d, begin on an intermediate %d, intermediates %d, differ from Qmax %d, changed %r"
          % (nonempty, start_mid, mids, differ, changed))
    assert nonempty >= 60 and start_mid >= 1 and mids >= 100 and differ >= 30
    assert all(n >= 1 for n in changed.values()), changed


def test_staircase_comes_near_the_bound():
    """A b / c staircase from (2, 2) on 40 x 40: every step adds an intermediate and a DP cell for
    three of rows plus columns, 24 steps fit, so 49 cells, two below the bound of
    floor(160 / 3) - 2 = 51 and well above min(M, N) = 40. One more hit above the first cell makes
    the path begin on an intermediate in row 1: 50 cells."""
    C = dp.make_staircase(40, 40, (2, 2), "bc")
    score, path, seg = dp.dmax_path(C)
    assert dp.path_bound(40, 40) == 51
    assert len(path) == 49 and score == 49.0 and seg[:2] == (2, 2)
    assert len(path) >= dp.path_bound(40, 40) - 2 and len(path) > 40
    s2, p2, _ = dp.dmax_path_cells(C)
    assert (s2, p2.tolist()) == (score, path.tolist())
    C[1, 2] = 1
    score, path, seg = dp.dmax_path(C)
    assert len(path) == 50 and score == 50.0 and seg[:2] == (1, 2)
    assert dp.resum(C, path) == 50.0
    # the smallest matrix meets the bound: 2 cells on 3 x 3
    score, path, _ = dp.dmax_path(_mat(3, 3, [(1, 2), (2, 2)]))
    assert path.tolist() == [[1, 2], [2, 2]] and score == 2.0 and dp.path_bound(3, 3) == 2


KNOWN = [
    # a path that starts on X: a hit whose three raw values are 0
    ("start on X", (5, 5), [(2, 2), (3, 3)], 2.0, [(2, 2), (3, 3)]),
    # X = (3, 3) through b: P = (1, 2) scores 0 (row 1), I = (2, 3) is a hit: the path begins on I
    ("start on I via b", (5, 5), [(2, 3), (3, 3)], 2.0, [(2, 3), (3, 3)]),
    # X = (3, 3) through c: P = (2, 1) scores 0 (column 1), I = (3, 2) is a hit
    ("start on I via c", (5, 5), [(3, 2), (3, 3)], 2.0, [(3, 2), (3, 3)]),
    # X = (2, 3) through b: I = (1, 3) lies in row 1 and is reported, P = (0, 2)
    ("start on I in row 1", (5, 5), [(1, 3), (2, 3)], 2.0, [(1, 3), (2, 3)]),
    # a b staircase: (3, 3) and (5, 4) are the intermediates of the steps to (4, 3) and (6, 4);
    # five cells on a 7 x 5 matrix, min(M, N) of them
    ("b staircase", (7, 5), [(2, 2), (3, 3), (4, 3), (5, 4), (6, 4)], 5.0,
     [(2, 2), (3, 3), (4, 3), (5, 4), (6, 4)]),
    # a miss on the path: (4, 4) is a miss reached by a from (3, 3), 2 - 0.5; (5, 5) a hit again
    ("through a miss", (7, 7), [(2, 2), (3, 3), (5, 5)], 2.5, [(2, 2), (3, 3), (4, 4), (5, 5)]),
]


@pytest.mark.parametrize("name,shape,hits,score,path", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers(name, shape, hits, score, path):
    C = _mat(shape[0], shape[1], hits)
    for got_score, got_path in (dp.dmax_path(C)[:2], dp.dmax_path_cells(C)[:2]):
        assert got_score == score
        assert [tuple(c) for c in got_path.tolist()] == path
    assert dp.dmax_path(C)[2] == path[0] + path[-1]
    assert oracle.align(C, which=1) == score
    assert dp.resum(C, np.array(path)) == score
