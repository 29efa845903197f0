"""CPU checks behind tests/test_gpu_crp_params.py: the generated cases reach every branch class
of the split selects (tests/crp_cases.py census), and the oracle's percentile, the reference of
every GPU threshold test, equals a plain numpy restatement bit for bit over the kappa sweep."""
import numpy as np
import pytest

import crp_cases
import oracle

MIN_LINES = 3


def test_run_track_gives_exact_tie_groups():
    """A run of g + 8 identical frames stacks (m = 9, tau = 1) into g identical frames: a line
    across a run track holds groups of bit-equal distances of exactly the drawn sizes."""
    rng = np.random.Generator(np.random.PCG64(1))
    alphabet = crp_cases.make_alphabet(rng)
    assert len(np.unique(alphabet, axis=0)) == len(alphabet)
    Y = crp_cases.run_track(rng, 900, crp_cases.SIZES, alphabet)
    assert Y.shape == (900, 12) and Y.dtype == np.float32
    edges = np.flatnonzero(np.any(Y[1:] != Y[:-1], axis=1)) + 1
    runs = np.diff(np.concatenate([[0], edges]))  # all but the last (cut at n)
    assert len(runs) > 5 and set(runs - 8) <= set(crp_cases.SIZES)
    X = crp_cases.natural_track(rng, 40)
    D = oracle.crp_dist(X, Y, 0)
    for a, r in zip(np.concatenate([[0], edges]), runs):
        blk = D[:, a:a + r - 8].view(np.uint32)
        assert np.all(blk == blk[:, :1])


@pytest.mark.parametrize("shape", list(crp_cases.LINE_SHAPES), ids=lambda s: "%dx%d" % s)
def test_census_reaches_every_class(shape):
    """Summed over both pairings and the kappa list the GPU test runs at this shape, every class
    holds at least MIN_LINES lines (counts per class: the message of a failure, or -s)."""
    M, N = shape
    total = dict.fromkeys(crp_cases.CLASSES, 0)
    for pairing in crp_cases.PAIRINGS:
        D = crp_cases.case(M, N, pairing)[3]
        prefixes = crp_cases.sorted_prefixes(D)
        for kappa in crp_cases.kappas_for(M, N):
            for c, v in crp_cases.census(D, kappa, prefixes).items():
                total[c] += v
    print("census %dx%d (%s): %s" % (M, N, crp_cases.LINE_SHAPES[shape], total))
    lines = 2 * ((M - 9) + (N - 9)) * len(crp_cases.kappas_for(M, N))
    assert sum(total.values()) == lines
    assert min(total.values()) >= MIN_LINES, total


def test_census_classes_on_built_lines():
    """The classifier itself, on lines built to sit in each class (n = 201, kappa = 0.5: q = 100
    an integer; kappa = 0.0975: q = 19.5, lo = 19, hi = 20)."""
    def line(groups):  # [(value, count), ...] ascending -> a (1, n) distance line
        return np.concatenate([np.full(c, v, np.float32) for v, c in groups])[None, :]

    def cls(groups, kappa):
        D = line(groups)
        assert D.shape[1] == 201
        S = np.sort(((D * D).view(np.uint32) >> 16).astype(np.uint16), axis=1)
        return crp_cases.CLASSES[int(crp_cases._line_classes(S, kappa)[0])]

    assert cls([(1.0, 90), (2.0, 20), (3.0, 91)], 0.5) == "int_q/g<=64"
    assert cls([(1.0, 90), (2.0, 111)], 0.5) == "int_q/g>64"
    assert cls([(1.0, 10), (2.0, 20), (3.0, 171)], 0.0975) == "same/g<=64"
    assert cls([(1.0, 10), (2.0, 70), (3.0, 121)], 0.0975) == "same/g>64"
    assert cls([(1.0, 20), (2.0, 44), (3.0, 137)], 0.0975) == "straddle/both<=64"
    assert cls([(1.0, 20), (2.0, 45), (3.0, 136)], 0.0975) == "straddle/sum>64"
    assert cls([(0.5, 1), (1.0, 19), (2.0, 65), (3.0, 116)], 0.0975) == "straddle/gh>64"
    assert cls([(2.0, 20), (3.0, 181)], 0.0975) == "straddle/gh>64"
    assert cls([(2.0, 20), (2.5, 1), (3.0, 180)], 0.0975) == "straddle/both<=64"
    assert cls([(1.0, 20), (2.0, 80), (3.0, 101)], 0.4975) == "straddle/g>64"  # q = 99.5
    # census() counts the rows and the columns: two rows with q = 100 inside groups of 181 and
    # 111, and 201 columns of two distinct elements (q = 0.5)
    D = np.concatenate([line([(2.0, 20), (3.0, 181)]), line([(1.0, 90), (2.0, 111)])])
    want = dict.fromkeys(crp_cases.CLASSES, 0)
    want.update({"int_q/g>64": 2, "straddle/both<=64": 201})
    assert crp_cases.census(D, 0.5) == want


@pytest.mark.parametrize("shape", [(300, 500), (700, 1000)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pairing", crp_cases.PAIRINGS)
def test_oracle_percentile_equals_numpy(shape, pairing):
    """oracle.crp_thresholds (nth_element + the minimum above it) against the full-sort numpy form,
    bit for bit, at every kappa of the sweep (kappa = 0 and 1: the minimum and the maximum)."""
    D = crp_cases.case(shape[0], shape[1], pairing)[3]
    for kappa in crp_cases.KAPPAS:
        tr, tc = oracle.crp_thresholds(D, kappa)
        nr, nc = crp_cases.np_thresholds(D, kappa)
        np.testing.assert_array_equal(tr.view(np.uint32), nr.view(np.uint32), err_msg="rows, kappa=%g" % kappa)
        np.testing.assert_array_equal(tc.view(np.uint32), nc.view(np.uint32), err_msg="cols, kappa=%g" % kappa)
    tr, tc = oracle.crp_thresholds(D, 0.0)
    np.testing.assert_array_equal(tr, D.min(1))
    np.testing.assert_array_equal(tc, D.min(0))
    tr, tc = oracle.crp_thresholds(D, 1.0)
    np.testing.assert_array_equal(tr, D.max(1))
    np.testing.assert_array_equal(tc, D.max(0))


def test_oracle_percentile_one_element_lines():
    """A one-row matrix: every column line has one element (n - 1 = 0, q = 0 at any kappa) and is
    its own threshold; the row line still interpolates. And its transpose."""
    D = np.ascontiguousarray(crp_cases.case(300, 500, "nat_x_runs")[3][7:8])
    for kappa in crp_cases.KAPPAS:
        for A in (D, np.ascontiguousarray(D.T)):
            tr, tc = oracle.crp_thresholds(A, kappa)
            nr, nc = crp_cases.np_thresholds(A, kappa)
            np.testing.assert_array_equal(tr.view(np.uint32), nr.view(np.uint32))
            np.testing.assert_array_equal(tc.view(np.uint32), nc.view(np.uint32))
        tr, tc = oracle.crp_thresholds(D, kappa)
        np.testing.assert_array_equal(tc.view(np.uint32), D[0].view(np.uint32))
    one = np.array([[0.625]], np.float32)
    for kappa in (0.0, 0.095, 1.0):
        tr, tc = oracle.crp_thresholds(one, kappa)
        assert tr.tolist() == [0.625] and tc.tolist() == [0.625]
