"""GPU parity of the split CRP's selects around their runs of lines, against the CPU oracle.

A wave of the fused row select (csrc/crp_split.hip) owns a run of 8 consecutive rows: each row's
search lists the cells of its tie groups, and one flush per run recomputes their exact keys, ranks
them and finishes the rows. A wave of the column select owns 2 or 4 consecutive columns and
finishes each on its own. The cases here sit where that splits: line counts around the run
lengths, every line type, runs that mix a line settled in place (a group above 64 members) with
listed ones, runs whose lists overflow, the kappas that change what a line lists, and a pair built
so that a threshold falls outside the listed groups (the reload path). Every case goes through
acoss_crp_pair / acoss_crp_align; thresholds are compared by their bits, masks with ==.

The CPU side of each constructed case (that it has the property it is named for) is asserted from
the oracle's distances before the GPU is asked.
"""
import numpy as np
import pytest

import crp_cases
import oracle
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

RUN_ROWS = 8     # rows of a wave's run (rows_body)
RUN_CAP = 128    # member cells a run's lists hold (kRunCap)
GROUP_MAX = 64   # a larger group is ranked by histograms, in place


# ------------------------------------------------------------------------------------------
# CPU model of what a line lists (line_plan / line_defer), from its sorted 16-bit prefixes; the
# column lines go through the same model where a case is about the keys, not about the run
# ------------------------------------------------------------------------------------------
def _ranks(n, kappa):
    q = np.float32(n - 1) * np.float32(kappa)
    return int(np.floor(q)), int(np.ceil(q))


def line_groups(S, kappa):
    """Per line of S (ascending prefixes): Pl, g (the group of rank lo), Ph, gh (the next group when
    rank hi falls into it, else 0, 0)."""
    n = S.shape[1]
    lo, hi = _ranks(n, kappa)
    Pl = S[:, lo]
    less = (S < Pl[:, None]).sum(1)
    le = (S <= Pl[:, None]).sum(1)
    straddle = (hi != lo) & (hi >= le)
    Ph = np.where(straddle, S[np.arange(len(S)), np.minimum(le, n - 1)], 0)
    gh = np.where(straddle, (S == Ph[:, None]).sum(1), 0)
    return Pl.astype(np.int64), le - less, Ph.astype(np.int64), gh


def sq_threshold(thr):
    """common.hpp's sq_threshold: the largest float32 T with sqrt(T) <= thr, in its closed form."""
    thr = np.ascontiguousarray(thr, np.float32)
    up = (thr.view(np.uint32) + np.uint32(1)).view(np.float32)
    m = (thr.astype(np.float64) + up.astype(np.float64)) * 0.5
    m2 = m * m

    def down(x):
        u = np.ascontiguousarray(x, np.float32).view(np.uint32)
        return np.where(u == 0, u, u - np.uint32(1)).astype(np.uint32).view(np.float32)

    t = m2.astype(np.float32)
    t = np.where(t.astype(np.float64) > m2, down(t), t).astype(np.float32)
    tie = (t.astype(np.float64) == m2) & ((thr.view(np.uint32) & np.uint32(1)) == 1)
    return np.where(tie, down(t), t).astype(np.float32)


def _check_sq_threshold_model():
    """The model above against its definition, by sqrt on T and on its upper neighbour."""
    rng = np.random.Generator(np.random.PCG64(5))
    thr = np.abs(rng.standard_normal(4096)).astype(np.float32) * 7
    T = sq_threshold(thr)
    up = (T.view(np.uint32) + np.uint32(1)).view(np.float32)
    assert np.all(np.sqrt(T) <= thr) and np.all(np.sqrt(up) > thr)


# ------------------------------------------------------------------------------------------
# One pair on the GPU against the oracle
# ------------------------------------------------------------------------------------------
def check_pair(X, Y, kappas, D=None, k=None):
    """acoss_crp_pair of (X, Y) at every kappa: OTI, thresholds (bits) and mask equal to the
    oracle's. Returns the oracle's (k, D)."""
    if D is None:
        k = oracle.oti(oracle.profile(X), oracle.profile(Y))
        D = oracle.crp_dist(X, Y, k)
    for kappa in kappas:
        got = _lib.crp_pair(X, Y, _lib.crp_params(kappa=kappa), dist=False)
        assert int(got["oti"].item()) == k
        tr, tc = oracle.crp_thresholds(D, kappa)
        crp_cases._assert_thresholds(got["thr_row"].cpu().numpy(), tr, D, kappa, 0)
        crp_cases._assert_thresholds(got["thr_col"].cpu().numpy(), tc, D, kappa, 1)
        C = ((D <= tr[:, None]) & (D <= tc[None, :])).astype(np.uint8)
        np.testing.assert_array_equal(got["crp"].cpu().numpy(), C, err_msg="mask, kappa=%r" % kappa)
    return k, D


def _tracks(seed, M, N, runs=(False, True), sizes=crp_cases.SIZES):
    rng = np.random.Generator(np.random.PCG64(seed))
    alphabet = crp_cases.make_alphabet(rng)
    out = []
    for n, r in zip((M, N), runs):
        out.append(crp_cases.run_track(rng, n, sizes, alphabet) if r else crp_cases.natural_track(rng, n))
    return out


KAPPAS = (0.0, 0.095, 0.5, 0.999, 1.0)


# Rows M' around the 8-row run and the 32-row strip; the columns are LineS<8> / Line<32> lines.
@pytest.mark.parametrize("Np", [200, 1100])
@pytest.mark.parametrize("Mp", [1, 7, 8, 9, 15, 17, 33])
def test_rows_around_a_run(Mp, Np):
    X, Y = _tracks(100 + Mp, Mp + 9, Np + 9)
    check_pair(X, Y, KAPPAS)


# Columns N' around a wave's 2 (long lines) and 4 (short lines) columns, and 8; the columns are lines of
# M' = 150 (LineS<8>), 700 (LineS<16>) and 1,100 (Line<32>) codes.
@pytest.mark.parametrize("Mp", [150, 700, 1100])
@pytest.mark.parametrize("Np", [1, 2, 3, 4, 5, 7, 8, 9])
def test_columns_around_a_run(Np, Mp):
    Y, X = _tracks(200 + Np, Np + 9, Mp + 9)  # the run track is the query: ties inside every column
    check_pair(X, Y, KAPPAS)


# One shape per line type, on the tie matrices of crp_cases (two run tracks: both groups large),
# and 2,100 x 40: Line2 columns of a matrix whose rows are one short run each.
@pytest.mark.parametrize("shape", list(crp_cases.LINE_SHAPES), ids=lambda s: "%dx%d" % s)
def test_line_types_on_tie_matrices(shape):
    X, Y, k, D = crp_cases.case(shape[0], shape[1], "runs_x_runs")
    check_pair(X, Y, (0.095, 0.35), D, k)


def test_line2_columns_short_rows():
    X, Y = _tracks(7, 2109, 49, runs=(True, False))
    assert oracle.stacked_len(2109) == 2100 and oracle.stacked_len(49) == 40
    check_pair(X, Y, (0.003, 0.095, 0.5))


# (n - 1) kappa an integer (one order statistic, no interpolation), the minimum, and the top of
# the line, on a tie matrix of 201-code lines: q = 100 at kappa = 0.5, 50 at 0.25.
def test_kappa_integral_zero_and_near_one():
    X, Y = _tracks(9, 210, 210, runs=(True, True))
    assert oracle.stacked_len(210) == 201
    assert _ranks(201, 0.5) == (100, 100) and _ranks(201, 0.25) == (50, 50)
    check_pair(X, Y, (0.0, 0.25, 0.5, 0.995, 0.999, 0.9999, 1.0))


# ------------------------------------------------------------------------------------------
# Runs that mix lines settled in place with listed ones; runs whose lists overflow
# ------------------------------------------------------------------------------------------
def _silence_pair(first_silent_row):
    """A 200-frame query whose stacked rows [a, a + 3) are all silent, against a reference where
    108 frames are the twelve rotations of one quiet chroma vector (dyadic entries: equal norms,
    bit for bit). A silent row's squared distance to a stacked frame is that frame's norm alone, so
    those rows hold 100 equal keys at the bottom of the line; every other row tells the rotations
    apart and ties only the columns 12 apart."""
    rng = np.random.Generator(np.random.PCG64(31))
    X = crp_cases.natural_track(rng, 200)
    Y = crp_cases.natural_track(rng, 400)
    a = first_silent_row
    X[a:a + 3 + 8] = 0.0
    v = np.array([0.5, 0.25, 0, 0.125, 0, 0, 0.25, 0, 0, 0.125, 0, 0], np.float32)
    for t in range(108):
        Y[150 + t] = np.roll(v, t % 12)
    return X, Y


@pytest.mark.parametrize("a", [40, 45, 50, 53], ids=lambda a: "silent_rows_%d" % a)
def test_run_with_a_line_settled_in_place(a):
    """Rows a .. a + 2 are silence lines (a group of 100 equal keys: big_group_rank); a = 40: they open
    their run of 8 rows, 45: they close it, 50: ordinary lines on both sides, 53: they end a run and
    the next ones begin the following one."""
    X, Y = _silence_pair(a)
    k = oracle.oti(oracle.profile(X), oracle.profile(Y))
    D = oracle.crp_dist(X, Y, k)
    kappa = 0.095
    S = crp_cases.sorted_prefixes(D)[0]
    _, g, _, gh = line_groups(S, kappa)
    assert np.all(D[a:a + 3, 150:250] == D[a, 150]) and D[a, 150] == D[a].min()
    assert np.all(g[a:a + 3] > GROUP_MAX), g[a:a + 3]
    run = slice(a // RUN_ROWS * RUN_ROWS, a // RUN_ROWS * RUN_ROWS + RUN_ROWS)
    small = (g[run] <= GROUP_MAX) & (gh[run] <= GROUP_MAX)
    assert 0 < small.sum() < RUN_ROWS, (g[run], gh[run])
    check_pair(X, Y, (kappa, 0.3), D, k)


def test_run_whose_lists_overflow():
    """Every row crosses runs of 40 .. 60 equal frames: each row lists 40 .. 124 cells, so the
    third row of every run at the latest finds the lists (128 cells) full."""
    X, Y = _tracks(41, 120, 900, sizes=(40, 50, 60))
    k = oracle.oti(oracle.profile(X), oracle.profile(Y))
    D = oracle.crp_dist(X, Y, k)
    kappa = 0.2
    _, g, _, gh = line_groups(crp_cases.sorted_prefixes(D)[0], kappa)
    full_runs = 0
    for r0 in range(0, len(g) - RUN_ROWS + 1, RUN_ROWS):
        gg, hh = g[r0:r0 + RUN_ROWS], gh[r0:r0 + RUN_ROWS]
        listed = (gg <= GROUP_MAX) & (hh <= GROUP_MAX)
        full_runs += int((gg + hh)[listed].sum() > RUN_CAP and listed.sum() >= 3)
    assert full_runs >= 3, (full_runs, g, gh)
    check_pair(X, Y, (kappa, 0.095), D, k)


# ------------------------------------------------------------------------------------------
# The reload path: a threshold T whose prefix is outside the listed groups
# ------------------------------------------------------------------------------------------
def _integer_pair(seed, M, N):
    """Chroma of small integers: every squared distance is an integer below 2^8, exact in float32
    whatever the order of the sums, with the low 16 bits of its float32 pattern zero. So every key
    is the LEAST key of its 16-bit prefix, and every prefix group is a group of equal keys."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, 3, size=(M, 12)).astype(np.float32),
            rng.integers(0, 3, size=(N, 12)).astype(np.float32))


def _integer_keys(X, Y, k):
    Yr = np.roll(Y, k, axis=1)
    F = ((X[:, None, :].astype(np.int64) - Yr[None, :, :].astype(np.int64)) ** 2).sum(2)
    Mp, Np = oracle.stacked_len(len(X)), oracle.stacked_len(len(Y))
    d2 = np.zeros((Mp, Np), np.int64)
    for u in range(9):
        d2 += F[u:u + Mp, u:u + Np]
    return d2


def reload_lines(K, thr, kappa):
    """Lines of the key matrix K (uint32 patterns, one line per row) that list their groups (both at
    most 64 members) and whose T = sq_threshold(thr) has a prefix that is neither Pl, nor Ph, nor
    between them: the flush cannot correct le_mask(Pl) into "key <= T" and reloads the line."""
    S = np.sort((K >> 16).astype(np.int64), axis=1)
    Pl, g, Ph, gh = line_groups(S, kappa)
    T16 = (sq_threshold(thr).view(np.uint32) >> 16).astype(np.int64)
    listed = (g <= GROUP_MAX) & (gh <= GROUP_MAX)
    ok = (T16 == Pl) | ((gh > 0) & (T16 > Pl) & (T16 <= Ph))
    return np.flatnonzero(listed & ~ok), listed, g + gh


def test_threshold_outside_the_listed_groups():
    """Both order statistics are the same integer key a (a tie): thr = s (hi - q) + s (q - lo) with
    s = sqrt(a) rounds below s for about 4 % of the integers at this kappa, T = sq_threshold(thr)
    is then below a, and a is the least key of its prefix: T's prefix is Pl - 1."""
    _check_sq_threshold_model()
    M, N, kappas = 200, 240, (0.31, 0.27, 0.61, 0.095)
    X, Y = _integer_pair(17, M, N)
    k = oracle.oti(oracle.profile(X), oracle.profile(Y))
    D = oracle.crp_dist(X, Y, k)
    d2 = _integer_keys(X, Y, k)
    assert d2.max() < 256
    keys = d2.astype(np.float32)
    np.testing.assert_array_equal(np.sqrt(keys).view(np.uint32), D.view(np.uint32))
    K = keys.view(np.uint32)
    assert np.all((K & 0xffff) == 0)
    n_rows = n_cols = 0
    for kappa in kappas:
        tr, tc = oracle.crp_thresholds(D, kappa)
        rows, _, cells_r = reload_lines(K, tr, kappa)
        cols, _, cells_c = reload_lines(np.ascontiguousarray(K.T), tc, kappa)
        # the lists of the lines' runs do not overflow (else the line would be settled in place)
        rows = [int(r) for r in rows if cells_r[r // 8 * 8:r // 8 * 8 + 8].sum() <= RUN_CAP]
        cols = [int(c) for c in cols if cells_c[c // 8 * 8:c // 8 * 8 + 8].sum() <= RUN_CAP]
        print("kappa %g reload lines: rows %s, columns %s" % (kappa, rows, cols))
        n_rows += len(rows)
        n_cols += len(cols)
    assert n_rows >= 2 and n_cols >= 2
    check_pair(X, Y, kappas, D, k)


# ------------------------------------------------------------------------------------------
# A mixed-length batch
# ------------------------------------------------------------------------------------------
def test_mixed_length_batch():
    """acoss_crp_align over all ordered pairs of six tracks of 40 .. 1,300 frames, two of them run
    tracks and one with a silence: runs of every line type of a long-line launch in one call."""
    rng = np.random.Generator(np.random.PCG64(51))
    alphabet = crp_cases.make_alphabet(rng)
    lengths = [40, 130, 333, 520, 700, 1300]
    tracks = []
    for t, n in enumerate(lengths):
        x = crp_cases.run_track(rng, n, crp_cases.SIZES, alphabet) if t in (2, 4) else crp_cases.natural_track(rng, n)
        if t == 3:
            x[n // 6:n // 2] = 0.0
        tracks.append(x)
    feats, off, lens = synthetic.pack(tracks)
    pairs = np.array([(i, j) for i in range(6) for j in range(6) if i != j], np.int32)
    for kappa in (0.095, 0.3):
        q, d, k = oracle.crp_batch(feats, off, lens, pairs, kappa=kappa)
        got = _lib.crp_align(feats, off, lens, int(lens.max()), pairs, _lib.crp_params(kappa=kappa), qmax=True,
                             dmax=True, oti=True)
        np.testing.assert_array_equal(got["oti"].cpu().numpy(), k)
        np.testing.assert_array_equal(got["qmax"].cpu().numpy(), q)
        np.testing.assert_array_equal(got["dmax"].cpu().numpy(), d)
