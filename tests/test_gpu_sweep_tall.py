"""GPU parity of the sweep (k_sweep_rows9, csrc/crp_split.hip) at strip borders, against the CPU
oracle.

A block walks one 32-row strip; the next strip's block starts the nine diagonal windows of rows
32, 64, ... anew from its own eight warm-up frames, and both write their halves of a column's
strip-major run. tests/test_gpu_sweep_emit.py covers the shapes of a line's end (N'); this file
covers where M' falls among the strips: a partial last strip after one to five full ones, a pair
that ends exactly on a strip, more than 64 strips (the launch whose columns take the two-half
line), and, in a batch, pairs whose trailing strips lie wholly inside what a longer pair left in
the planes. Every shape goes through the shipped sweep and selects (acoss_crp_pair /
acoss_crp_align); every comparison is exact (==, thresholds by their bits).

Shapes are stacked sizes M' x N' (frames = size + 9 at m = 9, tau = 1).
"""
import numpy as np
import pytest

import crp_cases
import oracle
from acoss import _lib, synthetic
from test_gpu_sweep_emit import _frames, check_pair, random_pair, run_pair

pytestmark = pytest.mark.gpu

# M': around every strip border up to five strips
MS = (33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 161)
# N': inside a piece, just past a 56-column block, just past the 4-wave round
NS = (7, 57, 225)
RUN_SHAPES = ((97, 113), (129, 225))
LONG = (2100, 40)  # 66 strips, rows of 40 codes, columns past 2048 codes: the KQ = 2 launch
BATCH_SIZES = (1, 33, 64, 65, 97, 129, 225, 449)


@pytest.mark.parametrize("Np", NS)
def test_strip_borders(Np):
    for Mp in MS:
        check_pair(*random_pair(Mp, Np))


def test_windows_at_strip_borders():
    """On a random pair every cell has its own key, so a window that starts late or one lane off
    where one strip's block hands over to the next changes the thresholds of the rows whose nine
    terms straddle that border (and of their neighbours). Those rows are compared border by
    border, so a failure names the border."""
    Mp, Np = 161, 57
    X, Y = random_pair(Mp, Np)
    k = oracle.oti(oracle.profile(X), oracle.profile(Y))
    D = oracle.crp_dist(X, Y, k, 9, 1)
    tr, tc = oracle.crp_thresholds(D, 0.095)
    got = _lib.crp_pair(X, Y, _lib.crp_params(kappa=0.095), dist=False)
    gr = got["thr_row"].cpu().numpy().view(np.uint32)
    C = ((D <= tr[:, None]) & (D <= tc[None, :])).astype(np.uint8)
    Cg = got["crp"].cpu().numpy()
    for border in range(32, Mp, 32):
        rows = slice(border - 8, min(border + 9, Mp))
        np.testing.assert_array_equal(gr[rows], tr.view(np.uint32)[rows],
                                      err_msg="row thresholds around the strip border at row %d" % border)
        np.testing.assert_array_equal(Cg[rows], C[rows], err_msg="mask around the strip border at row %d" % border)
    np.testing.assert_array_equal(gr, tr.view(np.uint32), err_msg="row thresholds")
    np.testing.assert_array_equal(got["thr_col"].cpu().numpy().view(np.uint32), tc.view(np.uint32),
                                  err_msg="column thresholds")
    np.testing.assert_array_equal(Cg, C, err_msg="mask")


@pytest.mark.parametrize("shape", RUN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_tie_groups_across_borders(shape):
    check_pair(*run_pair(*shape))


def test_long_columns():
    check_pair(*random_pair(*LONG), kappas=(0.095,))


def test_batch_mixed_lengths():
    """All ordered pairs of tracks of mixed lengths in one launch, then the same pairs in reverse
    order: each pair's planes (pitch and strips sized by the longest line) then hold what a pair
    with other lines left there. No stale row or column may reach a select."""
    rng = np.random.Generator(np.random.PCG64(23))
    alphabet = crp_cases.make_alphabet(rng)
    tracks = []
    for t, size in enumerate(BATCH_SIZES):
        n = _frames(size)
        tracks.append(crp_cases.run_track(rng, n, crp_cases.SIZES, alphabet) if t % 4 == 3
                      else rng.random((n, 12), dtype=np.float32))
    feats, off, lens = synthetic.pack(tracks)
    T = len(tracks)
    pairs = np.array([(i, j) for i in range(T) for j in range(T) if i != j], np.int32)
    q, d, k = oracle.crp_batch(feats, off, lens, pairs)
    for order in (np.arange(len(pairs)), np.arange(len(pairs))[::-1]):
        got = _lib.crp_align(feats, off, lens, int(lens.max()), np.ascontiguousarray(pairs[order]),
                             _lib.crp_params(), qmax=True, dmax=True, oti=True)
        np.testing.assert_array_equal(got["oti"].cpu().numpy(), k[order])
        np.testing.assert_array_equal(got["qmax"].cpu().numpy(), q[order])
        np.testing.assert_array_equal(got["dmax"].cpu().numpy(), d[order])
