"""GPU parity of the sweep's key-plane emit (k_sweep_rows9, csrc/crp_split.hip) against the CPU oracle.

The walk stages a column block's row-major 16-bit prefixes in a per-wave LDS tile of 32 rows x 56
columns and stores them as 16-byte pieces of 8 columns. What can go wrong there is a matter of
shape: the piece that straddles the line's end N', the skipped pieces behind it, the last rows of
a partial 32-row strip, the blocks' borders at multiples of 56 and the four waves' at multiples of
224, the `kNone` pad up to align32(N'), and, in a batch, the columns a longer pair left in the
planes. Every shape below goes through the shipped sweep and selects (acoss_crp_pair /
acoss_crp_align); every comparison is exact (==, thresholds by their bits).

Shapes are stacked sizes M' x N' (frames = size + 9 at m = 9, tau = 1).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import crp_cases
import oracle
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N': piece (8), block (56) and 4-wave (224) borders, N' % 8 and N' % 32 around the pad
NS = (1, 7, 8, 9, 47, 48, 55, 56, 57, 63, 64, 112, 113, 224, 225, 449)
# M': partial and full strips
MS = (1, 31, 32, 33, 69)
# a line past 2048 codes: the KQ = 2 launch
LONG = (40, 2100)
# run tracks (exact tie groups of every size, crp_cases.run_track) on these shapes: groups then
# lie across piece and block borders
RUN_SHAPES = ((57, 449), (69, 225), (33, 113))
KAPPAS = (0.095, 0.5)


def _frames(size):
    n = size + 9
    assert oracle.stacked_len(n, 9, 1) == size
    return n


def random_pair(Mp, Np, seed=5):
    """Chroma of independent uniform frames: no two cells of the CRP share a key, so a prefix that
    lands in the wrong column or row of a plane changes a threshold or a mask bit."""
    rng = np.random.Generator(np.random.PCG64([seed, Mp, Np]))
    return (rng.random((_frames(Mp), 12), dtype=np.float32), rng.random((_frames(Np), 12), dtype=np.float32))


def run_pair(Mp, Np):
    return crp_cases.make_pair(_frames(Mp), _frames(Np), "runs_x_runs")


def check_pair(X, Y, kappas=KAPPAS):
    """acoss_crp_pair == the oracle: OTI, row and column thresholds (bits), mask, Qmax."""
    k = oracle.oti(oracle.profile(X), oracle.profile(Y))
    D = oracle.crp_dist(X, Y, k, 9, 1)
    for kappa in kappas:
        got = _lib.crp_pair(X, Y, _lib.crp_params(kappa=kappa), dist=False)
        assert int(got["oti"].item()) == k
        tr, tc = oracle.crp_thresholds(D, kappa)
        where = "%d x %d, kappa=%r" % (D.shape + (kappa,))
        np.testing.assert_array_equal(got["thr_row"].cpu().numpy().view(np.uint32), tr.view(np.uint32),
                                      err_msg="row thresholds, " + where)
        np.testing.assert_array_equal(got["thr_col"].cpu().numpy().view(np.uint32), tc.view(np.uint32),
                                      err_msg="column thresholds, " + where)
        C = ((D <= tr[:, None]) & (D <= tc[None, :])).astype(np.uint8)
        Cg = got["crp"].cpu().numpy()
        np.testing.assert_array_equal(Cg, C, err_msg="mask, " + where)
        assert float(_lib.align_crp(got["crp"], 0).item()) == oracle.align(C, which=0), "Qmax, " + where


@pytest.mark.parametrize("Np", NS)
def test_emit_shapes(Np):
    for Mp in MS:
        check_pair(*random_pair(Mp, Np))


@pytest.mark.parametrize("shape", RUN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_emit_tie_groups(shape):
    check_pair(*run_pair(*shape))


def test_emit_long_lines():
    check_pair(*random_pair(*LONG), kappas=KAPPAS[:1])


def test_emit_no_short():
    """57 x 449 with the lane-strided short-line selects switched off: the long-line row select
    reads whole 32-element runs up to align32(N') (ACOSS_NO_SHORT is read once per process: hence
    the subprocess)."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_gpu_sweep_emit as t\n"
            "t.check_pair(*t.random_pair(57, 449))\n"
            "t.check_pair(*t.run_pair(57, 449))\n"
            "print('ok')\n" % [ROOT, os.path.join(ROOT, "acoss-1_amd"), os.path.join(ROOT, "tests")])
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ACOSS_NO_SHORT="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# stacked sizes of the batch's tracks: lines end inside a piece, on a piece, on a block; every
# pair but those of the longest track has N' < L
BATCH_SIZES = (1, 7, 9, 33, 47, 56, 57, 113, 225, 449, 600)


def test_emit_batch_mixed_lengths():
    """All ordered pairs of tracks of mixed lengths in one launch, then the same pairs in reverse
    order: each pair's planes (pitch and strips sized by the longest line L) then hold what a
    pair with other, often longer, lines left there. No stale column may reach a select."""
    rng = np.random.Generator(np.random.PCG64(17))
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
        got = _lib.crp_align(feats, off, lens, int(lens.max()), np.ascontiguousarray(pairs[order]), _lib.crp_params(),
                             qmax=True, dmax=True, oti=True)
        np.testing.assert_array_equal(got["oti"].cpu().numpy(), k[order])
        np.testing.assert_array_equal(got["qmax"].cpu().numpy(), q[order])
        np.testing.assert_array_equal(got["dmax"].cpu().numpy(), d[order])
