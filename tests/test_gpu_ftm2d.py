"""GPU tests of FTM2D (ftm2d.hip, acoss/algorithms/ftm2d.py) on the eight tracks of tests/ftm2d_np.py.

Bars: beat-synchronous medians bit-exact (float32, np.median's arithmetic); chrompwr within 1e-14
relative of the numpy restatement (device pow against numpy's is a few ulp); shingles within 1e-12
absolute on the unit-norm entries (about 300x the 3.5e-15 floor between a direct-DFT and an
fft2-based float64 restatement, room for the pow / log / sqrt ulps); mirror partners equal;
golden parity on A, B, C, E within 2e-7 (shingles) and 1e-7 (scores), 6x the reference's own
float32 floor (3.2e-8 / 1.3e-8); scores within 1e-12 relative of the restatement on the GPU's own
shingles; each track computed alone equals its row of the batch.
"""
import os

import numpy as np
import pytest

import ftm2d_np
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

NAMES = ftm2d_np.NAMES
GOLD_TRACKS = "ABCE"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ftm2d_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def tracks():
    return ftm2d_np.make_tracks()


@pytest.fixture(scope="module")
def ref(tracks):
    """The restatement, computed once: {name: (sync f32, chrompwr f64, shingle f64)}."""
    out = {}
    for k in NAMES:
        sync = ftm2d_np.beat_sync(*tracks[k])
        ch = ftm2d_np.chrompwr(sync)
        out[k] = (sync, ch, ftm2d_np.shingle_from_chroma(ch))
    return out


@pytest.fixture(scope="module")
def batch(tracks):
    """(8, 900) shingles of A..H from one call."""
    sh = _lib.ftm2d_shingles([tracks[k][0] for k in NAMES], [tracks[k][1] for k in NAMES])
    assert tuple(sh.shape) == (8, 900) and str(sh.dtype) == "torch.float64" and sh.is_cuda
    return sh


def test_beatsync_medians_and_chrompwr(tracks, ref):
    names = NAMES[:7]
    sync, chroma = _lib.ftm2d_beatsync([tracks[k][0] for k in names], [tracks[k][1] for k in names])
    for k, s, c in zip(names, sync, chroma):
        assert s.dtype == np.float32 and s.shape == ref[k][0].shape
        np.testing.assert_array_equal(s, ref[k][0], err_msg="track " + k)
        gap = np.abs(c - ref[k][1]).max() / np.abs(ref[k][1]).max()
        print("chrompwr %s: max |gap| / max = %.3g" % (k, gap))
        np.testing.assert_allclose(c, ref[k][1], rtol=1e-14, atol=1e-300, err_msg="track " + k)


def test_shingles_match_restatement(batch, ref):
    got = batch.cpu().numpy()
    for i, k in enumerate(NAMES):
        gap = np.abs(got[i] - ref[k][2]).max()
        print("shingle %s: max |gap| = %.3g" % (k, gap))
    for i, k in enumerate(NAMES):
        assert np.isfinite(got[i]).all(), k
        np.testing.assert_allclose(got[i], ref[k][2], rtol=0, atol=1e-12, err_msg="track " + k)
        np.testing.assert_allclose(np.sqrt(np.sum(got[i] ** 2)), 1.0, rtol=1e-14)


def test_shingles_mirror_symmetry_is_exact(batch):
    s = batch.cpu().numpy().reshape(8, 12, 75)
    r, q = np.meshgrid(np.arange(12), np.arange(75), indexing="ij")
    c, k = (r + 6) % 12, (q + 38) % 75  # the DFT indices at (r, q) after fftshift
    pr, pq = ((12 - c) % 12 + 6) % 12, ((75 - k) % 75 + 37) % 75
    np.testing.assert_array_equal(s, s[:, pr, pq])


def test_silent_track_is_nan_where_the_restatement_is():
    h = np.zeros((500, 12), np.float32)
    o = np.arange(5, 500, 5)
    got = _lib.ftm2d_shingles([h], [o]).cpu().numpy()[0]
    want = ftm2d_np.shingle(h, o)
    assert np.isnan(want).all()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))


def test_golden_parity(batch, gold):
    idx = [NAMES.index(k) for k in GOLD_TRACKS]
    got = batch.cpu().numpy()[idx]
    for k, g in zip(GOLD_TRACKS, got):
        print("golden shingle %s: max |gap| = %.3g" % (k, np.abs(g - gold[k + "_shingle"]).max()))
    pairs = np.array([(i, j) for i in idx for j in idx], np.int32)
    sc = _lib.ftm2d_scores(batch, pairs).cpu().numpy().reshape(4, 4)
    print("golden scores: max |gap| = %.3g" % np.abs(sc - gold["scores_f64"]).max())
    for k, g in zip(GOLD_TRACKS, got):
        np.testing.assert_allclose(g, gold[k + "_shingle"], rtol=0, atol=2e-7, err_msg="track " + k)
    np.testing.assert_allclose(sc, gold["scores_f64"], rtol=0, atol=1e-7)


def test_scores(batch):
    host = batch.cpu().numpy()
    pairs = np.array([(i, j) for i in range(8) for j in range(8)], np.int32)
    sc = _lib.ftm2d_scores(batch, pairs)
    assert str(sc.dtype) == "torch.float64"
    sc = sc.cpu().numpy()
    want = ftm2d_np.score_matrix(host).reshape(-1)
    np.testing.assert_allclose(sc, want, rtol=1e-12, atol=0)
    assert (sc.reshape(8, 8)[np.arange(8), np.arange(8)] == 1.0).all()
    perm = np.random.default_rng(5).permutation(len(pairs))
    np.testing.assert_array_equal(_lib.ftm2d_scores(batch, pairs[perm]).cpu().numpy(), sc[perm])
    assert _lib.ftm2d_scores(batch, np.zeros((0, 2), np.int32)).numel() == 0
    with pytest.raises(ValueError):
        _lib.ftm2d_scores(batch, np.array([[0, 8]], np.int32))


def test_batch_independence(batch, tracks):
    host = batch.cpu().numpy()
    for i, k in enumerate(NAMES[:7]):
        alone = _lib.ftm2d_shingles([tracks[k][0]], [tracks[k][1]]).cpu().numpy()[0]
        np.testing.assert_array_equal(alone, host[i], err_msg="track " + k)


def test_workspace_chunks_do_not_change_a_row(batch, tracks):
    """33 copies of H hold 135,168 windows, more than one pass through the workspace (131,072): the
    tracks after the chunk boundary (the last H and A) must come out as in the batch of eight."""
    names = ["H"] * 33 + ["A"]
    got = _lib.ftm2d_shingles([tracks[k][0] for k in names], [tracks[k][1] for k in names]).cpu().numpy()
    host = batch.cpu().numpy()
    for i in (0, 31, 32):
        np.testing.assert_array_equal(got[i], host[NAMES.index("H")], err_msg="row %d" % i)
    np.testing.assert_array_equal(got[33], host[NAMES.index("A")])


def test_c_abi_refuses_short_track_with_its_index(tracks):
    import ctypes
    import torch
    lib = _lib.load_library()
    h = [tracks["A"][0], tracks["A"][0][:370]]
    feats, off, lens, bounds, bound_off = _lib.ftm2d_bounds(h, [tracks["A"][1], np.arange(5, 370, 5)], win=0)
    d = [_lib._dev(feats, torch.float32), _lib._dev(off, torch.int64), _lib._dev(lens, torch.int32),
         _lib._dev(bounds, torch.int64), _lib._dev(bound_off, torch.int64)]
    out = torch.empty((2, 900), dtype=torch.float64, device="cuda")
    rc = lib.acoss_ftm2d_shingles(_lib._ptr(d[0]), _lib._ptr(d[1]), _lib._ptr(d[2]), 2, 373, _lib._ptr(d[3]),
                                  _lib._ptr(d[4]), 75, 1.96, 5.0, _lib._ptr(out), _lib._stream())
    assert rc == -2  # ACOSS_E_SHAPE
    assert b"track 1" in lib.acoss_last_error()


def test_plugin_flow(tmp_path, monkeypatch):
    from acoss import coverid, evaluation
    monkeypatch.chdir(tmp_path)
    tr, labels = synthetic.make_corpus("covers80", frames=2400, seed=11)
    keep = np.flatnonzero(labels < 8)
    tr, labels = [tr[k] for k in keep], labels[keep]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), tr, labels, with_mfcc=True, beat_period=20)
    algo = coverid.benchmark(csv, fdir, algorithm="FTM2D", shortname="t", cachedir=str(tmp_path / "cache"))
    D = np.asarray(algo.Ds["main"])
    n = len(tr)
    assert D.shape == (n, n) and D.dtype == np.float32
    np.testing.assert_array_equal(D, D.T)
    assert (np.diag(D) == 0).all()
    # the restatement on the features as the plugin read them back from disk
    from acoss.features_io import load_many
    feats = load_many(algo.filepaths, keys=("hpcp", "madmom_features", "label"))
    sh = [ftm2d_np.shingle(f["hpcp"], f["madmom_features"]["onsets"]) for f in feats]
    assert all(len(algo.load_features(i)) == 900 for i in range(n)) and len(algo.shingles) == n
    np.testing.assert_allclose(np.stack([algo.shingles[i] for i in range(n)]), np.stack(sh), rtol=0, atol=1e-12)
    want = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    want[iu] = ftm2d_np.score_matrix(sh)[iu].astype(np.float32)
    want += want.T
    np.testing.assert_allclose(D, want, rtol=2e-7, atol=0)
    stats = algo.getEvalStatistics("main")
    ref_stats = evaluation.eval_statistics(D, labels)
    assert stats[:4] == tuple(ref_stats[:4]) and list(stats[4]) == list(ref_stats[4])
