"""GPU tests of the located Qmax (acoss_locate_crp / acoss_crp_locate, crp_dp.hip k_crp_dp_trace)
against the numpy restatement tests/qmax_trace_np.py: segments and scores compare with `==`, and
the score also equals the shipped DP's (acoss_align_crp / acoss_crp_align) and the CPU oracle's."""
import numpy as np
import pytest

import oracle
import qmax_trace_np as qt
from qmax_trace_np import GAMMAS, SEEDS, SHAPES
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_locate_crp_matches_restatement(shape):
    """Degenerate shapes, dense tie-rich matrices (both tie rules decide answers there, see
    test_locate_host.py) and sparse ones with a planted run across rows 512, 1024 and 2048: every
    lane, band and strip edge of both rows-per-lane choices."""
    M, N, density, run = shape
    for seed in SEEDS:
        for go, ge in GAMMAS:
            C, score, seg = qt.expected(M, N, density, run, seed, go, ge)
            s, g = _lib.locate_crp(C, go, ge)
            got_s, got_g = float(s.item()), tuple(int(x) for x in g.cpu().numpy())
            print("%dx%d seed %d gamma (%g, %g): score %r seg %r, restatement %r %r"
                  % (M, N, seed, go, ge, got_s, got_g, score, seg))
            assert got_g == seg, (seed, go, ge)
            assert got_s == score, (seed, go, ge)
            assert got_s == float(_lib.align_crp(C, 0, go, ge).item()), (seed, go, ge)


def test_locate_crp_rejects_nonbinary():
    C = np.zeros((10, 10), np.uint8)
    C[3, 4] = 2
    with pytest.raises(_lib.AcossHipError):
        _lib.locate_crp(C)


def test_locate_crp_rejects_more_than_16_bits():
    with pytest.raises(_lib.AcossHipError):
        _lib.locate_crp(np.zeros((65536, 3), np.uint8))
    with pytest.raises(_lib.AcossHipError):
        _lib.locate_crp(np.zeros((3, 65536), np.uint8))


def _check_batch(tracks, pairs):
    feats, off, lens = synthetic.pack(tracks)
    q, _, k = oracle.crp_batch(feats, off, lens, pairs, dmax=False)
    P = _lib.crp_params()
    got = _lib.crp_locate(feats, off, lens, int(lens.max()), pairs, P)
    ship = _lib.crp_align(feats, off, lens, int(lens.max()), pairs, P, qmax=True, oti=True)
    qmax, oti, seg = got["qmax"].cpu().numpy(), got["oti"].cpu().numpy(), got["seg"].cpu().numpy()
    np.testing.assert_array_equal(oti, k)
    np.testing.assert_array_equal(oti, ship["oti"].cpu().numpy())
    np.testing.assert_array_equal(qmax, q)
    np.testing.assert_array_equal(qmax, ship["qmax"].cpu().numpy())
    want = np.array([qt.qmax_trace(oracle.crp_pair(tracks[a], tracks[b])["crp"])[1] for a, b in pairs], np.int32)
    np.testing.assert_array_equal(seg, want)
    return seg


@pytest.fixture(scope="module")
def covers24():
    tracks, _ = synthetic.make_corpus("covers80", frames=300, seed=7)
    tracks = tracks[:24]
    pairs = np.array([(i, j) for i in range(24) for j in range(i + 1, 24)], np.int32)
    return tracks, pairs


def test_crp_locate_batch(covers24):
    tracks, pairs = covers24
    seg = _check_batch(tracks, pairs)
    assert (seg[:, 0] >= 0).any()


def test_crp_locate_small_dp_batches(covers24, monkeypatch):
    """DP batches of 7 pairs (40 launches, the last of 3 pairs) give what one batch gives: the
    boundary records are reused and the outputs offset per batch."""
    tracks, pairs = covers24
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    one = _lib.crp_locate(feats, off, lens, int(lens.max()), pairs, P)
    monkeypatch.setenv("ACOSS_BATCH_PAIRS", "7")
    many = _lib.crp_locate(feats, off, lens, int(lens.max()), pairs, P)
    for key in ("qmax", "seg", "oti"):
        np.testing.assert_array_equal(many[key].cpu().numpy(), one[key].cpu().numpy(), err_msg=key)
    assert (one["seg"].cpu().numpy() != -1).any()


def test_crp_locate_ragged_batch():
    """Lengths 37 .. 1100 in one launch: both rows-per-lane kernels (CRPs of at most 512 rows and
    longer ones), two bands at 16 rows per lane, mixed dims, and silences (huge tie groups)."""
    rng = np.random.Generator(np.random.PCG64(99))
    tracks = []
    for n in [37, 120, 400, 700, 1100]:
        x = synthetic.render(rng, synthetic.base_sequence(rng, n))
        if n >= 700:
            x[50:300] = 0.0
        tracks.append(x)
    pairs = np.array([(i, j) for i in range(len(tracks)) for j in range(len(tracks)) if i != j], np.int32)
    _check_batch(tracks, pairs)


def test_plugin_localize(tmp_path, monkeypatch):
    from oracle import np_oracle as npo
    from acoss.algorithms.rqa_serra09 import Serra09
    from acoss.engine import segment_frames
    monkeypatch.chdir(tmp_path)
    tracks, labels = synthetic.make_corpus("covers80", frames=2390, seed=11)
    keep = np.flatnonzero(labels < 4)
    tracks, labels = [tracks[k] for k in keep], labels[keep]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), tracks, labels)
    algo = Serra09(csv, fdir, shortname="t", cachedir=str(tmp_path / "cache"))
    n = len(tracks)
    idxs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    loc = algo.localize(idxs)
    ds = [npo.median_downsample(t, 40) for t in tracks]
    feats, off, lens = synthetic.pack(ds)
    ref = _lib.crp_locate(feats, off, lens, int(lens.max()), idxs, _lib.crp_params())
    np.testing.assert_array_equal(loc["cells"], ref["seg"].cpu().numpy())
    np.testing.assert_array_equal(loc["oti"], ref["oti"].cpu().numpy())
    np.testing.assert_array_equal(loc["qmax"], algo._score(idxs)["qmax"])
    nf = np.array([len(t) for t in tracks])
    qf, rf = segment_frames(loc["cells"], 9, 1, 40, nf[idxs[:, 0]], nf[idxs[:, 1]])
    np.testing.assert_array_equal(loc["query_frames"], qf)
    np.testing.assert_array_equal(loc["reference_frames"], rf)
    found = loc["cells"][:, 0] >= 0
    assert found.any()
    assert (loc["query_frames"][found, 1] <= nf[idxs[found, 0]]).all()
    assert (loc["query_frames"][found, 0] < loc["query_frames"][found, 1]).all()
