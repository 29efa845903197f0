"""GPU tests of the Qmax alignment path (acoss_path_crp / acoss_crp_path, crp_dp.hip k_crp_dp_dir and
k_crp_backtrack) against the numpy restatement tests/qmax_path_np.py: lengths and cells compare
with `==`, the score with the shipped DP's and the segment with the tracing DP's."""
import numpy as np
import pytest

import oracle
import qmax_path_np as qp
import qmax_trace_np as qt
from qmax_trace_np import GAMMAS, SEEDS, SHAPES
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_path_crp_matches_restatement(shape):
    """Degenerate shapes, dense tie-rich matrices (the predecessor order decides paths there while
    the ends stay, see test_path_host.py) and sparse ones with a planted run across rows 32 / 64,
    512, 1024 and 2048: every lane, strip and band edge of both rows-per-lane choices lies on a path."""
    M, N, density, run = shape
    for seed in SEEDS:
        for go, ge in GAMMAS:
            C, score, path = qp.expected_path(M, N, density, run, seed, go, ge)
            s, g, cells = _lib.path_crp(C, go, ge)
            got_s, got_g, got = float(s.item()), g.cpu().numpy().tolist(), cells.cpu().numpy()
            print("%dx%d seed %d gamma (%g, %g): score %r seg %r, %d cells; restatement %r, %d cells"
                  % (M, N, seed, go, ge, got_s, got_g, len(got), score, len(path)))
            assert len(got) == len(path), (seed, go, ge)
            assert got.tolist() == path.tolist(), (seed, go, ge)
            assert got_s == float(_lib.align_crp(C, 0, go, ge).item()), (seed, go, ge)
            assert got_g == _lib.locate_crp(C, go, ge)[1].cpu().numpy().tolist(), (seed, go, ge)


def test_path_crp_rejects_nonbinary():
    C = np.zeros((10, 10), np.uint8)
    C[3, 4] = 2
    with pytest.raises(_lib.AcossHipError):
        _lib.path_crp(C)


def test_path_crp_rejects_more_than_16_bits():
    with pytest.raises(_lib.AcossHipError):
        _lib.path_crp(np.zeros((65536, 3), np.uint8))
    with pytest.raises(_lib.AcossHipError):
        _lib.path_crp(np.zeros((3, 65536), np.uint8))


def test_path_crp_rejects_a_short_path_cap():
    C = np.zeros((12, 9), np.uint8)
    _lib.path_crp(C, path_cap=9)
    with pytest.raises(_lib.AcossHipError):
        _lib.path_crp(C, path_cap=8)


def test_given_matrix_entries_agree():
    """align_crp, locate_crp and path_crp pack and check a matrix the same way: one score, one
    segment, all three refuse an element above 1, and an empty matrix scores 0 with no segment and
    no path."""
    rng = np.random.Generator(np.random.PCG64(0))
    C = (rng.random((40, 33)) < 0.3).astype(np.uint8)
    score, seg = qt.qmax_trace(C)
    assert score > 0
    a = float(_lib.align_crp(C, 0).item())
    ls, lg = _lib.locate_crp(C)
    ps, pg, cells = _lib.path_crp(C)
    assert a == float(ls.item()) == float(ps.item()) == score
    assert lg.cpu().numpy().tolist() == pg.cpu().numpy().tolist() == list(seg)
    assert cells.cpu().numpy()[0].tolist() == list(seg[:2]) and cells.cpu().numpy()[-1].tolist() == list(seg[2:])
    bad = C.copy()
    bad[17, 5] = 2
    for fn in (_lib.align_crp, _lib.locate_crp, _lib.path_crp):
        with pytest.raises(_lib.AcossHipError):
            fn(bad)
    for shape in ((0, 33), (40, 0)):
        E = np.zeros(shape, np.uint8)
        assert float(_lib.align_crp(E, 0).item()) == 0.0
        ls, lg = _lib.locate_crp(E)
        ps, pg, cells = _lib.path_crp(E)
        assert float(ls.item()) == 0.0 and float(ps.item()) == 0.0
        assert lg.cpu().numpy().tolist() == pg.cpu().numpy().tolist() == [-1, -1, -1, -1]
        assert tuple(cells.shape) == (0, 2)


def _paths(got):
    off = got["path_off"].cpu().numpy()
    cells = got["cells"].cpu().numpy()
    assert off.dtype == np.int64 and off[0] == 0 and off[-1] == len(cells)
    return [cells[off[p]:off[p + 1]] for p in range(len(off) - 1)]


_CRPS = {}


def _want_paths(name, tracks, pairs):
    """The restatement on the oracle's CRP of every pair, once per pair list."""
    if name not in _CRPS:
        _CRPS[name] = [qp.qmax_path(oracle.crp_pair(tracks[a], tracks[b])["crp"])[1] for a, b in pairs]
    return _CRPS[name]


def _check_batch(name, tracks, pairs):
    feats, off, lens = synthetic.pack(tracks)
    q, _, k = oracle.crp_batch(feats, off, lens, pairs, dmax=False)
    P = _lib.crp_params()
    got = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P)
    ship = _lib.crp_align(feats, off, lens, int(lens.max()), pairs, P, qmax=True, oti=True)
    loc = _lib.crp_locate(feats, off, lens, int(lens.max()), pairs, P)
    qmax, oti, seg = got["qmax"].cpu().numpy(), got["oti"].cpu().numpy(), got["seg"].cpu().numpy()
    np.testing.assert_array_equal(oti, k)
    np.testing.assert_array_equal(oti, ship["oti"].cpu().numpy())
    np.testing.assert_array_equal(qmax, q)
    np.testing.assert_array_equal(qmax, ship["qmax"].cpu().numpy())
    np.testing.assert_array_equal(seg, loc["seg"].cpu().numpy())
    paths = _paths(got)
    want = _want_paths(name, tracks, pairs)
    for p, (g, w) in enumerate(zip(paths, want)):
        assert g.tolist() == w.tolist(), (p, pairs[p].tolist())
    return got, paths


@pytest.fixture(scope="module")
def covers24():
    tracks, _ = synthetic.make_corpus("covers80", frames=300, seed=7)
    tracks = tracks[:24]
    pairs = np.array([(i, j) for i in range(24) for j in range(i + 1, 24)], np.int32)
    return tracks, pairs


def test_crp_path_batch(covers24):
    tracks, pairs = covers24
    _, paths = _check_batch("covers24", tracks, pairs)
    assert sum(len(p) > 0 for p in paths) > 0


def test_crp_path_ragged_batch():
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
    _check_batch("ragged", tracks, pairs)


def test_crp_path_small_dp_batches(covers24, monkeypatch):
    """DP batches of 7 pairs (40 launches, the last of 3 pairs) give what one batch gives: the plane,
    the end keys and the outputs are offset per batch."""
    tracks, pairs = covers24
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    one = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P)
    monkeypatch.setenv("ACOSS_BATCH_PAIRS", "7")
    many = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P)
    for key in ("qmax", "seg", "oti", "path_off", "cells"):
        np.testing.assert_array_equal(many[key].cpu().numpy(), one[key].cpu().numpy(), err_msg=key)
    assert int(one["path_off"][-1]) > 0


def test_crp_path_under_a_plane_budget(covers24, monkeypatch):
    """A plane budget below the batch's planes splits it into DP batches of equal size. 300 frames
    stack to L = 291 rows of pitch 296, so a plane is ceil(291 / 16) * 296 * 4 = 22,496 B, 22,528 B
    aligned to 256; 1,200,000 B hold 53 of them, 276 pairs need ceil(276 / 53) = 6 batches, and six
    equal ones have ceil(276 / 6) = 46 pairs: neither one batch nor one pair per batch."""
    tracks, pairs = covers24
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    one = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P)
    monkeypatch.setenv("ACOSS_PATH_BYTES", "1200000")
    many = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P)
    for key in ("qmax", "seg", "oti", "path_off", "cells"):
        np.testing.assert_array_equal(many[key].cpu().numpy(), one[key].cpu().numpy(), err_msg=key)
    assert int(one["path_off"][-1]) > 0


def test_plugin_align_path(tmp_path, monkeypatch):
    from acoss.algorithms.rqa_serra09 import Serra09
    from acoss.engine import path_frames
    monkeypatch.chdir(tmp_path)
    tracks, labels = synthetic.make_corpus("covers80", frames=2390, seed=11)
    keep = np.flatnonzero(labels < 4)
    tracks, labels = [tracks[k] for k in keep], labels[keep]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), tracks, labels)
    algo = Serra09(csv, fdir, shortname="t", cachedir=str(tmp_path / "cache"))
    n = len(tracks)
    idxs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    al = algo.align_path(idxs)
    loc = algo.localize(idxs)
    np.testing.assert_array_equal(al["cells"], loc["cells"])
    np.testing.assert_array_equal(al["qmax"], loc["qmax"])
    np.testing.assert_array_equal(al["oti"], loc["oti"])
    off, pc = al["path_off"], al["path_cells"]
    assert off.shape == (len(idxs) + 1,) and off[0] == 0 and off[-1] == len(pc)
    found = 0
    for p in range(len(idxs)):
        path = pc[off[p]:off[p + 1]]
        if al["cells"][p, 0] < 0:
            assert len(path) == 0
            continue
        found += 1
        assert path[0].tolist() == al["cells"][p, :2].tolist() and path[-1].tolist() == al["cells"][p, 2:].tolist()
        assert {tuple(d) for d in np.diff(path, axis=0).tolist()} <= {(1, 1), (2, 1), (1, 2)}
    assert found > 0
    assert al["path_frames"].dtype == np.int64
    np.testing.assert_array_equal(al["path_frames"], path_frames(pc, 1, 40))
