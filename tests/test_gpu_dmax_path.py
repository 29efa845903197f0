"""GPU tests of the located and traced dmax (chen17) alignment (acoss_locate_crp_dmax /
acoss_path_crp_dmax / acoss_crp_locate_dmax / acoss_crp_path_dmax: crp_dp.hip k_crp_dp_trace<1>,
k_crp_dp_dir<1> and k_crp_backtrack_dmax) against the numpy restatement tests/dmax_path_np.py:
cells, lengths and segments compare with `==`, the score with the shipped chen17 DP's."""
import numpy as np
import pytest

import dmax_path_np as dp
import oracle
from dmax_path_np import GAMMAS, SEEDS, SHAPES, STAIRS
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu


def _check_matrix(C, go, ge, score, path, seg, tag):
    s, g, cells = _lib.path_crp(C, go, ge, align=1)
    ls, lg = _lib.locate_crp(C, go, ge, align=1)
    got_s, got_g, got = float(s.item()), g.cpu().numpy().tolist(), cells.cpu().numpy()
    print("%s: score %r seg %r, %d cells; restatement %r seg %r, %d cells"
          % (tag, got_s, got_g, len(got), score, seg, len(path)))
    assert len(got) == len(path), tag
    assert got.tolist() == path.tolist(), tag
    assert got_g == list(seg), tag
    assert lg.cpu().numpy().tolist() == list(seg), tag
    if len(got):
        assert got_g == got[0].tolist() + got[-1].tolist(), tag
    assert got_s == score, tag
    assert got_s == float(ls.item()) == float(_lib.align_crp(C, 1, go, ge).item()), tag


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_path_and_locate_match_restatement(shape):
    """Degenerate shapes, dense tie-rich matrices (where the predecessor order decides the path) and
    sparse ones with a planted run across rows 32 / 64, 512, 1024 and 2048, at every gamma pair."""
    M, N, density, run = shape
    for seed in SEEDS:
        for go, ge in GAMMAS:
            C, score, path, seg = dp.expected_path(M, N, density, run, seed, go, ge)
            _check_matrix(C, go, ge, score, path, seg, "%dx%d seed %d gamma (%g, %g)" % (M, N, seed, go, ge))


@pytest.mark.parametrize("case", STAIRS, ids=lambda c: "%dx%d" % c[:2])
def test_staircases_across_lane_strip_and_band_edges(case):
    """b / c staircases through rows 32 / 64, 512, 1024 and 2048: a step's predecessor, its
    intermediate and its cell fall on either side of a lane, strip or band edge, so the bonus bit and
    the intermediate's key come from the lane or band above."""
    C, score, path, seg = dp.expected_stairs(*case)
    short = sum(tuple(d) in ((1, 0), (0, 1)) for d in np.diff(path, axis=0).tolist())
    assert short >= 20, "the planted staircase is on the path"
    _check_matrix(C, 0.5, 0.5, score, path, seg, "stairs %dx%d" % case[:2])


def test_path_longer_than_the_shorter_side():
    """49 cells on 40 x 40; one more hit in row 1 and the path begins there."""
    C = dp.make_staircase(40, 40, (2, 2), "bc")
    C[1, 2] = 1
    score, path, seg = dp.dmax_path(C)
    assert len(path) == 50 and seg[:2] == (1, 2)
    _check_matrix(C, 0.5, 0.5, score, path, seg, "staircase 40x40")


def test_rejects_a_short_path_cap_nonbinary_and_more_than_16_bits():
    C = np.zeros((12, 9), np.uint8)
    bound = dp.path_bound(12, 9)
    assert bound == 12 == _lib.dmax_path_bound(12, 9)
    _lib.path_crp(C, path_cap=bound, align=1)
    with pytest.raises(_lib.AcossHipError, match="12"):
        _lib.path_crp(C, path_cap=bound - 1, align=1)
    bad = C.copy()
    bad[3, 4] = 2
    for fn in (_lib.locate_crp, _lib.path_crp):
        with pytest.raises(_lib.AcossHipError):
            fn(bad, align=1)
        with pytest.raises(_lib.AcossHipError):
            fn(np.zeros((65536, 3), np.uint8), align=1)
    for shape in ((0, 33), (40, 0), (2, 9)):
        E = np.ones(shape, np.uint8)
        ls, lg = _lib.locate_crp(E, align=1)
        ps, pg, cells = _lib.path_crp(E, align=1)
        assert float(ls.item()) == 0.0 and float(ps.item()) == 0.0
        assert lg.cpu().numpy().tolist() == pg.cpu().numpy().tolist() == [-1, -1, -1, -1]
        assert tuple(cells.shape) == (0, 2)
    with pytest.raises(ValueError):
        _lib.path_crp(C, align=2)


def test_qmax_results_unchanged_next_to_dmax():
    """align=0 is the default and gives the same tensors before and after an align=1 call on the same
    workspace, on one matrix and one batch."""
    rng = np.random.Generator(np.random.PCG64(0))
    C = (rng.random((40, 33)) < 0.3).astype(np.uint8)
    before = [t.cpu().numpy() for t in _lib.path_crp(C)]
    d = _lib.path_crp(C, align=1)
    after = [t.cpu().numpy() for t in _lib.path_crp(C, align=0)]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert float(d[0].item()) == oracle.align(C, which=1) != float(before[0].item())
    tracks, _ = synthetic.make_corpus("covers80", frames=300, seed=7)
    feats, off, lens = synthetic.pack(tracks[:6])
    pairs = np.array([(i, j) for i in range(6) for j in range(i + 1, 6)], np.int32)
    P = _lib.crp_params()
    one = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P)
    dm = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P, align=1)
    two = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, P, align=0)
    assert sorted(one) == sorted(two) == ["cells", "oti", "path_off", "qmax", "seg"]
    assert sorted(dm) == ["cells", "dmax", "oti", "path_off", "seg"]
    for key in one:
        np.testing.assert_array_equal(one[key].cpu().numpy(), two[key].cpu().numpy(), err_msg=key)
    l0 = _lib.crp_locate(feats, off, lens, int(lens.max()), pairs, P)
    np.testing.assert_array_equal(l0["seg"].cpu().numpy(), one["seg"].cpu().numpy())
    np.testing.assert_array_equal(l0["qmax"].cpu().numpy(), one["qmax"].cpu().numpy())


def _paths(got):
    off = got["path_off"].cpu().numpy()
    cells = got["cells"].cpu().numpy()
    assert off.dtype == np.int64 and off[0] == 0 and off[-1] == len(cells)
    return [cells[off[p]:off[p + 1]] for p in range(len(off) - 1)]


_WANT = {}


def _want_paths(name, tracks, pairs):
    """The restatement on the oracle's CRP of every pair, once per pair list."""
    if name not in _WANT:
        _WANT[name] = [dp.dmax_path(oracle.crp_pair(tracks[a], tracks[b])["crp"]) for a, b in pairs]
    return _WANT[name]


def _check_batch(name, tracks, pairs):
    feats, off, lens = synthetic.pack(tracks)
    _, d, k = oracle.crp_batch(feats, off, lens, pairs, dmax=True)
    P = _lib.crp_params()
    L = int(lens.max())
    got = _lib.crp_path(feats, off, lens, L, pairs, P, align=1)
    ship = _lib.crp_align(feats, off, lens, L, pairs, P, qmax=False, dmax=True, oti=True)
    loc = _lib.crp_locate(feats, off, lens, L, pairs, P, align=1)
    dmax, oti, seg = got["dmax"].cpu().numpy(), got["oti"].cpu().numpy(), got["seg"].cpu().numpy()
    np.testing.assert_array_equal(oti, k)
    np.testing.assert_array_equal(oti, ship["oti"].cpu().numpy())
    np.testing.assert_array_equal(oti, loc["oti"].cpu().numpy())
    np.testing.assert_array_equal(dmax, d)
    np.testing.assert_array_equal(dmax, ship["dmax"].cpu().numpy())
    np.testing.assert_array_equal(dmax, loc["dmax"].cpu().numpy())
    np.testing.assert_array_equal(seg, loc["seg"].cpu().numpy())
    paths = _paths(got)
    for p, (g, (ws, wp, wseg)) in enumerate(zip(paths, _want_paths(name, tracks, pairs))):
        assert g.tolist() == wp.tolist(), (p, pairs[p].tolist())
        assert seg[p].tolist() == list(wseg), (p, pairs[p].tolist())
        assert float(dmax[p]) == ws, (p, pairs[p].tolist())
    return got, paths


@pytest.fixture(scope="module")
def covers24():
    tracks, _ = synthetic.make_corpus("covers80", frames=300, seed=7)
    tracks = tracks[:24]
    pairs = np.array([(i, j) for i in range(24) for j in range(i + 1, 24)], np.int32)
    return tracks, pairs


@pytest.fixture(scope="module")
def covers24_one(covers24):
    """The 276 pairs in one DP batch, checked against the oracle and the restatement: what the
    batch-splitting tests compare with."""
    tracks, pairs = covers24
    got, paths = _check_batch("covers24", tracks, pairs)
    assert sum(len(p) > 0 for p in paths) > 0
    return {key: v.cpu().numpy() for key, v in got.items()}


def test_crp_path_batch(covers24_one):
    assert int(covers24_one["path_off"][-1]) > 0


def test_crp_path_ragged_batch():
    """Lengths 37 .. 1100 in one launch: both rows-per-lane kernels, two bands at 16 rows per lane,
    mixed dims, and silences (huge tie groups): test_gpu_path.py's ragged set."""
    rng = np.random.Generator(np.random.PCG64(99))
    tracks = []
    for n in [37, 120, 400, 700, 1100]:
        x = synthetic.render(rng, synthetic.base_sequence(rng, n))
        if n >= 700:
            x[50:300] = 0.0
        tracks.append(x)
    pairs = np.array([(i, j) for i in range(len(tracks)) for j in range(len(tracks)) if i != j], np.int32)
    _check_batch("ragged", tracks, pairs)


@pytest.mark.parametrize("env,value", [("ACOSS_BATCH_PAIRS", "7"), ("ACOSS_PATH_BYTES", "1200000")])
def test_crp_path_split_batches(covers24, covers24_one, monkeypatch, env, value):
    """DP batches of 7 pairs, and a plane budget that splits the 276 pairs into six batches of 46
    (test_gpu_path.py works the numbers out), give what one batch gives."""
    tracks, pairs = covers24
    feats, off, lens = synthetic.pack(tracks)
    monkeypatch.setenv(env, value)
    many = _lib.crp_path(feats, off, lens, int(lens.max()), pairs, _lib.crp_params(), align=1)
    for key in ("dmax", "seg", "oti", "path_off", "cells"):
        np.testing.assert_array_equal(many[key].cpu().numpy(), covers24_one[key], err_msg=key)


def test_crp_path_rejects_a_short_path_cap(covers24):
    """The C entry refuses a path_cap one below floor(4 L / 3) - 2 at the longest stacked length."""
    import ctypes
    import torch
    tracks, pairs = covers24
    feats, off, lens = synthetic.pack(tracks[:2])
    P = _lib.crp_params()
    keep, n, lead = _lib._bank_args(feats, off, lens, int(lens.max()), pairs[:1], P)
    L = _lib.stacked_len(int(lens.max()))
    bound = _lib.dmax_path_bound(L, L)
    assert bound == 4 * L // 3 - 2
    out = torch.empty((bound, 2), dtype=torch.int32, device="cuda")
    num = torch.empty(1, dtype=torch.int32, device="cuda")
    lib = _lib.load_library()
    args = lambda cap: (*lead, None, None, None, cap, _lib._ptr(num), _lib._ptr(out), _lib._stream())
    assert lib.acoss_crp_path_dmax(*args(bound)) == 0
    assert lib.acoss_crp_path_dmax(*args(bound - 1)) == -1
    assert str(bound) in lib.acoss_last_error().decode()
    del keep


def test_plugin_dmax_align_path(tmp_path, monkeypatch):
    from acoss.algorithms.latefusion_chen import ChenFusion
    from acoss.engine import path_frames
    monkeypatch.chdir(tmp_path)
    tracks, labels = synthetic.make_corpus("covers80", frames=2390, seed=11)
    keep = np.flatnonzero(labels < 4)
    tracks, labels = [tracks[k] for k in keep], labels[keep]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), tracks, labels)
    algo = ChenFusion(csv, fdir, shortname="t", cachedir=str(tmp_path / "cache"))
    n = len(tracks)
    idxs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    al = algo.align_path(idxs, alignment="dmax")
    loc = algo.localize(idxs, "dmax")
    assert "qmax" not in al and "qmax" not in loc
    np.testing.assert_array_equal(al["cells"], loc["cells"])
    np.testing.assert_array_equal(al["dmax"], loc["dmax"])
    np.testing.assert_array_equal(al["dmax"], algo._score(idxs, dmax=True)["dmax"])
    np.testing.assert_array_equal(al["oti"], loc["oti"])
    off, pc = al["path_off"], al["path_cells"]
    assert off.shape == (len(idxs) + 1,) and off[0] == 0 and off[-1] == len(pc)
    found = 0
    for p in range(len(idxs)):
        path = pc[off[p]:off[p + 1]]
        if al["cells"][p, 0] < 0:
            assert len(path) == 0 and al["dmax"][p] == 0
            assert loc["query_frames"][p].tolist() == [-1, -1]
            continue
        found += 1
        assert path[0].tolist() == al["cells"][p, :2].tolist() and path[-1].tolist() == al["cells"][p, 2:].tolist()
        assert {tuple(d) for d in np.diff(path, axis=0).tolist()} <= dp.STEPS
        assert loc["query_frames"][p, 0] == al["cells"][p, 0] * 40
    assert found > 0
    assert al["path_frames"].dtype == np.int64
    np.testing.assert_array_equal(al["path_frames"], path_frames(pc, 1, 40))
    none = algo.align_path(np.zeros((0, 2), np.int32), alignment="dmax")
    assert none["dmax"].shape == (0,) and none["path_off"].tolist() == [0] and none["path_cells"].shape == (0, 2)
    # the default is the Qmax alignment, as before
    q = algo.align_path(idxs[:3])
    assert "qmax" in q and "dmax" not in q
    with pytest.raises(ValueError):
        algo.align_path(idxs[:3], alignment="chen17")
