"""CPU tests of the cross-recurrence quantification's restatement (tests/rqa_np.py) and of the host
side of Serra09's `measure` (no GPU): the vectorised histogram against the cell-by-cell one, the
identities of the definition, hand-worked answers, and that the planted cases of the GPU tests
cannot pass vacuously."""
import math

import numpy as np
import pytest

import qmax_trace_np as qt
import rqa_np
from rqa_np import CASES, LMINS, SMALL


@pytest.mark.parametrize("name", list(CASES))
def test_identities(name):
    C = rqa_np.matrix(name)
    M, N = C.shape
    for lmin in LMINS:
        e = rqa_np.expected(name, lmin)
        H = e["hist"]
        ls = np.arange(len(H))
        assert len(H) == min(M, N) + 1 and H[0] == 0
        assert int((ls * H).sum()) == e["n_rec"] == int(C.sum())
        assert e["n_lines"] == int(H.sum())
        assert e["n_lines_min"] == int(H[lmin:].sum()) <= e["n_lines"]
        assert e["n_pts_min"] <= e["n_rec"]
        assert e["rr"] == e["n_rec"] / (M * N)
        assert 0.0 <= e["det"] <= 1.0 and e["entr"] >= 0.0
        if lmin == 1:
            assert e["n_lines_min"] == e["n_lines"] and e["n_pts_min"] == e["n_rec"]
            assert e["det"] == (1.0 if e["n_rec"] else 0.0)
        assert e["smax"] == qt.qmax_trace(C, np.inf, np.inf)[0]
        assert e["smax"] <= e["n_rec"] and (e["smax"] == 0 or e["smax"] <= min(M, N) - 2)


@pytest.mark.parametrize("name", SMALL)
def test_vectorised_against_cells(name):
    C = rqa_np.matrix(name)
    np.testing.assert_array_equal(rqa_np.line_hist(C), rqa_np.line_hist_cells(C))
    assert rqa_np.smax(C) == rqa_np.smax_cells(C)


@pytest.mark.parametrize("shape", [s for s in qt.SHAPES if s[0] * s[1] <= 40 * 300], ids=lambda s: "%dx%d" % s[:2])
def test_smax_is_qmax_at_infinite_gamma(shape):
    M, N, density, run = shape
    for seed in qt.SEEDS:
        C = qt.make_matrix(M, N, density, run, seed)
        assert qt.qmax_trace(C, np.inf, np.inf)[0] == rqa_np.smax_cells(C)
        np.testing.assert_array_equal(rqa_np.line_hist(C), rqa_np.line_hist_cells(C))


def test_hand_worked():
    # 70 x 45 of ones: every diagonal is one line; 2 of each length 1..44, 70 - 45 + 1 = 26 of length 45
    e = rqa_np.expected("ones_70x45", 2)
    want = np.zeros(46, np.int64)
    want[1:45] = 2
    want[45] = 26
    np.testing.assert_array_equal(e["hist"], want)
    assert (e["n_rec"], e["n_lines"], e["n_lines_min"], e["n_pts_min"], e["lmax"]) == (3150, 114, 112, 3148, 45)
    assert e["rr"] == 1.0 and e["det"] == 3148 / 3150 and e["lmean"] == 3148 / 112
    p2, p26 = 2 / 112, 26 / 112
    assert e["entr"] == pytest.approx(-(43 * p2 * math.log(p2) + p26 * math.log(p26)), rel=1e-12)
    assert e["smax"] == 43.0  # the main diagonal from (2, 2) to (44, 44)
    # nothing set
    e = rqa_np.expected("zeros_70x45", 2)
    assert not e["hist"].any()
    assert all(e[k] == 0 for k in rqa_np.COUNT_KEYS + rqa_np.STAT_KEYS + ("lmax", "smax"))
    # one cell
    e = rqa_np.expected("1x1", 1)
    assert (e["n_rec"], e["n_lines"], e["lmax"], e["rr"], e["det"], e["lmean"], e["entr"], e["smax"]) == \
        (1, 1, 1, 1.0, 1.0, 1.0, 0.0, 0.0)
    assert rqa_np.expected("1x1", 2)["n_lines_min"] == 0 and rqa_np.expected("1x1", 2)["det"] == 0.0
    # a small one by hand: the main diagonal is one line of 4, (0,2) a line of 1 ((1,3) is unset),
    # (2,0)-(3,1) a line of 2
    C = np.array([[1, 0, 1, 0],
                  [0, 1, 0, 0],
                  [1, 0, 1, 0],
                  [0, 1, 0, 1]], np.uint8)
    np.testing.assert_array_equal(rqa_np.line_hist(C), [0, 1, 1, 0, 1])
    r = rqa_np.rqa(C, 2)
    assert (r["n_rec"], r["n_lines"], r["n_lines_min"], r["n_pts_min"], r["lmax"]) == (7, 3, 2, 6, 4)
    assert r["lmean"] == 3.0 and r["det"] == 6 / 7 and r["rr"] == 7 / 16
    assert r["entr"] == pytest.approx(math.log(2.0), rel=1e-12)
    assert r["smax"] == 2.0  # (2,2) -> (3,3); rows and columns 0 and 1 hold 0


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][1] is not None])
def test_planted_cases_are_not_vacuous(name):
    e = rqa_np.expected(name, 2)
    assert e["lmax"] >= CASES[name][1]
    assert np.count_nonzero(e["hist"]) >= 4
    assert e["n_lines_min"] > 0
    assert rqa_np.expected(name, 5)["n_lines_min"] > 0


def test_lanes_full_cases_have_hits_in_the_last_row():
    for name in ("lanes_512x40", "lanes_1024x40", "lanes_2048x40"):
        C = rqa_np.matrix(name)
        assert C.shape[0] in (512, 1024, 2048) and C[-1].sum() >= 20 and C[-1, -1] == 1


def test_serra09_measure_names_and_validation(tmp_path, monkeypatch):
    from acoss import coverid, synthetic
    from acoss.algorithms.rqa_serra09 import Serra09
    assert Serra09.MEASURES == ("qmax", "smax", "lmax", "det", "lmean", "entr", "rr")
    assert Serra09.algorithm_name() == Serra09.algorithm_name("qmax") == "Serra09"
    for m in Serra09.MEASURES[1:]:
        assert Serra09.algorithm_name(m) == "Serra09-" + m
    with pytest.raises(ValueError):
        Serra09.algorithm_name("laminarity")
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    tracks = [rng.random((50, 12)).astype(np.float32) for _ in range(4)]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), tracks, [0, 0, 1, 1])
    kw = dict(dataset_csv=csv, datapath=fdir, shortname="t", cachedir=str(tmp_path / "cache"))
    a, b = Serra09(**kw), Serra09(measure="lmax", lmin=3, **kw)
    assert (a.name, a.measure, a.lmin) == ("Serra09", "qmax", 2)
    assert (b.name, b.measure, b.lmin) == ("Serra09-lmax", "lmax", 3)
    assert a.get_cacheprefix() != b.get_cacheprefix()
    assert a._dmat_path("main") != b._dmat_path("main")
    with pytest.raises(ValueError):
        Serra09(measure="Qmax", **kw)
    with pytest.raises(ValueError):
        Serra09(measure="det", lmin=0, **kw)
    with pytest.raises(ValueError):
        coverid.benchmark(csv, fdir, algorithm="SiMPle", shortname="t", cachedir=str(tmp_path / "cache"),
                          measure="smax")
