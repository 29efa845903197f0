"""GPU tests of the plugin layer of the OTI-binary CRP: coverid.benchmark(binarize="oti") for Serra09
and LateFusionChen against the restatement tests/otib_np.py on the downsampled features with the
existing finish applied, the per-pair methods against the batch entries, and the default
binarisation's names and scores. The Serra09 dataset has 8 tracks of 4,000 .. 6,000 raw frames;
LateFusionChen's has 24 of them, because its late fusion (SNF, K = 20) takes K + 1 neighbours per
song and so needs more than 21 songs."""
import os

import numpy as np
import pytest

import oracle
import otib_np
from oracle import np_oracle as npo
from acoss import _lib, coverid, synthetic
from acoss.algorithms.rqa_serra09 import Serra09

pytestmark = pytest.mark.gpu


def _dataset(root, n_tracks):
    """n_tracks songs and covers of the hard corpus (covers rolled on the chroma axis), 4,000 .. 6,000
    frames each, on disk; and per (rank, i < j) the restated Qmax and dmax on the downsampled features."""
    tracks, labels = synthetic.make_hard_corpus("covers80", frames=4800, seed=9, fixed_length=False)
    keep = [k for k in range(len(tracks)) if 4000 <= len(tracks[k]) <= 6000][:n_tracks]
    assert len(keep) == n_tracks
    tracks, labels = [tracks[k] for k in keep], labels[keep]
    assert len(set(labels.tolist())) < n_tracks        # at least one clique of two
    csv, fdir = synthetic.write_feature_dataset(str(root), tracks, labels)
    ds = [npo.median_downsample(t, 40) for t in tracks]
    return {"csv": csv, "fdir": fdir, "n": n_tracks, "ds": ds, "lens": np.array([len(d) for d in ds], np.int64)}


def _restated_scores(ds, rank):
    """(Q, D) symmetric (n, n) float32 of the restated Qmax and dmax, the diagonal 0."""
    n = len(ds)
    Q, D = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
    for i in range(n):
        for j in range(i + 1, n):
            C = otib_np.otib(ds[i], ds[j], 9, 1, True, rank)["crp"]
            dens = otib_np.density(C)
            assert 0.01 <= dens <= 0.90, (i, j, dens)
            Q[i, j] = Q[j, i] = oracle.align(C, 0.5, 0.5, 0)
            D[i, j] = D[j, i] = oracle.align(C, 0.5, 0.5, 1)
    return Q, D


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = _dataset(tmp_path_factory.mktemp("otib_plugin8"), 8)
    n = d["n"]
    d["idxs"] = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    d["packed"] = synthetic.pack(d["ds"])
    return d


def _bank_args(d):
    feats, off, lens = d["packed"]
    return feats, off, lens, int(lens.max()), d["idxs"]


def test_benchmark_serra09_otib(small, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for rank, name in ((1, "Serra09-otib"), (2, "Serra09-otib2")):
        algo = coverid.benchmark(small["csv"], small["fdir"], algorithm="Serra09", shortname="t",
                                 cachedir=str(tmp_path / "cache"), binarize="oti", oti_rank=rank)
        assert algo.name == name
        assert os.path.exists("results_t_%s.csv" % name) and not os.path.exists("results_t_Serra09.csv")
        assert os.path.exists(str(tmp_path / "cache" / ("%s_t_Ds.npz" % name)))
        Q, _ = _restated_scores(small["ds"], rank)
        want = (Q / np.sqrt(small["lens"].astype(np.float64))[None, :]).astype(np.float32)
        np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), want)
        assert Q.any()


def test_benchmark_chen_otib(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    d = _dataset(tmp_path / "data", 24)
    algo = coverid.benchmark(d["csv"], d["fdir"], algorithm="LateFusionChen", shortname="t",
                             cachedir=str(tmp_path / "cache"), binarize="oti")
    assert algo.name == "LateFusionChen-otib"
    assert os.path.exists("results_t_LateFusionChen-otib.csv")
    Q, D = _restated_scores(d["ds"], 1)
    norm = np.sqrt(d["lens"].astype(np.float64))[None, :]
    with np.errstate(divide="ignore"):      # the finish: sqrt(n_j) / score, then the late fusion's sign flip
        np.testing.assert_array_equal(np.asarray(algo.Ds["qmax"]), -(norm / Q).astype(np.float32))
        np.testing.assert_array_equal(np.asarray(algo.Ds["dmax"]), -(norm / D).astype(np.float32))
    assert set(algo.Ds) == {"qmax", "dmax", "Late"} and np.isfinite(np.asarray(algo.Ds["Late"])).all()
    assert Q.any() and D.any() and (Q != D).any()


def test_per_pair_methods_agree_with_the_batch_entries(small, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    P = _lib.crp_params(binarize="oti", oti_rank=2)
    idxs = small["idxs"]
    algo = Serra09(small["csv"], small["fdir"], shortname="t", cachedir=str(tmp_path / "cache"), binarize="oti",
                   oti_rank=2)
    for alignment, align in (("qmax", 0), ("dmax", 1)):
        ref = {k: v.cpu().numpy() for k, v in _lib.crp_locate(*_bank_args(small), P, align=align).items()}
        got = algo.localize(idxs, alignment=alignment)
        np.testing.assert_array_equal(got[alignment], ref[alignment])
        np.testing.assert_array_equal(got["cells"], ref["seg"])
        np.testing.assert_array_equal(got["oti"], ref["oti"])
        pref = {k: v.cpu().numpy() for k, v in _lib.crp_path(*_bank_args(small), P, align=align).items()}
        path = algo.align_path(idxs, alignment=alignment)
        np.testing.assert_array_equal(path["path_cells"], pref["cells"])
        np.testing.assert_array_equal(path["path_off"], pref["path_off"])
        assert len(pref["cells"])
    L = _lib.stacked_len(int(small["packed"][2].max()))
    ref = {k: v.cpu().numpy() for k, v in _lib.crp_rqa(*_bank_args(small), P, lmin=2, hist_cap=L + 1).items()}
    got = algo.rqa(idxs, lmin=2, hist=True)
    for c, k in enumerate(_lib.RQA_STATS):
        np.testing.assert_array_equal(got[k], ref["stats"][:, c], err_msg=k)
    for c, k in enumerate(_lib.RQA_COUNTS):
        np.testing.assert_array_equal(got[k], ref["counts"][:, c], err_msg=k)
    for k in ("lmax", "smax", "oti", "hist"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    # and the batch entry's mask is the restated one: n_rec of a pair is its count of ones
    a, b = idxs[3]
    assert got["n_rec"][3] == int(otib_np.otib(small["ds"][a], small["ds"][b], 9, 1, True, 2)["crp"].sum())


def test_measure_on_the_otib_mask(small, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = Serra09(small["csv"], small["fdir"], shortname="t", cachedir=str(tmp_path / "cache"), measure="smax",
                   binarize="oti", oti_rank=2)
    assert algo.name == "Serra09-otib2-smax"
    algo.similarity(small["idxs"][:12])
    ref = _lib.crp_rqa(*_bank_args(small)[:4], small["idxs"][:12], _lib.crp_params(binarize="oti", oti_rank=2),
                       lines=False)["smax"].cpu().numpy()
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"])[small["idxs"][:12, 0], small["idxs"][:12, 1]], ref)
    assert ref.any()


def test_default_binarize_writes_todays_names_and_scores(small, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = coverid.benchmark(small["csv"], small["fdir"], algorithm="Serra09", shortname="t",
                             cachedir=str(tmp_path / "cache"))
    assert algo.name == "Serra09" and algo.binarize == "percentile"
    assert os.path.exists("results_t_Serra09.csv") and os.path.exists(str(tmp_path / "cache" / "Serra09_t_Ds.npz"))
    feats, off, lens = small["packed"]
    q, _, _ = oracle.crp_batch(feats, off, lens, small["idxs"], dmax=False)
    n, idxs = small["n"], small["idxs"]
    Q = np.zeros((n, n), np.float32)
    up = idxs[:, 0] < idxs[:, 1]
    Q[idxs[up, 0], idxs[up, 1]] = q[up]
    Q = Q + Q.T
    want = (Q / np.sqrt(small["lens"].astype(np.float64))[None, :]).astype(np.float32)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), want)
