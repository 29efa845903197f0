"""GPU tests of the plugin layer of the cross-recurrence quantification: ChromaBackedAlgorithm.rqa,
Serra09(measure=...) through all_pairwise / normalize_by_length, and coverid.benchmark(measure=...)."""
import os

import numpy as np
import pytest

from oracle import np_oracle as npo
from acoss import _lib, synthetic
from acoss.algorithms.rqa_serra09 import Serra09

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("rqa_plugin")
    tracks, labels = synthetic.make_corpus("covers80", frames=2390, seed=11)
    keep = np.flatnonzero(labels < 6)
    tracks, labels = [tracks[k] for k in keep], labels[keep]
    csv, fdir = synthetic.write_feature_dataset(str(root), tracks, labels)
    ds = [npo.median_downsample(t, 40) for t in tracks]
    n = len(tracks)
    assert 8 <= n <= 16
    idxs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    feats, off, lens = synthetic.pack(ds)
    L = _lib.stacked_len(int(lens.max()))
    ref = {k: v.cpu().numpy() for k, v in
           _lib.crp_rqa(feats, off, lens, int(lens.max()), idxs, _lib.crp_params(), lmin=2, hist_cap=L + 1).items()}
    return {"csv": csv, "fdir": fdir, "n": n, "idxs": idxs, "lens": lens, "ref": ref, "packed": (feats, off, lens)}


def _algo(dataset, tmp_path, **kw):
    return Serra09(dataset["csv"], dataset["fdir"], shortname="t", cachedir=str(tmp_path / "cache"), **kw)


def _matrix(n, idxs, v, symmetric):
    D = np.zeros((n, n), np.float32)
    keep = idxs[:, 0] < idxs[:, 1] if symmetric else np.ones(len(idxs), bool)
    D[idxs[keep, 0], idxs[keep, 1]] = v[keep]
    return D + D.T if symmetric else D


def test_rqa_matches_the_library(dataset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ref, idxs = dataset["ref"], dataset["idxs"]
    got = _algo(dataset, tmp_path).rqa(idxs, lmin=2, hist=True)
    assert set(got) == {"rr", "det", "lmean", "entr", "lmax", "smax", "n_rec", "n_lines", "n_lines_min", "n_pts_min",
                        "oti", "hist"}
    for c, k in enumerate(_lib.RQA_STATS):
        np.testing.assert_array_equal(got[k], ref["stats"][:, c], err_msg=k)
    for c, k in enumerate(_lib.RQA_COUNTS):
        np.testing.assert_array_equal(got[k], ref["counts"][:, c], err_msg=k)
    for k in ("lmax", "smax", "oti", "hist"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert (got["lmax"] >= 2).any() and got["hist"].shape == ref["hist"].shape
    assert "hist" not in _algo(dataset, tmp_path).rqa(idxs[:3])


def test_lmax_fills_Ds_and_is_normalised(dataset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    n, idxs, ref = dataset["n"], dataset["idxs"], dataset["ref"]
    algo = _algo(dataset, tmp_path, measure="lmax")
    assert algo.name == "Serra09-lmax"
    algo.all_pairwise(symmetric=True)
    D = _matrix(n, idxs, ref["lmax"].astype(np.float32), True)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), D)
    assert os.path.exists(str(tmp_path / "cache" / "Serra09-lmax_t_Ds.npz"))
    algo.normalize_by_length()
    want = (D / np.sqrt(dataset["lens"].astype(np.float64))[None, :]).astype(np.float32)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), want)
    assert (want != D).any()


def test_det_is_not_normalised_and_similarity_agrees(dataset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    n, idxs, ref = dataset["n"], dataset["idxs"], dataset["ref"]
    algo = _algo(dataset, tmp_path, measure="det")
    algo.all_pairwise(symmetric=False)
    D = _matrix(n, idxs, ref["stats"][:, 1].astype(np.float32), False)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), D)
    algo.normalize_by_length()
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), D)
    assert D.any()
    # the host pair loop (similarity) writes the same scores, and lmin reaches the kernel
    algo5 = _algo(dataset, tmp_path, measure="det", lmin=5)
    algo5.similarity(idxs[:10])
    feats, off, lens = dataset["packed"]
    r5 = _lib.crp_rqa(feats, off, lens, int(lens.max()), idxs[:10], _lib.crp_params(), lmin=5, smax=False)
    np.testing.assert_array_equal(np.asarray(algo5.Ds["main"])[idxs[:10, 0], idxs[:10, 1]],
                                  r5["stats"][:, 1].float().cpu().numpy())


def test_default_measure_is_qmax(dataset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    n, idxs = dataset["n"], dataset["idxs"]
    feats, off, lens = dataset["packed"]
    algo = _algo(dataset, tmp_path)
    assert algo.name == "Serra09"
    algo.all_pairwise(symmetric=True)
    q = _lib.crp_align(feats, off, lens, int(lens.max()), idxs, _lib.crp_params(), qmax=True)["qmax"].cpu().numpy()
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), _matrix(n, idxs, q, True))
    assert os.path.exists(str(tmp_path / "cache" / "Serra09_t_Ds.npz"))


def test_benchmark_with_measure(dataset, tmp_path, monkeypatch):
    from acoss import coverid
    monkeypatch.chdir(tmp_path)
    n, idxs, ref = dataset["n"], dataset["idxs"], dataset["ref"]
    algo = coverid.benchmark(dataset["csv"], dataset["fdir"], algorithm="Serra09", shortname="t",
                             cachedir=str(tmp_path / "cache"), measure="smax")
    assert algo.name == "Serra09-smax"
    assert os.path.exists("results_t_Serra09-smax.csv") and not os.path.exists("results_t_Serra09.csv")
    D = _matrix(n, idxs, ref["smax"], True)
    want = (D / np.sqrt(dataset["lens"].astype(np.float64))[None, :]).astype(np.float32)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), want)
    with pytest.raises(ValueError):
        coverid.benchmark(dataset["csv"], dataset["fdir"], algorithm="LateFusionChen", shortname="t",
                          cachedir=str(tmp_path / "cache"), measure="smax")
