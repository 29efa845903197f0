"""GPU tests of the plugin layer of best-of-n over the ranked OTI: Serra09(n_oti=2) and
ChenFusion(n_oti=2) through all_pairwise against the restatement tests/multi_oti_np.py on the
downsampled features with the existing finish applied, the per-pair methods and measure= on the
winning transposition, coverid.benchmark's name, and the default's names and scores. One dataset of
12 tracks of 4,000 .. 6,000 raw frames (100 .. 150 after the median downsampling)."""
import os

import numpy as np
import pytest

import multi_oti_np as mo
import oracle
import otib_np
import rqa_np
from oracle import np_oracle as npo
from acoss import coverid, synthetic
from acoss.algorithms.latefusion_chen import ChenFusion
from acoss.algorithms.rqa_serra09 import Serra09

pytestmark = pytest.mark.gpu

N = 12


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The dataset on disk and, per pair i < j, the two picks restated on the downsampled features."""
    tracks, labels = synthetic.make_hard_corpus("covers80", frames=4800, seed=9, fixed_length=False)
    keep = [k for k in range(len(tracks)) if 4000 <= len(tracks[k]) <= 6000][:N]
    assert len(keep) == N
    tracks, labels = [tracks[k] for k in keep], labels[keep]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path_factory.mktemp("multi_oti_plugin")), tracks, labels)
    ds = [npo.median_downsample(t, 40) for t in tracks]
    up = [(i, j) for i in range(N) for j in range(i + 1, N)]
    rows = {ij: mo.scored_picks(ds[ij[0]], ds[ij[1]], 2) for ij in up}
    best = {key: {ij: mo.best_of(rows[ij], key) for ij in up} for key in ("qmax", "dmax")}
    # the corpus is one where the second transposition changes the answer, for both aligners
    assert any(b[2] == 1 for b in best["qmax"].values()) and any(b[2] == 1 for b in best["dmax"].values())
    assert any(b[2] == 0 for b in best["qmax"].values())
    return {"csv": csv, "fdir": fdir, "ds": ds, "lens": np.array([len(d) for d in ds], np.int64), "up": up,
            "rows": rows, "best": best, "idxs": np.array(up, np.int32)}


def _matrix(best):
    S = np.zeros((N, N), np.float32)
    for (i, j), b in best.items():
        S[i, j] = S[j, i] = b[0]
    return S


def _kw(data, tmp_path):
    return dict(dataset_csv=data["csv"], datapath=data["fdir"], shortname="t", cachedir=str(tmp_path / "cache"))


def test_serra09_all_pairwise_is_the_best_of_two(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = Serra09(n_oti=2, **_kw(data, tmp_path))
    assert algo.name == "Serra09-oti2" and algo.n_oti == 2
    algo.all_pairwise(True, n_cores=-1, symmetric=True)
    algo.normalize_by_length()
    Q = _matrix(data["best"]["qmax"])
    want = (Q / np.sqrt(data["lens"].astype(np.float64))[None, :]).astype(np.float32)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), want)
    first = _matrix({ij: (r[0]["qmax"],) for ij, r in data["rows"].items()})
    assert (Q > first).any() and (Q >= first).all()
    algo.cleanup_memmap()


def test_chen_all_pairwise_is_the_best_of_two_per_aligner(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = ChenFusion(n_oti=2, **_kw(data, tmp_path))
    assert algo.name == "LateFusionChen-oti2"
    algo.all_pairwise(True, n_cores=-1, symmetric=True)
    algo.normalize_by_length()
    Q, D = _matrix(data["best"]["qmax"]), _matrix(data["best"]["dmax"])
    norm = np.sqrt(data["lens"].astype(np.float64))[None, :]
    with np.errstate(divide="ignore"):      # the finish: sqrt(n_j) / score
        np.testing.assert_array_equal(np.asarray(algo.Ds["qmax"]), (norm / Q).astype(np.float32))
        np.testing.assert_array_equal(np.asarray(algo.Ds["dmax"]), (norm / D).astype(np.float32))
    algo.cleanup_memmap()


def test_per_pair_methods_report_the_winning_transposition(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = Serra09(n_oti=2, **_kw(data, tmp_path))
    idxs = data["idxs"][:24]
    for alignment, seg, path in (("qmax", "qseg", "qpath"), ("dmax", "dseg", "dpath")):
        best = [data["best"][alignment][tuple(ij)] for ij in idxs]
        won = [otib_np.aligned(data["rows"][tuple(ij)][b[2]]["crp"]) for ij, b in zip(idxs, best)]
        assert {b[2] for b in best} == {0, 1}
        loc = algo.localize(idxs, alignment=alignment)
        np.testing.assert_array_equal(loc["oti"], [b[1] for b in best])
        np.testing.assert_array_equal(loc[alignment], np.array([b[0] for b in best], np.float32))
        np.testing.assert_array_equal(loc["cells"], np.array([w[seg] for w in won], np.int32))
        got = algo.align_path(idxs, alignment=alignment)
        np.testing.assert_array_equal(got["oti"], loc["oti"])
        np.testing.assert_array_equal(got[alignment], loc[alignment])
        np.testing.assert_array_equal(np.diff(got["path_off"]), [len(w[path]) for w in won])
        np.testing.assert_array_equal(got["path_cells"], np.concatenate([w[path] for w in won]).reshape(-1, 2))
    # rqa: on the Qmax winner
    best = [data["best"]["qmax"][tuple(ij)] for ij in idxs]
    got = algo.rqa(idxs, lmin=2)
    np.testing.assert_array_equal(got["oti"], [b[1] for b in best])
    for p, (ij, b) in enumerate(zip(idxs, best)):
        q = rqa_np.rqa(data["rows"][tuple(ij)][b[2]]["crp"], 2)
        assert tuple(int(got[k][p]) for k in rqa_np.COUNT_KEYS) == tuple(q[k] for k in rqa_np.COUNT_KEYS), p
        assert int(got["lmax"][p]) == q["lmax"] and float(got["smax"][p]) == q["smax"], p
        assert float(got["det"][p]) == q["det"] and float(got["rr"][p]) == q["rr"], p
    algo.cleanup_memmap()


def test_measure_det_runs_on_the_qmax_winner(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = Serra09(measure="det", n_oti=2, **_kw(data, tmp_path))
    assert algo.name == "Serra09-oti2-det"
    idxs = data["idxs"][:24]
    algo.similarity(idxs)
    best = [data["best"]["qmax"][tuple(ij)] for ij in idxs]
    want = [rqa_np.rqa(data["rows"][tuple(ij)][b[2]]["crp"], 2)["det"] for ij, b in zip(idxs, best)]
    at_first = [rqa_np.rqa(data["rows"][tuple(ij)][0]["crp"], 2)["det"] for ij in idxs]
    assert want != at_first
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"])[idxs[:, 0], idxs[:, 1]], np.array(want, np.float32))
    algo.cleanup_memmap()


def test_benchmark_writes_under_the_suffixed_name(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = coverid.benchmark(data["csv"], data["fdir"], algorithm="Serra09", shortname="t",
                             cachedir=str(tmp_path / "cache"), n_oti=2)
    assert algo.name == "Serra09-oti2"
    assert os.path.exists("results_t_Serra09-oti2.csv") and not os.path.exists("results_t_Serra09.csv")
    assert os.path.exists(str(tmp_path / "cache" / "Serra09-oti2_t_Ds.npz"))
    Q = _matrix(data["best"]["qmax"])
    want = (Q / np.sqrt(data["lens"].astype(np.float64))[None, :]).astype(np.float32)
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), want)


def test_one_transposition_writes_todays_names_and_scores(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = coverid.benchmark(data["csv"], data["fdir"], algorithm="Serra09", shortname="t",
                             cachedir=str(tmp_path / "cache"), n_oti=1)
    assert algo.name == "Serra09" and algo.n_oti == 1
    assert os.path.exists("results_t_Serra09.csv") and os.path.exists(str(tmp_path / "cache" / "Serra09_t_Ds.npz"))
    feats, off, lens = synthetic.pack(data["ds"])
    q, d, _ = oracle.crp_batch(feats, off, lens, data["idxs"], dmax=True)
    Q, D = np.zeros((N, N), np.float32), np.zeros((N, N), np.float32)
    Q[data["idxs"][:, 0], data["idxs"][:, 1]] = q
    D[data["idxs"][:, 0], data["idxs"][:, 1]] = d
    Q, D = Q + Q.T, D + D.T
    norm = np.sqrt(data["lens"].astype(np.float64))[None, :]
    np.testing.assert_array_equal(np.asarray(algo.Ds["main"]), (Q / norm).astype(np.float32))
    chen = ChenFusion(**_kw(data, tmp_path))
    assert chen.name == "LateFusionChen"
    chen.all_pairwise(True, n_cores=-1, symmetric=True)
    chen.normalize_by_length()
    with np.errstate(divide="ignore"):
        np.testing.assert_array_equal(np.asarray(chen.Ds["qmax"]), (norm / Q).astype(np.float32))
        np.testing.assert_array_equal(np.asarray(chen.Ds["dmax"]), (norm / D).astype(np.float32))
    chen.cleanup_memmap()
