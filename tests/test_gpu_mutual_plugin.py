"""GPU tests of the plugin layer of the mutual nearest-neighbour binarisation: coverid.benchmark(
mutual=True) for EarlyFusionTraile, the names of what it writes, the shared block-feature cache, and
the per-pair methods of EarlyFusion(mutual=True) against the batched entries and the restatement
(mutual_np.py).

The corpus: the 12 cliques (24 tracks) of test_gpu_plugin.py's EarlyFusion test, with MFCCs that are
a projection of the chroma. Twelve TRACKS cannot run the benchmark at all: its late fusion (SNF,
K = 20) takes K + 1 neighbours per song and so needs more than 21 songs."""
import os

import numpy as np
import pytest

import mutual_np as mn
import oracle
from acoss import _lib, coverid, synthetic
from acoss.algorithms.earlyfusion_traile import EarlyFusion
from acoss.features_io import cache_readable

pytestmark = pytest.mark.gpu

KEYS = ("mfccs", "ssms", "chromas", "early")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("mutual_plugin")
    tracks, labels = synthetic.make_corpus("covers80", frames=2000, seed=11)
    keep = np.flatnonzero(labels < 12)
    csv, fdir = synthetic.write_feature_dataset(str(root), [tracks[k] for k in keep], labels[keep], with_mfcc=True,
                                                mfcc_from_chroma=True)
    n = len(keep)
    assert n == 24
    return {"csv": csv, "fdir": fdir, "n": n,
            "up": np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)}


def _expect_Ds(algo, up, n, mutual):
    sc = _lib.earlyfusion(algo._bank(), up, algo.kappa, algo.K, mutual=mutual).cpu().numpy()
    out = {}
    for s, key in enumerate(KEYS):
        D = np.zeros((n, n), np.float32)
        D[up[:, 0], up[:, 1]] = sc[:, s]
        out[key] = D + D.T
    return out, sc


def test_benchmark_mutual_then_default_share_the_block_cache(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cache = tmp_path / "cache"
    n, up = data["n"], data["up"]
    algo = coverid.benchmark(data["csv"], data["fdir"], algorithm="EarlyFusionTraile", shortname="t",
                             cachedir=str(cache), mutual=True)
    assert algo.name == "EarlyFusionTraile-mutual" and algo.mutual is True
    assert os.path.exists("results_t_EarlyFusionTraile-mutual.csv")
    assert not os.path.exists("results_t_EarlyFusionTraile.csv")
    assert os.path.exists(str(cache / "EarlyFusionTraile-mutual_t_hpcp_Ds.npz"))
    assert not os.path.exists(str(cache / "EarlyFusionTraile_t_hpcp_Ds.npz"))
    # the block features keep today's names
    blocks = [str(cache / ("EarlyFusionTraile_t_hpcp_%d.h5" % i)) for i in range(n)]
    assert all(cache_readable(p) for p in blocks)
    assert not any(f.startswith("EarlyFusionTraile-mutual_t_hpcp_0.") for f in os.listdir(str(cache)))
    stamp = {f: os.stat(str(cache / f)).st_mtime_ns for f in os.listdir(str(cache))
             if f.startswith("EarlyFusionTraile_t_hpcp_")}
    assert len(stamp) >= n
    want, sc_m = _expect_Ds(algo, up, n, True)
    for key in KEYS:
        np.testing.assert_array_equal(np.asarray(algo.Ds[key]), want[key], err_msg=key)
    assert set(algo.Ds) == set(KEYS) | {"late", "early+late"}

    # without mutual: the cached block features are read back, not made again, and Ds are today's
    plain = coverid.benchmark(data["csv"], data["fdir"], algorithm="EarlyFusionTraile", shortname="t",
                              cachedir=str(cache))
    assert plain.name == "EarlyFusionTraile" and plain.mutual is False
    assert os.path.exists("results_t_EarlyFusionTraile.csv")
    assert os.path.exists(str(cache / "EarlyFusionTraile_t_hpcp_Ds.npz"))
    for f, t in stamp.items():
        assert os.stat(str(cache / f)).st_mtime_ns == t, f
    want_r, sc_r = _expect_Ds(plain, up, n, False)
    for key in KEYS:
        np.testing.assert_array_equal(np.asarray(plain.Ds[key]), want_r[key], err_msg=key)
    differ = int((sc_m != sc_r).sum())
    print("mutual against rows: %d of %d scores differ" % (differ, sc_m.size))
    assert differ > sc_m.size // 10


def test_per_pair_methods_follow_mutual(data, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    n, up = data["n"], data["up"]
    ef = EarlyFusion(data["csv"], data["fdir"], shortname="t", cachedir=str(tmp_path / "cache"), mutual=True,
                     early_snf=True)
    assert ef.name == "EarlyFusionTraile-mutual" and "early_snf" in ef.Ds
    idxs = up[:40]
    ef.similarity(idxs)
    want = _lib.earlyfusion(ef._bank(), idxs, ef.kappa, ef.K, mutual=True).cpu().numpy()
    for s, key in enumerate(KEYS):
        np.testing.assert_array_equal(np.asarray(ef.Ds[key])[idxs[:, 0], idxs[:, 1]], want[:, s].astype(np.float32))
    snf = _lib.earlyfusion_snf(ef._bank(), idxs, ef.kappa, ef.K, ef.niters, mutual=True)["score"].cpu().numpy()
    rows = _lib.earlyfusion_snf(ef._bank(), idxs, ef.kappa, ef.K, ef.niters)["score"].cpu().numpy()
    np.testing.assert_array_equal(np.asarray(ef.Ds["early_snf"])[idxs[:, 0], idxs[:, 1]], snf.astype(np.float32))
    assert np.isfinite(snf).all() and (snf != rows).any()
    dev = ef._device_scores(idxs)
    for s, key in enumerate(KEYS):
        np.testing.assert_array_equal(dev[key].cpu().numpy(), want[:, s].astype(np.float32))
    np.testing.assert_array_equal(dev["early_snf"].cpu().numpy(), snf.astype(np.float32))

    # localize and align_path return similarity's scores
    loc, pth = ef.localize(idxs), ef.align_path(idxs)
    np.testing.assert_array_equal(loc["scores"], want)
    np.testing.assert_array_equal(pth["scores"], want)
    np.testing.assert_array_equal(pth["cells"], loc["cells"])

    # pair_matrices: the restatement's masks of the four matrices the plugin forms for the pair
    i, j = int(idxs[3, 0]), int(idxs[3, 1])
    a, b = ef._device(i), ef._device(j)
    oti = int(_lib.get_oti(a["chroma_med"], b["chroma_med"]).item())
    C = [_lib.csm(a["mfccs"], b["mfccs"], kind="euclidean"), _lib.csm(a["ssms"], b["ssms"], kind="euclidean"),
         _lib.csm(a["chromas"], b["chromas"], kind="cosine", oti_shift=oti)]
    wsum = C[0] * 0
    for D in C:
        wsum += _lib.wcsm(D, ef.K, ef.K, 0.5)
    four = [D.cpu().numpy() for D in C + [_lib.neg_exp(wsum)]]
    mats = [m.cpu().numpy() for m in ef.pair_matrices(i, j)]
    plain = EarlyFusion(data["csv"], data["fdir"], shortname="t", cachedir=str(tmp_path / "cache"))
    rows = [m.cpu().numpy() for m in plain.pair_matrices(i, j)]
    for s in range(4):
        assert np.array_equal(mats[s], mn.mutual_smallest(four[s], ef.kappa)), KEYS[s]
        assert np.array_equal(rows[s], mn.rows_smallest(four[s], ef.kappa)), KEYS[s]
        assert oracle.sw_constrained(mats[s]) == want[3, s], KEYS[s]
    assert any(not np.array_equal(mats[s], rows[s]) for s in range(4))

    # pair_fusion returns the device's binary matrix: the mask of the cross block beside it
    cross, binary = ef.pair_fusion(i, j)
    assert binary.dtype == np.uint8 and np.isfinite(cross).all()
    assert np.array_equal(binary, mn.mutual_largest(cross, ef.kappa))
    assert oracle.sw_constrained(binary) == snf[3]
    cross_r, binary_r = plain.pair_fusion(i, j)
    assert np.array_equal(cross_r, cross) and np.array_equal(binary_r, mn.rows_largest(cross, ef.kappa))
