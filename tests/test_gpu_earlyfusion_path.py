"""GPU tests of EarlyFusion's located and traced alignments (acoss_earlyfusion_locate /
acoss_earlyfusion_path, EarlyFusion.localize / align_path) against the numpy restatement
tests/sw_path_np.py applied to the four canonical binary matrices of each pair.

The block features are integer-exact, as tests/test_gpu_earlyfusion_pin.py builds them (every CSM is
exact in any summation order), so the four binary matrices composed on the CPU from the oracle's
stages are the matrices the kernels align, and segments, lengths and paths compare with `==`."""
import numpy as np
import pytest

import oracle
import sw_path_np as sp
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

KAPPA, K, MU = 0.1, 10, 0.5


def _blocks(rng, nb):
    """Integer-exact block features of one song."""
    ch = np.zeros((nb, 480), np.float32)
    for b in range(nb):
        ch[b, rng.choice(480, 16, replace=False)] = 1.0
    return {"mfccs": rng.integers(-2, 3, size=(nb, 1000)).astype(np.float32),
            "ssms": rng.integers(0, 4, size=(nb, 1225)).astype(np.float32), "chromas": ch,
            "chroma_med": rng.permutation(12).astype(np.float32)}


def _cover(rng, base, nb):
    """The base's blocks resampled to nb blocks with integer perturbations (still exact)."""
    n0 = len(base["mfccs"])
    idx = np.minimum((np.arange(nb) * (n0 / nb) + rng.integers(0, 3)).astype(np.int64), n0 - 1)
    noise = lambda d: rng.integers(-1, 2, size=(nb, d)) * (rng.random((nb, d)) < 0.2)  # noqa: E731
    return {"mfccs": np.clip(base["mfccs"][idx] + noise(1000), -2, 2).astype(np.float32),
            "ssms": np.clip(base["ssms"][idx] + noise(1225), 0, 3).astype(np.float32),
            "chromas": base["chromas"][idx].copy(), "chroma_med": rng.permutation(12).astype(np.float32)}


def _corpus(seed, sizes):
    """Songs in cover pairs (2 k, 2 k + 1) with the given block counts."""
    rng = np.random.default_rng(seed)
    feats = []
    for k in range(0, len(sizes), 2):
        base = _blocks(rng, sizes[k])
        feats.append(base)
        if k + 1 < len(sizes):
            feats.append(_cover(rng, base, sizes[k + 1]))
    return feats


def _host_bank(feats):
    nbs = [len(f["mfccs"]) for f in feats]
    bank = {k: np.concatenate([f[k] for f in feats]) for k in ("mfccs", "ssms", "chromas")}
    bank["chroma_med"] = np.stack([f["chroma_med"] for f in feats])
    bank["nb"] = np.array(nbs, np.int32)
    bank["off"] = np.concatenate([[0], np.cumsum(nbs[:-1])]).astype(np.int64)
    return bank


def _dev_bank(host):
    import torch
    bank = {k: torch.as_tensor(host[k]).cuda() for k in ("mfccs", "ssms", "chromas", "chroma_med", "off", "nb")}
    bank["nb_host"] = host["nb"]
    bank["max_blocks"] = int(host["nb"].max())
    return bank


def _pair_matrices(a, b):
    """The four canonical binary matrices of a pair, from the oracle's stages: the three CSMs
    binarised, and E = canon_expf(-(((0 + W_m) + W_s) + W_c)) in float32, the order k_ef_wsum sums in."""
    C = [oracle.ef_csm(a["mfccs"], b["mfccs"], 0), oracle.ef_csm(a["ssms"], b["ssms"], 0),
         oracle.ef_csm(a["chromas"], b["chromas"], 1, a["chroma_med"], b["chroma_med"])]
    wsum = np.zeros_like(C[0])
    for D in C:
        wsum = (wsum + oracle.ef_wcsm(D, K, K, MU)).astype(np.float32)
    E = oracle.canon_expf(-wsum)
    return [oracle.ef_binarize(D, KAPPA) for D in C + [E]]


# name -> (seed, block counts, pairs): Da-TACOS-sized beat blocks (several matrices per wave), a
# second corpus of 40-90 blocks, and one with a 130-block track (17 lanes per matrix)
CORPORA = {
    "short": (1, [14, 22, 47, 31, 18, 40, 25, 36], [(i, j) for i in range(8) for j in range(8) if i != j]),
    "medium": (2, [40, 66, 90, 52, 75, 48], [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(3, 0), (5, 4)]),
    "long": (3, [130, 60, 35], [(0, 1), (1, 0), (0, 2), (2, 1)]),
}


@pytest.fixture(scope="module")
def cases():
    """name -> (device bank, pairs, restatement Results (P, 4), oracle scores): computed once."""
    out = {}
    for name, (seed, sizes, pairs) in CORPORA.items():
        feats = _corpus(seed, sizes)
        host = _host_bank(feats)
        pairs = np.array(pairs, np.int32)
        want = [[sp.sw_path(B) for B in _pair_matrices(feats[i], feats[j])] for i, j in pairs]
        out[name] = (_dev_bank(host), pairs, want, oracle.ef_batch(host, pairs, KAPPA, K=K, mu=MU), feats)
    return out


@pytest.mark.parametrize("name", list(CORPORA))
def test_the_composition_is_the_oracles(cases, name):
    """Before it is used: the restatement's scores of the composed matrices are oracle.ef_batch's."""
    _, pairs, want, canon, _ = cases[name]
    got = np.array([[r.score for r in row] for row in want])
    np.testing.assert_array_equal(got, canon)
    assert np.count_nonzero(got) > 2 * len(pairs)


def _check(bank, pairs, want):
    ref = _lib.earlyfusion(bank, pairs, KAPPA, K, MU).cpu().numpy()
    loc = _lib.earlyfusion_locate(bank, pairs, KAPPA, K, MU)
    pth = _lib.earlyfusion_path(bank, pairs, KAPPA, K, MU)
    lscore, lseg = loc["scores"].cpu().numpy(), loc["seg"].cpu().numpy()
    pscore, pseg = pth["scores"].cpu().numpy(), pth["seg"].cpu().numpy()
    off, cells = pth["path_off"].cpu().numpy(), pth["cells"].cpu().numpy()
    np.testing.assert_array_equal(lscore, ref)  # bit for bit
    np.testing.assert_array_equal(pscore, ref)
    assert off.shape == (4 * len(pairs) + 1,) and off[-1] == len(cells)
    for p, row in enumerate(want):
        for s, res in enumerate(row):
            t = "pair %d %s matrix %d" % (p, pairs[p].tolist(), s)
            got = cells[off[4 * p + s]:off[4 * p + s + 1]]
            print("%s: score %r seg %r, %d cells; restatement %r seg %r, %d cells"
                  % (t, ref[p, s], pseg[p, s].tolist(), len(got), res.score, res.seg, len(res.path)))
            assert ref[p, s] == res.score, t
            assert lseg[p, s].tolist() == list(res.seg), t
            assert pseg[p, s].tolist() == list(res.seg), t
            assert len(got) == len(res.path), t
            assert got.tolist() == res.path.tolist(), t


@pytest.mark.parametrize("name", list(CORPORA))
def test_locate_and_path_match_restatement(cases, name, monkeypatch):
    """All four matrices of every pair, with a workspace budget that splits the pairs into several
    chunks, so both streams and both scratch sets are used."""
    bank, pairs, want, _, _ = cases[name]
    monkeypatch.setenv("ACOSS_EF_BYTES", str({"short": 400_000, "medium": 1_500_000, "long": 1_000_000}[name]))
    _check(bank, pairs, want)


def test_one_chunk(cases):
    bank, pairs, want, _, _ = cases["short"]
    _check(bank, pairs[:9], want[:9])


def test_a_long_pair_list_comes_back_in_the_callers_order(cases):
    """More than 4096 pairs run in (reference band, query) order, as earlyfusion()'s do; scores,
    segments and the ragged paths come back in the order given."""
    bank, pairs, want, canon, _ = cases["short"]
    reps = 4096 // len(pairs) + 1
    rng = np.random.default_rng(0)
    pick = rng.permutation(np.tile(np.arange(len(pairs)), reps))
    assert len(pick) > 4096
    loc = _lib.earlyfusion_locate(bank, pairs[pick], KAPPA, K, MU)
    pth = _lib.earlyfusion_path(bank, pairs[pick], KAPPA, K, MU)
    np.testing.assert_array_equal(_lib.earlyfusion(bank, pairs[pick], KAPPA, K, MU).cpu().numpy(), canon[pick])
    seg = np.array([[r.seg for r in row] for row in want], np.int32)[pick]
    for got in (loc, pth):
        np.testing.assert_array_equal(got["scores"].cpu().numpy(), canon[pick])
        np.testing.assert_array_equal(got["seg"].cpu().numpy(), seg)
    lens = np.array([[len(r.path) for r in row] for row in want])[pick].reshape(-1)
    np.testing.assert_array_equal(np.diff(pth["path_off"].cpu().numpy()), lens)
    cells = np.concatenate([r.path for p in pick for r in want[p]])
    np.testing.assert_array_equal(pth["cells"].cpu().numpy(), cells)


def test_refuses_a_short_path_cap(cases):
    import torch
    bank, pairs, _, _, _ = cases["short"]
    dp, _, lead, tail = _lib._ef_args(bank, pairs[:2], KAPPA, K, MU)
    bound = int(bank["max_blocks"]) - 3

    def call(cap):
        sc = torch.empty((2, 4), dtype=torch.float64, device="cuda")
        lens = torch.empty((2, 4), dtype=torch.int32, device="cuda")
        path = torch.empty((2, 4, bound, 2), dtype=torch.int32, device="cuda")
        rc = _lib.load_library().acoss_earlyfusion_path(*lead, _lib._ptr(dp), 2, *tail, _lib._ptr(sc), _lib._ptr(None),
                                                        cap, _lib._ptr(lens), _lib._ptr(path), _lib._stream())
        torch.cuda.synchronize()
        return rc, _lib.load_library().acoss_last_error().decode()

    assert call(bound)[0] == 0
    rc, msg = call(bound - 1)
    assert rc == -1 and "= %d" % bound in msg  # ACOSS_E_ARG, naming the bound


def _write_cache(ef, feats):
    from acoss.features_io import save_features
    for i, bf in enumerate(feats):
        save_features("%s_%i.h5" % (ef.get_cacheprefix(), i), bf)


def test_plugin_localize_and_align_path(cases, tmp_path, monkeypatch):
    """Through the plugin class, on the cached block features of the short corpus; its feature files
    carry no beat onsets, which frames=True says."""
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    _, pairs, want, canon, feats = cases["short"]
    monkeypatch.chdir(tmp_path)
    tracks = [np.zeros((8, 12), np.float32) for _ in feats]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), tracks, np.arange(len(feats)) // 2)
    ef = EarlyFusion(csv, fdir, shortname="where", cachedir=str(tmp_path / "cache"))
    _write_cache(ef, feats)
    loc = ef.localize(pairs)
    np.testing.assert_array_equal(loc["scores"], canon)
    assert loc["cells"].shape == (len(pairs), 4, 4)
    for p, row in enumerate(want):
        for s, res in enumerate(row):
            assert loc["cells"][p, s].tolist() == list(res.seg)
            r0, c0, r1, c1 = res.seg
            assert loc["query_blocks"][p, s].tolist() == ([r0, r1 + 1] if res.score > 0 else [-1, -1])
            assert loc["reference_blocks"][p, s].tolist() == ([c0, c1 + 1] if res.score > 0 else [-1, -1])
    ap = ef.align_path(pairs)
    np.testing.assert_array_equal(ap["scores"], canon)
    np.testing.assert_array_equal(ap["cells"], loc["cells"])
    assert ap["path_off"].shape == (4 * len(pairs) + 1,)
    for p, row in enumerate(want):
        for s, res in enumerate(row):
            got = ap["path_cells"][ap["path_off"][4 * p + s]:ap["path_off"][4 * p + s + 1]]
            assert got.tolist() == res.path.tolist()
    with pytest.raises(ValueError, match="onsets"):
        ef.localize(pairs[:2], frames=True)


def test_plugin_localize_frames(tmp_path, monkeypatch):
    """frames=True on a corpus written with beat onsets: the ranges are engine.block_frames of the
    cells, from the onsets and chroma lengths of the feature files."""
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    from acoss.features_io import load_features
    monkeypatch.chdir(tmp_path)
    songs, labels = synthetic.make_corpus("covers80", frames=2000, seed=5)
    songs, labels = songs[:4], labels[:4]
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), songs, labels, with_mfcc=True, mfcc_from_chroma=True)
    ef = EarlyFusion(csv, fdir, shortname="frames", cachedir=str(tmp_path / "cache"))
    pairs = np.array([(0, 1), (1, 0), (2, 3), (0, 3)], np.int32)
    loc = ef.localize(pairs, frames=True)
    assert np.count_nonzero(loc["scores"]) >= 8
    info = []
    for i in range(4):
        f = load_features(ef.filepaths[i], keys=("hpcp", "madmom_features"))
        info.append((np.asarray(f["madmom_features"]["onsets"], np.int64), len(f["hpcp"])))
    for p, (a, b) in enumerate(pairs):
        for s in range(4):
            r0, c0, r1, c1 = loc["cells"][p, s]
            for key, song, lo, hi in (("query_frames", a, r0, r1), ("reference_frames", b, c0, c1)):
                o, n = info[song]
                want = [-1, -1] if lo < 0 else [int(o[lo]), min(int(o[hi + ef.blocksize]), n)]
                assert loc[key][p, s].tolist() == want
                if lo >= 0:
                    assert 0 <= want[0] < want[1] <= n
