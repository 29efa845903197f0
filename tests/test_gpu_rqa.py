"""GPU tests of the cross-recurrence quantification (acoss_rqa_crp / acoss_crp_rqa, crp_dp.hip
k_crp_rqa) against the numpy restatement tests/rqa_np.py. The integers, lmax, Smax, the histogram
and RR, DET, LMEAN compare with `==`; ENTR at rtol 1e-11 (a sum of at most 16,384 non-negative
terms, each good to a few ulp, on either side: about 1.8e-12 each), and with `==` where no line
reaches lmin."""
import numpy as np
import pytest

import oracle
import rqa_np
from rqa_np import CASES, COUNT_KEYS, LMINS, STAT_KEYS
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

INF = float("inf")


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check_one(got, p, want, what):
    """Pair p of a batch result (or p = None: a matrix result) against measures(...) of the restatement."""
    counts = got["counts"] if p is None else got["counts"][p]
    stats = got["stats"] if p is None else got["stats"][p]
    lmax = got["lmax"][0 if p is None else p]
    print("%s: counts %r lmax %d stats %r; restatement %r" % (what, counts.tolist(), lmax, stats.tolist(),
                                                              {k: want[k] for k in COUNT_KEYS + ("lmax",) + STAT_KEYS}))
    assert tuple(int(x) for x in counts) == tuple(want[k] for k in COUNT_KEYS), what
    assert int(lmax) == want["lmax"], what
    for c, k in enumerate(STAT_KEYS[:3]):
        assert float(stats[c]) == want[k], (what, k)
    if want["n_lines_min"] == 0:
        assert float(stats[3]) == 0.0 == want["entr"], what
    else:
        np.testing.assert_allclose(float(stats[3]), want["entr"], rtol=1e-11, atol=0.0, err_msg=what)


@pytest.mark.parametrize("name", list(CASES))
def test_rqa_crp_matches_restatement(name):
    C = rqa_np.matrix(name)
    for lmin in LMINS:
        want = rqa_np.expected(name, lmin)
        got = _host(_lib.rqa_crp(C, lmin=lmin, smax=True, hist=True))
        _check_one(got, None, want, "%s lmin %d" % (name, lmin))
        np.testing.assert_array_equal(got["hist"], want["hist"])
        assert float(got["smax"][0]) == want["smax"], (name, lmin)
    assert want["smax"] == float(_lib.align_crp(C, 0, INF, INF).item())


def test_rqa_crp_without_smax_or_lines():
    C = rqa_np.matrix("rand_33x70")
    r = _lib.rqa_crp(C, smax=False)
    assert "smax" not in r and "hist" not in r
    _check_one(_host(r), None, rqa_np.expected("rand_33x70", 2), "no smax")


def test_rqa_crp_empty_matrix():
    for shape in ((0, 5), (5, 0)):
        got = _host(_lib.rqa_crp(np.zeros(shape, np.uint8), hist=4))
        assert not got["counts"].any() and not got["stats"].any() and not got["hist"].any()
        assert got["lmax"][0] == 0 and got["smax"][0] == 0.0


def test_rqa_crp_refusals():
    C = np.zeros((10, 10), np.uint8)
    C[3, 4] = 2
    with pytest.raises(_lib.AcossHipError):
        _lib.rqa_crp(C)
    with pytest.raises(_lib.AcossHipError):
        _lib.rqa_crp(rqa_np.matrix("rand_33x70"), lmin=0)
    with pytest.raises(_lib.AcossHipError):  # a line could have 16,384 cells: more than the histogram takes
        _lib.rqa_crp(np.zeros((16384, 16384), np.uint8), smax=False)


def test_rqa_crp_short_hist_cap_keeps_the_counts():
    C = rqa_np.matrix("ones_70x45")
    want = rqa_np.expected("ones_70x45", 2)
    got = _host(_lib.rqa_crp(C, hist=5))
    assert want["lmax"] == 45 and got["hist"].shape == (5,)
    np.testing.assert_array_equal(got["hist"], want["hist"][:5])
    _check_one(got, None, want, "hist_cap 5")
    wide = _host(_lib.rqa_crp(C, hist=100))["hist"]  # beyond min(M, N): zeros
    np.testing.assert_array_equal(wide[:46], want["hist"])
    assert not wide[46:].any()


# ---- the batch entry ----
def _reference(tracks, pairs):
    """Per pair the oracle's CRP and its line histogram."""
    out = []
    for a, b in pairs:
        C = oracle.crp_pair(tracks[a], tracks[b])["crp"]
        out.append((C.shape, rqa_np.line_hist(C)))
    return out


def _check_batch(tracks, pairs, ref, lmin=2):
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    L = _lib.stacked_len(int(lens.max()))
    got = _host(_lib.crp_rqa(feats, off, lens, int(lens.max()), pairs, P, lmin=lmin, smax=True, hist_cap=L + 1))
    ship = _host(_lib.crp_align(feats, off, lens, int(lens.max()), pairs, P, qmax=True, oti=True))
    Pinf = _lib.crp_params(gamma_open=INF, gamma_ext=INF)
    sinf = _host(_lib.crp_align(feats, off, lens, int(lens.max()), pairs, Pinf, qmax=True))
    np.testing.assert_array_equal(got["oti"], ship["oti"])
    np.testing.assert_array_equal(got["smax"], sinf["qmax"])
    for p, ((M, N), H) in enumerate(ref):
        _check_one(got, p, rqa_np.measures(H, M, N, lmin), "pair %d (%d x %d)" % (p, M, N))
        np.testing.assert_array_equal(got["hist"][p, :len(H)], H)
        assert not got["hist"][p, len(H):].any()
    return got, ship


@pytest.fixture(scope="module")
def covers24():
    tracks, _ = synthetic.make_corpus("covers80", frames=300, seed=7)
    tracks = tracks[:24]
    pairs = np.array([(i, j) for i in range(24) for j in range(i + 1, 24)], np.int32)
    return tracks, pairs, _reference(tracks, pairs)


def test_crp_rqa_batch(covers24):
    tracks, pairs, ref = covers24
    got, _ = _check_batch(tracks, pairs, ref)
    assert (got["lmax"] >= 3).any() and (got["smax"] > 0).any()
    _check_batch(tracks, pairs[:40], ref[:40], lmin=5)


def test_crp_rqa_small_dp_batches(covers24, monkeypatch):
    """DP batches of 7 pairs (40 launches, the last of 3 pairs) give what one batch gives."""
    tracks, pairs, _ = covers24
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    one = _host(_lib.crp_rqa(feats, off, lens, int(lens.max()), pairs, P, hist_cap=40))
    monkeypatch.setenv("ACOSS_BATCH_PAIRS", "7")
    many = _host(_lib.crp_rqa(feats, off, lens, int(lens.max()), pairs, P, hist_cap=40))
    for key in ("counts", "lmax", "stats", "smax", "oti", "hist"):
        np.testing.assert_array_equal(many[key], one[key], err_msg=key)
    assert one["counts"][:, 0].any() and one["hist"][:, 3:].any()


def test_crp_rqa_keeps_to_its_workspace(covers24):
    """crp_align before and after crp_rqa gives the same Qmax, and crp_rqa the same after it."""
    tracks, pairs, _ = covers24
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    args = (feats, off, lens, int(lens.max()), pairs, P)
    before = _lib.crp_align(*args, qmax=True)["qmax"].cpu().numpy()
    first = _host(_lib.crp_rqa(*args))
    after = _lib.crp_align(*args, qmax=True)["qmax"].cpu().numpy()
    second = _host(_lib.crp_rqa(*args))
    np.testing.assert_array_equal(before, after)
    for key in first:
        np.testing.assert_array_equal(first[key], second[key], err_msg=key)


def test_crp_rqa_ragged_batch():
    """Lengths 37 .. 1100 in one launch: 32 rows per lane, mixed dims, and silences."""
    rng = np.random.Generator(np.random.PCG64(99))
    tracks = []
    for n in [37, 120, 400, 700, 1100]:
        x = synthetic.render(rng, synthetic.base_sequence(rng, n))
        if n >= 700:
            x[50:300] = 0.0
        tracks.append(x)
    pairs = np.array([(i, j) for i in range(len(tracks)) for j in range(len(tracks)) if i != j], np.int32)
    _check_batch(tracks, pairs, _reference(tracks, pairs))
    # and at 8 rows per lane: the three short tracks alone
    short = np.array([(i, j) for i in range(3) for j in range(3) if i != j], np.int32)
    _check_batch(tracks[:3], short, _reference(tracks[:3], short))
