"""GPU tests of acoss_simple_profile: the SiMPle matrix profile and its index per pair.

sslen = 10 runs k_simple_mfma<1> at every length, sslen = 7 k_simple_pair<1> (simple.hip). Bars:
mp and mpi bit-equal to the numpy restatement of the oracle's loops (tests/simple_profile_np.py,
pinned to the C oracle by tests/test_simple_profile_host.py) on small pairs; at length, where the
rational-arithmetic restatement is too slow, median(mp) == acoss_simple_mp's score bit for bit,
exact zeros and indices where the answer is planted, and against a plain float64 numpy distance
matrix D (BLAS dots): |D[i, mpi[i]] - mp[i]| <= 1e-12 and min_j D[i, j] >= mp[i] - 1e-12. That
tolerance is derived: a distance is about 40 roundings of values of magnitude <= 20, about 9e-14
per evaluation, two evaluations differ by at most twice that, and 1e-12 is five times above."""
import ctypes

import numpy as np
import pytest

import oracle
from simple_profile_np import dist_matrix, frame_dots, simple_profile_np, unit_columns

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def lib():
    from acoss import _lib
    _lib.load_library()
    return _lib


def _np(r):
    return {k: v.detach().cpu().numpy() for k, v in r.items()}


def _same(a, b):
    """Equal values, NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _rows(r, p):
    return r["mp"][r["off"][p]:r["off"][p + 1]], r["mpi"][r["off"][p]:r["off"][p + 1]]


def _check_bound(mp, mpi, D, cols=None):
    """mp and mpi against the plain numpy distance matrix D (over the columns `cols` if given)."""
    assert (mpi >= 0).all() and (mpi < D.shape[1]).all()
    assert np.abs(D[np.arange(len(mp)), mpi] - mp).max() <= TOL
    Dm = D if cols is None else D[:, cols]
    assert (Dm.min(axis=1) >= mp - TOL).all()


# ------------------------------------------------------------------ 1. exact, small pairs
SMALL_LENS = [9, 10, 11, 23, 37, 45, 64]
# (10, x) and (x, 10): P = 1 and Q = 1 at sslen 10; the 9-column track on either side
SMALL_PAIRS = [(1, 3), (3, 1), (4, 5), (5, 4), (6, 4), (2, 6), (3, 3), (0, 3), (3, 0), (1, 1)]


@pytest.fixture(scope="module")
def small():
    """The tracks and, per (pair, rolled or not), the frame dots of the restatement (they depend on
    no sslen, and forming them in rational arithmetic is what takes the time)."""
    rng = np.random.default_rng(23)
    feats = [unit_columns(rng, n) for n in SMALL_LENS]
    dots = {}
    for a, b in SMALL_PAIRS:
        k = oracle.simple_oti(feats[a], feats[b])
        for kk in {0, k}:
            dots[a, b, kk] = frame_dots(feats[a], feats[b], kk)
    return feats, dots


@pytest.mark.parametrize("apply_oti", [True, False])
@pytest.mark.parametrize("sslen", [10, 7])
def test_exact_vs_restatement(lib, small, sslen, apply_oti):
    feats, dots = small
    r = _np(lib.simple_profile(feats, np.array(SMALL_PAIRS, np.int32), sslen=sslen, apply_oti=apply_oti))
    lens = np.array(SMALL_LENS)
    assert np.array_equal(r["off"], lib.simple_profile_offsets(lens, SMALL_PAIRS, sslen))
    assert r["mp"].dtype == np.float64 and r["mpi"].dtype == np.int32 and len(r["mp"]) == r["off"][-1]
    for p, (a, b) in enumerate(SMALL_PAIRS):
        k = oracle.simple_oti(feats[a], feats[b])
        assert r["oti"][p] == k
        kk = k if apply_oti else 0
        mp, mpi = simple_profile_np(feats[a], feats[b], sslen, kk, ga=dots[a, b, kk])
        gmp, gmpi = _rows(r, p)
        assert _same(gmp, mp), (a, b)
        assert np.array_equal(gmpi, mpi), (a, b)
        assert _same(r["score"][p], oracle.simple_sim(feats[a], feats[b], sslen, k=kk)), (a, b)
    if sslen == 10:  # the 9-column track: no rows as the query, rows of (NaN, -1) as the reference
        assert r["off"][8] - r["off"][7] == 0 and np.isnan(r["score"][7])
        mp, mpi = _rows(r, 8)
        assert len(mp) == 14 and np.isnan(mp).all() and (mpi == -1).all() and np.isnan(r["score"][8])


# ------------------------------------------------------------------ 2. long, ragged, multi-group
@pytest.fixture(scope="module")
def long_tracks():
    rng = np.random.default_rng(15)
    feats = [unit_columns(rng, n) for n in [700, 1300, 513, 257, 96]]
    feats.append(feats[0].copy())  # identical tracks: zero distances
    return feats


@pytest.mark.parametrize("sslen", [10, 7])
def test_long_ragged(lib, long_tracks, sslen):
    feats = long_tracks
    n = len(feats)
    pairs = np.array([(i, j) for i in range(n) for j in range(n) if (i + j) % 2 == 0 or i == 5], np.int32)
    r = _np(lib.simple_profile(feats, pairs, sslen=sslen))
    score, oti = lib.simple_mp(feats, pairs, sslen=sslen)
    score, oti = score.cpu().numpy(), oti.cpu().numpy()
    assert np.array_equal(r["oti"], oti)
    assert np.array_equal(r["score"], score)
    for p, (a, b) in enumerate(pairs):
        mp, mpi = _rows(r, p)
        assert len(mp) == feats[a].shape[1] - sslen + 1
        assert np.median(mp) == score[p], (a, b)
        _check_bound(mp, mpi, dist_matrix(feats[a], feats[b], sslen, int(oti[p])))
        if {int(a), int(b)} == {0, 5}:
            assert np.array_equal(mp, np.zeros(len(mp))) and np.array_equal(mpi, np.arange(len(mp)))


# ------------------------------------------------------------------ 3. planted exact answer
@pytest.mark.parametrize("sslen", [10, 7])
def test_planted_copy_is_found_in_the_first_place(lib, sslen):
    rng = np.random.default_rng(31)
    A = unit_columns(rng, 700)
    s, w = 250, 200
    cut = A[:, s:s + w]
    B = np.concatenate([unit_columns(rng, 300), cut, unit_columns(rng, 400), cut, unit_columns(rng, 200)], axis=1)
    assert B.shape[1] == 1300
    r = _np(lib.simple_profile([A, B], np.array([[0, 1]], np.int32), sslen=sslen, apply_oti=False))
    rows = np.arange(s, s + w - sslen + 1)
    assert np.array_equal(r["mp"][rows], np.zeros(len(rows)))
    assert np.array_equal(r["mpi"][rows], 300 + rows - s)  # the first copy, never the second (at 900)
    _check_bound(r["mp"], r["mpi"], dist_matrix(A, B, sslen))


# ------------------------------------------------------------------ 4. ties at scale
@pytest.mark.parametrize("sslen", [10, 7])
def test_all_ties(lib, sslen):
    """Every distance of a silent track ties: the contention case of the second walk."""
    Z = np.zeros((12, 300))
    R = unit_columns(np.random.default_rng(41), 300)
    pairs = np.array([[0, 0], [0, 1], [1, 0]], np.int32)
    r1 = _np(lib.simple_profile([Z, R], pairs, sslen=sslen))
    r2 = _np(lib.simple_profile([Z, R], pairs, sslen=sslen))
    P = 300 - sslen + 1
    assert np.array_equal(r1["mp"].view(np.int64), r2["mp"].view(np.int64)) and np.array_equal(r1["mpi"], r2["mpi"])
    mp, mpi = _rows(r1, 0)
    assert np.array_equal(mp, np.zeros(P)) and np.array_equal(mpi, np.zeros(P, np.int32))
    # silent query: dist(i, j) = the reference's window norm sb[j], the same row P times
    mp, mpi = _rows(r1, 1)
    assert (mp == mp[0]).all() and (mpi == mpi[0]).all()
    assert abs(mp[0] - sslen) < 1e-9  # sslen unit columns
    # silent reference: dist(i, j) = sa[i] for every j, so the first column
    mp, mpi = _rows(r1, 2)
    assert (mpi == 0).all() and np.abs(mp - sslen).max() < 1e-9


# ------------------------------------------------------------------ 5. NaN column
@pytest.mark.parametrize("sslen", [10, 7])
def test_nan_column(lib, sslen):
    rng = np.random.default_rng(51)
    A, B = unit_columns(rng, 420), unit_columns(rng, 380)
    c = 133
    An, Bn = A.copy(), B.copy()
    An[:, c] = np.nan
    Bn[:, c] = np.nan
    pairs = np.array([[0, 1], [2, 1], [0, 3]], np.int32)
    r = _np(lib.simple_profile([A, B, An, Bn], pairs, sslen=sslen, apply_oti=False))
    clean_mp, clean_mpi = _rows(r, 0)
    # NaN in the query: the rows whose window holds column c have no distance
    mp, mpi = _rows(r, 1)
    hit = np.zeros(len(mp), bool)
    hit[c - sslen + 1:c + 1] = True
    assert np.isnan(mp[hit]).all() and (mpi[hit] == -1).all()
    assert np.array_equal(mp[~hit], clean_mp[~hit]) and np.array_equal(mpi[~hit], clean_mpi[~hit])
    score, _ = lib.simple_mp([A, B, An, Bn], pairs, sslen=sslen, apply_oti=False)
    assert _same(r["score"], score.cpu().numpy())
    # NaN in the reference: the columns whose window holds it are never the nearest
    mp, mpi = _rows(r, 2)
    assert not np.isnan(mp).any()
    assert not ((mpi >= c - sslen + 1) & (mpi <= c)).any()
    cols = np.ones(380 - sslen + 1, bool)
    cols[c - sslen + 1:c + 1] = False
    _check_bound(mp, mpi, dist_matrix(A, B, sslen), cols)
    assert np.median(mp) == r["score"][2]


# ------------------------------------------------------------------ 6. maximum length
def test_max_length(lib):
    rng = np.random.default_rng(4096)
    feats = [unit_columns(rng, 4096), unit_columns(rng, 350)]
    pairs = np.array([(0, 1), (1, 0)], np.int32)
    r = _np(lib.simple_profile(feats, pairs))
    score, oti = lib.simple_mp(feats, pairs)
    score, oti = score.cpu().numpy(), oti.cpu().numpy()
    assert np.array_equal(r["score"], score) and np.array_equal(r["oti"], oti)
    for p, (a, b) in enumerate(pairs):
        mp, mpi = _rows(r, p)
        assert len(mp) == feats[a].shape[1] - 9
        assert np.median(mp) == score[p]
        _check_bound(mp, mpi, dist_matrix(feats[a], feats[b], 10, int(oti[p])))


# ------------------------------------------------------------------ 7. list semantics
@pytest.mark.parametrize("sslen", [10, 7])
def test_list_semantics(lib, monkeypatch, sslen):
    """A pair's ranges depend on the pair alone: listed twice, in a shuffled list that names only
    some of the tracks, and across launches of three pairs (ACOSS_SIMPLE_PROFILE_BATCH)."""
    rng = np.random.default_rng(71)
    feats = [unit_columns(rng, n) for n in [40, 300, 12, 150, 64, 77]]
    pairs = np.array([(3, 1), (5, 3), (1, 5), (3, 1), (5, 5), (1, 3), (3, 5)], np.int32)  # tracks 0, 2, 4 unnamed
    r = _np(lib.simple_profile(feats, pairs, sslen=sslen))
    a, b = _rows(r, 0), _rows(r, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for p in (0, 1, 2, 4):
        one = _np(lib.simple_profile(feats, pairs[p:p + 1], sslen=sslen))
        mp, mpi = _rows(r, p)
        assert np.array_equal(one["mp"], mp) and np.array_equal(one["mpi"], mpi)
        assert one["score"][0] == r["score"][p] and one["oti"][0] == r["oti"][p]
    monkeypatch.setenv("ACOSS_SIMPLE_PROFILE_BATCH", "3")
    rb = _np(lib.simple_profile(feats, pairs, sslen=sslen))
    for key in ("off", "mp", "mpi", "score", "oti"):
        assert np.array_equal(r[key], rb[key]), key


# ------------------------------------------------------------------ 8. refusals
def test_refusals(lib):
    import torch
    L = lib.load_library()
    rng = np.random.default_rng(81)
    feats = [unit_columns(rng, n) for n in [30, 50, 20]]
    flat = torch.from_numpy(np.concatenate([f.ravel() for f in feats])).cuda()
    lens = np.array([30, 50, 20], np.int32)
    toff = torch.from_numpy(np.array([0, 12 * 30, 12 * 80], np.int64)).cuda()
    tlen = torch.from_numpy(lens).cuda()
    pairs = torch.from_numpy(np.array([[0, 1], [1, 2], [2, 0]], np.int32)).cuda()
    good = lib.simple_profile_offsets(lens, [(0, 1), (1, 2), (2, 0)], 10)  # 0, 21, 62, 73

    def call(off, total, sslen=10, max_len=50):
        mp = torch.full((80,), -7.0, dtype=torch.float64, device="cuda")
        mpi = torch.full((80,), -7, dtype=torch.int32, device="cuda")
        score = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
        oti = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        off_d = torch.from_numpy(np.asarray(off, np.int64)).cuda()
        rc = L.acoss_simple_profile(flat.data_ptr(), toff.data_ptr(), tlen.data_ptr(), 3, max_len, pairs.data_ptr(), 3,
                                    sslen, 1, off_d.data_ptr(), total, mp.data_ptr(), mpi.data_ptr(),
                                    score.data_ptr(), oti.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        untouched = bool((mp == -7).all() and (mpi == -7).all() and (score == -7).all() and (oti == -7).all())
        return rc, untouched, L.acoss_last_error().decode()

    rc, untouched, _ = call(good, 73)
    assert rc == 0 and not untouched
    rc, untouched, msg = call([0, 21, 61, 73], 73)  # pair 1 needs 41 rows, has 40
    assert rc == -1 and untouched and "pair 1" in msg
    rc, untouched, msg = call(good, 72)  # prof_total too small for the last pair
    assert rc == -1 and untouched and "pair 2" in msg
    rc, untouched, msg = call([-1, 21, 62, 73], 73)
    assert rc == -1 and untouched and "pair 0" in msg
    rc, untouched, _ = call(good, 73, sslen=17)
    assert rc == -1 and untouched
    rc, untouched, _ = call(good, 73, max_len=4097)
    assert rc == -2 and untouched


# ------------------------------------------------------------------ 9. the plugin
def test_plugin_profile(tmp_path, monkeypatch):
    from acoss import synthetic
    from acoss.algorithms.simple_silva import Simple
    from acoss.engine import subsequence_frames
    monkeypatch.chdir(tmp_path)
    tracks, labels = synthetic.make_corpus("covers80", frames=3050, seed=11)
    keep = np.flatnonzero(labels < 3)
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), [tracks[k] for k in keep], labels[keep])
    algo = Simple(csv, fdir, shortname="t", cachedir=str(tmp_path / "cache"))
    n = algo.N
    idxs = np.array([(i, j) for i in range(n) for j in range(n) if i != j][:12], np.int32)
    algo.similarity(idxs)
    r = algo.profile(idxs)
    assert np.array_equal((-r["score"]).astype(np.float32), np.asarray(algo.Ds["main"])[idxs[:, 0], idxs[:, 1]])
    T = np.array([algo.all_feats[i].shape[1] for i in range(n)])
    assert np.array_equal(np.diff(r["off"]), T[idxs[:, 0]] - algo.SSLEN + 1)
    assert r["mp"].shape == r["mpi"].shape == (r["off"][-1],) and (r["mpi"] >= 0).all()
    rows = np.diff(r["off"])
    i = np.arange(r["off"][-1]) - np.repeat(r["off"][:-1], rows)
    nq, nr = np.repeat(algo._n_frames[idxs[:, 0]], rows), np.repeat(algo._n_frames[idxs[:, 1]], rows)
    assert np.array_equal(r["query_frames"], subsequence_frames(i, algo.SSLEN, algo.WIN, algo.SKIP, nq))
    assert np.array_equal(r["reference_frames"], subsequence_frames(r["mpi"], algo.SSLEN, algo.WIN, algo.SKIP, nr))
    assert (r["reference_frames"][:, 1] <= nr).all() and (r["reference_frames"][:, 0] < r["reference_frames"][:, 1]).all()
    for p in range(len(idxs)):
        assert np.median(r["mp"][r["off"][p]:r["off"][p + 1]]) == r["score"][p]
