"""GPU tests of acoss_simple_self_profile: the SiMPle self-join per track, its motif and discord.

sslen = 10 runs k_simple_mfma<1, 1> at every length, sslen = 7 k_simple_pair<1, 1> (simple.hip).
Bars: mp, mpi, motif and discord bit-equal to the numpy restatement of the definition
(tests/simple_self_np.py, pinned to the oracle-pinned simple_profile_np by
tests/test_simple_self_host.py) on small tracks; at length, where the rational-arithmetic
restatement is too slow, against a plain float64 numpy distance matrix D with the band masked,
with test_gpu_simple_profile.py's derived tolerance (a distance is about 40 roundings of values of
magnitude <= 20, about 9e-14 per evaluation; two evaluations differ by at most twice that; 1e-12
is five times above): |D[i, mpi[i]] - mp[i]| <= 1e-12 and min_j D[i, j] >= mp[i] - 1e-12; the
closure mp[mpi[i]] <= mp[i], exact because dist(i, j) == dist(j, i) bit for bit; and exact zeros
and indices where the answer is planted."""
import ctypes

import numpy as np
import pytest

from simple_profile_np import dist_matrix, frame_dots, unit_columns
from simple_self_np import masked_profile_np, motif_discord_np, self_dist_np

pytestmark = pytest.mark.gpu

TOL = 1e-12
SSLENS = [10, 7]


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


def _rows(r, e):
    return r["mp"][r["off"][e]:r["off"][e + 1]], r["mpi"][r["off"][e]:r["off"][e + 1]]


def _excl(sslen, excl):
    return sslen // 2 if excl is None else excl


def _check_motif(r, e):
    mp, mpi = _rows(r, e)
    motif, discord = motif_discord_np(mp, mpi)
    assert tuple(r["motif"][e]) == motif and r["discord"][e] == discord, e


# ------------------------------------------------------------------ 1. exact, small tracks
# at sslen 10: P = 0, 1, 2 rows; 138 columns: P - 1 = 128, so diagonal 0 is lane 0 of the second
# 128-diagonal group and the band straddles a group edge; 150: three groups
SMALL_LENS = [9, 10, 11, 16, 23, 37, 64, 138, 150]


@pytest.fixture(scope="module")
def small():
    """The tracks, their frame dots (they depend on neither sslen nor excl, and forming them in
    rational arithmetic is what takes the time) and, per (track, sslen), the distance matrix."""
    rng = np.random.default_rng(123)
    feats = [unit_columns(rng, n) for n in SMALL_LENS]
    dots = [frame_dots(f, f) for f in feats]
    dist = {(t, L): self_dist_np(feats[t], L, dots[t])
            for t in range(len(feats)) for L in SSLENS if SMALL_LENS[t] - L + 1 > 0}
    return feats, dist


@pytest.mark.parametrize("excl", [0, 4, 5, 30, None])
@pytest.mark.parametrize("sslen", SSLENS)
def test_exact_vs_restatement(lib, small, sslen, excl):
    feats, dist = small
    r = _np(lib.simple_self_profile(feats, sslen=sslen, excl=excl))
    assert np.array_equal(r["off"], lib.simple_self_profile_offsets(SMALL_LENS, np.arange(len(feats)), sslen))
    assert r["mp"].dtype == np.float64 and r["mpi"].dtype == np.int32 and len(r["mp"]) == len(r["mpi"]) == r["off"][-1]
    assert r["motif"].dtype == np.int32 and r["motif"].shape == (len(feats), 2)
    assert r["discord"].dtype == np.int32 and r["discord"].shape == (len(feats),)
    for t, n in enumerate(SMALL_LENS):
        gmp, gmpi = _rows(r, t)
        assert len(gmp) == max(n - sslen + 1, 0)
        if len(gmp) == 0:
            assert tuple(r["motif"][t]) == (-1, -1) and r["discord"][t] == -1
            continue
        mp, mpi = masked_profile_np(dist[t, sslen], _excl(sslen, excl))
        assert _same(gmp, mp), (n, np.flatnonzero(~((gmp == mp) | (np.isnan(gmp) & np.isnan(mp)))))
        assert np.array_equal(gmpi, mpi), (n, np.flatnonzero(gmpi != mpi))
        motif, discord = motif_discord_np(mp, mpi)
        assert tuple(r["motif"][t]) == motif and r["discord"][t] == discord, n
        if len(gmp) - 1 <= _excl(sslen, excl):
            assert np.isnan(gmp).all() and (gmpi == -1).all() and motif == (-1, -1) and discord == -1


# ------------------------------------------------------------------ 2. planted exact answer
@pytest.mark.parametrize("sslen", SSLENS)
def test_planted_copies(lib, sslen):
    """Three copies of a 30-column cut at columns 20, 75 and 122 of a 164-column track: the rows of
    the first copy are at distance exactly 0 from the second, the rows of the other two from the
    first (the smallest admissible column, never the row itself)."""
    rng = np.random.default_rng(231)
    cut = unit_columns(rng, 30)
    A = np.concatenate([unit_columns(rng, 20), cut, unit_columns(rng, 25), cut, unit_columns(rng, 17), cut,
                        unit_columns(rng, 12)], axis=1)
    assert A.shape[1] == 164
    r = _np(lib.simple_self_profile([A], sslen=sslen))
    w = np.arange(30 - sslen + 1)
    for start, to in ((20, 75), (75, 20), (122, 20)):
        assert np.array_equal(r["mp"][start + w].view(np.int64), np.zeros(len(w), np.int64)), start
        assert np.array_equal(r["mpi"][start + w], to + w), start
    assert (r["mp"][:20] > 0).all()
    assert tuple(r["motif"][0]) == (20, 75)
    _check_motif(r, 0)


# ------------------------------------------------------------------ 3. at length
@pytest.mark.parametrize("n", [513, 1300, 4096])
@pytest.mark.parametrize("sslen", SSLENS)
def test_at_length(lib, sslen, n):
    A = unit_columns(np.random.default_rng(n), n)
    excl = 37 if n == 1300 else sslen // 2
    r = _np(lib.simple_self_profile([A], sslen=sslen, excl=None if n != 1300 else excl))
    mp, mpi = r["mp"], r["mpi"]
    P = n - sslen + 1
    assert len(mp) == P and not np.isnan(mp).any()
    D = dist_matrix(A, A, sslen)
    i = np.arange(P)
    D[np.abs(i[:, None] - i[None, :]) <= excl] = np.inf
    assert (mpi >= 0).all() and (mpi < P).all() and (np.abs(mpi - i) > excl).all()
    assert np.abs(D[i, mpi] - mp).max() <= TOL
    assert (D.min(axis=1) >= mp - TOL).all()
    assert (mp[mpi] <= mp).all()  # closure: row mpi[i] has row i among its admissible columns
    _check_motif(r, 0)


# ------------------------------------------------------------------ 4. silent track: all ties
@pytest.mark.parametrize("excl", [None, 0, 128])
@pytest.mark.parametrize("sslen", SSLENS)
def test_silent_track(lib, sslen, excl):
    """Every distance of a silent track is 0: the contention case of the second walk, and the
    smallest admissible column everywhere."""
    Z = np.zeros((12, 300))
    r1 = _np(lib.simple_self_profile([Z], sslen=sslen, excl=excl))
    r2 = _np(lib.simple_self_profile([Z], sslen=sslen, excl=excl))
    for key in ("mp", "mpi", "motif", "discord"):
        assert np.array_equal(r1[key].view(np.int64 if key == "mp" else np.int32),
                              r2[key].view(np.int64 if key == "mp" else np.int32)), key
    P, e = 300 - sslen + 1, _excl(sslen, excl)
    i = np.arange(P)
    assert np.array_equal(r1["mp"].view(np.int64), np.zeros(P, np.int64))
    assert np.array_equal(r1["mpi"], np.where(i > e, 0, e + 1 + i))
    assert tuple(r1["motif"][0]) == (0, e + 1) and r1["discord"][0] == 0


# ------------------------------------------------------------------ 5. NaN column
@pytest.mark.parametrize("sslen", SSLENS)
def test_nan_column(lib, sslen):
    A = unit_columns(np.random.default_rng(251), 420)
    c = 133
    An = A.copy()
    An[:, c] = np.nan
    r = _np(lib.simple_self_profile([A, An], sslen=sslen))
    clean_mp, clean_mpi = _rows(r, 0)
    mp, mpi = _rows(r, 1)
    hit = np.zeros(len(mp), bool)
    hit[c - sslen + 1:c + 1] = True  # the subsequences whose window holds column c
    assert np.isnan(mp[hit]).all() and (mpi[hit] == -1).all()
    assert not np.isnan(mp[~hit]).any() and (mpi[~hit] >= 0).all()
    assert not hit[mpi[~hit]].any()
    keep = ~hit & ~hit[clean_mpi]  # the clean row's nearest subsequence is still there
    assert keep.sum() > 300
    assert np.array_equal(mp[keep], clean_mp[keep]) and np.array_equal(mpi[keep], clean_mpi[keep])
    moved = ~hit & hit[clean_mpi]
    assert (mp[moved] >= clean_mp[moved]).all()
    _check_motif(r, 0)
    _check_motif(r, 1)


# ------------------------------------------------------------------ 6. list semantics
@pytest.mark.parametrize("sslen", SSLENS)
def test_list_semantics(lib, monkeypatch, sslen):
    """An entry's ranges depend on its track alone: listed twice, in a list that names only some
    of the tracks, with tracks that have no row mixed in, one at a time, and across launches of
    three entries (ACOSS_SIMPLE_PROFILE_BATCH)."""
    rng = np.random.default_rng(271)
    lens = [40, 300, 12, 150, 8, 77, 5]
    feats = [unit_columns(rng, n) for n in lens]
    tracks = np.array([3, 1, 4, 3, 5, 6, 1], np.int32)  # tracks 0 and 2 unnamed; 6 (and 4 at sslen 10) without rows
    r = _np(lib.simple_self_profile(feats, tracks, sslen=sslen))
    assert np.array_equal(np.diff(r["off"]), np.maximum(np.array(lens)[tracks] - sslen + 1, 0))
    for a, b in ((0, 3), (1, 6)):
        assert _same(_rows(r, a)[0], _rows(r, b)[0]) and np.array_equal(_rows(r, a)[1], _rows(r, b)[1])
        assert np.array_equal(r["motif"][a], r["motif"][b]) and r["discord"][a] == r["discord"][b]
    assert tuple(r["motif"][5]) == (-1, -1) and r["discord"][5] == -1
    for e in range(len(tracks)):
        one = _np(lib.simple_self_profile(feats, tracks[e:e + 1], sslen=sslen))
        mp, mpi = _rows(r, e)
        assert _same(one["mp"], mp) and np.array_equal(one["mpi"], mpi), e
        assert np.array_equal(one["motif"][0], r["motif"][e]) and one["discord"][0] == r["discord"][e], e
    every = _np(lib.simple_self_profile(feats, sslen=sslen))  # tracks=None: every track, in order
    for e, t in enumerate(tracks):
        assert _same(_rows(every, t)[0], _rows(r, e)[0]) and np.array_equal(_rows(every, t)[1], _rows(r, e)[1])
    monkeypatch.setenv("ACOSS_SIMPLE_PROFILE_BATCH", "3")
    rb = _np(lib.simple_self_profile(feats, tracks, sslen=sslen))
    for key in ("off", "mpi", "motif", "discord"):
        assert np.array_equal(r[key], rb[key]), key
    assert _same(r["mp"], rb["mp"])


# ------------------------------------------------------------------ 7. refusals
def test_refusals(lib):
    import torch
    L = lib.load_library()
    rng = np.random.default_rng(281)
    feats = [unit_columns(rng, n) for n in [30, 50, 20]]
    flat = torch.from_numpy(np.concatenate([f.ravel() for f in feats])).cuda()
    lens = np.array([30, 50, 20], np.int32)
    toff = torch.from_numpy(np.array([0, 12 * 30, 12 * 80], np.int64)).cuda()
    tlen = torch.from_numpy(lens).cuda()
    good = lib.simple_self_profile_offsets(lens, [0, 1, 2], 10)  # 0, 21, 62, 73

    def call(off, total, sslen=10, max_len=50, excl=5, tracks=(0, 1, 2), n_tracks=3):
        mp = torch.full((80,), -7.0, dtype=torch.float64, device="cuda")
        mpi = torch.full((80,), -7, dtype=torch.int32, device="cuda")
        motif = torch.full((3, 2), -7, dtype=torch.int32, device="cuda")
        discord = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        off_d = torch.from_numpy(np.asarray(off, np.int64)).cuda()
        trk = torch.from_numpy(np.asarray(tracks, np.int32)).cuda()
        rc = L.acoss_simple_self_profile(flat.data_ptr(), toff.data_ptr(), tlen.data_ptr(), n_tracks, max_len,
                                         trk.data_ptr(), 3, sslen, excl, off_d.data_ptr(), total, mp.data_ptr(),
                                         mpi.data_ptr(), motif.data_ptr(), discord.data_ptr(),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        untouched = bool((mp == -7).all() and (mpi == -7).all() and (motif == -7).all() and (discord == -7).all())
        return rc, untouched, L.acoss_last_error().decode()

    rc, untouched, _ = call(good, 73)
    assert rc == 0 and not untouched
    rc, untouched, msg = call(good, 73, excl=-1)
    assert rc == -1 and untouched and "excl" in msg
    rc, untouched, _ = call(good, 73, sslen=17)
    assert rc == -1 and untouched
    rc, untouched, _ = call(good, 73, sslen=0)
    assert rc == -1 and untouched
    rc, untouched, _ = call(good, 73, max_len=4097)
    assert rc == -2 and untouched
    rc, untouched, msg = call([0, 21, 61, 73], 73)  # entry 1 needs 41 rows, has 40
    assert rc == -1 and untouched and "entry 1" in msg
    rc, untouched, msg = call(good, 72)  # prof_total too small for the last entry
    assert rc == -1 and untouched and "entry 2" in msg
    rc, untouched, msg = call([-1, 21, 62, 73], 73)
    assert rc == -1 and untouched and "entry 0" in msg
    rc, untouched, msg = call(good, 73, tracks=(0, 3, 2))
    assert rc == -1 and untouched and "entry 1" in msg
    rc, untouched, msg = call(good, 73, tracks=(0, 1, -1))
    assert rc == -1 and untouched and "entry 2" in msg
    rc, untouched, msg = call(good, 73, tracks=(2, 1, 0), n_tracks=2)  # index 2 outside [0, 2)
    assert rc == -1 and untouched and "entry 0" in msg
    with pytest.raises(ValueError):
        lib.simple_self_profile(feats, excl=-1)
    # without the optional outputs the profile alone is written
    mp = torch.full((73,), -7.0, dtype=torch.float64, device="cuda")
    mpi = torch.full((73,), -7, dtype=torch.int32, device="cuda")
    off_d = torch.from_numpy(good).cuda()
    trk = torch.from_numpy(np.arange(3, dtype=np.int32)).cuda()
    rc = L.acoss_simple_self_profile(flat.data_ptr(), toff.data_ptr(), tlen.data_ptr(), 3, 50, trk.data_ptr(), 3, 10, 5,
                                     off_d.data_ptr(), 73, mp.data_ptr(), mpi.data_ptr(), None, None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ref = _np(lib.simple_self_profile(feats))
    assert rc == 0 and _same(mp.cpu().numpy(), ref["mp"]) and np.array_equal(mpi.cpu().numpy(), ref["mpi"])


# ------------------------------------------------------------------ 8. the plugin
def test_plugin_self_profile(tmp_path, monkeypatch):
    from acoss import synthetic
    from acoss.algorithms.simple_silva import Simple
    from acoss.engine import subsequence_frames
    monkeypatch.chdir(tmp_path)
    tracks, labels = synthetic.make_corpus("covers80", frames=3050, seed=11)
    keep = np.flatnonzero(labels < 3)
    csv, fdir = synthetic.write_feature_dataset(str(tmp_path), [tracks[k] for k in keep], labels[keep])
    algo = Simple(csv, fdir, shortname="t", cachedir=str(tmp_path / "cache"))
    n = algo.N
    idxs = np.array([(i, j) for i in range(n) for j in range(n) if i != j][:8], np.int32)
    algo.similarity(idxs)
    before_d = np.asarray(algo.Ds["main"])[idxs[:, 0], idxs[:, 1]].copy()
    before_p = algo.profile(idxs)
    r = algo.self_profile()
    T = np.array([algo.all_feats[i].shape[1] for i in range(n)])
    rows = T - algo.SSLEN + 1
    assert np.array_equal(np.diff(r["off"]), rows) and r["mp"].shape == r["mpi"].shape == (r["off"][-1],)
    raw = _np(_lib_self(algo))
    for key in ("off", "mpi", "motif", "discord"):
        assert np.array_equal(r[key], raw[key]), key
    assert _same(r["mp"], raw["mp"])
    i = np.arange(r["off"][-1]) - np.repeat(r["off"][:-1], rows)
    assert (np.abs(r["mpi"] - i) > algo.SSLEN // 2).all()
    nf = np.repeat(algo._n_frames, rows)
    assert np.array_equal(r["frames"], subsequence_frames(i, algo.SSLEN, algo.WIN, algo.SKIP, nf))
    assert np.array_equal(r["match_frames"], subsequence_frames(r["mpi"], algo.SSLEN, algo.WIN, algo.SKIP, nf))
    assert r["motif_frames"].shape == (n, 2, 2) and r["discord_frames"].shape == (n, 2)
    for e in range(n):
        _check_motif(r, e)
        for c in range(2):
            assert np.array_equal(r["motif_frames"][e, c], subsequence_frames(
                r["motif"][e, c:c + 1], algo.SSLEN, algo.WIN, algo.SKIP, algo._n_frames[e])[0])
        assert np.array_equal(r["discord_frames"][e], subsequence_frames(
            r["discord"][e:e + 1], algo.SSLEN, algo.WIN, algo.SKIP, algo._n_frames[e])[0])
    # a list of songs, one of them twice, and an exclusion zone that leaves nothing
    sub = algo.self_profile([2, 0, 2], excl=3)
    assert np.array_equal(np.diff(sub["off"]), rows[[2, 0, 2]])
    assert np.array_equal(sub["motif"][0], sub["motif"][2]) and np.array_equal(sub["frames"][:rows[2]],
                                                                               r["frames"][r["off"][2]:r["off"][3]])
    none = algo.self_profile([1], excl=int(rows[1]))
    assert np.isnan(none["mp"]).all() and (none["mpi"] == -1).all() and (none["match_frames"] == -1).all()
    assert (none["motif_frames"] == -1).all() and (none["discord_frames"] == -1).all()
    assert (none["frames"] >= 0).all()
    # the object's scores and cross profiles are what they were
    algo.similarity(idxs)
    assert np.array_equal(np.asarray(algo.Ds["main"])[idxs[:, 0], idxs[:, 1]], before_d)
    after_p = algo.profile(idxs)
    for key in before_p:
        assert _same(before_p[key], after_p[key]), key


def _lib_self(algo):
    from acoss import _lib
    out, off, T = algo._packed
    return _lib.simple_self_profile_packed(out, off, T, np.arange(algo.N, dtype=np.int32), algo.SSLEN)
