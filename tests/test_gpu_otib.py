"""GPU tests of the OTI-binary CRP (crp_otib.hip k_crp_otib under the seven entries ending in 2) against
the restatement tests/otib_np.py. Everything compares with `==`: every cell of every mask, count and
distance matrix, every score, segment, path cell and CRQA integer; ENTR alone at rtol 1e-11, as in
tests/test_gpu_rqa.py (a float64 sum of logs, a few ulp on either side).

Inputs are songs and covers of acoss.synthetic.make_hard_corpus (phrases in random keys, covers
rolled on the chroma axis) cut to length. Every generated pair's restated masks at ranks 1 and 2
hold between 1 % and 90 % ones, asserted (rank 12 is all ones by definition, asserted too): the cut
of a shape is the first of a fixed sequence of offsets whose restated masks do (the restatement
alone chooses it), so a mask of 1 x 3 cells is neither empty nor full. The constructed tie cases are
exempt."""
import ctypes

import numpy as np
import pytest

import otib_np
import rqa_np
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 12)
MS = (1, 31, 32, 33, 70)          # stacked lengths that straddle a 32-row strip
NS = (3, 255, 256, 257, 300)      # and a 256-column panel


def _host(r):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def _params(m=9, tau=1, oti=True, rank=1, **kw):
    return _lib.crp_params(m=m, tau=tau, oti=oti, binarize="oti", oti_rank=rank, **kw)


def _in_range(C):
    return 0.01 <= otib_np.density(C) <= 0.90


def _restate(X, Y, m=9, tau=1):
    """The restatement by (oti, rank), OTI on and off, the three ranks."""
    return {(oti, rank): r for oti in (True, False) for rank, r in otib_np.otib_ranks(X, Y, m, tau, oti, RANKS).items()}


_TRACKS = {}


def _song_and_cover(which):
    if not _TRACKS:
        tracks, labels = synthetic.make_hard_corpus("covers80", frames=700, seed=5)
        sizes = np.bincount(labels)
        _TRACKS["cliques"] = [np.flatnonzero(labels == lab) for lab in np.flatnonzero(sizes > 1)]
        _TRACKS["tracks"] = tracks
    members = _TRACKS["cliques"][which % len(_TRACKS["cliques"])]
    return _TRACKS["tracks"][members[0]], _TRACKS["tracks"][members[1]]


def _generated_pair(Mp, Np, m, tau):
    """(X, Y, restatements by (oti, rank)) with stacked lengths (Mp, Np): the first cut of a fixed list
    whose restated masks at ranks 1 and 2, OTI on and off, hold 1 % .. 90 % ones."""
    nq, nr = otib_np.frames_for(Mp, m, tau), otib_np.frames_for(Np, m, tau)
    for which in range(6):
        A, B = _song_and_cover(which)
        for sb in range(0, len(B) - nr + 1, 3):     # a mask of a few cells needs a chord change under it
            sa = (5 * sb) % (len(A) - nq + 1)
            X = np.ascontiguousarray(A[sa:sa + nq])
            Y = np.ascontiguousarray(B[sb:sb + nr])
            ref = _restate(X, Y, m, tau)
            if all(_in_range(ref[oti, rank]["crp"]) for oti in (True, False) for rank in (1, 2)):
                return X, Y, ref
    raise AssertionError("no cut of the corpus gives %d x %d masks with 1 %% .. 90 %% ones" % (Mp, Np))


def _check_pair2(X, Y, m, tau, ref, what, generated=True):
    """acoss_crp_pair2 against the restatement for OTI on and off and the three ranks: every cell."""
    for (oti, rank), want in ref.items():
        got = _host(_lib.crp_pair(X, Y, _params(m, tau, oti, rank)))
        dens = otib_np.density(want["crp"])
        print("%s oti %d rank %d: %s cells, ones %.4f, closer max %d, g %d" % (
            what, oti, rank, want["crp"].shape, dens, int(want["closer"].max()), want["oti"]))
        assert set(got) == {"dist", "crp", "oti", "closer"}
        assert int(got["oti"][0]) == want["oti"], (what, oti, rank)
        np.testing.assert_array_equal(got["closer"], want["closer"], err_msg="%s closer" % what)
        np.testing.assert_array_equal(got["crp"], want["crp"], err_msg="%s crp" % what)
        np.testing.assert_array_equal(got["dist"], want["dist"], err_msg="%s dist" % what)
        if rank == 12:
            assert want["crp"].all()
        elif generated:
            assert 0.01 <= dens <= 0.90, (what, oti, rank, dens)


@pytest.mark.parametrize("Mp", MS)
def test_pair2_shape_grid(Mp):
    for Np in NS:
        X, Y, ref = _generated_pair(Mp, Np, 9, 1)
        assert ref[True, 1]["crp"].shape == (Mp, Np)
        _check_pair2(X, Y, 9, 1, ref, "%d x %d" % (Mp, Np))


@pytest.mark.parametrize("m,tau", [(1, 1), (5, 2), (64, 1)])
def test_pair2_other_stackings(m, tau):
    X, Y, ref = _generated_pair(70, 300, m, tau)
    assert ref[True, 1]["crp"].shape == (70, 300)
    _check_pair2(X, Y, m, tau, ref, "m %d tau %d" % (m, tau))


def _constructed():
    X, R5 = otib_np.roll5_track()
    Z = otib_np.zero_block_track()
    K = otib_np.constant_track()
    rng = np.random.Generator(np.random.PCG64(4))
    E = (rng.integers(0, 9, (60, 12)) / 8.0).astype(np.float32)
    return {"self": (X, X), "roll5": (X, R5), "zero_rows": (Z, X), "zero_cols": (X, Z), "const_ref": (X, K),
            "const_both": (K, K), "const_query_exact": (K, E)}


@pytest.mark.parametrize("name", ["self", "roll5", "zero_rows", "zero_cols", "const_ref", "const_both",
                                  "const_query_exact"])
def test_pair2_constructed_ties(name):
    X, Y = _constructed()[name]
    ref = _restate(X, Y)
    _check_pair2(X, Y, 9, 1, ref, name, generated=False)
    one = ref[False, 1]
    if name == "self":
        assert np.diagonal(one["crp"]).all()
    if name == "roll5":
        assert not np.diagonal(one["crp"]).any() and np.diagonal(ref[True, 1]["crp"]).all()
    if name == "zero_rows":
        assert one["crp"][20:24].all()
    if name == "zero_cols":
        assert one["crp"][:, 20:24].all()
    if name.startswith("const"):
        assert one["crp"].all()


# ---- the batch entries ----
LENS = (40, 75, 120, 190, 250, 300, 330, 64, 155, 47)
PAIRS = np.array([(0, 6), (6, 0), (1, 5), (5, 1), (2, 4), (4, 2), (3, 7), (7, 3), (8, 9), (9, 8), (0, 1), (6, 5),
                  (2, 8), (4, 4)], np.int32)


@pytest.fixture(scope="module")
def batch():
    """10 tracks of 40 .. 330 frames, 14 ordered pairs (queries longer and shorter than references),
    and per rank the restated mask of every pair with what the aligners make of it."""
    tracks = []
    for t, n in enumerate(LENS):
        A, B = _song_and_cover(t // 2)
        src = A if t % 2 == 0 else B
        tracks.append(np.ascontiguousarray(src[13 * t:13 * t + n]))
    assert len(PAIRS) >= 12 and min(LENS) >= 40 and max(LENS) <= 330
    longer = [LENS[a] > LENS[b] for a, b in PAIRS]
    assert any(longer) and not all(longer)
    ref = {}
    for rank in (1, 2):
        rows = []
        for a, b in PAIRS:
            r = otib_np.otib(tracks[a], tracks[b], 9, 1, True, rank)
            dens = otib_np.density(r["crp"])
            print("batch rank %d pair (%d, %d): %s cells, ones %.4f" % (rank, a, b, r["crp"].shape, dens))
            assert 0.01 <= dens <= 0.90, (rank, a, b, dens)
            r.update(otib_np.aligned(r["crp"]))
            rows.append(r)
        ref[rank] = rows
    feats, off, lens = synthetic.pack(tracks)
    return {"args": (feats, off, lens, int(lens.max()), PAIRS), "ref": ref}


@pytest.mark.parametrize("rank", [1, 2])
def test_align2_scores(batch, rank):
    got = _host(_lib.crp_align(*batch["args"], _params(rank=rank), qmax=True, dmax=True, oti=True))
    want = batch["ref"][rank]
    np.testing.assert_array_equal(got["oti"], [r["oti"] for r in want])
    np.testing.assert_array_equal(got["qmax"], np.array([r["qmax"] for r in want], np.float32))
    np.testing.assert_array_equal(got["dmax"], np.array([r["dmax"] for r in want], np.float32))
    assert (got["qmax"] > 0).any()


@pytest.mark.parametrize("rank", [1, 2])
def test_locate2_and_path2(batch, rank):
    want = batch["ref"][rank]
    for align, key, seg, path in ((0, "qmax", "qseg", "qpath"), (1, "dmax", "dseg", "dpath")):
        loc = _host(_lib.crp_locate(*batch["args"], _params(rank=rank), align=align))
        np.testing.assert_array_equal(loc[key], np.array([r[key] for r in want], np.float32))
        np.testing.assert_array_equal(loc["seg"], np.array([r[seg] for r in want], np.int32))
        np.testing.assert_array_equal(loc["oti"], [r["oti"] for r in want])
        got = _host(_lib.crp_path(*batch["args"], _params(rank=rank), align=align))
        np.testing.assert_array_equal(got[key], loc[key])
        np.testing.assert_array_equal(got["seg"], loc["seg"])
        np.testing.assert_array_equal(np.diff(got["path_off"]), [len(r[path]) for r in want])
        np.testing.assert_array_equal(got["cells"], np.concatenate([r[path] for r in want]).reshape(-1, 2))
        assert len(got["cells"])


@pytest.mark.parametrize("rank", [1, 2])
def test_rqa2(batch, rank):
    want = batch["ref"][rank]
    L = _lib.stacked_len(batch["args"][3])
    got = _host(_lib.crp_rqa(*batch["args"], _params(rank=rank), lmin=2, smax=True, hist_cap=L + 1))
    np.testing.assert_array_equal(got["oti"], [r["oti"] for r in want])
    for p, r in enumerate(want):
        q = r["rqa"]
        assert tuple(int(x) for x in got["counts"][p]) == tuple(q[k] for k in rqa_np.COUNT_KEYS), p
        assert int(got["lmax"][p]) == q["lmax"] and float(got["smax"][p]) == q["smax"], p
        for c, k in enumerate(rqa_np.STAT_KEYS[:3]):
            assert float(got["stats"][p, c]) == q[k], (p, k)
        np.testing.assert_allclose(float(got["stats"][p, 3]), q["entr"], rtol=1e-11, atol=0.0)
        np.testing.assert_array_equal(got["hist"][p, :len(q["hist"])], q["hist"])
        assert not got["hist"][p, len(q["hist"]):].any()


def test_small_dp_batches_give_the_same(batch, monkeypatch):
    one = _host(_lib.crp_align(*batch["args"], _params(rank=2), qmax=True, dmax=True, oti=True))
    monkeypatch.setenv("ACOSS_BATCH_PAIRS", "5")
    many = _host(_lib.crp_align(*batch["args"], _params(rank=2), qmax=True, dmax=True, oti=True))
    for key in one:
        np.testing.assert_array_equal(many[key], one[key], err_msg=key)


def test_percentile_through_the_wide_struct_is_the_old_entry(batch):
    """binarize = 0 through acoss_crp_align2 runs the percentile CRP, and oti_rank is ignored."""
    wide = _lib.CrpParams2(_lib.crp_params(), 0, 99)
    got = _host(_lib.crp_align(*batch["args"], wide, qmax=True, dmax=True, oti=True))
    old = _host(_lib.crp_align(*batch["args"], _lib.crp_params(), qmax=True, dmax=True, oti=True))
    for key in old:
        np.testing.assert_array_equal(got[key], old[key], err_msg=key)
    X, Y = _constructed()["roll5"]
    a, b = _host(_lib.crp_pair(X, Y, wide)), _host(_lib.crp_pair(X, Y, _lib.crp_params()))
    assert set(a) == set(b) == {"dist", "thr_row", "thr_col", "crp", "oti"}
    for key in b:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_kappa_is_not_read(batch):
    a = _host(_lib.crp_align(*batch["args"], _params(rank=1, kappa=0.095), qmax=True))
    b = _host(_lib.crp_align(*batch["args"], _params(rank=1, kappa=7.0), qmax=True))
    np.testing.assert_array_equal(a["qmax"], b["qmax"])


def test_refusals(batch):
    X, Y = _constructed()["roll5"]
    with pytest.raises(_lib.AcossHipError, match="ACOSS_E_SHAPE"):     # 9 frames: no stacked frame at m = 9
        _lib.crp_pair(X[:9], Y, _params())
    feats, off, lens, _, pairs = batch["args"]
    with pytest.raises(_lib.AcossHipError, match="ACOSS_E_SHAPE"):     # as acoss_crp_align: max_len too short
        _lib.crp_align(feats, off, lens, 9, pairs, _params(), qmax=True)
    for bad in (_lib.CrpParams2(_lib.crp_params(), 1, 0), _lib.CrpParams2(_lib.crp_params(), 1, 13),
                _lib.CrpParams2(_lib.crp_params(), 2, 1), _lib.CrpParams2(_lib.crp_params(), -1, 1)):
        with pytest.raises(_lib.AcossHipError, match="ACOSS_E_ARG"):
            _lib.crp_align(*batch["args"], bad, qmax=True)
        with pytest.raises(_lib.AcossHipError, match="ACOSS_E_ARG"):
            _lib.crp_pair(X, Y, bad)
    # thresholds do not exist under ACOSS_BIN_OTI
    torch = _lib._torch()
    lib = _lib.load_library()
    dX, dY = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    thr = torch.zeros(64, dtype=torch.float32, device="cuda")
    P = _params()
    rc = lib.acoss_crp_pair2(_lib._ptr(dX), len(X), _lib._ptr(dY), len(Y), ctypes.byref(P), None, _lib._ptr(thr), None,
                             None, None, None, _lib._stream())
    assert rc == -1
