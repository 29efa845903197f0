"""GPU tests of the ranked OTI (crp.hip k_oti_rank, k_pair_oti's pick, k_oti_fold under acoss_oti_ranked
and the seven entries ending in 3) against the restatement tests/multi_oti_np.py. Everything compares
with `==`: every shift and dot (as bits), every cell of every mask, threshold and distance, every
score, winner, segment, path cell and CRQA integer; ENTR alone at rtol 1e-11, as in
tests/test_gpu_rqa.py (a float64 sum of logs, a few ulp on either side).

Inputs are tracks of otib_np.hard_tracks(200, 5) (phrases in random keys, covers rolled on the chroma
axis) cut to 40 .. 200 frames, with the constructed tie cases; at most 16 pairs per batch."""
import ctypes

import numpy as np
import pytest

import multi_oti_np as mo
import otib_np
import rqa_np
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

BINARIZE = ("percentile", "oti")


def _host(r):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def _params(binarize="percentile", m=9, tau=1, oti=True, **kw):
    return _lib.crp_params(m=m, tau=tau, oti=oti, binarize=binarize, oti_rank=1, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- acoss_oti_ranked ----
def test_oti_ranked_against_the_exact_chain():
    tracks, _ = otib_np.hard_tracks(200, 5)
    rng = np.random.Generator(np.random.PCG64(21))
    bank = [np.ascontiguousarray(tracks[t][:int(rng.integers(40, 201))]) for t in range(24)]
    K, _ = mo.constant_pair()
    R6 = mo.roll6_invariant_track()
    X, R5 = otib_np.roll5_track()
    Z = np.zeros((45, 12), np.float32)
    first = len(bank)
    bank += [K, R6, X, R5, Z]
    iK, iR6, iX, iR5, iZ = range(first, first + 5)
    pairs = [(2 * p, 2 * p + 1) for p in range(12)] + [(2 * p + 1, 2 * p) for p in range(12)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, 24, (30, 2))]
    special = [(iK, iK), (iR6, iR6), (iX, iR5), (iR5, iX), (iZ, 3), (3, iZ), (iZ, iZ), (iK, 5)]
    pairs = np.array(pairs + special, np.int32)
    assert 55 <= len(pairs) <= 70
    feats, off, lens = synthetic.pack(bank)
    got = _host(_lib.oti_ranked(feats, off, lens, pairs))
    assert got["shifts"].shape == got["dots"].shape == (len(pairs), 12)
    first_picks = set()
    for p, (a, b) in enumerate(pairs):
        order, d = mo.ranked_tracks(bank[a], bank[b])
        np.testing.assert_array_equal(got["shifts"][p], order, err_msg="pair %d (%d, %d)" % (p, a, b))
        np.testing.assert_array_equal(_bits(got["dots"][p]), _bits(d), err_msg="pair %d (%d, %d)" % (p, a, b))
        first_picks.add(int(order[0]))
    assert len(first_picks) >= 6                      # the corpus is transposed material
    at = {tuple(pr): got["shifts"][len(pairs) - len(special) + s] for s, pr in enumerate(special)}
    np.testing.assert_array_equal(at[iK, iK], np.arange(12))
    np.testing.assert_array_equal(at[iZ, 3], np.arange(12))
    np.testing.assert_array_equal(at[iZ, iZ], np.arange(12))
    assert tuple(at[iR6, iR6][:2]) == (0, 6)
    assert (5 + at[iX, iR5][0]) % 12 == 0             # rolling the reference by 7 undoes its roll by 5
    only = _host(_lib.oti_ranked(feats, off, lens, pairs, dots=False))
    assert set(only) == {"shifts"}
    np.testing.assert_array_equal(only["shifts"], got["shifts"])


# ---- acoss_crp_pair3 ----
@pytest.mark.parametrize("m,tau", [(9, 1), (5, 2)])
@pytest.mark.parametrize("binarize", BINARIZE)
def test_pair3_at_all_twelve_picks(m, tau, binarize):
    X, Y = mo.hard_cut(0, 70, 1, 100)
    order, _ = mo.ranked_tracks(X, Y)
    masks = set()
    for pick in range(12):
        want = mo.pick_at(X, Y, pick, m, tau, 0.095, binarize, 1, order)
        got = _host(_lib.crp_pair(X, Y, _lib.crp_params3(_params(binarize, m, tau), oti_pick=pick)))
        assert set(got) == set(want), (pick, sorted(got))
        assert int(got.pop("oti")[0]) == want.pop("oti") == order[pick]
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg="pick %d %s" % (pick, key))
        masks.add(want["crp"].tobytes())
    # twelve transpositions, twelve masks (an OTI-binary mask may be empty at two unlikely shifts)
    assert len(masks) >= (12 if binarize == "percentile" else 11)


# ---- the batch entries ----
def _batch_tracks():
    tracks, _ = otib_np.hard_tracks(200, 5)
    cuts = ((0, 150), (1, 120), (12, 160), (13, 140), (4, 160), (5, 140), (28, 90), (29, 200), (7, 40), (50, 64))
    bank = [np.ascontiguousarray(tracks[t][:n]) for t, n in cuts]
    return bank + [mo.constant_pair()[0], mo.roll6_invariant_track()]


PAIRS = np.array([(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6), (8, 9), (9, 8), (0, 3), (2, 5),
                  (10, 10), (11, 11), (8, 7), (7, 8)], np.int32)
CONST, ROLL6 = 12, 13   # rows of PAIRS


@pytest.fixture(scope="module")
def batch():
    """12 tracks of 40 .. 200 frames and 16 ordered pairs (queries longer and shorter than references),
    the 150 / 120 cut of tracks 0 and 1 first; per binarisation and pair the twelve picks restated with
    their scores."""
    bank = _batch_tracks()
    lens = [len(t) for t in bank]
    assert 12 <= len(PAIRS) <= 16 and min(lens) >= 40 and max(lens) <= 330
    longer = [lens[a] > lens[b] for a, b in PAIRS]
    assert any(longer) and not all(longer)
    rows = {b: [mo.scored_picks(bank[a], bank[c], 12, binarize=b) for a, c in PAIRS] for b in BINARIZE}
    feats, off, ln = synthetic.pack(bank)
    return {"bank": bank, "args": (feats, off, ln, int(ln.max()), PAIRS), "rows": rows}


def _want_best(rows, n):
    q = [mo.best_of(r, "qmax", n) for r in rows]
    d = [mo.best_of(r, "dmax", n) for r in rows]
    return {"qmax": np.array([v[0] for v in q], np.float32), "oti": np.array([v[1] for v in q], np.int32),
            "pick_q": np.array([v[2] for v in q], np.int32), "dmax": np.array([v[0] for v in d], np.float32),
            "oti_d": np.array([v[1] for v in d], np.int32), "pick_d": np.array([v[2] for v in d], np.int32)}


@pytest.mark.parametrize("binarize", BINARIZE)
@pytest.mark.parametrize("n_oti", [1, 2, 3, 12])
def test_align3_best_of_n(batch, binarize, n_oti):
    want = _want_best(batch["rows"][binarize], n_oti)
    got = _host(_lib.crp_align(*batch["args"], _lib.crp_params3(_params(binarize), n_oti=n_oti), qmax=True, dmax=True))
    assert set(got) == set(want)
    for key in want:
        print(binarize, n_oti, key, got[key].tolist())
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    if n_oti > 1:   # from the restatement: the input is one where the later picks change the answer
        assert (want["pick_q"] > 0).any() and (want["pick_d"] > 0).any()
        assert (want["qmax"] > _want_best(batch["rows"][binarize], 1)["qmax"]).any()
    else:
        assert not want["pick_q"].any() and not want["pick_d"].any()
    if binarize == "percentile" and n_oti >= 2:   # the 150 / 120 cut: 17.5 at the OTI, 68.5 at the second pick
        assert (got["qmax"][0], got["pick_q"][0], got["oti"][0]) == (68.5, 1, 5)
    same = _host(_lib.crp_align(*batch["args"], _params(binarize), qmax=True, dmax=True, n_oti=n_oti))
    for key in (want if n_oti > 1 else ("qmax", "dmax")):
        np.testing.assert_array_equal(same[key], want[key], err_msg=key)


@pytest.mark.parametrize("binarize", BINARIZE)
def test_ties_go_to_the_first_pick(batch, binarize):
    rows = batch["rows"][binarize]
    assert len({r["qmax"] for r in rows[CONST]}) == 1 and len({r["dmax"] for r in rows[CONST]}) == 1
    assert rows[ROLL6][0]["qmax"] == rows[ROLL6][1]["qmax"] > 0
    assert (rows[ROLL6][0]["oti"], rows[ROLL6][1]["oti"]) == (0, 6)
    np.testing.assert_array_equal(rows[ROLL6][0]["crp"], rows[ROLL6][1]["crp"])
    got = _host(_lib.crp_align(*batch["args"], _params(binarize), qmax=True, dmax=True, n_oti=12))
    for p in (CONST, ROLL6):
        assert (got["pick_q"][p], got["pick_d"][p], got["oti"][p], got["oti_d"][p]) == (0, 0, 0, 0)


def test_one_output_at_a_time(batch):
    want = _want_best(batch["rows"]["percentile"], 3)
    feats, off, lens, max_len, pairs = batch["args"]
    torch = _lib._torch()
    lib = _lib.load_library()
    keep, P, lead = _lib._bank_args(feats, off, lens, max_len, pairs, _lib.crp_params3(_params(), n_oti=3))
    for slot, key in enumerate(("qmax", "dmax", "oti", "oti_d", "pick_q", "pick_d")):
        out = torch.full((P,), -7, dtype=torch.float32 if slot < 2 else torch.int32, device="cuda")
        ptrs = [None] * 6
        ptrs[slot] = _lib._ptr(out)
        assert lib.acoss_crp_align3(*lead, *ptrs, _lib._stream()) == 0
        np.testing.assert_array_equal(out.cpu().numpy(), want[key], err_msg=key)


@pytest.mark.parametrize("binarize", BINARIZE)
def test_one_transposition_through_3_is_the_entry_ending_in_2(batch, binarize):
    args = batch["args"]
    p2 = _lib.CrpParams2(_lib.crp_params(), _lib.BINARIZE[binarize], 1)
    p3 = _lib.crp_params3(p2)
    assert (p3.n_oti, p3.oti_pick) == (1, 0)
    old = _host(_lib.crp_align(*args, p2, qmax=True, dmax=True, oti=True))
    new = _host(_lib.crp_align(*args, p3, qmax=True, dmax=True))
    for key in old:
        np.testing.assert_array_equal(_bits(new[key]) if key != "oti" else new[key],
                                      _bits(old[key]) if key != "oti" else old[key], err_msg=key)
    np.testing.assert_array_equal(new["oti_d"], old["oti"])
    assert not new["pick_q"].any() and not new["pick_d"].any()
    if binarize == "percentile":
        plain = _host(_lib.crp_align(*args, _lib.crp_params(), qmax=True, dmax=True, oti=True))
        for key in plain:
            np.testing.assert_array_equal(new[key], plain[key], err_msg=key)
    L = _lib.stacked_len(args[3])
    for align in (0, 1):
        for fn in (_lib.crp_locate, _lib.crp_path):
            a, b = _host(fn(*args, p3, align=align)), _host(fn(*args, p2, align=align))
            assert set(a) == set(b)
            for key in b:
                np.testing.assert_array_equal(a[key], b[key], err_msg="%s %s" % (fn.__name__, key))
    a, b = (_host(_lib.crp_rqa(*args, p, lmin=2, smax=True, hist_cap=L + 1)) for p in (p3, p2))
    for key in b:
        np.testing.assert_array_equal(a[key], b[key], err_msg="rqa %s" % key)
    X, Y = batch["bank"][0], batch["bank"][1]
    a, b = _host(_lib.crp_pair(X, Y, p3)), _host(_lib.crp_pair(X, Y, p2))
    assert set(a) == set(b)
    for key in b:
        np.testing.assert_array_equal(a[key], b[key], err_msg="pair %s" % key)


PICKS = (np.arange(len(PAIRS), dtype=np.int32) * 3 + 1) % 4   # 1, 0, 3, 2, ...: differs from pair to pair


@pytest.fixture(scope="module")
def picked(batch):
    """Per binarisation and pair: the mask at the pair's pick of PICKS with what the aligners make of it."""
    assert set(PICKS.tolist()) == {0, 1, 2, 3}
    out = {}
    for b in BINARIZE:
        rows = []
        for p, r in enumerate(batch["rows"][b]):
            at = r[PICKS[p]]
            rows.append(dict(otib_np.aligned(at["crp"]), oti=at["oti"]))
        out[b] = rows
    return out


@pytest.mark.parametrize("binarize", BINARIZE)
def test_locate3_and_path3_with_a_pick_plane(batch, picked, binarize):
    want = picked[binarize]
    for align, key, seg, path in ((0, "qmax", "qseg", "qpath"), (1, "dmax", "dseg", "dpath")):
        loc = _host(_lib.crp_locate(*batch["args"], _params(binarize), align=align, picks=PICKS))
        np.testing.assert_array_equal(loc["oti"], [r["oti"] for r in want])
        np.testing.assert_array_equal(loc[key], np.array([r[key] for r in want], np.float32))
        np.testing.assert_array_equal(loc["seg"], np.array([r[seg] for r in want], np.int32))
        got = _host(_lib.crp_path(*batch["args"], _params(binarize), align=align, picks=PICKS))
        np.testing.assert_array_equal(got["oti"], loc["oti"])
        np.testing.assert_array_equal(got[key], loc[key])
        np.testing.assert_array_equal(got["seg"], loc["seg"])
        np.testing.assert_array_equal(np.diff(got["path_off"]), [len(r[path]) for r in want])
        np.testing.assert_array_equal(got["cells"], np.concatenate([r[path] for r in want]).reshape(-1, 2))
        assert len(got["cells"])
    # the picks changed the answer: not what the entry ending in 2 locates
    first = _host(_lib.crp_locate(*batch["args"], _params(binarize), align=1))
    assert (first["oti"] != loc["oti"]).any() and (first["seg"] != loc["seg"]).any()


@pytest.mark.parametrize("binarize", BINARIZE)
def test_rqa3_with_a_pick_plane(batch, picked, binarize):
    want = picked[binarize]
    L = _lib.stacked_len(batch["args"][3])
    got = _host(_lib.crp_rqa(*batch["args"], _params(binarize), lmin=2, smax=True, hist_cap=L + 1, picks=PICKS))
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


def test_a_scalar_pick_is_a_constant_plane(batch):
    p3 = _lib.crp_params3(_params(), oti_pick=2)
    a = _host(_lib.crp_locate(*batch["args"], p3))
    b = _host(_lib.crp_locate(*batch["args"], _params(), picks=np.full(len(PAIRS), 2, np.int32)))
    for key in b:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    np.testing.assert_array_equal(a["oti"], [r[2]["oti"] for r in batch["rows"]["percentile"]])
    np.testing.assert_array_equal(a["qmax"], np.array([r[2]["qmax"] for r in batch["rows"]["percentile"]], np.float32))


@pytest.mark.parametrize("binarize", BINARIZE)
def test_small_dp_batches_give_the_same(batch, binarize, monkeypatch):
    one = _host(_lib.crp_align(*batch["args"], _params(binarize), qmax=True, dmax=True, n_oti=3))
    loc = _host(_lib.crp_locate(*batch["args"], _params(binarize), picks=PICKS))
    monkeypatch.setenv("ACOSS_BATCH_PAIRS", "5")
    many = _host(_lib.crp_align(*batch["args"], _params(binarize), qmax=True, dmax=True, n_oti=3))
    want = _want_best(batch["rows"][binarize], 3)
    for key in want:
        np.testing.assert_array_equal(many[key], one[key], err_msg=key)
        np.testing.assert_array_equal(many[key], want[key], err_msg=key)
    loc5 = _host(_lib.crp_locate(*batch["args"], _params(binarize), picks=PICKS))
    for key in loc:
        np.testing.assert_array_equal(loc5[key], loc[key], err_msg=key)


def _refused(fn, *a, **kw):
    with pytest.raises(_lib.AcossHipError, match="ACOSS_E_ARG"):
        fn(*a, **kw)


def test_refusals(batch):
    args = batch["args"]
    X, Y = batch["bank"][0], batch["bank"][1]
    P3 = _lib.crp_params3
    for binarize in BINARIZE:
        on, off = _params(binarize), _params(binarize, oti=False)
        for n in (0, 13, -1):
            _refused(_lib.crp_align, *args, P3(on, n_oti=n))
        _refused(_lib.crp_align, *args, P3(on, n_oti=2, oti_pick=1))
        _refused(_lib.crp_align, *args, P3(on, oti_pick=1))               # align3 takes no pick
        for bad in (P3(on, n_oti=2), P3(on, oti_pick=12), P3(on, oti_pick=-1), P3(on, n_oti=0)):
            for align in (0, 1):
                _refused(_lib.crp_locate, *args, bad, align=align)
                _refused(_lib.crp_path, *args, bad, align=align)
            _refused(_lib.crp_rqa, *args, bad)
            _refused(_lib.crp_pair, X, Y, bad)
        # oti = 0 has no ranking
        _refused(_lib.crp_align, *args, P3(off, n_oti=2))
        _refused(_lib.crp_locate, *args, P3(off, oti_pick=1))
        _refused(_lib.crp_locate, *args, off, picks=np.zeros(len(PAIRS), np.int32))
        _refused(_lib.crp_path, *args, P3(off, oti_pick=3))
        _refused(_lib.crp_rqa, *args, off, picks=np.zeros(len(PAIRS), np.int32))
        _refused(_lib.crp_pair, X, Y, P3(off, oti_pick=1))
        # but oti = 0 at one transposition is the entry ending in 2
        a, b = _host(_lib.crp_align(*args, P3(off), qmax=True)), _host(_lib.crp_align(*args, off, qmax=True))
        np.testing.assert_array_equal(a["qmax"], b["qmax"])
        assert not a["oti"].any()
        # a pick plane holding 12, or -1
        for v in (12, -1):
            plane = PICKS.copy()
            plane[7] = v
            for align in (0, 1):
                _refused(_lib.crp_locate, *args, on, align=align, picks=plane)
                _refused(_lib.crp_path, *args, on, align=align, picks=plane)
            _refused(_lib.crp_rqa, *args, on, picks=plane)
        # and the flag does not stick: the next call with a good plane passes
        _lib.crp_locate(*args, on, picks=PICKS)
    with pytest.raises(ValueError):
        _lib.crp_locate(*args, _params(), picks=PICKS[:5])
    # NULL params
    lib = _lib.load_library()
    keep, P, lead = _lib._bank_args(*args, P3(_params()))
    assert lib.acoss_crp_align3(*lead[:7], None, None, None, None, None, None, None, _lib._stream()) == -1
    feats, off, lens, _, pairs = args
    torch = _lib._torch()
    out = torch.zeros((len(PAIRS), 12), dtype=torch.int32, device="cuda")
    assert lib.acoss_oti_ranked(lead[0], lead[1], lead[2], lead[3], lead[5], P, None, None, _lib._stream()) == -1
    assert lib.acoss_oti_ranked(lead[0], lead[1], lead[2], lead[3], lead[5], -1, _lib._ptr(out), None,
                                _lib._stream()) == -1
    assert lib.acoss_oti_ranked(lead[0], lead[1], lead[2], lead[3], lead[5], 0, _lib._ptr(out), None,
                                _lib._stream()) == 0
