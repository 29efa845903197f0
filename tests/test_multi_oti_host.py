"""CPU tests of the ranked OTI: known answers of the restatement tests/multi_oti_np.py (the definition
in include/acoss_hip.h, acoss_crp_params3) and the host logic around it: the params struct and the
entries the binding picks, the cache and result names, the ValueErrors. No GPU."""
import ctypes

import numpy as np
import pytest

import multi_oti_np as mo
import oracle
import otib_np
from acoss import _lib, coverid
from acoss.algorithms.latefusion_chen import ChenFusion
from acoss.algorithms.rqa_serra09 import Serra09


def _cuts():
    """36 pairs of hard_tracks(200, 5) cut to 40 .. 200 frames, queries longer and shorter."""
    tracks, _ = otib_np.hard_tracks(200, 5)
    rng = np.random.Generator(np.random.PCG64(9))
    out = []
    for p in range(36):
        a, b = (2 * p, 2 * p + 1) if p < 18 else (int(rng.integers(0, 60)), int(rng.integers(60, 120)))
        nq, nr = int(rng.integers(40, 201)), int(rng.integers(40, 201))
        out.append((np.ascontiguousarray(tracks[a][:nq]), np.ascontiguousarray(tracks[b][:nr])))
    return out


def test_pick_zero_is_the_oracles_oti_and_crp():
    for X, Y in _cuts():
        order, d = mo.ranked_tracks(X, Y)
        assert sorted(order) == list(range(12))
        assert (np.diff(d[order]) <= 0).all()
        assert order[0] == oracle.oti(oracle.profile(X), oracle.profile(Y))
        want = oracle.crp_pair(X, Y)
        at = mo.crp_at(X, Y, order[0])
        np.testing.assert_array_equal(at["crp"], want["crp"])
        assert oracle.align(at["crp"], 0.5, 0.5, 0) == want["qmax"]
        assert oracle.align(at["crp"], 0.5, 0.5, 1) == want["dmax"]


def test_the_chain_rounds_once_per_step_to_nearest_even():
    """Known answers of the exact chain and of its rounding: a unit profile picks single bins, ties
    go to even, subnormals keep their spacing."""
    e = np.zeros(12, np.float32)
    e[3] = 1.0
    p = np.arange(12, dtype=np.float32) / 16.0
    d = mo.dots(e, p)                       # dot_k = p[(3 - k) % 12], exactly
    np.testing.assert_array_equal(d, [p[(3 - k) % 12] for k in range(12)])
    # 1 + 2^-24 is the tie between 1 and 1 + 2^-23: to even, 1
    assert mo._rn32(mo.Fraction(1) + mo.Fraction(1, 2 ** 24)) == np.float32(1.0)
    assert mo._rn32(mo.Fraction(1) + mo.Fraction(3, 2 ** 25)) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert mo._rn32(mo.Fraction(1, 2 ** 150)) == 0.0
    assert mo._rn32(mo.Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148)


def test_constant_track_against_itself_ranks_the_shifts_in_order():
    K, _ = mo.constant_pair()
    order, d = mo.ranked_tracks(K, K)
    np.testing.assert_array_equal(order, np.arange(12))
    assert len(set(d.tolist())) == 1


def test_roll6_invariant_track_ranks_0_then_6_with_equal_dots():
    X = mo.roll6_invariant_track()
    np.testing.assert_array_equal(X[:, :6], X[:, 6:])
    order, d = mo.ranked_tracks(X, X)
    assert (order[0], order[1]) == (0, 6)
    assert d[0].tobytes() == d[6].tobytes()
    assert d[order[2]] < d[6]


def test_the_150_120_cut_is_won_by_the_second_transposition():
    X, Y = mo.hard_cut(0, 150, 1, 120)
    order, d = mo.ranked_tracks(X, Y)
    assert (order[0], order[1]) == (2, 5)
    rows = mo.scored_picks(X, Y, 2)
    assert (rows[0]["qmax"], rows[1]["qmax"]) == (17.5, 68.5)
    assert (rows[0]["dmax"], rows[1]["dmax"]) == (25.5, 87.0)
    assert mo.best_of(rows, "qmax") == (np.float32(68.5), 5, 1)
    assert mo.best_of(rows, "dmax") == (np.float32(87.0), 5, 1)
    assert mo.best_of(rows, "qmax", 1) == (np.float32(17.5), 2, 0)


def test_best_of_keeps_the_smallest_pick_on_a_tie():
    rows = [{"oti": 4, "q": 3.0}, {"oti": 7, "q": 5.0}, {"oti": 1, "q": 5.0}]
    assert mo.best_of(rows, "q") == (np.float32(5.0), 7, 1)
    assert mo.best_of(rows[:1] * 3, "q") == (np.float32(3.0), 4, 0)


def test_otib_at_the_first_pick_is_otib():
    X, Y = otib_np.cut_pair(90, 110)
    a, b = mo.pick_at(X, Y, 0, binarize="oti", oti_rank=2), otib_np.otib(X, Y, oti_rank=2)
    assert a["oti"] == b["oti"]
    for key in ("dist", "closer", "crp"):
        np.testing.assert_array_equal(a[key], b[key])


# ---- host logic ----
def test_crp_params3_wraps_either_struct():
    old = _lib.crp_params(m=7, tau=2)
    p = _lib.crp_params3(old, n_oti=3)
    assert type(p) is _lib.CrpParams3 and ctypes.sizeof(p) == 40
    assert _lib.CrpParams3.n_oti.offset == 32 and _lib.CrpParams3.oti_pick.offset == 36
    assert (p.m, p.tau, p.oti, p.binarize, p.oti_rank, p.n_oti, p.oti_pick) == (7, 2, 1, 0, 1, 3, 0)
    q = _lib.crp_params3(_lib.crp_params(binarize="oti", oti_rank=2), oti_pick=4)
    assert (q.binarize, q.oti_rank, q.n_oti, q.oti_pick) == (1, 2, 1, 4)
    assert _lib.crp_params3(q, n_oti=2).oti_rank == 2
    assert _lib._entry("acoss_crp_align", p) == "acoss_crp_align3"
    assert _lib._entry(_lib._aligner(1, "acoss_crp_path")[1], p) == "acoss_crp_path_dmax3"
    for name in ("locate", "locate_dmax", "path", "path_dmax", "rqa"):
        assert len(_lib.SIGNATURES["acoss_crp_%s3" % name]) == len(_lib.SIGNATURES["acoss_crp_%s2" % name]) + 1
    for name in ("align", "locate", "locate_dmax", "path", "path_dmax", "rqa", "pair"):
        assert ctypes.POINTER(_lib.CrpParams3) in _lib.SIGNATURES["acoss_crp_%s3" % name]
    assert len(_lib.SIGNATURES["acoss_crp_align3"]) == len(_lib.SIGNATURES["acoss_crp_align2"]) + 3
    assert len(_lib.SIGNATURES["acoss_crp_pair3"]) == len(_lib.SIGNATURES["acoss_crp_pair2"])
    assert "acoss_oti_ranked" in _lib.SIGNATURES


@pytest.mark.parametrize("bad", [0, 13, 2.5, True, -1])
def test_n_oti_value_errors(bad, tmp_path):
    with pytest.raises(ValueError):
        _lib.check_n_oti(bad)
    with pytest.raises(ValueError):
        Serra09.algorithm_name(n_oti=bad)
    for cls in (Serra09, ChenFusion):
        with pytest.raises(ValueError):
            cls(str(tmp_path / "none.csv"), str(tmp_path), n_oti=bad)


def test_n_oti_needs_the_oti(tmp_path):
    assert _lib.check_n_oti(1, oti=False) == 1 and _lib.check_n_oti(2.0) == 2
    with pytest.raises(ValueError, match="oti=True"):
        _lib.check_n_oti(2, oti=False)
    for cls in (Serra09, ChenFusion):
        with pytest.raises(ValueError, match="oti=True"):
            cls(str(tmp_path / "none.csv"), str(tmp_path), oti=False, n_oti=2)


def test_cache_and_result_names():
    assert _lib.n_oti_suffix() == "" and _lib.n_oti_suffix(1) == "" and _lib.n_oti_suffix(3) == "-oti3"
    assert Serra09.algorithm_name(n_oti=1) == "Serra09"
    assert Serra09.algorithm_name(n_oti=2) == "Serra09-oti2"
    assert Serra09.algorithm_name("det", n_oti=2) == "Serra09-oti2-det"
    assert Serra09.algorithm_name("det", "oti", 2, 2) == "Serra09-otib2-oti2-det"
    assert Serra09.algorithm_name("qmax", "oti", 1, 12) == "Serra09-otib-oti12"
    assert Serra09.algorithm_name("det", "oti", 2, 1) == "Serra09-otib2-det"
    assert ChenFusion.algorithm_name(n_oti=1) == "LateFusionChen"
    assert ChenFusion.algorithm_name(n_oti=3) == "LateFusionChen-oti3"
    assert ChenFusion.algorithm_name("oti", 3, 2) == "LateFusionChen-otib3-oti2"


@pytest.mark.parametrize("algorithm", ["EarlyFusionTraile", "FTM2D", "SiMPle"])
def test_benchmark_takes_n_oti_for_the_crp_scorers_only(algorithm, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="Serra09 and LateFusionChen"):
        coverid.benchmark("none.csv", str(tmp_path), algorithm=algorithm, n_oti=2)


def test_benchmark_refuses_a_bad_n_oti(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for bad in (0, 13, 2.5):
        with pytest.raises(ValueError, match="n_oti"):
            coverid.benchmark("none.csv", str(tmp_path), algorithm="Serra09", n_oti=bad)


def test_command_line_has_n_oti():
    assert coverid.parser_args(["-i", "x.csv", "--n-oti", "3"]).n_oti == 3
    assert coverid.parser_args(["-i", "x.csv"]).n_oti == 1
