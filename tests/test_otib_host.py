"""CPU tests of the OTI-binary CRP: known answers of the restatement tests/otib_np.py (the definition
in include/acoss_hip.h, acoss_crp_params2) and the host logic around it: the params struct the
binding picks, the cache and result names, the ValueErrors. No GPU."""
import ctypes

import numpy as np
import pytest

import oracle
import otib_np
from acoss import _lib, coverid
from acoss.algorithms.latefusion_chen import ChenFusion
from acoss.algorithms.rqa_serra09 import Serra09


def _diag(C):
    return np.diagonal(C)


def test_track_against_itself_has_a_main_diagonal_of_ones():
    X, _ = otib_np.roll5_track()
    r = otib_np.otib(X, X, oti=False, oti_rank=1)
    assert r["oti"] == 0 and r["crp"].shape == (51, 51)
    assert _diag(r["crp"]).all() and not _diag(r["closer"]).any()
    assert not _diag(r["dist"]).any()          # distance 0 on the diagonal: nothing is strictly closer
    assert 0.0 < otib_np.density(r["crp"]) < 0.9


def test_roll_by_five_bins_is_found_by_the_global_oti_only():
    X, Y = otib_np.roll5_track()
    on = otib_np.otib(X, Y, oti=True, oti_rank=1)
    # rolling the reference by g undoes its roll by 5: (5 + g) % 12 == 0
    assert (5 + on["oti"]) % 12 == 0
    assert _diag(on["crp"]).all()
    np.testing.assert_array_equal(on["crp"], otib_np.otib(X, X, oti=False)["crp"])
    off = otib_np.otib(X, Y, oti=False, oti_rank=1)
    assert off["oti"] == 0
    assert not _diag(off["crp"]).any()         # shift 7 restores the track: strictly closer everywhere
    assert (_diag(off["closer"]) >= 1).all()


def test_masks_are_nested_in_the_rank_and_rank_12_is_all_ones():
    X, Y = otib_np.cut_pair(120, 150)
    r1, r2, r12 = (otib_np.otib(X, Y, oti_rank=k)["crp"] for k in (1, 2, 12))
    assert (r1 <= r2).all() and (r2 <= r12).all() and r12.all()
    assert r1.sum() < r2.sum() < r12.sum()
    closer = otib_np.otib(X, Y)["closer"]
    assert closer.max() <= 11
    for k in (1, 2, 5, 12):
        np.testing.assert_array_equal(otib_np.otib(X, Y, oti_rank=k)["crp"], closer < k)


def test_a_block_of_zero_frames_gives_whole_rows_and_columns_of_ones():
    Z = otib_np.zero_block_track(n=80, start=20, length=12)
    X, _ = otib_np.roll5_track(n=70)
    rows = otib_np.otib(Z, X, oti_rank=1)
    assert rows["crp"][20:24].all() and not rows["closer"][20:24].any()   # stacked frames 20 .. 23 are all zero
    assert not rows["crp"][19].all() and not rows["crp"][24].all()
    cols = otib_np.otib(X, Z, oti_rank=1)
    assert cols["crp"][:, 20:24].all() and not cols["crp"][:, 19].all()


def test_constant_chroma_gives_all_ones():
    """A reference of constant chroma is its own roll, so the twelve distances are one computation:
    all ones against any query. A QUERY of constant chroma against an arbitrary reference is not
    covered by the definition: a roll re-orders the twelve products of the fmaf chain, and float32
    sums of the same terms in another order may differ in the last bit. It is covered where those
    sums are exact, as for a reference whose bins are multiples of 1/8."""
    X, _ = otib_np.roll5_track()
    K = otib_np.constant_track()
    rng = np.random.Generator(np.random.PCG64(4))
    E = (rng.integers(0, 9, (60, 12)) / 8.0).astype(np.float32)
    for a, b in ((X, K), (K, K), (K, E)):
        r = otib_np.otib(a, b, oti_rank=1)
        assert r["crp"].all() and not r["closer"].any()


def test_restatement_follows_m_and_tau():
    X, Y = otib_np.cut_pair(90, 110)
    for m, tau in ((1, 1), (5, 2), (64, 1)):
        r = otib_np.otib(X, Y, m=m, tau=tau)
        assert r["crp"].shape == (oracle.stacked_len(90, m, tau), oracle.stacked_len(110, m, tau))
        np.testing.assert_array_equal(r["dist"], oracle.crp_dist(X, Y, r["oti"], m, tau))


def test_aligned_reports_what_the_entries_report():
    X, Y = otib_np.cut_pair(100, 140)
    C = otib_np.otib(X, Y)["crp"]
    a = otib_np.aligned(C)
    assert a["qmax"] > 0 and a["dmax"] > 0
    assert len(a["qpath"]) and tuple(a["qpath"][-1]) == a["qseg"][2:] and tuple(a["qpath"][0]) == a["qseg"][:2]
    assert len(a["dpath"]) and tuple(a["dpath"][-1]) == a["dseg"][2:]
    assert a["rqa"]["n_rec"] == int(C.sum())


# ---- host logic ----
def test_crp_params_picks_the_struct():
    old = _lib.crp_params(m=7, tau=2, kappa=0.2)
    assert type(old) is _lib.CrpParams and ctypes.sizeof(old) == 24
    same = _lib.crp_params(m=7, tau=2, kappa=0.2, binarize="percentile", oti_rank=1)
    assert type(same) is _lib.CrpParams
    new = _lib.crp_params(m=7, tau=2, oti=False, binarize="oti", oti_rank=2)
    assert type(new) is _lib.CrpParams2 and ctypes.sizeof(new) == 32
    assert (new.m, new.tau, new.oti, new.binarize, new.oti_rank) == (7, 2, 0, 1, 2)
    assert new.base.m == 7 and _lib.CrpParams2.base.offset == 0 and _lib.CrpParams2.binarize.offset == 24
    assert _lib._entry("acoss_crp_align", old) == "acoss_crp_align"
    assert _lib._entry("acoss_crp_align", new) == "acoss_crp_align2"
    assert _lib._entry(_lib._aligner(1, "acoss_crp_path")[1], new) == "acoss_crp_path_dmax2"
    for name in ("align", "locate", "locate_dmax", "path", "path_dmax", "rqa", "pair"):
        assert "acoss_crp_%s2" % name in _lib.SIGNATURES
        assert ctypes.POINTER(_lib.CrpParams2) in _lib.SIGNATURES["acoss_crp_%s2" % name]
        assert ctypes.POINTER(_lib.CrpParams) not in _lib.SIGNATURES["acoss_crp_%s2" % name]
    assert len(_lib.SIGNATURES["acoss_crp_pair2"]) == len(_lib.SIGNATURES["acoss_crp_pair"]) + 1


@pytest.mark.parametrize("bad", [dict(binarize="otib"), dict(binarize=1), dict(binarize="oti", oti_rank=0),
                                 dict(binarize="oti", oti_rank=13), dict(binarize="oti", oti_rank=1.5),
                                 dict(binarize="percentile", oti_rank=0)])
def test_crp_params_value_errors(bad):
    with pytest.raises(ValueError):
        _lib.crp_params(**bad)


def test_cache_and_result_names():
    assert Serra09.algorithm_name() == "Serra09"
    assert Serra09.algorithm_name("det") == "Serra09-det"
    assert Serra09.algorithm_name(binarize="oti") == "Serra09-otib"
    assert Serra09.algorithm_name(binarize="oti", oti_rank=2) == "Serra09-otib2"
    assert Serra09.algorithm_name("smax", "oti", 1) == "Serra09-otib-smax"
    assert Serra09.algorithm_name("det", "oti", 2) == "Serra09-otib2-det"
    assert Serra09.algorithm_name("qmax", "percentile", 1) == "Serra09"
    assert ChenFusion.algorithm_name() == "LateFusionChen"
    assert ChenFusion.algorithm_name("oti") == "LateFusionChen-otib"
    assert ChenFusion.algorithm_name("oti", 3) == "LateFusionChen-otib3"
    with pytest.raises(ValueError):
        Serra09.algorithm_name("qmax", "oti", 0)
    with pytest.raises(ValueError):
        ChenFusion.algorithm_name("percentil")


def test_constructors_refuse_before_they_read_anything(tmp_path):
    for cls in (Serra09, ChenFusion):
        with pytest.raises(ValueError):
            cls(str(tmp_path / "none.csv"), str(tmp_path), binarize="oti", oti_rank=13)
        with pytest.raises(ValueError):
            cls(str(tmp_path / "none.csv"), str(tmp_path), binarize="binary")


@pytest.mark.parametrize("algorithm", ["EarlyFusionTraile", "FTM2D", "SiMPle"])
def test_benchmark_takes_binarize_for_the_crp_scorers_only(algorithm, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="Serra09 and LateFusionChen"):
        coverid.benchmark("none.csv", str(tmp_path), algorithm=algorithm, binarize="oti")
    with pytest.raises(ValueError, match="Serra09 and LateFusionChen"):
        coverid.benchmark("none.csv", str(tmp_path), algorithm=algorithm, oti_rank=2)


def test_benchmark_refuses_a_bad_binarize(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError):
        coverid.benchmark("none.csv", str(tmp_path), algorithm="Serra09", binarize="oti", oti_rank=0)
    with pytest.raises(ValueError):
        coverid.benchmark("none.csv", str(tmp_path), algorithm="LateFusionChen", binarize="serra08")


def test_command_line_has_the_pair():
    a = coverid.parser_args(["-i", "x.csv", "--binarize", "oti", "--oti-rank", "2"])
    assert (a.binarize, a.oti_rank) == ("oti", 2)
    d = coverid.parser_args(["-i", "x.csv"])
    assert (d.binarize, d.oti_rank) == ("percentile", 1)
