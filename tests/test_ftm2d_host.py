"""Host-side tests of FTM2D (no GPU): the numpy restatement against the reference's golden file,
the argument checks of the two C entry points, the host checks of _lib.ftm2d_shingles, and the
coverid dispatch.

Bars against the golden file (tests/golden/make_golden_ftm2d.py): the reference keeps float32
through the FFT (scipy.fftpack.fft2 of float32 is complex64), the restatement is float64 from
chrompwr on, so they differ by the reference's own float32 rounding: 2e-7 absolute on the
unit-norm shingle entries and 1e-7 on a score (6x the measured 3.2e-8 / 1.3e-8), 1e-6 relative
on chrompwr (a few float32 ulps).
"""
import ctypes
import os

import numpy as np
import pytest

import ftm2d_np
from acoss import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ftm2d_golden.npz")
GOLD_TRACKS = "ABCE"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def tracks():
    return ftm2d_np.make_tracks()


def test_generator_matches_golden_inputs(gold, tracks):
    for k in GOLD_TRACKS:
        np.testing.assert_array_equal(tracks[k][0], gold[k + "_hpcp"])
        np.testing.assert_array_equal(tracks[k][1], gold[k + "_onsets"])
    beats = {k: len(ftm2d_np.boundaries(o, len(h))) - 1 for k, (h, o) in tracks.items()}
    assert beats == {"A": 75, "B": 76, "C": 91, "D": 120, "E": 240, "F": 121, "G": 101, "H": 4170}
    assert ftm2d_np.boundaries(tracks["F"][1], 900)[1] == 300


def test_restatement_matches_golden(gold, tracks):
    sh = []
    for k in GOLD_TRACKS:
        sync = ftm2d_np.beat_sync(*tracks[k])
        assert sync.dtype == np.float32
        np.testing.assert_array_equal(sync, gold[k + "_sync"])
        np.testing.assert_allclose(ftm2d_np.chrompwr(sync), gold[k + "_chrompwr"], rtol=1e-6, atol=1e-7)
        s = ftm2d_np.shingle(*tracks[k])
        assert s.shape == (900,) and s.dtype == np.float64
        np.testing.assert_allclose(s, gold[k + "_shingle"], rtol=0, atol=2e-7)
        sh.append(s)
    # the 2-D DFT magnitudes alone, on the reference's own (float32) chrompwr
    mags = ftm2d_np.fft_mags(gold["A_chrompwr"])
    np.testing.assert_allclose(mags.T, gold["A_fftmat"], rtol=0, atol=1e-5 * gold["A_fftmat"].max())
    np.testing.assert_allclose(ftm2d_np.score_matrix(sh), gold["scores_f64"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(ftm2d_np.score_matrix(sh).astype(np.float32), gold["scores"], rtol=2e-7, atol=0)


def test_restatement_shingle_is_mirror_symmetric(tracks):
    s = ftm2d_np.shingle(*tracks["C"]).reshape(12, 75)
    r, q = np.meshgrid(np.arange(12), np.arange(75), indexing="ij")
    c, k = (r + 6) % 12, (q + 38) % 75
    np.testing.assert_allclose(s, s[((12 - c) % 12 + 6) % 12, ((75 - k) % 75 + 37) % 75], rtol=0, atol=1e-14)


def test_c_entry_points_check_arguments_without_gpu():
    lib = _lib.load_library()
    buf = (ctypes.c_double * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    E_ARG = -1
    # win != 75: the twiddle size is a compile-time constant
    for win in (0, 74, 76, 150):
        assert lib.acoss_ftm2d_shingles(p, p, p, 1, 400, p, p, win, 1.96, 5.0, p, null) == E_ARG
        assert b"win" in lib.acoss_last_error()
    assert lib.acoss_ftm2d_shingles(p, p, p, 1, 400, p, p, 75, 1.96, 5.0, null, null) == E_ARG  # null output
    assert lib.acoss_ftm2d_shingles(null, p, p, 1, 400, p, p, 75, 1.96, 5.0, p, null) == E_ARG
    assert lib.acoss_ftm2d_shingles(p, p, p, 1, 400, null, p, 75, 1.96, 5.0, p, null) == E_ARG
    assert lib.acoss_ftm2d_shingles(p, p, p, -1, 400, p, p, 75, 1.96, 5.0, p, null) == E_ARG    # negative count
    assert lib.acoss_ftm2d_shingles(p, p, p, 1, -1, p, p, 75, 1.96, 5.0, p, null) == E_ARG
    assert lib.acoss_ftm2d_shingles(p, p, p, 0, 0, p, p, 75, 1.96, 5.0, p, null) == 0           # nothing to do
    assert lib.acoss_ftm2d_scores(p, 2, 900, p, 1, null, null) == E_ARG                         # null output
    assert lib.acoss_ftm2d_scores(null, 2, 900, p, 1, p, null) == E_ARG
    assert lib.acoss_ftm2d_scores(p, 2, 900, null, 1, p, null) == E_ARG
    assert lib.acoss_ftm2d_scores(p, 2, 900, p, -1, p, null) == E_ARG                           # negative counts
    assert lib.acoss_ftm2d_scores(p, -2, 900, p, 1, p, null) == E_ARG
    assert lib.acoss_ftm2d_scores(p, 2, 0, p, 1, p, null) == E_ARG
    assert lib.acoss_ftm2d_scores(p, 2, 2000, p, 1, p, null) == E_ARG
    assert lib.acoss_ftm2d_scores(p, 2, 900, p, 0, p, null) == 0
    assert lib.acoss_ftm2d_beatsync(p, p, p, -1, p, p, 10, 1.96, null, p, null) == E_ARG
    assert lib.acoss_ftm2d_beatsync(p, p, p, 1, p, p, 10, 1.96, null, null, null) == E_ARG


def test_lib_refuses_short_and_long_tracks_before_any_launch(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "_torch", no_gpu)
    ok = np.ones((400, 12), np.float32)
    short = np.ones((370, 12), np.float32)     # 73 onsets -> 74 beats
    long_ = np.ones((4171, 12), np.float32)    # an onset at every frame -> 4171 beats
    with pytest.raises(ValueError, match=r"track 1: 74 beats"):
        _lib.ftm2d_shingles([ok, short], [np.arange(5, 400, 5), np.arange(5, 370, 5)])
    with pytest.raises(ValueError, match=r"track 0: 4171 beats"):
        _lib.ftm2d_shingles([long_, ok], [np.arange(4171), np.arange(5, 400, 5)])
    with pytest.raises(ValueError) as e:
        _lib.ftm2d_shingles([short, ok, long_], [np.arange(5, 370, 5), np.arange(5, 400, 5), np.arange(4171)])
    assert "track 0" in str(e.value) and "track 2" in str(e.value) and "track 1" not in str(e.value)
    # 75 and 4170 beats pass the host check (and only then reach for the device)
    with pytest.raises(AssertionError, match="reached the device"):
        _lib.ftm2d_shingles([np.ones((373, 12), np.float32), np.ones((4170, 12), np.float32)],
                            [np.arange(5, 373, 5), np.arange(4170)])


def test_bounds_are_unique_clipped_and_packed():
    h = np.ones((500, 12), np.float32)
    o = np.array([10, 10, 499, 510, 3, -4], np.int64)
    feats, off, lens, bounds, bound_off = _lib.ftm2d_bounds([h, h[:20]], [o, np.array([7])], win=0)
    np.testing.assert_array_equal(bounds, [0, 3, 10, 499, 500, 0, 7, 20])
    np.testing.assert_array_equal(bound_off, [0, 5, 8])
    assert bounds.dtype == np.int64 and bound_off.dtype == np.int64
    np.testing.assert_array_equal(bounds[:5], ftm2d_np.boundaries(o, 500))
    assert feats.shape == (520, 12) and list(off) == [0, 500] and list(lens) == [500, 20]


def test_plugin_import_and_coverid_dispatch(tmp_path, monkeypatch):
    from acoss import coverid
    from acoss.algorithms import FTM2D as exported
    from acoss.algorithms import ftm2d as mod
    from acoss.algorithms.ftm2d import FTM2D
    assert exported is FTM2D
    import inspect
    params = inspect.signature(FTM2D.__init__).parameters
    assert [params[k].default for k in ("chroma_type", "PWR", "WIN", "C")] == ["hpcp", 1.96, 75, 5]
    assert "cachedir" in params
    calls = []

    class Fake(object):
        Ds = {"main": None}

        def __init__(self, **kw):
            calls.append(("init", kw))

        def prepare(self):
            calls.append("prepare")

        def all_pairwise(self, parallel, n_cores=1, symmetric=False):
            calls.append(("all_pairwise", symmetric))

        def getEvalStatistics(self, s):
            calls.append(("stats", s))

        def cleanup_memmap(self):
            calls.append("cleanup")

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(mod, "FTM2D", Fake)
    algo = coverid.benchmark("x.csv", "y/", algorithm="FTM2D", shortname="t", cachedir="c")
    assert isinstance(algo, Fake)
    assert calls[0] == ("init", dict(dataset_csv="x.csv", datapath="y/", chroma_type="hpcp", shortname="t",
                                     cachedir="c"))
    assert calls[1:] == ["prepare", ("all_pairwise", True), ("stats", "main"), "cleanup"]
