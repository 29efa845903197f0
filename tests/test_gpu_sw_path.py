"""GPU tests of the located and traced constrained Smith-Waterman alignment (acoss_sw_locate /
acoss_sw_path: sw.hip k_swt<false>, k_swt<true>, k_sw_backtrack) against the numpy restatement
tests/sw_path_np.py. Everything compares with `==`: scores, segments, lengths and paths; the score
also with acoss_sw_constrained's."""
import ctypes

import numpy as np
import pytest
import torch

import sw_path_np as sp
from acoss import _lib

pytestmark = pytest.mark.gpu


def _extremes(M, N):
    return [np.zeros((M, N), np.uint8), np.ones((M, N), np.uint8)]


def _batch(cases, extremes=()):
    """(matrices, restatement results) of some of sp.CASES plus all-zero and all-ones matrices."""
    mats, want = [], []
    for c in cases:
        B, res = sp.expected(*c)
        mats.append(B)
        want.append(res)
    for M, N in extremes:
        for B in _extremes(M, N):
            mats.append(B)
            want.append(sp.sw_path(B))
    return mats, want


def _check(mats, want, tag):
    loc = _lib.sw_locate(mats)
    pth = _lib.sw_path(mats)
    ref = _lib.sw_constrained(mats).cpu().numpy()
    lscore, lseg = loc["score"].cpu().numpy(), loc["seg"].cpu().numpy()
    pscore, pseg = pth["score"].cpu().numpy(), pth["seg"].cpu().numpy()
    off, cells = pth["path_off"].cpu().numpy(), pth["cells"].cpu().numpy()
    assert off[0] == 0 and off[-1] == len(cells)
    for k, (B, res) in enumerate(zip(mats, want)):
        t = "%s #%d %dx%d" % (tag, k, B.shape[0], B.shape[1])
        got = cells[off[k]:off[k + 1]]
        print("%s: score %r seg %r, %d cells; restatement %r seg %r, %d cells"
              % (t, pscore[k], pseg[k].tolist(), len(got), res.score, res.seg, len(res.path)))
        assert lscore[k] == res.score and pscore[k] == res.score and ref[k] == res.score, t
        assert lseg[k].tolist() == list(res.seg), t
        assert pseg[k].tolist() == list(res.seg), t
        assert len(got) == len(res.path), t
        assert got.tolist() == res.path.tolist(), t


def test_the_inputs_meet_the_hard_cases():
    """Asserted from the restatement, so the comparisons below cannot pass by never meeting them."""
    got = [sp.expected(*c) for c in sp.CASES]
    lane = [any(sp.crosses_row(r, k) for k in range(sp.LANE_ROWS, B.shape[0], sp.LANE_ROWS)) for B, r in got]
    assert any(lane), "a path across a lane boundary"
    assert any(sp.crosses_row(r, sp.BAND_ROWS) for _, r in got), "a path across row 512"
    assert any(sp.crosses_row(r, 2 * sp.BAND_ROWS) for _, r in got), "a path across row 1024"
    assert any(sp.crosses_row(r, 4 * sp.BAND_ROWS) for _, r in got), "a path across row 2048"
    assert any(sp.tie_cells(B, r) for B, r in got), "a tie cell on a reported path"
    assert any(sp.miss_cells(B, r) for B, r in got), "a miss on a path"
    assert any(r.score == 0 for _, r in got) and any(len(r.path) == sp.path_bound(*B.shape) > 0 for B, r in got)


def test_all_sizes_in_one_batch():
    """Every case and the all-zero and all-ones matrices together: one matrix per wave in bands, the
    matrices of a launch of every size."""
    mats, want = _batch(sp.CASES, [(33, 40), (260, 70), (1030, 40), (4, 4)])
    _check(mats, want, "all")


def test_small_sizes_share_waves():
    """Matrices of at most 64 rows: 8 lanes each, 8 per wave, groups holding matrices of different
    sizes; the count is no multiple of 8."""
    cases = [c for c in sp.CASES if c[0] <= 64]
    mats, want = _batch(cases, [(33, 40), (64, 65)])
    if len(mats) % 8 == 0:
        mats, want = mats[:-1], want[:-1]
    assert len(mats) % 8 != 0
    _check(mats, want, "small")


@pytest.mark.parametrize("shape", sp.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_each_shape_in_a_batch_of_its_own(shape):
    """The lanes per matrix follow the batch's largest row count: 1 (3 x 9) to 17 (130 x 70) lanes with
    several matrices per wave, the whole wave from 260 rows on, three bands at 1030 and five at 2050;
    the score kernel keeps 16 rows per lane from 530 rows on (one band there, three at 2050). The
    count is no multiple of the matrices per wave."""
    M, N, _ = shape
    mats, want = _batch([c for c in sp.CASES if c[:2] == (M, N)], [(M, N)])
    LP = (M + 7) // 8
    G = 64 // LP if LP <= 32 else 1
    if G > 1 and len(mats) % G == 0:
        mats, want = mats[:-1], want[:-1]
    assert G == 1 or len(mats) % G != 0
    _check(mats, want, "%dx%d" % (M, N))


def _raw_path(mats, cap):
    """acoss_sw_path with buffers of this test's own: (rc, lengths, padded paths, sentinel intact)."""
    lib = _lib.load_library()
    flat, off, rows, cols, mr, mc = _lib._pack_mats([_lib._as_binary_u8(m) for m in mats], torch.uint8)
    n = len(mats)
    lens = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    padded = torch.full((n + 1, max(1, cap), 2), -7, dtype=torch.int32, device="cuda")  # one entry more: untouched
    rc = lib.acoss_sw_path(_lib._ptr(flat), _lib._ptr(off), _lib._ptr(rows), _lib._ptr(cols), n, mr, mc,
                           ctypes.c_void_p(0), ctypes.c_void_p(0), cap, _lib._ptr(lens), _lib._ptr(padded),
                           _lib._stream())
    torch.cuda.synchronize()
    return rc, lens.cpu().numpy(), padded[:n].cpu().numpy(), bool((padded[n] == -7).all())


def test_padding_duplicates_and_null_outputs():
    """The entries after a path hold -1 and nothing past the matrices' entries is written; score_out
    and seg_out may be NULL; a matrix listed twice gets identical output."""
    cases = [(33, 40, 0.3, 2), (14, 47, 0.3, None), (33, 40, 0.3, 2), (5, 9, 0.1, None)]
    mats, want = _batch(cases, [(4, 4)])
    cap = sp.path_bound(33, 47)
    rc, lens, padded, intact = _raw_path(mats, cap)
    assert rc == 0 and intact
    for k, res in enumerate(want):
        assert lens[k] == len(res.path)
        assert padded[k, :lens[k]].tolist() == res.path.tolist()
        assert (padded[k, lens[k]:] == -1).all()
    assert lens[0] == lens[2] and np.array_equal(padded[0], padded[2])


def test_refusals():
    mats = [np.zeros((12, 9), np.uint8), np.zeros((5, 30), np.uint8)]
    bound = max(1, min(12, 30) - 3)
    assert bound == 9
    assert _raw_path(mats, bound)[0] == 0
    assert _raw_path(mats, bound - 1)[0] == -1  # ACOSS_E_ARG
    with pytest.raises(_lib.AcossHipError, match="= 9"):
        _lib.sw_path(mats, path_cap=bound - 1)
    bad = np.zeros((12, 9), np.uint8)
    bad[3, 4] = 2
    for fn in (_lib.sw_locate, _lib.sw_path):
        with pytest.raises(IOError, match="Non-binary"):
            fn([mats[0], bad])
        with pytest.raises(_lib.AcossHipError, match="SHAPE"):
            fn([np.zeros((65536, 4), np.uint8)])
    empty = _lib.sw_path([])
    assert empty["path_off"].tolist() == [0] and empty["cells"].shape == (0, 2)
    assert _lib.sw_locate([])["seg"].shape == (0, 4)
