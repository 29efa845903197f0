"""EarlyFusion's mutual nearest-neighbour binarisation on the GPU (csrc/ef_binarize.hip) against the
numpy restatement of the definition (mutual_np.py; include/acoss_hip.h, "mutual"). Every comparison
is exact (==).

Masks: acoss_binarize_mutual runs the pipeline's own row launch and column pass on a batch of
caller matrices; three batches whose largest sides pick the three row classes (<= 64: a wave or a
block per matrix; <= 512 and above: a wave per row with 8 / 16 key registers) and the column classes
(ld <= 64: a column per lane; <= 512 and <= 1024: a wave per column with 8 / 16 key registers), and a
fourth above 1024 (the lane-private radix kernel; the row kernel's bisection). Scores:
earlyfusion(mutual=True) == oracle.sw_constrained of the restatement's masks of the oracle's
matrices; locate / path == sw_path_np on those masks; early SNF: the binary matrix is the
restatement's mask of the cross block the same call returned.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import early_snf_cases as ec
import mutual_np as mn
import oracle
import sw_path_np as sp
from conftest import ROOT

pytestmark = pytest.mark.gpu

K, KAPPA, MU = ec.BANK_K, ec.BANK_KAPPA, 0.5

# (rows, cols) per batch: max_rows / max_cols of a batch choose the row and the column class
BATCHES = {
    1: [(1, 1), (1, 7), (7, 1), (4, 30), (30, 4), (15, 17), (16, 16), (17, 15), (33, 64), (64, 33), (64, 64)],
    2: [(65, 64), (64, 65), (130, 70), (70, 130), (257, 300), (512, 40), (40, 512)],
    3: [(600, 40), (40, 600), (513, 520), (1024, 40), (40, 1024)],
    4: [(1030, 40), (40, 1030)],
}


@functools.lru_cache(maxsize=None)
def batch_mats(b):
    return [D for M, N in BATCHES[b] for D in mn.tie_matrices(M, N, 100 + b)]


@functools.lru_cache(maxsize=None)
def batch_expected(b, kappa):
    """[(row mask, mutual mask)] of the batch from the restatement, computed once."""
    return [(mn.rows_smallest(D, kappa), mn.mutual_smallest(D, kappa)) for D in batch_mats(b)]


def check_batch(b, kappas=mn.KAPPAS):
    from acoss import _lib
    mats = batch_mats(b)
    for kappa in kappas:
        want = batch_expected(b, kappa)
        rows = [t.cpu().numpy() for t in _lib.binarize_mutual(mats, kappa, mutual=False)]
        both = [t.cpu().numpy() for t in _lib.binarize_mutual(mats, kappa, mutual=True)]
        differ = 0
        for i, D in enumerate(mats):
            t = "batch %d kappa %r matrix %d %s" % (b, kappa, i, D.shape)
            assert rows[i].dtype == np.uint8 and rows[i].shape == D.shape, t
            assert np.array_equal(rows[i], want[i][0]), t + " (rows)"
            assert np.array_equal(both[i], want[i][1]), t + " (mutual)"
            differ += not np.array_equal(rows[i], both[i])
        print("batch %d kappa %r: %d matrices, mutual differs from rows in %d" % (b, kappa, len(mats), differ))


@pytest.mark.parametrize("b", sorted(BATCHES))
def test_masks_equal_the_restatement(b):
    check_batch(b)


@pytest.mark.parametrize("env,batches", [
    # the block-per-matrix row kernel and the wave-per-column kernel in place of the per-lane ones
    ({"ACOSS_EF_LANEBIN": "0", "ACOSS_EF_COLLANES": "0"}, (1,)),
    # the lane-private radix column kernel at every size
    ({"ACOSS_EF_COLLANES": "0", "ACOSS_EF_COLWAVE": "0"}, (1, 2))])
def test_masks_other_kernels(env, batches):
    """The batches again in a fresh child process with the other kernels of a shape class; the
    switches are read once per process."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_gpu_mutual as t\n"
            "for b in %r:\n"
            "    t.check_batch(b)\n"
            "print('ok')\n" % ([ROOT, os.path.join(ROOT, "acoss-1_amd"), os.path.join(ROOT, "tests")], batches))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("b", sorted(BATCHES))
def test_rows_mode_is_binarize_rows(b):
    """ACOSS_EF_BIN_ROWS == acoss_binarize_rows, matrix by matrix. acoss_binarize_rows reads a count
    of 0 as kappa == 0 (all ones), so a row whose count rounds to 0 (empty by the definition, and
    checked against the restatement above) is compared as empty."""
    from acoss import _lib
    mats = batch_mats(b)
    for kappa in (0.1, 0.3, 5):
        rows = _lib.binarize_mutual(mats, kappa, mutual=False)
        for D, got in zip(mats, rows):
            nn = mn.count(kappa, D.shape[1])
            want = _lib.binarize_rows(D, nn).cpu().numpy() if nn > 0 else np.zeros(D.shape, np.uint8)
            assert np.array_equal(got.cpu().numpy(), want), (b, kappa, D.shape)


@pytest.mark.parametrize("b", sorted(BATCHES))
def test_transpose_closure_on_the_gpu(b):
    """mutual(D.T) == mutual(D).T on the GPU's own output."""
    from acoss import _lib
    mats = batch_mats(b)
    for kappa in (0.1, 0.3):
        a = _lib.binarize_mutual(mats, kappa)
        t = _lib.binarize_mutual([np.ascontiguousarray(D.T) for D in mats], kappa)
        for x, y in zip(a, t):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy().T), (b, kappa, tuple(x.shape))


def test_binarize_mutual_refuses():
    from acoss import _lib
    lib = _lib.load_library()
    import torch
    D = torch.zeros(12, dtype=torch.float32, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(12, dtype=torch.uint8, device="cuda")
    for rows, cols, mr, mc, kappa, binarize in [(3, 4, 3, 4, 0.1, 7), (3, 4, 3, 4, -0.1, 1), (3, 4, 2, 4, 0.1, 1),
                                                (0, 4, 3, 4, 0.1, 1)]:
        r = torch.tensor([rows], dtype=torch.int32, device="cuda")
        c = torch.tensor([cols], dtype=torch.int32, device="cuda")
        rc = lib.acoss_binarize_mutual(_lib._ptr(D), _lib._ptr(off), _lib._ptr(r), _lib._ptr(c), 1, mr, mc, kappa,
                                       binarize, _lib._ptr(out), _lib._stream())
        assert rc == -1, (rows, cols, mr, mc, kappa, binarize)


# ---- the four scores -------------------------------------------------------------------------------
def oracle_mats(a, b):
    """The four matrices of a pair from the oracle's stages: the three CSMs and
    E = canon_expf(-(((0 + W_m) + W_s) + W_c)) in float32, the order k_ef_wsum sums in."""
    C = [oracle.ef_csm(a["mfccs"], b["mfccs"], 0), oracle.ef_csm(a["ssms"], b["ssms"], 0),
         oracle.ef_csm(a["chromas"], b["chromas"], 1, a["chroma_med"], b["chroma_med"])]
    wsum = np.zeros_like(C[0])
    for D in C:
        wsum = (wsum + oracle.ef_wcsm(D, K, K, MU)).astype(np.float32)
    return C + [oracle.canon_expf(-wsum)]


def _feats_pairs(kind, name):
    if kind == "exact":  # ec.bank_case's tracks and pairs, without its SNF reference records
        blocks, seed, _ = ec.BANKS[name]
        feats = ec.bank_tracks(blocks, seed)
        T = len(blocks)
        pairs = ec.LONG_PAIRS if name == "long" else [(i, j) for i in range(T) for j in range(T)]
    elif kind == "float":
        blocks, seed, pairs = ec.FLOAT_BANKS[name]
        feats = ec.bank_tracks(blocks, seed, ec.FLOAT)
    elif kind == "dup":
        feats, pairs, _ = ec.duplicate_block_case()
    else:
        feats, pairs = ec.pair_tracks([(130, 70)], 51)
    return feats, np.asarray(pairs, np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def score_case(kind, name):
    """(feats, pairs, masks [P][4] under the mutual rule, scores (P, 4)): the restatement, once."""
    feats, pairs = _feats_pairs(kind, name)
    cache = {}
    for a, b in pairs:
        if (a, b) not in cache:
            cache[(a, b)] = [mn.mutual_smallest(D, KAPPA) for D in oracle_mats(feats[a], feats[b])]
    masks = [cache[(a, b)] for a, b in pairs]
    scores = np.array([[oracle.sw_constrained(B) for B in row] for row in masks])
    return feats, pairs, masks, scores


@functools.lru_cache(maxsize=None)
def _bank(kind, name):
    return ec.make_bank(_feats_pairs(kind, name)[0])[0]


SCORE_CASES = [("exact", "tiny"), ("exact", "short"), ("exact", "mid"), ("float", "short"), ("float", "mid"),
               ("exact", "long"), ("dup", "")]


@pytest.mark.parametrize("kind,name", SCORE_CASES)
def test_scores_equal_the_restatement(kind, name):
    from acoss import _lib
    _, pairs, _, want = score_case(kind, name)
    bank = _bank(kind, name)
    got = _lib.earlyfusion(bank, pairs, KAPPA, K, MU, mutual=True).cpu().numpy()
    rows = _lib.earlyfusion(bank, pairs, KAPPA, K, MU).cpu().numpy()
    print("%s %s: %d of %d scores differ from the row rule's" % (kind, name, int((got != rows).sum()), got.size))
    np.testing.assert_array_equal(got, want)
    if kind == "exact" and name != "long":  # all T^2 ordered pairs: once more in a permuted order
        perm = np.random.default_rng(7).permutation(len(pairs))
        again = _lib.earlyfusion(bank, pairs[perm], KAPPA, K, MU, mutual=True).cpu().numpy()
        np.testing.assert_array_equal(again, want[perm])
        assert (got != rows).any()


def test_scores_in_chunks_on_both_streams(monkeypatch):
    """The short bank under a workspace budget of a few pairs per chunk: several chunks, both streams."""
    from acoss import _lib
    _, pairs, _, want = score_case("exact", "short")
    monkeypatch.setenv("ACOSS_EF_BYTES", "400000")
    monkeypatch.delenv("ACOSS_EF_STREAMS", raising=False)
    got = _lib.earlyfusion(_bank("exact", "short"), pairs, KAPPA, K, MU, mutual=True).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def _lead(bank, pairs):
    from acoss import _lib
    return (_lib._ptr(bank["mfccs"]), _lib._ptr(bank["ssms"]), _lib._ptr(bank["chromas"]), _lib._ptr(bank["chroma_med"]),
            _lib._ptr(bank["off"]), _lib._ptr(bank["nb"]), int(bank["nb"].shape[0]), int(bank["max_blocks"]),
            int(bank["mfccs"].shape[1]), int(bank["ssms"].shape[1]), int(bank["chromas"].shape[1]), _lib._ptr(pairs),
            int(pairs.shape[0]), float(KAPPA), int(K), float(MU))


def test_rows_mode_gives_the_twins_bits_and_unknown_mode_is_refused():
    import torch
    from acoss import _lib
    lib = _lib.load_library()
    _, pairs, _, _ = score_case("exact", "short")
    bank = _bank("exact", "short")
    P = len(pairs)
    dp = torch.as_tensor(pairs).cuda()
    cap = max(1, _lib.sw_path_bound(int(bank["max_blocks"]), int(bank["max_blocks"])))
    new = lambda dt, *s: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    res = {}
    for tag, binarize in (("twin", None), ("rows", 0), ("bad", 7)):
        sc, ls, ps = new(torch.float64, P, 4), new(torch.float64, P, 4), new(torch.float64, P, 4)
        lseg, pseg = new(torch.int32, P, 4, 4), new(torch.int32, P, 4, 4)
        lens, cells = new(torch.int32, P, 4), new(torch.int32, P, 4, cap, 2)
        extra = () if binarize is None else (binarize,)
        sfx = "" if binarize is None else "2"
        rcs = [getattr(lib, "acoss_earlyfusion" + sfx)(*_lead(bank, dp), *extra, _lib._ptr(sc), _lib._stream()),
               getattr(lib, "acoss_earlyfusion_locate" + sfx)(*_lead(bank, dp), *extra, _lib._ptr(ls), _lib._ptr(lseg),
                                                              _lib._stream()),
               getattr(lib, "acoss_earlyfusion_path" + sfx)(*_lead(bank, dp), *extra, _lib._ptr(ps), _lib._ptr(pseg), cap,
                                                            _lib._ptr(lens), _lib._ptr(cells), _lib._stream())]
        torch.cuda.synchronize()
        if tag == "bad":
            assert rcs == [-1, -1, -1]  # ACOSS_E_ARG
            continue
        assert rcs == [0, 0, 0], lib.acoss_last_error()
        res[tag] = [t.cpu().numpy() for t in (sc, ls, ps, lseg, pseg, lens, cells)]
    for x, y in zip(res["twin"], res["rows"]):
        assert np.array_equal(x, y)
    assert np.count_nonzero(res["twin"][0]) > P


# ---- locate and path -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("exact", "tiny"), ("exact", "short"), ("pair", "130x70")])
def test_locate_and_path_on_the_mutual_masks(kind, name):
    from acoss import _lib
    _, pairs, masks, want = score_case(kind, name)
    bank = _bank(kind, name)
    ref = _lib.earlyfusion(bank, pairs, KAPPA, K, MU, mutual=True).cpu().numpy()
    loc = _lib.earlyfusion_locate(bank, pairs, KAPPA, K, MU, mutual=True)
    pth = _lib.earlyfusion_path(bank, pairs, KAPPA, K, MU, mutual=True)
    np.testing.assert_array_equal(ref, want)
    np.testing.assert_array_equal(loc["scores"].cpu().numpy(), ref)
    np.testing.assert_array_equal(pth["scores"].cpu().numpy(), ref)
    lseg, pseg = loc["seg"].cpu().numpy(), pth["seg"].cpu().numpy()
    off, cells = pth["path_off"].cpu().numpy(), pth["cells"].cpu().numpy()
    for p, row in enumerate(masks):
        for s, B in enumerate(row):
            res = sp.sw_path(B)
            t = "pair %d %s matrix %d" % (p, pairs[p].tolist(), s)
            assert res.score == ref[p, s], t
            assert lseg[p, s].tolist() == list(res.seg) and pseg[p, s].tolist() == list(res.seg), t
            assert cells[off[4 * p + s]:off[4 * p + s + 1]].tolist() == res.path.tolist(), t


# ---- early SNF -------------------------------------------------------------------------------------
def _snf(bank, pairs, niters, mutual, k=K):
    from acoss import _lib
    r = _lib.earlyfusion_snf(bank, pairs, KAPPA, k, niters, want_cross=True, mu=MU, mutual=mutual, want_binary=True)
    off = r["cross_off"].cpu().numpy()
    return r["score"].cpu().numpy(), r["cross"].cpu().numpy(), r["binary"].cpu().numpy(), off


@pytest.mark.parametrize("name", ["tiny", "short", "mid", "long"])
def test_snf2_binary_is_the_mask_of_its_own_cross(name):
    from acoss import _lib
    feats, pairs = _feats_pairs("exact", name)
    if name == "long":
        pairs = pairs[1:2]  # one long pair: (300, 512)
    niters = ec.BANKS[name][2]
    bank = _bank("exact", name)
    score, cross, binary, off = _snf(bank, pairs, niters, True)
    rscore, rcross, rbinary, _ = _snf(bank, pairs, niters, False)
    twin = _lib.earlyfusion_snf(bank, pairs, KAPPA, K, niters, want_cross=True, mu=MU)
    assert np.array_equal(rscore, twin["score"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(rcross, twin["cross"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(cross, rcross, equal_nan=True)
    differ = 0
    for p, (a, b) in enumerate(pairs):
        M, N = ec.shape_of(feats, (a, b))
        assert mn.count(KAPPA, N) < N and ec.es.pair_ok(M, N, K)
        X = cross[off[p]:off[p + 1]].reshape(M, N)
        B = binary[off[p]:off[p + 1]].reshape(M, N)
        Br = rbinary[off[p]:off[p + 1]].reshape(M, N)
        assert np.array_equal(B, mn.mutual_largest(X, KAPPA)), (name, p, M, N)
        assert np.array_equal(Br, mn.rows_largest(X, KAPPA)), (name, p, M, N)
        assert score[p] == oracle.sw_constrained(B), (name, p)
        assert rscore[p] == oracle.sw_constrained(Br), (name, p)
        differ += not np.array_equal(B, Br)
    print("%s: the mutual matrix differs from the row matrix in %d of %d pairs" % (name, differ, len(pairs)))
    assert differ > 0


def test_snf2_refused_pair():
    """K = 3: (14, 47) cannot be fused (k1 = int(42 / 61) = 0): NaN, a zero matrix, neighbours untouched."""
    feats, pairs = ec.pair_tracks([(22, 23), (14, 47), (23, 23)], 52)
    pairs = np.asarray(pairs, np.int32)
    bank = ec.make_bank(feats)[0]
    score, cross, binary, off = _snf(bank, pairs, 3, True, k=3)
    alone = [_snf(bank, pairs[p:p + 1], 3, True, k=3) for p in (0, 2)]
    assert np.isnan(score[1]) and np.isnan(cross[off[1]:off[2]]).all() and not binary[off[1]:off[2]].any()
    for q, p in enumerate((0, 2)):
        assert score[p] == alone[q][0][0] and np.isfinite(score[p])
        assert np.array_equal(binary[off[p]:off[p + 1]], alone[q][2])
        M, N = ec.shape_of(feats, pairs[p])
        X = cross[off[p]:off[p + 1]].reshape(M, N)
        assert np.array_equal(binary[off[p]:off[p + 1]].reshape(M, N), mn.mutual_largest(X, KAPPA))
