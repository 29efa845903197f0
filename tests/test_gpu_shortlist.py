"""Shortlist-and-rerank on the GPU: acoss_ftm2d_topk against acoss_ftm2d_scores over all pairs plus a
stable host argsort (indices and scores compared exactly), and the candidate-restricted
all_pairwise of Serra09 and SiMPle through coverid.benchmark against the unrestricted run.
"""
import numpy as np
import pytest

from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().as_tensor(np.ascontiguousarray(a, np.float64)).cuda()


def _score_rows(q, r):
    """(n_q, n_r) float64 scores of every (query, reference) pair by the pair kernel."""
    nq, nr = len(q), len(r)
    table = _dev(np.concatenate([q, r]))
    pairs = np.stack(np.meshgrid(np.arange(nq), nq + np.arange(nr), indexing="ij"), -1).reshape(-1, 2)
    return _lib.ftm2d_scores(table, pairs.astype(np.int32)).cpu().numpy().reshape(nq, nr)


def _want(q, r, k, self_off):
    rows = _score_rows(q, r)
    idx = np.full((len(q), k), -1, np.int32)
    score = np.full((len(q), k), np.nan)
    for i, row in enumerate(rows):
        row = row.copy()
        if self_off >= 0:
            row[self_off + i] = np.nan
        order = np.argsort(-row, kind="stable")  # NaN last
        order = order[:min(k, int((~np.isnan(row)).sum()))]
        idx[i, :len(order)] = order
        score[i, :len(order)] = row[order]
    return idx, score


def _check(q, r, k, self_off=-1):
    idx, score = _lib.ftm2d_topk(_dev(q), _dev(r), k, self_off)
    assert str(idx.dtype) == "torch.int32" and str(score.dtype) == "torch.float64"
    assert tuple(idx.shape) == tuple(score.shape) == (len(q), k)
    want_idx, want_score = _want(q, r, k, self_off)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(score.cpu().numpy(), want_score)
    return want_idx


def _table(n, dim, seed):
    t = np.random.default_rng(seed).standard_normal((n, dim))
    return t / np.linalg.norm(t, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def t37():
    return _table(37, 900, 1)


@pytest.mark.parametrize("k", [1, 5, 36, 64])
def test_plain(t37, k):
    idx = _check(t37, t37, k, self_off=0)
    assert (idx[:, :min(k, 36)] >= 0).all() and (idx != np.arange(37)[:, None]).all()
    if k == 64:
        assert (idx[:, 36:] == -1).all()


@pytest.mark.parametrize("dim", [1, 64, 65, 1024])
def test_rectangular(dim):
    rng = np.random.default_rng(dim)
    _check(0.3 * rng.standard_normal((5, dim)) / np.sqrt(dim), 0.3 * rng.standard_normal((131, dim)) / np.sqrt(dim), 9)


def test_ties_go_to_the_lower_index():
    t = _table(131, 64, 3)
    t[17] = t[3]
    t[90] = t[3]
    q = np.stack([t[3] + 0.01, t[3], t[50]])
    idx = _check(q, t, 4)
    assert list(idx[0, :3]) == [3, 17, 90] and list(idx[1, :3]) == [3, 17, 90]
    idx = _check(t, t, 4, self_off=0)
    assert list(idx[3, :2]) == [17, 90] and list(idx[17, :2]) == [3, 90] and list(idx[90, :2]) == [3, 17]


def test_nan_rows():
    r = _table(40, 900, 4)
    r[7] = np.nan
    q = r[:6].copy()
    q[2] = np.nan
    idx, score = _lib.ftm2d_topk(_dev(q), _dev(r), 40)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    assert (idx[2] == -1).all() and np.isnan(score[2]).all()
    assert not (idx == 7).any()
    assert idx[0, -1] == -1 and (idx[0, :-1] >= 0).all()  # 39 of the 40 references are not NaN
    _check(q, r, 40)
    _check(r, r, 5, self_off=0)  # the NaN row as a query and as a reference


@pytest.mark.parametrize("rising", [True, False])
def test_every_candidate_beats_the_threshold(rising):
    """Reference rows ordered so that every later row scores higher: each one enters the list, which
    is compacted again and again; then the reverse order, where none after the first k does."""
    q = _table(1, 64, 5)
    step = (700 - np.arange(700.0)) if rising else (1 + np.arange(700.0))
    r = np.repeat(q, 700, 0)
    r[:, 0] += step * 1e-3
    idx = _check(q, r, 100)
    assert list(idx[0]) == (list(range(699, 599, -1)) if rising else list(range(100)))


@pytest.mark.parametrize("n_q", [300, 301, 3, 2052, 4100])
def test_many_queries(n_q):
    """More queries than one block holds (4), a last block with 1, 3 or 4 of them, and the counts at
    which the launch stops splitting the reference rows into ranges: 75 and 76 blocks take 4 ranges of
    the 50 rows, 1 block 4, 513 blocks 3, 1025 blocks one (the partial lists and their merge are gone)."""
    _check(_table(n_q, 900, 6), _table(50, 900, 7), 7)


def test_one_tile_of_references():
    """Ten rows are one 16-row tile: a single range whatever the query count, fewer candidates than k."""
    _check(_table(6, 900, 12), _table(10, 900, 13), 12)
    _check(_table(10, 900, 13), _table(10, 900, 13), 12, self_off=0)


def test_stripe_equals_rows_of_the_full_call():
    t = _dev(_table(40, 900, 8))
    full_idx, full_score = _lib.ftm2d_topk(t, t, 6, self_off=0)
    idx, score = _lib.ftm2d_topk(t[10:25], t, 6, self_off=10)
    np.testing.assert_array_equal(idx.cpu().numpy(), full_idx[10:25].cpu().numpy())
    np.testing.assert_array_equal(score.cpu().numpy(), full_score[10:25].cpu().numpy())
    _check(t[10:25].cpu().numpy(), t.cpu().numpy(), 6, self_off=10)


def test_large_k_and_empty_tables():
    """k > 512 takes the largest LDS lists; no references or no queries launch nothing that reads."""
    torch = _torch()
    _check(_table(5, 64, 9), _table(1100, 64, 10), 1024)
    idx, score = _lib.ftm2d_topk(_dev(_table(3, 64, 9)), torch.empty((0, 64), dtype=torch.float64, device="cuda"), 4)
    assert (idx.cpu().numpy() == -1).all() and np.isnan(score.cpu().numpy()).all()
    idx, score = _lib.ftm2d_topk(torch.empty((0, 64), dtype=torch.float64, device="cuda"), _dev(_table(3, 64, 9)), 4)
    assert tuple(idx.shape) == (0, 4)


def test_bad_arguments():
    torch = _torch()
    lib = _lib.load_library()
    t = _dev(_table(4, 64, 11))
    idx = torch.empty((4, 4), dtype=torch.int32, device="cuda")
    score = torch.empty((4, 4), dtype=torch.float64, device="cuda")
    for dim, k in ((64, 0), (64, 1025), (1025, 4)):
        rc = lib.acoss_ftm2d_topk(_lib._ptr(t), 4, _lib._ptr(t), 4, dim, -1, k, _lib._ptr(idx), _lib._ptr(score),
                                  _lib._stream())
        assert rc == -1  # ACOSS_E_ARG
        assert b"acoss_ftm2d_topk" in lib.acoss_last_error()
    wide = torch.zeros((2, 1025), dtype=torch.float64, device="cuda")
    for args in ((t, t, 0), (t, t, 1025), (wide, wide, 1), (t, t[:, :32], 1), (t.float(), t, 1), (t.cpu(), t, 1),
                 (t, t, 1, -2)):
        with pytest.raises(ValueError):
            _lib.ftm2d_topk(*args)


# ---- the plugin flow: FTM2D shortlist -> candidate-restricted Serra09 / SiMPle ----

class _Flow:
    """One small dataset on disk and coverid.benchmark runs over it, each in a cache directory of its own."""

    def __init__(self, root):
        self.root = root
        tr, labels = synthetic.make_corpus("covers80", frames=2400, seed=11)
        keep = np.flatnonzero(labels < 8)
        self.labels = labels[keep]
        self.n = len(keep)
        self.csv, self.fdir = synthetic.write_feature_dataset(str(root), [tr[k] for k in keep], self.labels,
                                                              with_mfcc=True, beat_period=20)
        self._runs = {}

    def run(self, algorithm, shortlist=None):
        """(Ds['main'] as an array, getEvalStatistics('main')) of one benchmark run, made once."""
        import os
        from acoss import coverid
        key = (algorithm, shortlist)
        if key not in self._runs:
            cwd = os.getcwd()
            os.chdir(str(self.root))  # the results CSV and the log go to the working directory
            try:
                algo = coverid.benchmark(self.csv, self.fdir, algorithm=algorithm, shortname="t", shortlist=shortlist,
                                         cachedir=str(self.root / ("cache_%s_%s" % key)))
                self._runs[key] = (np.array(algo.Ds["main"]), algo.getEvalStatistics("main"))
            finally:
                os.chdir(cwd)
        return self._runs[key]

    def raw_serra09(self, tag, candidates):
        """Ds['main'] of Serra09.all_pairwise(symmetric=True) before normalize_by_length, which divides
        column j by sqrt(n_j) and so ends the symmetry that the scores themselves have."""
        from acoss.algorithms.rqa_serra09 import Serra09
        algo = Serra09(self.csv, self.fdir, shortname="t", cachedir=str(self.root / ("cache_raw_" + tag)))
        algo.all_pairwise(symmetric=True, candidates=candidates)
        D = np.array(algo.Ds["main"])
        algo.cleanup_memmap()
        return D

    def candidates(self, k):
        from acoss.algorithms.ftm2d import FTM2D
        f = FTM2D(self.csv, self.fdir, shortname="t", cachedir=str(self.root / "cache_ftm2d"))
        cands = f.shortlist(k)
        f.cleanup_memmap()
        return cands


@pytest.fixture(scope="module")
def flow(tmp_path_factory):
    return _Flow(tmp_path_factory.mktemp("shortlist_flow"))


def _same_stats(a, b):
    assert tuple(a[:4]) == tuple(b[:4]) and list(a[4]) == list(b[4])


def test_plugin_shortlist_is_the_topk_of_the_score_matrix(flow):
    from acoss.algorithms.ftm2d import FTM2D
    f = FTM2D(flow.csv, flow.fdir, shortname="t", cachedir=str(flow.root / "cache_ftm2d_full"))
    cands = f.shortlist(5)
    assert cands.shape == (flow.n, 5) and cands.dtype == np.int32
    want, _ = _want(f._bank.cpu().numpy(), f._bank.cpu().numpy(), 5, 0)
    np.testing.assert_array_equal(cands, want)
    np.testing.assert_array_equal(f.shortlist(5, rows=(3, 9)), want[3:9])
    with pytest.raises(ValueError):
        f.shortlist(5, rows=(3, flow.n + 1))
    f.cleanup_memmap()


@pytest.mark.parametrize("algorithm,symmetric", [("Serra09", True), ("SiMPle", False)])
def test_plugin_flow(flow, algorithm, symmetric):
    from acoss import evaluation
    n = flow.n
    full, full_stats = flow.run(algorithm)
    got, stats = flow.run(algorithm, shortlist=5)
    cands = flow.candidates(5)
    assert (cands >= 0).all()
    scored = np.zeros((n, n), bool)
    scored[np.repeat(np.arange(n), 5), cands.reshape(-1)] = True  # j in cands[i]
    if symmetric:
        scored |= scored.T                                          # or i in cands[j]
        # benchmark() has normalised by length (column j over sqrt(n_j)): the scored set is symmetric
        # there, the matrix itself before that step
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(got).T)
        raw, raw_full = flow.raw_serra09("cand", cands), flow.raw_serra09("full", None)
        np.testing.assert_array_equal(raw, raw.T)
        np.testing.assert_array_equal(raw[scored], raw_full[scored])
        assert (raw[~scored & ~np.eye(n, dtype=bool)] == -np.inf).all() and (np.diag(raw) == 0).all()
    else:
        assert not np.array_equal(scored, scored.T)  # the ordered pairs are not a symmetric set here
    assert got.dtype == np.float32 and not scored.diagonal().any()
    np.testing.assert_array_equal(got[scored], full[scored])
    off = ~scored & ~np.eye(n, dtype=bool)
    assert off.any() and (got[off] == -np.inf).all()
    np.testing.assert_array_equal(np.diag(got), np.diag(full))
    _same_stats(stats, evaluation.eval_statistics(got, flow.labels))
    # every other song shortlisted: the unrestricted run
    all_got, all_stats = flow.run(algorithm, shortlist=n - 1)
    np.testing.assert_array_equal(all_got, full)
    _same_stats(all_stats, full_stats)


def test_plugin_refuses_a_shortlist_for_the_fused_algorithms(flow):
    from acoss import coverid
    with pytest.raises(ValueError, match="Serra09 and SiMPle"):
        coverid.benchmark(flow.csv, flow.fdir, algorithm="LateFusionChen", shortname="t", shortlist=5,
                          cachedir=str(flow.root / "cache_chen"))
