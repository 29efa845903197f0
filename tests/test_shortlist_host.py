"""CPU tests of the shortlist path's host logic (no GPU): the candidate-pair enumeration per row
stripe, shortlist_recall, and all_pairwise(candidates=...) on the host `similarity` loop."""
import numpy as np
import pytest

from acoss import distributed as D
from acoss import evaluation, synthetic
from acoss.algorithms.algorithm_template import CoverAlgorithm

# row i lists song i's candidates: empty slots, self entries, mutual entries (0 <-> 1, 2 <-> 4), a repeat
HAND = np.array([[1, -1, 3],
                 [0, 1, -1],
                 [4, 4, 2],
                 [-1, -1, -1],
                 [2, 0, 5],
                 [5, 3, 1]])


def test_hand_written_pairs():
    sym = D.candidate_pairs(HAND, 0, 6, symmetric=True)
    assert sym.dtype == np.int32
    assert sym.tolist() == [[0, 1], [0, 3], [0, 4], [1, 5], [2, 4], [3, 5], [4, 5]]
    ordered = D.candidate_pairs(HAND, 0, 6, symmetric=False)
    assert ordered.tolist() == [[0, 1], [0, 3], [1, 0], [2, 4], [4, 0], [4, 2], [4, 5], [5, 1], [5, 3]]
    # a stripe owns the symmetric pairs whose smaller index it holds, whichever row listed them
    assert D.candidate_pairs(HAND, 3, 5, symmetric=True).tolist() == [[3, 5], [4, 5]]
    assert D.candidate_pairs(HAND, 3, 5, symmetric=False).tolist() == [[4, 0], [4, 2], [4, 5]]
    assert D.candidate_pairs(HAND, 3, 4, symmetric=False).shape == (0, 2)
    for bad in (HAND.astype(np.float64), HAND[0], np.where(HAND == 5, 6, HAND), np.where(HAND == 5, -2, HAND)):
        with pytest.raises(ValueError):
            D.candidate_pairs(bad, 0, 6)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("symmetric", [True, False])
def test_stripes_partition_the_candidate_pairs(world, symmetric):
    rng = np.random.default_rng(world)
    n = 40
    cands = rng.integers(-1, n, size=(n, 6))
    i, j = np.repeat(np.arange(n), 6), cands.reshape(-1)
    keep = (j >= 0) & (j != i)
    i, j = i[keep], j[keep]
    if symmetric:
        i, j = np.minimum(i, j), np.maximum(i, j)
    whole = sorted(set(zip(i.tolist(), j.tolist())))
    bounds = D.stripe_bounds(rng.integers(50, 200, n), world, symmetric, m=0, tau=0)
    assert bounds[0][0] == 0 and bounds[-1][1] == n
    got = []
    for r0, r1 in bounds:
        p = [tuple(x) for x in D.candidate_pairs(cands, r0, r1, symmetric).tolist()]
        assert p == sorted(set(p)) and all(r0 <= a < r1 for a, _ in p)  # lexicographic, no repeat, own rows
        got += p
    assert got == whole  # disjoint (no repeat across stripes) and complete; stripes in order keep the order


def test_shortlist_recall():
    cliques = {"a": {0, 1, 2}, "b": {3, 4}, "c": {5}}
    # ordered same-clique pairs: 6 in a, 2 in b. Listed: (0,1) (0,2) (1,0) (4,3) -> 4 of 8; row 2 lists
    # itself and strangers, row 0 lists 1 twice
    cands = np.array([[1, 2, 1], [0, 5, -1], [2, 3, 5], [-1, -1, 5], [3, 0, 1], [0, 1, 2]])
    assert evaluation.shortlist_recall(cands, cliques) == 0.5
    assert evaluation.shortlist_recall(cands, [[0, 1, 2], [3, 4], [5]]) == 0.5
    n = 6
    full = np.array([[j for j in range(n) if j != i] for i in range(n)])
    assert evaluation.shortlist_recall(full, cliques) == 1.0
    assert evaluation.shortlist_recall(np.full((n, 3), -1), cliques) == 0.0
    assert np.isnan(evaluation.shortlist_recall(full, {"x": {0}, "y": {1}}))


class IndexScore(CoverAlgorithm):
    """score(i, j) = i N + j: every entry says which pair wrote it."""

    def similarity(self, idxs):
        idxs = np.asarray(idxs)
        for key in self.Ds:
            self.Ds[key][idxs[:, 0], idxs[:, 1]] = (idxs[:, 0] * self.N + idxs[:, 1]).astype(np.float32)


class DenseOnly(IndexScore):
    _takes_candidates = False


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("shortlist_host")
    rng = np.random.default_rng(0)
    tracks = [rng.random((20, 12)).astype(np.float32) for _ in range(6)]
    csv, fdir = synthetic.write_feature_dataset(str(root), tracks, [0, 0, 1, 1, 2, 2])
    return root, csv, fdir


def _algo(dataset, name, cls=IndexScore):
    root, csv, fdir = dataset
    return cls(csv, name=name, datapath=fdir, shortname="t", cachedir=str(root / ("cache_" + name)),
               similarity_types=["main", "other"])


@pytest.mark.parametrize("symmetric", [True, False])
def test_all_pairwise_with_candidates_on_the_host_path(dataset, symmetric, monkeypatch):
    monkeypatch.chdir(dataset[0])
    n = 6
    dense = _algo(dataset, "dense%d" % symmetric)
    dense.all_pairwise(symmetric=symmetric)
    full = np.array(dense.Ds["main"])
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    today = (i * n + j).astype(np.float32)
    if symmetric:
        today = np.triu(today, 1) + np.triu(today, 1).T
    np.fill_diagonal(today, 0)
    np.testing.assert_array_equal(full, today)  # candidates=None: the matrix it gives today

    a = _algo(dataset, "cand%d" % symmetric)
    a.all_pairwise(symmetric=symmetric, candidates=HAND)
    scored = np.zeros((n, n), bool)
    p = D.candidate_pairs(HAND, 0, n, symmetric)
    scored[p[:, 0], p[:, 1]] = True
    if symmetric:
        scored |= scored.T
    for key in ("main", "other"):
        got = np.array(a.Ds[key])
        np.testing.assert_array_equal(got[scored], full[scored])
        off = ~scored & ~np.eye(n, dtype=bool)
        assert off.any() and (got[off] == -np.inf).all()
        np.testing.assert_array_equal(np.diag(got), np.zeros(n, np.float32))
    # the stable evaluation order takes -inf entries
    stats = a.getEvalStatistics("main")
    assert np.isfinite(stats[0])
    # reloading ignores candidates (b maps a's memmap file anew: keep a's matrix first)
    kept = np.array(a.Ds["main"])
    b = _algo(dataset, "cand%d" % symmetric)
    b.all_pairwise(precomputed=True, candidates=HAND[:2])
    np.testing.assert_array_equal(np.array(b.Ds["main"]), kept)
    for x in (dense, a):
        x.cleanup_memmap()


def test_all_pairwise_refuses_bad_candidates(dataset, monkeypatch):
    monkeypatch.chdir(dataset[0])
    a = _algo(dataset, "bad")
    for bad in (HAND[:5], HAND.astype(np.float32), HAND[:, 0]):
        with pytest.raises(ValueError):
            a.all_pairwise(symmetric=True, candidates=bad)
    with pytest.raises(ValueError, match="dense"):
        _algo(dataset, "denseonly", DenseOnly).all_pairwise(symmetric=True, candidates=HAND)
    a.cleanup_memmap()


def test_fused_algorithms_and_benchmark_refuse_a_shortlist():
    from acoss import coverid
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    from acoss.algorithms.latefusion_chen import ChenFusion
    assert not EarlyFusion._takes_candidates and not ChenFusion._takes_candidates
    for name in ("LateFusionChen", "EarlyFusionTraile", "FTM2D"):
        with pytest.raises(ValueError, match="Serra09 and SiMPle"):
            coverid.benchmark("none.csv", "none", algorithm=name, shortlist=5)
    assert coverid.parser_args(["-k", "7"]).shortlist == 7 and coverid.parser_args([]).shortlist is None


def _rank_worker(rank, world, port, csv, fdir, cache, out, symmetric):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    a = IndexScore(csv, name="Idx", datapath=fdir, shortname="w", cachedir=cache, similarity_types=["main"])
    a.all_pairwise(symmetric=symmetric, candidates=HAND)
    if rank == 0:
        np.save(out, np.asarray(a.Ds["main"]))
    a.getEvalStatistics("main")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("symmetric", [True, False])
def test_candidates_on_two_gloo_ranks_equal_one(dataset, symmetric, tmp_path, monkeypatch):
    """Each rank scores the candidate pairs of its stripe, the one gather is unchanged: rank 0's
    matrix equals the single-process run's, -inf entries included."""
    import socket
    import torch.multiprocessing as mp
    monkeypatch.chdir(tmp_path)
    one = _algo(dataset, "one%d" % symmetric)
    one.all_pairwise(symmetric=symmetric, candidates=HAND)
    want = np.array(one.Ds["main"])
    one.cleanup_memmap()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "rank0.npy")
    mp.start_processes(_rank_worker, args=(2, port, dataset[1], dataset[2], str(tmp_path / "c2"), out, symmetric),
                       nprocs=2, join=True, start_method="spawn")
    np.testing.assert_array_equal(np.load(out), want)
    assert np.isneginf(want).any()
