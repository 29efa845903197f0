"""SiMPle — similarity matrix profile (acoss/algorithms/simple_silva.py), MI355X engine.

Silva, Yeh, Batista, Keogh. SiMPle: Assessing music similarity using subsequences joins.
ISMIR 2016.

`prepare()` computes every track's SiMPle features once on the GPU (features.hip: window
means, Hann smoothing, column L2 norm; the reference recomputes them for every pair,
:120-126), and `similarity(idxs)` scores a chunk of ordered pairs with one acoss_simple_mp
call (simple.hip: Simple.oti + matrix profile + median). Ds['main'][i, j] = -median(MP).
`profile(idxs)` returns the matrix profile itself and its index per pair (acoss_simple_profile):
which part of the reference each part of the query is nearest to.
`self_profile(tracks)` is the paper's other join, a song against itself without the trivial
matches (acoss_simple_self_profile): its repeated section (motif) and its most unusual passage
(discord).
"""
import argparse

import numpy as np

from .. import _lib
from ..engine import subsequence_frames
from .algorithm_template import CoverAlgorithm

__all__ = ["Simple"]


class Simple(CoverAlgorithm):
    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='Covers80', SSLEN=10, WIN=200,
                 SKIP=100, cachedir="cache"):
        self.SSLEN = SSLEN
        self.WIN = WIN
        self.SKIP = SKIP
        self.chroma_type = chroma_type
        self.all_feats = {}
        self._packed = None
        self._n_frames = None  # frames of chroma_type per song before the window means (prepare)
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name="SiMPle", datapath=datapath, shortname=shortname,
                                cachedir=cachedir)

    def _features(self, chromas):
        from ..synthetic import pack
        feats, off, lens = pack([np.asarray(c, np.float32) for c in chromas])
        return _lib.simple_features(feats, off, lens, win=self.WIN, skip=self.SKIP)

    def load_features(self, i, do_plot=False):
        """(12, floor(n / SKIP)) float64 SiMPle features of song i (simple_silva.py:34-43)."""
        if i not in self.all_feats:
            feats = CoverAlgorithm.load_features(self, i)
            out, _, T = self._features([feats[self.chroma_type]])
            self.all_feats[i] = out.cpu().numpy().reshape(12, int(T[0]))
        return self.all_feats[i]

    def prepare(self):
        if self._prepared:
            return
        chromas = [f[self.chroma_type] for f in self.load_features_many((self.chroma_type,))]
        self._n_frames = np.array([len(c) for c in chromas], np.int64)
        out, out_off, T = self._features(chromas)
        host = out.cpu().numpy()
        for i in range(self.N):
            self.all_feats[i] = host[out_off[i]:out_off[i] + 12 * T[i]].reshape(12, int(T[i]))
        self._packed = (out, out_off, T)
        self._prepared = True

    def track_lengths(self):
        self.prepare()
        return np.maximum(self._packed[2].astype(np.int64), 1)

    def oti(self, seq_a, seq_b):
        """(roll(seq_b, k*), argsort of the 12 shift scores) (simple_silva.py:45-54)."""
        pa, pb = np.sum(seq_a, 1), np.sum(seq_b, 1)
        v = np.array([np.dot(pa, np.roll(pb, i, axis=0)) for i in range(12)])
        order = np.argsort(v, kind="stable")
        return np.roll(seq_b, order[-1], axis=0), order

    def simple_sim(self, seq_a, seq_b):
        """median of the matrix profile of seq_a against seq_b (simple_silva.py:68-118), on the GPU."""
        score, _ = _lib.simple_mp([seq_a, seq_b], np.array([[0, 1]], np.int32), self.SSLEN, apply_oti=False)
        return float(score.cpu().numpy()[0])

    def similarity(self, idxs):
        idxs = np.asarray(idxs)
        if len(idxs) == 0:
            return
        self.prepare()
        out, off, T = self._packed
        score, _ = _lib.simple_mp_packed(out, off, T, idxs.astype(np.int32), self.SSLEN)
        self.Ds['main'][idxs[:, 0], idxs[:, 1]] = -score.cpu().numpy()

    def profile(self, idxs):
        """The matrix profile of every (query, reference) pair of idxs and its index: a dict of
        host arrays 'score' (P,) (Ds['main'] holds -score), 'oti' (P,), 'off' (P + 1,) int64, 'mp'
        (total,) float64 and 'mpi' (total,) int32, and 'query_frames' / 'reference_frames'
        (total, 2) int64. Row i of pair p sits at off[p] + i: mp is the distance of the query's
        subsequence i (SSLEN feature columns from column i) to its nearest subsequence of the
        reference, mpi that subsequence's first column (the smallest among equal distances; -1,
        with NaN in mp, where there is none), and the frame arrays hold the half-open ranges the
        two cover in frames of `chroma_type` before the window means (engine.subsequence_frames;
        the reference's is (-1, -1) where mpi is -1). Not collective: a rank profiles the pairs it
        is given."""
        self.prepare()
        idxs = np.asarray(idxs, np.int32).reshape(-1, 2)
        out, off, T = self._packed
        r = {k: v.cpu().numpy() for k, v in _lib.simple_profile_packed(out, off, T, idxs, self.SSLEN).items()}
        rows = np.diff(r["off"])
        i = np.arange(r["off"][-1]) - np.repeat(r["off"][:-1], rows)
        r["query_frames"] = subsequence_frames(i, self.SSLEN, self.WIN, self.SKIP,
                                               np.repeat(self._n_frames[idxs[:, 0]], rows))
        r["reference_frames"] = subsequence_frames(r["mpi"], self.SSLEN, self.WIN, self.SKIP,
                                                   np.repeat(self._n_frames[idxs[:, 1]], rows))
        return r

    def self_profile(self, tracks=None, excl=None):
        """The self-join of every song of `tracks` (None: every song): its matrix profile against
        itself without the trivial matches, the rows within `excl` subsequences of the row itself
        (None: SSLEN // 2), its motif and its discord (acoss_simple_self_profile). A dict of host
        arrays: 'off' (n + 1,) int64, 'mp' (total,) float64 and 'mpi' (total,) int32 (row i of
        entry e at off[e] + i: the distance of subsequence i to its nearest admissible subsequence
        of the same song and that subsequence's first column; NaN and -1 where there is none),
        'motif' (n, 2) int32 (the row of the smallest mp and its mpi: the song's repeated section)
        and 'discord' (n,) int32 (the row of the largest mp: its most unusual passage), -1 where a
        song has no row; and the half-open ranges in frames of `chroma_type` before the window
        means (engine.subsequence_frames, (-1, -1) where an index is -1): 'frames' and
        'match_frames' (total, 2) int64 of row i and of mpi, 'motif_frames' (n, 2, 2) and
        'discord_frames' (n, 2). Not collective: a rank profiles the songs it is given."""
        self.prepare()
        tracks = np.arange(self.N, dtype=np.int32) if tracks is None else np.asarray(tracks, np.int32).reshape(-1)
        out, off, T = self._packed
        r = {k: v.cpu().numpy()
             for k, v in _lib.simple_self_profile_packed(out, off, T, tracks, self.SSLEN, excl).items()}
        rows = np.diff(r["off"])
        i = np.arange(r["off"][-1]) - np.repeat(r["off"][:-1], rows)
        nf = self._n_frames[tracks]
        nrow = np.repeat(nf, rows)
        r["frames"] = subsequence_frames(i, self.SSLEN, self.WIN, self.SKIP, nrow)
        r["match_frames"] = subsequence_frames(r["mpi"], self.SSLEN, self.WIN, self.SKIP, nrow)
        r["motif_frames"] = subsequence_frames(r["motif"].reshape(-1), self.SSLEN, self.WIN, self.SKIP,
                                               np.repeat(nf, 2)).reshape(-1, 2, 2)
        r["discord_frames"] = subsequence_frames(r["discord"], self.SSLEN, self.WIN, self.SKIP, nf)
        return r

    def _device_scores(self, idxs):
        """-median(MP) per ordered pair as float32 device scores (the memmap's dtype)."""
        idxs = np.asarray(idxs)
        self.prepare()
        out, off, T = self._packed
        score, _ = _lib.simple_mp_packed(out, off, T, idxs.astype(np.int32), self.SSLEN)
        return {'main': (-score).float()}


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description="Benchmarking with Similarity Matrix Profile-based similarity",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-i", '--dataset_csv', type=str, action="store", help="Input dataset csv file")
    parser.add_argument("-d", '--datapath', type=str, action="store", default='features_covers80',
                        help="Path to data files")
    parser.add_argument("-s", "--shortname", type=str, action="store", default="Covers80", help="Short name for dataset")
    parser.add_argument("-c", '--chroma_type', type=str, action="store", default='crema',
                        help="Type of chroma to use for experiments")
    parser.add_argument("-p", '--parallel', type=int, choices=(0, 1), action="store", default=0, help="Ignored")
    parser.add_argument("-n", '--n_cores', type=int, action="store", default=1, help="Ignored")
    cmd_args = parser.parse_args()
    simple = Simple(dataset_csv=cmd_args.dataset_csv, datapath=cmd_args.datapath, chroma_type=cmd_args.chroma_type,
                    shortname=cmd_args.shortname)
    simple.all_pairwise(cmd_args.parallel, cmd_args.n_cores, symmetric=False)
    for similarity_type in simple.Ds.keys():
        simple.getEvalStatistics(similarity_type)
    simple.cleanup_memmap()
    print("... Done ....")
