"""FTM2D — 2-D Fourier transform magnitude shingles (acoss/algorithms/ftm2d.py), MI355X engine.

Ellis, Bertin-Mahieux. Large-scale cover song recognition using the 2D Fourier transform
magnitude. ISMIR 2012.

`prepare()` reads every track's chroma and beat onsets and makes all shingles in one
acoss_ftm2d_shingles call (ftm2d.hip: beat-synchronous float32 medians, chrompwr, the 2-D DFT
magnitudes of every 12 x WIN beat window on the f64 MFMA, per-window normalisation and log, the
per-coefficient median over the windows; the reference does this per song in numpy, :52-66), and
`similarity(idxs)` scores a chunk of pairs with one acoss_ftm2d_scores call.
Ds['main'][i, j] = exp(-|s_i - s_j|^2) (:93-97). `shortlist(k)` (not in the reference) lists every
song's k best-scoring other songs with one acoss_ftm2d_topk call, for
`all_pairwise(candidates=...)` of an alignment scorer.

Reference defects not reproduced: `os` and `dd` are used without being imported (:44,47,82), and a
track with fewer than WIN beats crashes on None.T (:61,129-130); here such a track raises a
ValueError naming it before anything runs. There is no on-disk shingle cache.
"""
import argparse

import numpy as np

from .. import _lib
from .algorithm_template import CoverAlgorithm

__all__ = ["FTM2D"]


class FTM2D(CoverAlgorithm):
    """Same attributes as CoverAlgorithm, plus `shingles` {song index: (12 * WIN,) float64 shingle}
    and `chroma_type` (key into the features)."""

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='Covers80', PWR=1.96, WIN=75, C=5,
                 cachedir="cache"):
        self.PWR = PWR
        self.WIN = WIN
        self.C = C
        self.chroma_type = chroma_type
        self.shingles = {}
        self._bank = None
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name="FTM2D", datapath=datapath, shortname=shortname,
                                cachedir=cachedir)

    def get_cacheprefix(self):
        return "%s/%s_%s_%s" % (self.cachedir, self.name, self.shortname, self.chroma_type)

    def _shingles(self, feats):
        chromas = [f[self.chroma_type] for f in feats]
        onsets = [np.asarray(f['madmom_features']['onsets'], np.int64) for f in feats]
        return _lib.ftm2d_shingles(chromas, onsets, win=self.WIN, pwr=self.PWR, C=self.C)

    def load_features(self, i, do_plot=False):
        """(12 * WIN,) float64 shingle of song i (ftm2d.py:38-83)."""
        if i not in self.shingles:
            feats = CoverAlgorithm.load_features(self, i)
            self.shingles[i] = self._shingles([feats]).cpu().numpy()[0]
        return self.shingles[i]

    def prepare(self):
        if self._prepared:
            return
        feats = self.load_features_many((self.chroma_type, 'madmom_features'))
        self._bank = self._shingles(feats)
        host = self._bank.cpu().numpy()
        for i in range(self.N):
            self.shingles[i] = host[i]
        self._prepared = True

    def similarity(self, idxs):
        idxs = np.asarray(idxs)
        if len(idxs) == 0:
            return
        self.prepare()
        score = _lib.ftm2d_scores(self._bank, idxs.astype(np.int32))
        self.Ds['main'][idxs[:, 0], idxs[:, 1]] = score.cpu().numpy()

    def shortlist(self, k, rows=None):
        """The k songs of largest FTM2D score for each song of rows = (r0, r1) (default: all), the
        song itself left out, best first, equal scores by increasing index: a host (r1 - r0, k)
        int32 array, -1 in a slot with no candidate (k > N - 1, or a silent track's NaN shingle).
        One acoss_ftm2d_topk call over the shingle bank; the score matrix is never formed. Pass the
        result as all_pairwise(candidates=...) of an alignment scorer on the same dataset CSV."""
        self.prepare()
        r0, r1 = (0, self.N) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= r0 <= r1 <= self.N:
            raise ValueError("rows must be a range within [0, %d], got (%d, %d)" % (self.N, r0, r1))
        idx, _ = _lib.ftm2d_topk(self._bank[r0:r1], self._bank, k, self_off=r0)
        return idx.cpu().numpy()

    def _device_scores(self, idxs):
        """exp(-|s_i - s_j|^2) per pair as float32 device scores (the memmap's dtype)."""
        idxs = np.asarray(idxs)
        self.prepare()
        return {'main': _lib.ftm2d_scores(self._bank, idxs.astype(np.int32)).float()}


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description="Benchmarking with 2D Fourier Transform Magnitude Coefficients",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-i", '--dataset_csv', type=str, action="store", help="Input dataset csv file")
    parser.add_argument("-d", '--datapath', type=str, action="store", default='../features_covers80',
                        help="Path to data files")
    parser.add_argument("-s", "--shortname", type=str, action="store", default="Covers80", help="Short name for dataset")
    parser.add_argument("-c", '--chroma_type', type=str, action="store", default='hpcp',
                        help="Type of chroma to use for experiments")
    parser.add_argument("-p", '--parallel', type=int, choices=(0, 1), action="store", default=0, help="Ignored")
    parser.add_argument("-n", '--n_cores', type=int, action="store", default=1, help="Ignored")
    cmd_args = parser.parse_args()
    ftm2d = FTM2D(dataset_csv=cmd_args.dataset_csv, datapath=cmd_args.datapath, chroma_type=cmd_args.chroma_type,
                  shortname=cmd_args.shortname)
    ftm2d.prepare()
    print('Feature loading done.')
    ftm2d.all_pairwise(cmd_args.parallel, cmd_args.n_cores, symmetric=True)
    for similarity_type in ftm2d.Ds.keys():
        ftm2d.getEvalStatistics(similarity_type)
    ftm2d.cleanup_memmap()
    print("... Done ....")
