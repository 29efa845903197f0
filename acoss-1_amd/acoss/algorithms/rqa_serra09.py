"""Serra09 — cross recurrence quantification (acoss/algorithms/rqa_serra09.py), MI355X engine.

Serra, J., Serra, X., & Andrzejak, R. G. (2009). Cross recurrence quantification for cover
song identification. New Journal of Physics, 11(9), 093017.

Per pair the reference builds essentia ChromaCrossSimilarity(frameStackSize=m,
frameStackStride=tau, binarizePercentile=kappa, oti) and CoverSongSimilarity('serra09',
'symmetric') and stores Qmax (:55-69). Here `prepare()` median-downsamples every track on
the GPU (features.hip) into one packed HBM block, and `similarity(idxs)` scores a whole chunk
of pairs with one acoss_crp_align call (crp_split.hip / crp.hip).
"""
import argparse
import sys

import numpy as np

from .. import _lib
from ..engine import ChromaBank, path_frames, segment_frames
from .algorithm_template import CoverAlgorithm

__all__ = ["Serra09", "ChromaBackedAlgorithm"]


class ChromaBackedAlgorithm(CoverAlgorithm):
    """Shared by Serra09 and ChenFusion: cached median-downsampled chroma + a device bank."""

    def _init_chroma(self, chroma_type, oti, kappa, tau, m, downsample_fac, binarize="percentile", oti_rank=1,
                     n_oti=1):
        self.oti_rank = _lib.check_binarize(binarize, oti_rank)
        self.n_oti = _lib.check_n_oti(n_oti, oti)
        self.binarize = binarize
        self.oti = oti
        self.tau = tau
        self.m = m
        self.chroma_type = chroma_type
        self.kappa = kappa
        self.downsample_fac = downsample_fac
        self.all_feats = {}  # i -> downsampled chroma (n_i, 12) float32, as the reference caches
        self._bank = None
        self._n_frames = None  # frames of chroma_type per song before downsampling (prepare)

    def _downsample(self, chromas):
        from ..synthetic import pack
        feats, off, lens = pack([np.asarray(c, np.float32) for c in chromas])
        out, out_off, out_len = _lib.median_downsample(feats, off, lens, self.downsample_fac)
        return out, out_off, out_len

    def load_features(self, i):
        """Median-downsampled chroma of song i (rqa_serra09.py:44-53), cached."""
        if i not in self.all_feats:
            feats = CoverAlgorithm.load_features(self, i)
            out, _, _ = self._downsample([feats[self.chroma_type]])
            self.all_feats[i] = out.cpu().numpy()
        return self.all_feats[i]

    def prepare(self):
        if self._prepared:
            return
        chromas = [f[self.chroma_type] for f in self.load_features_many((self.chroma_type,))]
        self._n_frames = np.array([len(c) for c in chromas], np.int64)
        out, out_off, out_len = self._downsample(chromas)
        host = out.cpu().numpy()
        for i in range(self.N):
            self.all_feats[i] = host[out_off[i]:out_off[i] + out_len[i]]
        self._bank = ChromaBank(packed=(out, out_off, out_len))
        self._prepared = True

    def track_lengths(self):
        self.prepare()
        return np.maximum(self._bank.lens.astype(np.int64) - self.m * self.tau, 1)

    def _crp_kw(self):
        """What every bank call of this algorithm takes: the CRP's parameters and its binarisation."""
        return dict(m=self.m, tau=self.tau, kappa=self.kappa, oti=self.oti, binarize=self.binarize,
                    oti_rank=self.oti_rank)

    def _score_dev(self, idxs, dmax=False):
        """Qmax (and dmax) of the pairs, the best of the n_oti best transpositions; with n_oti > 1
        also the winners: "oti", "pick_q" (and "oti_d", "pick_d")."""
        self.prepare()
        return self._bank.crp_align(np.asarray(idxs, np.int32), qmax=True, dmax=dmax, n_oti=self.n_oti,
                                    **self._crp_kw())

    def _picks_kw(self, idxs, align=0):
        """The picks= of a bank call that must run on the transposition that won the pairs' best of
        n_oti: the Qmax winner (align 0; RQA and every measure), the dmax winner (align 1). One more
        scoring pass over the pairs; nothing at n_oti = 1."""
        if self.n_oti == 1:
            return {}
        r = self._bank.crp_align(np.asarray(idxs, np.int32).reshape(-1, 2), qmax=not align, dmax=bool(align),
                                 n_oti=self.n_oti, **self._crp_kw())
        return {"picks": r["pick_d" if align else "pick_q"]}

    def _score(self, idxs, dmax=False):
        return {k: v.cpu().numpy() for k, v in self._score_dev(idxs, dmax).items()}

    _ALIGNMENTS = {"qmax": 0, "dmax": 1}  # serra09 / chen17, the library's align

    def _alignment(self, alignment):
        if alignment not in self._ALIGNMENTS:
            raise ValueError("alignment must be 'qmax' (serra09) or 'dmax' (chen17), not %r" % (alignment,))
        return self._ALIGNMENTS[alignment]

    def localize(self, idxs, alignment="qmax"):
        """Where the Qmax alignment of every (query, reference) pair of idxs lies: a dict of host
        arrays 'qmax' (P,), 'oti' (P,), 'cells' (P, 4) = (i0, j0, i1, j1) in stacked-frame rows and
        columns of the pair's CRP, and 'query_frames' / 'reference_frames' (P, 2): half-open ranges
        in frames of `chroma_type` before downsampling (engine.segment_frames). A pair whose Qmax
        is 0 has cells (-1, -1, -1, -1) and ranges (-1, -1). Not collective: a rank localises the
        pairs it is given.
        alignment="dmax": the chen17 alignment instead, its score under 'dmax' in place of 'qmax'.
        That path may begin on the intermediate cell of a (2, 1) or (1, 2) step, so i0 or j0 may be 1
        (a Qmax path never begins before row and column 2).
        With n_oti > 1 the alignment is that of the winning transposition (the Qmax winner, or the
        dmax winner under alignment="dmax"), 'oti' the shift applied and the score the best of n_oti;
        finding the winner costs one extra scoring pass over idxs (also in align_path and rqa)."""
        align = self._alignment(alignment)
        self.prepare()
        idxs = np.asarray(idxs, np.int32).reshape(-1, 2)
        r = self._bank.crp_locate(idxs, align=align, **self._crp_kw(), **self._picks_kw(idxs, align))
        cells = r["seg"].cpu().numpy()
        qf, rf = segment_frames(cells, self.m, self.tau, self.downsample_fac, self._n_frames[idxs[:, 0]],
                                self._n_frames[idxs[:, 1]])
        return {alignment: r[alignment].cpu().numpy(), "oti": r["oti"].cpu().numpy(), "cells": cells,
                "query_frames": qf, "reference_frames": rf}

    def align_path(self, idxs, alignment="qmax"):
        """The Qmax alignment of every (query, reference) pair of idxs, cell by cell: a dict of host
        arrays 'qmax' (P,), 'oti' (P,) and 'cells' (P, 4) as localize, 'path_off' (P + 1,) int64,
        'path_cells' (total, 2) int32 and 'path_frames' (total, 2) int64. The path of pair p is
        path_cells[path_off[p]:path_off[p + 1]]: (i, j) in stacked-frame rows and columns of the
        pair's CRP from cells[p, :2] to cells[p, 2:], each step (1, 1), (2, 1) or (1, 2);
        path_frames holds the first frame of `chroma_type` before downsampling of each of them
        (engine.path_frames). A pair whose Qmax is 0 has an empty path. Not collective.
        alignment="dmax": the chen17 alignment instead, its score under 'dmax' in place of 'qmax'.
        Its five steps are (1, 1), (2, 1), (1, 2) and, exactly after the intermediate cell that a
        (2, 1) or (1, 2) step passed and that is a hit, (1, 0) and (0, 1): non-decreasing in i and j,
        possibly longer than the shorter track, and i0 or j0 may be 1."""
        align = self._alignment(alignment)
        self.prepare()
        idxs = np.asarray(idxs, np.int32).reshape(-1, 2)
        r = self._bank.crp_path(idxs, align=align, **self._crp_kw(), **self._picks_kw(idxs, align))
        pc = r["cells"].cpu().numpy()
        return {alignment: r[alignment].cpu().numpy(), "oti": r["oti"].cpu().numpy(), "cells": r["seg"].cpu().numpy(),
                "path_off": r["path_off"].cpu().numpy(), "path_cells": pc,
                "path_frames": path_frames(pc, self.tau, self.downsample_fac)}

    def _rqa_dev(self, idxs, lmin=2, smax=True, hist_cap=0, lines=True):
        self.prepare()
        idxs = np.asarray(idxs, np.int32).reshape(-1, 2)
        return self._bank.crp_rqa(idxs, lmin=lmin, smax=smax, hist_cap=hist_cap, lines=lines, **self._crp_kw(),
                                  **self._picks_kw(idxs))

    def rqa(self, idxs, lmin=2, hist=False):
        """Cross-recurrence quantification of every (query, reference) pair of idxs (the definition:
        include/acoss_hip.h, acoss_crp_rqa): a dict of host arrays, each (P,): 'rr', 'det', 'lmean',
        'entr' (float64), 'lmax' (int32), 'smax' (float32), 'n_rec', 'n_lines', 'n_lines_min',
        'n_pts_min' (int64) and 'oti'. lmin: the shortest diagonal line that 'det', 'lmean', 'entr'
        and the two '_min' counts take. hist=True adds 'hist' (P, L + 1) int32, L the longest stacked
        length of the bank: hist[p, l] = the number of diagonal lines of length l in pair p's CRP.
        Not collective: a rank quantifies the pairs it is given."""
        self.prepare()
        cap = _lib.stacked_len(self._bank.max_len, self.m, self.tau) + 1 if hist else 0
        r = {k: v.cpu().numpy() for k, v in self._rqa_dev(idxs, lmin=lmin, hist_cap=cap).items()}
        out = {k: r["stats"][:, c] for c, k in enumerate(_lib.RQA_STATS)}
        out.update({k: r["counts"][:, c] for c, k in enumerate(_lib.RQA_COUNTS)})
        out.update(lmax=r["lmax"], smax=r["smax"], oti=r["oti"])
        if hist:
            out["hist"] = r["hist"]
        return out

    def _norm_factors(self):
        """sqrt(n_j) in float64, n_j = downsampled frames of song j."""
        return np.sqrt(np.array([self.load_features(j).shape[0] for j in range(self.N)], np.float64))


class Serra09(ChromaBackedAlgorithm):
    # what all_pairwise can fill Ds with: the paper's three maxima, which grow with the tracks, and
    # the intensive CRQA measures, which do not
    MAXIMA = ("qmax", "smax", "lmax")
    MEASURES = MAXIMA + ("det", "lmean", "entr", "rr")

    @classmethod
    def algorithm_name(cls, measure="qmax", binarize="percentile", oti_rank=1, n_oti=1):
        """The name under which a Serra09 that scores by `measure` keeps its Ds cache and writes its
        results: 'Serra09' for Qmax (the reference's), 'Serra09-<measure>' for any other. On the
        OTI-binary CRP (binarize='oti') 'Serra09-otib', 'Serra09-otib<rank>' above rank 1, comes before
        the measure: 'Serra09-otib2-det'. Best of n_oti > 1 transpositions adds '-oti<n>' after it:
        'Serra09-oti2', 'Serra09-otib2-oti2-det'."""
        if measure not in cls.MEASURES:
            raise ValueError("measure must be one of %s, not %r" % (", ".join(cls.MEASURES), measure))
        name = "Serra09" + _lib.binarize_suffix(binarize, oti_rank) + _lib.n_oti_suffix(n_oti)
        return name if measure == "qmax" else "%s-%s" % (name, measure)

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='benchmark', oti=True, kappa=0.095,
                 tau=1, m=9, downsample_fac=40, cachedir="cache", measure="qmax", lmin=2, binarize="percentile",
                 oti_rank=1, n_oti=1):
        """binarize='oti': every CRP of this object (similarity, localize, align_path, rqa, measure=,
        the shortlist flow) is the OTI-binary CRP of Serra08 at oti_rank in 1 .. 12 (include/acoss_hip.h,
        acoss_crp_params2) in place of the percentile CRP; kappa is then not read.
        n_oti in 1 .. 12 (needs oti): Qmax is the best over the n_oti most probable transpositions of
        the ranked OTI (Serra, Serra and Andrzejak 2009; include/acoss_hip.h, acoss_crp_params3), at
        about n_oti times the scoring cost. localize, align_path, rqa and every measure other than
        'qmax' run on the transposition that won Qmax (alignment="dmax": that won dmax), which they
        first find with one extra scoring pass over their pairs."""
        name = self.algorithm_name(measure, binarize, oti_rank, _lib.check_n_oti(n_oti, oti))
        if int(lmin) != lmin or lmin < 1:
            raise ValueError("lmin must be an integer >= 1, not %r" % (lmin,))
        self.measure = measure
        self.lmin = int(lmin)
        self._init_chroma(chroma_type, oti, kappa, tau, m, downsample_fac, binarize, oti_rank, n_oti)
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name=name, datapath=datapath, shortname=shortname,
                                cachedir=cachedir)

    def _measure_dev(self, idxs):
        """The (P,) float32 device scores of the pairs by self.measure."""
        if self.measure == "qmax":
            return self._score_dev(idxs)["qmax"]
        if self.measure == "smax":
            return self._rqa_dev(idxs, lines=False)["smax"]
        r = self._rqa_dev(idxs, lmin=self.lmin, smax=False)
        if self.measure == "lmax":
            return r["lmax"].float()
        return r["stats"][:, _lib.RQA_STATS.index(self.measure)].float()

    def similarity(self, idxs):
        """Qmax (or self.measure) of every (query, reference) pair into every Ds key (rqa_serra09.py:55-69)."""
        idxs = np.asarray(idxs)
        if len(idxs) == 0:
            return
        q = self._measure_dev(idxs).cpu().numpy()
        for key in self.Ds.keys():
            self.Ds[key][idxs[:, 0], idxs[:, 1]] = q

    def _device_scores(self, idxs):
        q = self._measure_dev(idxs)
        return {key: q for key in self.Ds}

    def normalize_by_length(self):
        """D[i, j] /= sqrt(n_j), n_j = downsampled frames of song j (rqa_serra09.py:71-83);
        the quotient is taken in float64 and stored in the float32 matrix, as the reference
        (acoss_ds_finish mode 'serra09'). The three maxima grow with the tracks and are divided; the
        intensive measures (rr, det, lmean, entr) are left as they are."""
        if self.measure in self.MAXIMA:
            self._finish_device(self._norm_factors(), "serra09")


def parser_args(args):
    parser = argparse.ArgumentParser(sys.argv[0], description="Benchmarking with Joan Serra's Cover id algorithm",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-i", '--dataset_csv', type=str, action="store", help="Input dataset csv file")
    parser.add_argument("-d", '--datapath', type=str, action="store", help="Path to data files")
    parser.add_argument("-s", "--shortname", type=str, action="store", default="covers80",
                        help="Short name for dataset")
    parser.add_argument("-c", '--chroma_type', type=str, action="store", default="hpcp",
                        help="Type of chroma to use for experiments")
    parser.add_argument("-p", '--parallel', type=int, choices=(0, 1), action="store", default=0,
                        help="Parallel computing or not (ignored: pairs are batched on the GPU)")
    parser.add_argument("-n", '--n_cores', type=int, action="store", default=1, help="Ignored (see --parallel)")
    return parser.parse_args(args)


if __name__ == '__main__':
    cmd_args = parser_args(sys.argv[1:])
    # keyword arguments: the reference passes these positionally in the wrong order (:108)
    serra09 = Serra09(dataset_csv=cmd_args.dataset_csv, datapath=cmd_args.datapath,
                      chroma_type=cmd_args.chroma_type, shortname=cmd_args.shortname)
    serra09.all_pairwise(cmd_args.parallel, cmd_args.n_cores, symmetric=True)
    serra09.normalize_by_length()
    for similarity_type in serra09.Ds.keys():
        print(similarity_type)
        serra09.getEvalStatistics(similarity_type)
    serra09.cleanup_memmap()
    print("... Done ....")
