"""EarlyFusion — early MFCC/HPCP fusion (acoss/algorithms/earlyfusion_traile.py), MI355X engine.

Tralie, C.J., 2017. Early mfcc and hpcp fusion for robust cover song identification.
arXiv preprint arXiv:1707.04680.

Per pair (A15, :157-198) everything runs on the GPU through the C-ABI: three CSMs on MFMA
(euclidean on the MFCC blocks and on the SSM blocks, blocked-OTI cosine on the chroma
blocks), kappa-NN binarisation, getWCSM of each CSM, their sum -> exp(-sum) -> binarisation,
and the four constrained Smith-Waterman alignments of a chunk in one launch.

The beat-synchronous block features (load_features, :67-154) are computed
on the GPU too (efblocks.hip acoss_ef_block_features: every block of a batch of tracks in one
launch, skimage's resize restated in float64), batched over all songs in prepare() and cached on
disk as the reference does. `resize_block` (:214-247) stays as the reference's public helper: it
restates skimage >= 0.19 `resize(..., anti_aliasing=True, mode='constant')` (Gaussian pre-filter
with sigma = max(0, (factor - 1) / 2), then a grid-mode linear zoom with zero fill) with
scipy.ndimage. skimage is absent here, so both restatements are pinned against each other and
against an independent loop restatement (tests/test_earlyfusion_host.py), not against skimage.
"""
import argparse
import os
import time

import numpy as np

from .. import _lib
from ..features_io import load_features as _load_feature_file
from ..features_io import save_features as _save_feature_file
from .algorithm_template import CoverAlgorithm
from .utils.cross_recurrence import nneighbs
from .utils.similarity_fusion import doSimilarityFusion

__all__ = ["EarlyFusion", "resize_block"]


def resize_block(X, i1, i2, frames_per_block, median_aggregate=False):
    """Resample X[i1:i2] to frames_per_block rows (earlyfusion_traile.py:214-247)."""
    from scipy import ndimage
    if median_aggregate:
        raise NotImplementedError("median_aggregate=True needs librosa.util.sync (absent); the reference default "
                                  "is False")
    x = np.asarray(X[i1:i2, :], dtype=np.float64)
    factor = x.shape[0] / float(frames_per_block)
    sigma = max(0.0, (factor - 1.0) / 2.0)
    if sigma > 0:
        x = ndimage.gaussian_filter(x, (sigma, 0.0), mode="constant", cval=0.0)
    ret = ndimage.zoom(x, (frames_per_block / float(x.shape[0]), 1.0), order=1, mode="grid-constant", cval=0.0,
                       grid_mode=True)
    ret[np.isinf(ret)] = 0
    ret[np.isnan(ret)] = 0
    return ret


class EarlyFusion(CoverAlgorithm):
    # the SNF late fusion runs on every rank (row-sharded): every rank needs the assembled Ds
    _Ds_on_every_rank = True
    _takes_candidates = False  # the fusion needs every pair's score

    @classmethod
    def algorithm_name(cls, mutual=False):
        """The name of the Ds cache and the results: 'EarlyFusionTraile' (the reference's row rule),
        'EarlyFusionTraile-mutual' under the mutual nearest-neighbour binarisation."""
        return "EarlyFusionTraile" + _lib.ef_mutual_suffix(mutual)

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='Covers80', blocksize=20,
                 mfccs_per_block=50, ssm_res=50, chromas_per_block=40, kappa=0.1, K=10, niters=5, log_times=False,
                 cachedir="cache", mutual=False, early_snf=False):
        """mutual=True: every binary matrix of this object (similarity, localize, align_path,
        pair_matrices, pair_fusion, the early_snf score) keeps a cell only if it is among the
        nearest neighbours of its row AND of its column (Tralie 2017; include/acoss_hip.h, "mutual")
        instead of the reference's row rule."""
        name = self.algorithm_name(mutual)
        self.mutual = bool(mutual)
        self.chroma_type = chroma_type
        self.blocksize = blocksize
        self.mfccs_per_block = mfccs_per_block
        self.chromas_per_block = chromas_per_block
        self.kappa = kappa
        self.K = K
        self.niters = niters
        # early_snf=True adds the per-pair similarity network fusion score (acoss_earlyfusion_snf:
        # niters rounds of cross-diffusion of the three (M+N) x (M+N) parent matrices of a pair)
        self.early_snf = bool(early_snf)
        if self.early_snf:
            _lib.ef_snf_check_args(kappa, K, niters, 1.0)
        self.all_block_feats = {}
        self.log_times = log_times
        if log_times:
            self.times = {'features': [], 'raw': []}
        self._dev = {}
        self._pending = []  # background cache writes (flush_cache)
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name=name, datapath=datapath,
                                shortname=shortname,
                                similarity_types=["mfccs", "ssms", "chromas", "early"] +
                                (["early_snf"] if self.early_snf else []), cachedir=cachedir)

    def get_cacheprefix(self):
        return "%s/%s_%s_%s" % (self.cachedir, self.name, self.shortname, self.chroma_type)

    def _block_cacheprefix(self):
        """The per-song block-feature files: they do not depend on `mutual`, so both share them."""
        return "%s/%s_%s_%s" % (self.cachedir, self.algorithm_name(), self.shortname, self.chroma_type)

    def load_features(self, i, do_plot=False):
        """Blocked features of song i: 'mfccs', 'ssms', 'chromas', 'chroma_med' (:67-154),
        cached in memory and on disk ('<prefix>_<i>.npz'); computed on the GPU."""
        filepath = "%s_%i.h5" % (self._block_cacheprefix(), i)
        if i in self.all_block_feats:
            return self.all_block_feats[i]
        try:
            self.all_block_feats[i] = _load_feature_file(filepath)
            CoverAlgorithm.load_features(self, i)
            return self.all_block_feats[i]
        except IOError:
            pass
        return self._compute_blocks([i])[0]

    def _compute_blocks(self, idx):
        """Block features of songs idx in one acoss_ef_block_features launch; cached in memory and
        on disk like load_features. Under torch.distributed every rank computes the blocks on its
        own GPU (one launch per 256 songs) and only rank 0 writes the disk cache, so W ranks do not
        write the same 15,000 files W times."""
        tic = time.time()
        from ..features_io import load_many
        feats = load_many([self.filepaths[i] for i in idx],
                          keys=(self.chroma_type, "mfcc_htk", "madmom_features", "label"))
        for i, f in zip(idx, feats):
            self._record_clique(i, f["label"])
        chroma = [np.asarray(f[self.chroma_type], np.float32) for f in feats]
        mfcc = [np.array(f['mfcc_htk'], dtype=np.float32).T for f in feats]
        onsets = [np.asarray(f['madmom_features']['onsets'], np.int64) for f in feats]
        out = _lib.ef_block_features(chroma, mfcc, onsets, self.blocksize, self.mfccs_per_block,
                                     self.chromas_per_block)
        host = {k: out[k].cpu().numpy() for k in ("mfccs", "ssms", "chromas", "chroma_med")}
        from .algorithm_template import _dist_info
        write_cache = _dist_info()[1] == 0
        res = []
        for t, i in enumerate(idx):
            b0, nb = int(out["block_off"][t]), int(out["n_blocks"][t])
            bf = {"mfccs": host["mfccs"][b0:b0 + nb], "ssms": host["ssms"][b0:b0 + nb],
                  "chromas": host["chromas"][b0:b0 + nb], "chroma_med": host["chroma_med"][t]}
            self.all_block_feats[i] = bf
            if write_cache:  # on a background thread: ~1 ms of np.savez per song (15 s at 15,000 songs)
                self._pending.append(self._cache_writer().submit(
                    _save_feature_file, "%s_%i.h5" % (self._block_cacheprefix(), i), bf))
            res.append(bf)
        if self.log_times:
            self.times['features'].append((time.time() - tic) / max(1, len(idx)))
        return res

    def _cache_writer(self):
        """One background thread for the block-feature disk cache, so the ~1 ms np.savez per song
        overlaps the GPU work that follows prepare() instead of adding to it. The exit hook holds
        only a weak reference, so it never keeps an instance (its ~2 GB of block features at
        Da-TACOS size, its device tensors) alive."""
        if getattr(self, "_writer", None) is None:
            import atexit
            import weakref
            from concurrent.futures import ThreadPoolExecutor
            self._writer = ThreadPoolExecutor(max_workers=1)
            ref = weakref.ref(self)

            def _flush_at_exit():
                obj = ref()
                if obj is not None:
                    obj.flush_cache()

            self._atexit = _flush_at_exit
            atexit.register(_flush_at_exit)
        return self._writer

    def flush_cache(self):
        """Wait until every block-feature cache file of prepare() is on disk (re-raises the first
        failed write), then stop the writer thread; all_pairwise and interpreter exit call it."""
        pending, self._pending = self._pending, []
        writer, self._writer = getattr(self, "_writer", None), None
        hook = getattr(self, "_atexit", None)
        if hook is not None:
            import atexit
            atexit.unregister(hook)
            self._atexit = None
        try:
            for f in pending:
                f.result()
        finally:
            if writer is not None:
                writer.shutdown(wait=True)

    def all_pairwise(self, *args, **kwargs):
        try:
            out = CoverAlgorithm.all_pairwise(self, *args, **kwargs)
        except BaseException:
            try:  # the scoring error is the one to see; a cache-write error is only chained
                self.flush_cache()
            except Exception as e:  # noqa: BLE001
                import warnings
                warnings.warn("EarlyFusion block-feature cache write failed: %r" % (e,))
            raise
        self.flush_cache()
        return out

    def _device(self, i):
        if i not in self._dev:
            torch = _lib._torch()
            f = self.load_features(i)
            self._dev[i] = {k: torch.as_tensor(np.ascontiguousarray(f[k], np.float32)).cuda()
                            for k in ("mfccs", "ssms", "chromas")}
            self._dev[i]["chroma_med"] = np.asarray(f["chroma_med"], np.float32)
        return self._dev[i]

    def pair_matrices(self, i, j):
        """The four binary matrices of pair (i, j) (device uint8), in score order
        mfccs, ssms, chromas, early (:157-189); under `mutual` the mutual masks (the batched
        pipeline's row launch and column pass, through acoss_binarize_mutual)."""
        torch = _lib._torch()
        a, b = self._device(i), self._device(j)
        csms = {}
        csms['mfccs'] = _lib.csm(a['mfccs'], b['mfccs'], kind="euclidean")
        csms['ssms'] = _lib.csm(a['ssms'], b['ssms'], kind="euclidean")
        oti = int(_lib.get_oti(a['chroma_med'], b['chroma_med']).item())
        csms['chromas'] = _lib.csm(a['chromas'], b['chromas'], kind="cosine", oti_shift=oti)
        ncols = csms['mfccs'].shape[1]
        nn = nneighbs(self.kappa, ncols)
        wsum = torch.zeros_like(csms['mfccs'])
        for s in ('mfccs', 'ssms', 'chromas'):
            wsum += _lib.wcsm(csms[s], self.K, self.K, 0.5)
        four = [csms[s] for s in ('mfccs', 'ssms', 'chromas')] + [_lib.neg_exp(wsum)]
        if self.mutual:
            err = _lib.ef_neighbour_error([four[0].shape[0]], [ncols], self.kappa, self.K, True)
            if err is not None:
                raise err
            return _lib.binarize_mutual(four, self.kappa)
        return [_lib.binarize_rows(D, nn) for D in four]

    def _bank(self):
        """All tracks' block features packed once into HBM for the batched kernels."""
        if getattr(self, "_dev_bank", None) is None:
            torch = _lib._torch()
            self.prepare()
            feats = [self.load_features(i) for i in range(self.N)]
            nb = np.array([f["mfccs"].shape[0] for f in feats], np.int32)
            off = np.zeros(self.N, np.int64)
            off[1:] = np.cumsum(nb[:-1])

            def cat(key):
                return torch.as_tensor(np.ascontiguousarray(np.concatenate([f[key] for f in feats]), np.float32)).cuda()

            self._dev_bank = {"mfccs": cat("mfccs"), "ssms": cat("ssms"), "chromas": cat("chromas"),
                              "chroma_med": torch.as_tensor(np.stack([np.asarray(f["chroma_med"], np.float32)
                                                                      for f in feats])).cuda(),
                              "off": torch.as_tensor(off).cuda(), "nb": torch.as_tensor(nb).cuda(), "nb_host": nb,
                              "max_blocks": int(nb.max())}
        return self._dev_bank

    def similarity(self, idxs, do_plot=False):
        """The four scores of every pair, one batched C-ABI call (acoss_earlyfusion)."""
        idxs = np.asarray(idxs)
        if len(idxs) == 0:
            return
        tic = time.time()
        scores = _lib.earlyfusion(self._bank(), idxs.astype(np.int32), self.kappa, self.K,
                                  mutual=self.mutual).cpu().numpy()
        if self.log_times:
            self.times['raw'].append((time.time() - tic) / len(idxs))
        for s, key in enumerate(("mfccs", "ssms", "chromas", "early")):
            self.Ds[key][idxs[:, 0], idxs[:, 1]] = scores[:, s]
        if self.early_snf:
            snf = _lib.earlyfusion_snf(self._bank(), idxs.astype(np.int32), self.kappa, self.K, self.niters,
                                       mutual=self.mutual)
            self.Ds["early_snf"][idxs[:, 0], idxs[:, 1]] = snf["score"].cpu().numpy()

    def _device_scores(self, idxs):
        """The four scores of every pair as float32 device tensors (the memmap's dtype), from one
        acoss_earlyfusion call: all_pairwise keeps the stripe on the device and all-gathers it
        across ranks (algorithm_template._device_all_pairwise)."""
        idxs = np.asarray(idxs)
        tic = time.time()
        sc = _lib.earlyfusion(self._bank(), idxs.astype(np.int32), self.kappa, self.K, mutual=self.mutual)
        if self.log_times:
            self.times['raw'].append((time.time() - tic) / max(1, len(idxs)))
        out = {key: sc[:, s].float() for s, key in enumerate(("mfccs", "ssms", "chromas", "early"))}
        if self.early_snf:
            out["early_snf"] = _lib.earlyfusion_snf(self._bank(), idxs.astype(np.int32), self.kappa, self.K,
                                                    self.niters, mutual=self.mutual)["score"].float()
        return out

    def pair_fusion(self, i, j):
        """(cross, binary) of pair (i, j): the M x N cross block F[:M, M:] + F[M:, :M].T of the pair's
        fused matrix (host float64; NaN where the reference cannot fuse the pair) and the binary
        matrix the early_snf score aligns, as the device wrote it (host uint8: round(kappa N) ones per
        row at the largest values, ties to the lowest column; under `mutual` only those also among
        the round(kappa M) largest of their column; all zero where the pair cannot be fused). Beside
        pair_matrices, for the plots of the reference's do_plot branch (:184-196)."""
        r = _lib.earlyfusion_snf(self._bank(), np.array([[i, j]], np.int32), self.kappa, self.K, self.niters,
                                 want_cross=True, mutual=self.mutual, want_binary=True)
        nb = self._bank()["nb_host"]
        shape = (int(nb[i]), int(nb[j]))
        return r["cross"].cpu().numpy().reshape(shape), r["binary"].cpu().numpy().reshape(shape)

    def _onsets(self, songs):
        """{song: (beat onsets int64, chroma frame count)} read from the songs' feature files; the
        block-feature cache holds neither."""
        from ..features_io import load_many
        songs = [int(i) for i in songs]
        feats = load_many([self.filepaths[i] for i in songs], keys=(self.chroma_type, "madmom_features"))
        out = {}
        for i, f in zip(songs, feats):
            mm = f.get("madmom_features")
            if not isinstance(mm, dict) or "onsets" not in mm or self.chroma_type not in f:
                raise ValueError("frames=True needs the beat onsets ('madmom_features'/'onsets') and the '%s' chroma "
                                 "of song %d, and %s has none: the cached block features do not keep them"
                                 % (self.chroma_type, i, self.filepaths[i]))
            out[i] = (np.asarray(mm["onsets"], np.int64).reshape(-1), len(f[self.chroma_type]))
        return out

    def localize(self, idxs, frames=False):
        """Where the four Smith-Waterman alignments of every (query, reference) pair of idxs lie
        (acoss_earlyfusion_locate): a dict of host arrays 'scores' (P, 4) in the order mfccs, ssms,
        chromas, early (similarity()'s values), 'cells' (P, 4, 4) = (r0, c0, r1, c1) in beat blocks
        of the query (rows) and the reference (columns), 'query_blocks' and 'reference_blocks'
        (P, 4, 2): the same as half-open block ranges [r0, r1 + 1) and [c0, c1 + 1). A matrix whose
        score is 0 has cells (-1, -1, -1, -1) and ranges (-1, -1).
        frames=True adds 'query_frames' and 'reference_frames' (P, 4, 2): half-open ranges of
        `chroma_type` frames (engine.block_frames), from the beat onsets of the songs involved,
        read from their feature files on demand; a ValueError names a song whose file has none.
        Not collective: a rank localises the pairs it is given."""
        idxs = np.asarray(idxs, np.int32).reshape(-1, 2)
        r = _lib.earlyfusion_locate(self._bank(), idxs, self.kappa, self.K, mutual=self.mutual)
        cells = r["seg"].cpu().numpy()
        out = {"scores": r["scores"].cpu().numpy(), "cells": cells}
        none = cells[:, :, 0] < 0
        for key, lo, hi in (("query_blocks", 0, 2), ("reference_blocks", 1, 3)):
            b = np.stack([cells[:, :, lo], cells[:, :, hi] + 1], 2).astype(np.int64)
            b[none] = -1
            out[key] = b
        if frames:
            from ..engine import block_frames
            on = self._onsets(np.unique(idxs))
            for key, col, lo, hi in (("query_frames", 0, 0, 2), ("reference_frames", 1, 1, 3)):
                fr = np.full((len(idxs), 4, 2), -1, np.int64)
                for p, song in enumerate(idxs[:, col]):
                    o, n = on[int(song)]
                    fr[p] = block_frames(cells[p][:, [lo, hi]], o, self.blocksize, n)
                out[key] = fr
        return out

    def align_path(self, idxs):
        """The four alignments of every (query, reference) pair of idxs, cell by cell
        (acoss_earlyfusion_path): a dict of host arrays 'scores' (P, 4) and 'cells' (P, 4, 4) as
        localize, 'path_off' (4 P + 1,) int64 and 'path_cells' (total, 2) int32. The path of matrix s
        (mfccs, ssms, chromas, early) of pair p is path_cells[path_off[4 p + s]:path_off[4 p + s + 1]]:
        (query block, reference block) from cells[p, s, :2] to cells[p, s, 2:], each step (1, 1),
        (2, 1) or (1, 2); empty where the score is 0. Not collective."""
        idxs = np.asarray(idxs, np.int32).reshape(-1, 2)
        r = _lib.earlyfusion_path(self._bank(), idxs, self.kappa, self.K, mutual=self.mutual)
        return {"scores": r["scores"].cpu().numpy(), "cells": r["seg"].cpu().numpy(),
                "path_off": r["path_off"].cpu().numpy(), "path_cells": r["cells"].cpu().numpy()}

    def track_lengths(self):
        """Beat blocks per song: a pair costs nb_i * nb_j (three CSMs, four SW), so the row
        stripes balance that (acoss.distributed.stripe_bounds with m = tau = 0)."""
        self.prepare()
        return np.array([max(1, self.all_block_feats[i]["mfccs"].shape[0]) for i in range(self.N)], np.int64)

    def prepare(self, chunk=256):
        """Every song's block features: from the memory / disk cache, the rest on the GPU in
        batches of `chunk` songs. The cached block features and the cached songs' labels are read
        by the native reader in two batched calls (features_io.load_many), not one np.load per
        file."""
        if not self._prepared:
            from ..features_io import cache_readable, load_many
            todo = [i for i in range(self.N) if i not in self.all_block_feats]
            paths = {i: "%s_%i.h5" % (self._block_cacheprefix(), i) for i in todo}
            have = [i for i in todo if cache_readable(paths[i])]
            if have:
                for i, bf in zip(have, load_many([paths[i] for i in have])):
                    self.all_block_feats[i] = bf
                for i, f in zip(have, load_many([self.filepaths[i] for i in have], keys=("label",))):
                    self._record_clique(i, f["label"])
            done = set(have)
            missing = [i for i in todo if i not in done]
            for c0 in range(0, len(missing), chunk):
                self._compute_blocks(missing[c0:c0 + chunk])
            self._prepared = True

    def do_late_fusion(self):
        """SNF of 1/(1 + D) for the late and early+late outputs (:200-206)."""
        self.Ds["late"] = doSimilarityFusion([1.0 / (1.0 + self.Ds[s]) for s in ["chromas", "ssms", "mfccs"]], K=20,
                                             niters=20, reg_diag=1)[1]
        self.Ds["early+late"] = doSimilarityFusion([1.0 / (1.0 + self.Ds[s])
                                                    for s in ["chromas", "ssms", "mfccs", "early"]], K=20, niters=20,
                                                   reg_diag=1)[1]


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description="Benchmarking with Early Similarity Network Fusion of HPCP, MFCC, "
                                                 "and MFCC SSMs",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-i", '--dataset_csv', type=str, action="store", help="Input dataset csv file")
    parser.add_argument("-d", '--datapath', type=str, action="store", default='../features_covers80',
                        help="Path to data files")
    parser.add_argument("-s", "--shortname", type=str, action="store", default="Covers80", help="Short name for dataset")
    parser.add_argument("-c", '--chroma_type', type=str, action="store", default='hpcp',
                        help="Type of chroma to use for experiments")
    parser.add_argument("-p", '--parallel', type=int, choices=(0, 1), action="store", default=0, help="Ignored")
    parser.add_argument("-n", '--n_cores', type=int, action="store", default=1, help="Ignored")
    parser.add_argument("-l", '--log_times', type=int, choices=(0, 1), action="store", default=0,
                        help="Whether to log times to a file")
    cmd_args = parser.parse_args()
    ef = EarlyFusion(dataset_csv=cmd_args.dataset_csv, datapath=cmd_args.datapath, chroma_type=cmd_args.chroma_type,
                     shortname=cmd_args.shortname, log_times=bool(cmd_args.log_times))
    for i in range(len(ef.filepaths)):
        ef.load_features(i)
    ef.all_pairwise(cmd_args.parallel, cmd_args.n_cores, symmetric=True)
    ef.do_late_fusion()
    for similarity_type in ef.Ds:
        ef.getEvalStatistics(similarity_type)
    ef.cleanup_memmap()
    if ef.log_times:
        for s in ef.times:
            print("%s: %.3g" % (s, np.mean(ef.times[s])))
    print("... Done ....")
