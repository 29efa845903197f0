"""Benchmark entry point (acoss/coverid.py): `benchmark(...)` and `algorithm_names`.

Same dispatch and call sequence per algorithm as the reference (coverid.py:22-148). Two
reference defects are not reproduced: "EarlyFusionTraile" dispatches
(the reference only matches "EarlyFusion", :72), and `parallel` does not crash (the pairs
are batched on the GPU; with torch.distributed initialised every rank takes a stripe).
All five names of `algorithm_names` run on the engine; FTM2D (coverid.py:107-122) makes its
shingles in `prepare()` and scores the pairs symmetrically.
`shortlist=k` (not in the reference) spends an alignment only on each song's k best FTM2D
candidates: Serra09 and SiMPle score the pairs FTM2D.shortlist(k) names and leave the rest -inf.
"""
import argparse
import sys
import time

from .utils import log

__all__ = ['benchmark', 'algorithm_names']

_LOG_FILE_PATH = "acoss.coverid.log"

algorithm_names = ["Serra09", "EarlyFusionTraile", "LateFusionChen", "FTM2D", "SiMPle"]
shortlist_algorithms = ("Serra09", "SiMPle")  # the alignment scorers that take an FTM2D shortlist
binarize_algorithms = ("Serra09", "LateFusionChen")  # the scorers on a CRP, which take its binarisation and n_oti
mutual_algorithms = ("EarlyFusionTraile", "EarlyFusion")  # the mutual nearest-neighbour binarisation


def benchmark(dataset_csv, feature_dir, feature_type="hpcp", algorithm="Serra09", shortname="covers80",
              parallel=True, n_workers=-1, cachedir="cache", shortlist=None, measure="qmax", binarize="percentile",
              oti_rank=1, mutual=False, n_oti=1):
    """Run one cover-ID algorithm over a dataset CSV and print/write its evaluation statistics.
    Returns the algorithm object (its Ds hold the similarity matrices).
    shortlist: None, or k: Serra09 / SiMPle score only each song's k best FTM2D candidates (shingles
    made from the same CSV, features, chroma type and cache directory); the entries of Ds they do
    not score are -inf.
    measure: what Serra09 fills Ds with, one of Serra09.MEASURES ('qmax', the reference's, 'smax', 'lmax',
    'det', 'lmean', 'entr', 'rr'); any other than 'qmax' runs, caches and reports as 'Serra09-<measure>'.
    binarize, oti_rank: Serra09 / LateFusionChen on the OTI-binary CRP of Serra08 (binarize='oti', oti_rank in
    1 .. 12; include/acoss_hip.h, acoss_crp_params2) in place of the percentile CRP; they run, cache and report
    as 'Serra09-otib', 'LateFusionChen-otib', with the rank appended above 1.
    n_oti: Serra09 / LateFusionChen keep the best score over the n_oti (1 .. 12) most probable transpositions of the
    ranked OTI (include/acoss_hip.h, acoss_crp_params3); above 1 they run, cache and report with '-oti<n>' appended:
    'Serra09-oti2'.
    mutual: EarlyFusionTraile binarises by mutual nearest neighbours (Tralie 2017; include/acoss_hip.h,
    "mutual") in place of the reference's row rule; it runs, caches and reports as 'EarlyFusionTraile-mutual'."""
    logger = log(_LOG_FILE_PATH)
    if algorithm not in algorithm_names and algorithm != "EarlyFusion":
        warn = ("acoss.coverid: Couldn't find '%s' algorithm in acoss Available cover id algorithms are %s "
                % (algorithm, str(algorithm_names)))
        logger.debug(warn)
        raise NotImplementedError(warn)
    if shortlist is not None and algorithm not in shortlist_algorithms:
        raise ValueError("shortlist is supported by %s only, not by '%s'"
                         % (" and ".join(shortlist_algorithms), algorithm))
    if measure != "qmax" and algorithm != "Serra09":
        raise ValueError("measure is supported by Serra09 only, not by '%s'" % algorithm)
    from ._lib import check_binarize
    oti_rank = check_binarize(binarize, oti_rank)
    if (binarize != "percentile" or oti_rank != 1) and algorithm not in binarize_algorithms:
        raise ValueError("binarize and oti_rank are supported by %s only, not by '%s'"
                         % (" and ".join(binarize_algorithms), algorithm))
    from ._lib import check_n_oti
    n_oti = check_n_oti(n_oti)
    if n_oti != 1 and algorithm not in binarize_algorithms:
        raise ValueError("n_oti is supported by %s only, not by '%s'" % (" and ".join(binarize_algorithms), algorithm))
    from ._lib import check_ef_binarize
    if check_ef_binarize(mutual) and algorithm not in mutual_algorithms:
        raise ValueError("mutual is supported by EarlyFusionTraile only, not by '%s'" % algorithm)
    logger.info("Running acoss cover identification benchmarking for the algorithm - '%s'" % algorithm)
    start = time.monotonic()
    kw = dict(dataset_csv=dataset_csv, datapath=feature_dir, chroma_type=feature_type, shortname=shortname,
              cachedir=cachedir)
    candidates = None
    if shortlist is not None:
        from . import evaluation
        from .algorithms.ftm2d import FTM2D
        first = FTM2D(**kw)
        candidates = first.shortlist(int(shortlist))
        logger.info("FTM2D shortlist of %d per song: recall of the same-clique pairs %.4f"
                    % (int(shortlist), evaluation.shortlist_recall(candidates, first.cliques)))
        first.cleanup_memmap()
        del first
    if algorithm == "Serra09":
        from .algorithms.rqa_serra09 import Serra09
        algo = Serra09(measure=measure, binarize=binarize, oti_rank=oti_rank, n_oti=n_oti, **kw)
        logger.info('Computing pairwise similarity...')
        algo.all_pairwise(parallel, n_cores=n_workers, symmetric=True, candidates=candidates)
        algo.normalize_by_length()
    elif algorithm in ("EarlyFusionTraile", "EarlyFusion"):
        from .algorithms.earlyfusion_traile import EarlyFusion
        algo = EarlyFusion(mutual=mutual, **kw)
        # the reference's load_features(i) loop (coverid.py:80-81): the same per-song caches and clique
        # bookkeeping, with the uncached songs' block features made ceil(N / 256) launches at a time
        algo.prepare()
        logger.info('Feature loading done...')
        logger.info('Computing pairwise similarity...')
        algo.all_pairwise(parallel, n_cores=n_workers, symmetric=True)
        algo.do_late_fusion()
    elif algorithm == "LateFusionChen":
        from .algorithms.latefusion_chen import ChenFusion
        algo = ChenFusion(binarize=binarize, oti_rank=oti_rank, n_oti=n_oti, **kw)
        logger.info('Computing pairwise similarity...')
        algo.all_pairwise(parallel, n_cores=n_workers, symmetric=True)
        algo.normalize_by_length()
        algo.do_late_fusion()
    elif algorithm == "SiMPle":
        from .algorithms.simple_silva import Simple
        algo = Simple(**kw)
        algo.prepare()
        logger.info('Feature loading done...')
        logger.info('Computing pairwise similarity...')
        algo.all_pairwise(parallel, n_cores=n_workers, symmetric=False, candidates=candidates)
    else:  # "FTM2D" (coverid.py:107-122)
        from .algorithms.ftm2d import FTM2D
        algo = FTM2D(**kw)
        # the reference's load_features(i) loop (:114-115): every shingle in one launch
        algo.prepare()
        logger.info('Feature loading done...')
        logger.info('Computing pairwise similarity...')
        algo.all_pairwise(parallel, n_cores=n_workers, symmetric=True)
    logger.info('Running benchmark evaluations on the given dataset - %s' % dataset_csv)
    for similarity_type in list(algo.Ds.keys()):
        algo.getEvalStatistics(similarity_type)
    algo.cleanup_memmap()
    logger.info("acoss.coverid benchmarking finished in %s" % (time.monotonic() - start))
    logger.info("Log file located at '%s'" % _LOG_FILE_PATH)
    return algo


def parser_args(cmd_args):
    parser = argparse.ArgumentParser(sys.argv[0], description="Benchmark a specific cover id algorithm with a given "
                                                              "input dataset csv annotations",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-i", '--dataset_csv', type=str, action="store", help="Input dataset csv file")
    parser.add_argument("-d", '--feature_dir', type=str, action="store", default='../features_covers80',
                        help="Path to data files")
    parser.add_argument("-m", "--method", type=str, action="store", default="Serra09", help="Algorithm name")
    parser.add_argument("-s", "--shortname", type=str, action="store", default="covers80", help="Dataset short name")
    parser.add_argument("-c", '--chroma_type', type=str, action="store", default="hpcp",
                        help="Type of chroma to use for experiments")
    parser.add_argument("-p", '--parallel', type=int, choices=(0, 1), action="store", default=1,
                        help="Accepted for compatibility")
    parser.add_argument("-n", '--n_workers', type=int, action="store", default=-1, help="Accepted for compatibility")
    parser.add_argument("-k", '--shortlist', type=int, action="store", default=None,
                        help="Serra09 / SiMPle: score only each song's K best FTM2D candidates")
    parser.add_argument('--binarize', type=str, choices=("percentile", "oti"), action="store", default="percentile",
                        help="Serra09 / LateFusionChen: the percentile CRP or the OTI-binary CRP (Serra08)")
    parser.add_argument('--oti-rank', type=int, action="store", default=1,
                        help="with --binarize oti: a cell is a hit when fewer than this many further "
                             "transpositions are closer (1 .. 12)")
    parser.add_argument('--n-oti', type=int, action="store", default=1,
                        help="Serra09 / LateFusionChen: keep the best score over this many of the most probable "
                             "transpositions (1 .. 12)")
    parser.add_argument('--mutual', action="store_true",
                        help="EarlyFusionTraile: binarise by mutual nearest neighbours (rows and columns)")
    return parser.parse_args(cmd_args)


if __name__ == '__main__':
    args = parser_args(sys.argv[1:])
    benchmark(dataset_csv=args.dataset_csv, feature_dir=args.feature_dir, feature_type=args.chroma_type,
              algorithm=args.method, shortname=args.shortname, parallel=bool(args.parallel), n_workers=args.n_workers,
              shortlist=args.shortlist, binarize=args.binarize, oti_rank=args.oti_rank, mutual=args.mutual,
              n_oti=args.n_oti)
