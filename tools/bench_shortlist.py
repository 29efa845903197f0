"""Shortlist-and-rerank: the fused FTM2D top-k kernel against the dense route, and Serra09 on a
shortlist against Serra09 on every pair. One JSON, also written to profiles/shortlist/bench_shortlist.json.

    python tools/bench_shortlist.py [--sizes 15000,164] [--dim 900] [--k 100] [--warmup 2] [--repeats 5]
                                    [--datacos-tracks 15000] [--datacos-frames 500] [--beat-period 4]
                                    [--shortlist 100] [--no-unrestricted] [--out path.json]

Stage A (kernel, per size n of --sizes): a table of n random unit-norm float64 rows of --dim.
  fused:    `_lib.ftm2d_topk(table, table, k, self_off=0)`.
  baseline: what the library offered before it: acoss_ftm2d_scores over all n^2 ordered pairs in
            chunks of rows straight into an (n, n) float64 device matrix (the C entry point, without
            the Python wrapper's index checks; the pair lists are built on the device before the
            clock starts), -inf on the diagonal, `torch.topk(matrix, k, dim=1)`.
  Both are timed in the same run, alternating, each call closed by a device synchronisation: --warmup
  untimed rounds, then --repeats timed ones; the JSON holds every time, the medians, the ratio
  baseline / fused and min..max as the spread. The fused kernel's share of the f64 vector peak
  counts the subtract, multiply and add of every (pair, coefficient), 3 n^2 dim flop, against
  --peak-tflops; the peak counts a fused multiply-add as two, and none of these three operations is
  fused (the sum order is pinned), so half the peak is the most this arithmetic can reach.
  Scores of the two routes must be equal bit for bit; indices are compared where a row has no tie
  at its k-th place (torch.topk does not order ties by index).
Stage B (--datacos-tracks > 0): the Da-TACOS benchmark shape of tools/datacos_plugin.py (same
  corpus; the feature files also carry beat onsets every --beat-period frames for the shingles)
  through the plugin classes: FTM2D(csv, dir).shortlist(K) -> shortlist_recall ->
  Serra09(csv, dir, downsample_fac=1).all_pairwise(symmetric=True, candidates=...) ->
  normalize_by_length -> getEvalStatistics, then (unless --no-unrestricted) the same Serra09 on
  every pair on the same machine.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402


def log(msg, t0=[time.perf_counter()]):
    print("[shortlist %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)),
            "all_s": [round(x, 6) for x in times]}


def kernel_stage(a, n, res):
    import torch
    from acoss import _lib
    lib = _lib.load_library()
    k = min(a.k, n - 1)
    g = torch.Generator(device="cuda").manual_seed(a.seed + n)
    table = torch.randn((n, a.dim), dtype=torch.float64, device="cuda", generator=g)
    table /= table.norm(dim=1, keepdim=True)
    rows = max(1, min(n, a.chunk_pairs // n))
    col = torch.arange(n, dtype=torch.int32, device="cuda")
    chunks = []
    for r0 in range(0, n, rows):  # the pair lists live on the device before the clock starts
        r1 = min(n, r0 + rows)
        i = torch.arange(r0, r1, dtype=torch.int32, device="cuda")
        chunks.append((r0, torch.stack([i[:, None].expand(-1, n), col[None, :].expand(r1 - r0, -1)], 2).reshape(-1, 2)
                       .contiguous()))
    matrix = torch.empty((n, n), dtype=torch.float64, device="cuda")

    def baseline():
        for r0, pairs in chunks:
            rc = lib.acoss_ftm2d_scores(_lib._ptr(table), n, a.dim, _lib._ptr(pairs), int(pairs.shape[0]),
                                        _lib._ptr(matrix[r0]), _lib._stream())
            _lib._check(rc, "acoss_ftm2d_scores")
        matrix.fill_diagonal_(float("-inf"))
        return torch.topk(matrix, k, dim=1)

    def fused():
        return _lib.ftm2d_topk(table, table, k, self_off=0)

    tb, tf = [], []
    for it in range(a.warmup + a.repeats):
        sb, (bscore, bidx) = _timed(baseline, torch)
        sf, (fidx, fscore) = _timed(fused, torch)
        if it >= a.warmup:
            tb.append(sb)
            tf.append(sf)
    scores_equal = bool(torch.equal(bscore, fscore))
    # a row whose listed scores are distinct has one answer (a tie at the k-th place itself would still
    # show as an index mismatch: random rows do not tie)
    distinct = (fscore[:, 1:] != fscore[:, :-1]).all(dim=1)
    idx_equal = bool(torch.equal(bidx[distinct].int(), fidx[distinct]))
    b, f = _summary(tb), _summary(tf)
    flop = 3.0 * n * n * a.dim
    out = {"n": n, "dim": a.dim, "k": k, "baseline": b, "fused": f,
           "ratio_baseline_over_fused": round(b["median_s"] / f["median_s"], 3),
           "fused_not_slower": bool(f["median_s"] <= b["median_s"]),
           "fused_slowest_below_baseline_fastest": bool(f["max_s"] <= b["min_s"]),
           "fused_tflops": round(flop / f["median_s"] / 1e12, 3),
           "fused_fraction_of_f64_vector_peak": round(flop / f["median_s"] / 1e12 / a.peak_tflops, 4),
           "peak_tflops_assumed": a.peak_tflops,
           "scores_equal": scores_equal, "indices_equal_on_tie_free_rows": idx_equal,
           "tie_free_rows": int(distinct.sum())}
    res["kernel_n%d" % n] = out
    res["ok"] = res.get("ok", True) and scores_equal and idx_equal
    log("n=%d: %s" % (n, json.dumps(out)))
    del chunks, matrix


def serra_stage(a, res):
    import torch
    import datacos_plugin
    from acoss import evaluation, synthetic
    from acoss.algorithms.ftm2d import FTM2D
    from acoss.algorithms.rqa_serra09 import Serra09
    t = time.perf_counter()
    tracks, labels = datacos_plugin.corpus(a.datacos_tracks, a.datacos_frames, a.seed, "hard")
    n = len(tracks)
    work = a.workdir or tempfile.mkdtemp(prefix="shortlist_")
    csv, fdir = synthetic.write_feature_dataset(work, tracks, labels, with_mfcc=True, beat_period=a.beat_period,
                                                chroma_keys=("hpcp",))
    del tracks
    out = {"songs": n, "frames": a.datacos_frames, "beat_period": a.beat_period, "shortlist": a.shortlist,
           "write_features_s": round(time.perf_counter() - t, 2)}
    log("%d songs written in %.1f s" % (n, out["write_features_s"]))

    def serra(tag, candidates):
        st = {}
        t0 = time.perf_counter()
        algo = Serra09(csv, fdir, shortname="datacos", downsample_fac=1, cachedir=os.path.join(work, "cache_" + tag))
        algo.prepare()
        torch.cuda.synchronize()
        st["prepare_s"] = round(time.perf_counter() - t0, 2)
        t = time.perf_counter()
        algo.all_pairwise(symmetric=True, candidates=candidates)
        torch.cuda.synchronize()
        st["all_pairwise_s"] = round(time.perf_counter() - t, 2)
        t = time.perf_counter()
        algo.normalize_by_length()
        MR, MRR, MDR, MAP, tops = algo.getEvalStatistics("main")
        st["normalize_and_eval_s"] = round(time.perf_counter() - t, 2)
        st["wall_s"] = round(time.perf_counter() - t0, 2)
        st.update(MAP=float(MAP), MR1=float(MR), MRR=float(MRR), top=[int(x) for x in tops])
        algo.cleanup_memmap()
        log("%s: %s" % (tag, json.dumps(st)))
        return st

    t0 = time.perf_counter()
    first = FTM2D(csv, fdir, shortname="datacos", cachedir=os.path.join(work, "cache_ftm2d"))
    first.prepare()
    torch.cuda.synchronize()
    out["ftm2d_prepare_s"] = round(time.perf_counter() - t0, 2)
    t = time.perf_counter()
    cands = first.shortlist(a.shortlist)
    out["ftm2d_shortlist_s"] = round(time.perf_counter() - t, 3)
    out["shortlist_recall"] = float(evaluation.shortlist_recall(cands, first.cliques))
    first.cleanup_memmap()
    del first
    from acoss import distributed
    out["pairs_scored"] = int(len(distributed.candidate_pairs(cands, 0, n, True)))
    out["pairs_dense"] = n * (n - 1) // 2
    log("shortlist: recall %.4f, %d of %d pairs" % (out["shortlist_recall"], out["pairs_scored"], out["pairs_dense"]))
    out["restricted"] = serra("restricted", cands)
    out["restricted_wall_with_shortlist_s"] = round(time.perf_counter() - t0, 2)
    if a.unrestricted:
        out["unrestricted"] = serra("unrestricted", None)
        out["wall_ratio_unrestricted_over_restricted"] = round(
            out["unrestricted"]["wall_s"] / out["restricted_wall_with_shortlist_s"], 2)
    res["serra09_datacos"] = out
    if not a.workdir:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="15000,164")
    ap.add_argument("--dim", type=int, default=900)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk-pairs", type=int, default=1 << 24, help="baseline: pairs per acoss_ftm2d_scores call")
    ap.add_argument("--peak-tflops", type=float, default=78.6, help="MI355X f64 vector peak")
    ap.add_argument("--datacos-tracks", type=int, default=15000)
    ap.add_argument("--datacos-frames", type=int, default=500)
    ap.add_argument("--beat-period", type=int, default=4)
    ap.add_argument("--shortlist", type=int, default=100)
    ap.add_argument("--no-unrestricted", dest="unrestricted", action="store_false")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortlist", "bench_shortlist.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_shortlist.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    res = {"bench": "shortlist", "gpu": torch.cuda.get_device_name(0)}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        kernel_stage(a, n, res)
    if a.datacos_tracks > 0:
        serra_stage(a, res)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
