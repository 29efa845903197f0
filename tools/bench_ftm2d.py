"""FTM2D throughput: the shingle stage and the pair stage, one JSON line.

    python tools/bench_ftm2d.py [--tracks 164] [--frames 2000] [--beat-period 5]
                                [--datacos-tracks 15000] [--datacos-frames 1500] [--datacos-beat-period 4]
                                [--cpu-sample 32] [--out result.json]

Stage A (library calls, --tracks x --frames): `_lib.ftm2d_shingles` end to end (host packing, upload
and kernels; median of --repeats timed calls after --warmup untimed ones, each closed by a device
synchronisation) and the kernels alone from the library's phase timers (ftm_sync, ftm_dft,
ftm_median); `_lib.ftm2d_scores` on a device-resident list of every ordered pair, repeated to at
least 4 M pairs. The DFT kernel's fraction of the f64 MFMA peak counts the MFMA instructions it
issues (16 x 16 x 4 x 2 flop each; rows c = 0 and 6 run half of K), padding included, against
--peak-tflops.
Stage B (--datacos-tracks > 0): the Da-TACOS benchmark shape (1000 cliques x 13 + 2000 singletons)
through the plugin API as tools/datacos_plugin.py does for the other algorithms: feature files on
disk -> FTM2D(csv, dir).prepare() -> all_pairwise(symmetric=True) -> getEvalStatistics('main').
CPU baseline: the numpy restatement (tests/ftm2d_np.py, never the code under test) on
--cpu-sample songs of stage A, on the threads this process was granted.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402


def log(msg, t0=[time.perf_counter()]):
    print("[ftm2d %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def make_tracks(rng, sizes, frames, beat_period):
    """Cliques of noisy copies of a random chroma; onsets on a jittered grid."""
    tracks, onsets, labels = [], [], []
    for lab, size in enumerate(sizes):
        base = np.abs(rng.standard_normal((frames, 12), dtype=np.float32))
        for v in range(size):
            x = base if v == 0 else np.abs(base + 0.5 * rng.standard_normal((frames, 12), dtype=np.float32))
            tracks.append((x / x.max(1, keepdims=True)).astype(np.float32))
            g = np.arange(beat_period, frames, beat_period)
            onsets.append((g + rng.integers(0, 2, size=len(g))).astype(np.int64))
            labels.append(lab)
    return tracks, onsets, np.asarray(labels, np.int32)


def issued_mfma_flop(nw):
    tiles = (np.asarray(nw, np.int64) + 31) // 32
    return float(np.sum(tiles) * 5 * (5 * 38 + 2 * 19) * 4 * (16 * 16 * 4 * 2))


def stage_a(a, res):
    import torch
    import ftm2d_np
    from acoss import _lib
    rng = np.random.Generator(np.random.PCG64(a.seed))
    tracks, onsets, _ = make_tracks(rng, [1] * a.tracks, a.frames, a.beat_period)
    nw = np.array([len(ftm2d_np.boundaries(o, len(t))) - 75 for t, o in zip(tracks, onsets)])
    times = []
    for it in range(a.warmup + a.repeats):
        if it == a.warmup:
            _lib.profile_enable(True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        sh = _lib.ftm2d_shingles(tracks, onsets)
        torch.cuda.synchronize()
        if it >= a.warmup:
            times.append(time.perf_counter() - t)
    ph = _lib.profile_read()
    _lib.profile_enable(False)
    sec = float(np.median(times))
    kern = {k: round(ph[k][0] / a.repeats, 4) for k in ("ftm_sync", "ftm_dft", "ftm_median") if k in ph}
    dft_s = kern.get("ftm_dft", 0.0) / 1e3
    res["shingles"] = {"tracks": a.tracks, "frames": a.frames, "windows_per_track": float(nw.mean()),
                       "seconds_end_to_end": round(sec, 5), "songs_per_s_end_to_end": round(a.tracks / sec, 1),
                       "kernel_ms": kern, "songs_per_s_kernels": round(a.tracks / (sum(kern.values()) / 1e3), 1),
                       "all_times_s": [round(x, 5) for x in times]}
    if dft_s > 0:
        tf = issued_mfma_flop(nw) / dft_s / 1e12
        res["dft"] = {"issued_mfma_tflops": round(tf, 2), "fraction_of_f64_mfma_peak": round(tf / a.peak_tflops, 4),
                      "peak_tflops_assumed": a.peak_tflops}
    log("shingles: %s" % json.dumps(res["shingles"]))
    # pairs
    n = a.tracks
    ij = np.array([(i, j) for i in range(n) for j in range(n)], np.int32)
    reps = max(1, (4 << 20) // len(ij))
    pairs = torch.from_numpy(np.tile(ij, (reps, 1))).cuda()
    times = []
    for it in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        sc = _lib.ftm2d_scores(sh, pairs)
        torch.cuda.synchronize()
        if it >= a.warmup:
            times.append(time.perf_counter() - t)
    sec = float(np.median(times))
    res["pairs"] = {"pairs": int(len(pairs)), "seconds": round(sec, 5), "pairs_per_s": round(len(pairs) / sec, 1)}
    log("pairs: %s" % json.dumps(res["pairs"]))
    # CPU baseline: the restatement
    k = min(a.cpu_sample, n)
    t = time.perf_counter()
    ref = [ftm2d_np.shingle(tracks[i], onsets[i]) for i in range(k)]
    sec = time.perf_counter() - t
    gap = float(np.abs(sh[:k].cpu().numpy() - np.stack(ref)).max())
    res["numpy_restatement"] = {"songs": k, "seconds": round(sec, 3), "songs_per_s": round(k / sec, 2),
                                "threads": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
                                "max_gap_to_gpu": gap}
    res["ok"] = res.get("ok", True) and gap <= 1e-12
    log("numpy: %s" % json.dumps(res["numpy_restatement"]))


def stage_b(a, res):
    import torch
    from acoss import evaluation, synthetic
    from acoss.algorithms.ftm2d import FTM2D
    from acoss.features_io import save_features
    stages = {}
    t = time.perf_counter()
    sizes = list(synthetic.clique_sizes("datacos"))
    rng = np.random.Generator(np.random.PCG64(a.seed + 1))
    work = a.workdir or tempfile.mkdtemp(prefix="ftm2d_")
    fdir = os.path.join(work, "features") + "/"
    rows, total = [], 0
    for lab, size in enumerate(sizes):  # clique by clique: the corpus never sits in RAM as a whole
        size = min(size, a.datacos_tracks - total)
        if size <= 0:
            break
        tr, on, _ = make_tracks(rng, [size], a.datacos_frames, a.datacos_beat_period)
        for x, o in zip(tr, on):
            w, tid = "W%05d" % lab, "T%06d" % total
            save_features(fdir + w + "/" + tid + ".h5", {"hpcp": x, "label": w, "track_id": tid,
                                                         "madmom_features": {"onsets": o}})
            rows.append((w, tid))
            total += 1
    csv = os.path.join(work, "dataset.csv")
    with open(csv, "w") as fo:
        fo.write("work_id,track_id\n")
        for w, tid in rows:
            fo.write("%s,%s\n" % (w, tid))
    stages["write_features_s"] = round(time.perf_counter() - t, 2)
    log("%d songs written in %.1f s" % (total, stages["write_features_s"]))
    t = time.perf_counter()
    algo = FTM2D(csv, fdir, shortname="datacos", cachedir=os.path.join(work, "cache"))
    algo.prepare()
    torch.cuda.synchronize()
    stages["prepare_s"] = round(time.perf_counter() - t, 2)
    log("prepare (read + shingles) %.1f s" % stages["prepare_s"])
    t = time.perf_counter()
    algo.all_pairwise(symmetric=True)
    torch.cuda.synchronize()
    stages["all_pairwise_s"] = round(time.perf_counter() - t, 2)
    n_pairs = total * (total - 1) // 2
    log("all_pairwise %d pairs %.1f s" % (n_pairs, stages["all_pairwise_s"]))
    D = np.asarray(algo.Ds["main"])
    checks = {"symmetric": bool(np.array_equal(D, D.T)), "diagonal_zero": bool(np.all(np.diag(D) == 0)),
              "finite": bool(np.isfinite(D).all())}
    t = time.perf_counter()
    MR, MRR, MDR, MAP, tops = algo.getEvalStatistics("main")
    stages["eval_device_s"] = round(time.perf_counter() - t, 2)
    res["datacos"] = {"songs": total, "frames": a.datacos_frames, "beat_period": a.datacos_beat_period,
                      "api": "FTM2D(csv, dir).prepare() -> all_pairwise(symmetric=True) -> getEvalStatistics",
                      "pairs": n_pairs, "pairs_per_s_all_pairwise": round(n_pairs / stages["all_pairwise_s"], 1),
                      "songs_per_s_prepare": round(total / stages["prepare_s"], 1), "stages": stages,
                      "MAP": float(MAP), "MR1": float(MR), "checks": checks}
    res["ok"] = res.get("ok", True) and all(checks.values())
    algo.cleanup_memmap()
    if not a.workdir:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=164)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--beat-period", type=int, default=5)
    ap.add_argument("--datacos-tracks", type=int, default=15000)
    ap.add_argument("--datacos-frames", type=int, default=1500)
    ap.add_argument("--datacos-beat-period", type=int, default=4)
    ap.add_argument("--cpu-sample", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--peak-tflops", type=float, default=78.6, help="MI355X f64 matrix peak")
    ap.add_argument("--seed", type=int, default=20251019)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {"bench": "ftm2d", "gpu": torch.cuda.get_device_name(0)}
    stage_a(a, res)
    if a.datacos_tracks > 0:
        stage_b(a, res)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
