"""Tracing the Qmax alignment path (acoss_crp_path) against locating its two ends (acoss_crp_locate)
on the same pair lists. One JSON, also written to profiles/path/bench_path.json.

    python tools/bench_path.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                               [--no-headline] [--no-short] [--out path.json]

The two shapes of tools/bench_locate.py:
  headline:  the bench.py corpus, 164 covers80-shaped tracks of exactly 2,000 frames, all 13,366
             unordered pairs (one CRP of 1,991 x 1,991 per pair: 16 rows per lane, two bands; a
             direction plane of 1 MB per pair, so the 4 GiB plane budget splits the DP batch).
  shortlist: the Da-TACOS-shaped rerank case, --short-tracks tracks of 350..700 frames, each against
             --short-k others drawn at random (CRPs of 341..691 rows, so one launch mixes both
             rows-per-lane choices of the direction DP).
Per shape, in one process and alternating: --warmup untimed rounds, then --repeats timed ones of
`_lib.crp_locate` (unchanged by the path work: the yardstick) and `_lib.crp_path` (the library call
per chunk of pairs and the compaction of its padded output to the ragged form, on the device), each
call closed by a device synchronisation; the JSON holds every time, the medians, the ratio
path / locate and min..max as the spread. Then one call of each with the library's phase events on
(HIP events around the launches on the launch stream): the direction DP ("dp_dir") and the backtrack
("backtrack") alone, beside the tracing DP ("dp_trace"). qmax and seg of the two routes must be
equal, and every path must start and end on its seg; the run fails otherwise.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd")]

import numpy as np  # noqa: E402


def log(msg, t0=[time.perf_counter()]):
    print("[path %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)),
            "all_s": [round(x, 6) for x in times]}


def stage(a, name, tracks, pairs, res):
    import torch
    from acoss import _lib, synthetic
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    d_feats, d_off = torch.as_tensor(feats).cuda(), torch.as_tensor(off).cuda()
    d_len, d_pairs = torch.as_tensor(lens).cuda(), torch.as_tensor(pairs).cuda()
    max_len = int(lens.max())

    def locate():
        return _lib.crp_locate(d_feats, d_off, d_len, max_len, d_pairs, P)

    def path():
        return _lib.crp_path(d_feats, d_off, d_len, max_len, d_pairs, P)

    tl, tp = [], []
    for it in range(a.warmup + a.repeats):
        sl, rl = _timed(locate, torch)
        sp, rp = _timed(path, torch)
        if it >= a.warmup:
            tl.append(sl)
            tp.append(sp)
    qmax_equal = bool(torch.equal(rl["qmax"], rp["qmax"]))
    seg_equal = bool(torch.equal(rl["seg"], rp["seg"]))
    seg = rp["seg"].cpu().numpy()
    poff = rp["path_off"].cpu().numpy()
    cells = rp["cells"].cpu().numpy()
    n = np.diff(poff)
    found = seg[:, 0] >= 0
    ends_ok = bool(((n > 0) == found).all())
    if found.any():
        ends_ok = ends_ok and bool((cells[poff[:-1][found]] == seg[found, :2]).all()
                                   and (cells[poff[1:][found] - 1] == seg[found, 2:]).all())
    # the launches alone, by the library's HIP events
    ph_ms = {}
    for keys, fn in ((("dp_trace",), locate), (("dp_dir", "backtrack"), path)):
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        ph = _lib.profile_read()
        _lib.profile_enable(False)
        for key in keys:
            ph_ms[key + "_ms"] = round(ph[key][0], 4)
            ph_ms[key + "_launches"] = ph[key][1]
    lo, pa = _summary(tl), _summary(tp)
    out = {"tracks": len(tracks), "frames_min": int(lens.min()), "frames_max": max_len, "pairs": int(len(pairs)),
           "locate": lo, "path": pa, "ratio_path_over_locate": round(pa["median_s"] / lo["median_s"], 3),
           "qmax_equal": qmax_equal, "seg_equal": seg_equal, "path_ends_on_seg": ends_ok,
           "pairs_with_path": int(found.sum()), "path_cells_total": int(poff[-1]),
           "path_cells_median": float(np.median(n[found])) if found.any() else None,
           "path_cells_max": int(n.max()) if len(n) else 0}
    out.update(ph_ms)
    out["ratio_dp_dir_over_dp_trace"] = round(ph_ms["dp_dir_ms"] / ph_ms["dp_trace_ms"], 2)
    res[name] = out
    res["ok"] = res.get("ok", True) and qmax_equal and seg_equal and ends_ok
    log("%s: %s" % (name, json.dumps(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-headline", dest="headline", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path", "bench_path.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_path.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "path", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats}
    if a.headline:
        tracks, _ = synthetic.make_hard_corpus("covers80", frames=2000, seed=a.seed)
        n = len(tracks)
        pairs = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
        stage(a, "headline", tracks, pairs, res)
    if a.short:
        rng = np.random.Generator(np.random.PCG64(a.seed))
        n = a.short_tracks
        tracks = [synthetic.render(rng, synthetic.base_sequence(rng, int(L))) for L in rng.integers(350, 701, n)]
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "shortlist", tracks, pairs, res)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
