"""Locating the Qmax alignment (acoss_crp_locate) against scoring alone (acoss_crp_align, qmax only)
on the same pair lists. One JSON, also written to profiles/locate/bench_locate.json.

    python tools/bench_locate.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                                 [--no-headline] [--no-short] [--out path.json]

Two shapes:
  headline:  the bench.py corpus, 164 covers80-shaped tracks of exactly 2,000 frames, all 13,366
             unordered pairs (one CRP of 1,991 x 1,991 per pair: 16 rows per lane, two bands).
  shortlist: the Da-TACOS-shaped rerank case, --short-tracks tracks of 350..700 frames, each against
             --short-k others drawn at random (a shortlist's pair list; CRPs of 341..691 rows, so one
             launch mixes both rows-per-lane choices of the tracing DP).
Per shape, in the same run and alternating: --warmup untimed rounds, then --repeats timed ones of
`_lib.crp_align(qmax)` and `_lib.crp_locate`, each call closed by a device synchronisation; the JSON
holds every time, the medians, the ratio locate / align and min..max as the spread. Then one call of
each with the library's phase events on (HIP events around the DP launch on the launch stream):
the shipped DP ("dp_qmax") against the tracing DP ("dp_trace") alone. The scores of the two calls
must be equal bit for bit.
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
    print("[locate %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


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

    def align():
        return _lib.crp_align(d_feats, d_off, d_len, max_len, d_pairs, P, qmax=True)

    def locate():
        return _lib.crp_locate(d_feats, d_off, d_len, max_len, d_pairs, P)

    ta, tl = [], []
    for it in range(a.warmup + a.repeats):
        sa, ra = _timed(align, torch)
        sl, rl = _timed(locate, torch)
        if it >= a.warmup:
            ta.append(sa)
            tl.append(sl)
    equal = bool(torch.equal(ra["qmax"], rl["qmax"]))
    seg = rl["seg"].cpu().numpy()
    found = seg[:, 0] >= 0
    # the DP launches alone, by the library's HIP events
    dp = {}
    for key, fn in (("dp_qmax", align), ("dp_trace", locate)):
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        ph = _lib.profile_read()
        _lib.profile_enable(False)
        dp[key + "_ms"] = round(ph[key][0], 4)
        dp[key + "_launches"] = ph[key][1]
    al, lo = _summary(ta), _summary(tl)
    out = {"tracks": len(tracks), "frames_min": int(lens.min()), "frames_max": max_len, "pairs": int(len(pairs)),
           "align_qmax": al, "locate": lo, "ratio_locate_over_align": round(lo["median_s"] / al["median_s"], 3),
           "qmax_equal": equal, "pairs_located": int(found.sum()),
           "rows_spanned_median": float(np.median(seg[found, 2] - seg[found, 0] + 1)) if found.any() else None}
    out.update(dp)
    out["ratio_dp_trace_over_dp_qmax"] = round(dp["dp_trace_ms"] / dp["dp_qmax_ms"], 2)
    res[name] = out
    res["ok"] = res.get("ok", True) and equal
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate", "bench_locate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_locate.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "locate", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats}
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
