"""Locating and tracing the dmax (chen17) alignment (acoss_crp_locate_dmax, acoss_crp_path_dmax)
against scoring dmax alone (acoss_crp_align, dmax only) and against the Qmax twins
(acoss_crp_locate, acoss_crp_path) on the same pair lists. One JSON, also written to
profiles/dmax_path/bench_dmax_path.json.

    python tools/bench_dmax_path.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                                    [--no-headline] [--no-short] [--out path.json]

The two shapes of tools/bench_locate.py and tools/bench_path.py:
  headline:  the bench.py corpus, 164 covers80-shaped tracks of exactly 2,000 frames, all 13,366
             unordered pairs (one CRP of 1,991 x 1,991 per pair: 16 rows per lane, two bands).
  shortlist: the Da-TACOS-shaped rerank case, --short-tracks tracks of 350..700 frames, each against
             --short-k others drawn at random (CRPs of 341..691 rows: both rows-per-lane choices).
Per shape, in one process and alternating: --warmup untimed rounds, then --repeats timed ones of
the five calls `crp_align(dmax)`, `crp_locate`, `crp_locate(align=1)`, `crp_path`,
`crp_path(align=1)`, each closed by a device synchronisation (the path calls include the compaction
of their padded output on the device); the JSON holds every time, the medians, min..max as the
spread, and the ratios of the dmax calls to their Qmax twins and to the bare dmax score. Then one
call of each with the library's phase events on (HIP events around the launches on the launch
stream): the tracing DP ("dp_trace"), the direction DP ("dp_dir") and the backtrack ("backtrack")
of both aligners, beside the shipped chen17 DP ("dp_dmax"). dmax and seg of the three dmax routes
must be equal and every path must start and end on its seg; the run fails otherwise.
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
    print("[dmax_path %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


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
    bank = (d_feats, d_off, d_len, max_len, d_pairs, P)
    calls = {
        "score_dmax": lambda: _lib.crp_align(*bank, qmax=False, dmax=True),
        "locate_qmax": lambda: _lib.crp_locate(*bank),
        "locate_dmax": lambda: _lib.crp_locate(*bank, align=1),
        "path_qmax": lambda: _lib.crp_path(*bank),
        "path_dmax": lambda: _lib.crp_path(*bank, align=1),
    }
    times = {key: [] for key in calls}
    last = {}
    for it in range(a.warmup + a.repeats):
        for key, fn in calls.items():
            s, last[key] = _timed(fn, torch)
            if it >= a.warmup:
                times[key].append(s)
    rs, rl, rp = last["score_dmax"], last["locate_dmax"], last["path_dmax"]
    dmax_equal = bool(torch.equal(rs["dmax"], rl["dmax"]) and torch.equal(rs["dmax"], rp["dmax"]))
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
    # intermediate cells: those left by a (1, 0) or (0, 1) step inside one pair's path
    step = np.diff(cells, axis=0)
    inside = np.ones(len(step), bool)
    joins = poff[1:-1] - 1  # the last cell of a path and the first of the next
    inside[joins[(joins >= 0) & (joins < len(step))]] = False
    short = int((inside & (step.min(axis=1) == 0) & (step.max(axis=1) == 1)).sum()) if len(step) else 0
    qseg = last["path_qmax"]["seg"].cpu().numpy()
    # the launches alone, by the library's HIP events
    ph_ms = {}
    for tag, keys in (("score_dmax", ("dp_dmax",)), ("locate_qmax", ("dp_trace",)), ("locate_dmax", ("dp_trace",)),
                      ("path_qmax", ("dp_dir", "backtrack")), ("path_dmax", ("dp_dir", "backtrack"))):
        _lib.profile_enable(True)
        calls[tag]()
        torch.cuda.synchronize()
        ph = _lib.profile_read()
        _lib.profile_enable(False)
        suffix = "" if tag == "score_dmax" else "_" + tag.split("_")[1]
        for key in keys:
            ph_ms[key + suffix + "_ms"] = round(ph[key][0], 4)
            ph_ms[key + suffix + "_launches"] = ph[key][1]
    med = {key: _summary(t) for key, t in times.items()}
    ratio = lambda x, y: round(med[x]["median_s"] / med[y]["median_s"], 3)
    out = {"tracks": len(tracks), "frames_min": int(lens.min()), "frames_max": max_len, "pairs": int(len(pairs))}
    out.update(med)
    out.update({
        "ratio_locate_dmax_over_locate_qmax": ratio("locate_dmax", "locate_qmax"),
        "ratio_path_dmax_over_path_qmax": ratio("path_dmax", "path_qmax"),
        "ratio_locate_dmax_over_score_dmax": ratio("locate_dmax", "score_dmax"),
        "ratio_path_dmax_over_score_dmax": ratio("path_dmax", "score_dmax"),
        "dmax_equal": dmax_equal, "seg_equal": seg_equal, "path_ends_on_seg": ends_ok,
        "pairs_with_path": int(found.sum()), "path_cells_total": int(poff[-1]), "intermediate_cells": short,
        "path_cells_median": float(np.median(n[found])) if found.any() else None,
        "path_cells_max": int(n.max()) if len(n) else 0,
        "pairs_whose_segment_differs_from_qmax": int((qseg != seg).any(axis=1).sum())})
    out.update(ph_ms)
    for key in ("dp_trace", "dp_dir", "backtrack"):
        out["ratio_%s_dmax_over_qmax" % key] = round(ph_ms[key + "_dmax_ms"] / ph_ms[key + "_qmax_ms"], 2)
    out["ratio_dp_trace_dmax_over_dp_dmax"] = round(ph_ms["dp_trace_dmax_ms"] / ph_ms["dp_dmax_ms"], 2)
    out["ratio_dp_dir_dmax_over_dp_dmax"] = round(ph_ms["dp_dir_dmax_ms"] / ph_ms["dp_dmax_ms"], 2)
    res[name] = out
    res["ok"] = res.get("ok", True) and dmax_equal and seg_equal and ends_ok
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmax_path", "bench_dmax_path.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dmax_path.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "dmax_path", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats}
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
