"""Cross-recurrence quantification (acoss_crp_rqa), with Smax and without it, against scoring alone
(acoss_crp_align, qmax only) on the same pair lists. One JSON, also written to
profiles/rqa/bench_rqa.json.

    python tools/bench_rqa.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                              [--no-headline] [--no-short] [--parent-lib libacoss_hip.so] [--out path.json]

Two shapes:
  headline:  the bench.py corpus, 164 covers80-shaped tracks of exactly 2,000 frames, all 13,366
             unordered pairs (one CRP of 1,991 x 1,991 per pair: 32 rows per lane, one band).
  shortlist: the Da-TACOS-shaped rerank case, --short-tracks tracks of 350..700 frames, each against
             --short-k others drawn at random (CRPs of 341..691 rows: 16 rows per lane).
Per shape, in the same run and alternating: --warmup untimed rounds, then --repeats timed ones of
`_lib.crp_align(qmax)`, `_lib.crp_rqa(smax=True)` and `_lib.crp_rqa(smax=False)`, each call closed by
a device synchronisation; the JSON holds every time, the medians, the ratios rqa / align and
min..max as the spread. Then one call of each with the library's phase events on: the line walk
("rqa") against the shipped DP ("dp_qmax"; under crp_rqa that phase is the Smax DP). Smax must not
exceed n_rec, and the counts of the two rqa calls must be equal.
--parent-lib: a libacoss_hip.so built from the parent commit. Its acoss_crp_align and this tree's
run alternately in this process on the same pairs (the order swaps every round); both medians, the
spread and whether the scores are equal bit for bit go into the JSON.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd")]

import numpy as np  # noqa: E402


def log(msg, t0=[time.perf_counter()]):
    print("[rqa %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)),
            "all_s": [round(x, 6) for x in times]}


def parent_ab(a, lead, n_pairs):
    """acoss_crp_align (qmax only) of the parent commit's library and of this tree's, alternately."""
    import torch
    from acoss import _lib
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))  # it lacks the new entries: bind the one call
    parent.acoss_crp_align.argtypes = _lib.SIGNATURES["acoss_crp_align"]
    parent.acoss_crp_align.restype = ctypes.c_int
    libs = {"parent": parent, "this": _lib.load_library()}
    out = {k: torch.empty(n_pairs, dtype=torch.float32, device="cuda") for k in libs}

    def call(k):
        rc = libs[k].acoss_crp_align(*lead, _lib._ptr(out[k]), None, None, _lib._stream())
        if rc:
            raise RuntimeError("acoss_crp_align (%s) returned %d" % (k, rc))

    times = {k: [] for k in libs}
    for it in range(a.warmup + a.repeats):
        for k in (list(libs) if it % 2 == 0 else list(libs)[::-1]):  # neither library always runs second
            s, _ = _timed(lambda: call(k), torch)
            if it >= a.warmup:
                times[k].append(s)
    sm = {k: _summary(v) for k, v in times.items()}
    spread = max(v["max_s"] - v["min_s"] for v in sm.values())
    diff = sm["this"]["median_s"] - sm["parent"]["median_s"]
    return {"parent": sm["parent"], "this": sm["this"], "spread_s": round(spread, 6),
            "median_difference_s": round(diff, 6), "agree_within_spread": bool(abs(diff) <= spread),
            "same_scores": bool(torch.equal(out["parent"], out["this"]))}


def stage(a, name, tracks, pairs, res):
    import torch
    from acoss import _lib, synthetic
    feats, off, lens = synthetic.pack(tracks)
    P = _lib.crp_params()
    d_feats, d_off = torch.as_tensor(feats).cuda(), torch.as_tensor(off).cuda()
    d_len, d_pairs = torch.as_tensor(lens).cuda(), torch.as_tensor(pairs).cuda()
    max_len = int(lens.max())
    calls = {
        "align_qmax": lambda: _lib.crp_align(d_feats, d_off, d_len, max_len, d_pairs, P, qmax=True),
        "rqa_smax": lambda: _lib.crp_rqa(d_feats, d_off, d_len, max_len, d_pairs, P, smax=True),
        "rqa": lambda: _lib.crp_rqa(d_feats, d_off, d_len, max_len, d_pairs, P, smax=False),
    }
    times, got = {k: [] for k in calls}, {}
    for it in range(a.warmup + a.repeats):
        for k, fn in calls.items():
            s, got[k] = _timed(fn, torch)
            if it >= a.warmup:
                times[k].append(s)
    counts = got["rqa_smax"]["counts"]
    ok = bool(torch.equal(counts, got["rqa"]["counts"])) and bool(torch.equal(got["rqa_smax"]["stats"],
                                                                              got["rqa"]["stats"]))
    ok = ok and bool((got["rqa_smax"]["smax"].double() <= counts[:, 0].double()).all())
    phases = {}
    for k, fn in calls.items():
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        ph = _lib.profile_read()
        _lib.profile_enable(False)
        phases[k] = {p: {"ms": round(ph[p][0], 4), "launches": ph[p][1]} for p in ("rqa", "dp_qmax") if p in ph}
    sm = {k: _summary(v) for k, v in times.items()}
    st = got["rqa"]["stats"].cpu().numpy()
    out = {"tracks": len(tracks), "frames_min": int(lens.min()), "frames_max": max_len, "pairs": int(len(pairs))}
    out.update(sm)
    out.update({"ratio_rqa_smax_over_align": round(sm["rqa_smax"]["median_s"] / sm["align_qmax"]["median_s"], 3),
                "ratio_rqa_over_align": round(sm["rqa"]["median_s"] / sm["align_qmax"]["median_s"], 3),
                "phases": phases, "consistent": ok,
                "rr_median": float(np.median(st[:, 0])), "det_median": float(np.median(st[:, 1])),
                "lmax_median": float(np.median(got["rqa"]["lmax"].cpu().numpy())),
                "smax_median": float(np.median(got["rqa_smax"]["smax"].cpu().numpy()))})
    dpq = phases["align_qmax"].get("dp_qmax", {}).get("ms")
    if dpq:
        out["ratio_ph_rqa_over_ph_dp_qmax"] = round(phases["rqa"]["rqa"]["ms"] / dpq, 3)
    if a.parent_lib:
        lead = (_lib._ptr(d_feats), _lib._ptr(d_off), _lib._ptr(d_len), int(d_len.shape[0]), max_len,
                _lib._ptr(d_pairs.to(torch.int32).contiguous()), int(len(pairs)), ctypes.byref(P))
        out["align_parent_vs_this"] = parent_ab(a, lead, int(len(pairs)))
        ok = ok and out["align_parent_vs_this"]["same_scores"]
    res[name] = out
    res["ok"] = res.get("ok", True) and ok
    log("%s: %s" % (name, json.dumps(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-headline", dest="headline", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rqa", "bench_rqa.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rqa.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "rqa", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "parent_lib": bool(a.parent_lib)}
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
