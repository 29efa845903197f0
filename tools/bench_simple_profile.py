"""The SiMPle matrix profile and its index (acoss_simple_profile) against the score alone
(acoss_simple_mp) on the same pair lists. One JSON, also written to
profiles/simple_profile/bench_simple_profile.json.

    python tools/bench_simple_profile.py [--warmup 2] [--repeats 7] [--short-tracks 2000] [--short-k 100]
                                         [--no-headline] [--no-short] [--out path.json]

The two shapes of tools/bench_locate.py, in SiMPle columns:
  headline:  the bench.py SiMPle corpus, 164 covers80-shaped tracks of exactly 2,000 unit columns,
             all 26,732 ordered pairs (a profile of 1,991 rows per pair).
  shortlist: the Da-TACOS-shaped rerank case, --short-tracks tracks of 350..700 columns, each against
             --short-k others drawn at random (200,000 pairs by default).
Per shape, in the same run, on the same build and alternating: --warmup untimed rounds, then
--repeats timed ones of `_lib.simple_mp_packed` and `_lib.simple_profile_packed`, each call closed by
a device synchronisation (the profile call's time includes allocating its ragged output); the JSON
holds every time, the medians, pairs/s of both, the ratio profile / score and min..max as the spread.
By construction the profile call walks every pair twice, so a ratio near 2 is expected; nothing is
gated on it. The two calls' scores must be equal bit for bit, and on a sample of pairs
median(profile) must equal the score.
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
    print("[simple_profile %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times, pairs):
    med = float(np.median(times))
    return {"median_s": med, "min_s": float(min(times)), "max_s": float(max(times)),
            "pairs_per_s": round(pairs / med, 1), "all_s": [round(x, 6) for x in times]}


def _unit(F):
    return F / np.linalg.norm(F, axis=0, keepdims=True)


def stage(a, name, feats, pairs, res):
    import torch
    from acoss import _lib
    lens = np.array([f.shape[1] for f in feats], np.int32)
    off = np.concatenate([[0], np.cumsum(12 * lens.astype(np.int64))[:-1]])
    d_flat = torch.as_tensor(np.concatenate([f.ravel() for f in feats])).cuda()

    def score():  # host pairs: both calls upload them from pinned memory
        return _lib.simple_mp_packed(d_flat, off, lens, pairs)

    def profile():
        return _lib.simple_profile_packed(d_flat, off, lens, pairs)

    ts, tp = [], []
    for it in range(a.warmup + a.repeats):
        s_, rs = _timed(score, torch)
        p_, rp = _timed(profile, torch)
        if it >= a.warmup:
            ts.append(s_)
            tp.append(p_)
    sc = rs[0].cpu().numpy()
    equal = bool(np.array_equal(sc, rp["score"].cpu().numpy(), equal_nan=True)) and bool(torch.equal(rs[1], rp["oti"]))
    poff = rp["off"].cpu().numpy()
    sample = np.random.Generator(np.random.PCG64(7)).choice(len(pairs), min(200, len(pairs)), replace=False)
    med_ok = all(np.median(rp["mp"][poff[p]:poff[p + 1]].cpu().numpy()) == sc[p] for p in sample)
    mpi = rp["mpi"]
    so, po = _summary(ts, len(pairs)), _summary(tp, len(pairs))
    out = {"tracks": len(feats), "columns_min": int(lens.min()), "columns_max": int(lens.max()), "pairs": int(len(pairs)),
           "profile_rows": int(poff[-1]), "score": so, "profile": po,
           "ratio_profile_over_score": round(po["median_s"] / so["median_s"], 3),
           "score_equal": equal, "median_of_profile_is_score": bool(med_ok), "rows_without_index": int((mpi < 0).sum())}
    res[name] = out
    res["ok"] = res.get("ok", True) and equal and med_ok
    log("%s: %s" % (name, json.dumps(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-headline", dest="headline", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simple_profile", "bench_simple_profile.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_simple_profile.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "simple_profile", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats}
    if a.headline:  # bench.py's SiMPle corpus
        tracks, _ = synthetic.make_hard_corpus("covers80", frames=2000, seed=a.seed)
        feats = [_unit(np.ascontiguousarray(np.asarray(t, np.float64).T) + 1e-3) for t in tracks]
        n = len(feats)
        pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
        stage(a, "headline", feats, pairs, res)
    if a.short:
        rng = np.random.Generator(np.random.PCG64(a.seed))
        n = a.short_tracks
        feats = [_unit(np.abs(rng.standard_normal((12, int(L)))) + 1e-3) for L in rng.integers(350, 701, n)]
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "shortlist", feats, pairs, res)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
