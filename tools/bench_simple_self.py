"""The SiMPle self-join (acoss_simple_self_profile) against acoss_simple_profile on the pairs
(t, t) of the same tracks: the same cells, unmasked. One JSON, also written to
profiles/simple_self/bench_simple_self.json.

    python tools/bench_simple_self.py [--warmup 2] [--repeats 7] [--short-tracks 15000] [--excl E]
                                      [--no-headline] [--no-short] [--parent-lib path.so] [--out path.json]

Two shapes, in SiMPle columns:
  headline: the bench.py SiMPle corpus, 164 covers80-shaped tracks of exactly 2,000 unit columns
            (a self-profile of 1,991 rows per track).
  short:    the Da-TACOS-shaped case, --short-tracks tracks of 350..700 columns.
Per shape, in the same run, on the same build and alternating: --warmup untimed rounds, then
--repeats timed ones of `_lib.simple_profile_packed` on the pairs (t, t) (the baseline) and of
`_lib.simple_self_profile_packed` (excl = sslen // 2 unless --excl), each call closed by a device
synchronisation (a call's time includes allocating its ragged output). The JSON holds every time,
the medians, tracks/s of both, the ratio self / baseline and min..max as the spread. The bar: the
self-join takes at most 1.10 times the baseline call at either shape ("bar_met"). Checked on the
device: no index inside the band, the closure mp[mpi[i]] <= mp[i], and the motif and discord
against torch's own reductions of mp.

--parent-lib: a libacoss_hip.so built from the parent commit. acoss_simple_mp and
acoss_simple_profile are then also called through the C-ABI of both libraries, alternating in
this process on preallocated outputs, on every ordered pair of the first --nr-tracks tracks of
each shape ("vs_parent": medians, ratio this / parent, outputs equal bit for bit).
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

BAR = 1.10
SSLEN = 10


def log(msg, t0=[time.perf_counter()]):
    print("[simple_self %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times, n):
    med = float(np.median(times))
    return {"median_s": med, "min_s": float(min(times)), "max_s": float(max(times)),
            "per_s": round(n / med, 1), "all_s": [round(x, 6) for x in times]}


def _unit(F):
    return F / np.linalg.norm(F, axis=0, keepdims=True)


def _checks(r, excl, torch):
    """The self-join's own invariants, on the device."""
    off, mp, mpi = r["off"], r["mp"], r["mpi"].long()
    rows = off[1:] - off[:-1]
    ent = torch.repeat_interleave(torch.arange(len(rows), device=mp.device), rows)
    i = torch.arange(len(mp), device=mp.device) - off[ent]
    has = mpi >= 0
    band_ok = bool(((mpi - i).abs()[has] > excl).all())
    closure = bool((mp[(off[ent] + mpi)[has]] <= mp[has]).all())
    motif, discord = r["motif"].long(), r["discord"].long()
    ok = True
    for e in range(0, len(rows), max(1, len(rows) // 64)):  # a sample of entries
        m = mp[off[e]:off[e + 1]]
        if len(m) == 0 or bool(torch.isnan(m).all()):
            ok = ok and motif[e].tolist() == [-1, -1] and int(discord[e]) == -1
            continue
        v = torch.nan_to_num(m, nan=float("inf"))
        w = torch.nan_to_num(m, nan=float("-inf"))
        i0 = int((v == v.min()).nonzero()[0])
        i1 = int((w == w.max()).nonzero()[0])
        ok = ok and motif[e].tolist() == [i0, int(mpi[off[e] + i0])] and int(discord[e]) == i1
    return {"no_index_in_band": band_ok, "closure": closure, "motif_discord": bool(ok),
            "rows_without_index": int((~has).sum())}


def _raw(lib, d_flat, d_off, d_len, n_tracks, max_len, d_pairs, torch):
    """acoss_simple_mp and acoss_simple_profile of one library through the C-ABI, outputs preallocated."""
    from acoss import _lib
    for name in ("acoss_simple_mp", "acoss_simple_profile"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int
    P = d_pairs.shape[0]
    lens = d_len.cpu().numpy().astype(np.int64)
    poff = _lib.simple_profile_offsets(lens, d_pairs.cpu().numpy(), SSLEN)
    d_poff = torch.as_tensor(poff).cuda()
    total = int(poff[-1])
    score = torch.empty(P, dtype=torch.float64, device="cuda")
    score2 = torch.empty(P, dtype=torch.float64, device="cuda")
    oti = torch.empty(P, dtype=torch.int32, device="cuda")
    mp = torch.empty(total, dtype=torch.float64, device="cuda")
    mpi = torch.empty(total, dtype=torch.int32, device="cuda")
    keep = (d_poff,)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call_mp():
        rc = lib.acoss_simple_mp(d_flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n_tracks, max_len,
                                 d_pairs.data_ptr(), P, SSLEN, 1, score.data_ptr(), oti.data_ptr(), stream())
        assert rc == 0, rc
        return score

    def call_profile():
        rc = lib.acoss_simple_profile(d_flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n_tracks, max_len,
                                      d_pairs.data_ptr(), P, SSLEN, 1, d_poff.data_ptr(), total, mp.data_ptr(),
                                      mpi.data_ptr(), score2.data_ptr(), oti.data_ptr(), stream())
        assert rc == 0, rc
        return mp, mpi, score2

    return call_mp, call_profile, keep


def vs_parent(a, parent, feats, torch):
    """acoss_simple_mp / acoss_simple_profile of this build against the parent's, alternating."""
    from acoss import _lib
    feats = feats[:a.nr_tracks]
    n = len(feats)
    lens = np.array([f.shape[1] for f in feats], np.int32)
    off = np.concatenate([[0], np.cumsum(12 * lens.astype(np.int64))[:-1]])
    d_flat = torch.as_tensor(np.concatenate([f.ravel() for f in feats])).cuda()
    d_off, d_len = torch.as_tensor(off).cuda(), torch.as_tensor(lens).cuda()
    pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    d_pairs = torch.as_tensor(pairs).cuda()
    calls = {"this": _raw(_lib.load_library(), d_flat, d_off, d_len, n, int(lens.max()), d_pairs, torch),
             "parent": _raw(parent, d_flat, d_off, d_len, n, int(lens.max()), d_pairs, torch)}
    times = {(w, k): [] for w in calls for k in ("mp", "profile")}
    outs = {}
    for it in range(a.warmup + a.repeats):
        for k, idx in (("mp", 0), ("profile", 1)):
            for w in ("parent", "this"):
                t, o = _timed(calls[w][idx], torch)
                outs[w, k] = [x.clone() for x in (o if isinstance(o, tuple) else (o,))]
                if it >= a.warmup:
                    times[w, k].append(t)
    res = {"tracks": n, "pairs": int(len(pairs))}
    for k in ("mp", "profile"):
        p, t = _summary(times["parent", k], len(pairs)), _summary(times["this", k], len(pairs))
        same = all(bool(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                    y.view(torch.int64) if y.dtype == torch.float64 else y))
                   for x, y in zip(outs["parent", k], outs["this", k]))
        res[k] = {"parent": p, "this": t, "ratio_this_over_parent": round(t["median_s"] / p["median_s"], 4),
                  "outputs_bit_equal": same}
    return res


def stage(a, name, feats, res, parent):
    import torch
    from acoss import _lib
    lens = np.array([f.shape[1] for f in feats], np.int32)
    off = np.concatenate([[0], np.cumsum(12 * lens.astype(np.int64))[:-1]])
    d_flat = torch.as_tensor(np.concatenate([f.ravel() for f in feats])).cuda()
    tracks = np.arange(len(feats), dtype=np.int32)
    pairs = np.stack([tracks, tracks], 1)
    excl = SSLEN // 2 if a.excl is None else a.excl

    def baseline():
        return _lib.simple_profile_packed(d_flat, off, lens, pairs, SSLEN, apply_oti=False)

    def selfjoin():
        return _lib.simple_self_profile_packed(d_flat, off, lens, tracks, SSLEN, excl)

    tb, ts = [], []
    for it in range(a.warmup + a.repeats):
        b_, rb = _timed(baseline, torch)
        s_, rs = _timed(selfjoin, torch)
        if it >= a.warmup:
            tb.append(b_)
            ts.append(s_)
    bo, so = _summary(tb, len(feats)), _summary(ts, len(feats))
    ratio = so["median_s"] / bo["median_s"]
    out = {"tracks": len(feats), "columns_min": int(lens.min()), "columns_max": int(lens.max()), "excl": excl,
           "profile_rows": int(rs["off"][-1]), "baseline_profile_tt": bo, "self": so,
           "ratio_self_over_baseline": round(ratio, 4), "bar": BAR, "bar_met": bool(ratio <= BAR),
           "baseline_all_zero": bool((rb["mp"] == 0).all()), "checks": _checks(rs, excl, torch)}
    if parent is not None:
        out["vs_parent"] = vs_parent(a, parent, feats, torch)
    res[name] = out
    c = out["checks"]
    res["ok"] = res.get("ok", True) and c["no_index_in_band"] and c["closure"] and c["motif_discord"]
    log("%s: %s" % (name, json.dumps(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--short-tracks", type=int, default=15000)
    ap.add_argument("--excl", type=int, default=None)
    ap.add_argument("--nr-tracks", type=int, default=60, help="tracks of each shape in the --parent-lib comparison")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-headline", dest="headline", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simple_self", "bench_simple_self.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_simple_self.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import _lib, synthetic
    _lib.load_library()
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    res = {"bench": "simple_self", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "sslen": SSLEN, "symmetric_walk_tried": False}
    if a.headline:  # bench.py's SiMPle corpus
        tracks, _ = synthetic.make_hard_corpus("covers80", frames=2000, seed=a.seed)
        feats = [_unit(np.ascontiguousarray(np.asarray(t, np.float64).T) + 1e-3) for t in tracks]
        stage(a, "headline", feats, res, parent)
    if a.short:
        rng = np.random.Generator(np.random.PCG64(a.seed))
        feats = [_unit(np.abs(rng.standard_normal((12, int(L)))) + 1e-3) for L in rng.integers(350, 701, a.short_tracks)]
        stage(a, "short", feats, res, parent)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
