"""The OTI-binary CRP (acoss_crp_align2 under ACOSS_BIN_OTI, crp_otib.hip) beside the percentile CRP on
the same pair lists, and the entries that existed before it against the parent commit's library. One
JSON, also written to profiles/otib/bench_otib.json. The protocol is tools/bench_rqa.py's.

    python tools/bench_otib.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                               [--no-headline] [--no-short] [--parent-lib libacoss_hip.so] [--out path.json]

Two shapes:
  headline:  the bench.py corpus, 164 covers80-shaped hard tracks of exactly 2,000 frames, all 13,366
             unordered pairs.
  shortlist: --short-tracks tracks of 350..700 frames, each against --short-k others drawn at random
             (200,000 pairs at the defaults).
Per shape, in the same run and alternating: --warmup untimed rounds, then --repeats timed ones of
`_lib.crp_align(qmax)` with the percentile params, with binarize='oti' at rank 1 and at rank 2, each
call closed by a device synchronisation; the JSON holds every time, the medians, min..max as the
run-to-run spread and the ratios. Then one call of each with the library's phase events on (the
"crp_mask" phase is the OTI-binary kernel; the percentile call at m = 9 runs the split path, whose
phases are its own), and the density of ones of the masks (RR of acoss_crp_rqa / acoss_crp_rqa2 on up
to 20,000 of the pairs). On the headline corpus MAP, MR1 of Qmax / sqrt(n_j) for the three modes:
recorded, not asserted.

The bar (--parent-lib, a libacoss_hip.so built from the parent commit; shortlist shape): at m = 8 the
generic k_crp_panel<0> makes one Gram and one window per cell and the OTI-binary kernel twelve of
each, so this tree's "crp_mask" phase under binarize='oti' must not exceed 12 x the parent's
"crp_mask" phase of the percentile call, m = 8, same pairs. The two libraries run alternately in
this process, the order swapping every round; the ratio of the medians and both spreads go into the
JSON, and "within_bar" decides the exit code. The seven entries that existed before (acoss_crp_align,
_locate, _locate_dmax, _path, _path_dmax, _rqa on the first --old-pairs pairs of that shape,
acoss_crp_pair on its first pair) are timed the same way, parent against this tree: each must stay
within the larger of the two spreads and give the same output bits.
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

OLD_ENTRIES = ("acoss_crp_align", "acoss_crp_locate", "acoss_crp_locate_dmax", "acoss_crp_path",
               "acoss_crp_path_dmax", "acoss_crp_rqa", "acoss_crp_pair")


def log(msg, t0=[time.perf_counter()]):
    print("[otib %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)),
            "all_s": [round(x, 6) for x in times]}


def _phases(lib, fn, torch, names):
    """{phase name: ms} of one call of fn with the phase events of `lib` on."""
    lib.acoss_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    ms, cnt = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)()
    n = lib.acoss_profile_read(ms, cnt, 64)
    lib.acoss_profile_enable(0)
    out = {}
    for i in range(n):
        name = lib.acoss_profile_phase_name(i).decode()
        if name in names and cnt[i]:
            out[name] = round(ms[i], 4)
    return out


def _bind(path):
    """The parent commit's library: it lacks the entries ending in 2, so only what it has is bound."""
    from acoss import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in OLD_ENTRIES + ("acoss_profile_enable", "acoss_profile_read"):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    lib.acoss_profile_phase_name.restype = ctypes.c_char_p
    lib.acoss_profile_phase_name.argtypes = [ctypes.c_int]
    return lib


def _alternate(a, torch, calls):
    """calls: {key: fn}; --warmup + --repeats rounds, the order swapping every round. {key: summary}."""
    times = {k: [] for k in calls}
    for it in range(a.warmup + a.repeats):
        for k in (list(calls) if it % 2 == 0 else list(calls)[::-1]):
            s, _ = _timed(calls[k], torch)
            if it >= a.warmup:
                times[k].append(s)
    return {k: _summary(v) for k, v in times.items()}


def mask_bar(a, torch, lead_of, n_pairs):
    """The bar: "mask" phase of this tree's OTI-binary call against 12 x the parent's percentile call, m = 8."""
    from acoss import _lib
    this, parent = _lib.load_library(), _bind(a.parent_lib)
    P8 = _lib.crp_params(m=8)
    O8 = _lib.crp_params(m=8, binarize="oti")
    q = {k: torch.empty(n_pairs, dtype=torch.float32, device="cuda") for k in ("parent", "this")}

    def parent_call():
        rc = parent.acoss_crp_align(*lead_of(P8), _lib._ptr(q["parent"]), None, None, _lib._stream())
        assert rc == 0, rc

    def this_call():
        rc = this.acoss_crp_align2(*lead_of(O8), _lib._ptr(q["this"]), None, None, _lib._stream())
        assert rc == 0, rc

    ms = {"parent_percentile_m8": [], "this_otib_m8": []}
    for it in range(a.warmup + a.repeats):
        order = [("parent_percentile_m8", parent, parent_call), ("this_otib_m8", this, this_call)]
        for k, lib, fn in (order if it % 2 == 0 else order[::-1]):
            ph = _phases(lib, fn, torch, ("crp_mask",))
            if it >= a.warmup:
                ms[k].append(ph["crp_mask"])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ratio = med["this_otib_m8"] / med["parent_percentile_m8"]
    return {"mask_ms": {k: {"median": med[k], "min": min(v), "max": max(v), "all": v} for k, v in ms.items()},
            "ratio_otib_over_percentile": round(ratio, 3), "bound": 12.0, "within_bar": bool(ratio <= 12.0)}


def old_entries(a, torch, d, max_len, pairs, n_slice):
    """The seven entries that existed before, parent library against this tree's, on pairs[:n_slice]."""
    from acoss import _lib
    libs = {"parent": _bind(a.parent_lib), "this": _lib.load_library()}
    P = _lib.crp_params()
    n = int(min(n_slice, len(pairs)))
    sub = pairs[:n].contiguous()
    L = _lib.stacked_len(max_len)
    cap = max(1, _lib.dmax_path_bound(L, L), L)
    lead = (_lib._ptr(d["feats"]), _lib._ptr(d["off"]), _lib._ptr(d["len"]), int(d["len"].shape[0]), max_len,
            _lib._ptr(sub), n, ctypes.byref(P))
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")  # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")  # noqa: E731
    n_path = int(min(n, max(1, (1 << 28) // (8 * cap))))
    a0, b0 = (int(x) for x in pairs[0].tolist())
    lens = d["len"].cpu().numpy()
    offs = d["off"].cpu().numpy()
    X = d["feats"][offs[a0]:offs[a0] + lens[a0]].contiguous()
    Y = d["feats"][offs[b0]:offs[b0] + lens[b0]].contiguous()
    Mp, Np = _lib.stacked_len(int(lens[a0])), _lib.stacked_len(int(lens[b0]))
    res = {}
    for entry in OLD_ENTRIES:
        outs = {}
        calls = {}
        for k, lib in libs.items():
            if entry == "acoss_crp_align":
                o = outs[k] = (f32(n), f32(n), i32(n))
                args = lead + tuple(_lib._ptr(t) for t in o)
            elif entry.startswith("acoss_crp_locate"):
                o = outs[k] = (f32(n), i32(n, 4), i32(n))
                args = lead + tuple(_lib._ptr(t) for t in o)
            elif entry.startswith("acoss_crp_path"):
                o = outs[k] = (f32(n_path), i32(n_path, 4), i32(n_path), i32(n_path), i32(n_path, cap, 2))
                args = lead[:6] + (n_path, lead[7], _lib._ptr(o[0]), _lib._ptr(o[1]), _lib._ptr(o[2]), cap,
                                   _lib._ptr(o[3]), _lib._ptr(o[4]))
            elif entry == "acoss_crp_rqa":
                o = outs[k] = (torch.empty((n, 4), dtype=torch.int64, device="cuda"), i32(n),
                               torch.empty((n, 4), dtype=torch.float64, device="cuda"), f32(n), i32(n))
                args = lead + (2,) + tuple(_lib._ptr(t) for t in o) + (0, None)
            else:
                o = outs[k] = (f32(Mp, Np), f32(Mp), f32(Np), torch.empty((Mp, Np), dtype=torch.uint8, device="cuda"),
                               i32(1))
                args = (_lib._ptr(X), int(lens[a0]), _lib._ptr(Y), int(lens[b0]), ctypes.byref(P)) + tuple(
                    _lib._ptr(t) for t in o)

            def call(lib=lib, args=args, entry=entry):
                rc = getattr(lib, entry)(*args, _lib._stream())
                assert rc == 0, (entry, rc)
            calls[k] = call
        sm = _alternate(a, torch, calls)
        spread = max(v["max_s"] - v["min_s"] for v in sm.values())
        diff = sm["this"]["median_s"] - sm["parent"]["median_s"]
        same = all(bool(torch.equal(x, y)) for x, y in zip(outs["parent"], outs["this"]))
        res[entry] = {"parent": sm["parent"], "this": sm["this"], "spread_s": round(spread, 6),
                      "median_difference_s": round(diff, 6), "within_spread": bool(diff <= spread),
                      "same_bits": same}
        log("%s: %s" % (entry, json.dumps({k: v for k, v in res[entry].items() if k not in ("parent", "this")})))
    return res


def stage(a, name, tracks, labels, pairs, res, bar):
    import torch
    from acoss import _lib, evaluation, synthetic
    feats, off, lens = synthetic.pack(tracks)
    d = {"feats": torch.as_tensor(feats).cuda(), "off": torch.as_tensor(off).cuda(),
         "len": torch.as_tensor(lens).cuda()}
    d_pairs = torch.as_tensor(pairs).cuda().to(torch.int32).contiguous()
    max_len = int(lens.max())
    modes = {"percentile": _lib.crp_params(), "otib": _lib.crp_params(binarize="oti"),
             "otib2": _lib.crp_params(binarize="oti", oti_rank=2)}
    calls = {k: (lambda P=P: _lib.crp_align(d["feats"], d["off"], d["len"], max_len, d_pairs, P, qmax=True))
             for k, P in modes.items()}
    times, got = {k: [] for k in calls}, {}
    for it in range(a.warmup + a.repeats):
        for k in (list(calls) if it % 2 == 0 else list(calls)[::-1]):
            s, got[k] = _timed(calls[k], torch)
            if it >= a.warmup:
                times[k].append(s)
    sm = {k: _summary(v) for k, v in times.items()}
    out = {"tracks": len(tracks), "frames_min": int(lens.min()), "frames_max": max_len, "pairs": int(len(pairs))}
    out.update({"align_" + k: v for k, v in sm.items()})
    for k in ("otib", "otib2"):
        out["ratio_%s_over_percentile" % k] = round(sm[k]["median_s"] / sm["percentile"]["median_s"], 3)
    names = ("prep", "oti", "select_rows", "select_cols", "crp_mask", "sweep", "dp_qmax")
    out["phases_ms"] = {k: _phases(_lib.load_library(), calls[k], torch, names) for k in calls}
    # density of ones: n_rec / (M' N') of acoss_crp_rqa(2), line walk only, on a slice of the pairs
    ns = int(min(len(pairs), 20000))
    dens = {}
    for k, P in modes.items():
        r = _lib.crp_rqa(d["feats"], d["off"], d["len"], max_len, d_pairs[:ns], P, smax=False)
        rr = r["stats"][:, 0].cpu().numpy()
        dens[k] = {"mean": float(rr.mean()), "min": float(rr.min()), "max": float(rr.max()), "pairs": ns}
    out["density"] = dens
    if labels is not None:  # all unordered pairs of the corpus: Qmax / sqrt(n_j), symmetric
        n = len(tracks)
        out["map"] = {}
        for k in calls:
            D = np.zeros((n, n), np.float32)
            D[pairs[:, 0], pairs[:, 1]] = got[k]["qmax"].cpu().numpy()
            D = D + D.T
            D = (D / np.sqrt(lens.astype(np.float64))[None, :]).astype(np.float32)
            MR, MRR, MDR, MAP, tops = evaluation.eval_statistics(D, labels)
            out["map"][k] = {"MAP": float(MAP), "MR1": float(MR), "MRR": float(MRR)}
    ok = True
    if a.parent_lib:
        lead_of = lambda P: (_lib._ptr(d["feats"]), _lib._ptr(d["off"]), _lib._ptr(d["len"]),  # noqa: E731
                             int(d["len"].shape[0]), max_len, _lib._ptr(d_pairs), int(len(pairs)), ctypes.byref(P))
        if bar:
            out["bar_m8"] = mask_bar(a, torch, lead_of, int(len(pairs)))
            ok = ok and out["bar_m8"]["within_bar"]
            log("bar: %s" % json.dumps(out["bar_m8"]))
            out["old_entries"] = old_entries(a, torch, d, max_len, d_pairs, a.old_pairs)
            ok = ok and all(v["same_bits"] and v["within_spread"] for v in out["old_entries"].values())
    res[name] = out
    res["ok"] = res.get("ok", True) and ok
    log("%s: %s" % (name, json.dumps({k: v for k, v in out.items() if k != "old_entries"})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--old-pairs", type=int, default=20000, help="pairs of the old entries' parent-against-this runs")
    ap.add_argument("--no-headline", dest="headline", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "otib", "bench_otib.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_otib.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "otib", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "parent_lib": bool(a.parent_lib)}
    if a.headline:
        tracks, labels = synthetic.make_hard_corpus("covers80", frames=2000, seed=a.seed)
        n = len(tracks)
        pairs = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
        stage(a, "headline", tracks, labels, pairs, res, bar=False)
    if a.short:
        rng = np.random.Generator(np.random.PCG64(a.seed))
        n = a.short_tracks
        tracks = [synthetic.render(rng, synthetic.base_sequence(rng, int(L))) for L in rng.integers(350, 701, n)]
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "shortlist", tracks, None, pairs, res, bar=True)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
