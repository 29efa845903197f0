"""Best of n over the ranked OTI (acoss_crp_align3, crp.hip k_oti_rank / k_oti_fold) beside n scoring
calls of the parent commit's library, the entries that existed before against that library, and what
the extra transpositions do to the accuracy. One JSON, also written to
profiles/multi_oti/bench_multi_oti.json. The protocol is tools/bench_otib.py's.

    python tools/bench_multi_oti.py --parent-lib tools/abl/libabl_parent.so [--warmup 2] [--repeats 7]
                                    [--no-headline] [--no-short] [--out path.json]

--parent-lib: a libacoss_hip.so built from the parent commit (tools/abbuild.sh in a checkout of it).

Two shapes:
  headline:  the bench.py corpus, 164 covers80-shaped hard tracks of exactly 2,000 frames, all 13,366
             unordered pairs.
  shortlist: --short-tracks tracks of 350..700 frames, each against --short-k others drawn at random
             (200,000 pairs at the defaults).
--first parent|this: which of the two libraries is loaded and called first, and so allocates its
workspace first; a difference that changes sign with it belongs to the placement, not to the code.

Per shape, both libraries in this process, every call closed by a device synchronisation, --warmup
untimed rounds then --repeats timed ones, the order of the calls swapping every round; the JSON holds
every time, the medians and min..max as the run-to-run spread.
  (a) unchanged: acoss_crp_align (Qmax; Qmax + dmax) and acoss_crp_align2 (percentile; OTI-binary) of
      the parent and of this tree: the same output bits, and the difference of the medians within the
      larger of the two spreads.
  (b) the bar: acoss_crp_align3 at n_oti = 2 and 3, Qmax only and Qmax + dmax, against n x the parent's
      acoss_crp_align2 on the same pairs. A round repeats everything but the per-track preparation, so
      the ratio is expected at or just under n. Bar: median <= n x the parent's median + the spread
      (the larger of this call's max - min and n x the parent's).
  (c) accuracy (headline shape only), recorded and not asserted: MAP, MR1 of Qmax / sqrt(n_j) at
      n_oti = 1, 2, 3 and how many pairs each pick wins.
The exit code is 1 when (a) or (b) is missed.
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

PARENT_ENTRIES = ("acoss_crp_align", "acoss_crp_align2")


def log(msg, t0=[time.perf_counter()]):
    print("[multi_oti %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)),
            "all_s": [round(x, 6) for x in times]}


def _range(s):
    return s["max_s"] - s["min_s"]


def _bind(path):
    """The parent commit's library: it lacks the entries ending in 3, so only what is timed is bound."""
    from acoss import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in PARENT_ENTRIES:
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def _alternate(a, torch, calls):
    """calls: {key: fn}; --warmup + --repeats rounds, the order swapping every round. {key: summary}."""
    times = {k: [] for k in calls}
    for it in range(a.warmup + a.repeats):
        for k in (list(calls) if it % 2 == 0 else list(calls)[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            calls[k]()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append(time.perf_counter() - t)
    return {k: _summary(v) for k, v in times.items()}


def stage(a, name, tracks, labels, pairs, res):
    import torch
    from acoss import _lib, evaluation, synthetic
    feats, off, lens = synthetic.pack(tracks)
    d = {"feats": torch.as_tensor(feats).cuda(), "off": torch.as_tensor(off).cuda(),
         "len": torch.as_tensor(lens).cuda()}
    d_pairs = torch.as_tensor(pairs).cuda().to(torch.int32).contiguous()
    max_len, n = int(lens.max()), int(len(pairs))
    # the library bound and called first gets its workspace first: --first swaps the two, because a
    # difference that follows the order is the placement's and not the code's
    if a.first == "parent":
        libs = {"parent": _bind(a.parent_lib), "this": _lib.load_library()}
    else:
        libs = {"this": _lib.load_library(), "parent": _bind(a.parent_lib)}
    base = _lib.crp_params()
    wide = {"percentile": _lib.CrpParams2(base, 0, 1), "otib": _lib.crp_params(binarize="oti")}
    lead_of = lambda P: (_lib._ptr(d["feats"]), _lib._ptr(d["off"]), _lib._ptr(d["len"]),  # noqa: E731
                         int(d["len"].shape[0]), max_len, _lib._ptr(d_pairs), n, ctypes.byref(P))
    f32 = lambda: torch.empty(n, dtype=torch.float32, device="cuda")  # noqa: E731
    i32 = lambda: torch.empty(n, dtype=torch.int32, device="cuda")  # noqa: E731
    out = {"tracks": len(tracks), "frames_min": int(lens.min()), "frames_max": max_len, "pairs": n}
    ok = True

    # (a) the entries that existed before
    cases = {"align_qmax": ("acoss_crp_align", base, False), "align_qmax_dmax": ("acoss_crp_align", base, True),
             "align2_percentile_qmax": ("acoss_crp_align2", wide["percentile"], False),
             "align2_percentile_qmax_dmax": ("acoss_crp_align2", wide["percentile"], True),
             "align2_otib_qmax": ("acoss_crp_align2", wide["otib"], False)}
    if not a.otib:
        cases.pop("align2_otib_qmax")
    out["unchanged"] = {}
    for case, (entry, P, with_d) in cases.items():
        outs, calls = {}, {}
        for k, lib in libs.items():
            o = outs[k] = (f32(), f32() if with_d else None, i32())

            def call(lib=lib, entry=entry, P=P, o=o):
                rc = getattr(lib, entry)(*lead_of(P), _lib._ptr(o[0]), _lib._ptr(o[1]), _lib._ptr(o[2]), _lib._stream())
                assert rc == 0, (entry, rc)
            calls[k] = call
        sm = _alternate(a, torch, calls)
        spread = max(_range(v) for v in sm.values())
        diff = sm["this"]["median_s"] - sm["parent"]["median_s"]
        same = all(bool(torch.equal(x, y)) for x, y in zip(outs["parent"], outs["this"]) if x is not None)
        out["unchanged"][case] = {"parent": sm["parent"], "this": sm["this"], "spread_s": round(spread, 6),
                                  "median_difference_s": round(diff, 6), "within_spread": bool(diff <= spread),
                                  "same_bits": same}
        ok = ok and same and diff <= spread
        log("%s %s: %s" % (name, case, json.dumps({k: v for k, v in out["unchanged"][case].items()
                                                   if k not in ("parent", "this")})))

    # (b) best of n against n x the parent's scoring call
    out["best_of_n"] = {}
    for with_d in (False, True):
        what = "qmax_dmax" if with_d else "qmax"
        po = (f32(), f32() if with_d else None)

        def parent_call(po=po):
            rc = libs["parent"].acoss_crp_align2(*lead_of(wide["percentile"]), _lib._ptr(po[0]), _lib._ptr(po[1]), None,
                                                 _lib._stream())
            assert rc == 0, rc
        calls = {"parent_align2": parent_call}
        for n_oti in (2, 3):
            P3 = _lib.crp_params3(base, n_oti=n_oti)
            o = (f32(), f32() if with_d else None, i32(), i32() if with_d else None, i32(), i32() if with_d else None)

            def call(P3=P3, o=o):
                rc = libs["this"].acoss_crp_align3(*lead_of(P3), *(_lib._ptr(t) for t in o), _lib._stream())
                assert rc == 0, rc
            calls["this_align3_n%d" % n_oti] = call
        if a.first == "this":
            calls = dict(list(calls.items())[::-1])
        sm = _alternate(a, torch, calls)
        row = {"parent_align2": sm["parent_align2"]}
        for n_oti in (2, 3):
            s = sm["this_align3_n%d" % n_oti]
            spread = max(_range(s), n_oti * _range(sm["parent_align2"]))
            bound = n_oti * sm["parent_align2"]["median_s"] + spread
            row["n%d" % n_oti] = {"this_align3": s,
                                  "n_times_parent_s": round(n_oti * sm["parent_align2"]["median_s"], 6),
                                  "spread_s": round(spread, 6),
                                  "ratio_over_parent": round(s["median_s"] / sm["parent_align2"]["median_s"], 4),
                                  "within_bar": bool(s["median_s"] <= bound)}
            ok = ok and row["n%d" % n_oti]["within_bar"]
        out["best_of_n"][what] = row
        brief = {k: {kk: vv for kk, vv in v.items() if kk != "this_align3"} for k, v in row.items()
                 if k != "parent_align2"}
        log("%s best of n, %s: %s" % (name, what, json.dumps(brief)))

    # (c) accuracy: all unordered pairs of the corpus, Qmax / sqrt(n_j), symmetric
    if labels is not None:
        out["accuracy"] = {}
        nt = len(tracks)
        for n_oti in (1, 2, 3):
            r = _lib.crp_align(d["feats"], d["off"], d["len"], max_len, d_pairs, _lib.crp_params3(base, n_oti=n_oti),
                               qmax=True)
            D = np.zeros((nt, nt), np.float32)
            D[pairs[:, 0], pairs[:, 1]] = r["qmax"].cpu().numpy()
            D = D + D.T
            D = (D / np.sqrt(lens.astype(np.float64))[None, :]).astype(np.float32)
            MR, MRR, MDR, MAP, tops = evaluation.eval_statistics(D, labels)
            won = np.bincount(r["pick_q"].cpu().numpy(), minlength=n_oti)
            same = labels[pairs[:, 0]] == labels[pairs[:, 1]]
            won_cover = np.bincount(r["pick_q"].cpu().numpy()[same], minlength=n_oti)
            out["accuracy"]["n_oti_%d" % n_oti] = {"MAP": float(MAP), "MR1": float(MR), "MRR": float(MRR),
                                                   "pairs_won_by_pick": [int(v) for v in won],
                                                   "cover_pairs_won_by_pick": [int(v) for v in won_cover]}
        log("%s accuracy: %s" % (name, json.dumps(out["accuracy"])))
    res[name] = out
    res["ok"] = res.get("ok", True) and ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-headline", dest="headline", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--no-otib", dest="otib", action="store_false",
                    help="leave acoss_crp_align2 under ACOSS_BIN_OTI out of (a)")
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--first", choices=("parent", "this"), default="parent",
                    help="which library is loaded and called first (its workspace is allocated first)")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_oti", "bench_multi_oti.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_multi_oti.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    from acoss import synthetic
    res = {"bench": "multi_oti", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "first": a.first}
    if a.headline:
        tracks, labels = synthetic.make_hard_corpus("covers80", frames=2000, seed=a.seed)
        n = len(tracks)
        pairs = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
        stage(a, "headline", tracks, np.asarray(labels), pairs, res)
    if a.short:
        rng = np.random.Generator(np.random.PCG64(a.seed))
        n = a.short_tracks
        tracks = [synthetic.render(rng, synthetic.base_sequence(rng, int(L))) for L in rng.integers(350, 701, n)]
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "shortlist", tracks, None, pairs, res)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
