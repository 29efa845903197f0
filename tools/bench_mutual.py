"""The cost and the effect of EarlyFusion's mutual nearest-neighbour binarisation
(acoss_earlyfusion2 and its kin with ACOSS_EF_BIN_MUTUAL) against the row rule on the same pair lists.
One JSON, also written to profiles/mutual/bench_mutual.json.

    python tools/bench_mutual.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                                 [--no-blocks446] [--no-short] [--no-map] [--snf-pairs446 16]
                                 [--snf-pairs-short 20000] [--parent-lib libacoss_hip.so] [--out path.json]

The two EarlyFusion shapes the other tools use (bench_sw_path.py): blocks446, 80 tracks of 446 beat
blocks, all 3,160 unordered pairs; short, --short-tracks tracks of 14..47 blocks, each against
--short-k others (200,000 pairs). Per shape, all in one process, --warmup untimed rounds then
--repeats timed ones, the calls alternating and their order swapping every round, each call closed
by a device synchronisation; a spread is min..max.

  bar        the "binarize" phase (acoss_profile_read, HIP events round its launches, one stream) of
             acoss_earlyfusion2(mutual) over the "binarize" phase of acoss_earlyfusion of the
             reference library: --parent-lib, a libacoss_hip.so built from the parent commit, or,
             without it, this tree's own acoss_earlyfusion (reference = "this"). The bar is 2.5.
  calls      whole-call medians of score / locate / path / snf with mutual over the same call
             without (this tree's wrappers; early SNF on the first --snf-pairs* pairs of the list).
  unchanged  with --parent-lib: acoss_earlyfusion, _locate, _path and _snf of both libraries,
             alternately on the same buffers: the same output bits, and whether each median lies
             within the larger of the two spreads of its parent's. Where the parent's library exports
             the entries ending in 2, also those four with ACOSS_EF_BIN_MUTUAL, and the "binarize"
             phase of acoss_earlyfusion2 in both modes, under the same rule.
  density    ones in the four masks of a sample of pairs, row rule against mutual
             (acoss_binarize_mutual on the matrices EarlyFusion.pair_matrices forms).
  map        MAP and MR1 of the five scores on bench_early_snf.py's synthetic covers80-shaped
             corpus, row rule against mutual. Recorded, not asserted.
The run fails if the row mode of the new entries differs from the twins, or the parent's outputs
differ from this tree's.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

from bench_sw_path import _timed, make_bank  # noqa: E402

KAPPA, K, MU, NITERS, BAR = 0.1, 10, 0.5, 5, 2.5


def log(msg, t0=[time.perf_counter()]):
    print("[mutual %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _summary(v, unit="s"):
    return {"median_" + unit: float(np.median(v)), "min_" + unit: float(min(v)), "max_" + unit: float(max(v)),
            "all_" + unit: [round(x, 6) for x in v]}


def _rounds(a, names, measure):
    """{name: [measure(name) of each timed round]}: the calls alternating, the order swapping every round."""
    got = {k: [] for k in names}
    for it in range(a.warmup + a.repeats):
        for k in (names if it % 2 == 0 else names[::-1]):
            v = measure(k)
            if it >= a.warmup:
                got[k].append(v)
    return got


def _alternate(a, fns):
    """{name: [seconds]} and the last outputs of the alternating calls."""
    import torch
    got = {}

    def measure(k):
        s, got[k] = _timed(fns[k], torch)
        return s
    return _rounds(a, list(fns), measure), got


TWINS = ("acoss_earlyfusion", "acoss_earlyfusion_locate", "acoss_earlyfusion_path", "acoss_earlyfusion_snf")


def _bind(path):
    """The parent commit's library: the four twins, and the entries ending in 2 where it exports them."""
    from acoss import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.has2 = all(hasattr(lib, name + "2") for name in TWINS)
    for name in TWINS + tuple(n + "2" for n in TWINS if lib.has2) + ("acoss_profile_enable", "acoss_profile_read"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int
    lib.acoss_profile_phase_name.restype = ctypes.c_char_p
    lib.acoss_profile_phase_name.argtypes = [ctypes.c_int]
    return lib


def _phase_ms(lib, call, phase="binarize"):
    """Milliseconds of one phase of one call, with the library's phase events on."""
    import torch
    lib.acoss_profile_enable(1)
    call()
    torch.cuda.synchronize()
    ms, cnt = (ctypes.c_double * 32)(), (ctypes.c_int64 * 32)()
    k = lib.acoss_profile_read(ms, cnt, 32)
    lib.acoss_profile_enable(0)
    got = {lib.acoss_profile_phase_name(i).decode(): ms[i] for i in range(k) if cnt[i] > 0}
    return got[phase]


def _lead(bank, d_pairs):
    from acoss import _lib
    return (_lib._ptr(bank["mfccs"]), _lib._ptr(bank["ssms"]), _lib._ptr(bank["chromas"]), _lib._ptr(bank["chroma_med"]),
            _lib._ptr(bank["off"]), _lib._ptr(bank["nb"]), int(bank["nb"].shape[0]), int(bank["max_blocks"]), 1000,
            1225, 480, _lib._ptr(d_pairs), int(d_pairs.shape[0]), KAPPA, K, MU)


def bar_stage(a, bank, d_pairs, parent, out):
    """The binarize phase of acoss_earlyfusion2(mutual) over that of the reference's acoss_earlyfusion."""
    import torch
    from acoss import _lib
    this = _lib.load_library()
    ref = parent or this
    P = int(d_pairs.shape[0])
    sc = {k: torch.empty((P, 4), dtype=torch.float64, device="cuda") for k in ("ref", "mutual", "rows2")}
    lead = _lead(bank, d_pairs)

    def chk(rc):
        if rc:
            raise RuntimeError("library call returned %d: %s" % (rc, this.acoss_last_error()))

    calls = {"ref": (ref, lambda: chk(ref.acoss_earlyfusion(*lead, _lib._ptr(sc["ref"]), _lib._stream()))),
             "mutual": (this, lambda: chk(this.acoss_earlyfusion2(*lead, 1, _lib._ptr(sc["mutual"]), _lib._stream()))),
             "rows2": (this, lambda: chk(this.acoss_earlyfusion2(*lead, 0, _lib._ptr(sc["rows2"]), _lib._stream())))}
    ms = _rounds(a, list(calls), lambda k: _phase_ms(*calls[k]))
    sm = {k: _summary(v, "ms") for k, v in ms.items()}
    ratio = sm["mutual"]["median_ms"] / sm["ref"]["median_ms"]
    same = bool(torch.equal(sc["ref"], sc["rows2"]))
    out["bar"] = {"reference": "parent" if parent else "this", "binarize_ref": sm["ref"],
                  "binarize_mutual": sm["mutual"], "binarize_rows2": sm["rows2"], "ratio": round(ratio, 3), "bar": BAR,
                  "met": bool(ratio <= BAR), "rows2_equals_twin": same,
                  "scores_that_differ": int((sc["ref"] != sc["mutual"]).sum().item()), "scores": 4 * P}
    return same


def calls_stage(a, bank, d_pairs, n_snf, out):
    import torch
    from acoss import _lib
    snf_pairs = d_pairs[:n_snf].contiguous()
    fns = {}
    for tag, m in (("rows", False), ("mutual", True)):
        fns["score_" + tag] = lambda m=m: _lib.earlyfusion(bank, d_pairs, KAPPA, K, MU, mutual=m)
        fns["locate_" + tag] = lambda m=m: _lib.earlyfusion_locate(bank, d_pairs, KAPPA, K, MU, mutual=m)
        fns["path_" + tag] = lambda m=m: _lib.earlyfusion_path(bank, d_pairs, KAPPA, K, MU, mutual=m)
        fns["snf_" + tag] = lambda m=m: _lib.earlyfusion_snf(bank, snf_pairs, KAPPA, K, NITERS, mu=MU, mutual=m)
    times, got = _alternate(a, fns)
    res = {"snf_pairs": int(snf_pairs.shape[0])}
    for call in ("score", "locate", "path", "snf"):
        r, m = _summary(times[call + "_rows"]), _summary(times[call + "_mutual"])
        res[call] = {"rows": r, "mutual": m, "ratio": round(m["median_s"] / r["median_s"], 3)}
    res["locate_scores_equal_score"] = bool(torch.equal(got["score_mutual"], got["locate_mutual"]["scores"]) and
                                            torch.equal(got["score_mutual"], got["path_mutual"]["scores"]))
    out["calls"] = res
    return res["locate_scores_equal_score"]


def _agree(sm, unit, same):
    """The tool's rule for a pair of summaries: the same bits, the medians within the larger spread."""
    md, lo, hi = "median_" + unit, "min_" + unit, "max_" + unit
    spread = max(v[hi] - v[lo] for v in sm.values())
    diff = sm["this"][md] - sm["parent"][md]
    return {"parent": sm["parent"], "this": sm["this"], "spread_" + unit: round(spread, 6),
            "median_difference_" + unit: round(diff, 6), "agree_within_spread": bool(abs(diff) <= spread),
            "same_bits": same}


def unchanged_stage(a, bank, d_pairs, n_snf, parent, out):
    """The existing entries, parent's library against this tree's, alternately on the same buffers."""
    import torch
    from acoss import _lib
    libs = {"parent": parent, "this": _lib.load_library()}
    P = int(d_pairs.shape[0])
    cap = max(1, _lib.sw_path_bound(int(bank["max_blocks"]), int(bank["max_blocks"])))
    snf_pairs = d_pairs[:n_snf].contiguous()
    lead, lead_snf = _lead(bank, d_pairs), _lead(bank, snf_pairs)
    new = lambda dt, *s: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    buf = {k: {"score": new(torch.float64, P, 4), "seg": new(torch.int32, P, 4, 4), "lens": new(torch.int32, P, 4),
               "cells": new(torch.int32, P, 4, cap, 2), "snf": new(torch.float64, n_snf)} for k in libs}
    outputs = {"acoss_earlyfusion": ("score",), "acoss_earlyfusion_locate": ("score", "seg"),
               "acoss_earlyfusion_path": ("score", "seg", "lens", "cells"), "acoss_earlyfusion_snf": ("snf",)}

    def call(k, entry, mode=None):
        """`entry` of library k; mode: the binarize argument of its twin ending in 2."""
        b, p, st = buf[k], _lib._ptr, _lib._stream()
        fn = getattr(libs[k], entry + ("" if mode is None else "2"))
        m = () if mode is None else (mode,)
        if entry == "acoss_earlyfusion":
            rc = fn(*lead, *m, p(b["score"]), st)
        elif entry == "acoss_earlyfusion_locate":
            rc = fn(*lead, *m, p(b["score"]), p(b["seg"]), st)
        elif entry == "acoss_earlyfusion_path":
            rc = fn(*lead, *m, p(b["score"]), p(b["seg"]), cap, p(b["lens"]), p(b["cells"]), st)
        else:  # acoss_earlyfusion_snf2 also takes binary_out before the stream
            rc = fn(*lead_snf, *m, NITERS, 1.0, p(b["snf"]), None, 0, None, *(() if mode is None else (None,)), st)
        if rc:
            raise RuntimeError("%s (%s, mode %r) returned %d" % (entry, k, mode, rc))

    def same(entry):
        return all(bool(torch.equal(buf["parent"][q].view(torch.uint8), buf["this"][q].view(torch.uint8)))
                   for q in outputs[entry])

    res, ok = {}, True
    for mode in (None, 1) if parent.has2 else (None,):
        for entry in TWINS:
            times, _ = _alternate(a, {k: (lambda k=k: call(k, entry, mode)) for k in libs})
            r = _agree({k: _summary(v) for k, v in times.items()}, "s", same(entry))
            res[entry + ("" if mode is None else "2_mutual")] = r
            ok = ok and r["same_bits"]
    for tag, mode in (("rows", 0), ("mutual", 1)) if parent.has2 else ():
        ms = _rounds(a, list(libs), lambda k: _phase_ms(libs[k], lambda: call(k, "acoss_earlyfusion", mode)))
        r = _agree({k: _summary(v, "ms") for k, v in ms.items()}, "ms", same("acoss_earlyfusion"))
        res["binarize_phase_earlyfusion2_" + tag] = r
        ok = ok and r["same_bits"]
    out["unchanged"] = res
    return ok


def density_stage(bank, pairs, n, out):
    """Ones in the four masks of the first n pairs, row rule against mutual."""
    import torch
    from acoss import _lib
    off, nb = bank["off"].cpu().numpy(), bank["nb_host"]
    ones = {"rows": np.zeros(4), "mutual": np.zeros(4)}
    cells = 0
    for i, j in pairs[:n]:
        a = {k: bank[k][off[i]:off[i] + nb[i]] for k in ("mfccs", "ssms", "chromas")}
        b = {k: bank[k][off[j]:off[j] + nb[j]] for k in ("mfccs", "ssms", "chromas")}
        oti = int(_lib.get_oti(bank["chroma_med"][i], bank["chroma_med"][j]).item())
        C = [_lib.csm(a["mfccs"], b["mfccs"], kind="euclidean"), _lib.csm(a["ssms"], b["ssms"], kind="euclidean"),
             _lib.csm(a["chromas"], b["chromas"], kind="cosine", oti_shift=oti)]
        wsum = torch.zeros_like(C[0])
        for D in C:
            wsum += _lib.wcsm(D, K, K, MU)
        four = C + [_lib.neg_exp(wsum)]
        for tag, m in (("rows", False), ("mutual", True)):
            ones[tag] += np.array([int(B.sum().item()) for B in _lib.binarize_mutual(four, KAPPA, mutual=m)])
        cells += int(nb[i]) * int(nb[j])
    out["density"] = {"pairs": int(min(n, len(pairs))),
                      **{tag: dict(zip(("mfccs", "ssms", "chromas", "early"), (v / cells).round(5).tolist()))
                         for tag, v in ones.items()}}


def stage(a, name, bank, pairs, n_snf, parent, res):
    import torch
    from acoss import _lib
    d_pairs = torch.as_tensor(pairs).cuda()
    order = _lib._ef_band_order(d_pairs, int(bank["nb"].shape[0]))
    if order is not None:
        d_pairs = d_pairs[order].contiguous()
    out = {"tracks": int(bank["nb"].shape[0]), "blocks_min": int(bank["nb_host"].min()),
           "blocks_max": int(bank["nb_host"].max()), "pairs": int(len(pairs))}
    ok = bar_stage(a, bank, d_pairs, parent, out)
    log("%s bar: %s" % (name, json.dumps(out["bar"])))
    ok = calls_stage(a, bank, d_pairs, min(n_snf, len(pairs)), out) and ok
    log("%s calls: %s" % (name, json.dumps(out["calls"])))
    if parent is not None:
        ok = unchanged_stage(a, bank, d_pairs, min(n_snf, len(pairs)), parent, out) and ok
        log("%s unchanged: %s" % (name, json.dumps(out["unchanged"])))
    density_stage(bank, pairs, a.density_pairs, out)
    log("%s density: %s" % (name, json.dumps(out["density"])))
    res[name] = out
    res["ok"] = res.get("ok", True) and ok


def map_stage(res):
    """MAP and MR1 of the five scores on bench_early_snf.py's corpus, row rule against mutual."""
    from acoss import synthetic
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    tracks, labels = synthetic.make_corpus("covers80", frames=2000, seed=11)
    out = {}
    with tempfile.TemporaryDirectory(prefix="efmutual_") as root:
        csv, fdir = synthetic.write_feature_dataset(root, tracks, labels, with_mfcc=True, mfcc_from_chroma=True)
        for tag, m in (("rows", False), ("mutual", True)):
            ef = EarlyFusion(csv, fdir, shortname="bench", cachedir=os.path.join(root, "cache"), early_snf=True, mutual=m)
            t0 = time.perf_counter()
            ef.all_pairwise(symmetric=True)
            r = {"songs": int(ef.N), "all_pairwise_s": round(time.perf_counter() - t0, 3)}
            for key in ("mfccs", "ssms", "chromas", "early", "early_snf"):
                st = ef.getEvalStatistics(key)
                r["MAP_" + key], r["MR1_" + key] = float(st[3]), float(st[0])
            ef.cleanup_memmap()
            out[tag] = r
    res["map_covers80_synthetic"] = out
    log("map: %s" % json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-blocks446", dest="blocks446", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--no-map", dest="map", action="store_false")
    ap.add_argument("--snf-pairs446", type=int, default=16)
    ap.add_argument("--snf-pairs-short", type=int, default=20000)
    ap.add_argument("--density-pairs", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutual", "bench_mutual.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mutual.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    parent = _bind(a.parent_lib) if a.parent_lib else None
    res = {"bench": "mutual", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "parent_lib": bool(a.parent_lib), "kappa": KAPPA, "K": K}
    rng = np.random.Generator(np.random.PCG64(a.seed))
    if a.blocks446:
        NT = 80
        pairs = np.array([(i, j) for i in range(NT) for j in range(i + 1, NT)], np.int32)
        stage(a, "blocks446", make_bank(rng, np.full(NT, 446)), pairs, a.snf_pairs446, parent, res)
    if a.short:
        n = a.short_tracks
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "short", make_bank(rng, rng.integers(14, 48, n)), pairs, a.snf_pairs_short, parent, res)
    if a.map:
        map_stage(res)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
