"""Locating and tracing EarlyFusion's four Smith-Waterman alignments (acoss_earlyfusion_locate /
acoss_earlyfusion_path) against scoring alone (acoss_earlyfusion) on the same pair lists. One JSON,
also written to profiles/sw_path/bench_sw_path.json.

    python tools/bench_sw_path.py [--warmup 2] [--repeats 5] [--short-tracks 2000] [--short-k 100]
                                  [--no-blocks446] [--no-short] [--out path.json]
                                  [--parent-lib libacoss_hip.so [--window-s 1.0] [--this-first]]

The two EarlyFusion shapes the README quotes:
  blocks446: bench.py's EarlyFusion leg, 80 tracks of 446 beat blocks, all 3,160 unordered pairs
             (matrices of 446 x 446: one per wave, 56 of 64 lanes busy; a direction plane of 50 kB
             per matrix).
  short:     the Da-TACOS shape, --short-tracks tracks of 14..47 beat blocks, each against --short-k
             others drawn at random (six lanes per matrix, ten matrices per wave).
Per shape, in one process and alternating: --warmup untimed rounds, then --repeats timed ones of
`_lib.earlyfusion` (the yardstick), `_lib.earlyfusion_locate` and `_lib.earlyfusion_path` (the library
call per chunk of pairs and the compaction of its padded output to the ragged form, on the device),
each call closed by a device synchronisation; the JSON holds every time, the medians, the ratios
locate / score, path / locate and path / score, and min..max as the spread. Then one call of each
with the library's phase events on (HIP events around the launches on the launch stream, one stream
while they are on): the scoring walk ("sw", which for the locate and path calls is their own last
stage), the tracing DP ("dp_trace"), the direction DP ("dp_dir") and the backtrack ("backtrack")
alone. The scores of the three routes must be equal bit for bit, the segments of locate and path
equal, and every path must start and end on its segment; the run fails otherwise.

--parent-lib: a libacoss_hip.so built from the parent commit (same C-ABI). After the stages above,
that library and this tree's are called alternately in one process on the same buffers:
`earlyfusion`, `earlyfusion_locate` and `earlyfusion_path` on each shape. Every call is warmed on
both libraries before any is timed (the parent's goes first in every round, this tree's with
--this-first); a timed window is as many calls in a row as fill --window-s seconds, --repeats windows per
library, then the same windows with the phase events on ("sw", "dp_trace", "dp_dir": the kernels
alone). Per call and per phase the JSON ("parent_ab") holds every time, both medians, both min..max
spreads and the verdict: this tree's median is no higher than the parent's plus the parent's own
spread. The outputs of the two libraries must be equal and every verdict must hold; the run fails
otherwise.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd")]

import numpy as np  # noqa: E402

KAPPA, K, MU = 0.1, 10, 0.5


def log(msg, t0=[time.perf_counter()]):
    print("[sw_path %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)),
            "all_s": [round(x, 6) for x in times]}


def make_bank(rng, nbs):
    """bench.py's synthetic block features for tracks of nbs blocks, on the device."""
    import torch
    nbs = np.asarray(nbs, np.int32)
    tot = int(nbs.sum())
    off = np.zeros(len(nbs), np.int64)
    off[1:] = np.cumsum(nbs[:-1])
    return {"mfccs": torch.as_tensor(rng.standard_normal((tot, 1000), dtype=np.float32)).cuda(),
            "ssms": torch.as_tensor(np.abs(rng.standard_normal((tot, 1225), dtype=np.float32))).cuda(),
            "chromas": torch.as_tensor(np.abs(rng.standard_normal((tot, 480), dtype=np.float32))).cuda(),
            "chroma_med": torch.as_tensor(np.abs(rng.standard_normal((len(nbs), 12), dtype=np.float32))).cuda(),
            "off": torch.as_tensor(off).cuda(), "nb": torch.as_tensor(nbs).cuda(), "nb_host": nbs,
            "max_blocks": int(nbs.max())}


def _same(x, y):
    import torch
    if isinstance(x, dict):
        return all(_same(x[k], y[k]) for k in x)
    return bool(torch.equal(x, y))


def ef_jobs(name, bank, d_pairs):
    """The three EarlyFusion calls on one shape as (shape, call, fn(lib) -> output, phase keys)."""
    from acoss import _lib

    def via(fn):
        def run(lib):
            _lib._lib = lib  # the wrappers call through the handle load_library() returns
            assert _lib.load_library() is lib
            return fn(bank, d_pairs, KAPPA, K, MU)
        return run
    return [(name, "earlyfusion", via(_lib.earlyfusion), ("sw",)),
            (name, "earlyfusion_locate", via(_lib.earlyfusion_locate), ("sw", "dp_trace")),
            (name, "earlyfusion_path", via(_lib.earlyfusion_path), ("sw", "dp_dir"))]


def _verdict(sm):
    p, t = sm["parent"], sm["this"]
    margin = p["max_s"] - p["min_s"]
    diff = t["median_s"] - p["median_s"]
    return {"parent": p, "this": t, "median_difference_s": round(diff, 7), "parent_spread_s": round(margin, 7),
            "this_within_parent_spread": bool(diff <= margin),
            "agree_within_larger_spread": bool(abs(diff) <= max(margin, t["max_s"] - t["min_s"]))}


def parent_ab(a, jobs, res):
    """The parent commit's library and this tree's, alternately, on every job. All jobs are warmed
    first (the workspaces then have their final sizes); a timed window is `inner` calls in a row,
    enough for --window-s seconds; then the same windows with the phase events on. Times are per call."""
    import torch
    from acoss import _lib
    this = _lib.load_library()
    libs = {"parent": _lib.load_library(os.path.abspath(a.parent_lib)), "this": this}
    if a.this_first:  # the order inside every round; a second run in the other order shows what the order does
        libs = {k: libs[k] for k in ("this", "parent")}
    out, same_all, accepted = {}, True, True
    try:
        inner = []
        for shape, call, fn, _ in jobs:
            got = {}
            for it in range(max(1, a.warmup)):
                t1 = 0.0
                for k, lib in libs.items():
                    s, got[k] = _timed(lambda: fn(lib), torch)
                    t1 = max(t1, s)
            inner.append(max(1, int(np.ceil(a.window_s / t1))))
            out["%s.%s" % (shape, call)] = {"calls_per_window": inner[-1], "same_output": _same(got["parent"], got["this"])}
            del got
        for (shape, call, fn, phases), n in zip(jobs, inner):
            rec = out["%s.%s" % (shape, call)]

            def window(lib):
                for _ in range(n):
                    fn(lib)
            times = {k: [] for k in libs}
            for _ in range(a.repeats):
                for k, lib in libs.items():
                    times[k].append(_timed(lambda: window(lib), torch)[0] / n)
            rec.update(_verdict({k: _summary(v) for k, v in times.items()}))
            ph = {key: {k: [] for k in libs} for key in phases}
            for _ in range(a.repeats):
                for k, lib in libs.items():
                    _lib._lib = lib
                    _lib.profile_enable(True)
                    window(lib)
                    torch.cuda.synchronize()
                    got = _lib.profile_read()
                    _lib.profile_enable(False)
                    for key in phases:
                        ph[key][k].append(got[key][0] * 1e-3 / n)
            rec["phases"] = {key: _verdict({k: _summary(v) for k, v in ph[key].items()}) for key in phases}
            same_all = same_all and rec["same_output"]
            accepted = (accepted and rec["this_within_parent_spread"]
                        and all(v["this_within_parent_spread"] for v in rec["phases"].values()))
            log("parent A/B %s.%s: %s" % (shape, call, json.dumps(rec)))
    finally:
        _lib._lib = this
    res["parent_ab"] = {"window_s": a.window_s, "order": list(libs), "rule": "this median <= parent median + parent's min..max spread",
                        "calls": out, "same_outputs": same_all, "accepted": accepted}
    res["ok"] = res.get("ok", True) and same_all and accepted


def stage(a, name, bank, pairs, res, jobs):
    import torch
    from acoss import _lib
    # on the device and in the order the library runs them in, so the three calls and the parent's
    # library time the same launches
    d_pairs = torch.as_tensor(pairs).cuda()
    order = _lib._ef_band_order(d_pairs, int(bank["nb"].shape[0]))
    if order is not None:
        d_pairs = d_pairs[order].contiguous()
    fns = {"score": lambda: _lib.earlyfusion(bank, d_pairs, KAPPA, K, MU),
           "locate": lambda: _lib.earlyfusion_locate(bank, d_pairs, KAPPA, K, MU),
           "path": lambda: _lib.earlyfusion_path(bank, d_pairs, KAPPA, K, MU)}
    times = {k: [] for k in fns}
    got = {}
    for it in range(a.warmup + a.repeats):
        for k, fn in fns.items():
            s, got[k] = _timed(fn, torch)
            if it >= a.warmup:
                times[k].append(s)
    scores_equal = bool(torch.equal(got["score"], got["locate"]["scores"]) and
                        torch.equal(got["score"], got["path"]["scores"]))
    seg_equal = bool(torch.equal(got["locate"]["seg"], got["path"]["seg"]))
    seg = got["path"]["seg"].cpu().numpy().reshape(-1, 4)
    poff = got["path"]["path_off"].cpu().numpy()
    cells = got["path"]["cells"].cpu().numpy()
    n = np.diff(poff)
    found = seg[:, 0] >= 0
    ends_ok = bool(((n > 0) == found).all())
    if found.any():
        ends_ok = ends_ok and bool((cells[poff[:-1][found]] == seg[found, :2]).all()
                                   and (cells[poff[1:][found] - 1] == seg[found, 2:]).all())
    ph_ms = {}
    for call, keys in (("score", ("sw",)), ("locate", ("sw", "dp_trace")), ("path", ("sw", "dp_dir", "backtrack"))):
        _lib.profile_enable(True)
        fns[call]()
        torch.cuda.synchronize()
        ph = _lib.profile_read()
        _lib.profile_enable(False)
        for key in keys:
            ph_ms["%s_%s_ms" % (call, key)] = round(ph[key][0], 4)
    sm = {k: _summary(v) for k, v in times.items()}
    out = {"tracks": int(bank["nb"].shape[0]), "blocks_min": int(bank["nb_host"].min()),
           "blocks_max": int(bank["nb_host"].max()), "pairs": int(len(pairs)), "score": sm["score"],
           "locate": sm["locate"], "path": sm["path"],
           "ratio_locate_over_score": round(sm["locate"]["median_s"] / sm["score"]["median_s"], 3),
           "ratio_path_over_locate": round(sm["path"]["median_s"] / sm["locate"]["median_s"], 3),
           "ratio_path_over_score": round(sm["path"]["median_s"] / sm["score"]["median_s"], 3),
           "scores_equal": scores_equal, "seg_equal": seg_equal, "path_ends_on_seg": ends_ok,
           "matrices_with_path": int(found.sum()), "path_cells_total": int(poff[-1]),
           "path_cells_median": float(np.median(n[found])) if found.any() else None,
           "path_cells_max": int(n.max()) if len(n) else 0}
    out.update(ph_ms)
    out["ratio_dp_trace_over_sw"] = round(ph_ms["locate_dp_trace_ms"] / ph_ms["score_sw_ms"], 2)
    out["ratio_dp_dir_over_dp_trace"] = round(ph_ms["path_dp_dir_ms"] / ph_ms["locate_dp_trace_ms"], 2)
    ok = scores_equal and seg_equal and ends_ok
    jobs += ef_jobs(name, bank, d_pairs)
    res[name] = out
    res["ok"] = res.get("ok", True) and ok
    log("%s: %s" % (name, json.dumps(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-blocks446", dest="blocks446", action="store_false")
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--this-first", action="store_true")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sw_path", "bench_sw_path.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sw_path.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    res = {"bench": "sw_path", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "parent_lib": bool(a.parent_lib)}
    rng = np.random.Generator(np.random.PCG64(a.seed))
    jobs = []
    if a.blocks446:
        NT = 80
        pairs = np.array([(i, j) for i in range(NT) for j in range(i + 1, NT)], np.int32)
        stage(a, "blocks446", make_bank(rng, np.full(NT, 446)), pairs, res, jobs)
    if a.short:
        n = a.short_tracks
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "short", make_bank(rng, rng.integers(14, 48, n)), pairs, res, jobs)
    if a.parent_lib:
        parent_ab(a, jobs, res)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res.get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
