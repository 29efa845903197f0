"""EarlyFusion's per-pair similarity network fusion (acoss_earlyfusion_snf) against the four
scores of acoss_earlyfusion on the same pair lists, and against today's only other route to the
same quantity. One JSON, also written to profiles/early_snf/bench_early_snf.json.

    python tools/bench_early_snf.py [--warmup 1] [--repeats 4] [--short-tracks 2000] [--short-k 100]
                                    [--no-blocks446] [--blocks446-tracks 80] [--no-short] [--no-map]
                                    [--baseline-pairs 50]
                                    [--parent-lib libacoss_hip.so] [--out path.json]

The two shapes of tools/bench_sw_path.py:
  blocks446: 80 tracks of 446 beat blocks, all 3,160 unordered pairs (n = 892: the workspace regime)
  short:     the Da-TACOS shape, --short-tracks tracks of 14..47 beat blocks, each against --short-k
             others drawn at random (n = 28..94: the LDS regime)
Per shape, in one process and alternating (every other round in the opposite order): --warmup
untimed rounds, then --repeats timed ones of
`_lib.earlyfusion_snf` (K = 10, niters = 5) and `_lib.earlyfusion` (the yardstick; with --parent-lib
also the parent commit's acoss_earlyfusion, bound by ctypes, in the same alternation), each call
closed by a device synchronisation. The JSON holds every time, the medians and min..max as the
spread, the per-pair time, and from one call with the library's phase events on (one stream) the
split csm / wcsm (means, affinities, P and S) / snf (the cross-diffusion steps) / binarize / sw, the
share of the fusion steps, and their float64 rate: 2 flops x 2 products x K x n^2 per step,
3 niters steps per pair, against the 78.6 TFLOP/s float64 vector peak of the MI355X's public
specification.
baseline: --baseline-pairs pairs through today's route, one pair at a time: get_ssm / get_csm /
get_csm_cosine of the blocks (HIP, one call each), getWCSMSSM (assembled on the host), the package's
doSimilarityFusionWs (acoss_snf_step per step), numpy binarisation and acoss_sw_constrained.
map: EarlyFusion(early_snf=True) on a synthetic covers80-shaped corpus (160 songs): the MAP of
early_snf beside early's. Recorded, not asserted: the corpus is synthetic.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoss-1_amd")]

import numpy as np  # noqa: E402

from tools.bench_sw_path import _summary, _timed, make_bank  # noqa: E402

KAPPA, K, MU, NITERS = 0.1, 10, 0.5, 5
FP64_VECTOR_PEAK = 78.6e12


def log(msg, t0=[time.perf_counter()]):
    print("[early_snf %.1fs] %s" % (time.perf_counter() - t0[0], msg), file=sys.stderr, flush=True)


def baseline(bank, pairs, n_pairs):
    """Today's route, one pair at a time; returns (seconds per pair, scores)."""
    import torch
    from acoss import _lib
    from acoss.algorithms.utils import cross_recurrence as cr
    from acoss.algorithms.utils import similarity_fusion as sf
    host = {k: bank[k].cpu().numpy() for k in ("mfccs", "ssms", "chromas", "chroma_med")}
    off, nb = bank["off"].cpu().numpy(), bank["nb_host"]
    blocks = lambda key, t: host[key][off[t]:off[t] + nb[t]]
    times, scores = [], []
    for a, b in pairs[:n_pairs]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Ws = []
        for key in ("mfccs", "ssms"):
            Ws.append(sf.getWCSMSSM(cr.get_ssm(blocks(key, a)), cr.get_ssm(blocks(key, b)),
                                    cr.get_csm(blocks(key, a), blocks(key, b)), K, MU))
        ca, cb = blocks("chromas", a), blocks("chromas", b)
        Ws.append(sf.getWCSMSSM(cr.get_csm_cosine(ca, ca), cr.get_csm_cosine(cb, cb),
                                cr.get_csm_blocked_oti(ca, cb, host["chroma_med"][a], host["chroma_med"][b],
                                                       cr.get_csm_cosine), K, MU))
        F = sf.doSimilarityFusionWs(Ws, K, NITERS, 1)
        M = int(nb[a])
        cross = F[:M, M:] + F[M:, :M].T
        binary = np.zeros(cross.shape, np.uint8)
        nn = cr.nneighbs(KAPPA, cross.shape[1])
        np.put_along_axis(binary, np.argsort(-cross, axis=1, kind="stable")[:, :nn], 1, 1)
        scores.append(float(_lib.sw_constrained([binary])[0]))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, np.array(scores)


def stage(a, name, bank, pairs, res):
    import torch
    from acoss import _lib
    d_pairs = torch.as_tensor(pairs).cuda()
    order = _lib._ef_band_order(d_pairs, int(bank["nb"].shape[0]))
    if order is not None:
        d_pairs = d_pairs[order].contiguous()
    fns = {"early_snf": lambda: _lib.earlyfusion_snf(bank, d_pairs, KAPPA, K, NITERS, mu=MU)["score"],
           "earlyfusion": lambda: _lib.earlyfusion(bank, d_pairs, KAPPA, K, MU)}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.acoss_earlyfusion.argtypes = _lib.SIGNATURES["acoss_earlyfusion"]
        parent.acoss_earlyfusion.restype = ctypes.c_int
        pout = torch.empty((len(pairs), 4), dtype=torch.float64, device="cuda")
        args = (_lib._ptr(bank["mfccs"]), _lib._ptr(bank["ssms"]), _lib._ptr(bank["chromas"]),
                _lib._ptr(bank["chroma_med"]), _lib._ptr(bank["off"]), _lib._ptr(bank["nb"]),
                int(bank["nb"].shape[0]), int(bank["max_blocks"]), 1000, 1225, 480, _lib._ptr(d_pairs), len(pairs),
                KAPPA, K, MU)
        this = _lib.load_library()
        tout = torch.empty_like(pout)

        def raw(lib, out):
            rc = lib.acoss_earlyfusion(*args, _lib._ptr(out), _lib._stream())
            if rc:
                raise RuntimeError("acoss_earlyfusion returned %d" % rc)
            return out

        fns = {"early_snf": fns["early_snf"], "earlyfusion": lambda: raw(this, tout),
               "earlyfusion_parent": lambda: raw(parent, pout)}
    times = {k: [] for k in fns}
    got = {}
    for it in range(a.warmup + a.repeats):
        # every other round in the opposite order, so no call always follows the same neighbour
        for k in (list(fns) if it % 2 == 0 else list(fns)[::-1]):
            s, got[k] = _timed(fns[k], torch)
            if it >= a.warmup:
                times[k].append(s)
    sm = {k: _summary(v) for k, v in times.items()}
    _lib.profile_enable(True)
    fns["early_snf"]()
    torch.cuda.synchronize()
    ph = {k: round(v[0], 3) for k, v in _lib.profile_read().items()}
    _lib.profile_enable(False)
    nbh = bank["nb_host"].astype(np.int64)
    n = nbh[pairs[:, 0]] + nbh[pairs[:, 1]]
    ok = _lib.ef_snf_pair_ok(nbh[pairs[:, 0]], nbh[pairs[:, 1]], K)
    flops = float(np.sum(n[ok] ** 2)) * 2 * 2 * K * 3 * NITERS
    tot = sum(ph.values())
    score = got["early_snf"].cpu().numpy()
    out = {"tracks": int(len(nbh)), "blocks_min": int(nbh.min()), "blocks_max": int(nbh.max()),
           "pairs": int(len(pairs)), "pairs_fused": int(ok.sum()), "n_mean": float(n.mean()),
           "times": sm, "us_per_pair": {k: round(v["median_s"] / len(pairs) * 1e6, 3) for k, v in sm.items()},
           "ratio_early_snf_over_earlyfusion": round(sm["early_snf"]["median_s"] / sm["earlyfusion"]["median_s"], 2),
           "phases_ms": ph, "snf_share_of_phases": round(ph.get("snf", 0.0) / tot, 3) if tot else None,
           "snf_fp64_flops": flops,
           "snf_fp64_tflops": round(flops / (ph["snf"] * 1e-3) / 1e12, 3) if ph.get("snf") else None,
           "snf_fp64_fraction_of_vector_peak": round(flops / (ph["snf"] * 1e-3) / FP64_VECTOR_PEAK, 4)
           if ph.get("snf") else None,
           "scores_nan": int(np.isnan(score).sum()), "scores_nonzero": int(np.count_nonzero(np.nan_to_num(score)))}
    if a.parent_lib:
        spread = max(sm[k]["max_s"] - sm[k]["min_s"] for k in ("earlyfusion", "earlyfusion_parent"))
        diff = sm["earlyfusion"]["median_s"] - sm["earlyfusion_parent"]["median_s"]
        out["earlyfusion_vs_parent"] = {"median_difference_s": round(diff, 6), "spread_s": round(spread, 6),
                                        "agree_within_spread": bool(abs(diff) <= spread),
                                        "same_scores": bool(torch.equal(got["earlyfusion"], got["earlyfusion_parent"]))}
    if a.baseline_pairs:
        sel = np.linspace(0, len(pairs) - 1, a.baseline_pairs).astype(np.int64)
        bt, bs = baseline(bank, pairs[sel], a.baseline_pairs)
        mine = _lib.earlyfusion_snf(bank, pairs[sel], KAPPA, K, NITERS, mu=MU)["score"].cpu().numpy()
        out["baseline_pair_at_a_time"] = {"pairs": int(len(bt)), "s_per_pair": _summary(bt[1:] or bt),
                                          "scores_equal_to_early_snf": int(np.sum(bs == mine)),
                                          "speedup_per_pair": round(float(np.median(bt[1:] or bt)) /
                                                                    (sm["early_snf"]["median_s"] / len(pairs)), 1)}
    res[name] = out
    log("%s: %s" % (name, json.dumps(out)))


def map_stage(res):
    from acoss import synthetic
    from acoss.algorithms.earlyfusion_traile import EarlyFusion
    tracks, labels = synthetic.make_corpus("covers80", frames=2000, seed=11)
    with tempfile.TemporaryDirectory(prefix="efsnf_") as root:
        csv, fdir = synthetic.write_feature_dataset(root, tracks, labels, with_mfcc=True, mfcc_from_chroma=True)
        ef = EarlyFusion(csv, fdir, shortname="bench", cachedir=os.path.join(root, "cache"), early_snf=True)
        t0 = time.perf_counter()
        ef.all_pairwise(symmetric=True)
        dt = time.perf_counter() - t0
        nb = ef.track_lengths()
        out = {"songs": int(ef.N), "blocks_min": int(nb.min()), "blocks_max": int(nb.max()),
               "all_pairwise_s": round(dt, 3), "nan_scores": int(np.isnan(np.array(ef.Ds["early_snf"])).sum())}
        for key in ("early", "early_snf"):
            st = ef.getEvalStatistics(key)
            out["MAP_" + key], out["MR1_" + key] = float(st[3]), float(st[0])
        ef.cleanup_memmap()
    res["map_covers80_synthetic"] = out
    log("map: %s" % json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--short-tracks", type=int, default=2000)
    ap.add_argument("--short-k", type=int, default=100)
    ap.add_argument("--no-blocks446", dest="blocks446", action="store_false")
    ap.add_argument("--blocks446-tracks", type=int, default=80)
    ap.add_argument("--no-short", dest="short", action="store_false")
    ap.add_argument("--no-map", dest="map", action="store_false")
    ap.add_argument("--baseline-pairs", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_snf", "bench_early_snf.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_early_snf.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    res = {"bench": "early_snf", "gpu": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats,
           "kappa": KAPPA, "K": K, "niters": NITERS, "parent_lib": bool(a.parent_lib)}
    rng = np.random.Generator(np.random.PCG64(a.seed))

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")

    if a.short:
        n = a.short_tracks
        k = min(a.short_k, n - 1)
        cand = (np.arange(n)[:, None] + 1 + np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)])) % n
        pairs = np.stack([np.repeat(np.arange(n), k), cand.ravel()], 1).astype(np.int32)
        stage(a, "short", make_bank(rng, rng.integers(14, 48, n)), pairs, res)
        flush()
    if a.blocks446:
        NT = a.blocks446_tracks
        pairs = np.array([(i, j) for i in range(NT) for j in range(i + 1, NT)], np.int32)
        stage(a, "blocks446", make_bank(rng, np.full(NT, 446)), pairs, res)
        flush()
    if a.map:
        map_stage(res)
    flush()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
