"""bench.py's plain run on the GPU: the headline line alone, --steps honoured, and --dump-outputs.

One short run (200-frame tracks, 2 timed steps) in a child process, as the benchmark is started:
* the JSON line carries the headline fields and none of the legs that --full adds;
* DIR/scores.npy is the float32 (tracks x tracks) matrix the last timed step returned, and equals,
  bit for bit, the same path run here on the corpus the same arguments generate (so the inputs
  depend on the arguments only, and two builds can be compared score for score).
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
FRAMES, SEED = 200, 77


def test_plain_run_headline_and_dump(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", str(FRAMES),
                        "--seed", str(SEED), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["warmup"] == 1 and res["full"] is False
    assert res["unit"] == "song-pairs/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["ms_per_step"] > 0
    pairs = res["config"]["pairs_per_step"]
    assert pairs == 164 * 163 // 2
    # value and ms_per_step describe the same timed steps (both are rounded in the line)
    assert abs(res["value"] - pairs / (res["ms_per_step"] * 1e-3)) <= 1e-2 * res["value"]
    for leg in ("roofline", "cpu_baseline", "other_paths", "map_parity", "map", "multi_gpu"):
        assert leg not in res, leg
    assert sorted(os.listdir(out)) == ["scores.npy"]
    got = np.load(out / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (164, 164)

    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from acoss import distributed
    from acoss.engine import ChromaBank
    tracks, _ = bench.corpus_tracks(1, FRAMES, SEED, "hard")
    p = distributed.stripe_pairs(len(tracks), 0, len(tracks), symmetric=True)
    q = ChromaBank(tracks).crp_align(p, qmax=True)["qmax"]
    want = distributed.scatter_stripe(p, q, 0, len(tracks), len(tracks)).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.count_nonzero(np.triu(got, 1)) > 0 and not np.tril(got).any()
