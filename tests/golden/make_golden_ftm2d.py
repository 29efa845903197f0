"""Generate tests/golden/ftm2d_golden.npz from the reference's own FTM2D code.

TEST INFRASTRUCTURE, run in the build container only (it reads the reference checkout, which does
not exist on the GPU box):

    python tests/golden/make_golden_ftm2d.py

The reference's acoss/algorithms/ftm2d.py is imported by file path with make_golden.py's stubbing
approach, plus what the file needs to run at all (none of it changes the captured arithmetic):

* `os` and a no-op `dd` are injected into the module: ftm2d.py uses both without importing them
  (:44,47,82);
* `librosa.util.sync` is the restatement of step 1 in tests/ftm2d_np.py (librosa is not installed;
  "librosa sync unpinned");
* `CoverAlgorithm.load_features` returns the generated feature dicts.

Captured for tracks A, B, C and E of tests/ftm2d_np.py (reference file:line):
  librosa.util.sync stand-in -> chrompwr          ftm2d.py:58-59, 100-117
  btchroma_to_fftmat                              ftm2d.py:120-138 (track A's one window)
  FTM2D.load_features (the shingles)              ftm2d.py:52-66
  FTM2D.similarity (the 4 x 4 score matrix)       ftm2d.py:85-97
Data only: inputs and recorded results.
"""
import os
import sys
import tempfile
import types

import numpy as np
import scipy.fftpack  # noqa: F401  (ftm2d.py calls scipy.fftpack.* after a bare `import scipy`)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ftm2d_np  # noqa: E402
from make_golden import REF, _load, _stub  # noqa: E402

TRACKS = "ABCE"


def load_reference():
    _stub("numba", jit=lambda *a, **k: (lambda f: f))
    _stub("deepdish", io=types.SimpleNamespace(load=None, save=None))
    _stub("progress")
    _stub("progress.bar", Bar=object)
    sync = lambda data, idx, aggregate=None: ftm2d_np.beat_sync(np.asarray(data).T, idx)
    util = _stub("librosa.util", sync=sync)
    lib = _stub("librosa", util=util, filters=types.SimpleNamespace())
    lib.__path__ = []
    pkg = _stub("acoss")
    pkg.__path__ = [REF]
    _stub("acoss.utils", create_dataset_filepaths=lambda *a, **k: [])
    alg = _stub("acoss.algorithms")
    alg.__path__ = [REF + "/algorithms"]
    tpl = _load("acoss.algorithms.algorithm_template", REF + "/algorithms/algorithm_template.py")
    ftm = _load("acoss.algorithms.ftm2d", REF + "/algorithms/ftm2d.py")
    ftm.os = os
    ftm.dd = types.SimpleNamespace(io=types.SimpleNamespace(load=None, save=lambda *a, **k: None))
    return tpl, ftm


def main():
    tpl, ftm = load_reference()
    tracks = ftm2d_np.make_tracks()
    feats = [{"hpcp": tracks[k][0], "madmom_features": {"onsets": tracks[k][1]}, "label": k} for k in TRACKS]
    tpl.CoverAlgorithm.load_features = lambda self, i: feats[i]
    out = {}
    with tempfile.TemporaryDirectory() as td:
        a = ftm.FTM2D.__new__(ftm.FTM2D)
        a.PWR, a.WIN, a.C, a.chroma_type, a.shingles = 1.96, 75, 5, "hpcp", {}
        a.name, a.shortname, a.cachedir = "FTM2D", "golden", td
        n = len(TRACKS)
        a.Ds = {"main": np.zeros((n, n), np.float32)}
        for i, k in enumerate(TRACKS):
            hpcp, onsets = tracks[k]
            out["%s_hpcp" % k], out["%s_onsets" % k] = hpcp, np.asarray(onsets, np.int64)
            sync = ftm2d_np.beat_sync(hpcp, onsets)
            out["%s_sync" % k] = sync
            out["%s_chrompwr" % k] = ftm.chrompwr(sync, a.PWR)
            out["%s_shingle" % k] = np.asarray(a.load_features(i))
        out["A_fftmat"] = ftm.btchroma_to_fftmat(out["A_chrompwr"], a.WIN)
        pairs = np.array([(i, j) for i in range(n) for j in range(n)])
        a.similarity(pairs)
        out["scores"] = np.array(a.Ds["main"])
        # the same scores before the float32 memmap rounds them
        a.Ds = {"main": np.zeros((n, n), np.float64)}
        a.similarity(pairs)
        out["scores_f64"] = np.array(a.Ds["main"])
    path = os.path.join(HERE, "ftm2d_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
