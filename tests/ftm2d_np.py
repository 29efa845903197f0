"""FTM2D restated in numpy (acoss/algorithms/ftm2d.py:52-66, 85-138) and the eight test tracks.

TEST INFRASTRUCTURE (oracle/ is frozen, so the restatement lives with the tests). Step 1, the
beat-synchronous median, is float32 exactly as np.median on the float32 chroma; everything after
it is float64. The DFT is written out as matrix products (W12 @ X, then Z[:, i:i+75] @ W75), not
through an FFT, so that its summation is the plain dot product the kernels are compared with.

librosa is not installed: `beat_sync` restates librosa.util.sync(hpcp.T, onsets, aggregate=np.median)
from its documentation (boundaries = unique(concat([0], clip(onsets, 0, n), [n])), one aggregate
per slice), unpinned against librosa itself, as np_oracle.median_downsample is.
"""
import numpy as np

WIN = 75
PWR = 1.96
C = 5
MAX_WINDOWS = 4096
SEED = 20251019


def boundaries(onsets, n):
    """Segment boundaries of librosa.util.sync: int64, unique (sorted), clipped to [0, n]."""
    o = np.clip(np.asarray(onsets, np.int64).ravel(), 0, n)
    return np.unique(np.concatenate([[0], o, [n]])).astype(np.int64)


def beat_sync(hpcp, onsets):
    """(n, 12) float32 chroma -> (12, nb) float32 per-segment medians (ftm2d.py:58)."""
    hpcp = np.asarray(hpcp, np.float32)
    b = boundaries(onsets, len(hpcp))
    out = np.empty((12, len(b) - 1), np.float32)
    for s in range(len(b) - 1):
        out[:, s] = np.median(hpcp[b[s]:b[s + 1]], axis=0)
    return out


def chrompwr(X, P=PWR):
    """ftm2d.py:100-117 in float64."""
    X = np.asarray(X, np.float64)
    n1 = np.sqrt(np.sum(X * X, axis=0))
    n1[n1 == 0] = 1
    Y = np.power(X / n1, P)
    n2 = np.sqrt(np.sum(Y * Y, axis=0))
    n2[n2 == 0] = 1
    return n1 * (Y / n2)


def dft_matrix(n):
    k = np.arange(n)
    ang = 2.0 * np.pi * ((k[:, None] * k[None, :]) % n) / n
    return np.cos(ang) - 1j * np.sin(ang)


def fft_mags(chroma, win=WIN):
    """(nw, 12 * win) fftshift-ed 2-D DFT magnitudes of every window, row-major (ftm2d.py:120-138)."""
    chroma = np.asarray(chroma, np.float64)
    nb = chroma.shape[1]
    nw = nb - win + 1
    if nw < 1:
        raise ValueError("%d beats, fewer than win=%d" % (nb, win))
    Z = dft_matrix(12) @ chroma                                    # (12, nb)
    Wt = dft_matrix(win)
    idx = np.arange(nw)[:, None] + np.arange(win)[None, :]
    out = np.empty((nw, 12 * win))
    for i0 in range(0, nw, 512):                                   # bounded temporaries for the longest track
        F = Z[:, idx[i0:i0 + 512]].transpose(1, 0, 2) @ Wt         # (w, 12, win)
        M = np.sqrt(F.real ** 2 + F.imag ** 2)
        out[i0:i0 + 512] = np.fft.fftshift(M, axes=(1, 2)).reshape(len(M), -1)
    return out


def shingle_from_chroma(chroma, win=WIN, Cc=C):
    """Steps 3-5: (12, nb) float64 -> (12 * win,) float64 (ftm2d.py:61-66)."""
    S = fft_mags(chroma, win)
    norm = np.sqrt(np.sum(S ** 2, 1))
    norm[norm == 0] = 1
    S = np.log(Cc * S / norm[:, None] + 1)
    med = np.median(S, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return med / np.sqrt(np.sum(med ** 2))


def shingle(hpcp, onsets, win=WIN, pwr=PWR, Cc=C):
    return shingle_from_chroma(chrompwr(beat_sync(hpcp, onsets), pwr), win, Cc)


def score(s1, s2):
    """ftm2d.py:93-96."""
    return np.exp(-np.sum((s1 - s2) ** 2))


def score_matrix(shingles):
    n = len(shingles)
    return np.array([[score(shingles[i], shingles[j]) for j in range(n)] for i in range(n)])


def _chroma(rng, n):
    x = np.abs(rng.standard_normal((n, 12)))
    return (x / x.max(1, keepdims=True)).astype(np.float32)


def make_tracks():
    """The eight tracks: {name: (hpcp (n, 12) float32, onsets int64)}, beat period 5 frames."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    grid = lambda n: np.arange(5, n, 5, dtype=np.int64)
    t = {}
    t["A"] = (_chroma(rng, 373), grid(373))                        # 75 beats, 1 window
    t["B"] = (_chroma(rng, 378), grid(378))                        # 76 beats, 2 windows
    c = _chroma(rng, 452)
    t["C"] = (c, grid(452) + rng.integers(-1, 2, size=len(grid(452))))  # 91 beats, 17 windows
    d = _chroma(rng, 600)
    d[150:330] = 0                                                 # zero-norm beat columns
    t["D"] = (d, grid(600))
    e = _chroma(rng, 1200)
    e[100:600] = 0                                                 # all-zero windows
    t["E"] = (e, grid(1200))                                       # 166 windows
    g9 = grid(900)
    t["F"] = (_chroma(rng, 900), g9[g9 >= 300])                    # a 300-frame first segment
    g5 = grid(500)
    t["G"] = (_chroma(rng, 500), np.concatenate([g5[:40], [g5[7], g5[21]], g5[40:], [499, 510]]).astype(np.int64))
    t["H"] = (_chroma(rng, 4170), np.arange(4170, dtype=np.int64))  # 4170 beats, 4096 windows
    return t


NAMES = "ABCDEFGH"
