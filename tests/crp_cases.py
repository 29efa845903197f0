"""Inputs for the CRP threshold-select tests: tracks with exact tie groups, and a census of the
branches the split selects (csrc/crp_split.hip, line_plan / line_groups) take on them.

A plain helper module (no tests, no fixtures); tests/test_crp_select_cases.py checks on the CPU
that the cases below reach every class of the census, tests/test_gpu_crp_params.py runs them.

Why run tracks: the selects find the order statistics at ranks lo / hi = floor / ceil((n-1) kappa)
in two steps, first the 16-bit prefix group holding rank lo, then the exact key inside it. Which
code finds the exact keys depends on the size g of that group, on whether hi falls into the next
group (size gh), and on whether either is larger than a wave (64). A natural track almost never
makes a group above 64 away from a silence; a piecewise-constant track does, at every size wanted.
"""
import functools

import numpy as np

import oracle
from acoss import synthetic

SEED = 3
KAPPAS = (0.0, 0.003, 0.03, 0.095, 0.2, 0.35, 0.5, 0.77, 0.999, 1.0)
# Tie-group sizes around the selects' 32-element runs, the 64-lane wave and the 128-bin histogram.
SIZES = (1, 2, 31, 32, 33, 60, 63, 64, 65, 66, 68, 127, 128, 129)
N_ALPHABET = 48
PAIRINGS = ("nat_x_runs", "runs_x_runs")
# frames (M, N) -> the line type of the longest line (m = 9, tau = 1: M - 9 and N - 9 codes)
LINE_SHAPES = {(300, 500): "LineS<8>", (700, 1000): "LineS<16>", (1500, 2040): "Line<32>", (2200, 3000): "Line2"}
# lines of at most 512 codes (LineS<8>) inside a long-line / a Line2 launch
MIXED_SHAPES = ((300, 1500), (400, 2600))
CLASSES = ("int_q/g<=64", "int_q/g>64", "same/g<=64", "same/g>64", "straddle/both<=64", "straddle/sum>64",
           "straddle/g>64", "straddle/gh>64")


def kappas_for(M, N):
    """The kappa list the GPU test runs at frames (M, N); the census test sums over the same one.
    The whole sweep at every shape: the oracle's side of it takes under a second at 2200 x 3000."""
    return KAPPAS


def natural_track(rng, n):
    return synthetic.render(rng, synthetic.base_sequence(rng, n))


def make_alphabet(rng, k=N_ALPHABET):
    """k frames of a synthetic.render track, one per chord dwell (so they differ)."""
    x = natural_track(rng, 64 * k)
    return np.ascontiguousarray(x[rng.choice(len(x), size=k, replace=False)])


def run_track(rng, n, sizes, alphabet):
    """(n, 12) piecewise-constant chroma: runs of g + 8 identical frames, g drawn from `sizes`, the
    frame from `alphabet`. At m = 9, tau = 1 a run gives exactly g bit-identical stacked frames, so
    every CRP line crossing it holds a tie group of g equal keys."""
    out = np.empty((n, 12), np.float32)
    i = 0
    while i < n:
        g = int(sizes[int(rng.integers(0, len(sizes)))])
        out[i:i + g + 8] = alphabet[int(rng.integers(0, len(alphabet)))]
        i += g + 8
    return out


def make_pair(M, N, pairing, seed=SEED):
    """(X, Y) of M and N frames: 'nat_x_runs' a synthetic.render query against a run track,
    'runs_x_runs' two run tracks over one alphabet."""
    rng = np.random.Generator(np.random.PCG64(seed))
    alphabet = make_alphabet(rng)
    if pairing == "nat_x_runs":
        X = natural_track(rng, M)
    elif pairing == "runs_x_runs":
        X = run_track(rng, M, SIZES, alphabet)
    else:
        raise ValueError(pairing)
    return X, run_track(rng, N, SIZES, alphabet)


@functools.lru_cache(maxsize=2)
def case(M, N, pairing, m=9, tau=1):
    """(X, Y, oti, D) of one case; D, the oracle's distances under the pair's OTI, is computed once
    and must not be written to."""
    X, Y = make_pair(M, N, pairing)
    k = oracle.oti(oracle.profile(X), oracle.profile(Y))
    D = oracle.crp_dist(X, Y, k, m, tau)
    D.setflags(write=False)
    return X, Y, k, D


def _line_classes(S, kappa):
    """Class index (into CLASSES) of every row of S, the ascending 16-bit prefixes of the lines."""
    n = S.shape[1]
    q = np.float32(n - 1) * np.float32(kappa)
    lo, hi = int(np.floor(q)), int(np.ceil(q))
    Pl = S[:, lo:lo + 1]
    less = (S < Pl).sum(1)
    le = (S <= Pl).sum(1)
    g = le - less
    rows = np.arange(len(S))
    Pn = S[rows, np.minimum(le, n - 1)][:, None]  # the next group's prefix (none: le == n, gh = 0)
    gh = np.where(le < n, (S == Pn).sum(1), 0)
    big = g > 64
    if lo == hi:
        return np.where(big, 1, 0)
    straddle = np.where(big, 6, np.where(gh > 64, 7, np.where(g + gh > 64, 5, 4)))
    return np.where(hi < le, np.where(big, 3, 2), straddle)


def sorted_prefixes(D):
    """(row lines, column lines) of D as ascending 16-bit prefixes of the float32 squared distance,
    the selects' first-level key (one ulp off the kernel's own d2 at most: a line changes class
    only at a bin edge, and the census only chooses inputs)."""
    P = ((D * D).view(np.uint32) >> 16).astype(np.uint16)
    return np.sort(P, axis=1), np.sort(np.ascontiguousarray(P.T), axis=1)


def census(D, kappa, prefixes=None):
    """{class: lines} over every row and column line of D, classified as line_plan / line_groups
    branch on them: q = float32(n-1) * float32(kappa), lo / hi = floor / ceil(q); Pl the prefix at
    rank lo, g its group's size, gh the next group's.
      int_q/*      lo == hi: one order statistic, no interpolation
      same/*       hi inside Pl's group
      straddle/*   hi in the next group: both<=64 (g + gh <= 64, the two groups in one wave pass),
                   sum>64 (each <= 64, together not), g>64, gh>64 (g <= 64 < gh)."""
    out = dict.fromkeys(CLASSES, 0)
    for S in (prefixes or sorted_prefixes(D)):
        for c, cnt in zip(*np.unique(_line_classes(S, kappa), return_counts=True)):
            out[CLASSES[int(c)]] += int(cnt)
    return out


def np_thresholds(D, kappa):
    """The percentile thresholds of every row and column of D in plain numpy: full sort, q / lo / hi
    in float32, s[lo] when q is an integer, else s[lo]*(hi-q) + s[hi]*(q-lo) with each product and
    the sum rounded to float32."""
    out = []
    for A in (D, D.T):
        s = np.sort(np.asarray(A, np.float32), axis=1)
        n = s.shape[1]
        q = np.float32(n - 1) * np.float32(kappa)
        lo, hi = np.floor(q), np.ceil(q)
        assert q.dtype == np.float32 and lo.dtype == np.float32
        if lo == hi:
            out.append(s[:, int(lo)].copy())
        else:
            a = s[:, int(lo)] * np.float32(hi - q)
            b = s[:, int(hi)] * np.float32(q - lo)
            assert a.dtype == np.float32 and b.dtype == np.float32
            out.append(a + b)
    return out[0], out[1]


def _assert_thresholds(got, want, D, kappa, axis):
    """Bit equality of one side's thresholds; a failure names the census classes of the lines
    that differ (the branch of line_groups to read)."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    if np.array_equal(g, w):
        return
    bad = np.flatnonzero(g != w)
    S = sorted_prefixes(D)[axis]
    names = sorted({CLASSES[int(c)] for c in _line_classes(S, kappa)[bad]})
    i = int(bad[0])
    raise AssertionError("kappa=%r: %d of %d %s thresholds differ, first at line %d: got %r (0x%08x), oracle %r "
                         "(0x%08x); census classes (as at m = 9, tau = 1) of the differing lines: %s"
                         % (kappa, len(bad), len(w), ("row", "column")[axis], i, float(got[i]), int(g[i]),
                            float(want[i]), int(w[i]), ", ".join(names)))


def check_pair_on_gpu(M, N, pairing, kappas, m=9, tau=1):
    """One case through the single-pair entry point (acoss_crp_pair) at every kappa of `kappas`:
    OTI and distances (once) equal to the oracle's, thresholds bit for bit equal to
    oracle.crp_thresholds of the oracle's distances, the mask equal to what the definition gives
    from them, and Qmax / dmax of the GPU's mask (acoss_align_crp) equal to oracle.align."""
    from acoss import _lib
    X, Y, k, D = case(M, N, pairing, m, tau)
    for n, kappa in enumerate(kappas):
        got = _lib.crp_pair(X, Y, _lib.crp_params(m=m, tau=tau, kappa=kappa), dist=(n == 0))
        assert int(got["oti"].item()) == k
        if n == 0:
            np.testing.assert_array_equal(got["dist"].cpu().numpy().view(np.uint32), D.view(np.uint32))
        tr, tc = oracle.crp_thresholds(D, kappa)
        _assert_thresholds(got["thr_row"].cpu().numpy(), tr, D, kappa, 0)
        _assert_thresholds(got["thr_col"].cpu().numpy(), tc, D, kappa, 1)
        C = ((D <= tr[:, None]) & (D <= tc[None, :])).astype(np.uint8)
        Cg = got["crp"].cpu().numpy()
        np.testing.assert_array_equal(Cg, C, err_msg="mask, kappa=%r" % kappa)
        for which in (0, 1):
            assert float(_lib.align_crp(got["crp"], which).item()) == oracle.align(Cg, which=which), (kappa, which)
