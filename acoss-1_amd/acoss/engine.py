"""Device-resident song banks and the batched pair scorers built on the C-ABI.

A bank packs every track of a corpus once into HBM (one contiguous (sum n, 12) float32
block + offsets/lengths, SURVEY.md §8f row 3 layout); the scorers then take (P, 2) pair
index lists and return one score per pair, computed by the HIP kernels in a single
stream-ordered call. This replaces the reference's per-pair Python loop
(CoverAlgorithm.similarity, acoss/algorithms/algorithm_template.py:121-140 and the plugin
overrides) with one batched call per pair chunk.
"""
import numpy as np

from . import _lib
from ._lib import stacked_len  # also this module's public name for it
from .synthetic import pack


def segment_frames(seg, m, tau, factor, n_query, n_reference):
    """Cells of located alignments -> half-open ranges of original feature frames (pure numpy).
    seg: (P, 4) (i0, j0, i1, j1) in stacked-frame rows (query) and columns (reference); n_query,
    n_reference: (P,) (or scalar) frame counts of the tracks before downsampling by `factor`.
    Stacked row i covers the downsampled frames i*tau .. (i + m - 1)*tau and downsampled frame d
    the original frames [d*factor, min((d + 1)*factor, n)), so the query range is
    [i0*tau*factor, min(((i1 + m - 1)*tau + 1)*factor, n_query)) and the reference range the same
    in j. Returns (query_frames (P, 2), reference_frames (P, 2)) int64; an empty segment
    (-1, -1, -1, -1) maps to (-1, -1) in both."""
    seg = np.asarray(seg, np.int64).reshape(-1, 4)
    P = len(seg)
    out = []
    for a, b, n in ((seg[:, 0], seg[:, 2], n_query), (seg[:, 1], seg[:, 3], n_reference)):
        n = np.broadcast_to(np.asarray(n, np.int64), (P,))
        lo = a * tau * factor
        hi = np.minimum(((b + m - 1) * tau + 1) * factor, n)
        r = np.stack([lo, hi], 1)
        r[seg[:, 0] < 0] = -1
        out.append(r)
    return out[0], out[1]


def path_frames(cells, tau, factor):
    """Cells of alignment paths -> original feature frames (pure numpy). cells: (n, 2) (i, j) in
    stacked-frame rows (query) and columns (reference). Stacked row i starts at downsampled frame
    i*tau, which starts at original frame i*tau*factor: the convention of segment_frames' lower
    ends. Returns (n, 2) int64 (query frame, reference frame)."""
    return np.asarray(cells, np.int64).reshape(-1, 2) * (int(tau) * int(factor))


def subsequence_frames(idx, sslen, win, skip, n_frames):
    """SiMPle subsequence indices -> half-open ranges of original feature frames (pure numpy).
    idx: (n,) subsequence indices (rows of a matrix profile, or its index entries); n_frames: (n,)
    (or scalar) frame counts of the tracks before the window means. SiMPle column c is the mean of
    the original frames [c*skip, min(c*skip + win, n)) (simple_silva.py:38-41) and subsequence i
    the columns i .. i + sslen - 1, so its range is [i*skip, min((i + sslen - 1)*skip + win, n)).
    Returns (n, 2) int64; an index of -1 (no nearest subsequence) maps to (-1, -1), as an empty
    segment does in segment_frames."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    n = np.broadcast_to(np.asarray(n_frames, np.int64), idx.shape)
    r = np.stack([idx * skip, np.minimum((idx + sslen - 1) * skip + win, n)], 1)
    r[idx < 0] = -1
    return r


def block_frames(blocks, onsets, blocksize, n_frames):
    """EarlyFusion beat blocks -> half-open ranges of chroma frames (pure numpy). blocks: (n, 2)
    inclusive block ranges [b0, b1] of one track (or (n,) single blocks); onsets: the track's beat
    onsets (frame indices), blocksize: beats per block, n_frames: its chroma frame count. Block b
    covers the frames [o[b], min(o[b + blocksize], n_frames)) (acoss_ef_block_features), so a range
    of blocks covers from the first block's start to the last block's end. Returns (n, 2) int64;
    a block of -1 (no alignment) maps to (-1, -1), as an empty segment does in segment_frames."""
    b = np.asarray(blocks, np.int64)
    b = np.stack([b, b], 1) if b.ndim == 1 else b.reshape(-1, 2)
    o = np.asarray(onsets, np.int64).reshape(-1)
    ok = (b[:, 0] >= 0) & (b[:, 1] >= 0)
    r = np.full((len(b), 2), -1, np.int64)
    if ok.any():
        if int(b[ok].max()) + blocksize >= len(o):
            raise ValueError("block %d of a track with %d onsets at %d beats per block"
                             % (int(b[ok].max()), len(o), blocksize))
        r[ok, 0] = o[b[ok, 0]]
        r[ok, 1] = np.minimum(o[b[ok, 1] + blocksize], int(n_frames))
    return r


class ChromaBank:
    """12-bin chroma of a whole corpus resident on the current GPU."""

    def __init__(self, tracks=None, packed=None):
        """tracks: list of (n_i, 12) arrays, or packed=(feats (sum n, 12) f32 device tensor,
        frame offsets, lengths) already resident in HBM."""
        torch = _lib._torch()
        if packed is not None:
            feats, off, lens = packed
            self.lens = np.asarray(lens, np.int32)
            self.feats = feats
            self.off = torch.as_tensor(np.asarray(off, np.int64)).cuda()
        else:
            feats, off, lens = pack([np.asarray(t, np.float32) for t in tracks])
            self.lens = lens
            self.feats = torch.as_tensor(feats).cuda()
            self.off = torch.as_tensor(off).cuda()
        self.n_tracks = len(self.lens)
        self.max_len = int(self.lens.max()) if len(self.lens) else 0
        self.len = torch.as_tensor(self.lens).cuda()

    def _pairs(self, pairs, m, tau):
        """(P, 2) pairs as the scorers take them, None if there are none; raises for a pair that
        holds a track too short for the frame stacking."""
        torch = _lib._torch()
        # host pairs stay on the host until _lib checks them there and uploads them without a
        # stream synchronisation (chunk after chunk keeps the GPU busy)
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2) if not isinstance(pairs, torch.Tensor) else pairs
        if (pairs.size if isinstance(pairs, np.ndarray) else pairs.numel()) == 0:
            return None
        short = []
        if stacked_len(int(self.lens.min()), m, tau) <= 0:  # only then can a pair hold a short track
            hp = pairs if isinstance(pairs, np.ndarray) else pairs.cpu().numpy()
            short = [i for i in np.unique(hp) if stacked_len(self.lens[i], m, tau) <= 0]
        if short:
            raise ValueError("tracks %s are too short for frameStackSize=%d, frameStackStride=%d (essentia raises)"
                             % (short[:5], m, tau))
        return pairs

    def _crp(self, fn, empty, pairs, crp, **want):
        """The three scorers below: fn = the _lib function (want: its output switches); empty = (key,
        shape, dtype name) of what it returns, for an empty pair list; crp = crp_params' arguments, the
        last two of them (binarize, oti_rank)."""
        torch = _lib._torch()
        params = _lib.crp_params(*crp)  # also the check of binarize and oti_rank
        pairs = self._pairs(pairs, crp[0], crp[1])
        if pairs is None:
            return {k: torch.zeros(shape, dtype=getattr(torch, dt), device="cuda") for k, shape, dt in empty}
        return fn(self.feats, self.off, self.len, self.max_len, pairs, params, **want)

    @staticmethod
    def _located(align):
        """(key, shape, dtype name) of what crp_locate returns, for an empty pair list."""
        return ((_lib.score_key(align), 0, "float32"), ("seg", (0, 4), "int32"), ("oti", 0, "int32"))

    def oti_ranked(self, pairs, dots=True):
        """The ranked OTI of (query, reference) pairs: {"shifts" (P, 12), with dots "dots" (P, 12)}
        device tensors (see _lib.oti_ranked): the twelve transpositions of the reference by descending
        profile dot, shifts[:, 0] the OTI every CRP applies."""
        torch = _lib._torch()
        if (np.asarray(pairs).size if not isinstance(pairs, torch.Tensor) else pairs.numel()) == 0:
            out = {"shifts": torch.zeros((0, 12), dtype=torch.int32, device="cuda")}
            if dots:
                out["dots"] = torch.zeros((0, 12), dtype=torch.float32, device="cuda")
            return out
        return _lib.oti_ranked(self.feats, self.off, self.len, pairs, dots=dots)

    def crp_align(self, pairs, m=9, tau=1, kappa=0.095, oti=True, gamma_open=0.5, gamma_ext=0.5, qmax=True,
                  dmax=False, want_oti=False, binarize="percentile", oti_rank=1, n_oti=1):
        """Serra09 (Qmax) / Chen (dmax) scores for (query, reference) pairs. binarize='oti': on the
        OTI-binary CRP of Serra08 at oti_rank (include/acoss_hip.h, acoss_crp_params2; kappa is then
        not read) in place of the percentile CRP; the same two arguments on the three methods below.
        n_oti > 1: the best score over the n_oti best transpositions of the ranked OTI
        (acoss_crp_params3), each aligner with its own winner: "oti" and "pick_q" come with Qmax,
        "oti_d" and "pick_d" with dmax (see _lib.crp_align)."""
        n_oti = _lib.check_n_oti(n_oti, oti)
        empty = [(k, 0, dt) for k, dt, on in (("qmax", "float32", qmax), ("dmax", "float32", dmax),
                                              ("oti", "int32", want_oti)) if on]
        if n_oti == 1:
            return self._crp(_lib.crp_align, empty, pairs,
                             (m, tau, kappa, oti, gamma_open, gamma_ext, binarize, oti_rank), qmax=qmax, dmax=dmax,
                             oti=want_oti)
        if qmax or want_oti:
            empty += [("oti", 0, "int32")] * (not want_oti) + [("pick_q", 0, "int32")]
        if dmax:
            empty += [("oti_d", 0, "int32"), ("pick_d", 0, "int32")]
        return self._crp(_lib.crp_align, empty, pairs, (m, tau, kappa, oti, gamma_open, gamma_ext, binarize, oti_rank),
                         qmax=qmax, dmax=dmax, oti=want_oti, n_oti=n_oti)

    @staticmethod
    def _picks(picks):
        """The picks= of the three methods below as _lib takes it: nothing when None."""
        return {} if picks is None else {"picks": picks}

    def crp_locate(self, pairs, m=9, tau=1, kappa=0.095, oti=True, gamma_open=0.5, gamma_ext=0.5, align=0,
                   binarize="percentile", oti_rank=1, picks=None):
        """Qmax of (query, reference) pairs and where it lies: {"qmax", "seg" (P, 4), "oti"} device
        tensors (see _lib.crp_locate); the scores are crp_align's. align=1: dmax and the chen17
        alignment, the score under "dmax". picks ((P,) int32; also on the two methods below): the rank
        of the ranked OTI each pair runs at, crp_align(n_oti=...)'s "pick_q" or "pick_d" for the
        alignment that won; "oti" is the shift applied."""
        return self._crp(_lib.crp_locate, self._located(align), pairs,
                         (m, tau, kappa, oti, gamma_open, gamma_ext, binarize, oti_rank), align=align,
                         **self._picks(picks))

    def crp_path(self, pairs, m=9, tau=1, kappa=0.095, oti=True, gamma_open=0.5, gamma_ext=0.5, align=0,
                 binarize="percentile", oti_rank=1, picks=None):
        """Qmax of (query, reference) pairs with the whole alignment path of each: {"qmax", "seg"
        (P, 4), "oti", "path_off" (P + 1,), "cells" (total, 2)} device tensors (see _lib.crp_path);
        scores and segments are crp_locate's. align=1: dmax and the chen17 path, the score under
        "dmax"; its steps also include (1, 0) and (0, 1) and i0 or j0 may be 1 (_lib.crp_path)."""
        empty = self._located(align) + (("path_off", 1, "int64"), ("cells", (0, 2), "int32"))
        return self._crp(_lib.crp_path, empty, pairs, (m, tau, kappa, oti, gamma_open, gamma_ext, binarize, oti_rank),
                         align=align, **self._picks(picks))

    def crp_rqa(self, pairs, m=9, tau=1, kappa=0.095, oti=True, lmin=2, smax=True, hist_cap=0, lines=True,
                binarize="percentile", oti_rank=1, picks=None):
        """Cross-recurrence quantification of (query, reference) pairs: {"counts" (P, 4), "lmax",
        "stats" (P, 4), "oti"} device tensors, with smax "smax", with hist_cap > 0 "hist"
        (P, hist_cap) (see _lib.crp_rqa); the CRP is crp_align's. lines=False: "oti" and "smax" only."""
        empty = [("oti", 0, "int32")]
        if lines:
            empty += [("counts", (0, 4), "int64"), ("lmax", 0, "int32"), ("stats", (0, 4), "float64")]
        if smax:
            empty.append(("smax", 0, "float32"))
        if hist_cap:
            empty.append(("hist", (0, int(hist_cap)), "int32"))
        return self._crp(_lib.crp_rqa, empty, pairs, (m, tau, kappa, oti, 0.5, 0.5, binarize, oti_rank), lmin=lmin,
                         smax=smax, hist_cap=hist_cap, lines=lines, **self._picks(picks))
