"""EarlyFusion's CSM kernels at narrow feature widths (GPU).

Every other EarlyFusion test has rows of 1000 / 1225 / 480 floats, dozens of whole k-blocks per
row. The wave-tile kernels (csrc/ef_csm.hip: ef_wave_dot) read a row in blocks of 16 floats
(euclid; the SSM rows padded to a multiple of 4) or 24 (cosine), three blocks in flight, then a
zero-filled partial block. The widths here take its other paths:

  (4, 5, 24)     no whole euclid block, only the tail (the SSM rows padded 5 -> 8); one whole
                 cosine block, no tail
  (20, 33, 48)   one and two whole blocks, fewer than the ring is deep: its look-ahead loads are
                 clamped; tails of 4 floats (33 -> 36)
  (36, 8, 72)    two whole blocks and a tail; a tail alone; exactly three cosine blocks
  (52, 17, 24)   three whole blocks (one round of the ring) and a tail; 17 -> 20: one block and a tail
  (48, 96, 72)   whole blocks only: 3, 6 and 3, multiples of the ring's depth
  (6, 7, 36)     d_mfcc % 4 != 0 and d_chroma % 24 != 0: the LDS kernel for both, the wave tiles
                 for the padded SSM rows, in the same call

on three banks, one per choice of kernels (ef_launch_csms): every track within 64 blocks (32 x 32
tiles: packed euclid columns, two pairs per wave for the cosine CSM), within 128 (packed euclid
columns, 64 x 64 cosine tiles) and beyond (64 x 64 tiles of one pair). All four scores of every
ordered pair must equal the canonical CPU oracle's (oracle/ef_oracle.cpp), which takes any width.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

WIDTHS = [(4, 5, 24), (20, 33, 48), (36, 8, 72), (52, 17, 24), (48, 96, 72), (6, 7, 36)]
BANKS = [[14, 31, 33, 47, 64], [30, 65, 70, 96, 128], [64, 65, 129, 140]]
KAPPA, K = 0.1, 10


@pytest.mark.parametrize("nbs", BANKS, ids=lambda b: "blocks%d-%d" % (min(b), max(b)))
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "d%d-%d-%d" % w)
def test_earlyfusion_equals_oracle_at_narrow_widths(widths, nbs):
    import torch
    from acoss import _lib
    d_mfcc, d_ssm, d_chroma = widths
    rng = np.random.default_rng(31)
    T, R = len(nbs), sum(nbs)
    host = {"mfccs": rng.standard_normal((R, d_mfcc), dtype=np.float32),
            "ssms": np.abs(rng.standard_normal((R, d_ssm), dtype=np.float32)),
            "chromas": np.abs(rng.standard_normal((R, d_chroma), dtype=np.float32)),
            "chroma_med": np.abs(rng.standard_normal((T, 12), dtype=np.float32)),
            "nb": np.array(nbs, np.int32), "off": np.concatenate([[0], np.cumsum(nbs[:-1])]).astype(np.int64)}
    bank = {k: torch.as_tensor(host[k]).cuda() for k in ("mfccs", "ssms", "chromas", "chroma_med", "off", "nb")}
    bank["max_blocks"] = max(nbs)
    pairs = np.array([(i, j) for i in range(T) for j in range(T) if i != j], np.int32)
    got = _lib.earlyfusion(bank, pairs, KAPPA, K).cpu().numpy()
    ref = oracle.ef_batch(host, pairs, KAPPA, K=K)
    assert np.isfinite(ref).all() and len(np.unique(ref, axis=0)) > len(pairs) // 2  # no vacuous equality
    np.testing.assert_array_equal(got, ref)
